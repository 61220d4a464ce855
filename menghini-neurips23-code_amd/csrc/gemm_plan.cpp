// gemm_plan: the rule set that gives every f16 GEMM launch its kernel, grid and LDS (see gemm_plan.h).  Pure: the same inputs give the same plan on any
// machine; the only state of this file is the once-read GemmTuning behind gemm_tuning().
#include "gemm_plan.h"

#include <stdarg.h>

#include <initializer_list>
#include <stdlib.h>

#include "host_common.h"
#include "../../include/grip_amd_debug.h"

namespace {
constexpr int BN = 128, BK = 64, BK2 = 32;     // column panel, K slice, K slice of gemm_big_kernel (as gemm.hip)

int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
bool resid_epi(int epi) { return epi == EPI_BIAS_RESID || epi == EPI_BIAS_RESID_STATS; }

__attribute__((format(printf, 2, 3))) GemmPlan& refuse(GemmPlan& p, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.msg, sizeof p.msg, fmt, ap);
    va_end(ap);
    p.status = GRIP_ERR_ARG;
    return p;
}
#define PLAN_REQUIRE(cond, ...)                      \
    do {                                             \
        if (!(cond)) return refuse(p, __VA_ARGS__);  \
    } while (0)

int env_int(const char* name, int unset) {
    const char* v = getenv(name);
    return v ? atoi(v) : unset;
}

// Tile counts of one launch, computed once.  t<R> = tiles of R rows x 128 columns; the 256-column kernels count tm<R> tile rows x N / 256.
struct TileCounts {
    int64_t tn, t32, t64, t96, t128, tm192, tm256;
    TileCounts(int M, int N) : tn(N / BN), t32(cdiv(M, 32) * tn), t64(cdiv(M, 64) * tn), t96(cdiv(M, 96) * tn), t128(cdiv(M, 128) * tn), tm192(cdiv(M, 192)), tm256(cdiv(M, 256)) {}
};

// variant = 0: the tile shape by (measured relative rate) x (fill of the last wave of workgroups over 256 CUs).
int auto_variant(const GemmShape& g, const GemmTuning& t, int epi, bool can_big, const TileCounts& c) {
    if (c.t128 <= 256) {
        // fewer 128-row tiles than CUs: the launch is one workgroup per CU whatever the shape, and its time is k-steps x (bytes a CU stages per step),
        // which the 64-row tile cuts by a quarter (measured at M = 425 and 2 142: 6-25 % faster) ...
        // ... unless the 64-row tiles outnumber the CUs: one round of 128-row tiles on loader waves beats a round and a bit of 64-row ones on a long
        // walk (M = 3 408, N = 768, K = 3 072: 25.6 us against 31)
        return (t.r128 && g.ksplit <= 1 && c.t64 > 256 && g.K > 12 * BK) ? 1 : 4;
    }
    auto fill = [](int64_t tiles, int64_t slots) { return (double)tiles / (double)(((tiles + slots - 1) / slots) * slots); };
    double best = 0.85 * fill(c.t128, 512);                  // 128x128: two workgroups per CU
    int v = 1;
    const double s4 = 0.70 * fill(c.t64, 768);               // 64x128: three 48-KiB workgroups per CU
    if (s4 > best) { best = s4; v = 4; }
    if (!can_big) return v;
    const double s3 = 0.93 * fill(c.tm256 * c.tn, 512);      // 256x128: two per CU
    if (s3 > best) { best = s3; v = 3; }
    if (g.N % 256) return v;
    const int64_t t256 = c.tm256 * (g.N / 256), t192 = c.tm192 * (g.N / 256);
    const double s2 = 1.0 * fill(t256, 256);                 // 256x256: one per CU
    if (s2 > best) {
        // the 64-wide two-stage kernel (whole-line DMA) is 2-6 % faster than the 32-wide ring, and persistent (one workgroup per CU walking its
        // XCD's tiles) once every CU gets several tiles
        best = s2;
        v = t.big ? t.big : (t256 >= 512 ? 6 : 5);
    }
    // fewer tiles than CUs: one tile-time whatever the tile holds, so the 192-row form of the same kernel when it fills more CUs
    if (v == 5 && !t.big && c.tm192 * 192 <= g.m_pad && t192 <= 256 && epi != EPI_BIAS_RESID_STATS && fill(t192, 256) > best) v = 8;
    return v;
}

void set_launch(GemmPlan& p, GemmFamily family, int tile_m, int tile_n, int nst, int M, int N, int64_t grid_x, int64_t grid_y, unsigned block, int64_t lds) {
    p.family = family;
    p.tile_m = tile_m; p.tile_n = tile_n; p.nst = nst;
    p.tiles_m = (int)cdiv(M, tile_m); p.tiles_n = N / tile_n;
    p.grid_x = (unsigned)grid_x; p.grid_y = (unsigned)grid_y; p.block = block;
    p.lds = (int)lds;
}

// gemm_k64p_kernel: grid, tile walk and epilogue form
void plan_persistent(GemmPlan& p, const GemmShape& g, const GemmTuning& t) {
    const int64_t tiles_m = cdiv(g.M, 256), tiles_n = g.N / 256, tiles = tiles_m * tiles_n;
    // every XCD owns ceil or floor(tiles_m / 8) row panels: the grid has enough workgroups per XCD for the largest band
    const int64_t band = cdiv(tiles_m, 8) * tiles_n;
    int colgroup = 0;
    if (t.colgroup > 0 && tiles_m >= 64) {
        colgroup = (int)tiles_n;
        if (g.K <= 1024 && t.colgroup > 1)
            for (int c = t.colgroup; c >= 2; --c)
                if (tiles_n % c == 0 && tiles_n > c) { colgroup = c; break; }
    }
    const int64_t grid = colgroup ? (band * 8 >= g.n_cu ? g.n_cu : band * 8) : (tiles >= g.n_cu ? g.n_cu : ((tiles + 7) & ~(int64_t)7));
    set_launch(p, GEMM_K64P, 256, 256, 2, g.M, g.N, grid, 1, 512, 2 * 512 * BK * 2 + 8 * 4096);   // two stages + eight 4 KiB slabs = the whole 160 KiB
    p.colgroup = colgroup;
    // the three pool-encode epilogues have several forms (GemmTuning::emode); every other epilogue has form 0 only
    const int epi = p.epi;
    if (epi != EPI_LNFOLD_F16 && epi != EPI_LNFOLD_GELU_F16 && epi != EPI_BIAS_RESID_STATS) return;
    int emode = t.emode < 100 ? t.emode : (epi == EPI_LNFOLD_F16 ? t.emode / 100 : epi == EPI_LNFOLD_GELU_F16 ? (t.emode / 10) % 10 : t.emode % 10);
    if (epi == EPI_BIAS_RESID_STATS && (emode == 2 || emode == 4)) emode = 1;     // forms 2 and 4: LayerNorm-folded epilogues only
    if (emode == 4 && g.out2) emode = 1;      // the f16-slab form has no pre-activation copy (train-mode forwards)
    // single-block sub-step 1: the default form of each of the three only
    p.sd = t.sd && emode == (epi == EPI_LNFOLD_F16 ? 4 : epi == EPI_LNFOLD_GELU_F16 ? 2 : 1);
    p.emode = (emode == 0 || emode == 2 || emode == 4) ? emode : 1;
}
}  // namespace

const GemmTuning& gemm_tuning() {
    static const GemmTuning tuning = [] {
        GemmTuning t;
        t.r32 = env_int("GRIP_GEMM_R32", 1) != 0;
        t.r96 = env_int("GRIP_GEMM_R96", 2);
        t.r128 = env_int("GRIP_GEMM_R128", 1) != 0;
        t.wspec = env_int("GRIP_GEMM_WSPEC", 1) != 0;
        t.ring = env_int("GRIP_GEMM_RING", -1);
        t.big = env_int("GRIP_GEMM_BIG", 0);
        t.ksplit = env_int("GRIP_GEMM_KSPLIT", 0);
        t.coop_split = env_int("GRIP_COOP_SPLIT", 0);
        t.krot_m = env_int("GRIP_KROT_M", 0);
        t.colgroup = env_int("GRIP_GEMM_COLGROUP", 0);
        t.emode = env_int("GRIP_GEMM_EMODE", 421);
        t.sd = env_int("GRIP_GEMM_SD", 1) != 0;
        return t;
    }();
    return tuning;
}

// Cooperative split-K of an epilogue-carrying GEMM (GemmArgs::coop_scratch): worth it when a handful of 64-row tiles walk a long K each -- every tile
// stages its slices at the ~80 GB/s one CU pulls, whatever the other 200 CUs do.  The largest factor of {2, 4} that leaves every split >= 4 slices and
// the launch <= 256 workgroups.
int gemm_pick_coop_split(int M, int N, int K, const GemmTuning& t) {
    if (!t.wspec) return 1;                          // the form lives in the loader-wave kernel only
    const int64_t tiles = (cdiv(M, 64) * (N / BN) + 7) / 8 * 8;
    const int nk = K / BK;
    if (N % BN || K % BK || nk < 16 || tiles > 64) return 1;
    if (t.coop_split >= 1) return (nk % t.coop_split == 0 && nk / t.coop_split >= 3 && tiles * t.coop_split <= 256) ? t.coop_split : 1;
    int best = 1;
    for (int f : {2, 4})
        if (nk % f == 0 && nk / f >= 4 && tiles * f <= 256) best = f;
    return best;
}

// Split-K factor for an EPI_F32 product whose output has too few 64x128 tiles while K is long (the input-gradient GEMMs of the prompt steps: 136 tiles
// x 32 k-steps at M = 2 142, N = 512, K = 2 048): the SMALLEST factor that puts a workgroup on every CU (>= 256 workgroups) with >= 4 k-steps each, and
// at least 2 below 512 tiles.  Measured (tools/small_gemm_bench.py, SWEEP=1): text 15.5 us unsplit -> 11.7 at 2 = 11.7 at 4; image (324 tiles) 30.7 ->
// 24.7 at 2, 26.7 at 4 -- beyond one workgroup per CU more partials only add traffic for the consumer (ln_bwd_add reads every partial).
int gemm_pick_ksplit(int M, int N, int K, const GemmTuning& t) {
    const int64_t tiles = cdiv(M, 64) * (N / BN);
    const int nk = K / BK;
    if (t.ksplit >= 1) return nk % t.ksplit == 0 ? t.ksplit : 1;
    if (tiles >= 512) return 1;
    // More 64-row tiles than CUs (the image tower's input-gradient GEMMs: M = 3 408, N = 768 -> 324): 128-row tiles instead, split so that about two of
    // their 64-KiB workgroups share a CU -- the largest factor with <= 512 workgroups and >= 8 K tiles each.  VPT step in situ: 2 x 324 workgroups of
    // 64x128 23.2 us, 2 x 162 of 128x128 23.2 us, 3 x 162 of 128x128 20.0 us (the third partial costs ln_bwd_add 1.5 us: 10.0 -> 11.5).
    const int64_t t128 = cdiv(M, 128) * (N / BN);
    if (tiles > 256 && t128 <= 256) {
        int f128 = 1;
        for (int f : {2, 3, 4})
            if (nk % f == 0 && nk / f >= 8 && t128 * f <= 512) f128 = f;
        if (f128 > 1) return f128;
    }
    int best = 1;
    const int64_t t32 = cdiv(M, 32) * (N / BN);
    for (int f : {2, 3, 4, 6, 8}) {
        if (nk % f || nk / f < 3) continue;
        best = f;                                   // a few dozen tiles (the shared-prefix text rows): as many K slices as keep 3 k-steps each
        // workgroups of the launch: small launches run on 32-row tiles (gemm_plan), which doubles them -- so half the splits already reach (nearly)
        // every CU: M = 425, N = 512, K = 1 536 / 2 048: 4 splits x 56 tiles = 224 workgroups walking 6 - 8 slices instead of 8 x 28 walking 3 - 4,
        // and ln_bwd_add sums 4 partials instead of 8 (graphed CoOp step 1.075 -> 1.041 ms, profiles/r06_ksplit_ab.txt)
        const int64_t wgs = (tiles * f <= 128 && t32 * f <= 256) ? t32 * f : tiles * f;
        if (nk / f >= 4 && wgs >= 224) break;       // the smallest factor that reaches (7/8 of) every CU
    }
    return best;
}
int gemm_pick_ksplit(int M, int N, int K) { return gemm_pick_ksplit(M, N, K, gemm_tuning()); }
int gemm_pick_coop_split(int M, int N, int K) { return gemm_pick_coop_split(M, N, K, gemm_tuning()); }

namespace {
GemmPlan plan_rules(const GemmShape& g, const GemmTuning& t) {
    GemmPlan p{};
    p.epi = g.epi;
    // Row-dependent K rotation (GemmArgs::rot_rows = the caller's permission: train-mode launches only).  In a prompt step every GEMM reads weights
    // nobody has touched since the previous step; with all tile rows of a column panel walking K in lockstep, each of them waits out the memory
    // latency of every slice.  Staggered, a slice is fetched by one tile row and found in the L2 by the next.
    p.rot_rows = (g.rot_rows && !g.f32 && t.krot_m >= 0) ? (t.krot_m > 0 ? t.krot_m : (g.ksplit > 1 ? 1 : 2)) : 0;
    if (g.f32 == 2) { p.family = GEMM_SPLIT; p.variant = 7; return p; }
    if (g.f32) { p.family = GEMM_F32; p.variant = 0; return p; }

    const int epi = p.epi = (g.epi == EPI_BIAS_RESID && g.stat_part) ? (int)EPI_BIAS_RESID_STATS : g.epi;
    PLAN_REQUIRE(epi != EPI_BIAS_RESID_STATS || (g.stat_part && g.N % 64 == 0), "gemm: row statistics need stat_part and N %% 64 == 0");
    PLAN_REQUIRE(g.N % BN == 0 && g.K % BK == 0 && g.M > 0, "gemm: need N %% 128 == 0 and K %% 64 == 0 (M=%d N=%d K=%d)", g.M, g.N, g.K);
    PLAN_REQUIRE(g.ldc % 4 == 0, "gemm: ldc %% 4 != 0");
    PLAN_REQUIRE(((int64_t)g.M + 256) * g.ldc < ((int64_t)1 << 31), "gemm: output larger than 2^31 elements (M=%d ldc=%d)", g.M, g.ldc);

    const TileCounts c(g.M, g.N);
    const int ksplit = g.ksplit > 1 ? g.ksplit : 1;
    const int nk = g.K / BK / ksplit;                                      // K slices one workgroup walks
    const bool can_big = g.m_pad >= c.tm256 * 256 && g.K >= 4 * BK2;       // A must be padded to the 256-row tile
    const bool coop = ksplit > 1 && resid_epi(epi);
    const bool fits96 = cdiv(g.M, 96) * 96 <= g.m_pad;                     // the 96-row tiles' rows are allocated

    // ---- the tile shape ("variant": 1 = 128 rows, 4 = 64 rows, 2 / 3 / 5 / 6 / 8 = the 256- and 192-row kernels)
    int variant = g.variant ? g.variant : auto_variant(g, t, epi, can_big, c);
    if (coop) {     // cooperative split-K: loader-wave kernel on 64-row tiles only (GemmArgs::coop_scratch)
        PLAN_REQUIRE(g.coop && (g.K / BK) % ksplit == 0 && nk >= 3 && ((c.t64 + 7) / 8 * 8) * ksplit <= 256,
                     "gemm: cooperative split-K needs the scratch and counter buffers, (K/64) %% ksplit == 0 with >= 3 slices per split and <= 256 workgroups (M=%d N=%d K=%d ksplit=%d)",
                     g.M, g.N, g.K, ksplit);
        variant = 4;
    } else if (ksplit > 1) {
        PLAN_REQUIRE(epi == EPI_F32 && (g.K / BK) % ksplit == 0 && g.split_stride >= (int64_t)g.M * g.ldc,
                     "gemm: split-K needs EPI_F32, (K/64) %% ksplit == 0 and a partial stride >= M*ldc (K=%d ksplit=%d)", g.K, ksplit);
        // 128-row tiles where gemm_pick_ksplit sized the split for them (more 64-row tiles than CUs: about two 128-row workgroups per CU)
        if (g.variant == 0 && c.t64 > 256 && c.t128 * ksplit <= 512) variant = 1;
        else if (variant != 1) variant = 4;
    }
    if (variant == 5 && epi == EPI_BIAS_RESID_STATS) variant = 6;   // the one-tile-per-workgroup 64-wide kernel has no registers left for the statistics
    p.variant = variant;
    PLAN_REQUIRE(g.stat_parts <= 0 || g.stat_in, "gemm: stat_parts without stat_in");      // (every kernel but the persistent one reads the partial sums itself)
    if (g.stat_parts > 0 && variant == 6) {      // the persistent kernel (pool-sized M) takes finalised statistics only
        PLAN_REQUIRE(g.rowstat, "gemm: partial row sums on the persistent kernel need a rowstat buffer to finalise into");
        p.finalize_stats = true;
    }

    // ---- the 256-column kernels
    if (variant == 2) {
        PLAN_REQUIRE(can_big && g.N % 256 == 0, "gemm: 256x256 tile needs N %% 256 == 0 and A padded to 256 rows");
        set_launch(p, GEMM_BIG, 256, 256, 4, g.M, g.N, c.tm256 * (g.N / 256), 1, 512, 4 * (256 + 256) * BK2 * 2);
        return p;
    }
    if (variant == 3) {
        PLAN_REQUIRE(can_big, "gemm: 256x128 tile needs A padded to 256 rows");
        set_launch(p, GEMM_BIG, 256, 128, 3, g.M, g.N, c.tm256 * c.tn, 1, 256, 3 * (256 + 128) * BK2 * 2);
        return p;
    }
    if (variant == 5 || variant == 6) {
        PLAN_REQUIRE(can_big && g.N % 256 == 0 && g.K >= 2 * BK, "gemm: 256x256x64 tile needs N %% 256 == 0, K >= 128 and A padded to 256 rows");
        if (variant == 5) set_launch(p, GEMM_K64, 256, 256, 2, g.M, g.N, c.tm256 * (g.N / 256), 1, 512, 2 * (256 + 256) * BK * 2);
        else plan_persistent(p, g, t);
        return p;
    }
    if (variant == 8) {      // (7 is the f32 kernel in the debug hook)
        PLAN_REQUIRE(g.N % 256 == 0 && g.K >= 2 * BK && c.tm192 * 192 <= g.m_pad && epi != EPI_BIAS_RESID_STATS,
                     "gemm: 192x256x64 tile needs N %% 256 == 0, K >= 128, A padded to a multiple of 192 rows and an epilogue without row statistics");
        set_launch(p, GEMM_K64, 192, 256, 2, g.M, g.N, c.tm192 * (g.N / 256), 1, 512, 2 * (192 + 256) * BK * 2);
        return p;
    }

    // ---- the 128-column kernels: 64-row tiles for variant 4, 128-row tiles otherwise, one grid row per K split
    const int bmt = variant == 4 ? 64 : 128;
    const int64_t tiles = variant == 4 ? c.t64 : c.t128;
    auto ringw = [&](int rows, int nst, int64_t grid_x, int64_t grid_y) {
        set_launch(p, GEMM_RINGW, rows, BN, nst, g.M, g.N, grid_x, grid_y, 512, (int64_t)nst * (rows + BN) * BK * 2);
        return p;
    };
    if (coop) {
        PLAN_REQUIRE(t.wspec, "gemm: cooperative split-K needs the loader-wave kernels (GRIP_GEMM_WSPEC=0 is set)");
        return ringw(64, 4, (tiles + 7) / 8 * 8, ksplit);       // the splits of a tile on one XCD
    }
    const bool plain96 = t.wspec && ksplit == 1 && g.variant == 0 && fits96 && c.t96 <= 256;    // what every 96-row rule needs
    // 96-row loader-wave tiles (residual and plain f16 epilogues only) for SHORT walks whose 64-row tiles outnumber the CUs (M = 3 408, N = K = 768: 324
    // tiles of 64 rows at two workgroups per CU against 216 of 96 rows at one: VPT step 2.82 -> 2.78 ms, UPT 3.15 -> 3.12, profiles/r06_r96_ab.txt)
    if (plain96 && t.r96 >= 2 && variant == 4 && (resid_epi(epi) || epi == EPI_F16) && c.t64 > 256 && g.K / BK >= 4) return ringw(96, 5, c.t96, 1);
    // At most one workgroup per CU: the ring with the feed on its own waves
    if (t.wspec && tiles * ksplit <= 256) {
        // 32-row tiles where the 64-row ones fill at most half the chip -- the text tower's M = 425 GEMMs of a CoOp step: each tile stages 160 instead
        // of 192 rows per K slice through its CU's LDS-DMA path (profiles/r06_r32_ab.txt); split-K EPI_F32 partials too while all splits fit one per CU
        if (t.r32 && variant == 4 && nk >= 3 && (ksplit == 1 || epi == EPI_F32) && g.variant == 0 && tiles * ksplit <= 128 && c.t32 * ksplit <= 256)
            return ringw(32, 4, c.t32, ksplit);
        if (variant == 4 && nk >= 3) return ringw(64, 4, tiles, ksplit);
        // long walk, residual epilogue, fewer 128-row tiles than CUs: the 96-row form when it fills more of them (M = 3 408, N = 768: 216 tiles of 96
        // rows put 84 % of the chip on a walk that is a quarter shorter per tile than that of 162 tiles of 128)
        if (plain96 && t.r96 != 0 && variant == 1 && nk > 12 && resid_epi(epi) && c.t96 > tiles) return ringw(96, 5, c.t96, 1);
        // 128-row tiles: a 5-slot ring (the whole LDS) for long walks, a 3-slot one for short ones
        if (variant == 1 && nk > 12) return ringw(128, 5, tiles, ksplit);
        if (variant == 1 && nk >= 2) return ringw(128, 3, tiles, ksplit);
    }
    if (variant == 4) {
        // ring depth by workgroups per CU: <= 1 -> four stages (96 KiB), <= 2 -> three (72 KiB, two per CU); beyond that three co-resident two-stage
        // workgroups already keep three tiles in flight per CU
        const int64_t wgs = tiles * ksplit;
        int nst = t.ring >= 0 ? t.ring : (wgs <= 256 ? 4 : (wgs <= 512 ? 3 : 0));
        if (nst && nk < nst - 1) nst = 0;
        if (nst) {
            set_launch(p, GEMM_RING, 64, BN, nst == 3 ? 3 : 4, g.M, g.N, tiles, ksplit, 256, (int64_t)nst * (64 + BN) * BK * 2);
            return p;
        }
    }
    set_launch(p, GEMM_TWO_STAGE, bmt, BN, 2, g.M, g.N, tiles, ksplit, 256, 0);
    return p;
}
}  // namespace

GemmPlan gemm_plan(const GemmShape& g, const GemmTuning& t) {
    GemmPlan p = plan_rules(g, t);
    if (p.status == GRIP_OK && !g.f32) PLAN_REQUIRE(p.epi >= 0 && p.epi < EPI_COUNT, "gemm: unknown epilogue %d", p.epi);
    return p;
}

int gemm_plan_text(const GemmPlan& p, char* out, int out_len) {
    char name[64];
    switch (p.family) {
        case GEMM_TWO_STAGE: snprintf(name, sizeof name, "gemm_f16_kernel<%d, %d>", p.epi, p.tile_m / 32); break;
        case GEMM_RING: snprintf(name, sizeof name, "gemm_ring_kernel<%d, %d>", p.epi, p.nst); break;
        case GEMM_RINGW: snprintf(name, sizeof name, "gemm_ringw_kernel<%d, %d, %d>", p.epi, p.nst, p.tile_m / 32); break;
        case GEMM_BIG: snprintf(name, sizeof name, "gemm_big_kernel<%d, %d, %d, %d>", p.epi, p.tile_m, p.tile_n, p.nst); break;
        case GEMM_K64: snprintf(name, sizeof name, "gemm_k64_kernel<%d, 8, %d>", p.epi, p.tile_m / 32); break;
        case GEMM_K64P: snprintf(name, sizeof name, "gemm_k64p_kernel<%d, %d, %s>", p.epi, p.emode, p.sd ? "true" : "false"); break;
        case GEMM_F32: snprintf(name, sizeof name, "f32"); break;
        case GEMM_SPLIT: snprintf(name, sizeof name, "split"); break;
    }
    const int lds_static = p.family == GEMM_TWO_STAGE ? 2 * (p.tile_m + BN) * BK * 2 : 0;      // gemm_f16_kernel keeps its two stages in static LDS
    return snprintf(out, (size_t)out_len, "%s grid %ux%u block %u lds %d static_lds %d tiles %dx%d colgroup %d rot %d finalize %d variant %d", name, p.grid_x, p.grid_y,
                    p.block, p.lds, lds_static, p.tiles_m, p.tiles_n, p.colgroup, p.rot_rows, (int)p.finalize_stats, p.variant);
}

extern "C" int grip_debug_gemm_plan(int epi, int M, int N, int K, int ldc, int64_t m_pad, int variant, int ksplit, int f32, int rot_rows, int present,
                                    int stat_parts, int64_t split_stride, int n_cu, char* text, int text_len) {
    GemmShape g{};
    g.epi = epi; g.M = M; g.N = N; g.K = K; g.ldc = ldc; g.m_pad = m_pad; g.variant = variant; g.ksplit = ksplit; g.f32 = f32; g.rot_rows = rot_rows;
    g.stat_parts = stat_parts; g.split_stride = split_stride; g.n_cu = n_cu;
    g.stat_part = present & 1; g.stat_in = present & 2; g.rowstat = present & 4; g.out2 = present & 8; g.coop = present & 16;
    const GemmPlan p = gemm_plan(g, gemm_tuning());
    if (p.status) {
        grip_set_error("%s", p.msg);
        if (text && text_len > 0) snprintf(text, (size_t)text_len, "%s", p.msg);
        return p.status;
    }
    if (text && text_len > 0) gemm_plan_text(p, text, text_len);
    return GRIP_OK;
}
