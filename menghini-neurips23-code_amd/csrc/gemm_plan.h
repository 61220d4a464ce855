// Which kernel an f16 GEMM launch gets, as a pure host function: gemm_plan(shape, tuning) -> GemmPlan.  Plain C++ (no HIP): it builds with g++ for
// the host sanitizers and answers on a machine without a GPU (grip_debug_gemm_plan, tests/test_host_gemm_plan.py).  launch_gemm (gemm.hip) makes the
// plan and launches what it says; nothing else decides.
#pragma once
#include <stdint.h>

// GEMM: C[M,N] = epilogue(A[M,K] * W[N,K]^T).  A and W are f16, K-contiguous; accumulate f32.
enum GemmEpi {
    EPI_F32 = 0,             // out_f32 = acc
    EPI_BIAS_F16 = 1,        // out_f16 = acc + bias
    EPI_BIAS_GELU_F16 = 2,   // out_f16 = quickgelu(acc + bias); if out2 != null, out2_f16 = acc + bias (pre-activation)
    EPI_BIAS_RESID = 3,      // out_resid = resid + acc + bias   (residual stream, resid_t)
    EPI_F16 = 4,             // out_f16 = acc
    EPI_GELUGRAD_F16 = 5,    // out_f16 = acc * quickgelu'(aux_f16)       (backward of c_fc activation)
    EPI_F32_SCALE = 6,       // out_f32 = acc * scalar
    // LayerNorm folded into the GEMM that consumes it (A = the RAW residual stream, W = gamma-scaled weights W' = f16(gamma o W)):
    //   LN(x) W^T + b  =  rstd_r * (x W'^T - mean_r * colsum(W')) + (W beta + b)
    // rowstat[r] = (mean_r, rstd_r), colsum[n] = sum_k W'[n][k], bias[n] = (W beta + b)[n]
    EPI_LNFOLD_F16 = 7,      // out_f16 = rstd * (acc - mean * colsum) + bias
    EPI_LNFOLD_GELU_F16 = 8, // out_f16 = quickgelu(that); if out2 != null, out2_f16 = that (pre-activation)
    EPI_BIAS_RESID_STATS = 9,// EPI_BIAS_RESID + the row statistics (GemmArgs.stat_part); chosen by the launcher, never passed in by callers
    EPI_COUNT = 10
};

enum GemmFamily {
    GEMM_TWO_STAGE = 0,   // gemm_f16_kernel<EPI, WMF>: 64- or 128-row tile, two LDS stages (static LDS)
    GEMM_RING,            // gemm_ring_kernel<EPI, NST>: 64-row tile, 3- or 4-slot ring
    GEMM_RINGW,           // gemm_ringw_kernel<EPI, NST, WMF>: ring fed by loader waves, 32 / 64 / 96 / 128-row tiles
    GEMM_BIG,             // gemm_big_kernel<EPI, BMT, BNT, NSTAGE>: 256-row tiles on a ring of 32-wide K tiles
    GEMM_K64,             // gemm_k64_kernel<EPI, 8, RF>: 256x256x64 (RF = 8) or 192x256x64 (RF = 6), one tile per workgroup
    GEMM_K64P,            // gemm_k64p_kernel<EPI, EMODE, SD>: 256x256x64, persistent
    GEMM_F32,             // exact mode (gemm_f32.hip keeps its own launcher)
    GEMM_SPLIT            // split-f16 tier (gemm_split.hip keeps its own launcher)
};

// Every run-time knob of the decision (developer A/B switches).  gemm_tuning() fills one from the environment, once per process.
struct GemmTuning {
    // GRIP_GEMM_R32=0: no 32-row loader-wave tiles.  Default on: the text tower's M = 425 GEMMs of a CoOp step run 56 - 224 tiles of 32 rows instead of
    // 28 - 112 of 64, graphed CoOp step 1.11 - 1.16 -> 1.076 ms (profiles/r06_r32_ab.txt)
    bool r32 = true;
    // GRIP_GEMM_R96: 0 = no 96-row tiles, 1 = long K walks only, 2 (default) = short walks too.  Long: M = 3 408, N = 768, K = 3 072: 216 tiles of 96 rows
    // instead of 162 of 128.  Short (N = K = 768): VPT step 2.82 -> 2.78 ms, UPT 3.15 -> 3.12 (profiles/r06_r96_ab.txt)
    int r96 = 2;
    // GRIP_GEMM_R128=0: keep 64-row tiles where they outnumber the CUs while the 128-row ones do not.  Default on: M = 3 408, N = 768, K = 3 072 one round of
    // 128-row tiles on loader waves 25.6 us against 31
    bool r128 = true;
    // GRIP_GEMM_WSPEC=0: no loader-wave kernels (gemm_ringw_kernel), and with them no cooperative split-K
    bool wspec = true;
    // GRIP_GEMM_RING=0 / 3 / 4: ring depth of gemm_ring_kernel (0 = the two-stage kernel); -1 = by workgroups per CU
    int ring = -1;
    // GRIP_GEMM_BIG=2 / 5 / 6: which 256x256 kernel the automatic choice takes (0 = by K and tile count)
    int big = 0;
    // GRIP_GEMM_KSPLIT=n: split-K factor of the EPI_F32 input-gradient GEMMs (1 = off, 0 = gemm_pick_ksplit's rule)
    int ksplit = 0;
    // GRIP_COOP_SPLIT=n: factor of the cooperative split-K (1 = off, 0 = gemm_pick_coop_split's rule)
    int coop_split = 0;
    // GRIP_KROT_M: stride of the row-dependent K rotation of train-mode launches (-1 = off, 0 = the default 2, or 1 under split-K).  VPT step in situ,
    // GEMM time per step 2 245 us unrotated -> 2 025 at stride 2 (1: 2 050, 3: 2 057, 5: 2 055, 11: 2 053); the split-K launches like 1 best
    int krot_m = 0;
    // GRIP_GEMM_COLGROUP=n: row-band / column-group tile walk of the persistent kernel (0 = the even N-fastest split).  Off: measured slower on the pool
    // encode (r02: c_fc 794 vs 839 TF/s, QKV 891 vs 922 with groups of 4 / 3 column tiles)
    int colgroup = 0;
    // GRIP_GEMM_EMODE: epilogue form of the persistent kernel, three digits for QKV / c_fc / residual (below 100: one mode for all).  0 = 8-byte stores
    // through the f32 slab, 1 = 16-byte stores, 2 = direct with permuted W fragment rows, 4 = fold arithmetic in the fragment layout + f16 slab.
    // TF/s in the loop: QKV 942 (1) / 929 (2) / 972 (4); c_fc 870 (1) / 892 (2) / 872 (4); residual 1 007 (1) / 954 (2)
    int emode = 421;
    // GRIP_GEMM_SD=0: the branchy sub-step 1 for the three default pool-encode instantiations.  Default on: loop +0.9 %, residual GEMM 987 -> 1 010 TF/s
    bool sd = true;
};
const GemmTuning& gemm_tuning();    // the process's knobs, read from the environment at the first call

// What the decision reads of a launch: the integers of GemmArgs, which optional buffers are present, and the CUs the launch may use.
struct GemmShape {
    int epi;
    int M, N, K, ldc;
    int64_t m_pad;
    int variant, ksplit, f32, rot_rows;
    int stat_parts;
    int64_t split_stride;
    bool stat_part, stat_in, rowstat, out2, coop;   // coop: coop_scratch and coop_counter both set
    int n_cu;                                       // device CUs, already cut by grip_cu_budget()
};

struct GemmPlan {
    int status;           // GRIP_OK, or GRIP_ERR_ARG with the message in msg
    GemmFamily family;
    int epi;              // the instantiation's epilogue (EPI_BIAS_RESID becomes EPI_BIAS_RESID_STATS when stat_part is set)
    int tile_m, tile_n;   // tile rows / columns.  WMF of gemm_ringw_kernel and RF of gemm_k64_kernel = tile_m / 32; WMF of gemm_f16_kernel = tile_m / 32
    int nst;              // ring depth / LDS stages
    int emode;            // gemm_k64p_kernel only
    bool sd;              // gemm_k64p_kernel only
    int tiles_m, tiles_n; // kernel arguments
    int colgroup;         // kernel argument of gemm_k64p_kernel
    unsigned grid_x, grid_y, block;
    int lds;              // dynamic LDS bytes
    int rot_rows;         // GemmArgs::rot_rows as the kernel sees it: the K-rotation stride
    bool finalize_stats;  // ln_stats_finalize(stat_in -> rowstat) runs first and the kernel sees stat_parts = 0
    int variant;          // profiler variant: slot = variant * 16 + epi
    char msg[240];
};

GemmPlan gemm_plan(const GemmShape& g, const GemmTuning& t);
// "gemm_ringw_kernel<3, 4, 1> grid 56x4 block 512 lds 81920 ...": the kernel as a profiler names it, then the launch (lds = dynamic bytes)
int gemm_plan_text(const GemmPlan& p, char* out, int out_len);

int gemm_pick_ksplit(int M, int N, int K, const GemmTuning& t);
int gemm_pick_coop_split(int M, int N, int K, const GemmTuning& t);
int gemm_pick_ksplit(int M, int N, int K);        // with gemm_tuning()
int gemm_pick_coop_split(int M, int N, int K);    // split factor of the cooperative form (1 = not worth it / not applicable)
