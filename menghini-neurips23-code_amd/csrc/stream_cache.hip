// Test-time streaming cache (include/grip_amd.h, grip_stream_cache_plan / grip_stream_cache_head; after TDA, Karmanov et al., CVPR 2024, as the model of
// the header states it).  The test items stream by in dataset order; per class a positive and a negative queue keep the lowest-entropy items seen so
// far, and item i is scored against the queue contents of ITS moment.  The queue updates depend on the BASE logits alone, so the stream splits in two:
//   plan   sc_row_kernel      a wave per row: H, the first arg-max and the mask row of 'uncertain' classes (the statements of view_entropy.hip), and
//                             leave[j] := j (never admitted) for both polarities;
//          sc_scan_kernel     a wave per (class, polarity) walks pred 64 items at a time (one ballot per chunk) and plays the queue of its class: lane q
//                             holds resident q, the resident with the largest (H, index) is a 4-step shuffle maximum over 16 lanes.  The queues of
//                             different classes never interact: no atomic, no cross-workgroup wait.  An item's leave is written ONCE, by the wave of
//                             its class: at its eviction (the evicting item's index) or at the end (INT32_MAX);
//          sc_compact_kernel  one workgroup per polarity packs the ever-admitted items (leave[j] != j), ascending, into the key list and counts them.
//   head   sc_rnorm_kernel    1 / |f_i| per row into the workspace (cache_head.hip's kernel and rule: applied to the SCORE, img_emb is never copied);
//          sc_head_kernel     cache_head.hip's f32-MFMA main loop (64 rows x 64 keys, e staged 32 floats at a time through two LDS buffers), with the
//                             key rows GATHERED from img_emb through the key list.  A workgroup owns 64 rows of one polarity and stops at the last
//                             key tile that holds a key j <= its last row (the tiles beyond lie wholly in its future: none of their terms is in a sum).
//                             Per key tile the 64 x 64 scores go to the LDS; thread (row, q) walks the tile's keys in ascending order and, for a LIVE
//                             pair (j <= i < leave_j) only, forms exp(-beta (1 - s rn_i rn_j)) and adds it to S[pol][i, y] of the classes y = q mod 4
//                             it owns: one writer per element, ascending j, no atomics; the [n, m] affinities never exist in memory.
//          sc_finish_kernel   out = base, then + alpha_p S_pos where S_pos != 0, then - alpha_n S_neg where S_neg != 0 (products rounded, then added).
// A row's bits depend on its own operands only (an MFMA chain over e per pair, the ascending-j sum): not on n, not on where the tiles fall.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {
constexpr int SC_BM = 64;                         // rows per workgroup (16 per wave)
constexpr int SC_BN = 64;                         // keys per tile
constexpr int SC_BK = 32;                         // floats of e per stage
constexpr int SC_STAGE = (SC_BM + SC_BN) * SC_BK; // floats per stage = 16 KiB
constexpr int SC_AP = SC_BN + 1;                  // pitch of the score tile
constexpr int SC_MAX_E = 1024;
constexpr int SC_MAX_CAP = 16;                    // a queue lives in the low 16 lanes of its wave
constexpr int SC_MAX_N = 1 << 30;

__device__ __forceinline__ float sc_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// A wave per row.  lse and H: the statements of view_entropy.hip (lane l adds the classes l, l + 64, ... ascending, then wave_sum).
__global__ __launch_bounds__(256) void sc_row_kernel(const float* __restrict__ x, int n, int c, float mask_lo, float mask_hi, float* __restrict__ H,
                                                     int32_t* __restrict__ pred, int32_t* __restrict__ pos_leave, int32_t* __restrict__ neg_leave,
                                                     int32_t* __restrict__ negbits) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;       // per wave
    const float* xr = x + (size_t)row * c;
    float m = -INFINITY, bv = -INFINITY;
    int bi = INT_MAX;
    for (int j = lane; j < c; j += 64) {
        const float v = xr[j];
        m = fmaxf(m, v);
        if (v > bv) { bv = v; bi = j; }       // the lane's first maximum
    }
    m = sc_wave_max(m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    float sum = 0.f;
    for (int j = lane; j < c; j += 64) sum += expf(xr[j] - m);
    sum = wave_sum(sum);
    const float lse = m + logf(sum);
    float h = 0.f;
    const int words = (c + 31) >> 5;
    int32_t* nb = negbits + (size_t)row * words;
    for (int j0 = 0; j0 < c; j0 += 64) {       // (per wave: the ballot needs every lane)
        const int j = j0 + lane;
        bool bit = false;
        if (j < c) {
            const float d = lse - xr[j];      // >= 0
            const float p = expf(-d);
            h += p * d;
            bit = mask_lo < p && p < mask_hi;
        }
        const unsigned long long bits = __ballot(bit);
        if (lane == 0) {
            nb[j0 >> 5] = (int32_t)(uint32_t)bits;
            if ((j0 >> 5) + 1 < words) nb[(j0 >> 5) + 1] = (int32_t)(uint32_t)(bits >> 32);
        }
    }
    h = wave_sum(h);
    if (lane == 0) {
        H[row] = h;
        pred[row] = bi == INT_MAX ? 0 : bi;      // (INT_MAX: no entry compared greater than -inf, e.g. a row of NaNs; its H is not finite)
        pos_leave[row] = (int32_t)row;
        neg_leave[row] = (int32_t)row;
    }
}

// A wave per (class, polarity): wave w plays the queue of class w >> 1, polarity w & 1 (0 positive, 1 negative).
__global__ __launch_bounds__(256) void sc_scan_kernel(const float* __restrict__ H, const int32_t* __restrict__ pred, int n, int c, int pos_cap, int neg_cap,
                                                      float ent_lo, float ent_hi, float logc, int32_t* __restrict__ pos_leave,
                                                      int32_t* __restrict__ neg_leave) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int cls = w >> 1, pol = w & 1;
    if (cls >= c) return;       // per wave; the kernel has no barrier
    const int cap = pol ? neg_cap : pos_cap;
    if (cap == 0) return;
    int32_t* leave = pol ? neg_leave : pos_leave;
    float qh = -INFINITY;       // lane q < cnt holds resident q; every other lane (-inf, -1), which never is the largest
    int qi = -1, cnt = 0;
    for (int b = 0; b < n; b += 64) {
        const int j = b + lane;
        const bool mine = j < n && pred[j] == cls;
        const float h = mine ? H[j] : 0.f;
        bool ok = mine && (h - h == 0.f);       // a non-finite H is never admitted
        if (pol) {
            const float hn = c > 1 ? h / logc : 0.f;
            ok = ok && ent_lo < hn && hn < ent_hi;
        }
        unsigned long long bits = __ballot(ok);
        while (bits) {       // the chunk's candidates in stream order; everything below is wave-uniform but the lane's own resident
            const int src = __builtin_ctzll(bits);
            bits &= bits - 1;
            const float hj = __shfl(h, src);
            const int jj = b + src;
            if (cnt < cap) {
                if (lane == cnt) { qh = hj; qi = jj; }
                ++cnt;
                continue;
            }
            float wh = qh;
            int wi = qi;
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) {
                const float oh = __shfl_xor(wh, off);
                const int oi = __shfl_xor(wi, off);
                if (oh > wh || (oh == wh && oi > wi)) { wh = oh; wi = oi; }
            }
            wh = __shfl(wh, 0);
            wi = __shfl(wi, 0);
            if (hj < wh && lane < SC_MAX_CAP && qi == wi) {
                leave[wi] = jj;       // the resident with the largest (H, index) leaves when jj enters
                qh = hj;
                qi = jj;
            }
        }
    }
    if (lane < cnt) leave[qi] = INT32_MAX;
}

// grid 2: workgroup `pol` packs the items with leave[j] != j, ascending, and writes their count.
__global__ __launch_bounds__(256) void sc_compact_kernel(const int32_t* __restrict__ pos_leave, const int32_t* __restrict__ neg_leave, int n,
                                                         int32_t* __restrict__ pos_key, int32_t* __restrict__ neg_key, int32_t* __restrict__ counts) {
    __shared__ int wtot[4];
    const int pol = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* leave = pol ? neg_leave : pos_leave;
    int32_t* key = pol ? neg_key : pos_key;
    int base = 0;
    for (int b = 0; b < n; b += 256) {
        const int j = b + tid;
        const bool in = j < n && leave[j] != j;
        const unsigned long long bits = __ballot(in);
        if (lane == 0) wtot[wave] = __popcll(bits);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q < wave) off += wtot[q];
            tot += wtot[q];
        }
        if (in) key[off + __popcll(bits & ((1ull << lane) - 1ull))] = j;
        base += tot;
        __syncthreads();
    }
    if (tid == 0) counts[pol] = base;
}

__global__ __launch_bounds__(256) void sc_rnorm_kernel(const float* __restrict__ f, float* __restrict__ rnorm, int n, int e) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;       // per wave
    const f32x4* p = (const f32x4*)(f + (size_t)row * e);
    float s = 0.f;
    for (int i = lane; i < (e >> 2); i += 64) {
        const f32x4 v = p[i];
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    s = wave_sum(s);
    if (lane == 0) rnorm[row] = 1.0f / sqrtf(s);
}

// exp(-beta (1 - f^_i . f^_j)) from the row-scaled score; both polarities inline it and must round alike
__device__ __forceinline__ float sc_affinity(float s_rni, float rnj, float beta) {
#pragma clang fp contract(off)
    const float s = s_rni * rnj;
    return expf(-(beta * (1.0f - s)));
}

// grid (ceil(n / 64), polarities).  S [polarities][n, c], zero on entry.
__global__ __launch_bounds__(256) void sc_head_kernel(const float* __restrict__ f, const float* __restrict__ rnorm, const int32_t* __restrict__ pred,
                                                      const int32_t* __restrict__ negbits, const int32_t* __restrict__ pos_leave,
                                                      const int32_t* __restrict__ neg_leave, const int32_t* __restrict__ pos_key,
                                                      const int32_t* __restrict__ neg_key, const int32_t* __restrict__ counts, float pos_beta, float neg_beta,
                                                      int n, int c, int e, float* __restrict__ S) {
    __shared__ __attribute__((aligned(16))) float lds[2 * SC_STAGE];
    __shared__ float At[SC_BM * SC_AP];
    __shared__ int kj[SC_BN], klv[SC_BN], kc[SC_BN];
    __shared__ float krn[SC_BN];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int r0 = blockIdx.x * SC_BM, pol = blockIdx.y;
    const int32_t* key = pol ? neg_key : pos_key;
    const int32_t* leave = pol ? neg_leave : pos_leave;
    const float beta = pol ? neg_beta : pos_beta;
    float* Sp = S + (size_t)pol * n * c;
    const int words = (c + 31) >> 5;
    // the keys that are not in the future of the tile's last row: the list is ascending, so they are its first m_eff entries
    const int m = min(max(counts[pol], 0), n), r_last = min(r0 + SC_BM, n) - 1;
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] <= r_last) lo = mid + 1;
        else hi = mid;
    }
    const int m_eff = lo;
    const int nec = (e + SC_BK - 1) / SC_BK, nkt = (m_eff + SC_BN - 1) / SC_BN, T = nkt * nec;
    if (T == 0) return;       // (the whole workgroup)

    // staging as in cache_head.hip; the key row of tile slot `row` is img_emb[key[kt * 64 + row]] (a slot past m_eff, or an index outside [0, n): zeros)
    f32x4 fr[2], kr[2];
    const float* krow[2] = {f, f};
    bool kok[2] = {false, false};
    auto gload = [&](int kt, int ec) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, col = ec * SC_BK + (id & 7) * 4;
            const int gr = r0 + row, gk = kt * SC_BN + row;
            if (ec == 0) {
                const int jj = gk < m_eff ? key[gk] : -1;
                kok[i] = jj >= 0 && jj < n;
                krow[i] = f + (size_t)(kok[i] ? jj : 0) * e;
            }
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            fr[i] = (gr < n && col < e) ? *(const f32x4*)(f + (size_t)gr * e + col) : zero;
            kr[i] = (kok[i] && col < e) ? *(const f32x4*)(krow[i] + col) : zero;
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, ch = (id & 7) ^ (row & 7);
            float* st = lds + buf * SC_STAGE + row * SC_BK + ch * 4;
            *(f32x4*)st = fr[i];
            *(f32x4*)(st + SC_BM * SC_BK) = kr[i];
        }
    };

    int a_off[2], b_off[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int chunk = (kk * 4 + fgrp) ^ (lane & 7);
        a_off[kk] = (wave * 16 + frow) * SC_BK + chunk * 4;
        b_off[kk] = SC_BM * SC_BK + frow * SC_BK + chunk * 4;
    }
    const int my_row = r0 + wave * 16 + frow;
    const float rn = my_row < n ? rnorm[my_row] : 0.f;

    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    gload(0, 0);
    sstore(0);
    __syncthreads();
    int kt = 0, ec = 0;
    for (int t = 0; t < T; ++t) {
        const int buf = t & 1;
        int nkt_ = kt, nec_ = ec + 1;
        if (nec_ == nec) { nec_ = 0; ++nkt_; }
        if (t + 1 < T) gload(nkt_, nec_);
        const float* st = lds + buf * SC_STAGE;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f32x4 bf[4];
            const f32x4 af = *(const f32x4*)(st + a_off[kk]);
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = *(const f32x4*)(st + b_off[kk] + j * 16 * SC_BK);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][s], af[s], acc[j], 0, 0, 0);
        }
        if (t + 1 < T) sstore(buf ^ 1);
        if (ec == nec - 1) {
            // lane (frow, fgrp) holds the scores of row wave*16 + frow against the tile's keys j*16 + fgrp*4 + {0..3}
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) At[(wave * 16 + frow) * SC_AP + j * 16 + fgrp * 4 + r] = acc[j][r] * rn;
                acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            if (tid < SC_BN) {       // what the tile's keys are: index, end of residence, class, 1 / |f_j|
                const int gk = kt * SC_BN + tid;
                const int jj = gk < m_eff ? key[gk] : -1;
                const bool ok = jj >= 0 && jj < n;
                kj[tid] = ok ? jj : INT_MAX;       // (INT_MAX: in every row's future)
                klv[tid] = ok ? leave[jj] : 0;
                kc[tid] = ok ? pred[jj] : -1;
                krn[tid] = ok ? rnorm[jj] : 0.f;
            }
            __syncthreads();
            const int row = tid & 63, gr = r0 + row, q = wave;
            if (gr < n) {
                const float* ar = At + row * SC_AP;
                float* srow = Sp + (size_t)gr * c;
                for (int kl = 0; kl < SC_BN; ++kl) {
                    const int jj = kj[kl];
                    if (jj > gr) break;                  // ascending: the rest is in this row's future too
                    if (gr >= klv[kl]) continue;         // it had left before item gr was scored
                    if (!pol) {
                        const int y = kc[kl];
                        if ((y & 3) == q && y >= 0 && y < c) srow[y] += sc_affinity(ar[kl], krn[kl], beta);
                    } else {
                        const int32_t* nb = negbits + (size_t)jj * words;
                        float a = 0.f;
                        bool have = false;
                        for (int wd = 0; wd < words; ++wd) {
                            uint32_t bits = (uint32_t)nb[wd] & (0x11111111u << q);       // the classes = q mod 4
                            while (bits) {
                                const int y = wd * 32 + __builtin_ctz(bits);
                                bits &= bits - 1;
                                if (y >= c) break;
                                if (!have) { a = sc_affinity(ar[kl], krn[kl], beta); have = true; }
                                srow[y] += a;
                            }
                        }
                    }
                }
            }
        }
        kt = nkt_;
        ec = nec_;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void sc_finish_kernel(const float* __restrict__ base, const float* __restrict__ S, int polarities, size_t total,
                                                        float pos_alpha, float neg_alpha, float* __restrict__ out) {
#pragma clang fp contract(off)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        float v = base[i];
        const float sp = S[i];
        if (sp != 0.f) {
            const float t = pos_alpha * sp;
            v = v + t;
        }
        if (polarities > 1) {
            const float sn = S[total + i];
            if (sn != 0.f) {
                const float t = neg_alpha * sn;
                v = v - t;
            }
        }
        out[i] = v;
    }
}

bool sc_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool sc_finite(float v) { return v - v == 0.f; }

int sc_check_shape(const char* who, int n, int c) {
    GRIP_REQUIRE(n >= 1 && n <= SC_MAX_N && c >= 1, "%s: n = %d, c = %d (1 <= n <= %d, c >= 1)", who, n, c, SC_MAX_N);
    return GRIP_OK;
}
int sc_check_e(const char* who, int e) {
    GRIP_REQUIRE(e >= 4 && e % 4 == 0 && e <= SC_MAX_E, "%s: e = %d (a multiple of 4, 4 .. %d)", who, e, SC_MAX_E);
    return GRIP_OK;
}
size_t sc_rnorm_bytes(int n) { return ((size_t)n * sizeof(float) + 255) & ~(size_t)255; }
size_t sc_head_ws_bytes(int n, int c) { return 256 + sc_rnorm_bytes(n) + 2 * (size_t)n * c * sizeof(float); }
}  // namespace

#define RUNC(x) do { int _rc = (x); if (_rc != GRIP_OK) return _rc; } while (0)

extern "C" int grip_stream_cache_plan_workspace(int n, int c, size_t* bytes) {
    GRIP_REQUIRE(bytes, "stream_cache_plan_workspace: null pointer");
    RUNC(sc_check_shape("stream_cache_plan_workspace", n, c));
    *bytes = 0;
    return GRIP_OK;
}

extern "C" int grip_stream_cache_plan(const float* base_logits, int n, int c, int pos_cap, int neg_cap, float ent_lo, float ent_hi, float mask_lo,
                                      float mask_hi, float* entropy_out, int32_t* pred_out, int32_t* pos_leave, int32_t* neg_leave, int32_t* negbits_out,
                                      int32_t* pos_key, int32_t* neg_key, int32_t* counts_out, void* workspace, size_t workspace_bytes, void* stream) {
    RUNC(sc_check_shape("stream_cache_plan", n, c));
    GRIP_REQUIRE(pos_cap >= 1 && pos_cap <= SC_MAX_CAP && neg_cap >= 0 && neg_cap <= SC_MAX_CAP,
                 "stream_cache_plan: pos_cap = %d, neg_cap = %d (1 .. %d and 0 .. %d)", pos_cap, neg_cap, SC_MAX_CAP, SC_MAX_CAP);
    GRIP_REQUIRE(sc_finite(ent_lo) && sc_finite(ent_hi) && sc_finite(mask_lo) && sc_finite(mask_hi) && ent_lo <= ent_hi && mask_lo <= mask_hi,
                 "stream_cache_plan: entropy window (%g, %g), mask window (%g, %g) (finite, lo <= hi)", ent_lo, ent_hi, mask_lo, mask_hi);
    GRIP_REQUIRE(base_logits && entropy_out && pred_out && pos_leave && neg_leave && negbits_out && pos_key && neg_key && counts_out,
                 "stream_cache_plan: null pointer");
    (void)workspace;
    (void)workspace_bytes;
    hipStream_t s = (hipStream_t)stream;
    const float logc = (float)log((double)c);
    hipLaunchKernelGGL(sc_row_kernel, dim3((n + 3) / 4), dim3(256), 0, s, base_logits, n, c, mask_lo, mask_hi, entropy_out, pred_out, pos_leave, neg_leave,
                       negbits_out);
    GRIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_scan_kernel, dim3((unsigned)((2 * (int64_t)c + 3) / 4)), dim3(256), 0, s, entropy_out, pred_out, n, c, pos_cap, neg_cap, ent_lo,
                       ent_hi, logc, pos_leave, neg_leave);
    GRIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_compact_kernel, dim3(2), dim3(256), 0, s, pos_leave, neg_leave, n, pos_key, neg_key, counts_out);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}

extern "C" int grip_stream_cache_head_workspace(int n, int c, int e, size_t* bytes) {
    GRIP_REQUIRE(bytes, "stream_cache_head_workspace: null pointer");
    RUNC(sc_check_shape("stream_cache_head_workspace", n, c));
    RUNC(sc_check_e("stream_cache_head_workspace", e));
    *bytes = sc_head_ws_bytes(n, c);
    return GRIP_OK;
}

extern "C" int grip_stream_cache_head(const float* base_logits, const float* img_emb, const int32_t* pred, const int32_t* negbits, const int32_t* pos_leave,
                                      const int32_t* neg_leave, const int32_t* pos_key, const int32_t* neg_key, const int32_t* counts, float pos_alpha,
                                      float pos_beta, float neg_alpha, float neg_beta, int n, int c, int e, float* out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    RUNC(sc_check_shape("stream_cache_head", n, c));
    RUNC(sc_check_e("stream_cache_head", e));
    GRIP_REQUIRE(sc_finite(pos_alpha) && sc_finite(pos_beta) && sc_finite(neg_alpha) && sc_finite(neg_beta),
                 "stream_cache_head: alpha / beta = %g / %g (positive), %g / %g (negative) must be finite", pos_alpha, pos_beta, neg_alpha, neg_beta);
    GRIP_REQUIRE(base_logits && img_emb && pred && pos_leave && pos_key && counts && out && workspace, "stream_cache_head: null pointer");
    const bool neg = negbits || neg_leave || neg_key;
    GRIP_REQUIRE(!neg || (negbits && neg_leave && neg_key), "stream_cache_head: negbits, neg_leave and neg_key go together (all NULL: no negative term)");
    GRIP_REQUIRE(sc_aligned16(img_emb), "stream_cache_head: img_emb must be 16-byte aligned");
    GRIP_REQUIRE(workspace_bytes >= sc_head_ws_bytes(n, c), "stream_cache_head: workspace too small (%zu bytes, grip_stream_cache_head_workspace says %zu)",
                 workspace_bytes, sc_head_ws_bytes(n, c));
    hipStream_t s = (hipStream_t)stream;
    float* rnorm = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* S = (float*)((char*)rnorm + sc_rnorm_bytes(n));
    const int pols = neg ? 2 : 1;
    const size_t total = (size_t)n * c;
    GRIP_CHECK_HIP(hipMemsetAsync(S, 0, pols * total * sizeof(float), s));
    hipLaunchKernelGGL(sc_rnorm_kernel, dim3((n + 3) / 4), dim3(256), 0, s, img_emb, rnorm, n, e);
    GRIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_head_kernel, dim3((n + SC_BM - 1) / SC_BM, pols), dim3(256), 0, s, img_emb, rnorm, pred, negbits, pos_leave, neg_leave, pos_key,
                       neg_key, counts, pos_beta, neg_beta, n, c, e, S);
    GRIP_CHECK_HIP(hipGetLastError());
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(sc_finish_kernel, dim3(blocks), dim3(256), 0, s, base_logits, S, pols, total, pos_alpha, neg_alpha, out);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}
