// Transductive GMM pseudolabelling over a pool (after TransCLIP-ZS, Zanella et al., NeurIPS 2024 -- the recursion is the one of include/grip_amd.h, not
// that code): one Gaussian per class with a shared diagonal covariance fitted to the pool's unit image embeddings, the assignments anchored to the text
// head by a KL term and smoothed over the directed kNN graph of grip_knn_graph.  All f32 / int32, no atomics, every sum in a fixed order.
//   * grip_gmm_mstep: N_c = sum_i Z_ic, mu_c = (sum_i Z_ic F_i) / N_c, var_d = max(var_floor, (1 / n) sum_i sum_c Z_ic (F_id - mu_cd)^2).
//       - gmm_sum_kernel: Z^T F is a GEMM whose long dimension is n.  The rows are cut into chunks of GM_ROWS (a constant: the partition does not depend on
//         the device); a workgroup owns one chunk, 16 classes and 512 columns, a wave 16 classes x 128 columns in eight v_mfma_f32_16x16x4_f32
//         accumulators, four rows per step.  Both operands come straight from memory in MFMA layout (a lane's Z scalar; a lane's four consecutive floats
//         of F feed the four MFMAs of a column group), rows >= n, classes >= c and columns >= e are zeros.  The class counts are one more MFMA against
//         ones (wave 0 of the first column block).  A chunk's partial [c, e] and [c] go to the workspace.
//       - gmm_mean_kernel adds the partials in a FIXED order (four contiguous slices of the chunks, each ascending, then the slices ascending) and
//         divides; N_c == 0 gives a zero centre.
//       - gmm_var_kernel is the direct two-pass form on the VALU: a wave owns GM_VROWS rows and 256 columns (a lane four), eight centres at a time in
//         registers, the weights Z_ic wave-uniform; gmm_var_final_kernel adds the partials in a fixed order (sixteen contiguous slices, each ascending, then the
//         slices ascending), divides by n and applies the floor.
//   * grip_gmm_estep: G_ic = F_i . (mu_c / var) - 1/2 sum_d mu_cd^2 / var_d, then z_iters Jacobi sweeps Z_i <- softmax_c(G_ic + lam log max(P_ic, 2^-126)
//     + sum_j max(0, sim_ij) Z_{idx_ij, c}).
//       - gmm_prep_kernel (a wave per class) writes W_c = mu_c / var and the bias 1/2 mu_c . W_c to the workspace;
//       - gmm_score_kernel is the main loop of knn_graph.hip / cache_head.hip (64 rows per workgroup, the classes 64 at a time, e staged 32 floats per
//         step through two XOR-swizzled LDS buffers, the loads of step t + 1 in flight under the MFMAs of step t; the chain over e ascending) with an
//         epilogue that subtracts the bias, adds lam log max(P, 2^-126) -- the part of a sweep's argument that no sweep changes -- and writes the [n, c]
//         static scores to the workspace.  A score depends on the row of F and the row of W only: bit-equal classes score bit-equally.
//       - gmm_sweep_kernel is a wave per row in the manner of lp_step_kernel: lanes over classes, the k neighbour rows gathered and added IN LIST ORDER,
//         the softmax with the row's maximum subtracted first.  A sweep reads the previous sweep's Z (ping-pong between z_out and the workspace, never in
//         place); the last one also writes the row's first arg-max.  Up to 128 classes the row's scores stay in registers; beyond, they wait in the
//         sweep's own output row between the passes (a lane re-reads only what it wrote itself).
#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {
constexpr int GM_ROWS = 256;                      // rows per chunk of the M-step's sums (engine.GMM_MSTEP_ROWS)
constexpr int GM_VROWS = 32;                      // rows per chunk of the M-step's variance
constexpr int GM_CT = 16;                         // classes per workgroup of gmm_sum_kernel
constexpr int GM_ET = 512;                        // columns per workgroup of gmm_sum_kernel (128 per wave)
constexpr int GM_VC = 8;                          // centres held in registers at a time by gmm_var_kernel
constexpr int GM_MS = 4;                          // slices of the chunk partials in gmm_mean_kernel
constexpr int GM_VS = 16;                         // slices of the chunk partials in gmm_var_final_kernel
constexpr int GM_BM = 64;                         // rows per workgroup of gmm_score_kernel (16 per wave)
constexpr int GM_BN = 64;                         // classes per tile
constexpr int GM_BK = 32;                         // floats of e per stage (one 128-byte line per row)
constexpr int GM_STAGE = (GM_BM + GM_BN) * GM_BK; // floats per stage = 16 KiB
constexpr int GM_MAX_K = 32;
constexpr int GM_MAX_E = 2048;
constexpr int GM_REG_C = 128;                     // classes a sweep keeps in registers at most (two per lane)

// partial sums of chunk blockIdx.x / ctiles: psum[chunk, cls, :] = sum over the chunk's rows of Z[row, cls] F[row, :], pcnt[chunk, cls] = sum of Z[row, cls]
__global__ __launch_bounds__(256) void gmm_sum_kernel(const float* __restrict__ z, const float* __restrict__ f, int n, int c, int e, int ctiles,
                                                      float* __restrict__ psum, float* __restrict__ pcnt) {
    const int lane = threadIdx.x & 63, frow = lane & 15, fgrp = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunk = blockIdx.x / ctiles, c0 = (blockIdx.x - chunk * ctiles) * GM_CT;
    const int d0 = blockIdx.y * GM_ET + wave * 128;
    if (d0 >= e) return;        // per wave (the kernel has no barrier)
    const int r0 = chunk * GM_ROWS, r1 = min(n, r0 + GM_ROWS);
    const bool cls_ok = c0 + frow < c;
    const bool counts = blockIdx.y == 0 && wave == 0;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[2][4], cnt = zero;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[h][j] = zero;
    // lane (frow, fgrp) of step r: Z[r + fgrp, c0 + frow] (A: class x row) and F[r + fgrp, d0 + h * 64 + frow * 4 + j] (B of MFMA (h, j): row x column)
    for (int r = r0; r < r1; r += 4) {
        const int row = r + fgrp;
        const bool ok = row < r1;
        const float a = (ok && cls_ok) ? z[(size_t)row * c + c0 + frow] : 0.f;
        f32x4 b[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int col = d0 + h * 64 + frow * 4;
            b[h] = (ok && col < e) ? *(const f32x4*)(f + (size_t)row * e + col) : zero;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[h][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[h][j], acc[h][j], 0, 0, 0);
        if (counts) cnt = __builtin_amdgcn_mfma_f32_16x16x4f32(a, 1.0f, cnt, 0, 0, 0);
    }
    // the lane holds classes c0 + fgrp * 4 + {0..3} of columns d0 + h * 64 + frow * 4 + {j}
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int cls = c0 + fgrp * 4 + r;
        if (cls >= c) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int col = d0 + h * 64 + frow * 4;
            if (col < e) *(f32x4*)(psum + ((size_t)chunk * c + cls) * e + col) = (f32x4){acc[h][0][r], acc[h][1][r], acc[h][2][r], acc[h][3][r]};
        }
        if (counts && frow == 0) pcnt[(size_t)chunk * c + cls] = cnt[r];
    }
}

// 64 (class, four columns) items per workgroup, GM_MS threads per item: thread (item, s) adds the partials of the chunks [s per, (s + 1) per), per =
// ceil(nch / GM_MS), in ascending order, and thread (item, 0) adds the GM_MS slices in ascending order -- an order fixed by n alone; mean = sum / count, the
// zero vector where the count is exactly 0
__global__ __launch_bounds__(64 * GM_MS) void gmm_mean_kernel(const float* __restrict__ psum, const float* __restrict__ pcnt, int nch, int c, int e,
                                                              float* __restrict__ count_out, float* __restrict__ mean_out) {
    __shared__ f32x4 ssum[GM_MS][64];
    __shared__ float scnt[GM_MS][64];
    const int e4 = e >> 2, it = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + it;
    const bool ok = t < c * e4;
    const int cls = ok ? t / e4 : 0, col = ok ? (t - cls * e4) * 4 : 0;
    const int per = (nch + GM_MS - 1) / GM_MS, ch0 = sl * per, ch1 = min(nch, ch0 + per);
    float cnt = 0.f;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (ok)
        for (int ch = ch0; ch < ch1; ++ch) {
            cnt += pcnt[(size_t)ch * c + cls];
            s += *(const f32x4*)(psum + ((size_t)ch * c + cls) * e + col);
        }
    ssum[sl][it] = s;
    scnt[sl][it] = cnt;
    __syncthreads();
    if (!ok || sl != 0) return;
#pragma unroll
    for (int q = 1; q < GM_MS; ++q) {
        cnt += scnt[q][it];
        s += ssum[q][it];
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    *(f32x4*)(mean_out + (size_t)cls * e + col) = cnt == 0.f ? zero : s / cnt;
    if (col == 0) count_out[cls] = cnt;
}

// pvar[chunk, :] = sum over the chunk's rows and all classes of Z[row, cls] (F[row, :] - mean[cls, :])^2: a wave per (chunk, 256 columns)
__global__ __launch_bounds__(64) void gmm_var_kernel(const float* __restrict__ z, const float* __restrict__ f, const float* __restrict__ mean, int n, int c,
                                                     int e, float* __restrict__ pvar) {
    const int col = blockIdx.y * 256 + threadIdx.x * 4;
    if (col >= e) return;
    const int r0 = blockIdx.x * GM_VROWS, r1 = min(n, r0 + GM_VROWS);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc = zero;
    for (int cb = 0; cb < c; cb += GM_VC) {
        f32x4 m[GM_VC];
#pragma unroll
        for (int q = 0; q < GM_VC; ++q) m[q] = cb + q < c ? -*(const f32x4*)(mean + (size_t)(cb + q) * e + col) : zero;     // (negated once: F + (-mu) packs, and is F - mu bit for bit)
        for (int row = r0; row < r1; ++row) {
            const f32x4 fv = *(const f32x4*)(f + (size_t)row * e + col);
            const float* zr = z + (size_t)row * c + cb;
#pragma unroll
            for (int q = 0; q < GM_VC; ++q) {
                const float w = cb + q < c ? zr[q] : 0.f;       // (wave-uniform)
                const f32x4 d = fv + m[q];
                acc += w * (d * d);
            }
        }
    }
    *(f32x4*)(pvar + (size_t)blockIdx.x * e + col) = acc;
}

// 64 columns per workgroup, GM_VS threads per column: thread (d, s) adds the partials of the chunks [s per, (s + 1) per), per = ceil(nvch / GM_VS), in
// ascending order, and thread (d, 0) adds the GM_VS slices in ascending order, divides by n and applies the floor
__global__ __launch_bounds__(64 * GM_VS) void gmm_var_final_kernel(const float* __restrict__ pvar, int nvch, int n, int e, float var_floor,
                                                                   float* __restrict__ var_out) {
    __shared__ float part[GM_VS][64];
    const int it = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int d = blockIdx.x * 64 + it;
    const int per = (nvch + GM_VS - 1) / GM_VS, ch0 = sl * per, ch1 = min(nvch, ch0 + per);
    float s = 0.f;
    if (d < e)
        for (int ch = ch0; ch < ch1; ++ch) s += pvar[(size_t)ch * e + d];
    part[sl][it] = s;
    __syncthreads();
    if (d >= e || sl != 0) return;
#pragma unroll
    for (int q = 1; q < GM_VS; ++q) s += part[q][it];
    var_out[d] = fmaxf(var_floor, s / (float)n);
}

// a wave per class: w[cls, :] = mean[cls, :] / var, bias[cls] = 1/2 sum_d mean[cls, d] w[cls, d]
__global__ __launch_bounds__(256) void gmm_prep_kernel(const float* __restrict__ mean, const float* __restrict__ var, int c, int e, float* __restrict__ w,
                                                       float* __restrict__ bias) {
    const int cls = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (cls >= c) return;       // per wave
    float s = 0.f;
    for (int i = lane; i < (e >> 2); i += 64) {
        const f32x4 m = *(const f32x4*)(mean + (size_t)cls * e + i * 4);
        const f32x4 q = m / *(const f32x4*)(var + i * 4);
        *(f32x4*)(w + (size_t)cls * e + i * 4) = q;
        s += m[0] * q[0] + m[1] * q[1] + m[2] * q[2] + m[3] * q[3];
    }
    s = wave_sum(s);
    if (lane == 0) bias[cls] = 0.5f * s;
}

// g[i, cls] = (F_i . W_cls - bias[cls]) + lam log max(probs[i, cls], 2^-126): the main loop of knn_graph_kernel with the classes as the base
__global__ __launch_bounds__(256) void gmm_score_kernel(const float* __restrict__ q, const float* __restrict__ base, const float* __restrict__ bias,
                                                        const float* __restrict__ probs, float lam, int n, int m, int e, float* __restrict__ g) {
    __shared__ __attribute__((aligned(16))) float lds[2 * GM_STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int r0 = blockIdx.x * GM_BM;
    const int nec = (e + GM_BK - 1) / GM_BK, nkt = (m + GM_BN - 1) / GM_BN;
    const int T = nkt * nec;

    // staging: thread t moves the 16-byte pieces t and t + 256 of the 64 x 32 row tile and of the class tile; the piece index within a row is XOR-swizzled
    // with (row & 7), so the fragment reads below are conflict-free.  Rows >= n, classes >= m and columns >= e are zeros.
    f32x4 fr[2], kr[2];
    auto gload = [&](int kt, int ec) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, col = ec * GM_BK + (id & 7) * 4;
            const int gr = r0 + row, gk = kt * GM_BN + row;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            fr[i] = (gr < n && col < e) ? *(const f32x4*)(q + (size_t)gr * e + col) : zero;
            kr[i] = (gk < m && col < e) ? *(const f32x4*)(base + (size_t)gk * e + col) : zero;
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            // each sixteen floats of a row are stored TRANSPOSED as 4 x 4 (float 4 s + g goes to chunk g, slot s): the MFMA of step s contracts the floats
            // 4 s .. 4 s + 3, so the chain over e is ASCENDING
            const int id = tid + 256 * i, row = id >> 3, kk = (id & 7) >> 2, sp = id & 3;
            float* st = lds + buf * GM_STAGE + row * GM_BK + sp;
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const int ch = (kk * 4 + gg) ^ (row & 7);
                st[ch * 4] = fr[i][gg];
                st[GM_BM * GM_BK + ch * 4] = kr[i][gg];
            }
        }
    };

    int a_off[2], b_off[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int chunk = (kk * 4 + fgrp) ^ (lane & 7);
        a_off[kk] = (wave * 16 + frow) * GM_BK + chunk * 4;
        b_off[kk] = GM_BM * GM_BK + frow * GM_BK + chunk * 4;
    }
    const int my_row = r0 + wave * 16 + frow;
    const bool row_ok = my_row < n;

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
        const float* st = lds + buf * GM_STAGE;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f32x4 bf[4];
            const f32x4 af = *(const f32x4*)(st + a_off[kk]);
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = *(const f32x4*)(st + b_off[kk] + j * 16 * GM_BK);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][s], af[s], acc[j], 0, 0, 0);
        }
        if (t + 1 < T) sstore(buf ^ 1);
        if (ec == nec - 1) {
            // lane (frow, fgrp) holds the scores of row wave*16 + frow against classes kt*64 + j*16 + fgrp*4 + {0..3}
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int cls = kt * GM_BN + j * 16 + fgrp * 4 + r;
                    if (row_ok && cls < m) {
                        const size_t o = (size_t)my_row * m + cls;
                        g[o] = (acc[j][r] - bias[cls]) + lam * logf(fmaxf(probs[o], FLT_MIN));
                    }
                }
                acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
        kt = nkt_;
        ec = nec_;
        __syncthreads();
    }
}

__device__ __forceinline__ float wave_max_all(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// one wave per row: zout[i, :] = softmax_c(g[i, c] + sum_j max(0, sim[i, j]) zin[idx[i, j], c]); argmax (optional): first index of the row's maximum.
// NP > 0: c <= 64 NP and the row's scores stay in registers; NP == 0: any c, they wait in zout[i, :] between the passes (zout is not zin).
template <int NP>
__global__ __launch_bounds__(256) void gmm_sweep_kernel(const float* __restrict__ g, const float* __restrict__ zin, const int32_t* __restrict__ idx,
                                                        const float* __restrict__ sim, int n, int c, int k, float* zout, int32_t* __restrict__ argmax) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;       // per wave
    const int my_idx = lane < k ? idx[(size_t)row * k + lane] : 0;
    const float my_w = lane < k ? fmaxf(0.f, sim[(size_t)row * k + lane]) : 0.f;
    const float* gr = g + (size_t)row * c;
    float* zr = zout + (size_t)row * c;
    auto score = [&](int cls) {
        float acc = 0.f;
        for (int j = 0; j < k; ++j) {
            const int nb = __builtin_amdgcn_readlane(my_idx, j);
            const float wj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_w), j));
            if (cls < c) acc = fmaf(wj, zin[(size_t)nb * c + cls], acc);
        }
        return cls < c ? gr[cls] + acc : -INFINITY;
    };
    constexpr int NR = NP > 0 ? NP : 1;
    float a[NR];
    float mx = -INFINITY, sum = 0.f;
    if (NP > 0) {
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            a[p] = score(p * 64 + lane);
            mx = fmaxf(mx, a[p]);
        }
        mx = wave_max_all(mx);
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            a[p] = expf(a[p] - mx);         // (a class >= c: exp(-inf) = 0)
            sum += a[p];
        }
    } else {
        for (int c0 = 0; c0 < c; c0 += 64) {
            const float v = score(c0 + lane);
            if (c0 + lane < c) zr[c0 + lane] = v;
            mx = fmaxf(mx, v);
        }
        mx = wave_max_all(mx);
        for (int c0 = 0; c0 < c; c0 += 64)
            if (c0 + lane < c) {
                const float x = expf(zr[c0 + lane] - mx);
                zr[c0 + lane] = x;
                sum += x;
            }
    }
    sum = wave_sum(sum);
    float bv = -INFINITY;
    int bi = INT_MAX;
    if (NP > 0) {
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int cls = p * 64 + lane;
            if (cls < c) {
                const float v = a[p] / sum;
                zr[cls] = v;
                if (v > bv) { bv = v; bi = cls; }
            }
        }
    } else {
        for (int c0 = 0; c0 < c; c0 += 64) {
            const int cls = c0 + lane;
            if (cls < c) {
                const float v = zr[cls] / sum;
                zr[cls] = v;
                if (v > bv) { bv = v; bi = cls; }
            }
        }
    }
    if (argmax) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) argmax[row] = bi;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}

int check_dims(const char* who, int n, int c, int e) {
    GRIP_REQUIRE(n > 0 && c > 0, "%s: n = %d, c = %d (each must be positive)", who, n, c);
    GRIP_REQUIRE(e > 0 && e % 4 == 0 && e <= GM_MAX_E, "%s: e = %d (a multiple of 4, 4 .. %d)", who, e, GM_MAX_E);
    GRIP_REQUIRE((int64_t)c * e <= INT_MAX && ((int64_t)n + GM_ROWS - 1) / GM_ROWS * ((c + GM_CT - 1) / GM_CT) <= INT_MAX,
                 "%s: n = %d, c = %d, e = %d (c e and the launch grid must stay below 2^31)", who, n, c, e);
    return GRIP_OK;
}
size_t pad64(size_t floats) { return (floats + 63) / 64 * 64; }
int m_chunks(int n) { return (n + GM_ROWS - 1) / GM_ROWS; }
int v_chunks(int n) { return (n + GM_VROWS - 1) / GM_VROWS; }
size_t m_psum(int n, int c, int e) { return pad64((size_t)m_chunks(n) * c * e); }
size_t m_pcnt(int n, int c) { return pad64((size_t)m_chunks(n) * c); }
size_t m_ws_bytes(int n, int c, int e) { return (m_psum(n, c, e) + m_pcnt(n, c) + pad64((size_t)v_chunks(n) * e)) * sizeof(float) + 256; }
size_t e_ws_bytes(int n, int c, int e) { return (pad64((size_t)c * e) + pad64((size_t)c) + 2 * pad64((size_t)n * c)) * sizeof(float) + 256; }
}  // namespace

#define RUNC(x) do { int _rc = (x); if (_rc != GRIP_OK) return _rc; } while (0)

extern "C" int grip_gmm_mstep_workspace(int n, int c, int e, size_t* bytes) {
    GRIP_REQUIRE(bytes, "gmm_mstep_workspace: null pointer");
    RUNC(check_dims("gmm_mstep_workspace", n, c, e));
    *bytes = m_ws_bytes(n, c, e);
    return GRIP_OK;
}

extern "C" int grip_gmm_mstep(const float* z, const float* feats, int n, int c, int e, float var_floor, float* count_out, float* mean_out, float* var_out,
                              void* workspace, size_t workspace_bytes, void* stream) {
    RUNC(check_dims("gmm_mstep", n, c, e));
    GRIP_REQUIRE(var_floor > 0.f && var_floor <= FLT_MAX, "gmm_mstep: var_floor = %g (a finite var_floor > 0)", (double)var_floor);
    GRIP_REQUIRE(z && feats && count_out && mean_out && var_out && workspace, "gmm_mstep: null pointer");
    GRIP_REQUIRE(aligned16(feats) && aligned16(mean_out), "gmm_mstep: feats and mean_out must be 16-byte aligned");
    const size_t zb = (size_t)n * c * 4, fb = (size_t)n * e * 4, mb = (size_t)c * e * 4;
    GRIP_REQUIRE(!overlap(mean_out, mb, z, zb) && !overlap(mean_out, mb, feats, fb) && !overlap(var_out, (size_t)e * 4, z, zb) &&
                     !overlap(var_out, (size_t)e * 4, feats, fb) && !overlap(count_out, (size_t)c * 4, z, zb) && !overlap(count_out, (size_t)c * 4, feats, fb),
                 "gmm_mstep: an output must not alias z or feats");
    GRIP_REQUIRE(workspace_bytes >= m_ws_bytes(n, c, e), "gmm_mstep: workspace too small (%zu bytes, grip_gmm_mstep_workspace says %zu)", workspace_bytes,
                 m_ws_bytes(n, c, e));
    hipStream_t s = (hipStream_t)stream;
    float* psum = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* pcnt = psum + m_psum(n, c, e);
    float* pvar = pcnt + m_pcnt(n, c);
    const int nch = m_chunks(n), nvch = v_chunks(n), ctiles = (c + GM_CT - 1) / GM_CT;
    hipLaunchKernelGGL(gmm_sum_kernel, dim3(nch * ctiles, (e + GM_ET - 1) / GM_ET), dim3(256), 0, s, z, feats, n, c, e, ctiles, psum, pcnt);
    GRIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(gmm_mean_kernel, dim3((c * (e >> 2) + 63) / 64), dim3(64 * GM_MS), 0, s, psum, pcnt, nch, c, e, count_out, mean_out);
    GRIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(gmm_var_kernel, dim3(nvch, (e + 255) / 256), dim3(64), 0, s, z, feats, mean_out, n, c, e, pvar);
    GRIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(gmm_var_final_kernel, dim3((e + 63) / 64), dim3(64 * GM_VS), 0, s, pvar, nvch, n, e, var_floor, var_out);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}

extern "C" int grip_gmm_estep_workspace(int n, int c, int e, int k, size_t* bytes) {
    GRIP_REQUIRE(bytes, "gmm_estep_workspace: null pointer");
    RUNC(check_dims("gmm_estep_workspace", n, c, e));
    GRIP_REQUIRE(k >= 1 && k <= GM_MAX_K, "gmm_estep_workspace: k = %d (1 .. %d)", k, GM_MAX_K);
    *bytes = e_ws_bytes(n, c, e);
    return GRIP_OK;
}

extern "C" int grip_gmm_estep(const float* feats, const float* mean, const float* var, const float* probs, const int32_t* idx, const float* sim,
                              const float* z_in, float lam, int z_iters, int n, int c, int e, int k, float* z_out, int32_t* argmax_out, void* workspace,
                              size_t workspace_bytes, void* stream) {
    RUNC(check_dims("gmm_estep", n, c, e));
    GRIP_REQUIRE(k >= 1 && k <= GM_MAX_K, "gmm_estep: k = %d (1 .. %d)", k, GM_MAX_K);
    GRIP_REQUIRE(lam >= 0.f && lam <= FLT_MAX, "gmm_estep: lam = %g (a finite lam >= 0)", (double)lam);
    GRIP_REQUIRE(z_iters >= 1, "gmm_estep: z_iters = %d (at least 1)", z_iters);
    GRIP_REQUIRE(feats && mean && var && probs && idx && sim && z_in && z_out && workspace, "gmm_estep: null pointer");
    GRIP_REQUIRE(aligned16(feats) && aligned16(mean) && aligned16(var), "gmm_estep: feats, mean and var must be 16-byte aligned");
    const size_t zb = (size_t)n * c * 4;
    GRIP_REQUIRE(!overlap(z_out, zb, z_in, zb) && !overlap(z_out, zb, probs, zb), "gmm_estep: z_out must not alias z_in or probs");
    GRIP_REQUIRE(workspace_bytes >= e_ws_bytes(n, c, e), "gmm_estep: workspace too small (%zu bytes, grip_gmm_estep_workspace says %zu)", workspace_bytes,
                 e_ws_bytes(n, c, e));
    hipStream_t s = (hipStream_t)stream;
    float* w = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* bias = w + pad64((size_t)c * e);
    float* g = bias + pad64((size_t)c);
    float* zt = g + pad64((size_t)n * c);
    hipLaunchKernelGGL(gmm_prep_kernel, dim3((c + 3) / 4), dim3(256), 0, s, mean, var, c, e, w, bias);
    GRIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(gmm_score_kernel, dim3((n + GM_BM - 1) / GM_BM), dim3(256), 0, s, feats, w, bias, probs, lam, n, c, e, g);
    GRIP_CHECK_HIP(hipGetLastError());
    const float* src = z_in;
    for (int t = 0; t < z_iters; ++t) {
        float* dst = ((z_iters - 1 - t) & 1) ? zt : z_out;      // the last sweep writes z_out
        int32_t* am = t == z_iters - 1 ? argmax_out : (int32_t*)nullptr;
        if (c <= 64)
            hipLaunchKernelGGL(gmm_sweep_kernel<1>, dim3((n + 3) / 4), dim3(256), 0, s, g, src, idx, sim, n, c, k, dst, am);
        else if (c <= GM_REG_C)
            hipLaunchKernelGGL(gmm_sweep_kernel<2>, dim3((n + 3) / 4), dim3(256), 0, s, g, src, idx, sim, n, c, k, dst, am);
        else
            hipLaunchKernelGGL(gmm_sweep_kernel<0>, dim3((n + 3) / 4), dim3(256), 0, s, g, src, idx, sim, n, c, k, dst, am);
        GRIP_CHECK_HIP(hipGetLastError());
        src = dst;
    }
    return GRIP_OK;
}
