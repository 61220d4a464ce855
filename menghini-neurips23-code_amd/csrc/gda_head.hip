// Gaussian discriminant head (after "A Hard-to-Beat Baseline for Training-free CLIP-based Adaptation", Wang et al., ICLR 2024 -- the model is the one of
// include/grip_amd.h, not that code): class means and ONE shared full covariance of the unit image embeddings give a linear classifier
// w_c = A^-1 mu_c that is added to the CLIP logits.  All f32 / int32, no atomics, every sum in a fixed order, no library math.
//   * grip_class_scatter: S = sum_i r_i (F_i - mu_{y_i}) (F_i - mu_{y_i})^T, a SYRK whose long dimension is n, on v_mfma_f32_16x16x4_f32.
//       - gda_scatter_kernel: a workgroup owns one 64 x 64 tile of the LOWER triangle of tiles and one K-slice of the rows; a wave 16 x 64 of it in four
//         accumulators, four rows per step.  Both operands come straight from memory in MFMA layout and are centred in the load path: a lane reads its
//         row's label, subtracts that class's mean (d = fl(F - mu), ONE rounding) and feeds r_i d_ia on the A side, d_ib on the B side.  Rows >= n, rows
//         with a label outside 0 .. c - 1 or a weight of 0, and columns >= e are zeros and are never loaded.  The rows are cut into chunks of GD_ROWS (a
//         constant) and the chunks into at most GD_SLICES contiguous K-slices of ceil(chunks / GD_SLICES) chunks: a slice is ONE chain over its rows in
//         ascending order, its [e, e] partial goes to the workspace (GD_SLICES e^2 floats at most, whatever n is).
//       - gda_scatter_final_kernel adds the slices in ascending order for every element a >= b and writes it to (a, b) AND (b, a): S is bit-symmetric
//         because only one triangle is ever computed (r d_a d_b and r d_b d_a round differently; the upper halves of the diagonal tiles are dropped).
//   * grip_spd_solve: M = a_scale a + ridge_rel a_scale tr(a) / e I, M = L L^T by blocked RIGHT-LOOKING Cholesky (panels of GS_NB = 64 columns, the last
//     one ragged) on the plain VALU, the right-hand sides appended as extra rows under the matrix so that the forward substitution rides along.
//       - gda_form_kernel writes the lower triangle of M and the c rows of rhs to the working matrix [e + c, e] (the trace is added by every workgroup
//         for itself in one fixed order: 256 strided partial sums, then those in ascending order) and clears info.
//       - gda_panel_kernel, ONE launch per panel: every workgroup factors the panel's diagonal block for itself (64 x 64, staged in LDS, factored in
//         the registers of one wave with v_readlane broadcasts: redundant and cheap, it is what removes any wait between workgroups), solves the rows
//         of the panel it needs against it (a thread per row, the row in registers, forward substitution with a true division) and either writes them
//         to the factor (the panel writers, blockIdx.y == the number of column tiles) or subtracts their product from its 64 x 64 tile of the trailing
//         matrix.  A launch reads the panel's columns of the working matrix and writes only columns
//         right of them and the factor buffer, so no workgroup reads what another one writes.
//       - gda_back_kernel: a workgroup per right-hand side solves L^T x = y from the last block of 64 to the first: the block's triangle in one wave
//         (lane = unknown, values passed by ds_bpermute), then y_j -= sum_k L[k, j] x_k for the columns left of it, k descending, all threads.
//       - gda_factor_copy_kernel (factor_out given): the lower triangle of L, zeros above.
//     A pivot that is not > 0 sets info = index + 1 (the first one wins); nothing loops on data, so the call returns whatever the matrix holds.
//   * grip_linear_head: logits[i, c] = base[i, c] + alpha ((f_i . w_c) / |f_i| - bias_c) on the main loop of gmm_score_kernel / knn_graph_kernel (64 rows
//     per workgroup, the classes 64 at a time, e staged 32 floats per step through two XOR-swizzled LDS buffers, the loads of step t + 1 in flight under
//     the MFMAs of step t; the chain over e ascending).  The row's sum of squares is accumulated ON CHIP from the same LDS fragments during the first
//     class tile (a lane adds its eight floats of a stage in ascending order, the four lanes of a row are then added as (l0 + l1) + (l2 + l3)); the
//     epilogue is score * (1 / sqrt(ss)) - bias, times alpha, plus base, then the first arg-max.  The [n, c] product never reaches memory on its own.
//     A row's bits depend on that row, w and bias alone.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {
constexpr int GD_ROWS = 256;                      // rows per chunk of the scatter (engine.GDA_SCATTER_ROWS)
constexpr int GD_SLICES = 16;                     // K-slices of the scatter at most (engine.GDA_SCATTER_SLICES)
constexpr int GD_T = 64;                          // tile of the scatter
constexpr int GD_MAX_E = 1024;
constexpr int GS_NB = 64;                         // columns per Cholesky panel
constexpr int GS_P = GS_NB + 1;                   // LDS pitch of a 64 x 64 block (a thread walks a row: conflict-free)
constexpr int LH_BM = 64;                         // rows per workgroup of gda_head_kernel (16 per wave)
constexpr int LH_BN = 64;                         // classes per tile
constexpr int LH_BK = 32;                         // floats of e per stage (one 128-byte line per row)
constexpr int LH_STAGE = (LH_BM + LH_BN) * LH_BK; // floats per stage = 16 KiB

// ---------------------------------------------------------------------------------------------------------------- scatter
// grid (lower tile pairs, slices): part[slice, a, b] = sum over the slice's rows of r_i d_ia d_ib for the tile's (a, b)
__global__ __launch_bounds__(256) void gda_scatter_kernel(const float* __restrict__ f, const int32_t* __restrict__ labels, const float* __restrict__ rw,
                                                          const float* __restrict__ mean, int n, int c, int e, int per, float* __restrict__ part) {
    const int lane = threadIdx.x & 63, frow = lane & 15, fgrp = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // tile pair p -> (ta, tb), tb <= ta: p = ta (ta + 1) / 2 + tb
    int ta = 0;
    {
        const int p = blockIdx.x;
        while ((ta + 1) * (ta + 2) / 2 <= p) ++ta;
    }
    const int tb = blockIdx.x - ta * (ta + 1) / 2;
    const int a0 = ta * GD_T + wave * 16, b0 = tb * GD_T;
    if (a0 >= e) return;        // per wave (the kernel has no barrier)
    const int r0 = blockIdx.y * per * GD_ROWS, r1 = (int)min((int64_t)n, (int64_t)r0 + (int64_t)per * GD_ROWS);
    const int acol = a0 + frow, bcol = b0 + frow * 4;
    const bool a_ok = acol < e, b_ok = bcol < e;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[4] = {zero, zero, zero, zero};
    // lane (frow, fgrp) of step r: r_i d[r + fgrp, a0 + frow] (A: column a x row) and d[r + fgrp, b0 + frow * 4 + j] (B of MFMA j: row x column b)
    // Sixteen rows per trip, as four steps of four: the labels and weights of all four steps are loaded first, then the operands, then the MFMAs in step
    // order -- the loads of a trip do not wait for each other (a step's chain label -> mean -> MFMA would otherwise be paid once per four rows).
    for (int r = r0; r < r1; r += 16) {
        int y[4];
        float w[4], fa[4], ma[4];
        f32x4 fb[4], mb[4];
        bool ok[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = r + s * 4 + fgrp;
            y[s] = row < r1 ? labels[row] : -1;
            w[s] = (row < r1 && rw) ? rw[row] : 1.0f;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = r + s * 4 + fgrp;
            ok[s] = y[s] >= 0 && y[s] < c && w[s] != 0.f;
            const float* fr = f + (size_t)row * e;
            const float* mr = mean + (size_t)(ok[s] ? y[s] : 0) * e;
            fa[s] = (ok[s] && a_ok) ? fr[acol] : 0.f;
            ma[s] = (ok[s] && a_ok) ? mr[acol] : 0.f;
            fb[s] = (ok[s] && b_ok) ? *(const f32x4*)(fr + bcol) : zero;
            mb[s] = (ok[s] && b_ok) ? *(const f32x4*)(mr + bcol) : zero;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float a = ok[s] ? w[s] * (fa[s] - ma[s]) : 0.f;
            const f32x4 b = fb[s] - mb[s];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[j], acc[j], 0, 0, 0);
        }
    }
    // the lane holds rows a0 + fgrp * 4 + {0..3} of columns b0 + frow * 4 + {j}
    float* out = part + (size_t)blockIdx.y * e * e;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ar = a0 + fgrp * 4 + q;
        if (ar < e && b_ok) *(f32x4*)(out + (size_t)ar * e + bcol) = (f32x4){acc[0][q], acc[1][q], acc[2][q], acc[3][q]};
    }
}

// a thread per element a >= b: the slices in ascending order, written to (a, b) and (b, a)
__global__ __launch_bounds__(256) void gda_scatter_final_kernel(const float* __restrict__ part, int slices, int e, float* __restrict__ s_out) {
    const int b = blockIdx.x * 64 + (threadIdx.x & 63), a = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (a >= e || b > a) return;
    float s = 0.f;
    for (int q = 0; q < slices; ++q) s += part[((size_t)q * e + a) * e + b];
    s_out[(size_t)a * e + b] = s;
    s_out[(size_t)b * e + a] = s;
}

// ---------------------------------------------------------------------------------------------------------------- SPD solve
// wk [e + c, e]: the lower triangle of M and the rows of rhs
__global__ __launch_bounds__(256) void gda_form_kernel(const float* __restrict__ a, float a_scale, float ridge_rel, const float* __restrict__ rhs, int e, int c,
                                                       float* __restrict__ wk, int32_t* __restrict__ info) {
    __shared__ float part[256];
    const int tid = threadIdx.x;
    float s = 0.f;
    for (int i = tid; i < e; i += 256) s += a[(size_t)i * e + i];
    part[tid] = s;
    __syncthreads();
    float tr = 0.f;
    for (int q = 0; q < 256; ++q) tr += part[q];       // (LDS broadcast reads: every thread adds the same chain)
    const float shift = ((ridge_rel * a_scale) * tr) / (float)e;
    if (blockIdx.x == 0 && tid == 0) *info = 0;
    const int row = blockIdx.x;
    if (row < e) {
        for (int j = tid; j <= row; j += 256) {
            const float v = a[(size_t)row * e + j];
            wk[(size_t)row * e + j] = j == row ? fmaf(a_scale, v, shift) : a_scale * v;
        }
    } else {
        for (int j = tid; j < e; j += 256) wk[(size_t)row * e + j] = rhs[(size_t)(row - e) * e + j];
    }
}

// Panel k0 .. k0 + nb - 1 of the factorisation.  Rows below the panel: k1 = k0 + nb .. R - 1 (R = e + c), in tiles of 64 from k1; trailing columns
// k1 .. e - 1 in tiles of 64 from k1 (nct of them).  grid (row tiles, nct + 1): y < nct updates tile (x, y) of the trailing matrix (y <= x: the lower
// triangle; the right-hand-side rows need every column tile and lie in row tiles >= nct - 1), y == nct writes rows x of the panel to the factor.
__global__ __launch_bounds__(256) void gda_panel_kernel(float* __restrict__ wk, float* __restrict__ lf, int e, int R, int k0, int nb, int nct,
                                                        int32_t* __restrict__ info) {
    __shared__ float D[GS_NB * GS_P], Pi[GS_NB * GS_P], Pj[GS_NB * GS_P];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ti = blockIdx.x, tj = blockIdx.y;
    const bool writer = tj == nct;
    if (!writer && tj > ti) return;     // per workgroup, before any barrier
    const int k1 = k0 + nb;
    const int ri0 = k1 + ti * GS_NB, rj0 = k1 + tj * GS_NB;
    const bool twin = !writer && ti == tj;
    // the diagonal block (lower triangle, zeros elsewhere), the panel rows of tile i and (updaters off the diagonal) of the rows that are tile j's columns
    for (int id = tid; id < GS_NB * GS_NB; id += 256) {
        const int r = id >> 6, q = id & 63;
        D[r * GS_P + q] = (r < nb && q <= r) ? wk[(size_t)(k0 + r) * e + k0 + q] : (r >= nb && q == r ? 1.f : 0.f);      // (a ragged panel: identity below)
        Pi[r * GS_P + q] = (ri0 + r < R && q < nb) ? wk[(size_t)(ri0 + r) * e + k0 + q] : 0.f;
        if (!writer && !twin) Pj[r * GS_P + q] = (rj0 + r < e && q < nb) ? wk[(size_t)(rj0 + r) * e + k0 + q] : 0.f;
    }
    __syncthreads();
    // Cholesky of D, column by column, in the registers of wave 0: lane r holds row r, the pivot and the column entries L[q, t] of the other rows come
    // by v_readlane (the lane index is a constant of the unrolled loops), so the 64 steps need no barrier and no LDS.  Step t: L[r, t] = D[r, t] / d,
    // d = sqrt(D[t, t]); D[r, q] -= L[r, t] L[q, t] for q > t (the rows r > t; what this leaves above the diagonal is dropped when the rows go back).
    int bad = 0;
    if (wave == 0) {
        const int lane = tid & 63;
        float dr[GS_NB];
#pragma unroll
        for (int q = 0; q < GS_NB; ++q) dr[q] = D[lane * GS_P + q];
#pragma unroll
        for (int t = 0; t < GS_NB; ++t) {
            const float p = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dr[t]), t));
            if (t < nb && bad == 0 && !(p > 0.f)) bad = k0 + t + 1;
            const float d = sqrtf(p);
            const float l = dr[t] / d;
            dr[t] = lane == t ? d : l;
            const float lr = lane > t ? l : 0.f;
#pragma unroll
            for (int q = t + 1; q < GS_NB; ++q) {
                const float lq = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dr[t]), q));
                dr[q] = fmaf(-lr, lq, dr[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < GS_NB; ++q) D[lane * GS_P + q] = q <= lane ? dr[q] : 0.f;
    }
    __syncthreads();
    // the panel rows against D^T: thread r < 64 owns row r of Pi, thread 64 + r row r of Pj
    // (per wave: waves 0 and 1.  The row lives in registers and both loops are unrolled over the full 64 columns -- the LDS reads of D are then
    // independent broadcasts that the scheduler issues ahead of the fmaf chain; with a ragged panel the columns >= nb are zeros against an identity)
    if (wave == 0 || (wave == 1 && !writer && !twin)) {
        float* pr = (wave == 0 ? Pi : Pj) + (tid & 63) * GS_P;
        float x[GS_NB];
#pragma unroll
        for (int t = 0; t < GS_NB; ++t) x[t] = pr[t];
#pragma unroll
        for (int t = 0; t < GS_NB; ++t) {
            float s = x[t];
#pragma unroll
            for (int q = 0; q < t; ++q) s = fmaf(-x[q], D[t * GS_P + q], s);
            x[t] = s / D[t * GS_P + t];
        }
#pragma unroll
        for (int t = 0; t < GS_NB; ++t) pr[t] = x[t];
    }
    __syncthreads();
    if (writer) {
        for (int id = tid; id < GS_NB * GS_NB; id += 256) {
            const int r = id >> 6, q = id & 63;
            if (q >= nb) continue;
            if (ri0 + r < R) lf[(size_t)(ri0 + r) * e + k0 + q] = Pi[r * GS_P + q];
            if (ti == 0 && r < nb && q <= r) lf[(size_t)(k0 + r) * e + k0 + q] = D[r * GS_P + q];
        }
        if (ti == 0 && tid == 0 && bad != 0 && *info == 0) *info = bad;
        return;
    }
    // wk[row, col] -= sum_q Pi[row, q] Pj[col, q], q ascending; thread (ty, tx) owns rows ty + 16 a, columns tx + 16 b
    const float* PJ = twin ? Pi : Pj;
    const int ty = tid >> 4, tx = tid & 15;
    float v[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int gr = ri0 + ty + 16 * a, gc = rj0 + tx + 16 * b;
            v[a][b] = (gr < R && gc < e && gc <= gr) ? wk[(size_t)gr * e + gc] : 0.f;
        }
    for (int q = 0; q < nb; ++q) {
        float pa[4], pb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) pa[a] = Pi[(ty + 16 * a) * GS_P + q];
#pragma unroll
        for (int b = 0; b < 4; ++b) pb[b] = PJ[(tx + 16 * b) * GS_P + q];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) v[a][b] = fmaf(-pa[a], pb[b], v[a][b]);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int gr = ri0 + ty + 16 * a, gc = rj0 + tx + 16 * b;
            if (gr < R && gc < e && gc <= gr) wk[(size_t)gr * e + gc] = v[a][b];
        }
}

// a workgroup per right-hand side: L^T x = y, y = row e + cls of the factor buffer
__global__ __launch_bounds__(256) void gda_back_kernel(const float* __restrict__ lf, int e, float* __restrict__ x_out) {
    __shared__ float y[GD_MAX_E];
    __shared__ float Lb[GS_NB * GS_P];
    const int tid = threadIdx.x, lane = tid & 63;
    const int cls = blockIdx.x;
    for (int j = tid; j < e; j += 256) y[j] = lf[(size_t)(e + cls) * e + j];
    __syncthreads();
    const int nblk = (e + GS_NB - 1) / GS_NB;
    for (int bl = nblk - 1; bl >= 0; --bl) {
        const int b0 = bl * GS_NB, nb = min(GS_NB, e - b0);
        for (int id = tid; id < GS_NB * GS_NB; id += 256) {
            const int r = id >> 6, q = id & 63;
            Lb[r * GS_P + q] = (r < nb && q <= r) ? lf[(size_t)(b0 + r) * e + b0 + q] : 0.f;
        }
        __syncthreads();
        if (tid < 64) {
            // lane l holds unknown b0 + l: x_t = y_t / L[t, t], then y_l -= L[t, l] x_t for l < t, t descending
            float v = lane < nb ? y[b0 + lane] : 0.f;
            for (int t = nb - 1; t >= 0; --t) {
                const float xt = __shfl(v, t) / Lb[t * GS_P + t];
                if (lane == t) v = xt;
                else if (lane < t) v = fmaf(-Lb[t * GS_P + lane], xt, v);
            }
            if (lane < nb) y[b0 + lane] = v;
        }
        __syncthreads();
        for (int j = tid; j < b0; j += 256) {
            float v = y[j];
#pragma unroll 8
            for (int t = nb - 1; t >= 0; --t) v = fmaf(-lf[(size_t)(b0 + t) * e + j], y[b0 + t], v);
            y[j] = v;
        }
        __syncthreads();
    }
    for (int j = tid; j < e; j += 256) x_out[(size_t)cls * e + j] = y[j];
}

__global__ __launch_bounds__(256) void gda_factor_copy_kernel(const float* __restrict__ lf, int e, float* __restrict__ out) {
    const int row = blockIdx.x;
    for (int j = threadIdx.x; j < e; j += 256) out[(size_t)row * e + j] = j <= row ? lf[(size_t)row * e + j] : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- linear head
// out[i, cls] = base[i, cls] + alpha ((f_i . w_cls) rn_i - bias[cls]), rn_i = 1 / sqrt(sum_d f_id^2); argmax (optional): first index of the row's maximum
__global__ __launch_bounds__(256) void gda_head_kernel(const float* __restrict__ q, const float* __restrict__ wgt, const float* __restrict__ bias, float alpha,
                                                       const float* base, int n, int m, int e, float* out, int32_t* __restrict__ argmax) {
    __shared__ __attribute__((aligned(16))) float lds[2 * LH_STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int r0 = blockIdx.x * LH_BM;
    const int nec = (e + LH_BK - 1) / LH_BK, nkt = (m + LH_BN - 1) / LH_BN;
    const int T = nkt * nec;

    // staging: thread t moves the 16-byte pieces t and t + 256 of the 64 x 32 row tile and of the class tile; the piece index within a row is XOR-swizzled
    // with (row & 7), so the fragment reads below are conflict-free.  Rows >= n, classes >= m and columns >= e are zeros.
    f32x4 fr[2], kr[2];
    auto gload = [&](int kt, int ec) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, col = ec * LH_BK + (id & 7) * 4;
            const int gr = r0 + row, gk = kt * LH_BN + row;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            fr[i] = (gr < n && col < e) ? *(const f32x4*)(q + (size_t)gr * e + col) : zero;
            kr[i] = (gk < m && col < e) ? *(const f32x4*)(wgt + (size_t)gk * e + col) : zero;
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            // each sixteen floats of a row are stored TRANSPOSED as 4 x 4 (float 4 s + g goes to chunk g, slot s): the MFMA of step s contracts the floats
            // 4 s .. 4 s + 3, so the chain over e is ASCENDING
            const int id = tid + 256 * i, row = id >> 3, kk = (id & 7) >> 2, sp = id & 3;
            float* st = lds + buf * LH_STAGE + row * LH_BK + sp;
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const int ch = (kk * 4 + gg) ^ (row & 7);
                st[ch * 4] = fr[i][gg];
                st[LH_BM * LH_BK + ch * 4] = kr[i][gg];
            }
        }
    };

    int a_off[2], b_off[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int chunk = (kk * 4 + fgrp) ^ (lane & 7);
        a_off[kk] = (wave * 16 + frow) * LH_BK + chunk * 4;
        b_off[kk] = LH_BM * LH_BK + frow * LH_BK + chunk * 4;
    }
    const int my_row = r0 + wave * 16 + frow;
    const bool row_ok = my_row < n;

    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float ss = 0.f, rn = 0.f, bv = 0.f;
    int bi = INT_MAX;

    gload(0, 0);
    sstore(0);
    __syncthreads();
    int kt = 0, ec = 0;
    for (int t = 0; t < T; ++t) {
        const int buf = t & 1;
        int nkt_ = kt, nec_ = ec + 1;
        if (nec_ == nec) { nec_ = 0; ++nkt_; }
        if (t + 1 < T) gload(nkt_, nec_);
        const float* st = lds + buf * LH_STAGE;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f32x4 bf[4];
            const f32x4 af = *(const f32x4*)(st + a_off[kk]);
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = *(const f32x4*)(st + b_off[kk] + j * 16 * LH_BK);
            // the lane's floats kk * 16 + 4 s + fgrp of the row, s ascending (first class tile only: the row is staged again for every tile)
            if (kt == 0) {
#pragma unroll
                for (int s = 0; s < 4; ++s) ss = fmaf(af[s], af[s], ss);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][s], af[s], acc[j], 0, 0, 0);
        }
        if (t + 1 < T) sstore(buf ^ 1);
        if (ec == nec - 1) {
            if (kt == 0) {
                // the four lanes (frow, 0..3) of a row: (l0 + l1) + (l2 + l3) in every one of them
                ss += __shfl_xor(ss, 16);
                ss += __shfl_xor(ss, 32);
                rn = 1.0f / sqrtf(ss);
            }
            // lane (frow, fgrp) holds the scores of row wave*16 + frow against classes kt*64 + j*16 + fgrp*4 + {0..3}
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int cls = kt * LH_BN + j * 16 + fgrp * 4 + r;
                    if (row_ok && cls < m) {
                        const size_t o = (size_t)my_row * m + cls;
                        float v = alpha * (acc[j][r] * rn - bias[cls]);
                        if (base) v = base[o] + v;
                        out[o] = v;
                        if (bi == INT_MAX || v > bv) { bv = v; bi = cls; }
                    }
                }
                acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
        kt = nkt_;
        ec = nec_;
        __syncthreads();
    }
    if (argmax) {
        // the row's four lanes: the larger value, the lower class where neither is larger (a tie; a row of NaNs, the zero row's, ends at class 0); a lane
        // without a class (INT_MAX) loses
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (!(bv > ov) && oi < bi))) {
                bv = ov;
                bi = oi;
            }
        }
        if (row_ok && fgrp == 0) argmax[my_row] = bi;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}
size_t pad64(size_t floats) { return (floats + 63) / 64 * 64; }

int check_e(const char* who, int e) {
    GRIP_REQUIRE(e > 0 && e % 4 == 0 && e <= GD_MAX_E, "%s: e = %d (a multiple of 4, 4 .. %d)", who, e, GD_MAX_E);
    return GRIP_OK;
}
// the K-slices of n rows: `per` chunks of GD_ROWS rows each, `slices` of them
void scatter_split(int n, int* per, int* slices) {
    const int nch = (n + GD_ROWS - 1) / GD_ROWS;
    *per = (nch + GD_SLICES - 1) / GD_SLICES;
    *slices = (nch + *per - 1) / *per;
}
size_t scatter_ws_bytes(int n, int e) {
    int per, slices;
    scatter_split(n, &per, &slices);
    return (size_t)slices * e * e * sizeof(float) + 256;
}
size_t solve_ws_bytes(int e, int c) { return 2 * pad64((size_t)(e + c) * e) * sizeof(float) + 256; }
size_t head_ws_bytes() { return 256; }
}  // namespace

#define RUNC(x) do { int _rc = (x); if (_rc != GRIP_OK) return _rc; } while (0)

extern "C" int grip_class_scatter_workspace(int n, int c, int e, size_t* bytes) {
    GRIP_REQUIRE(bytes, "class_scatter_workspace: null pointer");
    GRIP_REQUIRE(n > 0 && c > 0, "class_scatter_workspace: n = %d, c = %d (each must be positive)", n, c);
    RUNC(check_e("class_scatter_workspace", e));
    *bytes = scatter_ws_bytes(n, e);
    return GRIP_OK;
}

extern "C" int grip_class_scatter(const float* feats, const int32_t* labels, const float* row_weight, const float* mean, int n, int c, int e,
                                  float* scatter_out, void* workspace, size_t workspace_bytes, void* stream) {
    GRIP_REQUIRE(n > 0 && c > 0, "class_scatter: n = %d, c = %d (each must be positive)", n, c);
    RUNC(check_e("class_scatter", e));
    GRIP_REQUIRE((int64_t)c * e <= INT_MAX && n <= INT_MAX - GD_ROWS, "class_scatter: n = %d, c = %d, e = %d (c e and n + %d must stay below 2^31)", n, c, e,
                 GD_ROWS);
    GRIP_REQUIRE(feats && labels && mean && scatter_out && workspace, "class_scatter: null pointer");
    GRIP_REQUIRE(aligned16(feats) && aligned16(mean), "class_scatter: feats and mean must be 16-byte aligned");
    const size_t sb = (size_t)e * e * 4;
    GRIP_REQUIRE(!overlap(scatter_out, sb, feats, (size_t)n * e * 4) && !overlap(scatter_out, sb, mean, (size_t)c * e * 4) &&
                     !overlap(scatter_out, sb, labels, (size_t)n * 4) && !(row_weight && overlap(scatter_out, sb, row_weight, (size_t)n * 4)),
                 "class_scatter: scatter_out must not alias an input");
    GRIP_REQUIRE(workspace_bytes >= scatter_ws_bytes(n, e), "class_scatter: workspace too small (%zu bytes, grip_class_scatter_workspace says %zu)",
                 workspace_bytes, scatter_ws_bytes(n, e));
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    int per, slices;
    scatter_split(n, &per, &slices);
    const int nt = (e + GD_T - 1) / GD_T;
    hipLaunchKernelGGL(gda_scatter_kernel, dim3(nt * (nt + 1) / 2, slices), dim3(256), 0, s, feats, labels, row_weight, mean, n, c, e, per, part);
    GRIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(gda_scatter_final_kernel, dim3((e + 63) / 64, (e + 3) / 4), dim3(256), 0, s, part, slices, e, scatter_out);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}

extern "C" int grip_spd_solve_workspace(int e, int c, size_t* bytes) {
    GRIP_REQUIRE(bytes, "spd_solve_workspace: null pointer");
    GRIP_REQUIRE(c > 0, "spd_solve_workspace: c = %d (must be positive)", c);
    RUNC(check_e("spd_solve_workspace", e));
    GRIP_REQUIRE((int64_t)(e + (int64_t)c) * e <= INT_MAX, "spd_solve_workspace: e = %d, c = %d ((e + c) e must stay below 2^31)", e, c);
    *bytes = solve_ws_bytes(e, c);
    return GRIP_OK;
}

extern "C" int grip_spd_solve(const float* a, float a_scale, float ridge_rel, const float* rhs, int e, int c, float* x_out, float* factor_out,
                              int32_t* info_out, void* workspace, size_t workspace_bytes, void* stream) {
    GRIP_REQUIRE(c > 0, "spd_solve: c = %d (must be positive)", c);
    RUNC(check_e("spd_solve", e));
    GRIP_REQUIRE((int64_t)(e + (int64_t)c) * e <= INT_MAX, "spd_solve: e = %d, c = %d ((e + c) e must stay below 2^31)", e, c);
    GRIP_REQUIRE(a_scale > 0.f && a_scale <= FLT_MAX, "spd_solve: a_scale = %g (a finite a_scale > 0)", (double)a_scale);
    GRIP_REQUIRE(ridge_rel >= 0.f && ridge_rel <= FLT_MAX, "spd_solve: ridge_rel = %g (a finite ridge_rel >= 0)", (double)ridge_rel);
    GRIP_REQUIRE(a && rhs && x_out && info_out && workspace, "spd_solve: null pointer");
    const size_t ab = (size_t)e * e * 4, xb = (size_t)c * e * 4;
    GRIP_REQUIRE(!overlap(x_out, xb, a, ab) && !(factor_out && (overlap(factor_out, ab, a, ab) || overlap(factor_out, ab, rhs, xb) ||
                                                                overlap(factor_out, ab, x_out, xb))),
                 "spd_solve: x_out must not alias a, and factor_out no other operand");
    GRIP_REQUIRE(workspace_bytes >= solve_ws_bytes(e, c), "spd_solve: workspace too small (%zu bytes, grip_spd_solve_workspace says %zu)", workspace_bytes,
                 solve_ws_bytes(e, c));
    hipStream_t s = (hipStream_t)stream;
    float* wk = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* lf = wk + pad64((size_t)(e + c) * e);
    const int R = e + c;
    hipLaunchKernelGGL(gda_form_kernel, dim3(R), dim3(256), 0, s, a, a_scale, ridge_rel, rhs, e, c, wk, info_out);
    GRIP_CHECK_HIP(hipGetLastError());
    for (int k0 = 0; k0 < e; k0 += GS_NB) {
        const int nb = std::min(GS_NB, e - k0), k1 = k0 + nb;
        const int nrt = (R - k1 + GS_NB - 1) / GS_NB, nct = (e - k1 + GS_NB - 1) / GS_NB;
        hipLaunchKernelGGL(gda_panel_kernel, dim3(nrt, nct + 1), dim3(256), 0, s, wk, lf, e, R, k0, nb, nct, info_out);
        GRIP_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(gda_back_kernel, dim3(c), dim3(256), 0, s, lf, e, x_out);
    GRIP_CHECK_HIP(hipGetLastError());
    if (factor_out) {
        hipLaunchKernelGGL(gda_factor_copy_kernel, dim3(e), dim3(256), 0, s, lf, e, factor_out);
        GRIP_CHECK_HIP(hipGetLastError());
    }
    return GRIP_OK;
}

extern "C" int grip_linear_head_workspace(int n, int c, int e, size_t* bytes) {
    GRIP_REQUIRE(bytes, "linear_head_workspace: null pointer");
    GRIP_REQUIRE(n > 0 && c > 0, "linear_head_workspace: n = %d, c = %d (each must be positive)", n, c);
    RUNC(check_e("linear_head_workspace", e));
    *bytes = head_ws_bytes();
    return GRIP_OK;
}

extern "C" int grip_linear_head(const float* img_emb, const float* w, const float* bias, float alpha, const float* base_logits, int n, int c, int e,
                                float* logits_out, int32_t* argmax_out, void* workspace, size_t workspace_bytes, void* stream) {
    GRIP_REQUIRE(n > 0 && c > 0, "linear_head: n = %d, c = %d (each must be positive)", n, c);
    RUNC(check_e("linear_head", e));
    GRIP_REQUIRE((int64_t)c * e <= INT_MAX && ((int64_t)n + LH_BM - 1) / LH_BM <= INT_MAX, "linear_head: n = %d, c = %d, e = %d (c e must stay below 2^31)", n, c,
                 e);
    GRIP_REQUIRE(alpha == alpha && fabsf(alpha) <= FLT_MAX, "linear_head: alpha = %g (must be finite)", (double)alpha);
    GRIP_REQUIRE(img_emb && w && bias && logits_out && workspace, "linear_head: null pointer");
    GRIP_REQUIRE(aligned16(img_emb) && aligned16(w), "linear_head: img_emb and w must be 16-byte aligned");
    const size_t lb = (size_t)n * c * 4;
    GRIP_REQUIRE(!base_logits || base_logits == logits_out || !overlap(logits_out, lb, base_logits, lb),
                 "linear_head: logits_out may BE base_logits, but must not overlap it otherwise");
    GRIP_REQUIRE(!overlap(logits_out, lb, img_emb, (size_t)n * e * 4) && !overlap(logits_out, lb, w, (size_t)c * e * 4) &&
                     !overlap(logits_out, lb, bias, (size_t)c * 4),
                 "linear_head: logits_out must not alias img_emb, w or bias");
    GRIP_REQUIRE(workspace_bytes >= head_ws_bytes(), "linear_head: workspace too small (%zu bytes, grip_linear_head_workspace says %zu)", workspace_bytes,
                 head_ws_bytes());
    hipLaunchKernelGGL(gda_head_kernel, dim3((n + LH_BM - 1) / LH_BM), dim3(256), 0, (hipStream_t)stream, img_emb, w, bias, alpha, base_logits, n, c, e,
                       logits_out, argmax_out);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}
