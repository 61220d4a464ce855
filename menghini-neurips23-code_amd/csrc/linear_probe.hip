// Trained linear probe on the cached unit image embeddings (the "linear probe" of the CLIP / CoOp papers, text-initialised as in LP++ -- the model is
// the one of include/grip_amd.h, not that code): a zero-initialised residual on the CLIP logits, x_ic = base_ic + s (u_i . W_c) + b_c, trained by
// full-batch heavy-ball descent on a weighted soft/hard cross-entropy plus a ridge.  All f32 / int32, no atomics, every sum in a fixed order.
// The TWO-KERNEL form: the [c, e] accumulators of a fused form would need c e / 256 VGPRs per lane of a workgroup (204 at 102 x 512) or
// a K-split over e that re-reads the logits; writing the scaled residuals g [n, c] once costs n c floats against the n e of feats.
//   * probe_score_kernel: a workgroup owns PB_BM = 32 rows.  Scores on v_mfma_f32_16x16x4_f32 with the main loop of gda_head_kernel (e staged 32 floats
//     per step through two XOR-swizzled LDS buffers, the loads of step t + 1 in flight under the MFMAs of step t, the chain over e ascending); up to
//     four 64-class tiles ride on one staging of the rows (c <= 256: feats is read ONCE; above that one tile per pass and the row tile, 4 KiB a step, comes
//     again from the cache for each).  Wave (wr, wc) owns rows 16 wr .. 16 wr + 15 and the class sixteens 2 wc, 2 wc + 1 of every tile.  The logits
//     x = base + fmaf(s, score, b) go to LDS ([32, c] floats) and never to memory; then eight lanes per row: the row maximum, t . x, T (ascending c, every
//     lane the same chain), exp(x - max) in place and its sum (a lane's classes k = lane, lane + 8, .. ascending, then a three-step xor butterfly: the same
//     bits in all eight), lse = max + logf(sum).  g = r (T e_c / sum - t_c) is written ONCE to the workspace (zeros for the rows that do not contribute),
//     the workgroup's loss (its rows in ascending order) to one float.
//   * probe_contract_kernel: part[slice, c, d] = sum over the slice's rows of g_ic u_id, the transposed contraction, as gda_scatter_kernel does its SYRK:
//     a workgroup owns 128 classes x 64 columns and ONE contiguous K-slice of the rows, a wave 32 classes x 64 columns in eight accumulators, both
//     operands straight from memory in MFMA layout, sixteen rows a trip.  The rows are cut into chunks of PB_ROWS = 64 and the chunks into at most
//     slice_cap(c, e) contiguous slices of ceil(chunks / cap) chunks: a function of (n, c, e) alone.  The workgroups of column tile 0 also add their
//     lanes' g values (grad_b's partials: a lane's rows ascending, the four lanes of a class as (l0 + l1) + (l2 + l3)).  Rows that do not contribute
//     are never loaded.
//   * probe_final_kernel / probe_update_kernel: the slices in ascending order, times fl(norm scale) (grad_w) or norm (grad_b, loss; the loss partials
//     as 256 strided sums, then those in ascending order); the update kernel goes on with the heavy-ball step of include/grip_amd.h.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {
constexpr int PB_BM = 32;                         // rows per workgroup of probe_score_kernel (engine.PROBE_SCORE_ROWS)
constexpr int PB_BN = 64;                         // classes per tile
constexpr int PB_BK = 32;                         // floats of e per stage
constexpr int PB_MAXSUB = 4;                      // class tiles per staging of the rows at most
constexpr int PB_ROWS = 64;                       // rows per chunk of the contraction (engine.PROBE_ROWS)
constexpr int PB_CT = 128;                        // classes per workgroup of the contraction
constexpr int PB_ET = 64;                         // columns per workgroup of the contraction
constexpr int PB_MAX_E = 1024, PB_MAX_C = 1024;

__device__ __forceinline__ bool probe_row_ok(int y, float w, int c, bool has_soft) { return ((y >= 0 && y < c) || (y == -1 && has_soft)) && w != 0.f; }

// ---------------------------------------------------------------------------------------------------------------- scores + CE gradient
// dynamic LDS: two stages of (PB_BM + 64 nsub) x 32 floats | xs [PB_BM, xp] | y, r, sum, T, loss of the 32 rows
__global__ __launch_bounds__(256) void probe_score_kernel(const float* __restrict__ f, const float* __restrict__ wgt, const float* __restrict__ bias,
                                                          const float* __restrict__ base, const int32_t* __restrict__ labels, const float* __restrict__ soft,
                                                          const float* __restrict__ rw, float scale, int n, int c, int e, int nsub, int xp,
                                                          float* __restrict__ g, float* __restrict__ part_loss) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int stage = (PB_BM + PB_BN * nsub) * PB_BK;
    float* xs = lds + 2 * stage;
    int* s_y = (int*)(xs + PB_BM * xp);
    float* s_r = (float*)(s_y + PB_BM);
    float* s_sum = s_r + PB_BM;
    float* s_T = s_sum + PB_BM;
    float* s_loss = s_T + PB_BM;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave & 1, wc = wave >> 1;
    const int frow = lane & 15, fgrp = lane >> 4;
    const size_t r0 = (size_t)blockIdx.x * PB_BM;
    const int rows_here = (int)min((size_t)PB_BM, (size_t)n - r0);
    const int nec = (e + PB_BK - 1) / PB_BK, nkt = (c + PB_BN - 1) / PB_BN, nst = (nkt + nsub - 1) / nsub;
    const int T = nst * nec;

    // the rows' labels and weights: r = 0 marks a row that does not contribute (its features, base and soft rows are never read)
    if (tid < PB_BM) {
        int y = -2;
        float w = 0.f;
        if (tid < rows_here) {
            y = labels[r0 + tid];
            w = rw ? rw[r0 + tid] : 1.0f;
            if (!probe_row_ok(y, w, c, soft != nullptr)) w = 0.f;
        }
        s_y[tid] = y;
        s_r[tid] = w;
    }
    __syncthreads();
    const int srow = tid >> 3;      // the row this thread stages (and, below, one of the eight lanes that reduce it)
    const bool srow_ok = s_r[srow] != 0.f;

    f32x4 fr, kr[2 * PB_MAXSUB];
    auto gload = [&](int st, int ec) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const int col = ec * PB_BK + (tid & 7) * 4;
        fr = (srow_ok && col < e) ? *(const f32x4*)(f + (r0 + srow) * e + col) : zero;
#pragma unroll
        for (int i = 0; i < 2 * PB_MAXSUB; ++i)
            if (i < 2 * nsub) {
                const int gk = st * nsub * PB_BN + ((tid + 256 * i) >> 3);
                kr[i] = (gk < c && col < e) ? *(const f32x4*)(wgt + (size_t)gk * e + col) : zero;
            }
    };
    auto sstore = [&](int buf) {
        // each sixteen floats of a row are stored TRANSPOSED as 4 x 4 (float 4 s + g goes to chunk g, slot s): the MFMA of step s contracts the floats
        // 4 s .. 4 s + 3, so the chain over e is ASCENDING (gda_head_kernel's layout)
        const int kk = (tid & 7) >> 2, sp = tid & 3;
        float* sb = lds + buf * stage;
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) sb[srow * PB_BK + sp + (((kk * 4 + gg) ^ (srow & 7)) * 4)] = fr[gg];
#pragma unroll
        for (int i = 0; i < 2 * PB_MAXSUB; ++i)
            if (i < 2 * nsub) {
                const int row = (tid + 256 * i) >> 3;
                float* st = sb + (PB_BM + row) * PB_BK + sp;
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) st[((kk * 4 + gg) ^ (row & 7)) * 4] = kr[i][gg];
            }
    };

    int a_off[2], b_off[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int chunk = (kk * 4 + fgrp) ^ (lane & 7);
        a_off[kk] = (wr * 16 + frow) * PB_BK + chunk * 4;
        b_off[kk] = (PB_BM + wc * 32 + frow) * PB_BK + chunk * 4;
    }
    const int my_row = wr * 16 + frow;
    const bool my_ok = s_r[my_row] != 0.f;

    f32x4 acc[PB_MAXSUB][2];
#pragma unroll
    for (int q = 0; q < PB_MAXSUB; ++q)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[q][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    gload(0, 0);
    sstore(0);
    __syncthreads();
    int st = 0, ec = 0;
    for (int t = 0; t < T; ++t) {
        const int buf = t & 1;
        int nst_ = st, nec_ = ec + 1;
        if (nec_ == nec) { nec_ = 0; ++nst_; }
        if (t + 1 < T) gload(nst_, nec_);
        const float* sb = lds + buf * stage;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const f32x4 af = *(const f32x4*)(sb + a_off[kk]);
#pragma unroll
            for (int q = 0; q < PB_MAXSUB; ++q)
                if (q < nsub) {
                    f32x4 bf[2];
#pragma unroll
                    for (int j = 0; j < 2; ++j) bf[j] = *(const f32x4*)(sb + b_off[kk] + (q * PB_BN + j * 16) * PB_BK);
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[q][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][s], af[s], acc[q][j], 0, 0, 0);
                }
        }
        if (t + 1 < T) sstore(buf ^ 1);
        if (ec == nec - 1) {
            // lane (frow, fgrp) holds the scores of row 16 wr + frow against classes (st nsub + q) 64 + wc 32 + j 16 + fgrp 4 + {0..3}
#pragma unroll
            for (int q = 0; q < PB_MAXSUB; ++q)
                if (q < nsub) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int cls = (st * nsub + q) * PB_BN + wc * 32 + j * 16 + fgrp * 4 + r;
                            if (cls < c) {
                                float v = 0.f;
                                if (my_ok) {
                                    v = fmaf(scale, acc[q][j][r], bias ? bias[cls] : 0.f);
                                    if (base) v = base[(r0 + my_row) * c + cls] + v;
                                }
                                xs[my_row * xp + cls] = v;
                            }
                        }
                        acc[q][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    }
                }
        }
        st = nst_;
        ec = nec_;
        __syncthreads();
    }

    // eight lanes per row (the row srow, lanes sub = 0 .. 7 of one wave)
    {
        const int sub = tid & 7;
        float* xr = xs + srow * xp;
        const int y = s_y[srow];
        const float w = s_r[srow];
        float row_loss = 0.f, sum = 1.f, tsum = 1.f;
        if (srow_ok) {      // (uniform over the eight lanes of a row; the shuffles below stay inside them)
            float m = -FLT_MAX;
            for (int k = sub; k < c; k += 8) m = fmaxf(m, xr[k]);
            m = fmaxf(m, __shfl_xor(m, 1));
            m = fmaxf(m, __shfl_xor(m, 2));
            m = fmaxf(m, __shfl_xor(m, 4));
            float dot = 0.f;
            if (y >= 0) {
                dot = xr[y];
            } else {
                const float* sr = soft + (r0 + srow) * c;
                tsum = 0.f;
                for (int k = 0; k < c; ++k) tsum += sr[k];
                for (int k = sub; k < c; k += 8) dot = fmaf(sr[k], xr[k], dot);
                dot += __shfl_xor(dot, 1);
                dot += __shfl_xor(dot, 2);
                dot += __shfl_xor(dot, 4);
            }
            sum = 0.f;
            for (int k = sub; k < c; k += 8) {
                const float ex = expf(xr[k] - m);
                xr[k] = ex;
                sum += ex;
            }
            sum += __shfl_xor(sum, 1);
            sum += __shfl_xor(sum, 2);
            sum += __shfl_xor(sum, 4);
            const float lse = m + logf(sum);
            row_loss = w * fmaf(tsum, lse, -dot);
        }
        if (sub == 0) {
            s_sum[srow] = sum;
            s_T[srow] = tsum;
            s_loss[srow] = row_loss;
        }
    }
    __syncthreads();
    for (int id = tid; id < rows_here * c; id += 256) {
        const int row = id / c, k = id - row * c;
        const float w = s_r[row];
        float v = 0.f;
        if (w != 0.f) {
            const int y = s_y[row];
            const float p = xs[row * xp + k] / s_sum[row];
            const float tk = y >= 0 ? (k == y ? 1.f : 0.f) : soft[(r0 + row) * c + k];
            v = w * fmaf(s_T[row], p, -tk);
        }
        g[(r0 + row) * c + k] = v;
    }
    if (tid == 0) {
        float s = 0.f;
        for (int q = 0; q < PB_BM; ++q) s += s_loss[q];
        part_loss[blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------- transposed contraction
// grid (class tiles x column tiles, slices): part_w[slice, cls, d] = sum over the slice's rows of g[row, cls] f[row, d]; column tile 0 also part_b[slice, cls]
__global__ __launch_bounds__(256) void probe_contract_kernel(const float* __restrict__ f, const float* __restrict__ g, const int32_t* __restrict__ labels,
                                                             const float* __restrict__ rw, int has_soft, int n, int c, int e, int nct, int per,
                                                             float* __restrict__ part_w, float* __restrict__ part_b) {
    const int lane = threadIdx.x & 63, frow = lane & 15, fgrp = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ct = blockIdx.x % nct, et = blockIdx.x / nct;
    const int c0 = ct * PB_CT + wave * 32, b0 = et * PB_ET;
    if (c0 >= c) return;        // per wave (the kernel has no barrier)
    const int r0 = blockIdx.y * per * PB_ROWS, r1 = (int)min((int64_t)n, (int64_t)r0 + (int64_t)per * PB_ROWS);
    const int bcol = b0 + frow * 4;
    const bool b_ok = bcol < e;
    const bool a_ok[2] = {c0 + frow < c, c0 + 16 + frow < c};
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[2][4] = {{zero, zero, zero, zero}, {zero, zero, zero, zero}};
    float bsum[2] = {0.f, 0.f};
    // lane (frow, fgrp) of a step: g[r + fgrp, c0 + 16 a + frow] (A: class x row) and f[r + fgrp, b0 + 4 frow + j] (B of MFMA j: row x column).  Sixteen rows
    // a trip as four steps of four: labels and weights first, then the operands, then the MFMAs in step order (gda_scatter_kernel's schedule).
    for (int r = r0; r < r1; r += 16) {
        int y[4];
        float w[4], ga[4][2];
        f32x4 fb[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = r + s * 4 + fgrp;
            y[s] = row < r1 ? labels[row] : -2;
            w[s] = (row < r1 && rw) ? rw[row] : 1.0f;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = r + s * 4 + fgrp;
            const bool ok = probe_row_ok(y[s], w[s], c, has_soft != 0);
            const float* gr = g + (size_t)row * c + c0 + frow;
            ga[s][0] = (ok && a_ok[0]) ? gr[0] : 0.f;
            ga[s][1] = (ok && a_ok[1]) ? gr[16] : 0.f;
            fb[s] = (ok && b_ok) ? *(const f32x4*)(f + (size_t)row * e + bcol) : zero;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                bsum[a] += ga[s][a];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[a][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[s][a], fb[s][j], acc[a][j], 0, 0, 0);
            }
        }
    }
    // the lane holds classes c0 + 16 a + fgrp * 4 + {0..3} of columns b0 + frow * 4 + {j}
    float* out = part_w + (size_t)blockIdx.y * c * e;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int cls = c0 + a * 16 + fgrp * 4 + q;
            if (cls < c && b_ok) *(f32x4*)(out + (size_t)cls * e + bcol) = (f32x4){acc[a][0][q], acc[a][1][q], acc[a][2][q], acc[a][3][q]};
        }
        // the four lanes (frow, 0..3) of a class: (l0 + l1) + (l2 + l3) in every one of them
        float v = bsum[a];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (et == 0 && fgrp == 0 && a_ok[a]) part_b[(size_t)blockIdx.y * c + c0 + a * 16 + frow] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- finalise / update
__device__ __forceinline__ float probe_slice_sum(const float* __restrict__ part, int slices, size_t stride, size_t i) {
    float s = 0.f;
    for (int q = 0; q < slices; ++q) s += part[(size_t)q * stride + i];
    return s;
}
// the last workgroup of the two kernels below: norm times the nblk loss partials (256 strided sums, then those in ascending order)
__device__ __forceinline__ void probe_loss_sum(const float* __restrict__ part_loss, int nblk, float norm, float* __restrict__ out) {
    __shared__ float part[256];
    const int tid = threadIdx.x;
    float s = 0.f;
    for (int i = tid; i < nblk; i += 256) s += part_loss[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int q = 0; q < 256; ++q) t += part[q];
        *out = norm * t;
    }
}

// grid: ceil((c e + c) / 256) workgroups of elements, then one for the loss
__global__ __launch_bounds__(256) void probe_final_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b, const float* __restrict__ part_loss,
                                                          int slices, int nblk, int c, int e, float scale, float norm, float* __restrict__ loss_out,
                                                          float* __restrict__ grad_w, float* __restrict__ grad_b) {
    if (blockIdx.x == gridDim.x - 1) {      // per workgroup
        probe_loss_sum(part_loss, nblk, norm, loss_out);
        return;
    }
    const size_t ce = (size_t)c * e, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < ce) grad_w[i] = (norm * scale) * probe_slice_sum(part_w, slices, ce, i);
    else if (i < ce + c) grad_b[i - ce] = norm * probe_slice_sum(part_b, slices, (size_t)c, i - ce);
}

// the same sums, then the heavy-ball step (include/grip_amd.h): G = fmaf(l2, W, gw); m = fmaf(mu, m, G); W = fmaf(-lr, m, W); the bias without the ridge
__global__ __launch_bounds__(256) void probe_update_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b, const float* __restrict__ part_loss,
                                                           int slices, int nblk, int c, int e, float scale, float norm, float l2, float lr, float mu,
                                                           float* __restrict__ w, float* __restrict__ b, float* __restrict__ mw, float* __restrict__ mb,
                                                           float* __restrict__ loss_out) {
    if (blockIdx.x == gridDim.x - 1) {
        if (loss_out) probe_loss_sum(part_loss, nblk, norm, loss_out);
        return;
    }
    const size_t ce = (size_t)c * e, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < ce) {
        const float gw = (norm * scale) * probe_slice_sum(part_w, slices, ce, i);
        const float wi = w[i];
        const float m = fmaf(mu, mw[i], fmaf(l2, wi, gw));
        mw[i] = m;
        w[i] = fmaf(-lr, m, wi);
    } else if (i < ce + c) {
        const size_t k = i - ce;
        const float gb = norm * probe_slice_sum(part_b, slices, (size_t)c, k);
        const float m = fmaf(mu, mb[k], gb);
        mb[k] = m;
        b[k] = fmaf(-lr, m, b[k]);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return a && b && (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}
size_t pad64(size_t floats) { return (floats + 63) / 64 * 64; }
bool pos_finite(float x) { return x > 0.f && x <= FLT_MAX; }

struct ProbePlan {
    int nsub, xp, nblk, nct, net, per, slices;
    size_t lds_bytes, g_floats, pw_floats, pb_floats, bytes;
};
// everything below is a function of (n, c, e) alone
ProbePlan probe_plan(int n, int c, int e) {
    ProbePlan p;
    const int nkt = (c + PB_BN - 1) / PB_BN;
    p.nsub = nkt <= PB_MAXSUB ? nkt : 1;
    p.xp = nkt * PB_BN + 1;
    p.nblk = (n + PB_BM - 1) / PB_BM;
    p.lds_bytes = ((size_t)2 * (PB_BM + PB_BN * p.nsub) * PB_BK + (size_t)PB_BM * p.xp + 5 * PB_BM) * sizeof(float);
    p.nct = (c + PB_CT - 1) / PB_CT;
    p.net = (e + PB_ET - 1) / PB_ET;
    const int cap = std::min(64, std::max(4, 1024 / (p.nct * p.net)));     // (engine.probe_slice_cap)
    const int nch = (n + PB_ROWS - 1) / PB_ROWS;
    p.per = (nch + cap - 1) / cap;
    p.slices = (nch + p.per - 1) / p.per;
    p.g_floats = pad64((size_t)n * c);
    p.pw_floats = pad64((size_t)p.slices * c * e);
    p.pb_floats = pad64((size_t)p.slices * c);
    p.bytes = (p.g_floats + p.pw_floats + p.pb_floats + pad64((size_t)p.nblk)) * sizeof(float) + 256;
    return p;
}

int check_shape(const char* who, int n, int c, int e) {
    GRIP_REQUIRE(n > 0 && n <= INT_MAX - 1024, "%s: n = %d (1 .. 2^31 - 1025)", who, n);
    GRIP_REQUIRE(c > 0 && c <= PB_MAX_C, "%s: c = %d (1 .. %d)", who, c, PB_MAX_C);
    GRIP_REQUIRE(e > 0 && e % 4 == 0 && e <= PB_MAX_E, "%s: e = %d (a multiple of 4, 4 .. %d)", who, e, PB_MAX_E);
    return GRIP_OK;
}

struct Span {
    const void* p;
    size_t bytes;
};
bool any_overlap(const Span* outs, int n_out, const Span* ins, int n_in) {
    for (int i = 0; i < n_out; ++i) {
        for (int j = 0; j < n_in; ++j)
            if (overlap(outs[i].p, outs[i].bytes, ins[j].p, ins[j].bytes)) return true;
        for (int j = i + 1; j < n_out; ++j)
            if (overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes)) return true;
    }
    return false;
}

struct ProbeWs {
    float *g, *pw, *pb, *pl;
};
ProbeWs carve(void* workspace, const ProbePlan& p) {
    ProbeWs w;
    w.g = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    w.pw = w.g + p.g_floats;
    w.pb = w.pw + p.pw_floats;
    w.pl = w.pb + p.pb_floats;
    return w;
}

// the score kernel needs more than the 64 KiB of dynamic LDS a kernel gets by default from c = 129 on: the limit is raised on the current device, once
// per host call that needs it (not a stream operation: nothing is enqueued)
int allow_lds(const ProbePlan& p) {
    if (p.lds_bytes > 64 * 1024)
        GRIP_CHECK_HIP(hipFuncSetAttribute((const void*)probe_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return GRIP_OK;
}

// the two kernels every iteration starts with: g, the loss partials, the [slices, c, e] and [slices, c] partial sums
int launch_grad(const float* feats, const float* w, const float* b, const float* base, const int32_t* labels, const float* soft, const float* row_weight,
                float scale, int n, int c, int e, const ProbePlan& p, const ProbeWs& ws, hipStream_t s) {
    hipLaunchKernelGGL(probe_score_kernel, dim3(p.nblk), dim3(256), p.lds_bytes, s, feats, w, b, base, labels, soft, row_weight, scale, n, c, e, p.nsub, p.xp,
                       ws.g, ws.pl);
    GRIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(probe_contract_kernel, dim3(p.nct * p.net, p.slices), dim3(256), 0, s, feats, ws.g, labels, row_weight, soft ? 1 : 0, n, c, e, p.nct, p.per,
                       ws.pw, ws.pb);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}
}  // namespace

#define RUNC(x) do { int _rc = (x); if (_rc != GRIP_OK) return _rc; } while (0)

extern "C" int grip_probe_objective_workspace(int n, int c, int e, size_t* bytes) {
    GRIP_REQUIRE(bytes, "probe_objective_workspace: null pointer");
    RUNC(check_shape("probe_objective_workspace", n, c, e));
    *bytes = probe_plan(n, c, e).bytes;
    return GRIP_OK;
}

extern "C" int grip_probe_fit_workspace(int n, int c, int e, size_t* bytes) {
    GRIP_REQUIRE(bytes, "probe_fit_workspace: null pointer");
    RUNC(check_shape("probe_fit_workspace", n, c, e));
    *bytes = probe_plan(n, c, e).bytes;
    return GRIP_OK;
}

extern "C" int grip_probe_objective(const float* feats, const float* w, const float* b, const float* base, const int32_t* labels, const float* soft,
                                    const float* row_weight, float scale, float norm, int n, int c, int e, float* loss_out, float* grad_w, float* grad_b,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    RUNC(check_shape("probe_objective", n, c, e));
    GRIP_REQUIRE(pos_finite(scale) && pos_finite(norm), "probe_objective: scale = %g, norm = %g (each finite and > 0)", (double)scale, (double)norm);
    GRIP_REQUIRE(feats && w && labels && loss_out && grad_w && grad_b && workspace, "probe_objective: null pointer");
    GRIP_REQUIRE(aligned16(feats) && aligned16(w), "probe_objective: feats and w must be 16-byte aligned");
    const size_t nb = (size_t)n * 4, cb = (size_t)c * 4;
    const Span outs[] = {{loss_out, 4}, {grad_w, cb * e}, {grad_b, cb}};
    const Span ins[] = {{feats, nb * e}, {w, cb * e}, {b, cb}, {base, nb * c}, {labels, nb}, {soft, nb * c}, {row_weight, nb}};
    GRIP_REQUIRE(!any_overlap(outs, 3, ins, 7), "probe_objective: an output must not alias an input or another output");
    const ProbePlan p = probe_plan(n, c, e);
    GRIP_REQUIRE(workspace_bytes >= p.bytes, "probe_objective: workspace too small (%zu bytes, grip_probe_objective_workspace says %zu)", workspace_bytes,
                 p.bytes);
    RUNC(allow_lds(p));
    hipStream_t s = (hipStream_t)stream;
    const ProbeWs ws = carve(workspace, p);
    RUNC(launch_grad(feats, w, b, base, labels, soft, row_weight, scale, n, c, e, p, ws, s));
    const int nel = (int)(((size_t)c * e + c + 255) / 256);
    hipLaunchKernelGGL(probe_final_kernel, dim3(nel + 1), dim3(256), 0, s, ws.pw, ws.pb, ws.pl, p.slices, p.nblk, c, e, scale, norm, loss_out, grad_w, grad_b);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}

extern "C" int grip_probe_fit(const float* feats, const float* base, const int32_t* labels, const float* soft, const float* row_weight, float scale, float norm,
                              float l2, float lr, float momentum, int iters, int n, int c, int e, float* w, float* b, float* mom_w, float* mom_b,
                              float* loss_trace, void* workspace, size_t workspace_bytes, void* stream) {
    RUNC(check_shape("probe_fit", n, c, e));
    GRIP_REQUIRE(pos_finite(scale) && pos_finite(norm) && pos_finite(lr), "probe_fit: scale = %g, norm = %g, lr = %g (each finite and > 0)", (double)scale,
                 (double)norm, (double)lr);
    GRIP_REQUIRE(l2 >= 0.f && l2 <= FLT_MAX, "probe_fit: l2 = %g (a finite l2 >= 0)", (double)l2);
    GRIP_REQUIRE(momentum >= 0.f && momentum < 1.f, "probe_fit: momentum = %g (0 <= momentum < 1)", (double)momentum);
    GRIP_REQUIRE(iters >= 1, "probe_fit: iters = %d (must be positive)", iters);
    GRIP_REQUIRE(feats && labels && w && b && mom_w && mom_b && workspace, "probe_fit: null pointer");
    GRIP_REQUIRE(aligned16(feats) && aligned16(w), "probe_fit: feats and w must be 16-byte aligned");
    const size_t nb = (size_t)n * 4, cb = (size_t)c * 4;
    const Span outs[] = {{w, cb * e}, {b, cb}, {mom_w, cb * e}, {mom_b, cb}, {loss_trace, (size_t)iters * 4}};
    const Span ins[] = {{feats, nb * e}, {base, nb * c}, {labels, nb}, {soft, nb * c}, {row_weight, nb}};
    GRIP_REQUIRE(!any_overlap(outs, 5, ins, 5), "probe_fit: w, b, mom_w, mom_b and loss_trace must not alias an input or each other");
    const ProbePlan p = probe_plan(n, c, e);
    GRIP_REQUIRE(workspace_bytes >= p.bytes, "probe_fit: workspace too small (%zu bytes, grip_probe_fit_workspace says %zu)", workspace_bytes, p.bytes);
    RUNC(allow_lds(p));
    hipStream_t s = (hipStream_t)stream;
    const ProbeWs ws = carve(workspace, p);
    const int nel = (int)(((size_t)c * e + c + 255) / 256);
    for (int it = 0; it < iters; ++it) {
        RUNC(launch_grad(feats, w, b, base, labels, soft, row_weight, scale, n, c, e, p, ws, s));
        hipLaunchKernelGGL(probe_update_kernel, dim3(nel + 1), dim3(256), 0, s, ws.pw, ws.pb, ws.pl, p.slices, p.nblk, c, e, scale, norm, l2, lr, momentum, w, b,
                           mom_w, mom_b, loss_trace ? loss_trace + it : nullptr);
        GRIP_CHECK_HIP(hipGetLastError());
    }
    return GRIP_OK;
}
