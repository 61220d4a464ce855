// Weighted cross-entropy against SOFT targets gathered from a pool's assignment matrix (include/grip_amd.h, grip_soft_ce): the row kernel beside
// weighted_ce_kernel (head.hip).  One workgroup, wave w walks the rows w, w + 4, ... and the four waves' loss partials meet in that kernel's order.
//   * a HARD row (no matrix, or soft_row outside [0, soft_rows)) with smoothing == 0 runs weighted_ce_kernel's statements verbatim: the same bits.
//   * every other row builds its target per column, t_k = (1 - smoothing) s_k + smoothing / c, with s the one-hot of a hard row or, for a soft row r,
//     s[col_map[j]] = softmax_j(inv_temperature logf(max(soft[r, j], 2^-126))) (the floor and log-domain form of sinkhorn.hip; an all-zero matrix row is
//     uniform over the cz mapped columns) and 0 on the unmapped columns.  T = sum_k t_k, loss += w (T lse - sum_k t_k x_k), grad_k = w (T p_k - t_k).
// The scatter runs backwards: the workgroup first inverts col_map into the LDS (inv[k] = j or -1, c ints, the only shared state), and the lane that owns
// column k GATHERS soft[r, inv[k]] -- every output element has one writer, nothing is written twice and no [n, c] target block exists unless the
// caller asks for target_out.  t_k is recomputed (same statements, fp contraction off: same bits) where the gradient needs it after T is known.
// f32 throughout, no atomics, every sum in a fixed order; a row's bits depend on that row, its matrix row and col_map alone.
#include <float.h>
#include <math.h>

#include "common.h"

namespace {
constexpr int SCE_MAX_C = 16000;      // classes whose inverse column map fits the 64 KiB of LDS a kernel gets by default (soft given only)

struct SoftRow {      // a soft row's sharpened distribution: s_j = expf(L_j - mx) / sum
    const float* z;   // the matrix row [cz]
    float inv_t, mx, sum;
};

__device__ __forceinline__ float sce_logit(float z, float inv_t) {
#pragma clang fp contract(off)
    return inv_t * logf(fmaxf(z, FLT_MIN));
}

// t_k of the header comment.  j: the matrix column behind logits column k (soft rows), -1 none; hot: k is a hard row's in-range label
__device__ __forceinline__ float sce_target(const SoftRow& sr, int j, bool hot, float keep, float floor_) {
#pragma clang fp contract(off)
    float s = hot ? 1.f : 0.f;
    if (j >= 0) s = expf(sce_logit(sr.z[j], sr.inv_t) - sr.mx) / sr.sum;
    const float ks = keep * s;
    return ks + floor_;
}

__global__ __launch_bounds__(256) void soft_ce_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, const float* __restrict__ weight,
                                                      int n, int c, const float* __restrict__ soft, int64_t soft_rows, int cz,
                                                      const int32_t* __restrict__ soft_row, const int32_t* __restrict__ col_map, float inv_t, float smoothing,
                                                      float* __restrict__ loss, float* __restrict__ grad, float* __restrict__ target) {
    extern __shared__ int inv[];      // [c] when soft != nullptr
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (soft) {
        for (int k = threadIdx.x; k < c; k += 256) inv[k] = -1;
        __syncthreads();
        for (int j = threadIdx.x; j < cz; j += 256) {
            const int k = col_map[j];
            if (k >= 0 && k < c) inv[k] = j;      // (distinct entries in [0, c) are the caller's contract; nothing else is ever indexed)
        }
        __syncthreads();
    }
    const float keep = 1.f - smoothing, floor_ = smoothing / (float)c;
    float total = 0.f;
    for (int row = wave; row < n; row += 4) {
        const float* x = logits + (size_t)row * c;
        const float w = weight[row];
        const int lab = labels[row];
        const int64_t r = soft ? (int64_t)soft_row[row] : -1;
        const bool is_soft = r >= 0 && r < soft_rows;
        float m = -INFINITY;
        for (int j = lane; j < c; j += 64) m = fmaxf(m, x[j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        float sum = 0.f;
        for (int j = lane; j < c; j += 64) sum += expf(x[j] - m);
        sum = wave_sum(sum);
        const float lse = m + logf(sum);
        if (!is_soft && smoothing == 0.f) {      // (per wave) weighted_ce_kernel's own statements
            if (grad)
                for (int j = lane; j < c; j += 64) grad[(size_t)row * c + j] = w * (expf(x[j] - m) / sum - (j == lab ? 1.f : 0.f));
            if (target)
                for (int j = lane; j < c; j += 64) target[(size_t)row * c + j] = j == lab ? 1.f : 0.f;
            if (w != 0.f && lab >= 0 && lab < c) total += w * (lse - x[lab]);
            continue;
        }
        SoftRow sr = {nullptr, inv_t, 0.f, 1.f};
        if (is_soft) {
            sr.z = soft + (size_t)r * cz;
            float mx = -INFINITY, ssum = 0.f;
            for (int j = lane; j < cz; j += 64) mx = fmaxf(mx, sce_logit(sr.z[j], inv_t));
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            for (int j = lane; j < cz; j += 64) ssum += expf(sce_logit(sr.z[j], inv_t) - mx);
            sr.mx = mx;
            sr.sum = wave_sum(ssum);
        }
        float tsum = 0.f, dot = 0.f;
        for (int k = lane; k < c; k += 64) {
#pragma clang fp contract(off)
            const float t = sce_target(sr, is_soft ? inv[k] : -1, !is_soft && k == lab, keep, floor_);
            if (target) target[(size_t)row * c + k] = t;
            tsum += t;
            const float tx = t * x[k];
            dot += tx;
        }
        tsum = wave_sum(tsum);
        dot = wave_sum(dot);
        const bool counted = is_soft || (lab >= 0 && lab < c);
        if (!counted) tsum = 1.f;      // weighted_ce_kernel's rule for a label outside [0, c): the whole softmax stays, only the smoothing floor is subtracted
        if (grad)
            for (int k = lane; k < c; k += 64) {
#pragma clang fp contract(off)
                const float t = sce_target(sr, is_soft ? inv[k] : -1, !is_soft && k == lab, keep, floor_);
                const float tp = tsum * (expf(x[k] - m) / sum);
                grad[(size_t)row * c + k] = w * (tp - t);
            }
        if (w != 0.f && counted) {
#pragma clang fp contract(off)
            const float tl = tsum * lse;
            const float e = w * (tl - dot);
            total += e;
        }
    }
    if (lane == 0) part[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = ((part[0] + part[1]) + part[2]) + part[3];
}
}  // namespace

extern "C" int grip_soft_ce(const float* logits, const int32_t* labels, const float* row_weight, int n, int c, const float* soft, int64_t soft_rows, int cz,
                            const int32_t* soft_row, const int32_t* col_map, float inv_temperature, float smoothing, float* loss, float* grad_logits,
                            float* target_out, void* stream) {
    GRIP_REQUIRE(logits && labels && row_weight && loss, "soft_ce: null pointer");
    GRIP_REQUIRE(n > 0 && c > 0, "soft_ce: empty input (n = %d, c = %d)", n, c);
    GRIP_REQUIRE(inv_temperature > 0.f && inv_temperature <= FLT_MAX, "soft_ce: inv_temperature = %g (a finite value > 0)", (double)inv_temperature);
    GRIP_REQUIRE(smoothing >= 0.f && smoothing < 1.f, "soft_ce: smoothing = %g (in [0, 1))", (double)smoothing);
    size_t lds = 0;
    if (soft) {
        GRIP_REQUIRE(soft_row && col_map, "soft_ce: null pointer (soft_row and col_map come with soft)");
        GRIP_REQUIRE(cz >= 1 && cz <= c, "soft_ce: cz = %d (in [1, c = %d])", cz, c);
        GRIP_REQUIRE(c <= SCE_MAX_C, "soft_ce: c = %d with soft targets (at most %d: the inverse column map lives in the LDS)", c, SCE_MAX_C);
        lds = (size_t)c * sizeof(int);
    }
    hipLaunchKernelGGL(soft_ce_kernel, dim3(1), dim3(256), lds, (hipStream_t)stream, logits, labels, row_weight, n, c, soft, soft_rows, cz, soft_row, col_map,
                       inv_temperature, smoothing, loss, grad_logits, target_out);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}
