// Balanced (Sinkhorn-Knopp) assignment of a pool's class probabilities: rows sum to one, columns are pressed towards n x a class prior.  The recursion is
// the one of include/grip_amd.h: L = tau log max(P, 2^-126); `iters` times  q_i = softmax_c(L_i + b),  s_c = sum_i q_ic,
// b_c += log_target_c + log n - log max(s_c, 2^-126);  then Q_i = softmax_c(L_i + b), its first arg-max and mass_c = sum_i Q_ic.  The row scaling of
// Sinkhorn is the softmax normaliser: the only state between iterations is b [c].  All f32 / int32, no atomics, every sum in a fixed order.
//   * sk_pass_kernel: a wave owns one CHUNK of SK_ROWS consecutive rows (a constant: the partition does not depend on the device) and walks them in
//     ascending order -- lanes over classes, the row's maximum subtracted first, the softmax in the manner of gmm_sweep_kernel -- adding each row's q
//     to the chunk's column sums, which go to the workspace as part[chunk, :].  L is NOT materialised: a pass reads P (n c 4 bytes, the floor) and redoes
//     logf on the VALU, which a streaming kernel has to spare; a stored L would add a pass's worth of writes and save nothing a pass reads.
//       - up to 128 classes (NP = 1, 2) the chunk's P values are all loaded before the first row is worked on (one memory round trip per chunk,
//         SK_ROWS x NP registers), a row's arguments stay in registers and so do the column sums;
//       - beyond (NP = 0) the row's arguments wait in q[i, :] between the passes over the classes (a lane re-reads only what it wrote itself; q is an
//         output of the call and free until the final pass writes it) and the column sums are kept in part[chunk, :] itself, read and written by the
//         one lane that owns the class, rows ascending.
//     The final pass also writes Q and the first arg-max.  A row's bits depend on that row and b only: not on n, not on its place in a chunk.
//   * sk_final_kernel: 16 classes per workgroup, SK_FS threads per class: thread (class, s) adds the partials of the chunks [s per, (s + 1) per),
//     per = ceil(chunks / SK_FS), in ascending order, and thread (class, 0) adds the SK_FS slices in ascending order -- an order fixed by n alone.  It then
//     writes b_out = b_in + ((log_target + log n) - logf(max(s, 2^-126))), or on the final pass mass = s and b_out = b_in.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {
constexpr int SK_ROWS = 16;       // rows per chunk = per wave of sk_pass_kernel (engine.SINKHORN_ROWS)
constexpr int SK_FC = 16;         // classes per workgroup of sk_final_kernel
constexpr int SK_FS = 64;         // slices of the chunk partials per class in sk_final_kernel
constexpr int SK_REG_C = 128;     // classes a pass keeps in registers at most (two per lane)

// Maximum over the 64 lanes of a wave, returned in every lane: the DPP steps of wave_sum (common.h) with fmaxf.  Needs all 64 lanes active.
__device__ __forceinline__ float sk_wave_max(float v) {
#define SK_DPP_MAX(ctrl) v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, true)))
    SK_DPP_MAX(0xB1);     // quad_perm [1,0,3,2]
    SK_DPP_MAX(0x4E);     // quad_perm [2,3,0,1]
    SK_DPP_MAX(0x141);    // row_half_mirror
    SK_DPP_MAX(0x140);    // row_mirror
#undef SK_DPP_MAX
    const int b = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// the wave's (largest value, lowest class holding it) from every lane's own candidate; lane 0 writes it
__device__ __forceinline__ void sk_store_argmax(float bv, int bi, int lane, int32_t* dst) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) *dst = bi;
}

// NP > 0: c <= 64 NP.  chunk = blockIdx.x * 4 + wave; part[chunk, :] = sum over the chunk's rows, ascending, of softmax_c(tau log max(P, 2^-126) + b);
// q / argmax (the final pass; argmax optional): the rows themselves and their first arg-max.  b == nullptr: zeros.
template <int NP>
__global__ __launch_bounds__(256) void sk_pass_kernel(const float* __restrict__ probs, const float* __restrict__ b, float tau, int n, int c, int nch,
                                                      float* __restrict__ part, float* __restrict__ q, int32_t* __restrict__ argmax) {
    const int lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (chunk >= nch) return;       // per wave (the kernel has no barrier)
    const int r0 = chunk * SK_ROWS;
    float bb[NP], p[SK_ROWS][NP], col[NP];
#pragma unroll
    for (int h = 0; h < NP; ++h) {
        const int cls = h * 64 + lane;
        bb[h] = (b && cls < c) ? b[cls] : 0.f;
        col[h] = 0.f;
    }
#pragma unroll
    for (int r = 0; r < SK_ROWS; ++r)
#pragma unroll
        for (int h = 0; h < NP; ++h) {
            const int cls = h * 64 + lane;
            p[r][h] = (r0 + r < n && cls < c) ? probs[(size_t)(r0 + r) * c + cls] : 1.f;
        }
#pragma unroll
    for (int r = 0; r < SK_ROWS; ++r) {
        const int row = r0 + r;
        if (row >= n) break;        // (wave-uniform)
        float a[NP], mx = -INFINITY, sum = 0.f;
#pragma unroll
        for (int h = 0; h < NP; ++h) {
            a[h] = h * 64 + lane < c ? fmaf(tau, logf(fmaxf(p[r][h], FLT_MIN)), bb[h]) : -INFINITY;
            mx = fmaxf(mx, a[h]);
        }
        mx = sk_wave_max(mx);
#pragma unroll
        for (int h = 0; h < NP; ++h) {
            a[h] = expf(a[h] - mx);         // (a class >= c: exp(-inf) = 0)
            sum += a[h];
        }
        sum = wave_sum(sum);
        float bv = -INFINITY;
        int bi = INT_MAX;
#pragma unroll
        for (int h = 0; h < NP; ++h) {
            const int cls = h * 64 + lane;
            if (cls < c) {
                const float v = a[h] / sum;
                col[h] += v;
                if (q) q[(size_t)row * c + cls] = v;
                if (v > bv) { bv = v; bi = cls; }
            }
        }
        if (argmax) sk_store_argmax(bv, bi, lane, argmax + row);
    }
#pragma unroll
    for (int h = 0; h < NP; ++h) {
        const int cls = h * 64 + lane;
        if (cls < c) part[(size_t)chunk * c + cls] = col[h];
    }
}

// any c: the row's arguments wait in scratch[i, :] (the call's q: never probs) between the passes over the classes, the chunk's column sums in
// part[chunk, :].  final != 0: scratch IS the output and keeps the row; argmax optional.
__global__ __launch_bounds__(256) void sk_pass_any_kernel(const float* __restrict__ probs, const float* __restrict__ b, float tau, int n, int c, int nch,
                                                          float* __restrict__ part, float* __restrict__ scratch, int32_t* __restrict__ argmax) {
    const int lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (chunk >= nch) return;       // per wave
    const int r0 = chunk * SK_ROWS, r1 = min(n, r0 + SK_ROWS);
    float* pc = part + (size_t)chunk * c;
    for (int row = r0; row < r1; ++row) {
        const float* pr = probs + (size_t)row * c;
        float* zr = scratch + (size_t)row * c;
        float mx = -INFINITY, sum = 0.f;
        for (int c0 = 0; c0 < c; c0 += 64) {
            const int cls = c0 + lane;
            if (cls < c) {
                const float v = fmaf(tau, logf(fmaxf(pr[cls], FLT_MIN)), b ? b[cls] : 0.f);
                zr[cls] = v;
                mx = fmaxf(mx, v);
            }
        }
        mx = sk_wave_max(mx);
        for (int c0 = 0; c0 < c; c0 += 64) {
            const int cls = c0 + lane;
            if (cls < c) {
                const float x = expf(zr[cls] - mx);
                zr[cls] = x;
                sum += x;
            }
        }
        sum = wave_sum(sum);
        float bv = -INFINITY;
        int bi = INT_MAX;
        for (int c0 = 0; c0 < c; c0 += 64) {
            const int cls = c0 + lane;
            if (cls < c) {
                const float v = zr[cls] / sum;
                zr[cls] = v;
                pc[cls] = row == r0 ? v : pc[cls] + v;      // (the lane that owns the class, rows ascending)
                if (v > bv) { bv = v; bi = cls; }
            }
        }
        if (argmax) sk_store_argmax(bv, bi, lane, argmax + row);
    }
}

// s[cls] = the chunk partials added in the fixed order of the header comment; mass == nullptr: b_out = b_in + ((log_target + logn) - logf(max(s, 2^-126))),
// else mass = s and b_out = b_in.  b_in == nullptr: zeros; b_in may be b_out (a thread reads its class before it writes it).
__global__ __launch_bounds__(SK_FC * SK_FS) void sk_final_kernel(const float* __restrict__ part, int nch, int c, const float* __restrict__ log_target,
                                                                 float logn, const float* b_in, float* b_out, float* __restrict__ mass) {
    __shared__ float sl[SK_FS][SK_FC];
    const int it = threadIdx.x % SK_FC, s = threadIdx.x / SK_FC;
    const int cls = blockIdx.x * SK_FC + it;
    const int per = (nch + SK_FS - 1) / SK_FS, ch0 = min(nch, s * per), ch1 = min(nch, ch0 + per);
    float acc = 0.f;
    if (cls < c) {
        const float* src = part + cls;
#pragma unroll 8
        for (int ch = ch0; ch < ch1; ++ch) acc += src[(size_t)ch * c];
    }
    sl[s][it] = acc;
    __syncthreads();
    if (cls >= c || s != 0) return;
#pragma unroll
    for (int k = 1; k < SK_FS; ++k) acc += sl[k][it];
    const float bi = b_in ? b_in[cls] : 0.f;
    if (mass) {
        mass[cls] = acc;
        b_out[cls] = bi;
    } else {
        b_out[cls] = bi + ((log_target[cls] + logn) - logf(fmaxf(acc, FLT_MIN)));
    }
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}
int check_dims(const char* who, int n, int c) {
    GRIP_REQUIRE(n >= 1 && c >= 1, "%s: n = %d, c = %d (each must be at least 1)", who, n, c);
    return GRIP_OK;
}
int64_t chunks(int n) { return ((int64_t)n + SK_ROWS - 1) / SK_ROWS; }
size_t ws_bytes(int n, int c) { return (size_t)chunks(n) * c * sizeof(float) + 256; }
}  // namespace

#define RUNC(x) do { int _rc = (x); if (_rc != GRIP_OK) return _rc; } while (0)

extern "C" int grip_sinkhorn_workspace(int n, int c, size_t* bytes) {
    GRIP_REQUIRE(bytes, "sinkhorn_workspace: null pointer");
    RUNC(check_dims("sinkhorn_workspace", n, c));
    *bytes = ws_bytes(n, c);
    return GRIP_OK;
}

extern "C" int grip_sinkhorn_balance(const float* probs, const float* log_target, const float* log_scale_in, float tau, int iters, int n, int c, float* q,
                                     int32_t* pred, float* mass, float* log_scale_out, void* workspace, size_t workspace_bytes, void* stream) {
    RUNC(check_dims("sinkhorn_balance", n, c));
    GRIP_REQUIRE(tau > 0.f && tau <= FLT_MAX, "sinkhorn_balance: tau = %g (a finite tau > 0)", (double)tau);
    GRIP_REQUIRE(iters >= 0, "sinkhorn_balance: iters = %d (at least 0)", iters);
    GRIP_REQUIRE(probs && log_target && q && mass && log_scale_out && workspace, "sinkhorn_balance: null pointer");
    const size_t qb = (size_t)n * c * 4, cb = (size_t)c * 4;
    GRIP_REQUIRE(!overlap(q, qb, probs, qb), "sinkhorn_balance: q must not alias probs");
    GRIP_REQUIRE(!overlap(log_scale_out, cb, log_target, cb) && !overlap(mass, cb, log_target, cb) && !overlap(mass, cb, log_scale_out, cb) &&
                     (!log_scale_in || !overlap(mass, cb, log_scale_in, cb)),
                 "sinkhorn_balance: mass, log_scale_out and log_target must not alias one another (log_scale_in may be log_scale_out)");
    GRIP_REQUIRE(workspace_bytes >= ws_bytes(n, c), "sinkhorn_balance: workspace too small (%zu bytes, grip_sinkhorn_workspace says %zu)", workspace_bytes,
                 ws_bytes(n, c));
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const int nch = (int)chunks(n);
    const float logn = (float)log((double)n);
    const dim3 pgrid((nch + 3) / 4), fgrid((c + SK_FC - 1) / SK_FC);
    const float* b = log_scale_in;
    for (int t = 0; t <= iters; ++t) {
        const bool last = t == iters;
        float* qo = last ? q : (float*)nullptr;
        int32_t* am = last ? pred : (int32_t*)nullptr;
        if (c <= 64)
            hipLaunchKernelGGL(sk_pass_kernel<1>, pgrid, dim3(256), 0, s, probs, b, tau, n, c, nch, part, qo, am);
        else if (c <= SK_REG_C)
            hipLaunchKernelGGL(sk_pass_kernel<2>, pgrid, dim3(256), 0, s, probs, b, tau, n, c, nch, part, qo, am);
        else
            hipLaunchKernelGGL(sk_pass_any_kernel, pgrid, dim3(256), 0, s, probs, b, tau, n, c, nch, part, q, am);
        GRIP_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(sk_final_kernel, fgrid, dim3(SK_FC * SK_FS), 0, s, part, nch, c, log_target, logn, b, log_scale_out, last ? mass : (float*)nullptr);
        GRIP_CHECK_HIP(hipGetLastError());
        b = log_scale_out;
    }
    return GRIP_OK;
}
