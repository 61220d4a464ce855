// Multi-view mode (MTA: Zanella & Ben Ayed, CVPR 2024, as the model of include/grip_amd.h states it): the V view embeddings of an image are weighted by
// how much each view is an inlier -- helped by how similarly the views are classified -- and a robust mean-shift mode is moved to the dense part of them.
//   u_p = f_p / |f_p|,  G = U U^T,  d2_pq = max(0, 2 - 2 G_pq);  h2_p = max(mean of the r smallest d2_pq (q != p), h2_floor);  A = S S^T;
//   `outer` times:  k_p = exp(-|u_p - m|^2 / (2 h2_p));  `inner` times  y = softmax_p((k_p + lam sum_q A_pq y_q) / lam_y);
//                   m = sum_p y_p k_p u_p / max(sum_p y_p k_p, 2^-126).
// view_mode_kernel: ONE workgroup (four waves) per image, one launch per call, no workspace, no atomics, every sum in a fixed order.
//   * 1 / |f_p|: a wave per row (rows wave, wave + 4, ...), a lane adds its float4s in ascending order, then the DPP tree of wave_sum.
//   * G and A run on v_mfma_f32_16x16x4_f32: V is padded to 16-row tiles (rows >= v are ZERO operands and are never read back), a wave takes the tiles
//     wave, wave + 4, ... of the tile grid and contracts with four independent accumulator chains (chain s takes the columns that are s modulo 4 of
//     every 16-column step for U, read as one float4 per lane; for S, whose c is arbitrary, scalar loads), added as (c0 + c1) + (c2 + c3).
//     The operands of U are u = f * (1 / |f|), the product every later sweep forms too.  G_pq and G_qp are the same chain of commutative products.
//   * G, A [64][65], 1 / |f|, h2, the weights y_p k_p and m live in the LDS (38 KiB: four workgroups per CU); U is NOT kept there (64 x 1 024 floats do not
//     fit beside them) but re-read from L2 on every sweep: an image's views are at most 256 KiB and the sweeps of a workgroup follow one another.
//   * the bandwidth: thread p picks the r smallest (value, index) pairs of its row one after the other and adds them as it goes (plain f32, ascending).
//   * y lives in the registers of wave 0 (lane p owns view p; y_q reaches the sum over q through v_readlane, q ascending, one fmaf chain); the softmax
//     subtracts the maximum first; lanes >= v hold -inf / 0 and take no part.
//   * m: thread t owns the columns 4 t .. 4 t + 3 and adds the views in ascending order (fmaf chain), the denominator likewise.
// An image's bits depend on its own operands only: not on n, not on its place in the launch.
#include <float.h>
#include <math.h>

#include "common.h"

namespace {
constexpr int VM_MAXV = 64;       // views per image at most (engine.VIEW_MODE_MAX_VIEWS)
constexpr int VM_MAXE = 1024;     // embedding width at most: 256 threads x one float4
constexpr int VM_P = VM_MAXV + 1; // pitch of the two [V, V] matrices (a thread walks a row: conflict-free)

__device__ __forceinline__ float vm_wave_max(float v) {       // maximum over the 64 lanes in every lane (all lanes active)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// dst[i * VM_P + j] = sum_k X[i, k] X[j, k] (times scale[i] scale[j] on the operands when scale is given) for i, j < 16 tiles; X [v, w] row-major.
// VEC: w % 16 == 0 and 16-byte aligned rows (U); otherwise scalar loads with a column guard (S).
template <bool VEC>
__device__ __forceinline__ void vm_gram(const float* __restrict__ X, int v, int w, const float* scale, float* dst, int wave, int lane) {
    const int tiles = (v + 15) >> 4, frow = lane & 15, fgrp = lane >> 4;
    for (int t = wave; t < tiles * tiles; t += 4) {
        const int ti = t / tiles, tj = t % tiles;
        const int ri = ti * 16 + frow, rj = tj * 16 + frow;
        const float* xi = X + (size_t)ri * w;
        const float* xj = X + (size_t)rj * w;
        const float si = (scale && ri < v) ? scale[ri] : 1.f, sj = (scale && rj < v) ? scale[rj] : 1.f;
        f32x4 acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < w; k0 += 16) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if constexpr (VEC) {
                if (ri < v) a = *(const f32x4*)(xi + k0 + 4 * fgrp) * si;
                if (rj < v) b = *(const f32x4*)(xj + k0 + 4 * fgrp) * sj;
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int k = k0 + 4 * s + fgrp;
                    if (k < w && ri < v) a[s] = xi[k];
                    if (k < w && rj < v) b[s] = xj[k];
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc[s], 0, 0, 0);
        }
        // lane (frow, fgrp) holds rows ti*16 + 4 fgrp + {0..3}, column tj*16 + frow
#pragma unroll
        for (int r = 0; r < 4; ++r)
            dst[(ti * 16 + 4 * fgrp + r) * VM_P + tj * 16 + frow] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
    }
}

__global__ __launch_bounds__(256) void view_mode_kernel(const float* __restrict__ view_emb, const float* __restrict__ view_probs, int v, int c, int e, int r,
                                                        float lam, float lam_y, float h2_floor, int outer, int inner, const float* mode_in,
                                                        const float* y_in, float* mode_out, float* y_out, float* __restrict__ h2_out) {
    __shared__ float G[VM_MAXV * VM_P];
    __shared__ float A[VM_MAXV * VM_P];
    __shared__ __attribute__((aligned(16))) float m[VM_MAXE];
    __shared__ float rn[VM_MAXV], h2[VM_MAXV], kk[VM_MAXV], wgt[VM_MAXV];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t img = blockIdx.x;
    const float* F = view_emb + img * (size_t)v * e;
    const int e4 = e >> 2;

    for (int p = wave; p < v; p += 4) {
        const f32x4* fp = (const f32x4*)(F + (size_t)p * e);
        float s = 0.f;
        for (int i = lane; i < e4; i += 64) {
            const f32x4 x = fp[i];
            s += x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3];
        }
        s = wave_sum(s);
        if (lane == 0) rn[p] = 1.0f / sqrtf(s);
    }
    __syncthreads();

    vm_gram<true>(F, v, e, rn, G, wave, lane);
    if (view_probs) vm_gram<false>(view_probs + img * (size_t)v * c, v, c, nullptr, A, wave, lane);
    __syncthreads();

    if (tid < v) {
        // the r smallest d2 of row tid over q != tid, in ascending (value, index) order
        const float* g = G + tid * VM_P;
        float last_v = -1.f, sum = 0.f;      // (d2 >= 0: nothing precedes the first pick)
        int last_i = -1;
        for (int t = 0; t < r; ++t) {
            float bv = INFINITY;
            int bi = v;
            for (int q = 0; q < v; ++q) {
                if (q == tid) continue;
                const float d = fmaxf(0.f, 2.f - 2.f * g[q]);
                const bool after = d > last_v || (d == last_v && q > last_i);
                if (after && d < bv) { bv = d; bi = q; }      // (q ascends: the first of equal values wins)
            }
            sum += bv;
            last_v = bv;
            last_i = bi;
        }
        const float h = fmaxf(sum / (float)r, h2_floor);
        h2[tid] = h;
        if (h2_out) h2_out[img * v + tid] = h;
    }
    {
        const f32x4 f0 = tid < e4 ? ((const f32x4*)F)[tid] * rn[0] : (f32x4){0.f, 0.f, 0.f, 0.f};
        if (tid < e4) ((f32x4*)m)[tid] = mode_in ? ((const f32x4*)(mode_in + img * e))[tid] : f0;
    }
    float y = 0.f;      // wave 0, lane p: y_p (lanes >= v: 0)
    if (wave == 0 && lane < v) y = y_in ? y_in[img * v + lane] : 1.0f / (float)v;
    __syncthreads();

    for (int o = 0; o < outer; ++o) {
        for (int p = wave; p < v; p += 4) {
            const f32x4* fp = (const f32x4*)(F + (size_t)p * e);
            const float sc = rn[p];
            float s = 0.f;
            for (int i = lane; i < e4; i += 64) {
                const f32x4 d = fp[i] * sc - ((const f32x4*)m)[i];
                s += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
            }
            s = wave_sum(s);
            if (lane == 0) kk[p] = expf(-(s / (2.f * h2[p])));
        }
        __syncthreads();
        if (wave == 0) {
            const float k = lane < v ? kk[lane] : 0.f;
            const float* a = A + lane * VM_P;
            for (int it = 0; it < inner; ++it) {
                float arg = k;
                if (view_probs) {
                    float s = 0.f;
                    const int yb = __builtin_bit_cast(int, y);
                    for (int q = 0; q < v; ++q) s = fmaf(a[q], __builtin_bit_cast(float, __builtin_amdgcn_readlane(yb, q)), s);
                    arg = fmaf(lam, s, k);
                }
                arg = lane < v ? arg / lam_y : -INFINITY;
                const float mx = vm_wave_max(arg);
                const float x = lane < v ? expf(arg - mx) : 0.f;
                y = x / wave_sum(x);
            }
            if (lane < v) wgt[lane] = y * k;
        }
        __syncthreads();
        if (tid < e4) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            float den = 0.f;
            for (int p = 0; p < v; ++p) {
                const float w = wgt[p];
                const f32x4 u = ((const f32x4*)(F + (size_t)p * e))[tid] * rn[p];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(w, u[j], acc[j]);
                den += w;
            }
            den = fmaxf(den, FLT_MIN);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = acc[j] / den;
            ((f32x4*)m)[tid] = acc;
        }
        __syncthreads();
    }
    if (tid < e4) ((f32x4*)(mode_out + img * e))[tid] = ((const f32x4*)m)[tid];
    if (wave == 0 && lane < v) y_out[img * v + lane] = y;
}

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}
int check_dims(const char* who, int n, int v, int c, int e) {
    GRIP_REQUIRE(n >= 1 && c >= 1, "%s: n = %d, c = %d (each must be at least 1)", who, n, c);
    GRIP_REQUIRE(v >= 2 && v <= VM_MAXV, "%s: v = %d (2 .. %d views)", who, v, VM_MAXV);
    GRIP_REQUIRE(e >= 64 && e <= VM_MAXE && e % 64 == 0, "%s: e = %d (a multiple of 64 up to %d)", who, e, VM_MAXE);
    return GRIP_OK;
}
}  // namespace

#define RUNC(x) do { int _rc = (x); if (_rc != GRIP_OK) return _rc; } while (0)

extern "C" int grip_view_mode_workspace(int n, int v, int c, int e, size_t* bytes) {
    GRIP_REQUIRE(bytes, "view_mode_workspace: null pointer");
    RUNC(check_dims("view_mode_workspace", n, v, c, e));
    *bytes = 0;      // everything between the sweeps lives in the LDS
    return GRIP_OK;
}

extern "C" int grip_view_mode(const float* view_emb, const float* view_probs, int n, int v, int c, int e, float rho, float lam, float lam_y, float h2_floor,
                              int outer, int inner, const float* mode_in, const float* y_in, float* mode_out, float* y_out, float* h2_out, void* workspace,
                              size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    RUNC(check_dims("view_mode", n, v, c, e));
    GRIP_REQUIRE(rho > 0.f && rho <= 1.f, "view_mode: rho = %g (0 < rho <= 1)", (double)rho);
    GRIP_REQUIRE(lam >= 0.f && lam <= FLT_MAX, "view_mode: lam = %g (a finite lam >= 0)", (double)lam);
    GRIP_REQUIRE(lam_y > 0.f && lam_y <= FLT_MAX, "view_mode: lam_y = %g (a finite lam_y > 0)", (double)lam_y);
    GRIP_REQUIRE(h2_floor > 0.f && h2_floor <= FLT_MAX, "view_mode: h2_floor = %g (a finite h2_floor > 0)", (double)h2_floor);
    GRIP_REQUIRE(outer >= 0 && inner >= 0, "view_mode: outer = %d, inner = %d (each at least 0)", outer, inner);
    GRIP_REQUIRE(view_emb && mode_out && y_out, "view_mode: null pointer");
    const size_t fb = (size_t)n * v * e * 4, sb = (size_t)n * v * c * 4, mb = (size_t)n * e * 4, yb = (size_t)n * v * 4;
    const struct { const void* p; size_t b; } ins[] = {{view_emb, fb}, {view_probs, sb}}, outs[] = {{mode_out, mb}, {y_out, yb}, {h2_out, yb}};
    for (const auto& o : outs)
        for (const auto& i : ins) GRIP_REQUIRE(!o.p || !i.p || !overlap(o.p, o.b, i.p, i.b), "view_mode: an output must not alias view_emb or view_probs");
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            GRIP_REQUIRE(!outs[a].p || !outs[b].p || !overlap(outs[a].p, outs[a].b, outs[b].p, outs[b].b), "view_mode: the outputs must not alias one another");
    // a start state may be the output it continues into (a workgroup reads its image's start before it writes), or lie clear of every output
    const struct { const void* p; size_t b; const void* own; } starts[] = {{mode_in, mb, mode_out}, {y_in, yb, y_out}};
    for (const auto& st : starts)
        for (const auto& o : outs)
            GRIP_REQUIRE(!st.p || !o.p || (st.p == o.p && o.p == st.own) || !overlap(st.p, st.b, o.p, o.b),
                         "view_mode: mode_in / y_in must not alias an output (mode_in may BE mode_out, y_in may BE y_out)");
    GRIP_REQUIRE(((uintptr_t)view_emb | (uintptr_t)mode_out | (uintptr_t)mode_in) % 16 == 0, "view_mode: view_emb, mode_in and mode_out must be 16-byte aligned");
    int r = (int)floor((double)rho * (double)(v - 1));
    r = r < 1 ? 1 : r;
    hipLaunchKernelGGL(view_mode_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, view_emb, view_probs, v, c, e, r, lam, lam_y, h2_floor, outer, inner, mode_in,
                       y_in, mode_out, y_out, h2_out);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}
