// MaPLe coupling function (Khattak et al., CVPR 2023): every visual prompt is a trainable Linear of the text prompt of the same depth,
//   Y[l] = X[l] W[l]^T + b[l],   l = 0 (shallow: X = ctx, Y = vis_prefix) and l = 1 .. n_deep (X = deep_text[l - 1], Y = vis_deep[l - 1]),
// W [1 + n_deep, dv, dt] f32 with independent weights per depth.  With P <= 16 rows per matrix the work is the WEIGHT STREAM (ViT-B/16, n_deep = 11:
// 18.9 MB of W forward, W + d_w backward), so the kernels are shaped by bytes, not by launches or FLOPs:
//   * every element of W is read once per direction and d_w is written once, 16 bytes per lane, 1 KB contiguous per wave-instruction; there is no
//     transposed copy of W (the UPT mixer's backward rebuilds one per step: right for its 2 MB, 38 MB of extra traffic here);
//   * all depths share one launch: forward = 1 launch, backward = 2 (the products, then the fixed-order sum of the dX partials);
//   * forward: a wave owns output columns n (rows of W, contiguous in k), the P x dt operand rows sit in LDS, a cross-lane sum per (p, n);
//   * backward: a wave owns a 256-float slice of k and walks rows n of W.  It holds X[:, slice] in registers, so the row of W it has just loaded
//     gives d_w[n, slice] = sum_p dY[p, n] X[p, slice] (stored at once) AND its share of dX[p, slice] += dY[p, n] W[n, slice] (kept in registers):
//     both products from one pass over W.  The walk over dv is split over the waves of a workgroup and over workgroups (CPL_BROWS rows each);
//     the partial dX of a workgroup is the sum of its waves in wave order (through LDS), and couple_dx_kernel adds the workgroups' partials in
//     workgroup order.  No atomics, one writer per element: the same bits on every run.
// Parameters and arithmetic are f32 (MaPLe's fp16 rounding points are not modelled).
#include "common.h"

namespace {
constexpr int CPL_MAX_P = 16;        // prompt tokens
constexpr int CPL_MAX_DEEP = 31;     // deep prompt sets
constexpr int CPL_MAX_WIDTH = 1024;  // forward: the [16, text_width] operand rows are one LDS tile of at most 64 KB
constexpr int CPL_FCOLS = 16;        // forward: output columns per workgroup (4 per wave, two at a time)
constexpr int CPL_BROWS = 32;        // backward: rows of W per workgroup (8 per wave)

// Accumulators are sized by PT = 4, 8 or 16 >= P; rows p >= P are zeros (their sums are never stored).
template <int PT>
__global__ __launch_bounds__(256) void couple_fwd_kernel(const float* __restrict__ ctx, const float* __restrict__ deep, const float* __restrict__ w,
                                                         const float* __restrict__ b, float* __restrict__ y0, float* __restrict__ yd, int P, int dt, int dv) {
    extern __shared__ __attribute__((aligned(16))) float Xs[];      // [PT][dt]
    const int l = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, dt4 = dt >> 2;
    const f32x4* X4 = (const f32x4*)(l == 0 ? ctx : deep + (size_t)(l - 1) * P * dt);
    float* Y = l == 0 ? y0 : yd + (size_t)(l - 1) * P * dv;
    f32x4* Xs4 = (f32x4*)Xs;
    for (int i = threadIdx.x; i < PT * dt4; i += 256) Xs4[i] = i < P * dt4 ? X4[i] : (f32x4){0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    const float* bl = b + (size_t)l * dv;
    for (int c = 0; c < 4; c += 2) {
        const int n = blockIdx.x * CPL_FCOLS + wave * 4 + c;
        const f32x4* w0 = (const f32x4*)(w + ((size_t)l * dv + n) * dt);
        const f32x4* w1 = w0 + dt4;
        float a0[PT], a1[PT];
#pragma unroll
        for (int p = 0; p < PT; ++p) a0[p] = a1[p] = 0.f;
        for (int i = lane; i < dt4; i += 64) {
            const f32x4 u = w0[i], v = w1[i];
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                const f32x4 x = Xs4[p * dt4 + i];
                a0[p] += x[0] * u[0] + x[1] * u[1] + x[2] * u[2] + x[3] * u[3];
                a1[p] += x[0] * v[0] + x[1] * v[1] + x[2] * v[2] + x[3] * v[3];
            }
        }
        float o0 = 0.f, o1 = 0.f;       // lane p keeps row p's two sums
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            const float s0 = wave_sum(a0[p]), s1 = wave_sum(a1[p]);
            if (lane == p) { o0 = s0; o1 = s1; }
        }
        if (lane < P) {
            Y[(size_t)lane * dv + n] = o0 + bl[n];
            Y[(size_t)lane * dv + n + 1] = o1 + bl[n + 1];
        }
    }
}

// grid (k slices of 256 floats, dv / CPL_BROWS row chunks, 1 + n_deep).  part [1 + n_deep][chunks][P][dt]
template <int PT>
__global__ __launch_bounds__(256) void couple_bwd_kernel(const float* __restrict__ ctx, const float* __restrict__ deep, const float* __restrict__ w,
                                                         const float* __restrict__ dy0, const float* __restrict__ dyd, float* __restrict__ d_w,
                                                         float* __restrict__ d_b, float* __restrict__ part, int P, int dt, int dv) {
    __shared__ __attribute__((aligned(16))) float dys[CPL_BROWS][PT];       // dY[:, chunk] transposed: a row of W finds its PT factors side by side
    __shared__ f32x4 red[3][PT][64];
    const int s = blockIdx.x, c = blockIdx.y, l = blockIdx.z, C = gridDim.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, dt4 = dt >> 2;
    const f32x4* X4 = (const f32x4*)(l == 0 ? ctx : deep + (size_t)(l - 1) * P * dt);
    const float* dY = l == 0 ? dy0 : dyd + (size_t)(l - 1) * P * dv;
    const int r0 = c * CPL_BROWS;
    for (int i = threadIdx.x; i < CPL_BROWS * PT; i += 256) {
        const int p = i / CPL_BROWS, r = i % CPL_BROWS;
        dys[r][p] = p < P ? dY[(size_t)p * dv + r0 + r] : 0.f;
    }
    __syncthreads();
    if (s == 0 && threadIdx.x < CPL_BROWS) {       // d_b[n] = sum_p dY[p, n], in p order
        float sum = 0.f;
#pragma unroll
        for (int p = 0; p < PT; ++p) sum += dys[threadIdx.x][p];
        d_b[(size_t)l * dv + r0 + threadIdx.x] = sum;
    }
    const int k4 = s * 64 + lane;
    const bool act = k4 < dt4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 x[PT], acc[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        x[p] = act && p < P ? X4[p * dt4 + k4] : zero;
        acc[p] = zero;
    }
    if (act) {
        const size_t row = ((size_t)l * dv + r0 + wave * 8) * dt4 + k4;
        const f32x4* Wr = (const f32x4*)w + row;
        f32x4* dWr = (f32x4*)d_w + row;
        f32x4 wv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) wv[j] = Wr[(size_t)j * dt4];       // the wave's eight rows in flight together
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float* g = dys[wave * 8 + j];
            f32x4 dw = zero;
#pragma unroll
            for (int p = 0; p < PT; ++p) {
                const float gp = g[p];
                acc[p] += gp * wv[j];
                dw += gp * x[p];
            }
            dWr[(size_t)j * dt4] = dw;
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int p = 0; p < PT; ++p) red[wave - 1][p][lane] = acc[p];
    }
    __syncthreads();
    if (wave == 0 && act) {
        f32x4* out = (f32x4*)part + ((size_t)l * C + c) * P * dt4 + k4;
#pragma unroll
        for (int p = 0; p < PT; ++p)
            if (p < P) out[(size_t)p * dt4] = ((acc[p] + red[0][p][lane]) + red[1][p][lane]) + red[2][p][lane];
    }
}

// dX[l][p][k] = sum over the row chunks c, in chunk order; one thread per four k
__global__ __launch_bounds__(256) void couple_dx_kernel(const float* __restrict__ part, float* __restrict__ d_ctx, float* __restrict__ d_deep, int P, int L, int C, int dt4) {
    const int i = blockIdx.x * 256 + threadIdx.x, per = P * dt4;
    if (i >= L * per) return;
    const int l = i / per, r = i % per;
    const f32x4* src = (const f32x4*)part + (size_t)l * C * per + r;
    f32x4 sum = src[0];
    for (int c = 1; c < C; ++c) sum += src[(size_t)c * per];
    f32x4* dst = l == 0 ? (f32x4*)d_ctx + r : (f32x4*)d_deep + (size_t)(l - 1) * per + r;
    *dst = sum;
}

int check_couple(const char* who, int P, int D, int dt, int dv) {
    GRIP_REQUIRE(P >= 1 && P <= CPL_MAX_P, "%s: n_prompt = %d (1 .. %d prompt tokens)", who, P, CPL_MAX_P);
    GRIP_REQUIRE(D >= 0 && D <= CPL_MAX_DEEP, "%s: n_deep = %d out of range (0 .. %d deep prompt sets)", who, D, CPL_MAX_DEEP);
    GRIP_REQUIRE(dt >= 64 && dt <= CPL_MAX_WIDTH && dt % 64 == 0 && dv >= 64 && dv <= CPL_MAX_WIDTH && dv % 64 == 0,
                 "%s: widths %d / %d (text / vision: multiples of 64, 64 .. %d)", who, dt, dv, CPL_MAX_WIDTH);
    return GRIP_OK;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
size_t part_floats(int P, int D, int dt, int dv) { return (size_t)(1 + D) * (dv / CPL_BROWS) * P * dt; }
}  // namespace

#define RUNC(x) do { int _rc = (x); if (_rc != GRIP_OK) return _rc; } while (0)

extern "C" int grip_prompt_couple_workspace(int n_prompt, int n_deep, int text_width, int vision_width, size_t* bytes) {
    GRIP_REQUIRE(bytes, "prompt_couple_workspace: null pointer");
    RUNC(check_couple("prompt_couple_workspace", n_prompt, n_deep, text_width, vision_width));
    *bytes = part_floats(n_prompt, n_deep, text_width, vision_width) * sizeof(float) + 256;
    return GRIP_OK;
}

extern "C" int grip_prompt_couple_forward(const float* ctx, const float* deep_text, int n_prompt, int n_deep, int text_width, int vision_width, const float* w,
                                          const float* b, float* vis_prefix, float* vis_deep, void* stream) {
    RUNC(check_couple("prompt_couple_forward", n_prompt, n_deep, text_width, vision_width));
    GRIP_REQUIRE(ctx && w && b && vis_prefix, "prompt_couple_forward: null pointer");
    GRIP_REQUIRE(n_deep == 0 || (deep_text && vis_deep), "prompt_couple_forward: null deep_text / vis_deep with n_deep = %d", n_deep);
    GRIP_REQUIRE(aligned16(ctx) && aligned16(deep_text) && aligned16(w), "prompt_couple_forward: ctx, deep_text and w must be 16-byte aligned");
    const int P = n_prompt, dt = text_width, dv = vision_width, PT = P <= 4 ? 4 : P <= 8 ? 8 : 16;
    const size_t lds = (size_t)PT * dt * sizeof(float);
    const dim3 grid(dv / CPL_FCOLS, 1 + n_deep);
    hipStream_t s = (hipStream_t)stream;
    static size_t configured[3] = {0, 0, 0};
#define CPL_FWD(pt, slot)                                                                                                                                   \
    do {                                                                                                                                                    \
        if (lds > configured[slot]) {                                                                                                                       \
            GRIP_CHECK_HIP(hipFuncSetAttribute((const void*)couple_fwd_kernel<pt>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                  \
            configured[slot] = lds;                                                                                                                         \
        }                                                                                                                                                   \
        hipLaunchKernelGGL(couple_fwd_kernel<pt>, grid, dim3(256), lds, s, ctx, deep_text, w, b, vis_prefix, vis_deep, P, dt, dv);                          \
    } while (0)
    if (PT == 4) CPL_FWD(4, 0);
    else if (PT == 8) CPL_FWD(8, 1);
    else CPL_FWD(16, 2);
#undef CPL_FWD
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}

extern "C" int grip_prompt_couple_backward(const float* ctx, const float* deep_text, int n_prompt, int n_deep, int text_width, int vision_width, const float* w,
                                           const float* d_vis_prefix, const float* d_vis_deep, float* d_ctx, float* d_deep_text, float* d_w, float* d_b,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    RUNC(check_couple("prompt_couple_backward", n_prompt, n_deep, text_width, vision_width));
    GRIP_REQUIRE(ctx && w && d_vis_prefix && d_ctx && d_w && d_b && workspace, "prompt_couple_backward: null pointer");
    GRIP_REQUIRE(n_deep == 0 || (deep_text && d_vis_deep && d_deep_text), "prompt_couple_backward: null deep_text / d_vis_deep / d_deep_text with n_deep = %d", n_deep);
    GRIP_REQUIRE(aligned16(ctx) && aligned16(deep_text) && aligned16(w) && aligned16(d_ctx) && aligned16(d_deep_text) && aligned16(d_w),
                 "prompt_couple_backward: ctx, deep_text, w and their gradients must be 16-byte aligned");
    const int P = n_prompt, dt = text_width, dv = vision_width, L = 1 + n_deep, C = dv / CPL_BROWS, dt4 = dt / 4;
    float* part = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    GRIP_REQUIRE((char*)part + part_floats(P, n_deep, dt, dv) * sizeof(float) <= (char*)workspace + workspace_bytes, "prompt_couple_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((dt4 + 63) / 64, C, L);
    if (P <= 4) hipLaunchKernelGGL(couple_bwd_kernel<4>, grid, dim3(256), 0, s, ctx, deep_text, w, d_vis_prefix, d_vis_deep, d_w, d_b, part, P, dt, dv);
    else if (P <= 8) hipLaunchKernelGGL(couple_bwd_kernel<8>, grid, dim3(256), 0, s, ctx, deep_text, w, d_vis_prefix, d_vis_deep, d_w, d_b, part, P, dt, dv);
    else hipLaunchKernelGGL(couple_bwd_kernel<16>, grid, dim3(256), 0, s, ctx, deep_text, w, d_vis_prefix, d_vis_deep, d_w, d_b, part, P, dt, dv);
    GRIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(couple_dx_kernel, dim3((L * P * dt4 + 255) / 256), dim3(256), 0, s, part, d_ctx, d_deep_text, P, L, C, dt4);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}
