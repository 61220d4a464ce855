// Marginal entropy of an image's confident views and its gradient (include/grip_amd.h, grip_view_entropy; the loss of test-time prompt tuning, TPT: Shu et
// al., NeurIPS 2022, as the model of the header states it).  All f32 / int32.
//   per view p:   lse_p = max + logf(sum expf(x - max)),  p_pc = expf(x_pc - lse_p),  H_p = sum_c p_pc (lse_p - x_pc)         (every term >= 0)
//   selection:    the `keep` views of smallest H_p, ties to the lower index, a non-finite H_p after every finite one; a constant of the gradient
//   marginal:     pbar_c = (sum_{p selected, ascending} p_pc) / keep
//   loss_i = -sum_c pbar_c logf(max(pbar_c, 2^-126));   g_c = -(logf(max(pbar_c, 2^-126)) + 1) / keep
//   gradient:     a selected view  grad x_pj = (p_pj (g_j - sum_c p_pc g_c)) * (1 / n);  every other view +0.0
// view_entropy_kernel: ONE workgroup (four waves) per image, one launch for the per-image work, no workspace, no atomics, every sum in a fixed order.
//   1. a wave per view (views wave, wave + 4, ...): lane l adds the classes l, l + 64, ... in ascending order, then the DPP tree of wave_sum -- the bits of
//      lse_p and H_p depend on the row alone; both go to the LDS.
//   2. wave 0 ranks the <= 64 views, one lane per view (rank = the number of views that precede it), and a ballot packs the selected views, ascending,
//      into a list.  Then thread t owns the classes t, t + 256, ...: it adds the selected views' p_pc in ascending view order, divides by keep, writes
//      pbar_c out and g_c to the LDS, and adds its loss terms in ascending class order; wave_sum per wave, the four partials as ((a + b) + c) + d.
//   3. a wave per view again: a selected view forms its dot sum_c p_pc g_c as in 1 and writes its gradient row, any other view writes zeros: every element
//      of grad_logits has exactly one writer.
// An image's bits depend on its own [v, c] block (and keep) only: not on n, not on its place.  n enters ONCE, last, as the factor 1.0f / (float)n.
// The mean over n > 1 images is a second launch of one workgroup (the loss is [1] and there is no workspace to hand the per-image losses over in):
// view_entropy_mean_kernel re-adds every image's loss terms from mean_probs_out -- a wave per image with the SAME four-accumulator order, so loss_i has
// the bits the image's own workgroup formed -- or, when the caller passed no mean_probs_out, view_entropy_recompute_kernel walks the images through the
// same per-image function with every output off.  Either way the per-image losses are added in ascending i and multiplied by 1 / n.
#include <float.h>
#include <math.h>

#include "common.h"

namespace {
constexpr int VE_MAXV = 64;       // views per image at most (engine.VIEW_MODE_MAX_VIEWS): one lane per view in the ranking
constexpr int VE_MAXC = 16000;    // classes whose g_c fit the 64 KiB of LDS a kernel gets by default (the limit and the reason of grip_candidate_ce)

__device__ __forceinline__ float ve_wave_max(float v) {       // maximum over the 64 lanes in every lane (all lanes active)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

struct VeShared {
    float lse[VE_MAXV], H[VE_MAXV];
    int list[VE_MAXV];      // the selected views, ascending
    float part[4];
};

// acc - pbar log max(pbar, 2^-126), and the logarithm itself.  Contraction is off: the per-image workgroup and view_entropy_mean_kernel both inline it and
// must round alike (a product, then an addition).
__device__ __forceinline__ float ve_loss_add(float acc, float pbar, float& lg) {
#pragma clang fp contract(off)
    lg = logf(fmaxf(pbar, FLT_MIN));
    const float t = pbar * lg;
    return acc - t;
}

// The per-image work; every thread of the workgroup calls it.  Returns loss_i (valid in thread 0).  x: the image's [v, c] block; the outputs (each may
// be null) are the image's own rows.  Ends with a barrier: the LDS may be reused at once.
__device__ __forceinline__ float ve_image(const float* __restrict__ x, int v, int c, int keep, float inv_n, float* __restrict__ grad, float* __restrict__ ent_out,
                                          int32_t* __restrict__ sel_out, float* __restrict__ mean_out, VeShared& sh, float* g) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // 1. lse_p and H_p
    for (int p = wave; p < v; p += 4) {
        const float* xr = x + (size_t)p * c;
        float m = -INFINITY;
        for (int j = lane; j < c; j += 64) m = fmaxf(m, xr[j]);
        m = ve_wave_max(m);
        float sum = 0.f;
        for (int j = lane; j < c; j += 64) sum += expf(xr[j] - m);
        sum = wave_sum(sum);
        const float lse = m + logf(sum);
        float h = 0.f;
        for (int j = lane; j < c; j += 64) {
            const float d = lse - xr[j];      // >= 0: sum >= expf(0), so lse >= m >= x
            h += expf(-d) * d;
        }
        h = wave_sum(h);
        if (lane == 0) {
            sh.lse[p] = lse;
            sh.H[p] = h;
        }
    }
    __syncthreads();
    // 2. the selection (wave 0, lane p ranks view p) ...
    if (wave == 0) {
        const bool live = lane < v;
        const float hp = live ? sh.H[lane] : 0.f;
        const bool fp = hp - hp == 0.f;      // finite
        int rank = 0;
        for (int q = 0; q < v; ++q) {
            const float hq = sh.H[q];
            const bool fq = hq - hq == 0.f;
            const bool before = fq != fp ? fq : (fq && hq != hp) ? hq < hp : q < lane;
            rank += before ? 1 : 0;
        }
        const bool in = live && rank < keep;
        const unsigned long long bits = __ballot(in);
        if (in) sh.list[__popcll(bits & ((1ull << lane) - 1ull))] = lane;
        if (live) {
            if (ent_out) ent_out[lane] = hp;
            if (sel_out) sel_out[lane] = in ? 1 : 0;
        }
    }
    __syncthreads();
    // ... the marginal, g and the loss terms: thread t owns the classes t, t + 256, ...
    const float fkeep = (float)keep;
    float lt = 0.f;
    for (int j = tid; j < c; j += 256) {
        float s = 0.f;
        for (int k = 0; k < keep; ++k) {
            const int p = sh.list[k];
            s += expf(x[(size_t)p * c + j] - sh.lse[p]);
        }
        const float pbar = s / fkeep;
        float lg;
        lt = ve_loss_add(lt, pbar, lg);
        g[j] = -(lg + 1.0f) / fkeep;
        if (mean_out) mean_out[j] = pbar;
    }
    lt = wave_sum(lt);
    if (lane == 0) sh.part[wave] = lt;
    __syncthreads();
    const float loss_i = ((sh.part[0] + sh.part[1]) + sh.part[2]) + sh.part[3];
    // 3. the gradient rows: one writer per element
    if (grad) {
        for (int p = wave; p < v; p += 4) {
            // is view p selected?  (the list is ascending and short: every lane looks at one entry)
            const bool hit = lane < keep && sh.list[lane] == p;
            float* gr = grad + (size_t)p * c;
            if (__ballot(hit) == 0ull) {
                for (int j = lane; j < c; j += 64) gr[j] = 0.f;
                continue;
            }
            const float* xr = x + (size_t)p * c;
            const float lse = sh.lse[p];
            float dot = 0.f;
            for (int j = lane; j < c; j += 64) dot += expf(xr[j] - lse) * g[j];
            dot = wave_sum(dot);
            for (int j = lane; j < c; j += 64) gr[j] = (expf(xr[j] - lse) * (g[j] - dot)) * inv_n;
        }
    }
    __syncthreads();
    return loss_i;
}

__global__ __launch_bounds__(256) void view_entropy_kernel(const float* __restrict__ logits, int n, int v, int c, int keep, float inv_n, float* __restrict__ loss,
                                                           float* __restrict__ grad, float* __restrict__ ent_out, int32_t* __restrict__ sel_out,
                                                           float* __restrict__ mean_out) {
    extern __shared__ float g[];      // [c]
    __shared__ VeShared sh;
    const size_t img = blockIdx.x;
    const float l = ve_image(logits + img * (size_t)v * c, v, c, keep, inv_n, grad ? grad + img * (size_t)v * c : nullptr, ent_out ? ent_out + img * v : nullptr,
                             sel_out ? sel_out + img * v : nullptr, mean_out ? mean_out + img * (size_t)c : nullptr, sh, g);
    if (n == 1 && threadIdx.x == 0) loss[0] = l * inv_n;
}

// n > 1 with mean_probs_out: wave w re-adds the loss terms of the images w, w + 4, ... -- lane l keeps the four accumulators of the threads l, l + 64,
// l + 128, l + 192 of the image's own workgroup (classes l + 64 k + 256 m, m ascending), each goes through wave_sum, then ((a + b) + c) + d.
__global__ __launch_bounds__(256) void view_entropy_mean_kernel(const float* __restrict__ mean, int n, int c, float inv_n, float* __restrict__ loss) {
    __shared__ float part[4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float acc = 0.f;
    for (int base = 0; base < n; base += 4) {
        const int i = base + wave;
        if (i < n) {      // (per wave)
            const float* pb = mean + (size_t)i * c;
            float a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float t = 0.f, lg;
                for (int j = lane + 64 * k; j < c; j += 256) t = ve_loss_add(t, pb[j], lg);
                a[k] = wave_sum(t);
            }
            if (lane == 0) part[wave] = ((a[0] + a[1]) + a[2]) + a[3];
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 0; w < 4 && base + w < n; ++w) acc = base + w == 0 ? part[w] : acc + part[w];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = acc * inv_n;
}

// n > 1 without mean_probs_out: one workgroup walks the images with every output off
__global__ __launch_bounds__(256) void view_entropy_recompute_kernel(const float* __restrict__ logits, int n, int v, int c, int keep, float inv_n,
                                                                     float* __restrict__ loss) {
    extern __shared__ float g[];
    __shared__ VeShared sh;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) {
        const float l = ve_image(logits + (size_t)i * v * c, v, c, keep, inv_n, nullptr, nullptr, nullptr, nullptr, sh, g);
        acc = i == 0 ? l : acc + l;
    }
    if (threadIdx.x == 0) loss[0] = acc * inv_n;
}
bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}
}  // namespace

extern "C" int grip_view_entropy(const float* logits, int n, int v, int c, int keep, float* loss, float* grad_logits, float* view_entropy_out,
                                 int32_t* selected_out, float* mean_probs_out, void* stream) {
    GRIP_REQUIRE(logits && loss, "view_entropy: null pointer");
    GRIP_REQUIRE(n >= 1 && c >= 1, "view_entropy: empty input (n = %d, c = %d)", n, c);
    GRIP_REQUIRE(v >= 1 && v <= VE_MAXV, "view_entropy: v = %d (1 .. %d views)", v, VE_MAXV);
    GRIP_REQUIRE(keep >= 1 && keep <= v, "view_entropy: keep = %d (in [1, v = %d])", keep, v);
    GRIP_REQUIRE(c <= VE_MAXC, "view_entropy: c = %d (at most %d: g lives in the LDS)", c, VE_MAXC);
    const size_t xb = (size_t)n * v * c * 4, vb = (size_t)n * v * 4;
    const struct { const void* p; size_t b; } bufs[] = {{logits, xb}, {loss, 4}, {grad_logits, xb}, {view_entropy_out, vb}, {selected_out, vb},
                                                        {mean_probs_out, (size_t)n * c * 4}};
    for (int a = 0; a < 6; ++a)
        for (int b = a + 1; b < 6; ++b)
            GRIP_REQUIRE(!bufs[a].p || !bufs[b].p || !overlap(bufs[a].p, bufs[a].b, bufs[b].p, bufs[b].b),
                         "view_entropy: no output may alias logits or another output");
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)c * sizeof(float);
    const float inv_n = 1.0f / (float)n;
    hipLaunchKernelGGL(view_entropy_kernel, dim3(n), dim3(256), lds, s, logits, n, v, c, keep, inv_n, loss, grad_logits, view_entropy_out, selected_out,
                       mean_probs_out);
    GRIP_CHECK_HIP(hipGetLastError());
    if (n > 1) {
        if (mean_probs_out) hipLaunchKernelGGL(view_entropy_mean_kernel, dim3(1), dim3(256), 0, s, mean_probs_out, n, c, inv_n, loss);
        else hipLaunchKernelGGL(view_entropy_recompute_kernel, dim3(1), dim3(256), lds, s, logits, n, v, c, keep, inv_n, loss);
        GRIP_CHECK_HIP(hipGetLastError());
    }
    return GRIP_OK;
}
