// Train-time views on the GPU: RandomResizedCrop + RandomHorizontalFlip of the already-normalised f32 pool the strategies train on
// (the `augmentations=(aug1, aug2)` slot of the reference's datasets, data/dataset.py:18-79, which it fills on the host with PIL per item).
//   view v = crop the box [top, top + height) x [left, left + width) of image `row`, resample it to n_px x n_px with Pillow's antialiased
//   bicubic (a = -0.5), mirror left-right when `flip` is set.
// The coefficients are Pillow's precompute_coeffs applied to the BOX (crop() then resize(), taps clip at the box edge; nothing outside the box
// is read): evaluated and normalised in float64 on the device, rounded to f32 once, and held in LDS per output column / row of a tile -- never
// per element.  Two separable passes like Pillow's (horizontal, then vertical), both accumulating in f32.
//
// Work mapping: one workgroup of 256 threads owns a 32 x 32 output tile of one view, all three channels (the channels share every tap).
//   prologue    threads 0..31 / 32..63: (first tap, tap count, float64 weight sum) of the tile's 32 columns / 32 rows;
//   per chunk of AUG_RC source rows the tile's rows reach (one chunk for every box that is not shrunk: 32 rows need at most 36):
//     the vertical weights of the chunk's rows and, AUG_KC taps at a time, the horizontal weights go to LDS (one float64 evaluation per tap);
//     horizontal  thread (column j, slot): tmp[c][r][j] = sum_k wh[j][k] src[c][r][xmin_j + k] for the chunk's rows r = slot, slot + 8, ...:
//                 a wave reads 32 neighbouring columns of two rows, L1 / L2 hits after the first touch;
//     vertical    thread (4 columns, row y): acc[c][0..3] += wv[y][r] tmp[c][r][4 xq ..] -- one ds_read_b128 per four multiply-adds;
//   store       16 bytes per lane when n_px % 4 == 0 (and `out` is 16-byte aligned), scalar stores otherwise.
// Every loop over taps is bounded by the data: a box shrunk 100 times simply walks more chunks, LDS stays 22 KiB.  A flipped view is the same
// arithmetic on the mirrored column (the tile's column j takes the taps of column n_px - 1 - x), so it equals the mirror image bit for bit; the bits
// of a view depend on its own descriptor alone (tile origin and chunk origins are functions of the view, never of the launch).
// An identity box (height == width == n_px) has the weights 0, 1, 0, 0 exactly and is a bit-exact copy.
#include <type_traits>

#include "common.h"

namespace {
constexpr int AUG_T = 32;        // output tile edge
constexpr int AUG_RC = 40;       // source rows per chunk (>= 36: one chunk whenever the box is not shrunk)
constexpr int AUG_KC = 8;        // horizontal taps per chunk (>= 7: one chunk up to a 1.5 x shrink)

struct Axis {                    // Pillow's precompute_coeffs for one output index of one axis
    double center, ss;           // ss = 1 / filterscale
    int first, count;
};

__device__ __forceinline__ double bicubic(double x) {
    const double a = -0.5;
    x = fabs(x);
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Contraction off: `first` and `count` are truncations of these sums and must be the integers the host's float64 arithmetic gives.
__device__ __forceinline__ Axis axis_of(int xx, int in, int n_px) {
#pragma clang fp contract(off)
    const double scale = (double)in / (double)n_px;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs;
    Axis a;
    a.center = ((double)xx + 0.5) * scale;
    a.ss = 1.0 / fs;
    int lo = (int)(a.center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(a.center + support + 0.5);
    if (hi > in) hi = in;
    a.first = lo;
    a.count = hi - lo;
    return a;
}
__device__ __forceinline__ double tap(const Axis& a, int k) {       // un-normalised weight of tap k (input index first + k)
#pragma clang fp contract(off)
    return bicubic(((double)(k + a.first) - a.center + 0.5) * a.ss);
}
__device__ __forceinline__ double tap_sum(const Axis& a) {
    double s = 0.0;
    for (int k = 0; k < a.count; ++k) s += tap(a, k);
    return s;
}
__device__ __forceinline__ float tap_weight(const Axis& a, int k, double sum) {
    const double w = tap(a, k);
    return (float)(sum != 0.0 ? w / sum : w);
}

template <bool VEC>
__global__ __launch_bounds__(256) void augment_views_kernel(const float* __restrict__ src, int64_t n_src, int H, int W,
                                                            const grip_view* __restrict__ views, int n_px, int tiles, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tmp[3][AUG_RC][AUG_T];
    __shared__ float wh[AUG_T][AUG_KC];
    __shared__ float wv[AUG_T][AUG_RC];
    __shared__ double hsum[AUG_T], vsum[AUG_T];
    __shared__ int hfirst[AUG_T], hcount[AUG_T], vfirst[AUG_T], vcount[AUG_T];

    const int64_t v = blockIdx.x / (unsigned)(tiles * tiles);
    const int tile = blockIdx.x % (unsigned)(tiles * tiles);
    const int y0 = (tile / tiles) * AUG_T, x0 = (tile % tiles) * AUG_T;
    const grip_view vw = views[v];
    // a descriptor that does not lie inside the pool writes nothing (the host layer refuses such boxes before it launches)
    if (vw.row < 0 || vw.row >= n_src || vw.height < 1 || vw.width < 1 || vw.top < 0 || vw.left < 0 || vw.height > H - vw.top || vw.width > W - vw.left) return;
    const int t = threadIdx.x;

    // resized column of tile column j (mirrored when the view is flipped); -1 = outside the output
    auto column_of = [&](int j) { const int x = x0 + j; return x >= n_px ? -1 : (vw.flip ? n_px - 1 - x : x); };

    if (t < 2 * AUG_T) {
        const bool horiz = t < AUG_T;
        const int i = t & (AUG_T - 1);
        const int xx = horiz ? column_of(i) : (y0 + i < n_px ? y0 + i : -1);
        int first = 0, count = 0;
        double sum = 0.0;
        if (xx >= 0) {
            const Axis a = axis_of(xx, horiz ? vw.width : vw.height, n_px);
            first = a.first, count = a.count, sum = tap_sum(a);
        }
        if (horiz) hfirst[i] = first, hcount[i] = count, hsum[i] = sum;
        else vfirst[i] = first, vcount[i] = count, vsum[i] = sum;
    }
    __syncthreads();

    // block-uniform extents: the source rows the tile's rows reach, the longest horizontal window
    int r_lo = 0x7fffffff, r_hi = 0, k_max = 0;
    for (int i = 0; i < AUG_T; ++i) {
        if (vcount[i] > 0) {
            r_lo = min(r_lo, vfirst[i]);
            r_hi = max(r_hi, vfirst[i] + vcount[i]);
        }
        k_max = max(k_max, hcount[i]);
    }

    const int hj = t & (AUG_T - 1), hslot = t >> 5;           // horizontal pass: column, row slot (8 slots)
    const int xq = t & 7, vy = t >> 3;                        // vertical pass: column quad, row
    const int my_hfirst = hfirst[hj], my_hcount = hcount[hj];
    const int my_vfirst = vfirst[vy], my_vend = vfirst[vy] + vcount[vy];
    f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const float* box = src + ((int64_t)vw.row * 3 * H + vw.top) * W + vw.left;      // element (c, r, x) of the box: box[(c * H + r) * W + x]
    const int64_t plane = (int64_t)H * W;

    for (int r0 = r_lo; r0 < r_hi; r0 += AUG_RC) {
        const int rows = min(AUG_RC, r_hi - r0);
        {   // vertical weights of this chunk: thread (row vy, lane xq) takes the row's taps xq, xq + 8, ... that fall into the chunk
            const int lo = max(my_vfirst, r0), hi = min(my_vend, r0 + rows);
            if (lo < hi) {
                const Axis a = axis_of(y0 + vy, vw.height, n_px);
                const double sum = vsum[vy];
                for (int r = lo + xq; r < hi; r += 8) wv[vy][r - r0] = tap_weight(a, r - a.first, sum);
            }
        }
        for (int k0 = 0; k0 < k_max; k0 += AUG_KC) {
            if (k0 > 0) __syncthreads();        // the previous tap chunk's weights have been read
            {   // horizontal weights: thread (column t / 8, tap t % 8)
                const int j = t >> 3, k = k0 + (t & 7);
                float w = 0.f;
                if (k < hcount[j]) w = tap_weight(axis_of(column_of(j), vw.width, n_px), k, hsum[j]);
                wh[j][t & 7] = w;
            }
            __syncthreads();
            // Every tap of the chunk is loaded unconditionally (a predicated load per tap would wait for each one in turn): a tap beyond the column's window
            // has weight 0 and re-reads the window's last element, so nothing outside the box is touched.  Two unrolled forms: up to 5 taps (any box
            // that is not shrunk), up to AUG_KC.
            float w[AUG_KC];
            int col[AUG_KC];
#pragma unroll
            for (int k = 0; k < AUG_KC; ++k) {
                w[k] = wh[hj][k];
                col[k] = max(min(my_hfirst + k0 + k, my_hfirst + my_hcount - 1), 0);
            }
            auto rows_pass = [&](auto nk) {
                constexpr int NK = decltype(nk)::value;
                for (int rr = hslot; rr < rows; rr += 8) {
                    const float* p = box + (int64_t)(r0 + rr) * W;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float s = k0 == 0 ? 0.f : tmp[c][rr][hj];
#pragma unroll
                        for (int k = 0; k < NK; ++k) s = fmaf(w[k], p[c * plane + col[k]], s);
                        tmp[c][rr][hj] = s;
                    }
                }
            };
            if (k_max - k0 <= 5) rows_pass(std::integral_constant<int, 5>{});
            else rows_pass(std::integral_constant<int, AUG_KC>{});
        }
        __syncthreads();
        {
            const int lo = max(my_vfirst, r0), hi = min(my_vend, r0 + rows);
            for (int r = lo; r < hi; ++r) {
                const float wr = wv[vy][r - r0];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const f32x4 h = *(const f32x4*)&tmp[c][r - r0][4 * xq];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[c][e] = fmaf(wr, h[e], acc[c][e]);
                }
            }
        }
        __syncthreads();                        // tmp / wv / wh are rewritten by the next chunk
    }

    const int y = y0 + vy, x = x0 + 4 * xq;
    if (y >= n_px || x >= n_px) return;
    float* o = out + ((v * 3) * n_px + y) * (int64_t)n_px + x;
    const int64_t oplane = (int64_t)n_px * n_px;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (VEC) {
            *(f32x4*)(o + c * oplane) = acc[c];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < n_px) o[c * oplane + e] = acc[c][e];
        }
    }
}
}  // namespace

extern "C" int grip_augment_views(const float* src, int64_t n_src, int H, int W, const grip_view* views_device, int64_t n_views, int n_px,
                                  float* out, void* stream) {
    GRIP_REQUIRE(src && views_device && out && n_src > 0 && H > 0 && W > 0 && n_views > 0 && n_px > 0, "augment_views: bad arguments");
    const int64_t tiles = (n_px + AUG_T - 1) / AUG_T;
    GRIP_REQUIRE(tiles * tiles <= 0xffffff && n_views <= 0xffffff / (tiles * tiles), "augment_views: more than 2^24 - 1 tiles (2^32 threads) in one launch");
    const unsigned grid = (unsigned)(n_views * tiles * tiles);      // views ride on grid.x: no 65 535 limit
    const bool vec = n_px % 4 == 0 && ((uintptr_t)out & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(augment_views_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, n_src, H, W, views_device, n_px, (int)tiles, out);
    else
        hipLaunchKernelGGL(augment_views_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, n_src, H, W, views_device, n_px, (int)tiles, out);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}
