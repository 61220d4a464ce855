// Feature adapter (CLIP-Adapter, Gao et al., 2021): a bias-free bottleneck MLP on the image embedding, blended back into it,
//   x = ReLU(ReLU(F W1^T) W2^T),   out = ratio * x + (1 - ratio) * F,        F [n, e], W1 [h, e], W2 [e, h] (nn.Linear layout), all f32.
// Both products run on v_mfma_f32_16x16x4_f32 (the instruction of gemm_f32.hip / cache_head.hip: bitwise an fmaf chain per element).
//   * fa_fwd_kernel, ONE launch: a workgroup owns 64 image rows, a wave 16 of them.
//       phase 1  hidden = ReLU(F W1^T): the contraction over e is staged 32 floats at a time through two LDS buffers (64 x 32 of F and h x 32 of W1;
//                the global loads of step t + 1 are in flight during the MFMAs of step t, one barrier per step; 16-byte pieces XOR-swizzled with
//                (row & 7) as in gemm_f32.hip / cache_head.hip); a wave holds 16 rows x h in h / 16 accumulators.  ReLU in registers, and the
//                64 x h tile goes to LDS in the layout of the staged F tile (h / 32 chunks of [64][32], same swizzle) -- it never reaches memory
//                at inference.
//       phase 2  walks the e output columns 64 at a time: W2 rows are staged 64 x 32 through the same two buffers, the A operand is the hidden tile
//                in LDS; ReLU and the blend with F (loaded 16 bytes per lane during the tile's first stage) in registers, 16-byte stores.
//     A row's value is one k-ascending MFMA chain over e, ReLU, one chain over h, ReLU, one fmaf: its bits depend on that row, W1, W2 and ratio
//     only -- not on n, on the row's place in the tile or on the call.  Rows >= n are staged as zeros and never stored.  ratio = 0 gives F and
//     ratio = 1 gives x bit for bit (fmaf(ratio, x, (1 - ratio) * F) with x >= 0).  Training passes hidden_out / act_out and gets the two post-ReLU
//     tensors from the same registers.
//   * backward, TWO launches, no LDS, no atomics, no partial sums; every output element has one writer and is one MFMA chain in ascending row
//     (or column) order, so its bits are the same on every run and there is no grid-size decision that could change them:
//       fa_bwd_dh_gw2_kernel   workgroups 0 .. : dH = (dX W2) o [hidden > 0] into the workspace, dX = ratio * grad_out o [act > 0] formed on the fly
//                              (a wave: 16 rows x 16 columns of h, chain over e); the remaining workgroups: grad_w2 = dX^T hidden (a wave: 16 x 16
//                              of [e, h], chain over the n rows, four rows per MFMA, ascending);
//       fa_bwd_gw1_kernel      grad_w1 = dH^T F, same form.
//     Operands come straight from L2 (a training batch is 64 rows: 17 MFLOP), the next step's loads are in flight during the MFMAs of this one.
// LDS (forward, dynamic): 2 stages x (64 + max(h, 64)) x 128 B + the hidden tile ceil(h / 32) x 8 KiB:
//     h = 32: 40 KiB, h = 64: 48 KiB, h = 128: 80 KiB (two workgroups per CU), h = 192: 112 KiB, h = 256: 144 KiB (of the 160 KiB of a CU).
// Workspace (backward): n * h floats (dH) + 256 bytes of alignment slack.  No e * h partial exists, for any n.
#include <algorithm>

#include "common.h"

namespace {
constexpr int FA_BM = 64;        // image rows per workgroup (16 per wave)
constexpr int FA_BK = 32;        // floats per stage and row (one 128-byte line)
constexpr int FA_BN = 64;        // phase 2: output columns per tile
constexpr int FA_TILE = FA_BM * FA_BK;
constexpr int FA_MAX_E = 1024, FA_MAX_H = 256;

__host__ __device__ inline int fa_stage_floats(int h) { return (FA_BM + (h > FA_BN ? h : FA_BN)) * FA_BK; }
inline size_t fa_lds_bytes(int h) { return ((size_t)2 * fa_stage_floats(h) + (size_t)((h + 31) / 32) * FA_TILE) * sizeof(float); }

__device__ __forceinline__ f32x4 relu4(f32x4 v) {
    return (f32x4){v[0] > 0.f ? v[0] : 0.f, v[1] > 0.f ? v[1] : 0.f, v[2] > 0.f ? v[2] : 0.f, v[3] > 0.f ? v[3] : 0.f};
}

// NF: the h / 16 accumulators a wave is compiled for (h <= 16 NF); grid = ceil(n / 64)
template <int NF>
__global__ __launch_bounds__(256) void fa_fwd_kernel(const float* __restrict__ f, const float* __restrict__ w1, const float* __restrict__ w2, float ratio, int n,
                                                     int e, int h, float* __restrict__ out, float* __restrict__ hid_out, float* __restrict__ act_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int r0 = blockIdx.x * FA_BM;
    const int nf = h >> 4, stage = fa_stage_floats(h);
    float* Hs = lds + 2 * stage;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    int a_off[2], b_off[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int chunk = (kk * 4 + fgrp) ^ (lane & 7);
        a_off[kk] = (wave * 16 + frow) * FA_BK + chunk * 4;
        b_off[kk] = FA_TILE + frow * FA_BK + chunk * 4;
    }
    const int my_row = wave * 16 + frow, gr = r0 + my_row;

    // ---------------------------------------------------------------- phase 1: hidden = ReLU(F W1^T)
    // staging: thread t moves the 16-byte pieces t and t + 256 of the 64 x 32 tile of F and the pieces t + 256 i of the h x 32 tile of W1; rows >= n are zeros
    f32x4 fr[2], wr[NF / 2];
    auto gload1 = [&](int ec) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, col = ec * FA_BK + (id & 7) * 4;
            fr[i] = r0 + row < n ? *(const f32x4*)(f + (size_t)(r0 + row) * e + col) : zero;
        }
#pragma unroll
        for (int i = 0; i < NF / 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, col = ec * FA_BK + (id & 7) * 4;
            wr[i] = row < h ? *(const f32x4*)(w1 + (size_t)row * e + col) : zero;
        }
    };
    auto sstore1 = [&](int buf) {
        float* st = lds + buf * stage;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, ch = (id & 7) ^ (row & 7);
            *(f32x4*)(st + row * FA_BK + ch * 4) = fr[i];
        }
#pragma unroll
        for (int i = 0; i < NF / 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, ch = (id & 7) ^ (row & 7);
            if (row < h) *(f32x4*)(st + FA_TILE + row * FA_BK + ch * 4) = wr[i];
        }
    };

    constexpr int NA = NF < 4 ? 4 : NF;      // (the MFMA groups below are unrolled four accumulators at a time)
    f32x4 acc[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) acc[j] = zero;

    const int T1 = e / FA_BK;
    gload1(0);
    sstore1(0);
    __syncthreads();
    for (int t = 0; t < T1; ++t) {
        const int buf = t & 1;
        if (t + 1 < T1) gload1(t + 1);
        const float* st = lds + buf * stage;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const f32x4 af = *(const f32x4*)(st + a_off[kk]);
#pragma unroll
            for (int jg = 0; jg < NF; jg += 4) {
                if (jg < nf) {
                    f32x4 bf[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) bf[j] = (jg + j < nf) ? *(const f32x4*)(st + b_off[kk] + (jg + j) * 16 * FA_BK) : zero;
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (jg + j < nf) acc[jg + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][s], af[s], acc[jg + j], 0, 0, 0);
                }
            }
        }
        if (t + 1 < T1) sstore1(buf ^ 1);
        __syncthreads();
    }
    // lane (frow, fgrp) holds the pre-activations of row wave*16 + frow, hidden columns j*16 + fgrp*4 + {0..3}
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        if (j < nf) {
            const f32x4 v = relu4(acc[j]);
            const int ch = ((j & 1) * 4 + fgrp) ^ (lane & 7);
            *(f32x4*)(Hs + (j >> 1) * FA_TILE + my_row * FA_BK + ch * 4) = v;
            if (hid_out && gr < n) *(f32x4*)(hid_out + (size_t)gr * h + j * 16 + fgrp * 4) = v;
        }
    }

    // ---------------------------------------------------------------- phase 2: out = ratio * ReLU(hidden W2^T) + (1 - ratio) * F, 64 columns at a time
    const int nks = (h + FA_BK - 1) / FA_BK, T2 = (e / FA_BN) * nks;
    f32x4 w2r[2];
    auto gload2 = [&](int ct, int ks) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, col = ks * FA_BK + (id & 7) * 4;
            w2r[i] = col < h ? *(const f32x4*)(w2 + (size_t)(ct * FA_BN + row) * h + col) : zero;
        }
    };
    auto sstore2 = [&](int buf) {
        float* st = lds + buf * stage + FA_TILE;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, ch = (id & 7) ^ (row & 7);
            *(f32x4*)(st + row * FA_BK + ch * 4) = w2r[i];
        }
    };
    const float keep = 1.0f - ratio;
    f32x4 o[4], fb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fb[j] = zero;

    gload2(0, 0);      // (every wave has passed the last barrier of phase 1: no wave still reads a stage)
    sstore2(0);
    __syncthreads();   // also orders the hidden tile's stores before its reads
    int ct = 0, ks = 0;
    for (int t = 0; t < T2; ++t) {
        const int buf = t & 1;
        int nct = ct, nk = ks + 1;
        if (nk == nks) { nk = 0; ++nct; }
        if (t + 1 < T2) gload2(nct, nk);
        if (ks == 0 && gr < n) {
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = *(const f32x4*)(f + (size_t)gr * e + ct * FA_BN + j * 16 + fgrp * 4);
        }
        const float* st = lds + buf * stage;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            if (ks * 2 + kk < nf) {
                f32x4 bf[4];
                const f32x4 af = *(const f32x4*)(Hs + ks * FA_TILE + a_off[kk]);
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[j] = *(const f32x4*)(st + b_off[kk] + j * 16 * FA_BK);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][s], af[s], o[j], 0, 0, 0);
            }
        }
        if (t + 1 < T2) sstore2(buf ^ 1);
        if (ks == nks - 1) {
            // lane (frow, fgrp) holds row wave*16 + frow, output columns ct*64 + j*16 + fgrp*4 + {0..3}
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 x = relu4(o[j]);
                o[j] = zero;
                if (gr < n) {
                    const size_t at = (size_t)gr * e + ct * FA_BN + j * 16 + fgrp * 4;
                    f32x4 y;
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[r] = __builtin_fmaf(ratio, x[r], keep * fb[j][r]);
                    *(f32x4*)(out + at) = y;
                    if (act_out) *(f32x4*)(act_out + at) = x;
                }
            }
        }
        ct = nct;
        ks = nk;
        __syncthreads();
    }
}

// dX[row][col .. col + 3] = ratio * grad_out o [act > 0]
__device__ __forceinline__ f32x4 fa_dx4(const float* __restrict__ g, const float* __restrict__ act, size_t at, float ratio) {
    const f32x4 gv = *(const f32x4*)(g + at), av = *(const f32x4*)(act + at);
    return (f32x4){av[0] > 0.f ? ratio * gv[0] : 0.f, av[1] > 0.f ? ratio * gv[1] : 0.f, av[2] > 0.f ? ratio * gv[2] : 0.f, av[3] > 0.f ? ratio * gv[3] : 0.f};
}

// One wave = one 16 x 16 tile of C[i][j] = sum over the n rows of P[row][i0 + i] * Q[row][j0 + j], rows ascending, four per MFMA.
//   GW1 = false:  P = hidden [n, h], Q = dX (from grad_out / act, [n, e])       -> grad_w2 [e, h]: C^T stored, 16 bytes per lane along h
//   GW1 = true :  P = img_emb [n, e], Q = dH [n, h]                             -> grad_w1 [h, e]: C^T stored, 16 bytes per lane along e
// lane (frow, fgrp): MFMA s of a 16-row step takes row rb + 4 s + fgrp; A = P[row][i0 + frow], B = Q[row][j0 + frow]; D[i = fgrp*4 + r][j = frow].
template <bool GW1>
__device__ __forceinline__ void fa_rows_tile(const float* __restrict__ P, int ldp, const float* __restrict__ Q, const float* __restrict__ Qact, int ldq, float ratio,
                                             int n, int i0, int j0, float* __restrict__ C, int ldc) {
    const int lane = threadIdx.x & 63, frow = lane & 15, fgrp = lane >> 4;
    float a[4], b[4], an[4] = {0.f, 0.f, 0.f, 0.f}, bn[4] = {0.f, 0.f, 0.f, 0.f};
    auto load = [&](int rb, float (&av)[4], float (&bv)[4]) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = rb + 4 * s + fgrp;
            const bool ok = row < n;
            const size_t rr = (size_t)(ok ? row : 0);
            const float pv = P[rr * ldp + i0 + frow];
            float qv = Q[rr * ldq + j0 + frow];
            if (!GW1) qv = Qact[rr * ldq + j0 + frow] > 0.f ? ratio * qv : 0.f;
            av[s] = ok ? pv : 0.f;
            bv[s] = ok ? qv : 0.f;
        }
    };
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    load(0, a, b);
    for (int rb = 0; rb < n; rb += 16) {
        if (rb + 16 < n) load(rb + 16, an, bn);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) { a[s] = an[s]; b[s] = bn[s]; }
    }
    *(f32x4*)(C + (size_t)(j0 + frow) * ldc + i0 + fgrp * 4) = acc;
}

// workgroups 0 .. dh_blocks - 1: dH; the rest: grad_w2.  A wave works alone (no LDS, no barrier).
__global__ __launch_bounds__(256) void fa_bwd_dh_gw2_kernel(const float* __restrict__ w2, const float* __restrict__ hidden, const float* __restrict__ act,
                                                            const float* __restrict__ g, float ratio, int n, int e, int h, float* __restrict__ dH,
                                                            float* __restrict__ grad_w2, int dh_blocks) {
    const int lane = threadIdx.x & 63, frow = lane & 15, fgrp = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hf = h >> 4;
    if ((int)blockIdx.x < dh_blocks) {
        // dH[rows rb .. rb + 15][hc0 .. hc0 + 15] = (dX W2) o [hidden > 0]:  A[i = h column][k] = W2[k][hc0 + i],  B[k][j = row] = dX[row][k],
        // MFMA s of a 16-column step of e takes k = kb + fgrp*4 + s (one 16-byte load of grad_out and of act per step and lane)
        const int wt = blockIdx.x * 4 + wave, rb = (wt / hf) * 16, hc0 = (wt % hf) * 16;
        if (rb >= n) return;
        const int row = rb + frow;
        const bool ok = row < n;
        const size_t rbase = (size_t)(ok ? row : 0) * e;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        float a[4], an[4] = {0.f, 0.f, 0.f, 0.f};
        f32x4 b, bn = zero;
        auto load = [&](int kb, float (&av)[4], f32x4& bv) {
#pragma unroll
            for (int s = 0; s < 4; ++s) av[s] = w2[(size_t)(kb + fgrp * 4 + s) * h + hc0 + frow];
            const f32x4 d = fa_dx4(g, act, rbase + kb + fgrp * 4, ratio);
            bv = ok ? d : zero;
        };
        f32x4 acc = zero;
        load(0, a, b);
        for (int kb = 0; kb < e; kb += 16) {
            if (kb + 16 < e) load(kb + 16, an, bn);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
#pragma unroll
            for (int s = 0; s < 4; ++s) a[s] = an[s];
            b = bn;
        }
        // lane (frow, fgrp) holds dH[rb + frow][hc0 + fgrp*4 + {0..3}]
        if (ok) {
            const size_t at = (size_t)row * h + hc0 + fgrp * 4;
            const f32x4 hv = *(const f32x4*)(hidden + at);
            *(f32x4*)(dH + at) = (f32x4){hv[0] > 0.f ? acc[0] : 0.f, hv[1] > 0.f ? acc[1] : 0.f, hv[2] > 0.f ? acc[2] : 0.f, hv[3] > 0.f ? acc[3] : 0.f};
        }
        return;
    }
    const int wt = (blockIdx.x - dh_blocks) * 4 + wave;      // tile (e columns wt / hf, h columns wt % hf) of grad_w2 [e, h]
    if (wt >= (e >> 4) * hf) return;
    fa_rows_tile<false>(hidden, h, g, act, e, ratio, n, (wt % hf) * 16, (wt / hf) * 16, grad_w2, h);
}

__global__ __launch_bounds__(256) void fa_bwd_gw1_kernel(const float* __restrict__ f, const float* __restrict__ dH, int n, int e, int h,
                                                         float* __restrict__ grad_w1) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ef = e >> 4, wt = blockIdx.x * 4 + wave;       // tile (h columns wt / ef, e columns wt % ef) of grad_w1 [h, e]
    if (wt >= ef * (h >> 4)) return;
    fa_rows_tile<true>(f, e, dH, nullptr, h, 0.f, n, (wt % ef) * 16, (wt / ef) * 16, grad_w1, e);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_adapter(const char* who, int n, int e, int h) {
    GRIP_REQUIRE(n > 0, "%s: n = %d (must be positive)", who, n);
    GRIP_REQUIRE(e >= 64 && e <= FA_MAX_E && e % 64 == 0, "%s: e = %d (a multiple of 64, 64 .. %d)", who, e, FA_MAX_E);
    GRIP_REQUIRE(h >= 16 && h <= FA_MAX_H && h % 16 == 0, "%s: h = %d (a multiple of 16, 16 .. %d)", who, h, FA_MAX_H);
    return GRIP_OK;
}
size_t adapter_ws_bytes(int n, int h) { return (size_t)n * h * sizeof(float) + 256; }

template <int NF>
int launch_fwd(const float* f, const float* w1, const float* w2, float ratio, int n, int e, int h, float* out, float* hid, float* act, hipStream_t s) {
    static size_t configured = 0;
    const size_t lds = fa_lds_bytes(h);
    if (lds > configured) {
        GRIP_CHECK_HIP(hipFuncSetAttribute((const void*)fa_fwd_kernel<NF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        configured = lds;
    }
    hipLaunchKernelGGL(fa_fwd_kernel<NF>, dim3((n + FA_BM - 1) / FA_BM), dim3(256), lds, s, f, w1, w2, ratio, n, e, h, out, hid, act);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}
}  // namespace

#define RUNC(x) do { int _rc = (x); if (_rc != GRIP_OK) return _rc; } while (0)

extern "C" int grip_feature_adapter_workspace(int n, int e, int h, size_t* bytes) {
    GRIP_REQUIRE(bytes, "feature_adapter_workspace: null pointer");
    RUNC(check_adapter("feature_adapter_workspace", n, e, h));
    *bytes = adapter_ws_bytes(n, h);
    return GRIP_OK;
}

extern "C" int grip_feature_adapter_forward(const float* img_emb, const float* w1, const float* w2, float ratio, int n, int e, int h, float* out,
                                            float* hidden_out, float* act_out, void* stream) {
    RUNC(check_adapter("feature_adapter_forward", n, e, h));
    GRIP_REQUIRE(img_emb && w1 && w2 && out, "feature_adapter_forward: null pointer");
    GRIP_REQUIRE((hidden_out == nullptr) == (act_out == nullptr), "feature_adapter_forward: hidden_out and act_out are given together (training) or both null");
    GRIP_REQUIRE(out != img_emb, "feature_adapter_forward: out must not alias img_emb");
    GRIP_REQUIRE(aligned16(img_emb) && aligned16(w1) && aligned16(w2) && aligned16(out) && aligned16(hidden_out) && aligned16(act_out),
                 "feature_adapter_forward: every tensor must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (h <= 32) return launch_fwd<2>(img_emb, w1, w2, ratio, n, e, h, out, hidden_out, act_out, s);
    if (h <= 64) return launch_fwd<4>(img_emb, w1, w2, ratio, n, e, h, out, hidden_out, act_out, s);
    if (h <= 128) return launch_fwd<8>(img_emb, w1, w2, ratio, n, e, h, out, hidden_out, act_out, s);
    if (h <= 192) return launch_fwd<12>(img_emb, w1, w2, ratio, n, e, h, out, hidden_out, act_out, s);
    return launch_fwd<16>(img_emb, w1, w2, ratio, n, e, h, out, hidden_out, act_out, s);
}

extern "C" int grip_feature_adapter_backward(const float* img_emb, const float* w2, const float* hidden, const float* act, const float* grad_out, float ratio,
                                             int n, int e, int h, float* grad_w1, float* grad_w2, void* workspace, size_t workspace_bytes, void* stream) {
    RUNC(check_adapter("feature_adapter_backward", n, e, h));
    GRIP_REQUIRE(img_emb && w2 && hidden && act && grad_out && grad_w1 && grad_w2 && workspace, "feature_adapter_backward: null pointer");
    GRIP_REQUIRE(aligned16(img_emb) && aligned16(w2) && aligned16(hidden) && aligned16(act) && aligned16(grad_out) && aligned16(grad_w1) && aligned16(grad_w2),
                 "feature_adapter_backward: every tensor must be 16-byte aligned");
    GRIP_REQUIRE(workspace_bytes >= adapter_ws_bytes(n, h), "feature_adapter_backward: workspace too small (%zu bytes, grip_feature_adapter_workspace says %zu)",
                 workspace_bytes, adapter_ws_bytes(n, h));
    float* dH = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    hipStream_t s = (hipStream_t)stream;
    const int hf = h / 16, ef = e / 16;
    const int dh_blocks = (int)(((int64_t)((n + 15) / 16) * hf + 3) / 4), w_blocks = (ef * hf + 3) / 4;
    hipLaunchKernelGGL(fa_bwd_dh_gw2_kernel, dim3(dh_blocks + w_blocks), dim3(256), 0, s, w2, hidden, act, grad_out, ratio, n, e, h, dH, grad_w2, dh_blocks);
    GRIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(fa_bwd_gw1_kernel, dim3(w_blocks), dim3(256), 0, s, img_emb, dH, n, e, h, grad_w1);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}
