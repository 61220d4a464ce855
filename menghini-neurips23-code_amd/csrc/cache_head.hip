// Key/value cache head (Tip-Adapter, Zhang et al., ECCV 2022): the training set's image embeddings are the keys, their (pseudo)labels the values, and
//   out[i, y] = logits[i, y] + alpha * sum_{j in class y} v_j exp(-beta (1 - f^_i . k_j)),    f^_i = f_i / |f_i|,
// keys [m, e] grouped by class (class_start [c + 1]) and used as stored.  All f32.  n x m x e is a GEMM (84 GFLOP at 50 000 x 1 632 x 512), so the
// products run on v_mfma_f32_16x16x4_f32 (the instruction of gemm_f32.hip); what is specific to the head is the epilogue, which never leaves the chip:
//   * cache_rnorm_kernel: 1 / |f_i| per row into the workspace (one wave per row); it is applied to the SCORE, img_emb is never copied or normalised;
//   * cache_fwd_kernel: a workgroup owns 64 image rows and walks the keys 64 at a time.  Per key tile the contraction over e is staged 32 floats at a
//     time through two LDS buffers (global loads of step t + 1 are in flight during the MFMAs of step t; one barrier per step); each wave holds
//     16 rows x 64 keys in four accumulators.  At the end of a key tile exp and alpha * v_j are applied in registers, the 64 x 64 tile goes to LDS, and
//     the classes that the tile touches are summed there: thread (row, q) takes the tile's classes q, q + 4, ... and adds its keys IN KEY ORDER.  A class
//     that runs over the tile's end hands its partial sum to the next tile through an LDS carry, so every class is added to its logit exactly once, by
//     one thread, as ((0 + a_first) + ...) + a_last: no atomics, no [rows, c] accumulator (any c >= 1), the [n, m] affinity never exists in memory.
//     A row's bits depend on its own operands only (the MFMA chain over e and the key-order sum): not on n, not on the call it is in.  With few row
//     tiles (a training batch is ONE) the classes are dealt to up to m / 64 workgroups per row tile, each walking the keys of whole classes; tile
//     boundaries move with that split and no bit does.
//   * cache_bwd_kernel: dK = dS^T F^ with dS_ij = alpha beta v_j G[i, y(j)] A_ij, one workgroup per 16 keys (x 512 columns of e): 102 workgroups at
//     m = 1 632.  Per 64 training rows it recomputes the 64 x 16 scores (same MFMA chain as the forward, operands straight from L2: n is 16 .. 256),
//     writes dS_ij / |f_i| to LDS and contracts it with the rows of img_emb into 16 x 512 accumulators; rows in ascending order, one writer per element.
// LDS: forward 2 x 16 KiB stages + 16.25 KiB affinity tile + 512 B carry = 48.8 KiB (three workgroups per CU); backward 4.3 KiB.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {
constexpr int CH_BM = 64;                         // image rows per workgroup (16 per wave)
constexpr int CH_BN = 64;                         // keys per tile
constexpr int CH_BK = 32;                         // floats of e per stage (one 128-byte line per row)
constexpr int CH_STAGE = (CH_BM + CH_BN) * CH_BK; // floats per stage = 16 KiB
constexpr int CH_AP = CH_BN + 1;                  // pitch of the affinity tile (a thread walks a row: conflict-free)
constexpr int CH_MAX_E = 2048;
constexpr int CB_KT = 16;                         // backward: keys per workgroup
constexpr int CB_DS = 512;                        // backward: columns of e per workgroup (128 per wave)

// The class that owns key j: the largest y with class_start[y] <= j (empty classes before it share its start and lose).  j < class_start[c].
__device__ __forceinline__ int class_of(const int32_t* __restrict__ cs, int c, int j) {
    int lo = 0, hi = c - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cs[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// The first class that starts at or after key b: the smallest y in 0 .. c with class_start[y] >= b (class_start[c] = m >= b).
__device__ __forceinline__ int first_class_from(const int32_t* __restrict__ cs, int c, int b) {
    int lo = 0, hi = c;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cs[mid] >= b) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void cache_rnorm_kernel(const float* __restrict__ f, float* __restrict__ rnorm, int n, int e) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;       // per wave
    const f32x4* p = (const f32x4*)(f + (size_t)row * e);
    float s = 0.f;
    for (int i = lane; i < (e >> 2); i += 64) {
        const f32x4 v = p[i];
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    s = wave_sum(s);
    if (lane == 0) rnorm[row] = 1.0f / sqrtf(s);
}

__global__ __launch_bounds__(256) void cache_fwd_kernel(const float* __restrict__ f, const float* __restrict__ keys, const int32_t* __restrict__ cs,
                                                        const float* __restrict__ kw, const float* __restrict__ rnorm, float alpha, float beta, int n, int m,
                                                        int c, int e, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[2 * CH_STAGE];
    __shared__ float At[CH_BM * CH_AP];
    __shared__ float carry[2][CH_BM];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int r0 = blockIdx.x * CH_BM;
    // gridDim.y > 1 (few row tiles): the classes are dealt to gridDim.y workgroups per row tile, a class to the share in which it starts, so a workgroup
    // walks the keys kbeg .. kend - 1 of whole classes.  Where the tiles start changes no bit: a score is one MFMA chain and a class is one key-order sum.
    int kbeg = 0, kend = m;
    if (gridDim.y > 1) {
        const int sp = blockIdx.y, S = gridDim.y;
        kbeg = cs[first_class_from(cs, c, (int)((int64_t)sp * m / S))];
        if (sp + 1 < S) kend = cs[first_class_from(cs, c, (int)((int64_t)(sp + 1) * m / S))];
        kbeg = min(max(kbeg, 0), m);
        kend = min(kend, m);
        if (kbeg >= kend) return;       // no class starts in this share
    }
    const int nec = (e + CH_BK - 1) / CH_BK, nkt = (kend - kbeg + CH_BN - 1) / CH_BN, T = nkt * nec;

    // staging: thread t moves the 16-byte pieces t and t + 256 of the 64 x 32 image tile and of the key tile; the piece index within a row is XOR-swizzled
    // with (row & 7) as in gemm_f32.hip, so the fragment reads below are conflict-free.  Rows >= n, keys >= kend and columns >= e are zeros.
    f32x4 fr[2], kr[2];
    auto gload = [&](int kt, int ec) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, col = ec * CH_BK + (id & 7) * 4;
            const int gr = r0 + row, gk = kbeg + kt * CH_BN + row;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            fr[i] = (gr < n && col < e) ? *(const f32x4*)(f + (size_t)gr * e + col) : zero;
            kr[i] = (gk < kend && col < e) ? *(const f32x4*)(keys + (size_t)gk * e + col) : zero;
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, ch = (id & 7) ^ (row & 7);
            float* st = lds + buf * CH_STAGE + row * CH_BK + ch * 4;
            *(f32x4*)st = fr[i];
            *(f32x4*)(st + CH_BM * CH_BK) = kr[i];
        }
    };

    int a_off[2], b_off[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int chunk = (kk * 4 + fgrp) ^ (lane & 7);
        a_off[kk] = (wave * 16 + frow) * CH_BK + chunk * 4;
        b_off[kk] = CH_BM * CH_BK + frow * CH_BK + chunk * 4;
    }
    const int my_row = r0 + wave * 16 + frow;
    const float rn = my_row < n ? rnorm[my_row] : 0.f;

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
        const float* st = lds + buf * CH_STAGE;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f32x4 bf[4];
            const f32x4 af = *(const f32x4*)(st + a_off[kk]);
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = *(const f32x4*)(st + b_off[kk] + j * 16 * CH_BK);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][s], af[s], acc[j], 0, 0, 0);
        }
        if (t + 1 < T) sstore(buf ^ 1);
        if (ec == nec - 1) {
            // lane (frow, fgrp) holds the scores of row wave*16 + frow against keys j*16 + fgrp*4 + {0..3} of the tile
            const int j0 = kbeg + kt * CH_BN, j1 = min(j0 + CH_BN, kend);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kl = j * 16 + fgrp * 4 + r, key = j0 + kl;
                    const float w = key < kend ? alpha * (kw ? kw[key] : 1.0f) : 0.f;
                    const float s = acc[j][r] * rn;
                    At[(wave * 16 + frow) * CH_AP + kl] = expf(-(beta * (1.0f - s))) * w;
                }
                acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            __syncthreads();
            const int row = tid & 63, gr = r0 + row;
            const int y_lo = class_of(cs, c, j0), y_hi = class_of(cs, c, j1 - 1);
            for (int y = y_lo + wave; y <= y_hi; y += 4) {
                const int a = cs[y], b = cs[y + 1];
                const int lo = max(a, j0), hi = min(b, j1);
                if (lo >= hi) continue;       // a class without keys: its logit is never touched
                float sum = a < j0 ? carry[kt & 1][row] : 0.f;
                const float* ar = At + row * CH_AP - j0;
                for (int j = lo; j < hi; ++j) sum += ar[j];
                if (b > j1) carry[(kt + 1) & 1][row] = sum;
                else if (gr < n) out[(size_t)gr * c + y] += sum;
            }
        }
        kt = nkt_;
        ec = nec_;
        __syncthreads();
    }
}

// grid (ceil(m / 16), ceil(e / 512))
__global__ __launch_bounds__(256) void cache_bwd_kernel(const float* __restrict__ f, const float* __restrict__ keys, const int32_t* __restrict__ cs,
                                                        const float* __restrict__ kw, const float* __restrict__ rnorm, const float* __restrict__ G, float alpha,
                                                        float beta, int n, int m, int c, int e, float* __restrict__ dK) {
    __shared__ float dS[CH_BM][CB_KT + 1];
    __shared__ int ycls[CB_KT];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int key0 = blockIdx.x * CB_KT, d0 = blockIdx.y * CB_DS + wave * (CB_DS / 4);
    if (tid < CB_KT) ycls[tid] = key0 + tid < m ? class_of(cs, c, key0 + tid) : 0;
    __syncthreads();
    float w[4];
    int y[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int key = key0 + fgrp * 4 + r;
        y[r] = ycls[fgrp * 4 + r];
        w[r] = key < m ? alpha * beta * (kw ? kw[key] : 1.0f) : 0.f;
    }
    const int nfr = min(8, max(0, (e - d0 + 15) / 16));      // 16-column fragments of this wave that lie inside e
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[8];
#pragma unroll
    for (int jf = 0; jf < 8; ++jf) acc[jf] = zero;
    const int keyA = key0 + frow;
    const float* krow = keys + (size_t)min(keyA, m - 1) * e;

    for (int rt = 0; rt < n; rt += CH_BM) {
        // scores of rows rt + wave*16 + {0..15} against the 16 keys: the forward's chain (16 floats of e per pair of MFMA groups, ascending)
        const int row = rt + wave * 16 + frow;
        const bool rowok = row < n;
        const float* frow_p = f + (size_t)min(row, n - 1) * e;
        f32x4 s = zero;
        auto lda = [&](int k) { return (keyA < m && k < e) ? *(const f32x4*)(krow + k) : zero; };
        auto ldb = [&](int k) { return (rowok && k < e) ? *(const f32x4*)(frow_p + k) : zero; };
        f32x4 a = lda(fgrp * 4), b = ldb(fgrp * 4);
        for (int kb = 0; kb < e; kb += 16) {       // the operands of step kb + 16 are in flight during the MFMAs of step kb
            const f32x4 an = lda(kb + 16 + fgrp * 4), bn = ldb(kb + 16 + fgrp * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) s = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], b[q], s, 0, 0, 0);
            a = an;
            b = bn;
        }
        const float rn = rowok ? rnorm[row] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float sv = s[r] * rn;
            const float A = expf(-(beta * (1.0f - sv)));
            const float g = (rowok && key0 + fgrp * 4 + r < m) ? G[(size_t)row * c + y[r]] : 0.f;
            dS[wave * 16 + frow][fgrp * 4 + r] = (w[r] * g) * A * rn;      // dS_ij / |f_i|: the rows of img_emb below are not normalised
        }
        __syncthreads();
        // dK[key, d] += sum over the tile's rows dS[row, key] f[row, d], four rows per MFMA, ascending
        const int rows = min(CH_BM, n - rt);
        for (int st = 0; st * 4 < rows; ++st) {
            const int rr = rt + st * 4 + fgrp;
            const float bval = dS[st * 4 + fgrp][frow];
            const float* fp = f + (size_t)min(rr, n - 1) * e;
#pragma unroll
            for (int jf = 0; jf < 8; ++jf) {
                if (jf < nfr) {
                    const int d = d0 + jf * 16 + frow;
                    const float aval = (rr < n && d < e) ? fp[d] : 0.f;
                    acc[jf] = __builtin_amdgcn_mfma_f32_16x16x4f32(aval, bval, acc[jf], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // lane (frow, fgrp) holds dK[key0 + frow][d0 + jf*16 + fgrp*4 + {0..3}]
    if (keyA < m) {
#pragma unroll
        for (int jf = 0; jf < 8; ++jf) {
            const int d = d0 + jf * 16 + fgrp * 4;
            if (jf < nfr && d < e) *(f32x4*)(dK + (size_t)keyA * e + d) = acc[jf];
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_cache(const char* who, int n, int m, int c, int e) {
    GRIP_REQUIRE(n > 0 && m > 0 && c > 0, "%s: n = %d, m = %d, c = %d (each must be positive)", who, n, m, c);
    GRIP_REQUIRE(e > 0 && e % 4 == 0 && e <= CH_MAX_E, "%s: e = %d (a multiple of 4, 4 .. %d)", who, e, CH_MAX_E);
    return GRIP_OK;
}
size_t cache_ws_bytes(int n) { return (size_t)n * sizeof(float) + 256; }
}  // namespace

#define RUNC(x) do { int _rc = (x); if (_rc != GRIP_OK) return _rc; } while (0)

extern "C" int grip_cache_head_workspace(int n, int m, int c, int e, size_t* bytes) {
    GRIP_REQUIRE(bytes, "cache_head_workspace: null pointer");
    RUNC(check_cache("cache_head_workspace", n, m, c, e));
    *bytes = cache_ws_bytes(n);
    return GRIP_OK;
}

// the reciprocal row norms, at the workspace's first 256-byte boundary
static int cache_rnorm(const char* who, const float* img_emb, int n, int e, void* workspace, size_t workspace_bytes, hipStream_t s, float** rnorm) {
    float* rn = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    GRIP_REQUIRE(workspace_bytes >= cache_ws_bytes(n), "%s: workspace too small (%zu bytes, grip_cache_head_workspace says %zu)", who, workspace_bytes,
                 cache_ws_bytes(n));
    hipLaunchKernelGGL(cache_rnorm_kernel, dim3((n + 3) / 4), dim3(256), 0, s, img_emb, rn, n, e);
    GRIP_CHECK_HIP(hipGetLastError());
    *rnorm = rn;
    return GRIP_OK;
}

extern "C" int grip_cache_head_forward(const float* img_emb, const float* keys, const int32_t* class_start, const float* key_weight, float alpha, float beta,
                                       int n, int m, int c, int e, float* logits_inout, void* workspace, size_t workspace_bytes, void* stream) {
    RUNC(check_cache("cache_head_forward", n, m, c, e));
    GRIP_REQUIRE(img_emb && keys && class_start && logits_inout && workspace, "cache_head_forward: null pointer");
    GRIP_REQUIRE(aligned16(img_emb) && aligned16(keys), "cache_head_forward: img_emb and keys must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* rnorm;
    RUNC(cache_rnorm("cache_head_forward", img_emb, n, e, workspace, workspace_bytes, s, &rnorm));
    // few row tiles (a training batch): deal the classes to several workgroups per row tile, up to one per key tile, until ~512 workgroups exist
    const int row_tiles = (n + CH_BM - 1) / CH_BM, key_tiles = (m + CH_BN - 1) / CH_BN;
    const int split = std::max(1, std::min({key_tiles, (512 + row_tiles - 1) / row_tiles, 65535}));
    hipLaunchKernelGGL(cache_fwd_kernel, dim3(row_tiles, split), dim3(256), 0, s, img_emb, keys, class_start, key_weight, rnorm, alpha, beta, n, m, c, e,
                       logits_inout);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}

extern "C" int grip_cache_head_backward(const float* img_emb, const float* keys, const int32_t* class_start, const float* key_weight, float alpha, float beta,
                                        int n, int m, int c, int e, const float* grad_logits, float* grad_keys, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    RUNC(check_cache("cache_head_backward", n, m, c, e));
    GRIP_REQUIRE(img_emb && keys && class_start && grad_logits && grad_keys && workspace, "cache_head_backward: null pointer");
    GRIP_REQUIRE(aligned16(img_emb) && aligned16(keys) && aligned16(grad_keys), "cache_head_backward: img_emb, keys and grad_keys must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* rnorm;
    RUNC(cache_rnorm("cache_head_backward", img_emb, n, e, workspace, workspace_bytes, s, &rnorm));
    hipLaunchKernelGGL(cache_bwd_kernel, dim3((m + CB_KT - 1) / CB_KT, (e + CB_DS - 1) / CB_DS), dim3(256), 0, s, img_emb, keys, class_start, key_weight, rnorm,
                       grad_logits, alpha, beta, n, m, c, e, grad_keys);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}
