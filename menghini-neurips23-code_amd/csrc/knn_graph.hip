// Transductive label propagation over a pool (Zhu & Ghahramani 2002; Zhou et al. 2004; ZLaP, CVPR 2024, for CLIP zero-shot pools): a kNN graph of the
// pool's image embeddings and a random walk of the class probabilities over it.  All f32 / int32.
//   * grip_knn_graph: row i of `queries` gets the k rows of `base` of largest cosine, ordered (sim descending, index ascending).  n x m x e is a GEMM
//     (2.56 TFLOP at 50 000 x 50 000 x 512) whose [n, m] result must never exist (10 GB), so it is the main loop of cache_head.hip -- a workgroup owns
//     64 query rows and walks the base 64 rows at a time, e staged 32 floats per step through two XOR-swizzled LDS buffers with the loads of step t + 1
//     in flight under the v_mfma_f32_16x16x4_f32 of step t, a wave holding 16 rows x 64 base rows in four accumulators -- with a SELECT epilogue:
//       - knn_rnorm_kernel writes 1 / |row| of both operands into the workspace (once when the queries are a window of the base); the two factors
//         scale the SCORE, the operands are never copied or normalised;
//       - at the end of a base tile lane (frow, fgrp) holds 16 scores of row wave * 16 + frow.  The row's current top-k list sits in LDS, sorted by
//         the total order; the lane compares its scores with the list's last entry and inserts the survivors (a shift from the end).  The four lanes
//         of a row take turns in a wave-uniform loop, the 16 rows of a turn are 16 different lists: no two lanes ever touch one list at a time.  Once
//         the lists have filled nearly every score is rejected by that one compare, and a tile without a survivor in the whole wave skips the turns.
//       - base rows >= m and the excluded self row are masked before the compare.  A row's list is owned by one wave from start to finish: the
//         epilogue needs no workgroup barrier, no atomics, and a list is the exact top-k of the row's scores under the total order whatever order the
//         candidates arrive in.
//     A score is one MFMA chain over e in ASCENDING order (an f32 MFMA is a k-ordered fmaf chain; the staging stores each sixteen floats transposed
//     4 x 4 so that consecutive MFMAs take consecutive fours) times the two reciprocal norms: it depends on the two rows only -- not on n, m, the row's
//     place in a tile or the call -- so bit-identical base rows score bit-identically and the lower index wins.
//     LDS: 2 x 16 KiB stages + 64 x 33 x 8 B lists = 48.5 KiB: three workgroups per CU.
//       - 782 query tiles (n = 50 000) on 256 CUs leave the busiest CU with 4 tiles against an average of 3.05, and a `predict`-sized call has a
//         handful of tiles: below KG_ITEMS query tiles the base tiles are dealt to several workgroups per query tile (knn_shares: a function of n and
//         m), each writes the sorted top-k of its share to the workspace and knn_merge_kernel merges the shares under the same total order.  A score
//         does not depend on the share it is computed in, so no bit moves with the split.
//   * grip_label_propagate: Z <- (1 - alpha) probs + alpha W Z, `iters` times, W the row-stochastic softmax(gamma sim) over each row's k neighbours.
//     lp_weight_kernel writes W once (a thread per row, the k terms summed in list order); lp_step_kernel is a wave per row, lanes over classes, the
//     k neighbour rows gathered and added IN LIST ORDER (their index and weight are wave-uniform: one coalesced row read per neighbour).  One ABI
//     call enqueues weights + iters steps, ping-ponging between `out` and the workspace; the last step also writes the row's arg-max.
//     This is NOT ZLaP's symmetrised, conjugate-gradient-solved system: no class nodes, no symmetrisation, no convergence test.
#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {
constexpr int KG_BM = 64;                         // query rows per workgroup (16 per wave)
constexpr int KG_BN = 64;                         // base rows per tile
constexpr int KG_BK = 32;                         // floats of e per stage (one 128-byte line per row)
constexpr int KG_STAGE = (KG_BM + KG_BN) * KG_BK; // floats per stage = 16 KiB
constexpr int KG_MAX_K = 32;
constexpr int KG_LP = KG_MAX_K + 1;               // pitch of a row's list (16 lanes walk 16 lists: conflict-free)
constexpr int KG_MAX_E = 2048;
constexpr int KG_ITEMS = 3072;                    // workgroups wanted at least (12 per CU: the busiest CU then carries at most 1 / 12 more than the average)
constexpr int KG_MAX_SPLIT = 64;                  // shares of the base per query tile at most

__global__ __launch_bounds__(256) void knn_rnorm_kernel(const float* __restrict__ f, float* __restrict__ rnorm, int n, int e) {
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

// rb holds round_up(m, 64) floats (the tail is never used: those base rows are masked).  gridDim.y > 1 (fewer than KG_ITEMS query tiles): the base tiles
// are dealt to gridDim.y workgroups per query tile; each writes the sorted top-k of ITS share to part_idx / part_sim [gridDim.y, n, k] (entries a share
// cannot fill keep (-inf, INT_MAX)) and knn_merge_kernel merges them under the same total order.  A score does not depend on the share it is computed in.
__global__ __launch_bounds__(256) void knn_graph_kernel(const float* __restrict__ q, const float* __restrict__ base, const float* __restrict__ rq,
                                                        const float* __restrict__ rb, int n, int m, int e, int k, int self_offset,
                                                        int32_t* __restrict__ idx_out, float* __restrict__ sim_out, int32_t* __restrict__ part_idx,
                                                        float* __restrict__ part_sim) {
    __shared__ __attribute__((aligned(16))) float lds[2 * KG_STAGE];
    __shared__ float lsim[KG_BM * KG_LP];
    __shared__ int lidx[KG_BM * KG_LP];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fgrp = lane >> 4;
    const int r0 = blockIdx.x * KG_BM;
    const int nec = (e + KG_BK - 1) / KG_BK, nkt = (m + KG_BN - 1) / KG_BN;
    const int kt0 = (int)((int64_t)blockIdx.y * nkt / gridDim.y), kt1 = (int)((int64_t)(blockIdx.y + 1) * nkt / gridDim.y);
    const int T = (kt1 - kt0) * nec;
    if (gridDim.y > 1) {
        idx_out = part_idx + (size_t)blockIdx.y * n * k;
        sim_out = part_sim + (size_t)blockIdx.y * n * k;
    }

    // staging: thread t moves the 16-byte pieces t and t + 256 of the 64 x 32 query tile and of the base tile; the piece index within a row is
    // XOR-swizzled with (row & 7) as in gemm_f32.hip, so the fragment reads below are conflict-free.  Rows >= n, base rows >= m and columns >= e are zeros.
    f32x4 fr[2], kr[2];
    auto gload = [&](int kt, int ec) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int id = tid + 256 * i, row = id >> 3, col = ec * KG_BK + (id & 7) * 4;
            const int gr = r0 + row, gk = kt * KG_BN + row;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            fr[i] = (gr < n && col < e) ? *(const f32x4*)(q + (size_t)gr * e + col) : zero;
            kr[i] = (gk < m && col < e) ? *(const f32x4*)(base + (size_t)gk * e + col) : zero;
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            // Each sixteen floats of a row are stored TRANSPOSED as 4 x 4: float 4 s + g of the sixteen goes to (chunk g, slot s), so that the MFMA of step s
            // -- whose four k slots are the four lane groups g -- contracts the floats 4 s .. 4 s + 3: the chain over e is ASCENDING.  Four 4-byte writes per
            // 16-byte piece; over a wave they cover the 32 banks twice, as the one 16-byte write did.
            const int id = tid + 256 * i, row = id >> 3, kk = (id & 7) >> 2, sp = id & 3;
            float* st = lds + buf * KG_STAGE + row * KG_BK + sp;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = (kk * 4 + g) ^ (row & 7);
                st[ch * 4] = fr[i][g];
                st[KG_BM * KG_BK + ch * 4] = kr[i][g];
            }
        }
    };

    int a_off[2], b_off[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int chunk = (kk * 4 + fgrp) ^ (lane & 7);
        a_off[kk] = (wave * 16 + frow) * KG_BK + chunk * 4;
        b_off[kk] = KG_BM * KG_BK + frow * KG_BK + chunk * 4;
    }
    const int my_row = r0 + wave * 16 + frow;
    const bool row_ok = my_row < n;
    const float rn = row_ok ? rq[my_row] : 0.f;
    const int self = self_offset >= 0 ? self_offset + my_row : -1;
    float* ls = lsim + (wave * 16 + frow) * KG_LP;
    int* li = lidx + (wave * 16 + frow) * KG_LP;

    // the 16 lists of this wave start as k entries that every real candidate beats
    for (int t = lane; t < 16 * KG_LP; t += 64) {
        lsim[wave * 16 * KG_LP + t] = -INFINITY;
        lidx[wave * 16 * KG_LP + t] = INT_MAX;
    }

    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    gload(kt0, 0);
    sstore(0);
    __syncthreads();
    int kt = kt0, ec = 0;
    for (int t = 0; t < T; ++t) {
        const int buf = t & 1;
        int nkt_ = kt, nec_ = ec + 1;
        if (nec_ == nec) { nec_ = 0; ++nkt_; }
        if (t + 1 < T) gload(nkt_, nec_);
        const float* st = lds + buf * KG_STAGE;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f32x4 bf[4];
            const f32x4 af = *(const f32x4*)(st + a_off[kk]);
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[j] = *(const f32x4*)(st + b_off[kk] + j * 16 * KG_BK);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][s], af[s], acc[j], 0, 0, 0);
        }
        if (t + 1 < T) sstore(buf ^ 1);
        if (ec == nec - 1) {
            // lane (frow, fgrp) holds the scores of row wave*16 + frow against base rows j0 + j*16 + fgrp*4 + {0..3}
            const int j0 = kt * KG_BN;
            float sc[16];
            float best = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int key0 = j0 + j * 16 + fgrp * 4;
                const f32x4 rbv = *(const f32x4*)(rb + key0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = key0 + r;
                    const float s = (acc[j][r] * rn) * rbv[r];
                    sc[j * 4 + r] = (row_ok && key < m && key != self) ? s : -INFINITY;
                    best = fmaxf(best, sc[j * 4 + r]);
                }
                acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            // (the list's last entry only ever improves: a lane whose best score does not reach it now has nothing to insert in its turn either)
            if (__builtin_amdgcn_ballot_w64(best > -INFINITY && best >= ls[k - 1]) != 0) {
#pragma unroll 1
                for (int g = 0; g < 4; ++g) {
                    if (fgrp == g) {
                        float ts = ls[k - 1];
                        int ti = li[k - 1];
#pragma unroll
                        for (int c = 0; c < 16; ++c) {
                            const float s = sc[c];
                            const int id = j0 + (c >> 2) * 16 + fgrp * 4 + (c & 3);
                            if (s > -INFINITY && (s > ts || (s == ts && id < ti))) {
                                int p = k - 1;
                                while (p > 0) {
                                    const float ps = ls[p - 1];
                                    const int pi = li[p - 1];
                                    if (ps > s || (ps == s && pi < id)) break;
                                    ls[p] = ps;
                                    li[p] = pi;
                                    --p;
                                }
                                ls[p] = s;
                                li[p] = id;
                                ts = ls[k - 1];
                                ti = li[k - 1];
                            }
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        kt = nkt_;
        ec = nec_;
        __syncthreads();
    }
    // the wave writes its own 16 lists
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < 16 * k; t += 64) {
        const int r = t / k, p = t - r * k, gr = r0 + wave * 16 + r;
        if (gr < n) {
            idx_out[(size_t)gr * k + p] = lidx[(wave * 16 + r) * KG_LP + p];
            sim_out[(size_t)gr * k + p] = lsim[(wave * 16 + r) * KG_LP + p];
        }
    }
}

// out[i, :] = the best k of the `shares` sorted lists of row i: a thread per row and a cursor per share (a byte in LDS: k <= 32, shares <= KG_MAX_SPLIT);
// entry p is the best of the lists' heads under the total order, and that list's cursor moves on: k * shares loads per row.  The shares hold k real
// candidates between them (m - excluded >= k): no filler is ever taken.
__global__ __launch_bounds__(256) void knn_merge_kernel(const int32_t* __restrict__ part_idx, const float* __restrict__ part_sim, int n, int k, int shares,
                                                        int32_t* __restrict__ idx_out, float* __restrict__ sim_out) {
    __shared__ unsigned char cur[KG_MAX_SPLIT][256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int sh = 0; sh < shares; ++sh) cur[sh][threadIdx.x] = 0;       // (a column of `cur` is one thread's: no barrier)
    for (int p = 0; p < k; ++p) {
        float bs = -INFINITY;
        int bid = INT_MAX, bsh = 0;
        for (int sh = 0; sh < shares; ++sh) {
            const int j = cur[sh][threadIdx.x];
            if (j >= k) continue;
            const size_t o = ((size_t)sh * n + i) * k + j;
            const float s = part_sim[o];
            const int id = part_idx[o];
            if (s > bs || (s == bs && id < bid)) { bs = s; bid = id; bsh = sh; }
        }
        cur[bsh][threadIdx.x] += 1;
        idx_out[(size_t)i * k + p] = bid;
        sim_out[(size_t)i * k + p] = bs;
    }
}

// w[i, :] = softmax(gamma * sim[i, :]) with the row's first (largest) entry as the shift; the k terms are summed in list order
__global__ __launch_bounds__(256) void lp_weight_kernel(const float* __restrict__ sim, float gamma, int n, int k, float* __restrict__ w) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* s = sim + (size_t)i * k;
    float* o = w + (size_t)i * k;
    const float s0 = s[0];
    float sum = 0.f;
    for (int j = 0; j < k; ++j) {
        const float x = expf(gamma * (s[j] - s0));
        o[j] = x;
        sum += x;
    }
    for (int j = 0; j < k; ++j) o[j] = o[j] / sum;
}

// one wave per row: zout[i, :] = fmaf(alpha, sum_k w[i, k] zin[idx[i, k], :], (1 - alpha) probs[i, :]); argmax (optional): first index of the row's maximum
__global__ __launch_bounds__(256) void lp_step_kernel(const float* __restrict__ probs, const float* __restrict__ zin, const int32_t* __restrict__ idx,
                                                      const float* __restrict__ w, float alpha, float one_minus_alpha, int n, int c, int k,
                                                      float* __restrict__ zout, int32_t* __restrict__ argmax) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;       // per wave
    const int my_idx = lane < k ? idx[(size_t)row * k + lane] : 0;
    const float my_w = lane < k ? w[(size_t)row * k + lane] : 0.f;
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int c0 = 0; c0 < c; c0 += 64) {
        const int cls = c0 + lane;
        float acc = 0.f;
        for (int j = 0; j < k; ++j) {
            const int nb = __builtin_amdgcn_readlane(my_idx, j);
            const float wj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_w), j));
            if (cls < c) acc = fmaf(wj, zin[(size_t)nb * c + cls], acc);
        }
        if (cls < c) {
            const float z = fmaf(alpha, acc, one_minus_alpha * probs[(size_t)row * c + cls]);
            zout[(size_t)row * c + cls] = z;
            if (z > bv) { bv = z; bi = cls; }
        }
    }
    if (argmax) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) argmax[row] = bi;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_knn(const char* who, int n, int m, int e, int k) {
    GRIP_REQUIRE(n > 0 && m > 0, "%s: n = %d, m = %d (each must be positive)", who, n, m);
    GRIP_REQUIRE(e > 0 && e % 4 == 0 && e <= KG_MAX_E, "%s: e = %d (a multiple of 4, 4 .. %d)", who, e, KG_MAX_E);
    GRIP_REQUIRE(k >= 1 && k <= KG_MAX_K, "%s: k = %d (1 .. %d)", who, k, KG_MAX_K);
    return GRIP_OK;
}
size_t knn_rb_floats(int m) { return (size_t)round_up64(m, KG_BN); }
// shares of the base per query tile: 1 once the query tiles alone fill the chip KG_ITEMS / 256 times over, else enough to get there
int knn_shares(int n, int m) {
    const int row_tiles = (n + KG_BM - 1) / KG_BM, base_tiles = (m + KG_BN - 1) / KG_BN;
    return std::max(1, std::min({base_tiles, (KG_ITEMS + row_tiles - 1) / row_tiles, KG_MAX_SPLIT}));
}
size_t knn_part_entries(int n, int m, int k) { return knn_shares(n, m) > 1 ? (size_t)knn_shares(n, m) * n * k : 0; }
size_t knn_ws_bytes(int n, int m, int k) { return (knn_rb_floats(m) + (size_t)round_up64(n, 4) + 2 * knn_part_entries(n, m, k)) * sizeof(float) + 256; }

int check_lp(const char* who, int n, int c, int k) {
    GRIP_REQUIRE(n > 0 && c > 0, "%s: n = %d, c = %d (each must be positive)", who, n, c);
    GRIP_REQUIRE(k >= 1 && k <= KG_MAX_K, "%s: k = %d (1 .. %d)", who, k, KG_MAX_K);
    return GRIP_OK;
}
size_t lp_z_floats(int n, int c) { return (size_t)round_up64((int64_t)n * c, 64); }
size_t lp_ws_bytes(int n, int c, int k) { return (lp_z_floats(n, c) + (size_t)n * k) * sizeof(float) + 256; }
}  // namespace

#define RUNC(x) do { int _rc = (x); if (_rc != GRIP_OK) return _rc; } while (0)

extern "C" int grip_knn_graph_workspace(int n, int m, int e, int k, size_t* bytes) {
    GRIP_REQUIRE(bytes, "knn_graph_workspace: null pointer");
    RUNC(check_knn("knn_graph_workspace", n, m, e, k));
    *bytes = knn_ws_bytes(n, m, k);
    return GRIP_OK;
}

extern "C" int grip_knn_graph(const float* queries, const float* base, int n, int m, int e, int k, int self_offset, int32_t* idx_out, float* sim_out,
                              void* workspace, size_t workspace_bytes, void* stream) {
    RUNC(check_knn("knn_graph", n, m, e, k));
    GRIP_REQUIRE(self_offset >= -1, "knn_graph: self_offset = %d (-1: no row excluded, or the base row of query 0)", self_offset);
    GRIP_REQUIRE(self_offset < 0 || (int64_t)self_offset + n <= m, "knn_graph: self_offset = %d with n = %d queries runs past the m = %d base rows",
                 self_offset, n, m);
    GRIP_REQUIRE(m - (self_offset >= 0 ? 1 : 0) >= k, "knn_graph: k = %d neighbours out of %d eligible base rows (m = %d%s)", k,
                 m - (self_offset >= 0 ? 1 : 0), m, self_offset >= 0 ? ", the row itself excluded" : "");
    GRIP_REQUIRE(queries && base && idx_out && sim_out && workspace, "knn_graph: null pointer");
    GRIP_REQUIRE(aligned16(queries) && aligned16(base), "knn_graph: queries and base must be 16-byte aligned");
    GRIP_REQUIRE(workspace_bytes >= knn_ws_bytes(n, m, k), "knn_graph: workspace too small (%zu bytes, grip_knn_graph_workspace says %zu)", workspace_bytes,
                 knn_ws_bytes(n, m, k));
    hipStream_t s = (hipStream_t)stream;
    float* rb = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* rq = rb + knn_rb_floats(m);
    hipLaunchKernelGGL(knn_rnorm_kernel, dim3((m + 3) / 4), dim3(256), 0, s, base, rb, m, e);
    GRIP_CHECK_HIP(hipGetLastError());
    if (self_offset >= 0 && queries == base + (size_t)self_offset * e) {
        rq = rb + self_offset;      // the queries are a window of the base: one set of norms
    } else {
        hipLaunchKernelGGL(knn_rnorm_kernel, dim3((n + 3) / 4), dim3(256), 0, s, queries, rq, n, e);
        GRIP_CHECK_HIP(hipGetLastError());
    }
    const int shares = knn_shares(n, m);
    float* part_sim = rb + knn_rb_floats(m) + round_up64(n, 4);       // (behind the queries' norms, whether they are used or not)
    int32_t* part_idx = (int32_t*)(part_sim + knn_part_entries(n, m, k));
    hipLaunchKernelGGL(knn_graph_kernel, dim3((n + KG_BM - 1) / KG_BM, shares), dim3(256), 0, s, queries, base, rq, rb, n, m, e, k, self_offset, idx_out,
                       sim_out, part_idx, part_sim);
    GRIP_CHECK_HIP(hipGetLastError());
    if (shares > 1) {
        hipLaunchKernelGGL(knn_merge_kernel, dim3((n + 255) / 256), dim3(256), 0, s, part_idx, part_sim, n, k, shares, idx_out, sim_out);
        GRIP_CHECK_HIP(hipGetLastError());
    }
    return GRIP_OK;
}

extern "C" int grip_label_propagate_workspace(int n, int c, int k, size_t* bytes) {
    GRIP_REQUIRE(bytes, "label_propagate_workspace: null pointer");
    RUNC(check_lp("label_propagate_workspace", n, c, k));
    *bytes = lp_ws_bytes(n, c, k);
    return GRIP_OK;
}

extern "C" int grip_label_propagate(const float* probs, const int32_t* idx, const float* sim, float alpha, float gamma, int iters, int n, int c, int k,
                                    float* out, int32_t* argmax_out, void* workspace, size_t workspace_bytes, void* stream) {
    RUNC(check_lp("label_propagate", n, c, k));
    GRIP_REQUIRE(alpha >= 0.f && alpha < 1.f, "label_propagate: alpha = %g (0 <= alpha < 1)", (double)alpha);
    GRIP_REQUIRE(gamma >= 0.f && gamma <= FLT_MAX, "label_propagate: gamma = %g (a finite gamma >= 0)", (double)gamma);
    GRIP_REQUIRE(iters >= 1, "label_propagate: iters = %d (at least 1)", iters);
    GRIP_REQUIRE(probs && idx && sim && out && workspace, "label_propagate: null pointer");
    GRIP_REQUIRE(probs != out, "label_propagate: out must not alias probs");
    GRIP_REQUIRE(workspace_bytes >= lp_ws_bytes(n, c, k), "label_propagate: workspace too small (%zu bytes, grip_label_propagate_workspace says %zu)",
                 workspace_bytes, lp_ws_bytes(n, c, k));
    hipStream_t s = (hipStream_t)stream;
    float* z = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* w = z + lp_z_floats(n, c);
    hipLaunchKernelGGL(lp_weight_kernel, dim3((n + 255) / 256), dim3(256), 0, s, sim, gamma, n, k, w);
    GRIP_CHECK_HIP(hipGetLastError());
    const float* src = probs;
    for (int t = 0; t < iters; ++t) {
        float* dst = ((iters - 1 - t) & 1) ? z : out;      // the last step writes `out`
        hipLaunchKernelGGL(lp_step_kernel, dim3((n + 3) / 4), dim3(256), 0, s, probs, src, idx, w, alpha, 1.0f - alpha, n, c, k, dst,
                           t == iters - 1 ? argmax_out : (int32_t*)nullptr);
        GRIP_CHECK_HIP(hipGetLastError());
        src = dst;
    }
    return GRIP_OK;
}
