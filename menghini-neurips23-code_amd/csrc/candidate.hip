// Candidate pseudolabel SETS over a pool and the partial-label loss that trains on them (include/grip_amd.h, grip_candidate_select / grip_candidate_ce;
// Candidate Pseudolabel Learning, Zhang et al., ICML 2024).  All f32 / int32.
//
// grip_candidate_select.  threshold[c] = the claim-th largest value of column c, EXACT: a radix select over the bit patterns (non-negative floats order as
// their integers), four passes of 8 bits from the top.  Pass p:
//   * cs_hist_kernel: a workgroup owns CS_RB consecutive rows x CS_CT consecutive columns and counts, per column, the digit p of every element whose
//     higher digits equal the prefix found so far -- in an LDS histogram [256][CS_CT] (column fastest: the lanes of a row segment hit different banks),
//     flushed with integer adds to hist[c][256] in the workspace.  Counts are integers: no order of accumulation can change a bit.
//   * cs_pick_kernel: one thread per column walks its 256 bins from the top until `remaining` elements are covered, appends the digit to the prefix,
//     lowers `remaining` by the elements above the digit and zeroes the bins for the next pass.
// After the fourth pass the prefix IS the threshold's bit pattern.  cs_row_kernel then builds the sets, a wave per row: the inter members by one
// comparison per class; the intra prefix by EXTRACTION -- the next class in the order (probability descending, index ascending) is the largest key
// strictly below the last one taken, so the loop keeps no per-class state, adds s_j = s_{j-1} + p_(j) in plain f32 in rank order and stops at the first
// rank whose s_{j-1} >= tau.  The prefix is then described by its last key alone (class k is in iff its key is not below it), the two rules are combined
// per class, a wave ballot packs 64 classes into two mask words, and one arg-max over the members gives the label.  Up to CS_REG_C classes the row sits in
// registers (NP values per lane); beyond, every step re-reads the row (the caches hold it).  Given threshold, a row's outputs depend on that row alone.
// One call: 1 + 2 x 4 + 1 launches for every (n, c).
//
// grip_candidate_ce.  soft_ce_kernel's frame (soft_ce.hip): one workgroup, wave w walks the rows w, w + 4, ..., col_map inverted once into the LDS, the
// lane that owns logits column k looks up ITS bit of the mask row -- one writer per output element, no atomics.  A hard row and a candidate row run the
// same statements: the gradient subtracts q_k (the one-hot of the label, or softmax over the set S: expf(x_k - max_S) / sum_S inside S, 0 outside), the
// loss subtracts x[label] or lse_S = max_S + logf(sum_S).  For S = {y}: max_S = x_y, sum_S = expf(0) = 1, lse_S = x_y + 0 and q = onehot(y): the bits of
// the hard row with label y.  With cand == NULL every row is hard and the statements are weighted_ce_kernel's (head.hip).
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {
constexpr int CS_RB = 1024;       // rows per workgroup of cs_hist_kernel
constexpr int CS_CT = 32;         // columns per workgroup of cs_hist_kernel
constexpr int CS_REG_C = 256;     // classes cs_row_kernel keeps in registers at most (four per lane)
constexpr int CCE_MAX_C = 16000;  // classes whose inverse column map fits the 64 KiB of LDS a kernel gets by default (cand given only)

// ------------------------------------------------------------------------------------------ the column thresholds
__global__ __launch_bounds__(256) void cs_init_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ prefix, uint32_t* __restrict__ remaining, int c,
                                                      int claim) {
    const int64_t total = (int64_t)c * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) hist[i] = 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < c; i += (int64_t)gridDim.x * 256) {
        prefix[i] = 0u;
        remaining[i] = (uint32_t)claim;
    }
}

// shift = 24, 16, 8, 0: the digit counted; an element takes part when its bits above the digit equal the column's prefix
__global__ __launch_bounds__(256) void cs_hist_kernel(const float* __restrict__ probs, int n, int c, const uint32_t* __restrict__ prefix, int shift,
                                                      uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256 * CS_CT];
    for (int i = threadIdx.x; i < 256 * CS_CT; i += 256) h[i] = 0u;
    __syncthreads();
    const int tx = threadIdx.x % CS_CT, ty = threadIdx.x / CS_CT;
    const int col = blockIdx.y * CS_CT + tx;
    if (col < c) {
        const uint32_t pf = prefix[col];
        const int64_t r0 = (int64_t)blockIdx.x * CS_RB, r1 = r0 + CS_RB < n ? r0 + CS_RB : n;
        for (int64_t r = r0 + ty; r < r1; r += 256 / CS_CT) {
            const uint32_t bits = __float_as_uint(probs[(size_t)r * c + col]);
            const bool takes_part = shift == 24 || ((bits ^ pf) >> (shift + 8)) == 0u;
            if (takes_part) atomicAdd(&h[((bits >> shift) & 255u) * CS_CT + tx], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 256 * CS_CT; i += 256) {
        const uint32_t v = h[i];
        if (v) atomicAdd(&hist[(size_t)(blockIdx.y * CS_CT + i % CS_CT) * 256 + i / CS_CT], v);      // (a column >= c counted nothing)
    }
}

__global__ __launch_bounds__(64) void cs_pick_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ prefix, uint32_t* __restrict__ remaining, int c,
                                                     int shift, float* __restrict__ threshold) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= c) return;
    uint32_t* hc = hist + (size_t)col * 256;
    const uint32_t need = remaining[col];
    uint32_t above = 0u, digit = 0u, left = need;
    bool found = false;
#pragma unroll 8
    for (int d = 255; d >= 0; --d) {
        const uint32_t v = hc[d];
        hc[d] = 0u;
        if (!found && above + v >= need) {
            digit = (uint32_t)d;
            left = need - above;
            found = true;
        }
        above += v;
    }
    const uint32_t pf = prefix[col] | (digit << shift);
    prefix[col] = pf;
    remaining[col] = left;
    if (shift == 0 && threshold) threshold[col] = __uint_as_float(pf);
}

// ------------------------------------------------------------------------------------------ the sets
// the wave's best (largest value, lowest class) over every lane's candidate, in every lane; bi == INT_MAX: no lane had one
__device__ __forceinline__ void cs_wave_best(float& bv, int& bi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
}

// NP > 0: c <= 64 NP, the row in registers.  NP == 0: any c, the row re-read.  combine: 0 intra & inter, 1 intra | inter, 2 intra, 3 inter.
template <int NP>
__global__ __launch_bounds__(256) void cs_row_kernel(const float* __restrict__ probs, const float* __restrict__ thr, int n, int c, int words, float tau,
                                                     int combine, int32_t* __restrict__ mask, int32_t* __restrict__ count, int32_t* __restrict__ label) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= n) return;       // per wave (the kernel has no barrier)
    const float* pr = probs + (size_t)row * c;
    constexpr int NR = NP > 0 ? NP : 1;
    float p[NR];
    if (NP > 0) {
#pragma unroll
        for (int h = 0; h < NR; ++h) p[h] = h * 64 + lane < c ? pr[h * 64 + lane] : 0.f;
    }
    const int steps = (c + 63) / 64;      // (<= NP in the register form; 2 steps - 1 <= words)
    // the intra prefix: (cv, ck) = the key of its last member
    float cv = INFINITY;
    int ck = -1;
    if (combine != 3) {
        float s = 0.f;
        for (int j = 0; j < c; ++j) {
            if (j > 0 && !(s < tau)) break;
            float bv = 0.f;
            int bi = INT_MAX;
            if (NP > 0) {
#pragma unroll
                for (int h = 0; h < NR; ++h) {
                    const int k = h * 64 + lane;
                    const float v = p[h];
                    if (k < c && (v < cv || (v == cv && k > ck)) && (bi == INT_MAX || v > bv)) { bv = v; bi = k; }
                }
            } else {
                for (int k = lane; k < c; k += 64) {
                    const float v = pr[k];
                    if ((v < cv || (v == cv && k > ck)) && (bi == INT_MAX || v > bv)) { bv = v; bi = k; }
                }
            }
            cs_wave_best(bv, bi);
            if (bi == INT_MAX) break;       // (only a row that breaks the caller's contract: a NaN compares with nothing)
            cv = bv;
            ck = bi;
            s = j == 0 ? bv : s + bv;       // a plain f32 addition, in rank order
        }
    }
    int cnt = 0, li = INT_MAX;
    float lv = 0.f;
    for (int h = 0; h < steps; ++h) {
        const int k = h * 64 + lane;
        float v = 0.f;
        if (NP > 0) {
#pragma unroll
            for (int g = 0; g < NR; ++g)
                if (g == h) v = p[g];
        } else if (k < c) {
            v = pr[k];
        }
        bool in = false;
        if (k < c) {
            const bool intra = combine != 3 && (v > cv || (v == cv && k <= ck));
            const bool inter = combine != 2 && v >= thr[k];
            in = combine == 0 ? (intra && inter) : (intra || inter);
            if (in && (li == INT_MAX || v > lv)) { lv = v; li = k; }
        }
        const unsigned long long bits = __ballot(in);
        cnt += __popcll(bits);
        if (lane == 0) {
            int32_t* mrow = mask + (size_t)row * words;
            mrow[2 * h] = (int32_t)(uint32_t)bits;
            if (2 * h + 1 < words) mrow[2 * h + 1] = (int32_t)(uint32_t)(bits >> 32);
        }
    }
    cs_wave_best(lv, li);
    if (lane == 0) {
        if (count) count[row] = cnt;
        if (label) label[row] = li == INT_MAX ? -1 : li;
    }
}

// ------------------------------------------------------------------------------------------ the partial-label loss
__global__ __launch_bounds__(256) void candidate_ce_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                           const float* __restrict__ weight, int n, int c, const int32_t* __restrict__ cand, int64_t cand_rows,
                                                           int cz, const int32_t* __restrict__ cand_row, const int32_t* __restrict__ col_map,
                                                           float* __restrict__ loss, float* __restrict__ grad) {
    extern __shared__ int inv[];      // [c] when cand != nullptr
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (cand) {
        for (int k = threadIdx.x; k < c; k += 256) inv[k] = -1;
        __syncthreads();
        for (int j = threadIdx.x; j < cz; j += 256) {
            const int k = col_map[j];
            if (k >= 0 && k < c) inv[k] = j;      // (distinct entries in [0, c) are the caller's contract; nothing else is ever indexed)
        }
        __syncthreads();
    }
    const int words = (cz + 31) / 32;
    float total = 0.f;
    for (int row = wave; row < n; row += 4) {
        const float* x = logits + (size_t)row * c;
        const float w = weight[row];
        const int lab = labels[row];
        const int64_t r = cand ? (int64_t)cand_row[row] : -1;
        const bool is_cand = r >= 0 && r < cand_rows;
        const int32_t* mrow = cand + (is_cand ? (size_t)r * words : 0);
        float m = -INFINITY;
        for (int j = lane; j < c; j += 64) m = fmaxf(m, x[j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        float sum = 0.f;
        for (int j = lane; j < c; j += 64) sum += expf(x[j] - m);
        sum = wave_sum(sum);
        const float lse = m + logf(sum);
        float ms = -INFINITY, ssum = 1.f;
        if (is_cand) {      // (per wave) the set's own maximum and sum
            bool any = false;
            for (int j = lane; j < c; j += 64) {
                const int z = inv[j];
                if (z >= 0 && ((mrow[z >> 5] >> (z & 31)) & 1)) {
                    ms = fmaxf(ms, x[j]);
                    any = true;
                }
            }
            if (__ballot(any) == 0ull) {      // an empty mapped set: the row contributes nothing
                if (grad)
                    for (int j = lane; j < c; j += 64) grad[(size_t)row * c + j] = 0.f;
                continue;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ms = fmaxf(ms, __shfl_xor(ms, o));
            ssum = 0.f;
            for (int j = lane; j < c; j += 64) {
                const int z = inv[j];
                if (z >= 0 && ((mrow[z >> 5] >> (z & 31)) & 1)) ssum += expf(x[j] - ms);
            }
            ssum = wave_sum(ssum);
        }
        if (grad)
            for (int j = lane; j < c; j += 64) {
                float q = j == lab ? 1.f : 0.f;
                if (is_cand) {
                    const int z = inv[j];
                    q = (z >= 0 && ((mrow[z >> 5] >> (z & 31)) & 1)) ? expf(x[j] - ms) / ssum : 0.f;
                }
                grad[(size_t)row * c + j] = w * (expf(x[j] - m) / sum - q);
            }
        const bool counted = is_cand || (lab >= 0 && lab < c);
        if (w != 0.f && counted) {
            const float sub = is_cand ? ms + logf(ssum) : x[lab];
            total += w * (lse - sub);
        }
    }
    if (lane == 0) part[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = ((part[0] + part[1]) + part[2]) + part[3];
}

size_t cs_ws_bytes(int c) { return (size_t)c * 256 * sizeof(uint32_t) + 2 * (size_t)c * sizeof(uint32_t) + 256; }
int cs_check_dims(const char* who, int n, int c) {
    GRIP_REQUIRE(n >= 1 && c >= 1, "%s: n = %d, c = %d (each must be at least 1)", who, n, c);
    GRIP_REQUIRE(c <= CS_CT * 65535, "%s: c = %d (at most %d)", who, c, CS_CT * 65535);
    return GRIP_OK;
}
}  // namespace

#define RUNC(x) do { int _rc = (x); if (_rc != GRIP_OK) return _rc; } while (0)

extern "C" int grip_candidate_select_workspace(int n, int c, size_t* bytes) {
    GRIP_REQUIRE(bytes, "candidate_select_workspace: null pointer");
    RUNC(cs_check_dims("candidate_select_workspace", n, c));
    *bytes = cs_ws_bytes(c);
    return GRIP_OK;
}

extern "C" int grip_candidate_select(const float* probs, int n, int c, int claim, float tau, int combine, float* threshold, int32_t* mask, int32_t* count,
                                     int32_t* label, void* workspace, size_t workspace_bytes, void* stream) {
    RUNC(cs_check_dims("candidate_select", n, c));
    GRIP_REQUIRE(claim >= 1 && claim <= n, "candidate_select: claim = %d (in [1, n = %d])", claim, n);
    GRIP_REQUIRE(tau > 0.f && tau <= 1.f, "candidate_select: tau = %g (in (0, 1])", (double)tau);
    GRIP_REQUIRE(combine >= 0 && combine <= 3, "candidate_select: combine = %d (0 intersection, 1 union, 2 intra, 3 inter)", combine);
    GRIP_REQUIRE(probs && mask && workspace, "candidate_select: null pointer");
    GRIP_REQUIRE(workspace_bytes >= cs_ws_bytes(c), "candidate_select: workspace too small (%zu bytes, grip_candidate_select_workspace says %zu)",
                 workspace_bytes, cs_ws_bytes(c));
    hipStream_t s = (hipStream_t)stream;
    uint32_t* hist = (uint32_t*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    uint32_t* prefix = hist + (size_t)c * 256;
    uint32_t* remaining = prefix + c;
    const int64_t init_blocks = ((int64_t)c * 256 + 255) / 256;
    hipLaunchKernelGGL(cs_init_kernel, dim3((unsigned)(init_blocks < 1024 ? init_blocks : 1024)), dim3(256), 0, s, hist, prefix, remaining, c, claim);
    GRIP_CHECK_HIP(hipGetLastError());
    const dim3 hgrid((unsigned)(((int64_t)n + CS_RB - 1) / CS_RB), (unsigned)((c + CS_CT - 1) / CS_CT));
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(cs_hist_kernel, hgrid, dim3(256), 0, s, probs, n, c, prefix, shift, hist);
        GRIP_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(cs_pick_kernel, dim3((c + 63) / 64), dim3(64), 0, s, hist, prefix, remaining, c, shift, threshold);
        GRIP_CHECK_HIP(hipGetLastError());
    }
    const int words = (c + 31) / 32;
    const dim3 rgrid((unsigned)(((int64_t)n + 3) / 4));
    const float* thr = (const float*)prefix;      // the prefix after four passes is the threshold's bit pattern
#define CS_ROW(NP) hipLaunchKernelGGL(cs_row_kernel<NP>, rgrid, dim3(256), 0, s, probs, thr, n, c, words, tau, combine, mask, count, label)
    if (c <= 64) CS_ROW(1);
    else if (c <= 128) CS_ROW(2);
    else if (c <= CS_REG_C) CS_ROW(4);
    else CS_ROW(0);
#undef CS_ROW
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}

extern "C" int grip_candidate_ce(const float* logits, const int32_t* labels, const float* row_weight, int n, int c, const int32_t* cand, int64_t cand_rows,
                                 int cz, const int32_t* cand_row, const int32_t* col_map, float* loss, float* grad_logits, void* stream) {
    GRIP_REQUIRE(logits && labels && row_weight && loss, "candidate_ce: null pointer");
    GRIP_REQUIRE(n > 0 && c > 0, "candidate_ce: empty input (n = %d, c = %d)", n, c);
    size_t lds = 0;
    if (cand) {
        GRIP_REQUIRE(cand_row && col_map, "candidate_ce: null pointer (cand_row and col_map come with cand)");
        GRIP_REQUIRE(cz >= 1 && cz <= c, "candidate_ce: cz = %d (in [1, c = %d])", cz, c);
        GRIP_REQUIRE(c <= CCE_MAX_C, "candidate_ce: c = %d with candidate sets (at most %d: the inverse column map lives in the LDS)", c, CCE_MAX_C);
        lds = (size_t)c * sizeof(int);
    }
    hipLaunchKernelGGL(candidate_ce_kernel, dim3(1), dim3(256), lds, (hipStream_t)stream, logits, labels, row_weight, n, c, cand, cand_rows, cz, cand_row,
                       col_map, loss, grad_logits);
    GRIP_CHECK_HIP(hipGetLastError());
    return GRIP_OK;
}
