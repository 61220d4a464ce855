/* Test hooks and the in-library GEMM profiler of libgrip_amd.so.  NOT part of the drop-in ABI (include/grip_amd.h): nothing
 * in the reference binds to these.  They exist so that tests/test_gpu_kernels.py can check each kernel against a PyTorch fp32
 * reference through exactly the launchers the towers use, and so that bench.py can time the GEMM launches of the timed
 * region with HIP events on the launch stream (roofline block).  All return 0 or a GRIP_ERR_* code (grip_last_error()). */
#ifndef GRIP_AMD_DEBUG_H
#define GRIP_AMD_DEBUG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* out[M,N] = epilogue(A[M,K] W[N,K]^T).  epi: 0 f32 out, 1 +bias -> f16, 2 +bias, QuickGELU -> f16 (out2 = pre-activation or
 * NULL), 3 +bias +resid(f16) -> f16, 4 f16, 5 * QuickGELU'(aux) -> f16, 6 f32 * scalar.  A has m_pad >= M rows allocated.
 * variant: 0 = launcher's choice, 1..6 and 8 = a specific tile kernel (csrc/gemm_plan.cpp); 7 = the exact-mode kernel (csrc/gemm_f32.hip):
 * A, W, resid and every output are f32 (epi 0..3 and 6 only). */
int grip_debug_gemm(int epi, const void* A, const void* W, int M, int N, int K, const float* bias, const void* resid,
                    const void* aux, void* out, void* out2, float scalar, int m_pad, int variant, void* stream);
/* The LayerNorm-carrying epilogues (csrc/gemm.hip).  epi 3 with stat_part != NULL: the residual epilogue also writes, per row
 * and 64-column tile, (sum, sum of squares) of the stored values to stat_part [N/64, M, 2].  epi 7 / 8: LayerNorm folded into
 * the GEMM: out = [quickgelu](rstd_r (A W'^T - mean_r colsum) + bias) with rowstat [M, 2] = (mean, rstd), A = the raw rows. */
int grip_debug_gemm_ln(int epi, const void* A, const void* W, int M, int N, int K, const float* bias, const void* resid, void* out, void* out2,
                       float* stat_part, const float* rowstat, const float* colsum, int m_pad, int variant, void* stream);
/* The prompt-step forms of the text tower's train-mode forward (r04).  epi 7 / 8 with stat_in != NULL: the LayerNorm-folded GEMM reads the producer's
 * stat_parts partial (sum, sum of squares) pairs ([stat_parts, M, 2]) instead of finalised statistics -- inside the kernel on the loader-wave kernels,
 * through ln_stats_finalize into `rowstat` (writable, [M, 2]) otherwise.  epi 3 with ksplit > 1: cooperative split-K of the residual GEMM (partial tiles
 * in coop_scratch, >= tiles_of_64x128 * ksplit * 32 KiB; tickets in coop_counter, 4 ints per tile, zero on entry and zero again on return).
 * grip_debug_coop_split: the factor the tower would choose for this shape (1 = form not used). */
int grip_debug_gemm_train(int epi, const void* A, const void* W, int M, int N, int K, const float* bias, const void* resid, void* out, void* out2,
                          float* stat_part, float* rowstat, const float* colsum, const float* stat_in, int stat_parts, int ksplit,
                          float* coop_scratch, int* coop_counter, int m_pad, void* stream);
int grip_debug_coop_split(int M, int N, int K);
/* One f16 GEMM launch with every field of its argument block given (tests/test_gpu_gemm_kernels.py): what the four hooks above fix --
 * ldc = N, no compensated stream, rot_rows by hook -- is free here.  out / out2 / resid / aux are [M, ldc] (out may point N columns into a wider row);
 * resid_lo [M, ldc] f16 is the low half of a compensated residual stream (epi 3 with stat_part: read, and rewritten in place); epi 6 multiplies by scalar;
 * ksplit > 1 is split-K (epi 0: split_stride floats between the partials) or the cooperative form (epi 3 with coop_scratch and coop_counter).  Nothing
 * is checked beyond what the launcher itself checks. */
int grip_debug_gemm_args(int epi, const void* A, const void* W, int M, int N, int K, int ldc, const float* bias, const void* resid, void* resid_lo,
                         const void* aux, void* out, void* out2, float scalar, float* stat_part, float* rowstat, const float* colsum,
                         const float* stat_in, int stat_parts, int ksplit, int64_t split_stride, float* coop_scratch, int* coop_counter, int m_pad,
                         int variant, int rot_rows, void* stream);
/* Split-K product (the input-gradient GEMMs of the prompt steps): out = ksplit partial [M, N] f32 buffers, split_stride floats apart,
 * partial p = A[:, Kp] W[:, Kp]^T over the p-th K range.  ksplit = 0: the launcher's own choice; *ksplit_used receives the factor. */
int grip_debug_gemm_splitk(const void* A, const void* W, int M, int N, int K, float* out, int ksplit, int64_t split_stride, int* ksplit_used,
                           int m_pad, int variant, void* stream);
/* Which kernel a GEMM launch would get (csrc/gemm_plan.cpp), without launching anything: works on a machine without a GPU.  The inputs are what the
 * launcher reads of GemmArgs: the integers, `present` = which optional buffers are set (bit 0 stat_part, 1 stat_in, 2 rowstat, 3 out2, 4 coop_scratch and
 * coop_counter), and n_cu = the CUs the launch may use.  The GRIP_GEMM_* knobs of the process apply.  text receives one line,
 *   "gemm_ringw_kernel<3, 4, 1> grid 56x4 block 512 lds 81920 static_lds 0 tiles 14x4 colgroup 0 rot 2 finalize 0 variant 4"
 * (the kernel as a profiler names it; lds = dynamic bytes of the launch, static_lds = what the kernel itself declares), or the message of a refused shape, which is also the return code's grip_last_error(). */
int grip_debug_gemm_plan(int epi, int M, int N, int K, int ldc, int64_t m_pad, int variant, int ksplit, int f32, int rot_rows, int present,
                         int stat_parts, int64_t split_stride, int n_cu, char* text, int text_len);
/* Wg = f16(gamma o W) [N, K], colsum[n] = sum_k Wg[n][k], bias_out = bias + W beta; then, if stat_part != NULL,
 * rowstat [M, 2] = (mean, rstd) from the [parts, M, 2] partial sums over rows of width d.  W == NULL: the statistics alone. */
int grip_debug_ln_fold(const void* W, const float* gamma, const float* beta, const float* bias, void* Wg, float* colsum, float* bias_out,
                       int N, int K, const float* stat_part, int parts, float* rowstat, int M, int d, void* stream);
/* The split-f16 GEMM of precision-2 towers (csrc/gemm_split.hip) on f32 inputs: A [m_pad, K] and W [N, K] are rewritten in the split layout
 * ([32 x hi | 32 x lo'] f16 per 32 consecutive k) into the scratch buffers a_split / w_split (4 bytes per element), then out = epi(A W^T):
 * epi 0 f32, 1 +bias -> f32, 3 +bias +resid(f32) -> f32, 2 +bias, QuickGELU -> the split layout (4 bytes per element).  m_pad: rows of A
 * allocated, a multiple of 256.  grip_debug_split_rows: f32 rows -> the split layout. */
int grip_debug_gemm_split(int epi, const float* A, const float* W, int M, int N, int K, const float* bias, const float* resid, void* out,
                          void* a_split, void* w_split, int m_pad, void* stream);
int grip_debug_split_rows(const float* x, void* out, int64_t rows, int K, void* stream);
/* 1 when the last split-f16 GEMM launch formed the a_hi w_lo product, 0 when it ran the two-pass kernel (every element of W an f16 number:
 * grip_debug_gemm_split checks W itself, a tower at grip_tower_finalize), -1 before any launch. */
int grip_debug_split_last_wlo(void);
/* One GEMM launch of the f32 tower (tier 1: A, W, resid and every output f32) or of the split-f16 tower (tier 2: A and W images in the split layout,
 * bias / resid / out f32, the epi 2 output in the split layout; w_exact != 0: W is the duplicated image of f16-exact weights, the two-pass form) with every
 * field of its argument block given (tests/test_gpu_tier_gemm_kernels.py): out / out2 / resid are [M, ldc] (out may point some columns into a wider row).
 * Nothing is checked beyond what the launcher itself checks. */
int grip_debug_gemm_tier(int tier, int w_exact, int epi, const void* A, const void* W, int M, int N, int K, int ldc, const float* bias, const void* resid,
                         void* out, void* out2, float scalar, int64_t m_pad, void* stream);
/* The weight image of the split-f16 tier: W [rows, K] f32 -> image (4 bytes per element) in the split layout, scaled as the tier's kernels expect; dup != 0:
 * then rewritten in place as the duplicated image [32 hi | 32 hi].  flags_out[0] = 1 when a scaled element left the finite f16 range, flags_out[1] = 1 when an
 * element is not an f16 number (else 0). */
int grip_debug_split_weights(const float* W, void* image, int64_t rows, int K, int dup, int* flags_out, void* stream);
/* Attention of a precision-2 tower: qkv [B*S, 3*H*64] f32 -> out [B*S, H*64] in the split layout (4 bytes per element).  mfma != 0: the matrix-pipe
 * kernel (csrc/attention_split.hip, S <= 320), else the f32 vector-ALU kernel writing the split layout (any S). */
int grip_debug_attention_split(const void* qkv, void* out, int B, int S, int H, int causal, int mfma, void* stream);
/* out[B*S, H*64] = softmax(q k^T / 8 [+ causal mask]) v for qkv[B*S, 3*H*64] (f16). */
int grip_debug_attention(const void* qkv, void* out, int B, int S, int H, int causal, void* stream);
/* The same in f32 (exact mode, csrc/attention_f32.hip): qkv and out f32, any S. */
int grip_debug_attention_exact(const void* qkv, void* out, int B, int S, int H, int causal, void* stream);
/* dqkv from qkv, the saved forward output o and d_out (S <= 288). */
int grip_debug_attention_bwd(const void* qkv, const void* o, const void* d_out, void* dqkv, int B, int S, int H, int causal, void* stream);
/* The shared-prefix row layout of the text tower (csrc/common.h seq_row; causal only): qkv and out hold shared_rows + B (S - shared_rows) rows, the first
 * shared_rows positions once.  The backward also takes kv_part [B, shared_rows, 2, H*64] f32 (scratch: every sequence's share of the shared keys' dK / dV,
 * summed into dqkv by attn_shared_kv_reduce_kernel). */
int grip_debug_attention_shared(const void* qkv, void* out, int B, int S, int H, int shared_rows, void* stream);
int grip_debug_attention_bwd_shared(const void* qkv, const void* o, const void* d_out, void* dqkv, float* kv_part, int B, int S, int H, int shared_rows,
                                    void* stream);
/* ONE query row per sequence (the last block of a tower): out [B, H*64] f16 from qkv [B*S, 3*H*64] f16; the query of sequence b is row row_index[b] (NULL: row 0)
 * of the packed qkv or, qrows != NULL, row b of the compact qrows [B, H*64].  train != 0: the four-wave form (qrows must be NULL). */
int grip_debug_attention_row(const void* qkv, const void* qrows, const int32_t* row_index, void* out, int B, int S, int H, int causal, int train, void* stream);
/* Its backward: o_rows / do_rows [B, H*64] f16 -> the whole packed dqkv [B*S, 3*H*64] f16, zeros included. */
int grip_debug_attention_row_bwd(const void* qkv, const void* o_rows, const void* do_rows, const int32_t* row_index, void* dqkv, int B, int S, int H, int causal,
                                 void* stream);
/* The one-row form of the exact / split-f16 towers: qkv and qrows (required) f32; out [B, H*64] f32 or, split_out != 0, the split layout (4 bytes per element). */
int grip_debug_attention_row_exact(const void* qkv, const void* qrows, const int32_t* row_index, void* out, int B, int S, int H, int causal, int split_out,
                                   void* stream);
/* out[M,d] (f16) = LayerNorm(x[M,d] f32; gamma, beta), eps 1e-5. */
int grip_debug_layernorm(const float* x, const float* gamma, const float* beta, void* out, int M, int d, void* stream);
/* The backward row kernels (csrc/rowops_bwd.hip) through the launchers the towers call (tests/test_gpu_rowops_bwd.py).  x is f16, dxh f16, everything
 * else f32; widths d % 4 == 0, d <= 2048.  ln_bwd_add: dx[r] += LNbwd(sum_p dln[p * part_stride + r d ..]; x[r]), dxh = f16(dx), r < M.  ln_bwd_init:
 * dx[r] = LNbwd(..) + (r == b stride + index[b] ? rows_add[b] : 0), b = r / stride (index NULL: position 0). */
int grip_debug_ln_bwd_add(const void* x, const float* dln, int parts, int64_t part_stride, const float* gamma, float* dx, void* dxh, int M, int d, void* stream);
int grip_debug_ln_bwd_init(const void* x, const float* dln, int parts, int64_t part_stride, const float* gamma, const float* rows_add, const int32_t* index,
                           int stride, float* dx, void* dxh, int M, int d, void* stream);
/* dx[b stride + index[b]] = LNbwd(dy[b]; x[that row]), b < n.  fill = 0: only those n rows are written (first, M unused); fill = 1: every row r < M is
 * written, zero where it is no read row (sequences start at row `first`, first <= index[b] < first + stride). */
int grip_debug_ln_bwd_scatter(const void* x, const float* dy, const int32_t* index, int stride, int first, const float* gamma, float* dx, void* dxh, int n, int M,
                              int d, int fill, void* stream);
/* Visual prompt slice of dx [B*S, d] (rows b S + 1 + s).  mode 0: grad [P, d] = scale[1] sum_b LNbwd(dx row; prefix[s]); 1: per image, prefix and grad
 * [B, P, d]; 2: a deep prompt's slice, grad [P, d] = scale[1] sum_b dx row, the rows read then zeroed in dx and dxh (modes 0, 1 touch neither). */
int grip_debug_vit_prefix_grad(float* dx, void* dxh, const float* prefix, const float* gamma, const float* scale, float* grad, int B, int S, int P, int d, int mode,
                               void* stream);
/* Textual prompt slice of dx [C*T, d] (rows c T + 1 + p): grad [prefix_classes, P, d] = scale[1] x (the sum over classes in class order when
 * prefix_classes == 1, the class's own row when == C).  deep != 0: the rows summed are then zeroed in dx and dxh. */
int grip_debug_text_prefix_grad(float* dx, void* dxh, const float* scale, float* grad, int C, int T, int P, int prefix_classes, int d, int deep, void* stream);
/* scale[0] = 2^k with amax|g| 2^k in [32, 64) (|k| <= 40; k = 0 for a zero or non-finite amax), scale[1] = 2^-k, g16 = f16(g scale[0]). */
int grip_debug_grad_scale_cast(const float* g, void* g16, float* scale, int n, void* stream);
/* The forward row kernels (csrc/rowops.hip) through the launchers the towers call (tests/test_gpu_rowops_fwd.py); widths d % 4 == 0, d <= 2048.
 * LayerNorm of M rows, eps 1e-5.  f32 = 0: x f16 (the residual stream) -> out f16; 1: x f32 -> out f32; 2: x f32 -> out in the split layout (4 bytes per
 * element, d % 32 == 0).  gather = 0: row r reads x[r] (launch_layernorm_f16; row_index and row_stride unused).  gather = 1: row r reads
 * x[r * row_stride + (row_index ? row_index[r] : 0)] (launch_gather_ln_f16, the CLS / EOT form; f32 = 2 writes f32 as f32 = 1 does). */
int grip_debug_layernorm_modes(const void* x, const int32_t* row_index, int row_stride, const float* gamma, const float* beta, void* out, int f32, int gather,
                               int M, int d, void* stream);
/* Vision sequence assembly + ln_pre: x [B (1 + P + G2), d] (f32 != 0: f32, else f16) from patch_out [B G2, d], cls [d], pos [1 + G2, d] or NULL,
 * prefix [P, d] or, per_image != 0, [B, P, d]; rowstat [rows, 2] or NULL; x_lo [rows, d] f16 or NULL (f16 stream only). */
int grip_debug_vit_assemble(const float* patch_out, const float* cls, const float* pos, const float* prefix, int P, const float* gamma, const float* beta, void* x,
                            int f32, float* rowstat, int B, int G2, int d, void* x_lo, int per_image, void* stream);
/* Deep prompt rows written into a stream x of M rows.  text = 0 (launch_vit_deep_insert): rows b S + 1 + p := deep[p], b < B; prefix_classes and
 * shared_rows unused.  text != 0 (launch_text_deep_insert): B classes, deep [prefix_classes, P, d], shared_rows = 0 or P + 1 (x_lo unused).  stat_part
 * [d / 64, M, 2] and rowstat [M, 2] (each optional, f16 stream, d % 64 == 0): the statistics of the rows written. */
int grip_debug_deep_insert(const float* deep, int prefix_classes, void* x, int f32, void* x_lo, float* stat_part, float* rowstat, int B, int S, int P, int shared_rows,
                           int M, int d, int text, void* stream);
/* Token embedding + prompt splice: x [shared_rows + C (T - shared_rows), d] from ids [C, ld_ids] (clamped to [0, vocab)), tok_emb [vocab, d], pos [T, d] or NULL,
 * prefix [prefix_classes, P, d]; rowstat [rows, 2] or NULL. */
int grip_debug_text_embed(const int32_t* ids, int ld_ids, const float* tok_emb, const float* pos, const float* prefix, int P, int prefix_classes, void* x, int f32,
                          float* rowstat, int C, int T, int d, int vocab, int shared_rows, void* stream);
/* Patch gather: out [B (R / patch)^2, Kpad] (out_f32 ? f32 : f16) from images [B, 3, R, R] (images_f16 ? f16 : f32), columns >= 3 patch^2 zero. */
int grip_debug_patch_gather(const void* images, int images_f16, void* out, int out_f32, int B, int R, int patch, int Kpad, void* stream);
/* out [cols, rows] = in [rows, cols]^T, in rows ld_in elements apart (f32 ? f32 : f16). */
int grip_debug_transpose(const void* in, void* out, int f32, int rows, int cols, int ld_in, void* stream);
/* out[b] = x[b * row_stride + (row_index ? row_index[b] : 0)], rows of width d: f16 elements (d % 8 == 0), or four_byte != 0: 4-byte elements (d % 4 == 0). */
int grip_debug_gather_rows(const void* x, const int32_t* row_index, int row_stride, void* out, int n_rows, int d, int four_byte, void* stream);
/* The UPT mixer's workspace by name (csrc/mixer.hip carve_mixer, tests/test_gpu_mixer_kernels.py): buffer `index` of the carve-up for S = 2 + n_deep tokens --
 * its name (a string constant of the library), its offset in floats from the 256-byte-aligned base of the workspace and its used length in floats
 * (without the padding to 64 floats).  Non-zero past the end and for every shape the mixer refuses.  Host only: nothing is launched. */
int grip_debug_upt_mixer_slot(int n_prompt, int n_deep, int text_width, int vision_width, int dim, int index, const char** name, int64_t* offset_floats,
                              int64_t* floats);

/* The workspace of a tower pass by name (csrc/tower.hip carve, tests/test_gpu_tower_passes.py): buffer `index` of the carve-up grip_vit_forward /
 * grip_text_forward and their backwards use for (batch, n_prefix, seq_len, train, shared = the shared-prefix row layout) -- its name (a string constant of
 * the library), its layer (-1: not a per-layer buffer), its offset in bytes from the workspace base and the bytes the passes use of it (without the padding
 * to 256).  Recorded by the carve itself.  An alias is reported at the offset of the buffer it lies on ("patches" on "h").  Non-zero past the end and for
 * everything the carve refuses.  Host only: nothing is launched.  Weights: grip_layout_slot. */
int grip_debug_tower_slot(const struct grip_tower* tower, int batch, int n_prefix, int seq_len, int train, int shared, int index, const char** name, int* layer,
                          int64_t* offset_bytes, int64_t* bytes);
/* Launch budget of the NEXT tower pass of the calling host thread (grip_vit_forward*, grip_text_forward*, grip_*_backward_*): the pass issues its first n kernel
 * launches, then returns GRIP_ERR_LAUNCH_BUDGET between two launches; grip_last_error() reads "launch budget: stopped after <n> launches, before <the call
 * that would have come next>".  n <= 0: off (the default).  The budget switches itself off when it trips and when a pass returns, so n >= the launches of
 * the pass lets it finish.  Only kernel launches count.  A forward stopped early registers no pending state; a backward stopped early has consumed its
 * forward.  While off, a launch costs one comparison of a thread-local host integer, and a pass two stores to it. */
#define GRIP_ERR_LAUNCH_BUDGET 64
int grip_debug_launch_budget(int64_t n);

/* GEMM launch profiler: while enabled, every 4th GEMM launch is bracketed by HIP events on its stream. */
int grip_profile_enable(int on);
/* Per slot (variant * 16 + epilogue id) in [0, n): launches sampled, their total milliseconds and total 2*M*N*K. */
int grip_profile_collect(int n, int64_t* launches, double* total_ms, double* total_flops);

#ifdef __cplusplus
}
#endif
#endif
