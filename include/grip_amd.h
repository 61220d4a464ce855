/* grip_amd.h -- C ABI of the MI355X-native CLIP prompt-tuning + pseudolabel engine.
 *
 * The reference (BatsResearch/menghini-neurips23-code) is pure Python and has no FFI; its
 * "operator API" for the hot path is a set of Python classes over the third-party `clip`
 * package.  Each entry point below replaces the arithmetic behind one of them; the Python
 * host layer in menghini-neurips23-code_amd/{clip,models,utils} keeps the reference's class
 * and function signatures and binds these symbols with ctypes.
 *
 * Conventions: extern "C"; every function returns 0 on success and a non-zero grip_status
 * otherwise (grip_last_error() gives the message); no C++ exception crosses the boundary; the
 * caller owns every buffer; all device work is enqueued on the caller's hipStream_t (passed as
 * void*); handles are not thread-safe (one per process / GPU); no hidden device allocation after
 * grip_tower_create.  Device pointers are plain pointers into HBM (torch tensors' data_ptr()).
 *
 * Dtypes: GEMM operands and the residual stream f16 (MFMA v_mfma_f32_16x16x32_f16, f32 accumulate, adds into the
 * stream in f32); LayerNorm statistics, softmax, head, embeddings and gradients f32.  A tower created with
 * dims.precision = 1 computes everything in f32 instead (exact comparison mode, inference only); dims.precision = 2 is the f32 tower with its
 * block GEMMs and attention on the f16 matrix pipes as hi / lo operand pairs (three products, f32 accumulate: ~22 mantissa bits; inference only).
 */
#ifndef GRIP_AMD_H
#define GRIP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GRIP_OK = 0,
    GRIP_ERR_ARG = 1,        /* bad dimension / null pointer / unsupported shape */
    GRIP_ERR_HIP = 2,        /* a HIP runtime call or kernel launch failed */
    GRIP_ERR_WORKSPACE = 3,  /* workspace too small */
    GRIP_ERR_STATE = 4       /* backward without a matching training-mode forward, tower not finalized */
} grip_status;

const char* grip_last_error(void);
/* ABI version of this header; the host layer refuses a library that reports another one. */
int grip_abi_version(void);
#define GRIP_ABI_VERSION 9

/* ------------------------------------------------------------------------------------------
 * Tower description.  kind 0 = vision transformer (clip_model.visual, wrapped by
 * CustomVisionTransformer, models/clip_encoders.py:105-194), kind 1 = text transformer
 * (clip_model.{token_embedding, positional_embedding, transformer, ln_final, text_projection},
 * wrapped by CustomTextEncoder, models/clip_encoders.py:25-90).  Head dim is width / heads = 64. */
typedef struct {
    int32_t kind;        /* 0 vision, 1 text */
    int32_t width;       /* d: 768 (ViT-B), 1024 (ViT-L); text 512 / 768 */
    int32_t layers;
    int32_t heads;       /* width / 64 */
    int32_t embed_dim;   /* E: 512 / 768 */
    int32_t seq0;        /* tokens without prompt: grid^2 + 1 (vision) or context length 77 (text) */
    int32_t patch;       /* vision: patch size; text: 0 */
    int32_t resolution;  /* vision: input resolution; text: 0 */
    int32_t vocab;       /* text: vocabulary size; vision: 0 */
    int32_t max_prefix;  /* largest number of prompt tokens any call will use (sizes nothing but checks) */
    int32_t precision;   /* 0 = f16 GEMM operands + f16 residual stream (what clip.load gives the reference on a GPU);
                            1 = exact comparison mode: f32 weights, activations, residual stream and attention
                            (v_mfma_f32_16x16x4_f32), i.e. the arithmetic of the reference's CPU path (clip.load(..., "cpu")
                            keeps fp32).  Inference only: train != 0 is GRIP_ERR_ARG on a precision-1 tower.
                            2 = split f16 (the middle tier of the screen-and-refine pseudolabel pass): blobs, activations, residual stream,
                            LayerNorm, softmax and every interface as precision 1; the four GEMMs of a block and the attention products
                            carry each operand as f16 hi + f16 lo (x = hi + lo) and form a b from three v_mfma_f32_16x16x32_f16 with f32
                            accumulation (a_hi b_hi + a_hi b_lo + a_lo b_hi): embeddings within ~1e-6 relative of the precision-1 tower's
                            at ~2.5x its throughput.  grip_tower_finalize derives the split weight copies (slots "...#S").  Inference
                            only; width must be a multiple of 256. */
} grip_dims;

/* Weight layout.  A tower's frozen weights live in two caller-owned device blobs: one f16 (GEMM
 * operands) and one f32 (biases, LayerNorm affine, embeddings).  grip_layout_slot enumerates the
 * slots: `name` is the OpenAI state_dict key relative to the tower (e.g.
 * "transformer.resblocks.3.attn.in_proj_weight", "conv1.weight", "proj") for primary slots the
 * host fills, or ends in "#T" for derived slots (transposed copies used by the backward pass,
 * written by grip_tower_finalize).  Returns GRIP_OK, or GRIP_ERR_ARG when `slot` is past the end. */
typedef struct {
    char name[96];
    int32_t dtype;      /* 0 = GEMM-operand blob (f16; f32 elements when dims.precision != 0), 1 = f32 blob */
    int32_t derived;    /* 1 = written by grip_tower_finalize */
    int64_t offset;     /* element offset inside its blob (16-byte aligned) */
    int64_t rows;       /* logical shape rows x cols, row-major */
    int64_t cols;
    int64_t ld;         /* leading dimension in elements (>= cols; conv1 rows are zero-padded to a multiple of 64) */
} grip_slot;

int grip_layout_slot(const grip_dims* dims, int slot, grip_slot* out);
int grip_layout_size(const grip_dims* dims, int64_t* n_f16, int64_t* n_f32);

typedef struct grip_tower grip_tower;

/* Replaces clip.load's module construction for one tower.  Blobs must outlive the handle.  `f16_blob` is the GEMM-operand
 * blob of n_f16 ELEMENTS: f16, or f32 when dims.precision != 0. */
int grip_tower_create(const grip_dims* dims, void* f16_blob, void* f32_blob, grip_tower** out);
/* Builds derived weights (transposed copies) on `stream`; call after the primary slots are filled
 * and again whenever they change. */
int grip_tower_finalize(grip_tower* t, void* stream);
int grip_tower_destroy(grip_tower* t);

/* Workspace bytes for a forward over `batch` units (images, or class prompts for the text tower)
 * with `n_prefix` prompt tokens.  seq_len: text tower only, see grip_text_forward (0 = full context; pass 0 for the
 * vision tower).  train != 0 keeps the activations backward needs. */
int grip_workspace_bytes(const grip_tower* t, int batch, int n_prefix, int seq_len, int train, size_t* bytes);

/* ------------------------------------------------------------------------------------------
 * CustomVisionTransformer.forward(x, image_prefix) / clip_model.encode_image(x)
 * (models/clip_encoders.py:123-194; :93-102 with n_prefix = 0).
 *   images     [batch, 3, R, R] f32 (images_f16 = 0) or f16 (images_f16 = 1), NCHW
 *   prefix     [n_prefix, width] f32, or NULL when n_prefix == 0; inserted between CLS and the
 *              patches after the positional embedding, shared by the whole batch (image_prefix [P, d] / [1, P, d] expanded,
 *              :148).  With GRIP_FWD_PER_IMAGE_PREFIX: [batch, n_prefix, width] f32, image b's tokens 1 .. n_prefix are prefix[b]
 *              (image_prefix [B, P, d], one prompt per image).
 *   out_emb    [batch, embed_dim] f32 (un-normalised, as the reference returns it)
 *   flags      GRIP_FWD_TRAIN (= the `train` argument of earlier ABIs: 1 keeps the activations backward needs) and / or
 *              GRIP_FWD_NO_POS_EMB (forward(..., pos_emb=False), :141: CLS and patches without the positional embedding) and / or
 *              GRIP_FWD_PER_IMAGE_PREFIX (ABI 9: prefix holds one prompt per image, see above; valid with every tower precision and with
 *              GRIP_FWD_TRAIN, GRIP_FWD_NO_POS_EMB and GRIP_FWD_STREAM_HILO; an error on a text tower, whose per-class contexts are
 *              prefix_classes = n_class).  Without it every kernel runs exactly as in ABI 8.
 *   generation NULL, or receives the number of this train-mode forward (0 without GRIP_FWD_TRAIN).  Several train-mode forwards may
 *              be outstanding, each on its own workspace; a second one on the SAME workspace overwrites the first one's
 *              saved activations, and a backward that presents the first one's number then fails with GRIP_ERR_STATE.  The train-mode
 *              state also records GRIP_FWD_PER_IMAGE_PREFIX: it decides the shape of grip_vit_backward_prefix's grad_prefix.
 */
int grip_vit_forward(grip_tower* t, const void* images, int images_f16, const float* prefix, int n_prefix,
                     int batch, float* out_emb, void* workspace, size_t workspace_bytes, int flags, uint64_t* generation, void* stream);

/* Deep visual prompts (VPT-Deep; ABI 9 addition -- grip_vit_forward is this call with deep = NULL, n_deep = 0, and runs exactly as before):
 *   deep       [n_deep, n_prefix, width] f32, shared by the batch.  Before block l (1 <= l <= n_deep) the rows 1 .. n_prefix of every image's
 *              residual stream are replaced by deep[l - 1]: no LayerNorm, no positional embedding (the reference's deep_embs branch,
 *              models/clip_encoders.py:166-184, with its vpt_proj / vpt_dropout as identity).  Block 0 reads the shallow prompt as above.
 *   n_deep     0 .. layers - 1; n_deep > 0 needs n_prefix > 0 and deep != NULL, and is refused with GRIP_FWD_PER_IMAGE_PREFIX and on a text tower.
 * Every tower precision and flag otherwise as grip_vit_forward.  A train-mode forward records n_deep: its backward is grip_vit_backward_deep
 * (grip_vit_backward_prefix then fails with GRIP_ERR_STATE). */
int grip_vit_forward_deep(grip_tower* t, const void* images, int images_f16, const float* prefix, int n_prefix, const float* deep, int n_deep,
                          int batch, float* out_emb, void* workspace, size_t workspace_bytes, int flags, uint64_t* generation, void* stream);

/* Input-gradient chain of the frozen ViT down to the prompt slice (autograd of the above w.r.t.
 * image_prefix only; no weight gradients exist).  Must follow a train-mode forward on the same
 * workspace, exactly once per forward; generation = the number that forward returned (0 = do not check).  grad_emb [batch, embed_dim] f32 -> grad_prefix [n_prefix, width] f32 (summed over batch).
 * After a forward with GRIP_FWD_PER_IMAGE_PREFIX: prefix (the same tensor the forward read) and grad_prefix are [batch, n_prefix, width] f32 -- image b's
 * prompt gradient alone, no sum over the batch (autograd of image_prefix [B, P, d]); bit-reproducible (no atomics, one writer per element). */
int grip_vit_backward_prefix(grip_tower* t, const float* grad_emb, const float* prefix, float* grad_prefix,
                             void* workspace, size_t workspace_bytes, uint64_t generation, void* stream);

/* The same after grip_vit_forward_deep (ABI 9 addition): grad_prefix as grip_vit_backward_prefix, and grad_deep [n_deep, n_prefix, width] f32 -- grad_deep[l - 1]
 * is the gradient of the stream rows 1 .. n_prefix entering block l, summed over the batch in a fixed order (no atomics: the same bits on every run).
 * Those rows get no gradient below block l (they were overwritten), so the shallow prompt's gradient flows through block 0 alone.  After a forward
 * without deep prompts grad_deep is not touched (may be NULL). */
int grip_vit_backward_deep(grip_tower* t, const float* grad_emb, const float* prefix, float* grad_prefix, float* grad_deep,
                           void* workspace, size_t workspace_bytes, uint64_t generation, void* stream);

/* CustomTextEncoder.forward(class_embeddings, classes) / clip_model.encode_text(tokens)
 * (models/clip_encoders.py:43-90; :13-22 with n_prefix = 0).  Tokenisation stays on the host.
 *   token_ids  [n_class, seq0] int32 device; eot_index [n_class] int32 device (= token_ids.argmax(-1))
 *   prefix     [prefix_classes, n_prefix, width] f32; prefix_classes is 1 (broadcast, CoOp) or n_class
 *   seq_len    0 or seq0: encode all seq0 positions as the reference does.  0 < seq_len < seq0: encode only the first
 *              seq_len positions; must be > max(eot_index).  The text transformer is causal and only the EOT row is
 *              read, so positions after the last EOT cannot influence any output: the result is the same, the work
 *              shrinks by seq0 / seq_len (CoOp prompts are ~20 of 77 tokens).
 *   out_emb    [n_class, embed_dim] f32
 *   flags      GRIP_FWD_TRAIN: keep the activations grip_text_backward_prefix needs (the `train` argument of ABI <= 3).
 *              GRIP_FWD_SHARED_PREFIX: the caller vouches that token_ids[c][0 .. n_prefix] is the same for every class
 *              (SOT + the context placeholders of CustomTextEncoder, :63-74) and eot_index[c] > n_prefix.  With one shared
 *              context (prefix_classes == 1) those 1 + n_prefix positions then carry identical activations for every class
 *              in every layer -- same inputs, same positions, causal mask -- so the engine encodes them ONCE and keeps
 *              only the class-specific positions per class (1 + n_prefix + n_class * (seq_len - 1 - n_prefix) rows
 *              instead of n_class * seq_len: 425 instead of 2 142 for 102 classes x 21 positions, 16 context tokens); the
 *              class positions attend to the shared keys and their own, and the backward adds every class's share of
 *              the shared keys' gradient in class order.  Embeddings and prompt gradient are the same function of the
 *              inputs; ignored (plain layout) when prefix_classes != 1, n_prefix == 0 or dims.precision != 0.
 *              GRIP_FWD_NO_POS_EMB: CustomTextEncoder.forward(enable_pos_emb=False), x = token / prompt embeddings only.
 */
#define GRIP_FWD_TRAIN 1
#define GRIP_FWD_SHARED_PREFIX 2
#define GRIP_FWD_NO_POS_EMB 4 /* models/clip_encoders.py:70-74, enable_pos_emb=False: the positional embedding is not added */
#define GRIP_FWD_STREAM_HILO 8 /* grip_vit_forward, inference on an f16 tower (ABI 8): the residual stream is carried as a COMPENSATED pair of f16 numbers
                                  (hi + lo, ~22 mantissa bits; every add into it in f32 as before), so the 2 x layers roundings of the stream no longer
                                  accumulate -- measured: 2.5 - 3x less direction error against the f32 tower for ~2 bytes more traffic per stream element and
                                  residual GEMM.  GEMM operands stay f16 (the hi part).  The SCREEN of the pseudolabel pass (grip_amd.pseudolabels) runs in
                                  this mode; train-mode forwards and every other caller keep the plain f16 stream the reference's GPU path has. */
#define GRIP_FWD_PER_IMAGE_PREFIX 32 /* grip_vit_forward (ABI 9): prefix is [batch, n_prefix, width], one prompt per image (see grip_vit_forward).  Bit 16 stays unassigned. */
int grip_text_forward(grip_tower* t, const int32_t* token_ids, const int32_t* eot_index, const float* prefix,
                      int n_prefix, int prefix_classes, int n_class, int seq_len, float* out_emb,
                      void* workspace, size_t workspace_bytes, int flags, uint64_t* generation, void* stream);

/* Deep text prompts (deep CoOp, the language half of MaPLe-style deep prompting; ABI 9 addition -- grip_text_forward is this call with deep = NULL, n_deep = 0,
 * and runs exactly as before):
 *   deep       [n_deep, prefix_classes, n_prefix, width] f32.  Before block l (1 <= l <= n_deep) the positions 1 .. n_prefix of every class's residual stream
 *              are replaced by deep[l - 1] (class c reads deep[l - 1][c], or deep[l - 1][0] when prefix_classes == 1): no LayerNorm, no positional and no
 *              token embedding.  Block 0 reads the shallow context as above.  The replaced rows are again the same for every class when the context is
 *              shared and the mask is causal, so GRIP_FWD_SHARED_PREFIX stays valid: the shared layout writes the n_prefix rows once.
 *   n_deep     0 .. layers - 1; n_deep > 0 needs n_prefix > 0 and deep != NULL, and is refused on a vision tower (grip_vit_forward_deep is its call).
 * Every tower precision, flag and legal seq_len otherwise as grip_text_forward.  A train-mode forward records n_deep: its backward is
 * grip_text_backward_deep (grip_text_backward_prefix then fails with GRIP_ERR_STATE). */
int grip_text_forward_deep(grip_tower* t, const int32_t* token_ids, const int32_t* eot_index, const float* prefix,
                           int n_prefix, int prefix_classes, const float* deep, int n_deep, int n_class, int seq_len, float* out_emb,
                           void* workspace, size_t workspace_bytes, int flags, uint64_t* generation, void* stream);

/* grad_emb [n_class, embed_dim] -> grad_prefix [prefix_classes, n_prefix, width] (summed over classes
 * when prefix_classes == 1). */
int grip_text_backward_prefix(grip_tower* t, const float* grad_emb, float* grad_prefix,
                              void* workspace, size_t workspace_bytes, uint64_t generation, void* stream);

/* The same after grip_text_forward_deep (ABI 9 addition): grad_prefix as grip_text_backward_prefix, and grad_deep [n_deep, prefix_classes, n_prefix, width] f32 --
 * grad_deep[l - 1] is the gradient of the stream rows 1 .. n_prefix entering block l, summed over the classes in class order when prefix_classes == 1, each
 * class's own otherwise (no atomics: the same bits on every run).  Those rows get no gradient below block l (they were overwritten), so the shallow
 * context's gradient flows through block 0 alone.  After a forward without deep prompts grad_deep is not touched (may be NULL). */
int grip_text_backward_deep(grip_tower* t, const float* grad_emb, float* grad_prefix, float* grad_deep,
                            void* workspace, size_t workspace_bytes, uint64_t generation, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cosine x logit-scale head + softmax + argmax: the block inlined 45 times in the reference, e.g.
 * methods/semi_supervised_learning/textual_prompt.py:98-109, and utils/clip_pseudolabels.py:35-41.
 *   img_emb [n, e] f32, txt_emb [c, e] f32 (both un-normalised), scale = logit_scale.exp()
 *   logits [n, c] f32; probs [n, c] f32 (softmax) or NULL; argmax_logits / argmax_probs [n] int32 or NULL
 *   txt_norm_scratch [c, e] f32 device scratch
 */
int grip_cosine_head(const float* img_emb, const float* txt_emb, float scale, int n, int c, int e,
                     float* logits, float* probs, int32_t* argmax_logits, int32_t* argmax_probs,
                     float* txt_norm_scratch, void* stream);

/* Backward of logits = scale * normalize(img) @ normalize(txt).T :
 * grad_logits [n, c] -> grad_img [n, e] and/or grad_txt [c, e] (either may be NULL).  grad_logits is used as given: it carries no
 * labels, so a row whose label grip_weighted_ce found outside [0, c) arrives here as w_i * softmax (no one-hot subtracted) and
 * contributes that to both gradients. */
int grip_cosine_head_backward(const float* img_emb, const float* txt_emb, float scale, int n, int c, int e,
                              const float* grad_logits, float* grad_img, float* grad_txt, void* stream);

/* Mean cross-entropy over the rows with row_weight != 0, each weighted: the three FPL losses
 * (methods/semi_supervised_learning/textual_fpl.py:123-165, methods/transductive_zsl/textual_fpl.py:117-147,
 * methods/unsupervised_learning/visual_fpl.py:107-122) are sums of two such masked means; the host
 * passes per-row weights w_i = gamma_group / |group|.  loss [1] f32, grad_logits [n, c] f32 or NULL.
 * A label outside [0, c) is not an error: the row is left out of the loss (as a row of weight 0 is) and no one-hot is
 * subtracted from its gradient row, which is w_i * softmax(logits_i).  All weights zero: the loss is exactly 0. */
int grip_weighted_ce(const float* logits, const int32_t* labels, const float* row_weight, int n, int c,
                     float* loss, float* grad_logits, void* stream);

/* ------------------------------------------------------------------------------------------
 * UPTModel's prompt mixer (models/prompts_models.py:99-119 construct it, :129-146 run it): proj_coop_pre / proj_vpt_pre (Linear
 * to `dim`), clip.model.Transformer(width = dim, layers = 1, heads = 1) over the sequence cat((coop, vpt), dim 0) = [2, P, dim]
 * (sequence length 2, batch P), the .to(float16) round trip of :138-145, proj_coop_post / proj_vpt_post.  The only trainable
 * weights on the path: grip_upt_mixer_backward returns the gradient of EVERY tensor of the struct (float32 values; the
 * reference's float16 branch, multimodal_prompt.py:46, is the same kernels with fp16 rounding points: half_linears).
 * One struct describes the tensors (forward: values; backward's `grads`: buffers of the same shapes that receive the gradients):
 *   coop [P, text_width], vpt [P, vision_width]                 coop_embeddings / vpt_embeddings (P = n_prompt tokens each)
 *   coop_pre_w [dim, text_width], coop_pre_b [dim]              proj_coop_pre;   vpt_pre_* likewise with vision_width
 *   ln1_g, ln1_b [dim]; in_w [3 dim, dim], in_b [3 dim]; out_w [dim, dim], out_b [dim]      resblocks.0.ln_1 / attn.in_proj_* / attn.out_proj
 *   ln2_g, ln2_b [dim]; fc_w [4 dim, dim], fc_b [4 dim]; proj_w [dim, 4 dim], proj_b [dim]  resblocks.0.ln_2 / mlp.c_fc / mlp.c_proj
 *   coop_post_w [text_width, dim], coop_post_b [text_width]     proj_coop_post;  vpt_post_* likewise
 * forward:  coop_out [P, text_width], vpt_out [P, vision_width] (what CustomTextEncoder / CustomImageEncoder receive as prompts).
 * backward: d_coop_out / d_vpt_out = the prompt gradients grip_text_backward_prefix / grip_vit_backward_prefix returned; must follow
 * a forward on the same workspace (it holds the saved activations).  The gradient entering the fp16 tensor is rounded to fp16 as
 * autograd does.  All device pointers f32; work is enqueued on `stream`; no atomics (bit-reproducible). */
typedef struct {
    int32_t n_prompt, text_width, vision_width, dim;
    int32_t half_linears;   /* 1 = the reference's float16 branch (multimodal_prompt.py:46 on a GPU): the four projection Linears and the two prompt embeddings are
                               fp16 tensors around the fp32 block.  The host passes their values as f32 (exactly representable); the outputs of the pre / post
                               projections are rounded to fp16, and in the backward so are the gradient entering proj_*_pre (it crosses the fp16 -> fp32 cast
                               in front of the block) and the prompt gradients.  Parameter gradients come back f32; the host casts them to the parameters' dtype. */
    int32_t reserved_;
    float *coop, *vpt;
    float *coop_pre_w, *coop_pre_b, *vpt_pre_w, *vpt_pre_b;
    float *ln1_g, *ln1_b, *in_w, *in_b, *out_w, *out_b, *ln2_g, *ln2_b, *fc_w, *fc_b, *proj_w, *proj_b;
    float *coop_post_w, *coop_post_b, *vpt_post_w, *vpt_post_b;
} grip_upt_mixer;
int grip_upt_mixer_workspace(int n_prompt, int text_width, int vision_width, int dim, size_t* bytes);
int grip_upt_mixer_forward(const grip_upt_mixer* m, float* coop_out, float* vpt_out, void* workspace, size_t workspace_bytes, void* stream);
int grip_upt_mixer_backward(const grip_upt_mixer* m, const float* d_coop_out, const float* d_vpt_out, const grip_upt_mixer* grads,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Deep UPT (ABI 9 additions; with n_deep = 0 these are the three calls above, bit for bit): UPTModel's vpt_embeddings_deep (models/prompts_models.py:69,
 * :94-97) mixed with the prompts as :133-134 and :146 intend -- proj_vpt_pre(cat(vpt, vpt_deep)), the block over the sequence
 * (coop, vpt, deep[0] .. deep[n_deep - 1]) of length S = 2 + n_deep (batch P), proj_vpt_post of the rows 1 .. S - 1.  The outputs feed the image
 * tower's deep prompts (grip_vit_forward_deep).  Same struct, rounding points (half_linears) and determinism as the shallow mixer.
 *   n_deep           0 .. 31
 *   vpt_deep         [n_deep, P, vision_width]      the deep prompt embeddings (the backward takes the forward's values, as it does m->vpt)
 *   vpt_deep_out     [n_deep, P, vision_width]      proj_vpt_post of the deep rows: the deep visual prompts of blocks 1 .. n_deep
 *   d_vpt_deep_out   its gradient (grip_vit_backward_deep's grad_deep);  grad_vpt_deep [n_deep, P, vision_width] <- the deep embeddings' gradient
 * The workspace of n_deep > 0 is larger: grip_upt_mixer_deep_workspace. */
int grip_upt_mixer_deep_workspace(int n_prompt, int n_deep, int text_width, int vision_width, int dim, size_t* bytes);
int grip_upt_mixer_forward_deep(const grip_upt_mixer* m, const float* vpt_deep, int n_deep, float* coop_out, float* vpt_out, float* vpt_deep_out,
                                void* workspace, size_t workspace_bytes, void* stream);
int grip_upt_mixer_backward_deep(const grip_upt_mixer* m, const float* vpt_deep, int n_deep, const float* d_coop_out, const float* d_vpt_out,
                                 const float* d_vpt_deep_out, const grip_upt_mixer* grads, float* grad_vpt_deep, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 additions) MaPLe coupling function (models/prompts_models.py MaPLeModel; csrc/couple.hip): every visual prompt is a trainable Linear of
 * the text prompt of the same depth, independent weights per depth.  All tensors f32, device, 16-byte aligned.
 *   ctx          [P, text_width]                      the shallow text context
 *   deep_text    [n_deep, P, text_width]              the deep text prompts of blocks 1 .. n_deep (null when n_deep == 0)
 *   w            [1 + n_deep, vision_width, text_width], b [1 + n_deep, vision_width]      nn.Linear layout (y = x W^T + b); row 0 = shallow, row l = block l
 *   vis_prefix   [P, vision_width] = ctx w[0]^T + b[0];   vis_deep [n_deep, P, vision_width], vis_deep[l - 1] = deep_text[l - 1] w[l]^T + b[l]
 *   backward: d_vis_prefix / d_vis_deep (what grip_vit_backward_deep returns) -> d_w[l] = dY[l]^T X[l], d_b[l] = sum_p dY[l][p], d_ctx / d_deep_text = dY[l] w[l]
 *             (the coupling's share only: the text tower's gradient of the same tensors is added by the caller).
 *   P 1 .. 16, n_deep 0 .. 31, widths multiples of 64 up to 1024.  One launch forward; two backward (w is read once, d_w written once; the second launch
 *   adds the partial d_ctx / d_deep_text of the workspace in a fixed order: no atomics, bit-reproducible).  workspace: grip_prompt_couple_workspace bytes,
 *   scratch of the backward only. */
int grip_prompt_couple_workspace(int n_prompt, int n_deep, int text_width, int vision_width, size_t* bytes);
int grip_prompt_couple_forward(const float* ctx, const float* deep_text, int n_prompt, int n_deep, int text_width, int vision_width, const float* w,
                               const float* b, float* vis_prefix, float* vis_deep, void* stream);
int grip_prompt_couple_backward(const float* ctx, const float* deep_text, int n_prompt, int n_deep, int text_width, int vision_width, const float* w,
                                const float* d_vis_prefix, const float* d_vis_deep, float* d_ctx, float* d_deep_text, float* d_w, float* d_b,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 additions) Key/value cache head (Tip-Adapter; models/cache_models.py TipAdapterModel; csrc/cache_head.hip).  All tensors f32 on the device,
 * img_emb / keys / grad_keys 16-byte aligned.
 *   img_emb      [n, e]     image embeddings, NOT normalised (as grip_cosine_head takes them); f^_i = f_i / |f_i| is folded into the score
 *   keys         [m, e]     the cache keys, grouped by class and used as stored (not renormalised)
 *   class_start  [c + 1]    int32, device: class y owns the key rows class_start[y] .. class_start[y + 1] - 1; class_start[0] = 0, class_start[c] = m,
 *                           non-decreasing (the caller's duty: it is device data); a class may own no key
 *   key_weight   [m]        v_j, or NULL for 1
 *   forward:  logits_inout[i, y] += alpha * sum_{j in class y} v_j exp(-beta (1 - f^_i . k_j)); the column of a class without keys is not written
 *   backward: grad_keys[j, d] = alpha beta v_j sum_i grad_logits[i, y(j)] exp(-beta (1 - f^_i . k_j)) f^_id -- written, not accumulated; it recomputes
 *             the affinities and needs no forward before it.  (No gradient to img_emb: the image tower of the strategies that use the head is frozen.)
 *   e a multiple of 4 up to 2048; n, m, c >= 1, any c.  The products run on the f32 MFMA; the [n, m] affinities never reach memory; no atomics, one
 *   writer per element, fixed summation order: bit-reproducible, and the bits of a row do not depend on n or on the call the row is in.
 *   workspace: grip_cache_head_workspace bytes (the reciprocal row norms), scratch of either call. */
int grip_cache_head_workspace(int n, int m, int c, int e, size_t* bytes);
int grip_cache_head_forward(const float* img_emb, const float* keys, const int32_t* class_start, const float* key_weight, float alpha, float beta,
                            int n, int m, int c, int e, float* logits_inout, void* workspace, size_t workspace_bytes, void* stream);
int grip_cache_head_backward(const float* img_emb, const float* keys, const int32_t* class_start, const float* key_weight, float alpha, float beta,
                             int n, int m, int c, int e, const float* grad_logits, float* grad_keys, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 additions) Feature adapter (CLIP-Adapter; models/adapter_models.py ClipAdapterModel; csrc/feature_adapter.hip): a bias-free bottleneck MLP on
 * the image embedding, blended back into it.  All tensors f32 on the device and 16-byte aligned.
 *   img_emb  [n, e]   image embeddings, NOT normalised (the tower's output; grip_cosine_head normalises what this returns)
 *   w1 [h, e], w2 [e, h]   the two bias-free layers in nn.Linear layout
 *   forward:  out[n, e] = ratio * ReLU(ReLU(img_emb w1^T) w2^T) + (1 - ratio) * img_emb, ONE launch; the hidden activations stay in LDS.
 *             hidden_out [n, h] / act_out [n, e]: both NULL (inference) or both given (training): the post-ReLU hidden and the post-ReLU x, all the
 *             backward needs.  out must not alias img_emb.  ratio = 0 returns img_emb and ratio = 1 returns x, bit for bit.
 *   backward: dX = ratio * grad_out o [act > 0];  grad_w2 = dX^T hidden;  dH = (dX w2) o [hidden > 0];  grad_w1 = dH^T img_emb -- written, not
 *             accumulated; a pure function of its arguments (it needs no forward before it; the masks are read from hidden / act, strictly > 0).
 *             Two launches.  (No gradient to img_emb: the image tower of the strategies that use the head is frozen.)
 *   e a multiple of 64, 64 .. 1024; h a multiple of 16, 16 .. 256; n >= 1.  The products run on the f32 MFMA; no atomics, one writer per element,
 *   every element one chain in a fixed order (the rows of a gradient in ascending order): bit-reproducible, and the bits of a forward row do not
 *   depend on n, on the row's place in a tile or on the call the row is in.
 *   workspace (backward only): grip_feature_adapter_workspace bytes = n * h * 4 + 256 (dH and alignment slack): it holds NO e * h partial,
 *   whatever n is.  The workspace call needs no device. */
int grip_feature_adapter_workspace(int n, int e, int h, size_t* bytes);
int grip_feature_adapter_forward(const float* img_emb, const float* w1, const float* w2, float ratio, int n, int e, int h, float* out, float* hidden_out,
                                 float* act_out, void* stream);
int grip_feature_adapter_backward(const float* img_emb, const float* w2, const float* hidden, const float* act, const float* grad_out, float ratio, int n,
                                  int e, int h, float* grad_w1, float* grad_w2, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 additions) Transductive label propagation over a pool (pseudolabels.LabelPropagation; csrc/knn_graph.hip): a kNN graph of image
 * embeddings and a random walk of class probabilities over it.  All tensors f32 / int32 on the device; queries, base and out 16-byte aligned.
 *
 * grip_knn_graph: row i of idx_out / sim_out [n, k] lists the k rows j of `base` with the largest cosine s_ij = (q_i . x_j) / (|q_i| |x_j|), under
 * the TOTAL order (sim descending, then index ascending), written in that order.
 *   queries [n, e], base [m, e]   embeddings, NOT normalised (as grip_cosine_head takes them): the reciprocal norms scale the score
 *   self_offset   >= 0: query i IS base row self_offset + i and that row is excluded for it (pool on pool: queries == base, 0; a window of the
 *                 base: queries == base + self_offset * e -- the norms are then computed once); -1: nothing is excluded
 *   e a multiple of 4 up to 2048; 1 <= k <= 32; n, m >= 1; m - (self_offset >= 0) >= k; with self_offset >= 0, self_offset + n <= m.
 *   Finite rows of non-zero norm are the CALLER's duty (device data): a NaN or a zero row makes the lists of the rows that meet it meaningless.
 *   The products run on the f32 MFMA and the [n, m] scores never reach memory; no atomics.  A score is one MFMA chain over e in ascending order (an
 *   fmaf chain) times the two reciprocal norms, so the idx / sim bits of a query row depend on that row and the base only -- not on n, on the row's
 *   place in a tile or on the call -- and bit-identical base rows tie, the lower index first.
 *   workspace: grip_knn_graph_workspace bytes (the reciprocal norms and, with few query rows, the per-share lists that a second launch merges under
 *   the same total order).  The workspace call needs no device.
 *
 * grip_label_propagate: random-walk propagation on the DIRECTED kNN graph (idx refers to rows of the same set: values in [0, n) are the caller's duty)
 *   w_ik = exp(gamma (sim_ik - sim_i0)) / sum_k' exp(gamma (sim_ik' - sim_i0))        (sim_i0: the row's first = largest entry)
 *   Z^0 = probs,  Z^{t+1}_i = fmaf(alpha, sum_k w_ik Z^t_{idx_ik}, (1 - alpha) probs_i),  t = 0 .. iters - 1;  out = Z^iters
 *   probs, out [n, c]; idx, sim [n, k]; argmax_out [n] int32 or NULL: the first index of the maximum of out's row.  The k neighbours are added in
 *   list order; alpha = 0 returns probs bit for bit.  0 <= alpha < 1, gamma >= 0, iters >= 1, 1 <= k <= 32, any c >= 1; out must not alias probs.
 *   One call enqueues the weights and the `iters` steps, ping-ponging between out and the workspace (grip_label_propagate_workspace bytes).
 *   This is NOT ZLaP's symmetrised, conjugate-gradient-solved system: no class (text) nodes, no symmetrisation, no convergence test. */
int grip_knn_graph_workspace(int n, int m, int e, int k, size_t* bytes);
int grip_knn_graph(const float* queries, const float* base, int n, int m, int e, int k, int self_offset, int32_t* idx_out, float* sim_out,
                   void* workspace, size_t workspace_bytes, void* stream);
int grip_label_propagate_workspace(int n, int c, int k, size_t* bytes);
int grip_label_propagate(const float* probs, const int32_t* idx, const float* sim, float alpha, float gamma, int iters, int n, int c, int k,
                         float* out, int32_t* argmax_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 additions) Transductive GMM pseudolabelling over a pool (pseudolabels.TransductiveGMM; csrc/gmm_transduce.hip), after TransCLIP-ZS
 * (Zanella, Gerin, Ben Ayed, NeurIPS 2024): one Gaussian per class with a shared diagonal covariance on the pool's image embeddings, the assignments
 * anchored to the text head's probabilities and smoothed over the directed kNN graph of grip_knn_graph.  The recursion is the one written here, NOT
 * that paper's code: the first centres come from an M-step on the head's probabilities (no top-8 confident samples), the graph is directed, there is
 * no few-shot term.  A caller starts from Z = probs and alternates the two calls.  All tensors f32 / int32 on the device; no atomics.
 *
 * grip_gmm_mstep: z [n, c] (non-negative weights), feats [n, e] (unit rows are the CALLER's duty: the kernels take them as given)
 *   count_out[c]   = sum_i z_ic
 *   mean_out[c, :] = (sum_i z_ic feats_i) / count_out[c]; the zero vector where count_out[c] is exactly 0
 *   var_out[d]     = max(var_floor, (1 / n) sum_i sum_c z_ic (feats_id - mean_out[c, d])^2)        (the direct two-pass form)
 *   The rows are reduced over a FIXED partition (chunks of 256 rows for the sums, of 32 for the variance) and the partials added in an order that n
 *   alone fixes (contiguous slices of the chunks, each in ascending order, then the slices in ascending order): the result is bit-identical from call
 *   to call and does not depend on how many workgroups ran at once.  The sums run on the f32 MFMA.
 *   e a multiple of 4 up to 2048, any c >= 1, n >= 1, var_floor > 0; feats and mean_out 16-byte aligned; no output may alias z or feats.
 *
 * grip_gmm_estep: feats [n, e], mean [c, e], var [e], probs [n, c], (idx, sim) [n, k] the directed graph (idx values in [0, n) are the caller's duty),
 *   z_in [n, c] the current assignments:
 *   G_ic = feats_i . (mean_c / var) - 1/2 sum_d mean_cd^2 / var_d      (the class-independent terms of the log-density cancel in the softmax)
 *   then z_iters Jacobi sweeps   A_ic = G_ic + lam log(max(probs_ic, 2^-126)) + sum_j max(0, sim_ij) Z_{idx_ij, c},   Z_i <- softmax_c(A_i)
 *   (the maximum is subtracted first, the neighbours are added in list order, every sweep reads the previous sweep's Z: ping-pong between z_out and
 *   the workspace, never in place).  z_out [n, c]: the last sweep's Z; argmax_out [n] int32 or NULL: the first index of the maximum of z_out's row.
 *   G is computed once per call on the f32 MFMA (each score one chain over e in ascending order: bit-equal classes score bit-equally) and kept in
 *   the workspace.  lam >= 0, z_iters >= 1, 1 <= k <= 32, e a multiple of 4 up to 2048, any c >= 1, n >= 1; feats, mean and var 16-byte aligned;
 *   z_out must not alias z_in or probs.
 * Both calls refuse out-of-range arguments with nothing written; the workspace calls need no device. */
int grip_gmm_mstep_workspace(int n, int c, int e, size_t* bytes);
int grip_gmm_mstep(const float* z, const float* feats, int n, int c, int e, float var_floor, float* count_out, float* mean_out, float* var_out,
                   void* workspace, size_t workspace_bytes, void* stream);
int grip_gmm_estep_workspace(int n, int c, int e, int k, size_t* bytes);
int grip_gmm_estep(const float* feats, const float* mean, const float* var, const float* probs, const int32_t* idx, const float* sim, const float* z_in,
                   float lam, int z_iters, int n, int c, int e, int k, float* z_out, int32_t* argmax_out, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 additions) Gaussian discriminant head (models/gda_models.py GdaHeadModel; csrc/gda_head.hip), after "A Hard-to-Beat Baseline for
 * Training-free CLIP-based Adaptation" (Wang et al., ICLR 2024): class means and ONE shared full covariance of the unit image embeddings give the
 * linear classifier  w_c = A^-1 mu_c,  bias_c = 1/2 mu_c . w_c - log pi_c,  A = S / W + rho (tr(S) / (W e)) I,  added to the CLIP logits.  The model is
 * the one written here, NOT that paper's code: a ridge replaces its empirical-Bayes covariance estimate, rows may carry weights, the prior is the
 * caller's, a class without rows contributes nothing.  All tensors f32 / int32 on the device; no atomics; no library math.
 *
 * grip_class_scatter: scatter_out [e, e] = S = sum_i r_i (feats_i - mean[y_i]) (feats_i - mean[y_i])^T   (the direct form; r = row_weight, NULL = 1)
 *   feats [n, e], labels [n] int32, mean [c, e] (grip_gmm_mstep's, on Z_ic = r_i [y_i = c]).  A row whose label is outside 0 .. c - 1 or whose weight is 0
 *   contributes nothing and its feature row is not read.  d = fl(feats - mean) is rounded once in the load path and the products r d_a d_b run on
 *   the f32 MFMA.  The rows are reduced over a FIXED partition (chunks of 256 rows, grouped into at most 16 contiguous slices of
 *   ceil(chunks / 16) chunks; a slice is one chain over its rows in ascending order, the slices are added in ascending order): the summation order
 *   is a function of (n, e) alone, two calls are bit-equal, and the workspace is at most 16 e^2 floats whatever n is.  Only the lower triangle is
 *   computed and then mirrored: scatter_out is bit-symmetric.  e a multiple of 4 up to 1024, n, c >= 1; feats and mean 16-byte aligned;
 *   scatter_out must not alias an input.
 *
 * grip_spd_solve: M = a_scale a + ridge_rel a_scale (tr(a) / e) I,  M = L L^T,  M x_c = rhs_c for the c rows of rhs.
 *   a [e, e] is read as symmetric from its LOWER triangle only (the upper one may hold anything); rhs, x_out [c, e]; factor_out [e, e] or NULL: L, zeros
 *   above the diagonal; info_out: one device int32.  The trace is added in a fixed order on the device; M_ii = fmaf(a_scale, a_ii, shift) with
 *   shift = ((ridge_rel a_scale) tr) / e, M_ij = a_scale a_ij.  Blocked right-looking Cholesky in f32 (panels of 64 columns, the last one ragged, one
 *   launch per panel, no workgroup ever waits for another), the right-hand sides riding along as extra rows, then one back substitution per class;
 *   true divisions and square roots.  info_out = 0, or j + 1 for the first pivot j that is not > 0: x_out and factor_out are then unspecified, but the
 *   call returns and reads nothing out of bounds.  Bit-identical from call to call.  e a multiple of 4 up to 1024, c >= 1, a_scale > 0,
 *   ridge_rel >= 0; x_out may be rhs; x_out must not alias a, factor_out no other operand.
 *
 * grip_linear_head: logits_out[i, c] = base_logits[i, c] + alpha ((img_emb_i . w_c) rn_i - bias_c),   rn_i = 1 / sqrt(sum_d img_emb_id^2)
 *   img_emb [n, e] NOT normalised (as grip_cache_head_forward takes them, and with its rule: the reciprocal norm scales the SCORE, img_emb is never
 *   copied; a zero row has rn = inf and 0 * inf = NaN in every column -- rows of non-zero norm are the caller's duty); w [c, e], bias [c];
 *   base_logits [n, c] or NULL (0); logits_out may BE base_logits (in place).  argmax_out [n] int32 or NULL: the first index of the row's maximum
 *   (0 for a row of NaNs).  One launch on the f32 MFMA: a score is one chain over e in ascending order, the row's sum of squares is accumulated on
 *   chip in a fixed order, the [n, c] product never reaches memory on its own.  A row's bits depend on that row, w and bias alone -- not on n, on
 *   its place in a tile or on the call -- and bit-equal classes score bit-equally.  e a multiple of 4 up to 1024, n, c >= 1, alpha finite; img_emb
 *   and w 16-byte aligned.
 * Every call refuses out-of-range arguments with nothing written; the workspace calls need no device. */
int grip_class_scatter_workspace(int n, int c, int e, size_t* bytes);
int grip_class_scatter(const float* feats, const int32_t* labels, const float* row_weight, const float* mean, int n, int c, int e, float* scatter_out,
                       void* workspace, size_t workspace_bytes, void* stream);
int grip_spd_solve_workspace(int e, int c, size_t* bytes);
int grip_spd_solve(const float* a, float a_scale, float ridge_rel, const float* rhs, int e, int c, float* x_out, float* factor_out, int32_t* info_out,
                   void* workspace, size_t workspace_bytes, void* stream);
int grip_linear_head_workspace(int n, int c, int e, size_t* bytes);
int grip_linear_head(const float* img_emb, const float* w, const float* bias, float alpha, const float* base_logits, int n, int c, int e,
                     float* logits_out, int32_t* argmax_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 additions) Trained linear probe (models/probe_models.py LinearProbeModel; csrc/linear_probe.hip): the linear classifier on frozen features
 * that the CLIP and CoOp papers compare against, in the text-initialised form of LP++ -- a residual on the CLIP logits that starts at zero.  The model is
 * the one written here, NOT those papers' code.  All tensors f32 / int32 on the device; no atomics; every sum in a fixed order.
 *   x_ic   = base_ic + scale (feats_i . w_c) + b_c                 feats [n, e] taken as given (unit rows are the caller's duty), base [n, c] or NULL (0)
 *   t_i    = onehot(labels_i) for 0 <= labels_i < c;  soft_i (non-negative, [n, c]) for labels_i == -1 when soft is given
 *   T_i    = sum_c t_ic (ascending c)
 *   loss   = norm sum_i r_i (T_i lse(x_i) - t_i . x_i)             r = row_weight, NULL = 1; norm = 1 / sum_i r_i is the CALLER's
 *   g_ic   = r_i (T_i softmax(x_i)_c - t_ic),   grad_w = norm scale sum_i g_ic feats_i,   grad_b = norm sum_i g_ic
 * A row whose label is neither in 0 .. c - 1 nor a usable -1, or whose weight is exactly 0, contributes nothing and its feature, base and soft rows are
 * not read.  These are the DATA terms only: the ridge (l2 / 2) |w|^2 enters in grip_probe_fit's update.
 *
 * grip_probe_objective: loss_out [1], grad_w [c, e], grad_b [c] at (w [c, e], b [c] or NULL = zeros).  Three launches:
 *   1. scores on the f32 MFMA (a score is one chain over e in ascending order), x = base + fmaf(scale, score, b), the row maximum, sum of
 *      exp(x - max) and lse = max + logf(sum) on chip -- neither x nor softmax(x) is ever written to memory -- then g = r fmaf(T, exp(x - max) / sum, -t)
 *      written ONCE to the workspace, and r fmaf(T, lse, -t . x) added over the 32 rows of a workgroup in ascending order;
 *   2. the transposed contraction sum_i g_ic feats_id on the f32 MFMA over a FIXED row partition: chunks of 64 rows grouped into at most
 *      cap = min(64, max(4, 1024 / (ceil(c / 128) ceil(e / 64)))) contiguous slices of ceil(chunks / cap) chunks; a slice is one chain over its rows in
 *      ascending order (grad_b: the rows = fgrp mod 4 of a slice in four chains, then (l0 + l1) + (l2 + l3));
 *   3. the slices in ascending order, then ONE product: grad_w = fl(norm scale) sum, grad_b = norm sum, loss = norm sum (the workgroups' losses as 256
 *      strided sums, then those in ascending order).
 *   The order is a function of (n, c, e) alone: two calls are bit-equal whatever ran beside them, and bit-equal classes (w_c, b_c, base column, targets)
 *   get bit-equal grad_w rows and grad_b entries.  c <= 256 reads feats once for the scores (and once for the contraction); above that the row tile
 *   is staged again for every 64 classes.
 *
 * grip_probe_fit: `iters` iterations of launches 1 and 2 and the update (3 launches each, no host synchronisation, no allocation, capturable in a
 *   graph) -- full-batch heavy-ball descent with torch.optim.SGD(momentum) semantics, per element and in exactly this rounding sequence:
 *       gw = fl(norm scale) sum_slices         G = fmaf(l2, w, gw)         mom_w = fmaf(momentum, mom_w, G)        w = fmaf(-lr, mom_w, w)
 *       gb = norm sum_slices                                               mom_b = fmaf(momentum, mom_b, gb)       b = fmaf(-lr, mom_b, b)
 *   (three fused multiply-adds for w, two for b; the only plain products are norm scale and its product with the sum).  w, b, mom_w, mom_b are in/out
 *   and the caller's: fit(k1) followed by fit(k2) is bit-equal to fit(k1 + k2).  loss_trace [iters] or NULL: the data term at the START of each iteration.
 *
 * Limits: n >= 1, 1 <= c <= 1024, e a multiple of 4 up to 1024; feats and w 16-byte aligned; scale, norm, lr finite and > 0, l2 >= 0 finite,
 * 0 <= momentum < 1, iters >= 1; no output may alias an input or another output.  The workspace holds g [n, c], the slice partials and the workgroups'
 * losses.  Every call refuses out-of-range arguments with nothing written; the workspace calls need no device. */
int grip_probe_objective_workspace(int n, int c, int e, size_t* bytes);
int grip_probe_objective(const float* feats, const float* w, const float* b, const float* base, const int32_t* labels, const float* soft,
                         const float* row_weight, float scale, float norm, int n, int c, int e, float* loss_out, float* grad_w, float* grad_b,
                         void* workspace, size_t workspace_bytes, void* stream);
int grip_probe_fit_workspace(int n, int c, int e, size_t* bytes);
int grip_probe_fit(const float* feats, const float* base, const int32_t* labels, const float* soft, const float* row_weight, float scale, float norm,
                   float l2, float lr, float momentum, int iters, int n, int c, int e, float* w, float* b, float* mom_w, float* mom_b, float* loss_trace,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 additions) Balanced pseudolabel assignment over a pool (pseudolabels.BalancedAssignment; csrc/sinkhorn.hip): the [n, c] probabilities are
 * treated as an optimal-transport problem -- rows sum to one, columns to n x a class prior -- and Sinkhorn-Knopp iterated on it (Cuturi 2013; SeLa,
 * Asano et al. 2020; SwAV, Caron et al. 2020).  The row scaling is the softmax normaliser, so the only state between iterations is b [c]:
 *   L_ic = tau log max(probs_ic, 2^-126)
 *   b = log_scale_in (NULL: zeros);  `iters` times:   q_i = softmax_c(L_i + b),   s_c = sum_i q_ic,   b_c += log_target_c + log n - log max(s_c, 2^-126)
 *   q_out_i = softmax_c(L_i + b),  pred_i = the first index of the maximum of q_out's row,  mass_c = sum_i q_out_ic,  log_scale_out = b
 * (the row's maximum is subtracted first; L + b is one fused multiply-add).  Rows of q_out sum to one by construction; mass shows how far the columns
 * still are from n exp(log_target).  There is NO epsilon-scaled cost and NO stopping rule: `iters` is how hard the balance is pressed, and iters = 0 is
 * one bare softmax step under the given log_scale_in.  A column of probs that is zero in every row is legal: its b_c rises until the class has its share,
 * filled with arbitrary rows.
 *   probs, q_out [n, c]; log_target, log_scale_in, mass, log_scale_out [c] (log_target: the log of a prior that sums to one is the CALLER's duty);
 *   pred [n] int32 or NULL.  tau > 0 and finite, iters >= 0, any n >= 1, any c >= 1.  q_out must not alias probs; log_scale_in may be log_scale_out.
 *   The column sums run over a FIXED partition of the rows (chunks of 16, the rows of a chunk in ascending order) and the chunk partials are added in
 *   an order that n alone fixes (64 contiguous slices of the chunks, each ascending, then the slices ascending): no atomics, bit-identical from call to
 *   call.  With iters = 0 the bits of a row of q_out depend on that row and log_scale_in only -- not on n, not on the row's place.
 *   One call enqueues 2 (iters + 1) launches; the workspace (grip_sinkhorn_workspace bytes) holds the chunk partials.  The workspace call needs no
 *   device.  Out-of-range arguments are refused with nothing written. */
int grip_sinkhorn_workspace(int n, int c, size_t* bytes);
int grip_sinkhorn_balance(const float* probs, const float* log_target, const float* log_scale_in, float tau, int iters, int n, int c, float* q_out,
                          int32_t* pred, float* mass, float* log_scale_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weighted cross-entropy against soft targets gathered from a pool's assignment matrix (ABI 9 addition; csrc/soft_ce.hip): grip_weighted_ce for
 * prompt steps that train on the row of Z (label propagation, transductive GMM) or Q (Sinkhorn balance) behind a pseudolabel instead of its arg-max.
 *   logits [n, c], labels [n] int32, row_weight [n]: as grip_weighted_ce.
 *   soft [soft_rows, cz] f32: the matrix, read in place (NULL: every row is a hard row; soft_row and col_map may then be NULL).
 *   soft_row [n] int32: the matrix row of batch row i; a value < 0 or >= soft_rows marks a HARD row, whose target is onehot(labels[i]).
 *   col_map [cz] int32: the logits column of every matrix column -- distinct entries in [0, c) (the caller's contract; an entry outside [0, c) is
 *   skipped, never indexed).
 * Target of a soft row r:  L_j = inv_temperature logf(max(soft[r, j], 2^-126)),  s = softmax_j(L)  (the floor and log-domain form of
 * grip_sinkhorn_balance: soft ** inv_temperature renormalised; an all-zero matrix row is uniform over the cz mapped columns), s_j placed at column
 * col_map[j], every other column 0.  Every row:  t = (1 - smoothing) s + smoothing / c,  T = sum_c t_c,
 *   loss = sum over the rows with w_i != 0 of  w_i (T_i lse_i - sum_c t_ic x_ic),        grad_i = w_i (T_i softmax(x_i) - t_i),
 * target_out [n, c] f32 (optional) receives t.  A hard row whose label lies outside [0, c) keeps grip_weighted_ce's rule: it is left out of the loss,
 * no one-hot is subtracted (s = 0, t = smoothing / c) and the whole softmax stays, grad_i = w_i (softmax(x_i) - t_i) -- T_i is taken as 1 there; with
 * smoothing == 0 that is w_i softmax(x_i).  loss [1]; grad_logits and target_out may each be NULL.
 * With soft == NULL and smoothing == 0, loss and every gradient element are bit-equal to grip_weighted_ce on the same operands: hard rows without
 * smoothing run that kernel's arithmetic and the loss partials are added in its order.  No atomics, no scratch, no workspace; two calls are bit-equal;
 * a row's gradient and target bits depend on that row, its matrix row and col_map alone (not on n, its place in the batch or the other rows).
 * Refused with nothing written: a null operand, n or c <= 0, cz outside [1, c] with soft given, inv_temperature not finite or <= 0, smoothing outside
 * [0, 1), and c > 16000 with soft given (the inverse of col_map is held in the LDS). */
int grip_soft_ce(const float* logits, const int32_t* labels, const float* row_weight, int n, int c, const float* soft, int64_t soft_rows, int cz,
                 const int32_t* soft_row, const int32_t* col_map, float inv_temperature, float smoothing, float* loss, float* grad_logits,
                 float* target_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 additions) Candidate pseudolabel SETS over a pool and the partial-label loss on them (pseudolabels.CandidateSelection; csrc/candidate.hip;
 * Candidate Pseudolabel Learning, Zhang, Wei, Liu, Feng, ICML 2024): every image keeps a set of classes instead of one label.
 *   probs [n, c] f32: finite and >= 0 is the CALLER's duty (non-negative floats order as their bit patterns, which the selection relies on).
 *   claim in [1, n]: the rows every class claims.  tau in (0, 1].  combine: 0 intersection, 1 union, 2 intra only, 3 inter only.
 *   threshold [c] f32 = the claim-th largest value of column c, EXACT (a radix select over the bit patterns, four passes of 8 bits; the digit counts are
 *   integers, so no order of accumulation can change a bit).
 *   INTER set of row i: { c : probs[i, c] >= threshold[c] } -- ties at the threshold are all in.
 *   INTRA set of row i: rank the classes by probability descending, index ascending; s_0 = p_(0), s_j = s_{j-1} + p_(j) (plain f32 additions in rank
 *   order, no fused multiply-add, no reassociation); rank 0 is always in, rank j >= 1 is in iff s_{j-1} < tau.
 *   mask [n, words] int32, words = ceil(c / 32): class j is bit j % 32 of word j / 32; the bits at or above c are 0.
 *   count [n] int32 = the set's size; label [n] int32 = its member of highest rank, -1 for an empty set.
 *   threshold, count and label may each be NULL.  Any n >= 1, any c >= 1 (up to 256 classes a row is held in registers, beyond it is re-read).
 * Two calls are bit-equal.  Given threshold, a row's mask, count and label depend on that row alone -- not on n, not on its place.  No scratch.  One call
 * enqueues 10 launches whatever (n, c); the workspace (grip_candidate_select_workspace bytes: the digit histograms, c KiB) is overwritten; the workspace
 * call needs no device.  Out-of-range arguments (n, c, claim, tau, combine, a null probs / mask / workspace, a small workspace) are refused with nothing
 * written.
 *
 * grip_candidate_ce: grip_weighted_ce for batches whose rows may carry a candidate set (one workgroup, a wave per row, no atomics, no scratch, no
 * workspace).
 *   logits [n, c], labels [n] int32, row_weight [n]: as grip_weighted_ce.
 *   cand [cand_rows, ceil(cz / 32)] int32: the mask matrix of grip_candidate_select over cz classes, read in place (NULL: every row is a hard row;
 *   cand_row and col_map may then be NULL).
 *   cand_row [n] int32: the mask row of batch row i; a value outside [0, cand_rows) marks a HARD row (its label is the target).
 *   col_map [cz] int32: the logits column of every mask column, as grip_soft_ce: distinct entries in [0, c) are the caller's contract, an entry outside
 *   [0, c) is skipped, never indexed.
 * A candidate row with mapped set S = { col_map[j] : bit j set, col_map[j] in [0, c) }:
 *   loss_i = w_i (lse(x_i) - lse_{k in S}(x_ik)),        grad_i = w_i (softmax(x_i) - softmax_S(x_i)),  softmax_S zero outside S
 * (lse_S = max_S + logf(sum_S expf(x - max_S)); its label is not read).  A candidate row whose mapped set is EMPTY contributes nothing: no loss, a zero
 * gradient row.  Hard rows run grip_weighted_ce's statements and the loss partials are added in its order: with cand == NULL the loss and every gradient
 * element are grip_weighted_ce's bits.  A candidate row whose set is the single class y gives the bits of a hard row with label y.  loss [1]; grad_logits
 * may be NULL.  Two calls are bit-equal; a row's bits depend on that row, its mask row and col_map alone.
 * Refused with nothing written: a null operand, n or c <= 0, cz outside [1, c] with cand given, and c > 16000 with cand given (the inverse of col_map
 * is held in the LDS). */
int grip_candidate_select_workspace(int n, int c, size_t* bytes);
int grip_candidate_select(const float* probs, int n, int c, int claim, float tau, int combine, float* threshold, int32_t* mask, int32_t* count,
                          int32_t* label, void* workspace, size_t workspace_bytes, void* stream);
int grip_candidate_ce(const float* logits, const int32_t* labels, const float* row_weight, int n, int c, const int32_t* cand, int64_t cand_rows, int cz,
                      const int32_t* cand_row, const int32_t* col_map, float* loss, float* grad_logits, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 additions) Multi-view mode of an image's view embeddings (pseudolabels.MultiView; csrc/view_mode.hip).  After MTA (Zanella & Ben Ayed, "On the
 * test-time zero-shot generalization of vision-language models: Do we really need prompt learning?", CVPR 2024): training-free, a robust mean-shift over
 * the V views of an image with per-view inlier weights.  What follows is THE MODEL OF THIS HEADER, NOT THE PAPER'S CODE (no gradient steps on y, no
 * stopping rule, fixed counts, the bandwidth rule below).
 * Image i has V view embeddings f_p [e] and, optionally, the views' class probabilities s_p [c]; view 0 is the un-augmented image.
 *   1. u_p = f_p / |f_p|,  G = U U^T,  d2_pq = max(0, 2 - 2 G_pq).
 *   2. r = max(1, floor(rho (V - 1))) (the product in double on the f32 rho); h2_p = the mean of the r smallest d2_pq over q != p, added in ascending
 *      (value, index) order in plain f32 and divided by r; then h2_p = max(h2_p, h2_floor).
 *   3. A = S S^T [V, V], diagonal included (view_probs == NULL: the affinity term is off).
 *   4. m = mode_in (NULL: u_0),  y = y_in (NULL: 1 / V).
 *   5. `outer` times:
 *        k_p = exp(-sum_d (u_pd - m_d)^2 / (2 h2_p))                               (the direct form, not the expanded one)
 *        `inner` times:  y = softmax_p((k_p + lam sum_q A_pq y_q) / lam_y)         (q ascending; the maximum is subtracted first)
 *        m_d = sum_p y_p k_p u_pd / max(sum_p y_p k_p, 2^-126)                      (p ascending)
 *   6. mode_out = m (NOT normalised: the heads normalise their input), y_out = y, h2_out = h2 (may be NULL).  outer = 0: the start state and h2.
 *   view_emb [n, v, e], view_probs [n, v, c] or NULL, mode_in / mode_out [n, e], y_in / y_out / h2_out [n, v]; all f32, element offsets 64-bit.
 *   2 <= v <= 64; e a multiple of 64 up to 1 024; any c >= 1, any n >= 1; 0 < rho <= 1; lam >= 0, lam_y > 0, h2_floor > 0, all finite; outer, inner >= 0.
 *   view_emb, mode_in and mode_out 16-byte aligned.  mode_in may BE mode_out and y_in may BE y_out; no other aliasing.  A view of zero norm, or a norm
 *   whose square leaves the f32 range, is the caller's duty.
 * ONE launch per call (one workgroup per image; both [V, V] products on the f32-input MFMA, exact f32; V padded to 16-row tiles with zero rows that take
 * no part in the selection, the softmax or the sums), no atomics, no scratch, every reduction in a fixed order: two calls are bit-equal, and an image's
 * output bits depend on its own operands only -- not on n, not on its place in the launch.  The kernel keeps its state in the LDS: the workspace is
 * 0 bytes today (grip_view_mode_workspace says so; `workspace` may then be NULL) and the call needs no device.  Out-of-range arguments are refused with
 * nothing written.  This kernel is not where a multi-view pass spends its time: the V tower forwards per image are. */
int grip_view_mode_workspace(int n, int v, int c, int e, size_t* bytes);
int grip_view_mode(const float* view_emb, const float* view_probs, int n, int v, int c, int e, float rho, float lam, float lam_y, float h2_floor, int outer,
                   int inner, const float* mode_in, const float* y_in, float* mode_out, float* y_out, float* h2_out, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 additions) Marginal entropy of an image's confident views, and its gradient: the loss of a test-time prompt-tuning episode (tpt.TestTimeTuner;
 * csrc/view_entropy.hip).  After TPT (Shu et al., "Test-time prompt tuning for zero-shot generalization in vision-language models", NeurIPS 2022).  What
 * follows is THE MODEL OF THIS HEADER, NOT THE PAPER'S CODE.
 * Image i has V views; x[p, :] are the logits of view p over c classes (logits [n v, c], image-major: the rows pseudolabels.MultiView.aggregate hands to
 * the cosine head).
 *   per view:   lse_p = max + logf(sum_c expf(x_pc - max)),   p_pc = expf(x_pc - lse_p),   H_p = -sum_c p_pc (x_pc - lse_p)   (every term >= 0; lane l of a
 *               wave adds the classes l, l + 64, ... in ascending order, then the wave's fixed tree)
 *   selection:  the `keep` views of smallest H_p; ties go to the lower view index; a view whose H_p is not finite ranks after every finite one, index
 *               ascending.  The selection is a CONSTANT of the gradient.
 *   marginal:   pbar_c = (sum_{p selected, ascending} p_pc) / keep
 *   loss:       loss_i = -sum_c pbar_c logf(max(pbar_c, 2^-126))      (the floor of the Sinkhorn / soft-CE kernels)
 *               loss = (1 / n) sum_i loss_i, added in ascending i and multiplied by 1.0f / (float)n
 *   gradient:   g_c = -(logf(max(pbar_c, 2^-126)) + 1) / keep;  a selected view gets grad x_pj = (p_pj (g_j - sum_c p_pc g_c)) * (1.0f / (float)n), every
 *               other view exactly +0.0 in every element.  Every element of grad_logits has one writer.
 *   logits [n v, c]; loss [1]; grad_logits [n v, c], view_entropy_out [n, v] (H), selected_out [n, v] int32 (0 / 1) and mean_probs_out [n, c] (pbar) may
 *   each be NULL.  All f32 / int32, element offsets 64-bit.  1 <= v <= 64, 1 <= keep <= v, 1 <= c <= 16000 (g lives in the LDS: the limit and the reason
 *   of grip_candidate_ce), any n >= 1.  No output may alias logits or another output.  Logits that are not finite are the caller's duty.
 * ONE launch for the per-image work (one workgroup per image, a wave per view, views beyond the wave count round-robin), no atomics, no scratch, no
 * workspace.  n > 1 adds one single-workgroup launch for the mean over images: it re-adds the per-image loss terms from mean_probs_out in the image's own
 * order (the same bits), or, when mean_probs_out is NULL, walks the images once more with every output off -- pass mean_probs_out when n is large.  Two
 * calls are bit-equal.  H, selected, pbar and loss_i of an image depend on its [v, c] block and keep alone -- not on n, not on its place in the launch;
 * n enters its gradient last, as the one multiplication above.  Refused with nothing written: a null logits / loss, n or c <= 0, v or keep out of range,
 * c > 16000, an output that overlaps logits or another output. */
int grip_view_entropy(const float* logits, int n, int v, int c, int keep, float* loss, float* grad_logits, float* view_entropy_out, int32_t* selected_out,
                      float* mean_probs_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 additions) Test-time streaming cache over the items of one `predict` call (tda.StreamCache; csrc/stream_cache.hip).  After TDA (Karmanov et al.,
 * "Efficient test-time adaptation of vision-language models", the training-free dynamic adapter, CVPR 2024): no tower pass, no backward, any modality.
 * What follows is THE MODEL OF THIS HEADER, NOT THE PAPER'S CODE (one queue rule for both polarities, the stream is the whole call in dataset order,
 * nothing survives the call).
 * base_logits [n, c] (whatever the heads produced) and img_emb [n, e] (NOT normalised: 1 / |f| = 1.0f / sqrtf(sum f^2) multiplies the score, the rule of
 * grip_cache_head_forward), both in stream order.
 *   per item:   lse_i = max + logf(sum_c expf(x_ic - max)),  p_ic = expf(x_ic - lse_i),  H_i = -sum_c p_ic (x_ic - lse_i)   (grip_view_entropy's statements:
 *               lane l of a wave adds the classes l, l + 64, ... ascending, then the wave's fixed tree);  pred_i = the FIRST arg-max of x_i (a row in which
 *               nothing compares greater than -inf, e.g. a row of NaNs: 0);  Hn_i = H_i / L in f32 with L = (float)log((double)c), and 0 for c = 1;
 *               negbits_i: bit (y mod 32) of word y / 32 is set iff mask_lo < p_iy < mask_hi  ([n, ceil(c / 32)] int32 holding the 32 bits, the layout of
 *               grip_candidate_select's mask; bits >= c are zero).
 *   queues:     every class has a positive queue of capacity pos_cap and a negative one of capacity neg_cap (0: no negative queue); item i goes to the
 *               queues of class pred_i.  The negative queue admits only items with ent_lo < Hn_i < ent_hi.  A queue that is not full takes the item.  A
 *               full queue takes it only if H_i is STRICTLY smaller than H of the resident with the largest (H, index); that resident leaves.  The
 *               comparisons are on the f32 H written to entropy_out.  A non-finite H_i is never admitted.
 *   score:      item i is scored AFTER its own admission, against the residents of that moment:
 *                 out[i, y] = base[i, y] + pos_alpha Spos - neg_alpha Sneg,
 *                 Spos = sum_{j in Pos_i, pred_j = y} a(i, j; pos_beta),   Sneg = sum_{j in Neg_i, bit y of negbits_j} a(i, j; neg_beta),
 *                 a(i, j; beta) = expf(-(beta (1 - s_ij))),  s_ij = ((f_i . f_j) (1 / |f_i|)) (1 / |f_j|), the dot product one f32 MFMA chain over e.
 *               Each sum is one f32 chain over its live keys in ascending j starting from 0; the positive term is added first, each as a rounded product
 *               and a rounded sum.  A sum that is 0 (no live key, or every term underflowed) leaves the element alone: such a column is base, bit for bit.
 * The queue updates depend on the base logits alone, so the stream is evaluated in two calls, and the result is the sequential algorithm's item for item:
 * grip_stream_cache_plan (three launches: a wave per row; a wave per (class, polarity) that walks pred in order -- no atomic, no cross-workgroup wait; a
 * deterministic compaction) writes
 *   entropy_out [n] f32 (H), pred_out [n] int32, negbits_out [n, ceil(c / 32)] int32,
 *   pos_leave / neg_leave [n] int32: item j sat in the queue during the stream positions [j, leave_j): leave_j = j means never admitted, INT32_MAX still
 *   resident at the end, else the index of the item that evicted it,
 *   pos_key / neg_key [n] int32: the ever-admitted items, ascending (the first counts_out[0] / counts_out[1] entries; the rest is not written),
 *   counts_out [2] int32 on the device.
 * grip_stream_cache_head (a memset and three launches) is the f32-MFMA main loop of the cache head with the key rows gathered from img_emb through the
 * key lists (no key copy); item i sums exactly the keys j with j <= i < leave_j, tested in the epilogue; the [n, m] affinities are never written; one
 * writer per element, no atomics.  A row tile stops at the last key tile that holds a key j <= its last row.  It reads the two counts ON THE DEVICE: no
 * launch geometry depends on them and a stream costs no host read.  negbits, neg_leave and neg_key all NULL: no negative term.  out must not overlap an input.
 * The workspace holds the reciprocal norms and the two [n, c] sums (grip_stream_cache_head_workspace; the plan's is 0 bytes today and may be NULL).
 * Two calls are bit-equal.  CAUSALITY: rows 0 .. k-1 of every output of a run on the first k items are bit-equal to rows 0 .. k-1 of the run on all n,
 * but for leave (an item still resident after k items may leave later).  e a multiple of 4 up to 1 024, img_emb 16-byte aligned; any c >= 1,
 * 1 <= n <= 2^30; pos_cap 1 .. 16, neg_cap 0 .. 16; the windows finite with lo <= hi; alpha and beta finite.  The worst case m = n (entropies strictly
 * descending within one class) is served.  Out-of-range arguments are refused with nothing written; the _workspace calls need no device. */
int grip_stream_cache_plan_workspace(int n, int c, size_t* bytes);
int grip_stream_cache_plan(const float* base_logits, int n, int c, int pos_cap, int neg_cap, float ent_lo, float ent_hi, float mask_lo, float mask_hi,
                           float* entropy_out, int32_t* pred_out, int32_t* pos_leave, int32_t* neg_leave, int32_t* negbits_out, int32_t* pos_key,
                           int32_t* neg_key, int32_t* counts_out, void* workspace, size_t workspace_bytes, void* stream);
int grip_stream_cache_head_workspace(int n, int c, int e, size_t* bytes);
int grip_stream_cache_head(const float* base_logits, const float* img_emb, const int32_t* pred, const int32_t* negbits, const int32_t* pos_leave,
                           const int32_t* neg_leave, const int32_t* pos_key, const int32_t* neg_key, const int32_t* counts, float pos_alpha, float pos_beta,
                           float neg_alpha, float neg_beta, int n, int c, int e, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * CLIP preprocessing of one decoded image: the `_transform` the reference applies per item on the host
 * (data/dataset.py:64-79 via clip.load's preprocess): Resize(n_px, BICUBIC) -> CenterCrop(n_px) -> ToTensor -> Normalize.
 * Bit-exact with Pillow's 8-bit bicubic resample; only the cropped rows / columns are produced.
 *   img [H, W, 3] u8 device; out [3, n_px, n_px] f32 device; tmp [H * n_px * 3] u8 device scratch
 *   hcoef [W_out, hksize] / hbounds [W_out, 2] and vcoef [H_out, vksize] / vbounds [H_out, 2]: int32 device tables of
 *   Pillow's precompute_coeffs + normalize_coeffs_8bpc (22-bit fixed point; bounds = first input index, count);
 *   hksize = vksize = 0 (tables NULL): the image already has the resized size, crop + normalise only.
 *   mean3 / std3: HOST pointers to 3 floats. */
int grip_preprocess_image(const uint8_t* img, int H, int W,
                          const int32_t* hcoef, const int32_t* hbounds, int hksize, int W_out,
                          const int32_t* vcoef, const int32_t* vbounds, int vksize, int H_out,
                          int crop_left, int crop_top, int n_px, const float* mean3, const float* std3,
                          uint8_t* tmp, float* out, void* stream);

/* The same for a whole batch of decoded images of different sizes in ONE launch pair (the host decodes JPEGs on a thread pool and
 * uploads the batch as one packed buffer).  `items_device` is a DEVICE array of n_items descriptors; every pointer inside is a
 * device pointer; hksize = vksize = 0 marks an image that already has the resized size.  max_H = the largest H of the batch.
 * mean3 / std3: HOST pointers to 3 floats. */
typedef struct {
    const uint8_t* img;        /* [H, W, 3] u8 */
    int32_t H, W;
    const int32_t* hcoef;      /* [W_out, hksize] */
    const int32_t* hbounds;    /* [W_out, 2] */
    int32_t hksize, W_out;
    const int32_t* vcoef;      /* [H_out, vksize] */
    const int32_t* vbounds;    /* [H_out, 2] */
    int32_t vksize, H_out;
    int32_t crop_left, crop_top;
    uint8_t* tmp;              /* [H, n_px, 3] u8 scratch */
    float* out;                /* [3, n_px, n_px] f32 */
} grip_preprocess_item;
int grip_preprocess_batch(const grip_preprocess_item* items_device, int n_items, int max_H, int n_px,
                          const float* mean3, const float* std3, void* stream);

/* ------------------------------------------------------------------------------------------
 * (ABI 9 addition) Train-time views of the f32 pool (RandomResizedCrop + RandomHorizontalFlip; csrc/augment.hip; the `augmentations` slot of the
 * reference's datasets, data/dataset.py:18-79).  View v crops the box [top, top + height) x [left, left + width) of image `row`, resamples it to
 * n_px x n_px with Pillow's antialiased bicubic (a = -0.5: precompute_coeffs applied to the BOX, i.e. crop() followed by resize() -- taps clip at the
 * box edge and nothing outside the box is read) and, when `flip` is non-zero, mirrors the result left-right.
 *   src            [n_src, 3, H, W] f32, contiguous, device
 *   views_device   DEVICE array of n_views descriptors; 0 <= row < n_src, 1 <= height <= H - top, 1 <= width <= W - left, top, left >= 0.  The caller
 *                  validates them (grip_amd.augment.views does, on the host); a descriptor outside the pool writes nothing.
 *   out            [n_views, 3, n_px, n_px] f32 device; any n_px >= 1 (16-byte stores when n_px % 4 == 0 and out is 16-byte aligned)
 * Weights are evaluated and normalised in float64 on the device and rounded to f32 once; both passes accumulate in f32.  A box with
 * height == width == n_px and no flip is a bit-exact copy.  No allocation, no synchronisation, no atomics; a view's bits depend on its own descriptor
 * only (not on n_views, its position in the launch or the other views).  Element offsets are 64-bit. */
typedef struct {
    int64_t row;
    int32_t top, left, height, width, flip, pad;
} grip_view;
int grip_augment_views(const float* src, int64_t n_src, int H, int W, const grip_view* views_device, int64_t n_views, int n_px,
                       float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sequential per-class leaderboard: utils/clip_pseudolabels.py:49-112 and the nine
 * assign_pseudo_labels (e.g. methods/transductive_zsl/multimodal_fpl.py:194-285).  Host function,
 * exact: order-dependent, one pass in dataset order.
 *   probs [n, c] f32 host; pred [n] int32 host (arg-max the caller took: of probs in
 *   clip_pseudolabels.py:39, of logits in assign_pseudo_labels)
 *   path_rank [n] int64 host: rank of image i's path string among all paths (ties in the score are
 *   broken by the path, descending; equal strings get equal ranks)
 *   out_img / out_class: capacity c * min(k, n); *out_count = pairs emitted, boards concatenated
 *   in class order, each in its final list order.
 */
int grip_leaderboard_scan(const float* probs, const int32_t* pred, const int64_t* path_rank,
                          int64_t n, int c, int64_t k, int32_t* out_img, int32_t* out_class, int64_t* out_count);

/* The same scan over probabilities that are only known to a per-row relative accuracy (screen and refine): rows encoded by the
 * f16 towers carry rel_eps[i] > 0, rows re-encoded by an exact (precision = 1) tower carry 0.  Every order the reference's scan
 * depends on (the arg-max, utils/clip_pseudolabels.py:39; `board[-1].score < score`, :75 / :95; the sorted inserts, :79-82 /
 * :97-100) is decided on the intervals [p (1 - eps), p (1 + eps)].  ambiguous[i] is set to 1 for every row with rel_eps[i] > 0 that
 * took part in a comparison the intervals could not decide (an undecidable arg-max only counts when one of the candidate classes
 * could admit the image: when all of them certainly reject it the image spills to every class whichever of them is the true
 * arg-max).  *n_ambiguous == 0  =>  the lists written are the lists grip_leaderboard_scan returns on the TRUE probabilities,
 * provided every |true_i[j] - p_i[j]| <= rel_eps[i] * p_i[j] + abs_eps (abs_eps: absolute slack of the un-refined rows, for softmax outputs in
 * the denormal range, which have no relative accuracy; rows with rel_eps[i] == 0 are final and carry none).  A row may also carry the bound of an
 * intermediate tier (0 < rel_eps[i] << the screen's): any mix of per-row bounds is valid.  Otherwise the caller re-encodes the marked rows exactly, sets their
 * rel_eps to 0 and calls again; the marked set grows strictly, so the loop ends (host side: grip_amd.pseudolabels.refine_scan).
 *   k == 10000000 (the reference's "label everything" branch, :27-44): out_img / out_class need capacity n and every row
 *   whose arg-max is undecidable is marked.  Otherwise capacity c * min(k, n) as above.
 *   ambiguous [n] uint8 host (overwritten).
 *   bound_form (ABI 8): 0 = the RELATIVE form above.  1 = LOG-ODDS: rel_eps[i] is delta_i and the proviso reads "the ODDS p / (1 - p) of every
 *   entry of row i are within a factor e^{+-delta_i} of the true ones": the interval of an entry is [p / (p + (1 - p) e^delta),
 *   p / (p + (1 - p) e^-delta)] (with 2^-20 of slack for the f32 evaluation of p and 1 - p, and abs_eps).  It is what an error of a cheaper tower's
 *   embedding direction produces -- the LOGITS move by scale * <de, t_c> whatever the probabilities are, and the softmax
 *   (utils/clip_pseudolabels.py:38) turns a spread d of those errors over the classes into a factor within e^{+-d} on every entry's odds.  For
 *   p << 1 it is the relative form with eps = e^delta - 1; for the p ~ 0.9+ entries that sit on the board thresholds of a peaked pool it is
 *   (1 - p) times tighter.  delta < 700.
 *   threads (ABI 8): worker threads of the scan's pre-filter; 0 = $GRIP_SCAN_THREADS, else the CPUs the process may use divided by
 *   $LOCAL_WORLD_SIZE (at most 16).  The lists and marks do not depend on it. */
int grip_leaderboard_scan_bounded(const float* probs, const int32_t* pred, const int64_t* path_rank, const float* rel_eps, float abs_eps,
                                  int bound_form, int threads, int64_t n, int c, int64_t k, int32_t* out_img, int32_t* out_class,
                                  int64_t* out_count, uint8_t* ambiguous, int64_t* n_ambiguous);

/* ------------------------------------------------------------------------------------------
 * clip.tokenize's byte-level BPE (host function; the reference tokenises on every CustomTextEncoder.forward,
 * models/clip_encoders.py:60, and in utils/clip_pseudolabels.py:25).
 *   grip_bpe_create        merges = the text of the merges table, one "a b" pair per line in rank order (the lines of
 *                          bpe_simple_vocab_16e6.txt after its header, in the byte-to-unicode alphabet); ids follow openai/CLIP:
 *                          256 bytes, 256 end-of-word bytes, the merges, <|startoftext|>, <|endoftext|>
 *   grip_bpe_encode_word   one pre-token (raw UTF-8 bytes of one match of the CLIP pre-tokenisation pattern) -> ids
 *   grip_bpe_encode_ascii  a cleaned, lower-cased ASCII text: pre-tokenisation (the CLIP pattern restricted to ASCII) + BPE */
typedef struct grip_bpe grip_bpe;
int grip_bpe_create(const char* merges, size_t n_bytes, grip_bpe** out);
int grip_bpe_destroy(grip_bpe* t);
int grip_bpe_special_ids(const grip_bpe* t, int32_t* sot, int32_t* eot, int32_t* vocab_size);
int grip_bpe_encode_word(grip_bpe* t, const uint8_t* word, int n, int32_t* ids, int cap, int* n_out);
int grip_bpe_encode_ascii(grip_bpe* t, const char* text, int n, int32_t* ids, int cap, int* n_out);

/* ------------------------------------------------------------------------------------------
 * Launch width of the persistent kernels (ABI 7).  The pool-encode GEMMs and the pipelined attention size their grids to the WHOLE chip (one
 * workgroup per CU, each walking many tiles).  A host that runs an encode on a CU-masked stream (hipExtStreamCreateWithCUMask) next to other work --
 * the frozen image tower's look-ahead encode of a textual-prompt epoch beside the latency-bound prompt steps, textual_prompt.py:95-103 -- tells the
 * library how many CUs that stream owns, so that the persistent grids fit them (a 256-workgroup grid on 192 CUs would run in two rounds).
 * n_cus = 0 restores the full width.  Process-wide host state read at launch time: set it around the launches it is meant for.  Results do not
 * depend on it (tile -> workgroup assignment never changes an element's arithmetic). */
int grip_set_cu_budget(int n_cus);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU exchange (one process per GPU, RCCL over the xGMI mesh).  The unlabeled pool shards contiguously over the
 * ranks and the per-rank embeddings are all-gathered once per pass; this replaces the accelerator.gather
 * sites of the reference (e.g. methods/semi_supervised_learning/textual_prompt.py:146-147, 285-286) and, for the trainable
 * prompts, DDP's gradient all-reduce behind accelerator.backward (textual_prompt.py:131).
 *   grip_comm_unique_id   rank 0 fills 128 bytes (an ncclUniqueId) and hands them to the other ranks through any side
 *                         channel (torch.distributed store, a file, MPI)
 *   grip_comm_init_rank   collective over the n_ranks processes; the calling thread's current HIP device is the rank's GPU
 *   grip_allgather_embeddings   local [rows_per_rank, e] f32 device -> global [n_ranks * rows_per_rank, e] f32 device, rank-major
 *                         (the caller pads the last shard to rows_per_rank rows and drops the padding afterwards)
 *   grip_allreduce_mean   in place: every rank ends with the mean over ranks of grads[0..n)
 * Both collectives are enqueued on `stream`.  RCCL is loaded at run time ($GRIP_RCCL_LIBRARY, else librccl.so). */
typedef struct grip_comm grip_comm;
int grip_comm_unique_id(uint8_t* id128);
int grip_comm_init_rank(const uint8_t* id128, int n_ranks, int rank, grip_comm** out);
int grip_comm_destroy(grip_comm* comm);
int grip_allgather_embeddings(grip_comm* comm, const float* local, float* global, int64_t rows_per_rank, int e, void* stream);
int grip_allreduce_mean(grip_comm* comm, float* grads, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRIP_AMD_H */
