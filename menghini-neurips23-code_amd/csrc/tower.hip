// Tower handle, weight layout and the forward/backward launch sequences behind the C ABI
// (include/grip_amd.h).  A tower is the frozen CLIP ViT (kind 0) or text transformer (kind 1);
// the launch sequence follows CustomVisionTransformer.forward (models/clip_encoders.py:123-194)
// and CustomTextEncoder.forward (:43-90) of the reference, with the per-block arithmetic of the
// published openai/CLIP ResidualAttentionBlock: x += out_proj(MHSA(ln_1 x)); x += c_proj(QuickGELU(c_fc(ln_2 x))).
//
// HBM layout: residual stream x (resid_t = f16, accumulated in f32 inside the GEMM epilogues) [B*S, d] row-major (token-major, so every GEMM sees one
// [M, K] x [N, K]^T problem over all images of the chunk); GEMM operands (LayerNorm output, packed
// qkv [M, 3d], attention output, MLP hidden [M, 4d]) f16.  Row counts are padded to the 128-row GEMM
// tile in the workspace; padding rows are never stored to and never read back.
#include <stdarg.h>
#include <stdlib.h>

#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "../../include/grip_amd_debug.h"      // the hooks defined here are checked against their declarations

// ---------------------------------------------------------------------------------------------- errors
static thread_local char g_err[512] = "";
void grip_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* grip_last_error(void) { return g_err; }
extern "C" int grip_abi_version(void) { return GRIP_ABI_VERSION; }

static int g_cu_budget = 0;
int grip_cu_budget() { return g_cu_budget; }
extern "C" int grip_set_cu_budget(int n_cus) {
    GRIP_REQUIRE(n_cus >= 0 && (n_cus == 0 || n_cus >= 8), "set_cu_budget: %d (0 = all, else at least 8)", n_cus);
    g_cu_budget = n_cus;
    return GRIP_OK;
}

// ---------------------------------------------------------------------------------------------- layout
struct LayerW {
    // f16 (element offsets into the f16 blob)
    int64_t in_w, out_w, fc_w, proj_w;          // [3d,d] [d,d] [4d,d] [d,4d]
    int64_t in_wT, out_wT, fc_wT, proj_wT;      // derived transposes: [d,3d] [d,d] [d,4d] [4d,d]
    int64_t in_wG, fc_wG;                       // derived: LayerNorm-folded operands f16(gamma o W) of the QKV and c_fc GEMMs
    int64_t in_wS = -1, out_wS = -1, fc_wS = -1, proj_wS = -1;   // derived, precision 2 only: the four weights in the split layout of gemm_split.hip
    // f32
    int64_t ln1_g, ln1_b, in_b, out_b, ln2_g, ln2_b, fc_b, proj_b;
    int64_t in_cs, in_bb, fc_cs, fc_bb;         // derived: colsum(W') and W beta + b of the two folded GEMMs
};
struct Layout {
    std::vector<grip_slot> slots;
    std::vector<LayerW> layer;
    int64_t n16 = 0, n32 = 0;
    int kpad = 0;
    // vision
    int64_t conv_w = -1, cls = -1, pos = -1, lnpre_g = -1, lnpre_b = -1, lnpost_g = -1, lnpost_b = -1, proj = -1, projT = -1;
    // text
    int64_t tok = -1;
};

static int64_t add_slot(Layout& L, const std::string& name, int dtype, int derived, int64_t rows, int64_t cols, int64_t ld = 0) {
    grip_slot s;
    memset(&s, 0, sizeof(s));
    snprintf(s.name, sizeof(s.name), "%s", name.c_str());
    s.dtype = dtype;
    s.derived = derived;
    s.rows = rows;
    s.cols = cols;
    s.ld = ld ? ld : cols;
    int64_t& n = dtype == 0 ? L.n16 : L.n32;
    n = round_up64(n, 64);  // 128-byte (f16) / 256-byte (f32) aligned slots
    s.offset = n;
    n += rows * s.ld;
    L.slots.push_back(s);
    return s.offset;
}

static int build_layout(const grip_dims& D, Layout& L) {
    GRIP_REQUIRE(D.kind == 0 || D.kind == 1, "dims.kind must be 0 (vision) or 1 (text)");
    GRIP_REQUIRE(D.width > 0 && D.width % 128 == 0 && D.heads * 64 == D.width, "width must be a multiple of 128 with head dim 64 (width=%d heads=%d)", D.width, D.heads);
    GRIP_REQUIRE(D.embed_dim > 0 && D.embed_dim % 128 == 0, "embed_dim must be a multiple of 128");
    GRIP_REQUIRE(D.layers > 0 && D.seq0 > 0, "layers / seq0 must be positive");
    const int64_t d = D.width;
    if (D.kind == 0) {
        GRIP_REQUIRE(D.patch > 0 && D.resolution % D.patch == 0, "vision: resolution %% patch != 0");
        const int g = D.resolution / D.patch;
        GRIP_REQUIRE(D.seq0 == g * g + 1, "vision: seq0 must be grid^2 + 1");
        L.kpad = (int)round_up64(3 * D.patch * D.patch, 64);
        L.conv_w = add_slot(L, "conv1.weight", 0, 0, d, 3 * D.patch * D.patch, L.kpad);
        L.cls = add_slot(L, "class_embedding", 1, 0, 1, d);
        L.pos = add_slot(L, "positional_embedding", 1, 0, D.seq0, d);
        L.lnpre_g = add_slot(L, "ln_pre.weight", 1, 0, 1, d);
        L.lnpre_b = add_slot(L, "ln_pre.bias", 1, 0, 1, d);
    } else {
        GRIP_REQUIRE(D.vocab > 0, "text: vocab must be positive");
        L.tok = add_slot(L, "token_embedding.weight", 1, 0, D.vocab, d);
        L.pos = add_slot(L, "positional_embedding", 1, 0, D.seq0, d);
    }
    L.layer.resize((size_t)D.layers);
    for (int i = 0; i < D.layers; ++i) {
        LayerW& w = L.layer[(size_t)i];
        const std::string p = "transformer.resblocks." + std::to_string(i) + ".";
        w.ln1_g = add_slot(L, p + "ln_1.weight", 1, 0, 1, d);
        w.ln1_b = add_slot(L, p + "ln_1.bias", 1, 0, 1, d);
        w.in_w = add_slot(L, p + "attn.in_proj_weight", 0, 0, 3 * d, d);
        w.in_b = add_slot(L, p + "attn.in_proj_bias", 1, 0, 1, 3 * d);
        w.out_w = add_slot(L, p + "attn.out_proj.weight", 0, 0, d, d);
        w.out_b = add_slot(L, p + "attn.out_proj.bias", 1, 0, 1, d);
        w.ln2_g = add_slot(L, p + "ln_2.weight", 1, 0, 1, d);
        w.ln2_b = add_slot(L, p + "ln_2.bias", 1, 0, 1, d);
        w.fc_w = add_slot(L, p + "mlp.c_fc.weight", 0, 0, 4 * d, d);
        w.fc_b = add_slot(L, p + "mlp.c_fc.bias", 1, 0, 1, 4 * d);
        w.proj_w = add_slot(L, p + "mlp.c_proj.weight", 0, 0, d, 4 * d);
        w.proj_b = add_slot(L, p + "mlp.c_proj.bias", 1, 0, 1, d);
        w.in_wT = add_slot(L, p + "attn.in_proj_weight#T", 0, 1, d, 3 * d);
        w.out_wT = add_slot(L, p + "attn.out_proj.weight#T", 0, 1, d, d);
        w.fc_wT = add_slot(L, p + "mlp.c_fc.weight#T", 0, 1, d, 4 * d);
        w.proj_wT = add_slot(L, p + "mlp.c_proj.weight#T", 0, 1, 4 * d, d);
        w.in_wG = add_slot(L, p + "attn.in_proj_weight#G", 0, 1, 3 * d, d);
        w.fc_wG = add_slot(L, p + "mlp.c_fc.weight#G", 0, 1, 4 * d, d);
        w.in_cs = add_slot(L, p + "attn.in_proj#colsum", 1, 1, 1, 3 * d);
        w.in_bb = add_slot(L, p + "attn.in_proj#bias", 1, 1, 1, 3 * d);
        w.fc_cs = add_slot(L, p + "mlp.c_fc#colsum", 1, 1, 1, 4 * d);
        w.fc_bb = add_slot(L, p + "mlp.c_fc#bias", 1, 1, 1, 4 * d);
        if (D.precision == 2) {     // [N, K/32, 32 hi | 32 lo'] f16: as many bytes as the f32 matrix (the operand blob has f32 elements)
            w.in_wS = add_slot(L, p + "attn.in_proj_weight#S", 0, 1, 3 * d, d);
            w.out_wS = add_slot(L, p + "attn.out_proj.weight#S", 0, 1, d, d);
            w.fc_wS = add_slot(L, p + "mlp.c_fc.weight#S", 0, 1, 4 * d, d);
            w.proj_wS = add_slot(L, p + "mlp.c_proj.weight#S", 0, 1, d, 4 * d);
        }
    }
    const char* lnf = D.kind == 0 ? "ln_post" : "ln_final";
    L.lnpost_g = add_slot(L, std::string(lnf) + ".weight", 1, 0, 1, d);
    L.lnpost_b = add_slot(L, std::string(lnf) + ".bias", 1, 0, 1, d);
    const char* pj = D.kind == 0 ? "proj" : "text_projection";
    L.proj = add_slot(L, pj, 0, 0, d, D.embed_dim);
    L.projT = add_slot(L, std::string(pj) + "#T", 0, 1, D.embed_dim, d);
    L.n16 = round_up64(L.n16, 64);
    L.n32 = round_up64(L.n32, 64);
    return GRIP_OK;
}

extern "C" int grip_layout_slot(const grip_dims* dims, int slot, grip_slot* out) {
    GRIP_REQUIRE(dims && out, "layout_slot: null pointer");
    try {
        Layout L;
        int rc = build_layout(*dims, L);
        if (rc) return rc;
        GRIP_REQUIRE(slot >= 0 && slot < (int)L.slots.size(), "layout_slot: slot %d past the end (%d)", slot, (int)L.slots.size());
        *out = L.slots[(size_t)slot];
        return GRIP_OK;
    } catch (...) { grip_set_error("layout_slot: exception"); return GRIP_ERR_ARG; }
}

extern "C" int grip_layout_size(const grip_dims* dims, int64_t* n_f16, int64_t* n_f32) {
    GRIP_REQUIRE(dims && n_f16 && n_f32, "layout_size: null pointer");
    try {
        Layout L;
        int rc = build_layout(*dims, L);
        if (rc) return rc;
        *n_f16 = L.n16;
        *n_f32 = L.n32;
        return GRIP_OK;
    } catch (...) { grip_set_error("layout_size: exception"); return GRIP_ERR_ARG; }
}

// ---------------------------------------------------------------------------------------------- handle
// Activation buffers are declared half_t* but hold f32 elements in exact mode (element size `es` below); the forward passes
// them on as untyped pointers + the f32 flag, and the backward (f16 towers only) uses them as declared.
struct CarveRec { const char* name; int layer; size_t offset, bytes; };      // one buffer of a carve-up, as carve() handed it out (grip_debug_tower_slot)
struct Workspace {  // carve of the caller's buffer for one (batch, n_prefix, train) problem
    std::vector<CarveRec>* rec = nullptr;      // set by grip_debug_tower_slot alone: carve() notes every buffer here
    int batch = 0, P = 0, train = 0, S = 0, M = 0;
    int64_t Mp = 0;
    resid_t* x = nullptr;      // inference residual stream
    half_t* xn = nullptr;
    half_t* qkv = nullptr;
    half_t* att = nullptr;
    half_t* h = nullptr;
    half_t* cls16 = nullptr;   // [round_up(batch,128), d]
    half_t* patches = nullptr; // alias of h
    float* patch_out = nullptr;// alias of qkv
    half_t* row_x = nullptr;   // compact last-block buffers (f16 towers): [Bp, d] stream rows, [Bp, d] attention rows,
    half_t* row_att = nullptr; // [Bp, d] LayerNorm output, [Bp, 4d] MLP hidden
    half_t* row_xn = nullptr;
    half_t* row_h = nullptr;
    // ... and, when a TRAIN-mode forward runs its last block for the read rows only (rows_last): what that block saves for its backward
    // and the backward's own compact scratch
    int rows_last = 0;
    int ks_row = 1;            // split factor of the compact fc input-gradient GEMM
    half_t* row_hpre = nullptr;   // [Bp, 4d] pre-activations
    resid_t* row_xmid = nullptr;  // [Bp, d] stream rows after the attention branch
    resid_t* row_xout = nullptr;  // [Bp, d] stream rows after the block (what ln_post / ln_final reads)
    float* drow = nullptr;        // [Bp, d] f32 gradient of those stream rows
    half_t* drow_h = nullptr;     // ... its f16 copy (GEMM operand)
    half_t* row_dh = nullptr;     // [Bp, 4d]
    float* row_dln = nullptr;     // [ks_row][Bp, d]
    half_t* row_datt = nullptr;   // [Bp, d]
    float* stat_part = nullptr;// [d/64, M, 2] partial row sums emitted by the residual GEMM epilogues (f16 towers)
    float* rowstat = nullptr;  // [Mp, 2] (mean, rstd) of the residual stream's rows, consumed by the LayerNorm-folded GEMMs
    half_t* row_x_lo = nullptr;   // ... and of the last block's compact read rows
    half_t* x_lo = nullptr;    // inference, f16 towers: the lo parts of the stream when the forward runs with GRIP_FWD_STREAM_HILO (GemmArgs::resid_lo)
    int hilo = 0;              // ... and whether this forward does
    const float* deep = nullptr;   // deep visual prompts [n_deep, P, d] f32 (grip_vit_forward_deep): rows 1 .. P of block l's input := deep[l - 1], 1 <= l <= n_deep
    int n_deep = 0;
    int deep_classes = 1;          // text tower (grip_text_forward_deep): deep is [n_deep, deep_classes, P, d], one context per class when deep_classes == batch
    // train-mode saves, one per layer (x_in has layers+1 entries)
    std::vector<resid_t*> x_in, x_mid;
    std::vector<half_t*> qkv_l, att_l, hpre_l;
    // backward scratch
    float* dx = nullptr;
    float* dln = nullptr;      // [max(ks_fc, ks_in)][Mp, d] f32 split-K partials of the EPI_F32 input-gradient GEMMs
    int ks_fc = 1, ks_in = 1;  // their split factors (gemm_pick_ksplit)
    // shared-prefix layout of the text tower (common.h, seq_row): Ps = 1 + P shared leading rows, then S - Ps rows per class
    int Ps = 0;
    int rs = 0;                // rows between consecutive sequences for the (sequence, position) -> row gathers: S, or S - Ps
    float* kv_part = nullptr;  // [batch, Ps, 2, d] f32: per-class shares of the shared keys' dK / dV (train)
    // cooperative split-K of the train-mode c_proj GEMM (text tower; GemmArgs::coop_scratch): factor, partial tiles, (tile, wave) tickets
    int coop_ks = 1;
    float* coop_scratch = nullptr;
    int* coop_cnt = nullptr;
    size_t coop_cnt_bytes = 0;
    half_t* dxh = nullptr;
    half_t* dh = nullptr;
    half_t* dqkv = nullptr;
    half_t* datt = nullptr;
    float* dcls = nullptr;     // [round_up(batch,128), d] f32
    half_t* gemb16 = nullptr;  // [round_up(batch,128), E] f16
    float* scale = nullptr;    // [2] loss scale and its inverse
    size_t bytes = 0;
};

struct grip_tower {
    grip_dims D;
    Layout L;
    half_t* w16;      // GEMM-operand blob: f16, or f32 when f32 != 0 (exact mode) -- always addressed through wop()
    float* w32;
    int f32 = 0;      // dims.precision != 0: activations, residual stream, attention and the operand blob's primary slots are f32 (inference only)
    int w_exact = 0;  // precision 2: no block weight has a non-zero lo part and the split images are the duplicated ones (set by grip_tower_finalize; GemmArgs::w_exact)
    int split = 0;    // dims.precision == 2: the four GEMMs of a block run on the split-f16 kernel (gemm_split.hip); their A operands are written in
                      // its layout by the producers (LayerNorm, f32 attention, GELU epilogue), their weights by grip_tower_finalize (#S slots)
    uint64_t generation = 0;   // counts train-mode forwards (see `pending`)
    const void* wop(int64_t elem_off) const { return (const char*)w16 + elem_off * (f32 ? 4 : 2); }
    void* wop(int64_t elem_off) { return (char*)w16 + elem_off * (f32 ? 4 : 2); }
    bool finalized = false;
    // State of the train-mode forwards whose activations are still waiting for their backward, keyed by workspace: several
    // forwards may be outstanding at once (model(aug_1) and model(aug_2) before one loss.backward()), each on its own
    // workspace.  A second train-mode forward on the SAME workspace overwrites the first one's activations; its generation
    // number replaces the first one's, so a backward that presents the old generation fails with GRIP_ERR_STATE instead
    // of returning gradients of the wrong forward.
    struct TrainState {
        Workspace w;
        const int32_t* eot = nullptr;
        int prefix_classes = 0;
        bool per_image = false;    // vision: the forward ran with GRIP_FWD_PER_IMAGE_PREFIX (prefix and its gradient are [batch, n_prefix, width])
        int n_deep = 0;            // deep prompts of the forward (grip_vit_forward_deep / grip_text_forward_deep): its backward is grip_vit_backward_deep / grip_text_backward_deep
        uint64_t generation = 0;
        bool consumed = false;     // its backward has run (the backward works in place on the saved activations: one per forward)
    };
    std::map<void*, TrainState> pending;
};

// GRIP_LAST_BLOCK_FULL=1: the last block runs for every row, as the reference's does (A/B; the tests hold the two paths equal)
static bool last_block_full() {
    static const bool full = getenv("GRIP_LAST_BLOCK_FULL") && atoi(getenv("GRIP_LAST_BLOCK_FULL")) != 0;
    return full;
}

// Train-mode forwards of the text tower run LayerNorm-folded GEMMs (run_blocks).
static bool train_fold(const grip_tower* t) {
    // GRIP_TRAIN_FOLD (developer A/B): 0 = off, 1 = text tower only, 2 = both towers (default)
    static const int mode = getenv("GRIP_TRAIN_FOLD") ? atoi(getenv("GRIP_TRAIN_FOLD")) : 2;
    return !t->f32 && (mode >= 2 || (mode == 1 && t->D.kind == 1));
}

static int carve(const grip_tower* t, int batch, int P, int train, char* base, Workspace& w, int seq_len = 0, int shared = 0) {
    const grip_dims& D = t->D;
    GRIP_REQUIRE(batch > 0 && P >= 0 && P <= D.max_prefix, "batch must be positive and 0 <= n_prefix <= max_prefix (batch=%d n_prefix=%d max=%d)", batch, P, D.max_prefix);
    const int64_t d = D.width;
    const size_t es = t->f32 ? 4 : 2;      // activation / operand element size
    GRIP_REQUIRE(!(t->f32 && train), "exact (f32) towers are inference-only: no train-mode workspace");
    w.batch = batch; w.P = P; w.train = train;
    GRIP_REQUIRE(seq_len >= 0 && seq_len <= D.seq0 && (D.kind == 1 || seq_len == 0), "seq_len %d out of range", seq_len);
    w.S = D.kind == 0 ? D.seq0 + P : (seq_len ? seq_len : D.seq0);
    GRIP_REQUIRE(D.kind == 0 || P < w.S - 1, "text: n_prefix %d does not fit the sequence length %d", P, w.S);
    GRIP_REQUIRE(w.S <= 608, "sequence length %d exceeds the fused-attention limit 608", w.S);
    GRIP_REQUIRE(!shared || (D.kind == 1 && P > 0 && !t->f32), "the shared-prefix layout is the f16 text tower's, with a context (n_prefix > 0)");
    w.Ps = shared ? P + 1 : 0;
    w.rs = w.S - w.Ps;
    w.M = w.Ps + batch * (int64_t)w.rs;
    w.Mp = round_up64(w.M, 256);
    const int64_t Bp = round_up64(batch, 256);
    size_t off = 0;
    // every buffer is handed out by name: grip_debug_tower_slot (w.rec set) reports exactly what the passes get
    auto take = [&](const char* name, size_t nbytes, int layer = -1) {
        char* p = base ? base + off : nullptr;
        if (w.rec) w.rec->push_back({name, layer, off, nbytes});
        off += (nbytes + 255) / 256 * 256;
        return (void*)p;
    };
    if (!train) w.x = (resid_t*)take("x", w.Mp * d * es);
    if (!train && !t->f32) w.x_lo = (half_t*)take("x_lo", w.Mp * d * 2);      // lo parts of a compensated stream (GRIP_FWD_STREAM_HILO)
    w.xn = (half_t*)take("xn", w.Mp * d * es);
    if (!train) { w.qkv = (half_t*)take("qkv", w.Mp * 3 * d * es); w.att = (half_t*)take("att", w.Mp * d * es); }
    const size_t h_off = off;
    w.h = (half_t*)take("h", w.Mp * 4 * d * es);
    w.cls16 = (half_t*)take("cls16", Bp * d * es);
    w.rows_last = train && !t->f32 && !shared && !last_block_full();
    if (!train || w.rows_last) {       // compact [batch, .] buffers of a last block that runs for the read rows only (f32 / split towers: 4-byte elements)
        w.row_x = (half_t*)take("row_x", Bp * d * es);
        if (!train && !t->f32) w.row_x_lo = (half_t*)take("row_x_lo", Bp * d * 2);
        w.row_att = (half_t*)take("row_att", Bp * d * es);
        w.row_xn = (half_t*)take("row_xn", Bp * d * es);
        w.row_h = (half_t*)take("row_h", Bp * 4 * d * es);
    }
    if (w.rows_last) {
        w.row_hpre = (half_t*)take("row_hpre", Bp * 4 * d * 2);
        w.row_xmid = (resid_t*)take("row_xmid", Bp * d * sizeof(resid_t));
        w.row_xout = (resid_t*)take("row_xout", Bp * d * sizeof(resid_t));
        w.drow = (float*)take("drow", Bp * d * 4);
        w.drow_h = (half_t*)take("drow_h", Bp * d * 2);
        w.row_dh = (half_t*)take("row_dh", Bp * 4 * d * 2);
        w.ks_row = gemm_pick_ksplit(batch, d, 4 * d);
        w.row_dln = (float*)take("row_dln", Bp * d * 4 * (size_t)w.ks_row);
        w.row_datt = (half_t*)take("row_datt", Bp * d * 2);
    }
    if (!t->f32) {
        w.stat_part = (float*)take("stat_part", w.Mp * (d / 64) * 2 * sizeof(float));
        w.rowstat = (float*)take("rowstat", w.Mp * 2 * sizeof(float));
    }
    if (D.kind == 0) {
        const int64_t G2 = D.seq0 - 1;
        const int64_t prow = round_up64(batch * G2, 256);
        if (prow * t->L.kpad <= w.Mp * 4 * d) {      // alias of h when it fits: recorded at h's offset
            w.patches = w.h;
            if (w.rec) w.rec->push_back({"patches", -1, h_off, (size_t)(prow * t->L.kpad) * es});
        } else w.patches = (half_t*)take("patches", prow * t->L.kpad * es);
        w.patch_out = (float*)take("patch_out", batch * G2 * d * 4);
    }
    if (train) {
        const int Lc = D.layers;
        w.x_in.assign((size_t)Lc + 1, nullptr); w.x_mid.assign((size_t)Lc, nullptr);
        w.qkv_l.assign((size_t)Lc, nullptr); w.att_l.assign((size_t)Lc, nullptr); w.hpre_l.assign((size_t)Lc, nullptr);
        for (int i = 0; i <= Lc; ++i) w.x_in[(size_t)i] = (resid_t*)take("x_in", w.Mp * d * sizeof(resid_t), i);
        for (int i = 0; i < Lc; ++i) {
            w.x_mid[(size_t)i] = (resid_t*)take("x_mid", w.Mp * d * sizeof(resid_t), i);
            w.qkv_l[(size_t)i] = (half_t*)take("qkv_l", w.Mp * 3 * d * 2, i);
            w.att_l[(size_t)i] = (half_t*)take("att_l", w.Mp * d * 2, i);
            w.hpre_l[(size_t)i] = (half_t*)take("hpre_l", w.Mp * 4 * d * 2, i);
        }
        w.dx = (float*)take("dx", w.Mp * d * 4);
        // split-K partial buffers of the two EPI_F32 input-gradient GEMMs of a block (summed by ln_bwd_add)
        w.ks_fc = gemm_pick_ksplit((int)w.M, d, 4 * d);
        w.ks_in = gemm_pick_ksplit((int)w.M, d, 3 * d);
        w.dln = (float*)take("dln", w.Mp * d * 4 * (size_t)(w.ks_fc > w.ks_in ? w.ks_fc : w.ks_in));
        w.dxh = (half_t*)take("dxh", w.Mp * d * 2);
        w.dh = (half_t*)take("dh", w.Mp * 4 * d * 2);
        w.dqkv = (half_t*)take("dqkv", w.Mp * 3 * d * 2);
        w.datt = (half_t*)take("datt", w.Mp * d * 2);
        w.dcls = (float*)take("dcls", Bp * d * 4);
        w.gemb16 = (half_t*)take("gemb16", Bp * D.embed_dim * 2);
        w.scale = (float*)take("scale", 2 * sizeof(float));
        if (w.Ps) w.kv_part = (float*)take("kv_part", (size_t)batch * w.Ps * 2 * d * 4);
        if (D.kind == 1 && !t->f32) {      // text tower, f16
            w.coop_ks = gemm_pick_coop_split((int)w.M, d, 4 * d);
            if (w.coop_ks > 1) {
                const size_t tiles = (size_t)((w.M + 63) / 64) * (size_t)(d / 128);
                w.coop_scratch = (float*)take("coop_scratch", tiles * (size_t)w.coop_ks * 4 * 2048 * sizeof(float));
                w.coop_cnt_bytes = tiles * 4 * sizeof(int);
                w.coop_cnt = (int*)take("coop_cnt", w.coop_cnt_bytes);
            }
        }
    }
    w.bytes = off;
    return GRIP_OK;
}

extern "C" int grip_tower_create(const grip_dims* dims, void* f16_blob, void* f32_blob, grip_tower** out) {
    GRIP_REQUIRE(dims && f16_blob && f32_blob && out, "tower_create: null pointer");
    try {
        grip_tower* t = new grip_tower();
        t->D = *dims;
        if (dims->precision < 0 || dims->precision > 2) { delete t; GRIP_REQUIRE(false, "dims.precision must be 0 (f16), 1 (f32 exact) or 2 (split f16)"); }
        if (dims->precision == 2 && dims->width % 256 != 0) { delete t; GRIP_REQUIRE(false, "precision 2 (split f16) needs width %% 256 == 0 (256 x 256 GEMM tiles); width = %d", dims->width); }
        t->f32 = dims->precision != 0;
        t->split = dims->precision == 2;
        int rc = build_layout(*dims, t->L);
        if (rc) { delete t; return rc; }
        t->w16 = (half_t*)f16_blob;
        t->w32 = (float*)f32_blob;
        *out = t;
        return GRIP_OK;
    } catch (...) { grip_set_error("tower_create: exception"); return GRIP_ERR_ARG; }
}

extern "C" int grip_tower_destroy(grip_tower* t) {
    delete t;
    return GRIP_OK;
}

extern "C" int grip_tower_finalize(grip_tower* t, void* stream) {
    GRIP_REQUIRE(t, "tower_finalize: null handle");
    hipStream_t s = (hipStream_t)stream;
    const int d = t->D.width;
    int rc;
    const int f = t->f32;
    if (!f)       // the per-layer transposes feed the dgrad GEMMs only: exact towers have no backward
        for (const LayerW& w : t->L.layer) {
            if ((rc = launch_transpose(t->wop(w.in_w), t->wop(w.in_wT), f, 3 * d, d, d, s))) return rc;
            if ((rc = launch_transpose(t->wop(w.out_w), t->wop(w.out_wT), f, d, d, d, s))) return rc;
            if ((rc = launch_transpose(t->wop(w.fc_w), t->wop(w.fc_wT), f, 4 * d, d, d, s))) return rc;
            if ((rc = launch_transpose(t->wop(w.proj_w), t->wop(w.proj_wT), f, d, 4 * d, 4 * d, s))) return rc;
        }
    if (!f)       // LayerNorm-folded operands of the QKV and c_fc GEMMs (EPI_LNFOLD_*): W' = f16(gamma o W), colsum(W'), W beta + b
        for (const LayerW& w : t->L.layer) {
            float* F = t->w32;
            if ((rc = launch_ln_fold_weights(t->w16 + w.in_w, F + w.ln1_g, F + w.ln1_b, F + w.in_b, t->w16 + w.in_wG, F + w.in_cs, F + w.in_bb, 3 * d, d, s))) return rc;
            if ((rc = launch_ln_fold_weights(t->w16 + w.fc_w, F + w.ln2_g, F + w.ln2_b, F + w.fc_b, t->w16 + w.fc_wG, F + w.fc_cs, F + w.fc_bb, 4 * d, d, s))) return rc;
        }
    if (t->split) { // split-layout copies of the block weights (the f32 originals stay: patch embedding and the final projection use them)
        int* flag = nullptr;        // [0] raised by the split kernel when a scaled weight leaves the f16 range, [1] when a weight is not an f16 number
        GRIP_CHECK_HIP(hipMalloc((void**)&flag, 2 * sizeof(int)));      // (finalize is a one-off: a sync here is fine)
        hipError_t e = hipMemsetAsync(flag, 0, 2 * sizeof(int), s);
        rc = e == hipSuccess ? GRIP_OK : GRIP_ERR_HIP;
        for (const LayerW& w : t->L.layer) {
            if (rc) break;
            if ((rc = launch_split_rows((const float*)t->wop(w.in_w), t->wop(w.in_wS), 3 * d, d, d, s, 1, flag, flag + 1))) break;
            if ((rc = launch_split_rows((const float*)t->wop(w.out_w), t->wop(w.out_wS), d, d, d, s, 1, flag, flag + 1))) break;
            if ((rc = launch_split_rows((const float*)t->wop(w.fc_w), t->wop(w.fc_wS), 4 * d, d, d, s, 1, flag, flag + 1))) break;
            if ((rc = launch_split_rows((const float*)t->wop(w.proj_w), t->wop(w.proj_wS), d, 4 * d, 4 * d, s, 1, flag, flag + 1))) break;
        }
        int flags[2] = {0, 0};
        if (!rc && (hipMemcpyAsync(flags, flag, 2 * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)) rc = GRIP_ERR_HIP;
        const int over = flags[0];
        // fp16 checkpoints: no block weight needs its lo part -- the images become [32 w | 32 w] lines in place and the block GEMMs run as plain f16 GEMMs
        // over 2 K (GemmArgs::w_exact).  GRIP_SPLIT_WLO=1 keeps the standard images and with them the three-pass kernel.
        t->w_exact = flags[1] == 0 && gemm_split_dup_weights();
        (void)hipFree(flag);
        if (rc == GRIP_ERR_HIP) { grip_set_error("tower_finalize: HIP error while splitting the weights"); return rc; }
        if (rc) return rc;
        if (t->w_exact)
            for (const LayerW& w : t->L.layer) {
                if ((rc = launch_split_dup_weights(t->wop(w.in_wS), t->wop(w.in_wS), 3 * d, d, s))) return rc;
                if ((rc = launch_split_dup_weights(t->wop(w.out_wS), t->wop(w.out_wS), d, d, s))) return rc;
                if ((rc = launch_split_dup_weights(t->wop(w.fc_wS), t->wop(w.fc_wS), 4 * d, d, s))) return rc;
                if ((rc = launch_split_dup_weights(t->wop(w.proj_wS), t->wop(w.proj_wS), d, 4 * d, s))) return rc;
            }
        GRIP_REQUIRE(!over, "tower_finalize: a block weight times %g leaves the f16 range (or is not finite): split-f16 towers (precision 2) need |w| < %g",
                     (double)gemm_split_weight_scale(), 65504.0 / (double)gemm_split_weight_scale());
    }
    if ((rc = launch_transpose(t->wop(t->L.proj), t->wop(t->L.projT), f, d, t->D.embed_dim, t->D.embed_dim, s))) return rc;
    t->finalized = true;
    return GRIP_OK;
}

extern "C" int grip_workspace_bytes(const grip_tower* t, int batch, int n_prefix, int seq_len, int train, size_t* bytes) {
    GRIP_REQUIRE(t && bytes, "workspace_bytes: null pointer");
    try {
        Workspace w;
        int rc = carve(t, batch, n_prefix, train, nullptr, w, seq_len);
        if (rc) return rc;
        *bytes = w.bytes;
        if (t->D.kind == 1 && n_prefix > 0 && !t->f32) {     // either row layout of a text forward fits (GRIP_FWD_SHARED_PREFIX)
            Workspace ws;
            rc = carve(t, batch, n_prefix, train, nullptr, ws, seq_len, 1);
            if (rc) return rc;
            if (ws.bytes > *bytes) *bytes = ws.bytes;
        }
        return GRIP_OK;
    } catch (...) { grip_set_error("workspace_bytes: exception"); return GRIP_ERR_ARG; }
}

// The carve-up by name (include/grip_amd_debug.h): carve() itself, run without a base pointer, notes every buffer it hands out.
extern "C" int grip_debug_tower_slot(const grip_tower* t, int batch, int n_prefix, int seq_len, int train, int shared, int index, const char** name, int* layer,
                                     int64_t* offset_bytes, int64_t* bytes) {
    GRIP_REQUIRE(t && name && layer && offset_bytes && bytes, "debug_tower_slot: null pointer");
    try {
        std::vector<CarveRec> rec;
        Workspace w;
        w.rec = &rec;
        int rc = carve(t, batch, n_prefix, train, nullptr, w, seq_len, shared);
        if (rc) return rc;
        GRIP_REQUIRE(index >= 0 && index < (int)rec.size(), "debug_tower_slot: slot %d past the end (%d)", index, (int)rec.size());
        const CarveRec& r = rec[(size_t)index];
        *name = r.name; *layer = r.layer; *offset_bytes = (int64_t)r.offset; *bytes = (int64_t)r.bytes;
        return GRIP_OK;
    } catch (...) { grip_set_error("debug_tower_slot: exception"); return GRIP_ERR_ARG; }
}

// ---------------------------------------------------------------------------------------------- forward
#define RUN(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)

// Launch budget (grip_debug_launch_budget, include/grip_amd_debug.h): a test may let a tower pass issue its first n kernel launches only, to look at the
// workspace between two launches.  Off (0) unless a test sets it: every launch site then costs one comparison of a host integer.  The budget ends a pass
// BETWEEN launches and switches itself off when it trips or when the pass returns (PassScope), whatever the pass returns.  Per host thread, like the
// error text: a budget set on one thread governs the next pass of that thread alone, and passes on other threads neither see nor cancel it.
static thread_local int64_t g_launch_budget = 0;     // 0 = off, else launches the current pass may still issue + 1
static thread_local int64_t g_launch_count = 0;      // launches the current pass has issued under a budget
static bool launch_budget_spent(const char* what) {
    if (--g_launch_budget > 0) { ++g_launch_count; return false; }
    g_launch_budget = 0;
    grip_set_error("launch budget: stopped after %lld launches, before %s", (long long)g_launch_count, what);
    return true;
}
struct PassScope {      // a tower pass begins and ends: no budget outlives it
    PassScope() { g_launch_count = 0; }
    ~PassScope() { g_launch_budget = 0; }
};
#define LAUNCH(expr) do { if (g_launch_budget && launch_budget_spent(#expr)) return GRIP_ERR_LAUNCH_BUDGET; RUN(expr); } while (0)
extern "C" int grip_debug_launch_budget(int64_t n) {
    g_launch_budget = n > 0 ? n + 1 : 0;
    g_launch_count = 0;
    return GRIP_OK;
}

// One tower pass over the residual stream.  f16 towers never run a stand-alone LayerNorm inside the blocks: the statistics of
// every row travel with the stream -- the assembly / embedding kernel writes (mean, rstd) of x0, each residual GEMM epilogue
// emits the partial sums of the rows it stores and a 104-byte-per-row kernel finalises them -- and ln_1 / ln_2 are folded
// into the QKV / c_fc GEMMs, whose A operand is the raw stream (EPI_LNFOLD_*: rstd (x W'^T - mean colsum(W')) + (W beta + b)).
// That removes two full read + write passes over the stream per block (8.8 % of the pool encode's GPU time in round 1).
// Exact (f32) towers keep the literal LayerNorm -> GEMM sequence.
static int run_blocks(grip_tower* t, Workspace& w, resid_t* x0, int causal, const int32_t* read_rows, hipStream_t s, resid_t** x_final, bool* compact) {
    const int d = t->D.width, H = t->D.heads, f = t->f32;
    const int gf = t->split ? 2 : f;      // GemmArgs.f32 of the four block GEMMs, and the output layout of what feeds them
    const float* F = t->w32;
    resid_t* x = x0;
    const int parts = d / 64;
    // Train-mode forwards (the prompt-tuning batches: a few thousand rows) keep the literal LayerNorm -> GEMM sequence: there the
    // stream is L2-resident and a LayerNorm launch costs ~5 us, while the statistics-carrying epilogues make the 20-us GEMMs of
    // those steps 5 % slower (r02: VPT step 3.8 -> 4.0 ms with the fold).  The switch is the MODE, never the batch size: every
    // inference call computes a row the same way whatever chunk it arrives in (sharded / re-chunked encodes stay bit-identical).
    // r04: train-mode forwards fold as well, without a finalising launch: the GEMM that consumes a stream adds the producer's partial row sums itself
    // (GemmArgs::stat_in; gemm.hip row_stat, fetched per ROW before the K loop).  For the text tower's few hundred rows every kernel is a launch, not a byte
    // count (24 LayerNorm launches of 4.7 us in a 1.5-ms CoOp step); for the image tower's 3 408 rows the folded epilogues cost 1 - 4 us per GEMM against the
    // 5.5-us LayerNorm they replace (VPT step 2.98 -> 2.95 ms, UPT 3.29 -> 3.24 ms, 22 launches fewer; r02's form -- statistics loaded per row group in the
    // epilogue plus a finalising launch -- had been 5 % slower).  The backward is unchanged: it differentiates LayerNorm from the saved stream rows.
    // GRIP_TRAIN_FOLD = 0 / 1 / 2: off / text tower only / both (developer A/B).
    const bool fold = !f && (!w.train || train_fold(t));
    const bool parts_in = fold && w.train;     // consumers read stat_part directly
    // Last block at inference: only ONE row per sequence of the final stream is ever read (CLS: ln_post(x[:, 0]),
    // models/clip_encoders.py:189; EOT: :86-89), and past the block's attention rows do not mix.  So the block computes K and V for
    // every row but its attention output, out-proj, LayerNorm and MLP for that row alone (M = batch instead of batch x S):
    // 2.2 of the block's 2.9 GFLOP per ViT-B/16 image are never issued, the embedding is unchanged.  GRIP_LAST_BLOCK_FULL=1
    // computes the whole block as the reference does (A/B; the tests hold the two paths equal).
    const bool rows_only = fold && !w.train && !last_block_full() && !w.Ps;
    // Compensated stream (GRIP_FWD_STREAM_HILO; inference, folded f16 towers): the two residual epilogues of a block read hi + lo and write both; everything
    // else (the GEMMs' A operand, the last block's gathered rows, ln_post) reads the hi part, i.e. the stream as an f16 tower has always seen it.
    const bool hilo = w.hilo && fold && !w.train && w.x_lo;
    *compact = false;
    for (int l = 0; l < t->D.layers; ++l) {
        const LayerW& lw = t->L.layer[(size_t)l];
        const bool last = l + 1 == t->D.layers;
        if (l >= 1 && l <= w.n_deep) {    // deep prompts: the block's input rows 1 .. P := deep[l - 1] before anything reads x (train: x_in[l], what the backward differentiates)
            if (t->D.kind == 0)
                LAUNCH(launch_vit_deep_insert(w.deep + (size_t)(l - 1) * w.P * d, x, f, hilo ? w.x_lo : nullptr, parts_in ? w.stat_part : nullptr,
                                           (fold && !parts_in) ? w.rowstat : nullptr, w.batch, w.S, w.P, (int)w.M, d, s));
            else      // text tower: either row layout, one context for every class or one per class
                LAUNCH(launch_text_deep_insert(w.deep + (size_t)(l - 1) * w.deep_classes * w.P * d, w.deep_classes, x, f, parts_in ? w.stat_part : nullptr,
                                            (fold && !parts_in) ? w.rowstat : nullptr, w.batch, w.S, w.P, w.Ps, (int)w.M, d, s));
        }
        if (last && rows_only) {
            // K and V of every row (columns d .. 3d of the packed projection); Q only for the rows that are read
            GemmArgs a{};
            a.A = x; a.W = t->w16 + lw.in_wG + (int64_t)d * d; a.M = w.M; a.m_pad = w.Mp; a.N = 2 * d; a.K = d; a.bias = F + lw.in_bb + d; a.colsum = F + lw.in_cs + d;
            a.rowstat = w.rowstat; a.out = w.qkv + d; a.ldc = 3 * d;
            LAUNCH(launch_gemm(EPI_LNFOLD_F16, a, s));
            LAUNCH(launch_gather_rows(x, read_rows, w.S, w.row_x, w.batch, d, s));
            if (hilo) LAUNCH(launch_gather_rows(w.x_lo, read_rows, w.S, w.row_x_lo, w.batch, d, s));      // the read rows keep their compensation through the block's two adds
            LAUNCH(launch_layernorm_f16(w.row_x, F + lw.ln1_g, F + lw.ln1_b, w.row_xn, 0, w.batch, d, s));
            a = GemmArgs{};
            a.A = w.row_xn; a.W = t->w16 + lw.in_w; a.M = w.batch; a.m_pad = round_up64(w.batch, 256); a.N = d; a.K = d; a.bias = F + lw.in_b; a.out = w.row_h; a.ldc = d;
            LAUNCH(launch_gemm(EPI_BIAS_F16, a, s));
            LAUNCH(launch_attention_row(w.qkv, w.row_h, read_rows, w.row_att, w.batch, w.S, H, causal, s));
            const int64_t Bp = round_up64(w.batch, 256);
            a = GemmArgs{};
            a.A = w.row_att; a.W = t->w16 + lw.out_w; a.M = w.batch; a.m_pad = Bp; a.N = d; a.K = d; a.bias = F + lw.out_b; a.resid = w.row_x; a.out = w.row_x; a.ldc = d;
            if (hilo) { a.resid_lo = w.row_x_lo; a.stat_part = w.stat_part; }      // (the compensated form lives in the statistics-carrying epilogue; nobody reads these sums)
            LAUNCH(launch_gemm(EPI_BIAS_RESID, a, s));
            LAUNCH(launch_layernorm_f16(w.row_x, F + lw.ln2_g, F + lw.ln2_b, w.row_xn, 0, w.batch, d, s));
            a = GemmArgs{};
            a.A = w.row_xn; a.W = t->w16 + lw.fc_w; a.M = w.batch; a.m_pad = Bp; a.N = 4 * d; a.K = d; a.bias = F + lw.fc_b; a.out = w.row_h; a.ldc = 4 * d;
            LAUNCH(launch_gemm(EPI_BIAS_GELU_F16, a, s));
            a = GemmArgs{};
            a.A = w.row_h; a.W = t->w16 + lw.proj_w; a.M = w.batch; a.m_pad = Bp; a.N = d; a.K = 4 * d; a.bias = F + lw.proj_b; a.resid = w.row_x; a.out = w.row_x; a.ldc = d;
            if (hilo) { a.resid_lo = w.row_x_lo; a.stat_part = w.stat_part; }
            LAUNCH(launch_gemm(EPI_BIAS_RESID, a, s));
            x = w.row_x;
            *compact = true;
            break;
        }
        if (last && f && !w.train && !last_block_full() && !w.Ps) {
            // The same for the f32 / split-f16 towers (r04: the refinement tiers and the exact mode computed the whole 12th block -- 6 % of their FLOPs -- for
            // one row per image): ln_1 and the K / V projection for every row, then the read rows alone: Q, a one-row f32 attention, out-proj, ln_2, MLP.
            const int64_t Bp = round_up64(w.batch, 256);
            const size_t wb = (size_t)d * d * 4;                      // bytes of d weight rows (f32 elements, or the split layout: the same row pitch)
            const char* in_w = (const char*)t->wop(t->split ? lw.in_wS : lw.in_w);
            float* qkv32 = (float*)(void*)w.qkv;
            GemmArgs a{};
            LAUNCH(launch_layernorm_f16(x, F + lw.ln1_g, F + lw.ln1_b, w.xn, gf, w.M, d, s));
            a.f32 = gf; a.w_exact = t->w_exact; a.A = w.xn; a.W = in_w + wb; a.M = w.M; a.m_pad = w.Mp; a.N = 2 * d; a.K = d; a.bias = F + lw.in_b + d; a.out = qkv32 + d; a.ldc = 3 * d;
            LAUNCH(launch_gemm(EPI_BIAS_F16, a, s));
            LAUNCH(launch_gather_rows4(x, read_rows, w.S, w.row_x, w.batch, d, s));
            LAUNCH(launch_gather_rows4(w.xn, read_rows, w.S, w.row_xn, w.batch, d, s));
            a = GemmArgs{};
            a.f32 = gf; a.w_exact = t->w_exact; a.A = w.row_xn; a.W = in_w; a.M = w.batch; a.m_pad = Bp; a.N = d; a.K = d; a.bias = F + lw.in_b; a.out = w.row_h; a.ldc = d;
            LAUNCH(launch_gemm(EPI_BIAS_F16, a, s));
            LAUNCH(launch_attention_row_f32(qkv32, (const float*)(const void*)w.row_h, read_rows, (float*)(void*)w.row_att, w.batch, w.S, H, causal, s, t->split));
            a = GemmArgs{};
            a.f32 = gf; a.w_exact = t->w_exact; a.A = w.row_att; a.W = t->wop(t->split ? lw.out_wS : lw.out_w); a.M = w.batch; a.m_pad = Bp; a.N = d; a.K = d; a.bias = F + lw.out_b;
            a.resid = w.row_x; a.out = w.row_x; a.ldc = d;
            LAUNCH(launch_gemm(EPI_BIAS_RESID, a, s));
            LAUNCH(launch_layernorm_f16(w.row_x, F + lw.ln2_g, F + lw.ln2_b, w.row_xn, gf, w.batch, d, s));
            a = GemmArgs{};
            a.f32 = gf; a.w_exact = t->w_exact; a.A = w.row_xn; a.W = t->wop(t->split ? lw.fc_wS : lw.fc_w); a.M = w.batch; a.m_pad = Bp; a.N = 4 * d; a.K = d; a.bias = F + lw.fc_b; a.out = w.row_h; a.ldc = 4 * d;
            LAUNCH(launch_gemm(EPI_BIAS_GELU_F16, a, s));
            a = GemmArgs{};
            a.f32 = gf; a.w_exact = t->w_exact; a.A = w.row_h; a.W = t->wop(t->split ? lw.proj_wS : lw.proj_w); a.M = w.batch; a.m_pad = Bp; a.N = d; a.K = 4 * d; a.bias = F + lw.proj_b;
            a.resid = w.row_x; a.out = w.row_x; a.ldc = d;
            LAUNCH(launch_gemm(EPI_BIAS_RESID, a, s));
            x = w.row_x;
            *compact = true;
            break;
        }
        if (last && w.rows_last) {
            // The same in TRAIN mode (prompt steps; plain row layout): the block's K, V and -- one GEMM, saved for the backward -- Q of every
            // row, then attention output, out-proj, ln_2 and the MLP for the read rows alone, each saving what its backward needs in compact
            // [batch, .] buffers.  The backward (run_blocks_backward) mirrors it: 0.14 ms of a 3.15-ms VPT step.
            const int64_t Bp = round_up64(w.batch, 256);
            half_t* qkv = w.qkv_l[(size_t)l];
            GemmArgs a{};
            LAUNCH(launch_layernorm_f16(x, F + lw.ln1_g, F + lw.ln1_b, w.xn, 0, w.M, d, s));
            a.rot_rows = 1;
            a.A = w.xn; a.W = t->w16 + lw.in_w; a.M = w.M; a.m_pad = w.Mp; a.N = 3 * d; a.K = d; a.bias = F + lw.in_b; a.out = qkv; a.ldc = 3 * d;
            LAUNCH(launch_gemm(EPI_BIAS_F16, a, s));
            LAUNCH(launch_attention_row(qkv, nullptr, read_rows, w.row_att, w.batch, w.S, H, causal, s, /*train=*/1));
            LAUNCH(launch_gather_rows(x, read_rows, w.S, w.row_x, w.batch, d, s));
            a = GemmArgs{};
            a.A = w.row_att; a.W = t->w16 + lw.out_w; a.M = w.batch; a.m_pad = Bp; a.N = d; a.K = d; a.bias = F + lw.out_b; a.resid = w.row_x; a.out = w.row_xmid; a.ldc = d;
            LAUNCH(launch_gemm(EPI_BIAS_RESID, a, s));
            LAUNCH(launch_layernorm_f16(w.row_xmid, F + lw.ln2_g, F + lw.ln2_b, w.row_xn, 0, w.batch, d, s));
            a = GemmArgs{};
            a.A = w.row_xn; a.W = t->w16 + lw.fc_w; a.M = w.batch; a.m_pad = Bp; a.N = 4 * d; a.K = d; a.bias = F + lw.fc_b; a.out = w.row_h; a.out2 = w.row_hpre; a.ldc = 4 * d;
            LAUNCH(launch_gemm(EPI_BIAS_GELU_F16, a, s));
            a = GemmArgs{};
            a.A = w.row_h; a.W = t->w16 + lw.proj_w; a.M = w.batch; a.m_pad = Bp; a.N = d; a.K = 4 * d; a.bias = F + lw.proj_b; a.resid = w.row_xmid; a.out = w.row_xout; a.ldc = d;
            LAUNCH(launch_gemm(EPI_BIAS_RESID, a, s));
            x = w.row_xout;
            *compact = true;
            break;
        }
        half_t* qkv = w.train ? w.qkv_l[(size_t)l] : w.qkv;
        half_t* att = w.train ? w.att_l[(size_t)l] : w.att;
        resid_t* x_mid = w.train ? w.x_mid[(size_t)l] : x;
        resid_t* x_out = w.train ? w.x_in[(size_t)l + 1] : x;
        GemmArgs a{};
        a.rot_rows = w.train;     // train-mode GEMMs may stagger their K walks by tile row (common.h)
        if (!fold) {
            LAUNCH(launch_layernorm_f16(x, F + lw.ln1_g, F + lw.ln1_b, w.xn, gf, w.M, d, s));
            a.f32 = gf; a.w_exact = t->w_exact; a.A = w.xn; a.W = t->wop(t->split ? lw.in_wS : lw.in_w); a.M = w.M; a.m_pad = w.Mp; a.N = 3 * d; a.K = d; a.bias = F + lw.in_b; a.out = qkv; a.ldc = 3 * d;
            LAUNCH(launch_gemm(EPI_BIAS_F16, a, s));
            if (t->split && attention_split_supported(w.S)) LAUNCH(launch_attention_fwd_split((const float*)(const void*)qkv, att, w.batch, w.S, H, causal, s));
            else if (f) LAUNCH(launch_attention_fwd_f32((const float*)(const void*)qkv, (float*)(void*)att, w.batch, w.S, H, causal, s, t->split));
            else LAUNCH(launch_attention_fwd(qkv, att, w.batch, w.S, H, causal, s, w.Ps));
        } else {
            a.A = x; a.W = t->w16 + lw.in_wG; a.M = w.M; a.m_pad = w.Mp; a.N = 3 * d; a.K = d; a.bias = F + lw.in_bb; a.colsum = F + lw.in_cs; a.rowstat = w.rowstat;
            if (parts_in && l > 0) { a.stat_in = w.stat_part; a.stat_parts = parts; }      // (block 0: the embedding kernel wrote rowstat)
            a.out = qkv; a.ldc = 3 * d;
            LAUNCH(launch_gemm(EPI_LNFOLD_F16, a, s));
            LAUNCH(launch_attention_fwd(qkv, att, w.batch, w.S, H, causal, s, w.Ps));
        }
        a = GemmArgs{};
        a.rot_rows = w.train;
        a.f32 = gf; a.w_exact = t->w_exact; a.A = att; a.W = t->wop(t->split ? lw.out_wS : lw.out_w); a.M = w.M; a.m_pad = w.Mp; a.N = d; a.K = d; a.bias = F + lw.out_b; a.resid = x; a.out = x_mid; a.ldc = d;
        a.stat_part = fold ? w.stat_part : nullptr;
        a.resid_lo = hilo ? w.x_lo : nullptr;
        LAUNCH(launch_gemm(EPI_BIAS_RESID, a, s));
        a = GemmArgs{};
        a.rot_rows = w.train;
        if (!fold) {
            LAUNCH(launch_layernorm_f16(x_mid, F + lw.ln2_g, F + lw.ln2_b, w.xn, gf, w.M, d, s));
            a.f32 = gf; a.w_exact = t->w_exact; a.A = w.xn; a.W = t->wop(t->split ? lw.fc_wS : lw.fc_w); a.bias = F + lw.fc_b;
        } else {
            if (parts_in) { a.stat_in = w.stat_part; a.stat_parts = parts; }
            else LAUNCH(launch_ln_stats_finalize(w.stat_part, parts, w.rowstat, w.M, d, s));
            a.A = x_mid; a.W = t->w16 + lw.fc_wG; a.bias = F + lw.fc_bb; a.colsum = F + lw.fc_cs; a.rowstat = w.rowstat;
        }
        a.M = w.M; a.m_pad = w.Mp; a.N = 4 * d; a.K = d; a.out = w.h; a.ldc = 4 * d;
        a.out2 = w.train ? w.hpre_l[(size_t)l] : nullptr;
        if (fold) LAUNCH(launch_gemm(EPI_LNFOLD_GELU_F16, a, s));      // (two sites: a launch budget names the call it stops before)
        else LAUNCH(launch_gemm(EPI_BIAS_GELU_F16, a, s));
        a = GemmArgs{};
        a.rot_rows = w.train;
        a.f32 = gf; a.w_exact = t->w_exact; a.A = w.h; a.W = t->wop(t->split ? lw.proj_wS : lw.proj_w); a.M = w.M; a.m_pad = w.Mp; a.N = d; a.K = 4 * d; a.bias = F + lw.proj_b; a.resid = x_mid; a.out = x_out; a.ldc = d;
        a.stat_part = (!fold || (last && !hilo)) ? nullptr : w.stat_part;     // the final LayerNorm (CLS / EOT rows only) reads the stream itself
        a.resid_lo = hilo ? w.x_lo : nullptr;      // (the compensated form lives in the statistics-carrying epilogue: the last block's unread sums are its price)
        if (w.train && w.coop_ks > 1) { a.ksplit = w.coop_ks; a.coop_scratch = w.coop_scratch; a.coop_counter = w.coop_cnt; }
        LAUNCH(launch_gemm(EPI_BIAS_RESID, a, s));
        if (fold && !last && !parts_in) LAUNCH(launch_ln_stats_finalize(w.stat_part, parts, w.rowstat, w.M, d, s));
        x = x_out;
    }
    *x_final = x;
    return GRIP_OK;
}

static int check_ws(grip_tower* t, int batch, int P, int train, void* ws, size_t ws_bytes, Workspace& w, int seq_len = 0, int shared = 0) {
    GRIP_REQUIRE(t && ws, "null tower / workspace");
    if (!t->finalized) { grip_set_error("tower not finalized: call grip_tower_finalize after filling the weight blobs"); return GRIP_ERR_STATE; }
    RUN(carve(t, batch, P, train, (char*)ws, w, seq_len, shared));
    if (w.bytes > ws_bytes) { grip_set_error("workspace too small: need %zu bytes, got %zu", w.bytes, ws_bytes); return GRIP_ERR_WORKSPACE; }
    GRIP_REQUIRE(((uintptr_t)ws & 255) == 0, "workspace must be 256-byte aligned");
    return GRIP_OK;
}

// Book-keeping of a finished forward: a train-mode one registers its state under the workspace (replacing whatever
// forward used that workspace before) and hands out a fresh generation number; an inference one invalidates it.
static void note_forward(grip_tower* t, void* workspace, int train, const Workspace& w, const int32_t* eot, int prefix_classes, uint64_t* generation,
                         bool per_image = false, int n_deep = 0) {
    if (train) {
        // Consumed entries only serve a clearer error message ("already back-propagated"); workspaces that were freed since (pools dropped with a
        // key change, graph pins released per GRIP iteration) would otherwise stay in the map for good, and a recycled address could hit a stale one.
        if (t->pending.size() > 32)
            for (auto it = t->pending.begin(); it != t->pending.end();)
                it = (it->second.consumed && it->first != workspace) ? t->pending.erase(it) : std::next(it);
        grip_tower::TrainState& st = t->pending[workspace];
        st.w = w; st.eot = eot; st.prefix_classes = prefix_classes; st.per_image = per_image; st.n_deep = n_deep; st.generation = ++t->generation; st.consumed = false;
        if (generation) *generation = st.generation;
    } else {
        t->pending.erase(workspace);
        if (generation) *generation = 0;
    }
}

extern "C" int grip_vit_forward_deep(grip_tower* t, const void* images, int images_f16, const float* prefix, int n_prefix, const float* deep, int n_deep,
                                     int batch, float* out_emb, void* workspace, size_t workspace_bytes, int flags, uint64_t* generation, void* stream) {
    PassScope pass_scope;
    try {
        GRIP_REQUIRE(t && t->D.kind == 0, "vit_forward: not a vision tower%s", n_deep ? " (deep prompts are a vision-tower feature)" : "");
        GRIP_REQUIRE(n_deep >= 0 && n_deep <= t->D.layers - 1, "vit_forward_deep: n_deep = %d out of range: deep prompts replace the prompt rows entering blocks 1 .. n_deep, "
                     "0 <= n_deep <= layers - 1 = %d", n_deep, t->D.layers - 1);
        GRIP_REQUIRE(n_deep == 0 || n_prefix > 0, "vit_forward_deep: deep prompts replace the rows of the shallow prompt: n_prefix must be positive (n_deep = %d)", n_deep);
        GRIP_REQUIRE(n_deep == 0 || deep, "vit_forward_deep: null deep prompt pointer (n_deep = %d)", n_deep);
        GRIP_REQUIRE(n_deep == 0 || !(flags & GRIP_FWD_PER_IMAGE_PREFIX), "vit_forward_deep: deep prompts are shared by the batch: not valid with GRIP_FWD_PER_IMAGE_PREFIX");
        GRIP_REQUIRE((flags & ~(GRIP_FWD_TRAIN | GRIP_FWD_NO_POS_EMB | GRIP_FWD_STREAM_HILO | GRIP_FWD_PER_IMAGE_PREFIX)) == 0, "vit_forward: unknown flag bits 0x%x", flags);
        const int train = flags & GRIP_FWD_TRAIN;
        const int per_image = (flags & GRIP_FWD_PER_IMAGE_PREFIX) ? 1 : 0;      // prefix [batch, n_prefix, width]: rows (b, 1 .. P) read image b's prompt
        GRIP_REQUIRE(!(flags & GRIP_FWD_STREAM_HILO) || (!train && !t->f32), "vit_forward: GRIP_FWD_STREAM_HILO is an inference mode of the f16 towers");
        GRIP_REQUIRE(images && out_emb && (n_prefix == 0 || prefix), "vit_forward: null pointer");
        Workspace w;
        RUN(check_ws(t, batch, n_prefix, train, workspace, workspace_bytes, w));
        if (g_launch_budget) t->pending.erase(workspace);      // a forward that may stop early leaves no pending state behind
        w.deep = n_deep ? deep : nullptr;
        w.n_deep = n_deep;
        hipStream_t s = (hipStream_t)stream;
        const grip_dims& D = t->D;
        const int d = D.width, G2 = D.seq0 - 1, f = t->f32;
        const float* F = t->w32;
        LAUNCH(launch_im2col(images, images_f16, w.patches, f, batch, D.resolution, D.patch, t->L.kpad, s));
        GemmArgs a{};
        a.f32 = f; a.A = w.patches; a.W = t->wop(t->L.conv_w); a.M = batch * G2; a.m_pad = round_up64((int64_t)batch * G2, 256); a.N = d; a.K = t->L.kpad; a.out = w.patch_out; a.ldc = d;
        LAUNCH(launch_gemm(EPI_F32, a, s));
        resid_t* x0 = train ? w.x_in[0] : w.x;
        w.hilo = (flags & GRIP_FWD_STREAM_HILO) ? 1 : 0;
        LAUNCH(launch_vit_assemble_ln(w.patch_out, F + t->L.cls, (flags & GRIP_FWD_NO_POS_EMB) ? nullptr : F + t->L.pos, prefix, n_prefix, F + t->L.lnpre_g, F + t->L.lnpre_b, x0, f, (train && !train_fold(t)) ? nullptr : w.rowstat, batch, G2, d, s,
                                   w.hilo ? w.x_lo : nullptr, per_image));
        resid_t* xf = nullptr;
        bool compact = false;
        RUN(run_blocks(t, w, x0, /*causal=*/0, nullptr, s, &xf, &compact));
        LAUNCH(launch_gather_ln_f16(xf, nullptr, compact ? 1 : w.S, F + t->L.lnpost_g, F + t->L.lnpost_b, w.cls16, f, batch, d, s));
        a = GemmArgs{};
        a.f32 = f; a.A = w.cls16; a.W = t->wop(t->L.projT); a.M = batch; a.N = D.embed_dim; a.K = d; a.out = out_emb; a.ldc = D.embed_dim;
        LAUNCH(launch_gemm(EPI_F32, a, s));
        note_forward(t, workspace, train, w, nullptr, 0, generation, per_image != 0, n_deep);
        return GRIP_OK;
    } catch (...) { grip_set_error("vit_forward: exception"); return GRIP_ERR_ARG; }
}

extern "C" int grip_vit_forward(grip_tower* t, const void* images, int images_f16, const float* prefix, int n_prefix,
                                int batch, float* out_emb, void* workspace, size_t workspace_bytes, int flags, uint64_t* generation, void* stream) {
    return grip_vit_forward_deep(t, images, images_f16, prefix, n_prefix, nullptr, 0, batch, out_emb, workspace, workspace_bytes, flags, generation, stream);
}

extern "C" int grip_text_forward_deep(grip_tower* t, const int32_t* token_ids, const int32_t* eot_index, const float* prefix,
                                      int n_prefix, int prefix_classes, const float* deep, int n_deep, int n_class, int seq_len, float* out_emb,
                                      void* workspace, size_t workspace_bytes, int flags, uint64_t* generation, void* stream) {
    PassScope pass_scope;
    try {
        GRIP_REQUIRE(t && t->D.kind == 1, "text_forward: not a text tower%s", n_deep ? " (the vision tower's deep prompts go through grip_vit_forward_deep)" : "");
        GRIP_REQUIRE(n_deep >= 0 && n_deep <= t->D.layers - 1, "text_forward_deep: n_deep = %d out of range: deep prompts replace the context rows entering blocks 1 .. n_deep, "
                     "0 <= n_deep <= layers - 1 = %d", n_deep, t->D.layers - 1);
        GRIP_REQUIRE(n_deep == 0 || n_prefix > 0, "text_forward_deep: deep prompts replace the rows of the shallow context: n_prefix must be positive (n_deep = %d)", n_deep);
        GRIP_REQUIRE(n_deep == 0 || deep, "text_forward_deep: null deep prompt pointer (n_deep = %d)", n_deep);
        GRIP_REQUIRE(token_ids && eot_index && out_emb && (n_prefix == 0 || prefix), "text_forward: null pointer");
        GRIP_REQUIRE(!(flags & GRIP_FWD_PER_IMAGE_PREFIX), "text_forward: GRIP_FWD_PER_IMAGE_PREFIX is a vision-tower flag (one context per class: prefix_classes = n_class)");
        GRIP_REQUIRE(n_prefix == 0 || prefix_classes == 1 || prefix_classes == n_class, "text_forward: prefix_classes must be 1 or n_class");
        GRIP_REQUIRE((flags & ~(GRIP_FWD_TRAIN | GRIP_FWD_SHARED_PREFIX | GRIP_FWD_NO_POS_EMB)) == 0, "text_forward: unknown flag bits 0x%x", flags);
        const int train = flags & GRIP_FWD_TRAIN;
        // the caller vouches for identical tokens at positions 0 .. n_prefix in every class; exact (f32) towers keep the plain layout
        const int shared = (flags & GRIP_FWD_SHARED_PREFIX) && n_prefix > 0 && prefix_classes == 1 && !t->f32;
        Workspace w;
        RUN(check_ws(t, n_class, n_prefix, train, workspace, workspace_bytes, w, seq_len, shared));
        if (g_launch_budget) t->pending.erase(workspace);      // a forward that may stop early leaves no pending state behind
        w.deep = n_deep ? deep : nullptr;
        w.n_deep = n_deep;
        w.deep_classes = n_deep ? prefix_classes : 1;
        hipStream_t s = (hipStream_t)stream;
        const grip_dims& D = t->D;
        const int d = D.width, f = t->f32;
        const float* F = t->w32;
        resid_t* x0 = train ? w.x_in[0] : w.x;
        if (train && w.coop_cnt) GRIP_CHECK_HIP(hipMemsetAsync(w.coop_cnt, 0, w.coop_cnt_bytes, s));     // the tickets start at zero (and return to it)
        LAUNCH(launch_text_embed(token_ids, D.seq0, F + t->L.tok, (flags & GRIP_FWD_NO_POS_EMB) ? nullptr : F + t->L.pos, prefix, n_prefix, prefix_classes, x0, f, (train && !train_fold(t)) ? nullptr : w.rowstat, n_class, w.S, d, D.vocab, s, w.Ps));
        resid_t* xf = nullptr;
        bool compact = false;
        RUN(run_blocks(t, w, x0, /*causal=*/1, eot_index, s, &xf, &compact));
        LAUNCH(launch_gather_ln_f16(xf, compact ? nullptr : eot_index, compact ? 1 : w.rs, F + t->L.lnpost_g, F + t->L.lnpost_b, w.cls16, f, n_class, d, s));
        GemmArgs a{};
        a.f32 = f; a.A = w.cls16; a.W = t->wop(t->L.projT); a.M = n_class; a.N = D.embed_dim; a.K = d; a.out = out_emb; a.ldc = D.embed_dim;
        LAUNCH(launch_gemm(EPI_F32, a, s));
        note_forward(t, workspace, train, w, eot_index, prefix_classes, generation, false, n_deep);
        return GRIP_OK;
    } catch (...) { grip_set_error("text_forward: exception"); return GRIP_ERR_ARG; }
}

extern "C" int grip_text_forward(grip_tower* t, const int32_t* token_ids, const int32_t* eot_index, const float* prefix,
                                 int n_prefix, int prefix_classes, int n_class, int seq_len, float* out_emb,
                                 void* workspace, size_t workspace_bytes, int flags, uint64_t* generation, void* stream) {
    return grip_text_forward_deep(t, token_ids, eot_index, prefix, n_prefix, prefix_classes, nullptr, 0, n_class, seq_len, out_emb, workspace, workspace_bytes, flags,
                                  generation, stream);
}

// ---------------------------------------------------------------------------------------------- test hooks
// Kernel-level entry points for the unit parity tests (tests/test_gpu_kernels.py).  Not part of the
// drop-in ABI (declared in include/grip_amd_debug.h, not in grip_amd.h); they launch exactly the kernels the towers use.
extern "C" int grip_debug_gemm(int epi, const void* A, const void* W, int M, int N, int K, const float* bias, const void* resid,
                               const void* aux, void* out, void* out2, float scalar, int m_pad, int variant, void* stream) {
    GemmArgs a{};
    a.variant = variant & 0xff;
    a.rot_rows = (variant >> 8) & 1;                  // bit 8: the train-mode launches' row-dependent K rotation
    a.A = A; a.W = W; a.M = M; a.N = N; a.K = K; a.m_pad = m_pad; a.bias = bias; a.resid = resid;
    a.aux = aux; a.out = out; a.out2 = out2; a.ldc = N; a.scalar = scalar;
    if (a.variant == 7) { a.f32 = 1; a.variant = 0; } // f32 operands: the exact-mode kernel (gemm_f32.hip)
    return launch_gemm(epi, a, (hipStream_t)stream);
}
// Split-K EPI_F32 product: out holds `ksplit` partial [M, N] buffers `split_stride` floats apart (ksplit = 0: the launcher's
// own choice, returned through *ksplit_used); their sum in index order is what ln_bwd_add consumes.
extern "C" int grip_debug_gemm_splitk(const void* A, const void* W, int M, int N, int K, float* out, int ksplit, int64_t split_stride, int* ksplit_used,
                                      int m_pad, int variant, void* stream) {
    GemmArgs a{};
    a.variant = variant & 0xff;
    a.rot_rows = (variant >> 8) & 1;
    a.A = A; a.W = W; a.M = M; a.N = N; a.K = K; a.m_pad = m_pad; a.out = out; a.ldc = N;
    a.ksplit = ksplit ? ksplit : gemm_pick_ksplit(M, N, K);
    a.split_stride = split_stride;
    if (ksplit_used) *ksplit_used = a.ksplit;
    return launch_gemm(EPI_F32, a, (hipStream_t)stream);
}
extern "C" int grip_debug_gemm_ln(int epi, const void* A, const void* W, int M, int N, int K, const float* bias, const void* resid, void* out, void* out2,
                                  float* stat_part, const float* rowstat, const float* colsum, int m_pad, int variant, void* stream) {
    GemmArgs a{};
    a.variant = variant;
    a.A = A; a.W = W; a.M = M; a.N = N; a.K = K; a.m_pad = m_pad; a.bias = bias; a.resid = resid; a.out = out; a.out2 = out2; a.ldc = N;
    a.stat_part = stat_part; a.rowstat = rowstat; a.colsum = colsum;
    return launch_gemm(epi, a, (hipStream_t)stream);
}
// The two prompt-step forms of r04 (csrc/gemm.hip).  epi 7 / 8 with stat_in != NULL: the consumer adds the producer's stat_parts partial pairs itself
// (loader-wave kernels) or the launcher finalises them into `rowstat` (must be writable) first.  epi 3 with ksplit > 1: cooperative split-K, partial
// tiles through coop_scratch (>= tiles * ksplit * 32 KiB), tickets in coop_counter (tiles * 4 ints, zero on entry, zero again on exit).
extern "C" int grip_debug_gemm_train(int epi, const void* A, const void* W, int M, int N, int K, const float* bias, const void* resid, void* out, void* out2,
                                     float* stat_part, float* rowstat, const float* colsum, const float* stat_in, int stat_parts, int ksplit,
                                     float* coop_scratch, int* coop_counter, int m_pad, void* stream) {
    GemmArgs a{};
    a.rot_rows = 1;
    a.A = A; a.W = W; a.M = M; a.N = N; a.K = K; a.m_pad = m_pad; a.bias = bias; a.resid = resid; a.out = out; a.out2 = out2; a.ldc = N;
    a.stat_part = stat_part; a.rowstat = rowstat; a.colsum = colsum; a.stat_in = stat_in; a.stat_parts = stat_parts;
    a.ksplit = ksplit; a.coop_scratch = coop_scratch; a.coop_counter = coop_counter;
    return launch_gemm(epi, a, (hipStream_t)stream);
}
// Every field of GemmArgs that an f16 launch reads, as given (tests/test_gpu_gemm_kernels.py): ldc != N, the compensated stream (resid_lo), EPI_F32_SCALE,
// split-K and the cooperative form on any variant.  No logic of its own: what launch_gemm refuses is refused.
extern "C" int grip_debug_gemm_args(int epi, const void* A, const void* W, int M, int N, int K, int ldc, const float* bias, const void* resid, void* resid_lo,
                                    const void* aux, void* out, void* out2, float scalar, float* stat_part, float* rowstat, const float* colsum,
                                    const float* stat_in, int stat_parts, int ksplit, int64_t split_stride, float* coop_scratch, int* coop_counter, int m_pad,
                                    int variant, int rot_rows, void* stream) {
    GemmArgs a{};
    a.A = A; a.W = W; a.M = M; a.N = N; a.K = K; a.ldc = ldc; a.m_pad = m_pad; a.variant = variant; a.rot_rows = rot_rows;
    a.bias = bias; a.resid = resid; a.resid_lo = (half_t*)resid_lo; a.aux = aux; a.out = out; a.out2 = out2; a.scalar = scalar;
    a.stat_part = stat_part; a.rowstat = rowstat; a.colsum = colsum; a.stat_in = stat_in; a.stat_parts = stat_parts;
    a.ksplit = ksplit; a.split_stride = split_stride; a.coop_scratch = coop_scratch; a.coop_counter = coop_counter;
    return launch_gemm(epi, a, (hipStream_t)stream);
}
extern "C" int grip_debug_coop_split(int M, int N, int K) { return gemm_pick_coop_split(M, N, K); }
extern "C" int grip_debug_ln_fold(const void* W, const float* gamma, const float* beta, const float* bias, void* Wg, float* colsum, float* bias_out,
                                  int N, int K, const float* stat_part, int parts, float* rowstat, int M, int d, void* stream) {
    int rc = W ? launch_ln_fold_weights((const half_t*)W, gamma, beta, bias, (half_t*)Wg, colsum, bias_out, N, K, (hipStream_t)stream) : GRIP_OK;     // W == NULL: the statistics alone
    if (rc || !stat_part) return rc;
    return launch_ln_stats_finalize(stat_part, parts, rowstat, M, d, (hipStream_t)stream);
}
// Split-f16 GEMM (gemm_split.hip) on f32 inputs: A [m_pad, K] and W [N, K] are first rewritten in the split layout into the caller's scratch
// buffers a_split / w_split (4 bytes per element each), then out = epi(A W^T) -- f32, or the split layout for epi 2 (out: 4 bytes per element).
extern "C" int grip_debug_gemm_split(int epi, const float* A, const float* W, int M, int N, int K, const float* bias, const float* resid, void* out,
                                     void* a_split, void* w_split, int m_pad, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    RUN(launch_split_rows(A, a_split, m_pad, K, K, s));
    int* flag = nullptr;        // as grip_tower_finalize: is every element of W an f16 number?  (then the two-product kernel runs: GemmArgs::w_exact)
    GRIP_CHECK_HIP(hipMalloc((void**)&flag, sizeof(int)));
    int inexact = 1;
    int rc = hipMemsetAsync(flag, 0, sizeof(int), s) == hipSuccess ? launch_split_rows(W, w_split, N, K, K, s, 1, nullptr, flag) : GRIP_ERR_HIP;
    if (!rc && (hipMemcpyAsync(&inexact, flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)) rc = GRIP_ERR_HIP;
    (void)hipFree(flag);
    if (rc) return rc;
    GemmArgs a{};
    a.w_exact = !inexact && gemm_split_dup_weights();
    a.f32 = 2; a.A = a_split; a.W = w_split; a.M = M; a.N = N; a.K = K; a.m_pad = m_pad; a.bias = bias; a.resid = resid; a.out = out; a.ldc = N;
    if (!a.w_exact) return launch_gemm(epi, a, s);
    // f16-exact W: the GEMM reads the duplicated image, built in scratch of this call's own (w_split keeps the standard layout for the caller)
    void* w_dup = nullptr;
    GRIP_CHECK_HIP(hipMalloc(&w_dup, (size_t)N * K * 4));
    a.W = w_dup;
    rc = launch_split_dup_weights(w_split, w_dup, N, K, s);
    if (!rc) rc = launch_gemm(epi, a, s);
    if (hipStreamSynchronize(s) != hipSuccess && !rc) { grip_set_error("debug_gemm_split: HIP error"); rc = GRIP_ERR_HIP; }
    (void)hipFree(w_dup);
    return rc;
}
int gemm_split_last_wlo();
extern "C" int grip_debug_split_last_wlo(void) { return gemm_split_last_wlo(); }
// f32 rows -> the split layout (out: 4 bytes per element), e.g. to read a split-layout result back on the host side of a test
extern "C" int grip_debug_split_rows(const float* x, void* out, int64_t rows, int K, void* stream) {
    return launch_split_rows(x, out, rows, K, K, (hipStream_t)stream);
}
// One GEMM launch of the f32 (tier 1) or split-f16 (tier 2) tower with every field its launcher reads as given (tests/test_gpu_tier_gemm_kernels.py):
// ldc != N and the two-pass form on any shape.  No logic of its own: what launch_gemm refuses is refused.
extern "C" int grip_debug_gemm_tier(int tier, int w_exact, int epi, const void* A, const void* W, int M, int N, int K, int ldc, const float* bias, const void* resid,
                                    void* out, void* out2, float scalar, int64_t m_pad, void* stream) {
    GemmArgs a{};
    a.f32 = tier; a.w_exact = w_exact;
    a.A = A; a.W = W; a.M = M; a.N = N; a.K = K; a.ldc = ldc; a.m_pad = m_pad; a.bias = bias; a.resid = resid; a.out = out; a.out2 = out2; a.scalar = scalar;
    return launch_gemm(epi, a, (hipStream_t)stream);
}
// Weight image of the split-f16 tier as grip_tower_finalize builds it: W [rows, K] f32 -> the split layout (x SP1_W_SCALE), with dup != 0 then rewritten in
// place as the duplicated image; flags_out[0] = overflow, flags_out[1] = some element is no f16 number.
extern "C" int grip_debug_split_weights(const float* W, void* image, int64_t rows, int K, int dup, int* flags_out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int* flag = nullptr;
    GRIP_CHECK_HIP(hipMalloc((void**)&flag, 2 * sizeof(int)));
    int rc = hipMemsetAsync(flag, 0, 2 * sizeof(int), s) == hipSuccess ? launch_split_rows(W, image, rows, K, K, s, 1, flag, flag + 1) : GRIP_ERR_HIP;
    if (!rc && dup) rc = launch_split_dup_weights(image, image, rows, K, s);
    if (!rc && (hipMemcpyAsync(flags_out, flag, 2 * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)) {
        grip_set_error("debug_split_weights: HIP error");
        rc = GRIP_ERR_HIP;
    }
    (void)hipFree(flag);
    return rc;
}
// Attention of a precision-2 tower: qkv f32 -> out in the split layout (4 bytes per element); mfma != 0: attention_split.hip (S <= 320), else the
// f32 vector-ALU kernel with split output
extern "C" int grip_debug_attention_split(const void* qkv, void* out, int B, int S, int H, int causal, int mfma, void* stream) {
    if (mfma) return launch_attention_fwd_split((const float*)qkv, out, B, S, H, causal, (hipStream_t)stream);
    return launch_attention_fwd_f32((const float*)qkv, (float*)out, B, S, H, causal, (hipStream_t)stream, 1);
}
extern "C" int grip_debug_attention_exact(const void* qkv, void* out, int B, int S, int H, int causal, void* stream) {
    return launch_attention_fwd_f32((const float*)qkv, (float*)out, B, S, H, causal, (hipStream_t)stream);
}
extern "C" int grip_debug_attention(const void* qkv, void* out, int B, int S, int H, int causal, void* stream) {
    return launch_attention_fwd((const half_t*)qkv, (half_t*)out, B, S, H, causal, (hipStream_t)stream);
}
// the shared-prefix row layout (common.h seq_row) and the one-row kernels of the last block, through the launchers the towers call
extern "C" int grip_debug_attention_shared(const void* qkv, void* out, int B, int S, int H, int shared_rows, void* stream) {
    return launch_attention_fwd((const half_t*)qkv, (half_t*)out, B, S, H, 1, (hipStream_t)stream, shared_rows);
}
extern "C" int grip_debug_attention_row(const void* qkv, const void* qrows, const int32_t* row_index, void* out, int B, int S, int H, int causal, int train,
                                        void* stream) {
    return launch_attention_row((const half_t*)qkv, (const half_t*)qrows, row_index, (half_t*)out, B, S, H, causal, (hipStream_t)stream, train);
}
extern "C" int grip_debug_attention_row_exact(const void* qkv, const void* qrows, const int32_t* row_index, void* out, int B, int S, int H, int causal,
                                              int split_out, void* stream) {
    return launch_attention_row_f32((const float*)qkv, (const float*)qrows, row_index, (float*)out, B, S, H, causal, (hipStream_t)stream, split_out);
}
extern "C" int grip_debug_layernorm(const float* x, const float* gamma, const float* beta, void* out, int M, int d, void* stream) {
    return launch_layernorm_f16_from_f32(x, gamma, beta, (half_t*)out, M, d, (hipStream_t)stream);
}
// The backward row kernels (csrc/rowops_bwd.hip) through their launchers (tests/test_gpu_rowops_bwd.py).  x f16, everything else f32; dxh f16.
extern "C" int grip_debug_ln_bwd_add(const void* x, const float* dln, int parts, int64_t part_stride, const float* gamma, float* dx, void* dxh, int M, int d,
                                     void* stream) {
    return launch_ln_bwd_add((const resid_t*)x, dln, parts, part_stride, gamma, dx, (half_t*)dxh, M, d, (hipStream_t)stream);
}
extern "C" int grip_debug_ln_bwd_init(const void* x, const float* dln, int parts, int64_t part_stride, const float* gamma, const float* rows_add,
                                      const int32_t* index, int stride, float* dx, void* dxh, int M, int d, void* stream) {
    return launch_ln_bwd_init((const resid_t*)x, dln, parts, part_stride, gamma, rows_add, index, stride, dx, (half_t*)dxh, M, d, (hipStream_t)stream);
}
// fill = 0: ln_bwd_scatter (writes the n read rows only; first and M unused), fill = 1: ln_bwd_scatter_fill (writes every row r < M)
extern "C" int grip_debug_ln_bwd_scatter(const void* x, const float* dy, const int32_t* index, int stride, int first, const float* gamma, float* dx, void* dxh,
                                         int n, int M, int d, int fill, void* stream) {
    if (fill) return launch_ln_bwd_scatter_fill((const resid_t*)x, dy, index, stride, first, gamma, dx, (half_t*)dxh, n, M, d, (hipStream_t)stream);
    return launch_ln_bwd_scatter((const resid_t*)x, dy, index, stride, gamma, dx, (half_t*)dxh, n, d, (hipStream_t)stream);
}
// mode 0: shared prompts (prefix [P, d]), 1: per-image prompts (prefix and grad [B, P, d]), 2: a deep prompt's slice (no LayerNorm; zeroes the rows read in dx and dxh)
extern "C" int grip_debug_vit_prefix_grad(float* dx, void* dxh, const float* prefix, const float* gamma, const float* scale, float* grad, int B, int S, int P,
                                          int d, int mode, void* stream) {
    if (mode == 0) return launch_vit_prefix_grad(dx, prefix, gamma, scale, grad, B, S, P, d, (hipStream_t)stream);
    if (mode == 1) return launch_vit_prefix_grad_per_image(dx, prefix, gamma, scale, grad, B, S, P, d, (hipStream_t)stream);
    return launch_vit_deep_grad(dx, (half_t*)dxh, scale, grad, B, S, P, d, (hipStream_t)stream);
}
// deep = 0: text_prefix_grad (dxh unused), 1: text_deep_grad (zeroes the rows summed in dx and dxh)
extern "C" int grip_debug_text_prefix_grad(float* dx, void* dxh, const float* scale, float* grad, int C, int T, int P, int prefix_classes, int d, int deep,
                                           void* stream) {
    if (deep) return launch_text_deep_grad(dx, (half_t*)dxh, scale, grad, C, T, P, prefix_classes, d, (hipStream_t)stream);
    return launch_text_prefix_grad(dx, scale, grad, C, T, P, prefix_classes, d, (hipStream_t)stream);
}
extern "C" int grip_debug_grad_scale_cast(const float* g, void* g16, float* scale, int n, void* stream) {
    return launch_grad_scale_cast(g, (half_t*)g16, scale, n, (hipStream_t)stream);
}
// The forward row kernels (csrc/rowops.hip) through their launchers (tests/test_gpu_rowops_fwd.py).
extern "C" int grip_debug_layernorm_modes(const void* x, const int32_t* row_index, int row_stride, const float* gamma, const float* beta, void* out, int f32,
                                          int gather, int M, int d, void* stream) {
    if (gather) return launch_gather_ln_f16(x, row_index, row_stride, gamma, beta, out, f32, M, d, (hipStream_t)stream);
    return launch_layernorm_f16(x, gamma, beta, out, f32, M, d, (hipStream_t)stream);
}
extern "C" int grip_debug_vit_assemble(const float* patch_out, const float* cls, const float* pos, const float* prefix, int P, const float* gamma, const float* beta,
                                       void* x, int f32, float* rowstat, int B, int G2, int d, void* x_lo, int per_image, void* stream) {
    return launch_vit_assemble_ln(patch_out, cls, pos, prefix, P, gamma, beta, x, f32, rowstat, B, G2, d, (hipStream_t)stream, (half_t*)x_lo, per_image);
}
// text = 0: launch_vit_deep_insert; else launch_text_deep_insert with B classes
extern "C" int grip_debug_deep_insert(const float* deep, int prefix_classes, void* x, int f32, void* x_lo, float* stat_part, float* rowstat, int B, int S, int P,
                                      int shared_rows, int M, int d, int text, void* stream) {
    if (text) return launch_text_deep_insert(deep, prefix_classes, x, f32, stat_part, rowstat, B, S, P, shared_rows, M, d, (hipStream_t)stream);
    return launch_vit_deep_insert(deep, x, f32, (half_t*)x_lo, stat_part, rowstat, B, S, P, M, d, (hipStream_t)stream);
}
extern "C" int grip_debug_text_embed(const int32_t* ids, int ld_ids, const float* tok_emb, const float* pos, const float* prefix, int P, int prefix_classes, void* x,
                                     int f32, float* rowstat, int C, int T, int d, int vocab, int shared_rows, void* stream) {
    return launch_text_embed(ids, ld_ids, tok_emb, pos, prefix, P, prefix_classes, x, f32, rowstat, C, T, d, vocab, (hipStream_t)stream, shared_rows);
}
extern "C" int grip_debug_patch_gather(const void* images, int images_f16, void* out, int out_f32, int B, int R, int patch, int Kpad, void* stream) {
    return launch_im2col(images, images_f16, out, out_f32, B, R, patch, Kpad, (hipStream_t)stream);
}
extern "C" int grip_debug_transpose(const void* in, void* out, int f32, int rows, int cols, int ld_in, void* stream) {
    return launch_transpose(in, out, f32, rows, cols, ld_in, (hipStream_t)stream);
}
extern "C" int grip_debug_gather_rows(const void* x, const int32_t* row_index, int row_stride, void* out, int n_rows, int d, int four_byte, void* stream) {
    if (four_byte) return launch_gather_rows4(x, row_index, row_stride, out, n_rows, d, (hipStream_t)stream);
    return launch_gather_rows((const half_t*)x, row_index, row_stride, (half_t*)out, n_rows, d, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------- backward
// Input-gradient chain of one tower down to its prompt slice.  Enters with dx / dxh holding the
// (loss-scaled) gradient w.r.t. the final residual stream, leaves with dx = gradient w.r.t. x0.
// grad_deep (deep visual prompts, w.n_deep > 0): [n_deep, P, d]; before block l's backward, dx / dxh hold the gradient of x_in[l + 1], whose rows
// 1 .. P the forward overwrote with deep[l] when l + 1 <= n_deep: their batch sum is grad_deep[l], and they are zeroed (nothing flows below).
// Text tower: [n_deep, deep_classes, P, d], the class sum for one shared context, each class's own rows otherwise.  In the shared-prefix layout the
// classes' shares have already met in the shared rows (attention_bwd's kv_part reduction), so the slice runs as one sequence.
static int run_blocks_backward(grip_tower* t, Workspace& w, int causal, const int32_t* read_rows, hipStream_t s, float* grad_deep = nullptr) {
    const int d = t->D.width, H = t->D.heads;
    const half_t* W = t->w16;
    const float* F = t->w32;
    const int64_t part = (int64_t)w.Mp * d;       // floats between split-K partial buffers in w.dln
    for (int l = t->D.layers - 1; l >= 0; --l) {
        const LayerW& lw = t->L.layer[(size_t)l];
        if (grad_deep && l + 1 <= w.n_deep) {
            if (t->D.kind == 0)
                LAUNCH(launch_vit_deep_grad(w.dx, w.dxh, w.scale, grad_deep + (size_t)l * w.P * d, w.batch, w.S, w.P, d, s));
            else
                LAUNCH(launch_text_deep_grad(w.dx, w.dxh, w.scale, grad_deep + (size_t)l * w.deep_classes * w.P * d, w.Ps ? 1 : w.batch, w.S, w.P, w.deep_classes, d, s));
        }
        if (l + 1 == t->D.layers && w.rows_last) {
            // the last block ran for the read rows only (run_blocks): enters with drow / drow_h = the gradient of those stream rows
            const int64_t Bp = round_up64(w.batch, 256);
            const int64_t rpart = Bp * d;
            GemmArgs a{};
            a.A = w.drow_h; a.W = W + lw.proj_wT; a.M = w.batch; a.m_pad = Bp; a.N = 4 * d; a.K = d; a.aux = w.row_hpre; a.out = w.row_dh; a.ldc = 4 * d;
            LAUNCH(launch_gemm(EPI_GELUGRAD_F16, a, s));
            a = GemmArgs{};
            a.A = w.row_dh; a.W = W + lw.fc_wT; a.M = w.batch; a.m_pad = Bp; a.N = d; a.K = 4 * d; a.out = w.row_dln; a.ldc = d;
            a.ksplit = w.ks_row; a.split_stride = rpart;
            LAUNCH(launch_gemm(EPI_F32, a, s));
            LAUNCH(launch_ln_bwd_add(w.row_xmid, w.row_dln, w.ks_row, rpart, F + lw.ln2_g, w.drow, w.drow_h, w.batch, d, s));
            a = GemmArgs{};
            a.A = w.drow_h; a.W = W + lw.out_wT; a.M = w.batch; a.m_pad = Bp; a.N = d; a.K = d; a.out = w.row_datt; a.ldc = d;
            LAUNCH(launch_gemm(EPI_F16, a, s));
            // d(q, k, v) of every row from the read rows' d(attention output): rank-one in (q, dO) per head
            LAUNCH(launch_attention_row_bwd(w.qkv_l[(size_t)l], w.row_att, w.row_datt, read_rows, w.dqkv, w.batch, w.S, H, causal, s));
            a = GemmArgs{};
            a.rot_rows = 1;
            a.A = w.dqkv; a.W = W + lw.in_wT; a.M = w.M; a.m_pad = w.Mp; a.N = d; a.K = 3 * d; a.out = w.dln; a.ldc = d;
            a.ksplit = w.ks_in; a.split_stride = part;
            LAUNCH(launch_gemm(EPI_F32, a, s));
            // the stream gradient entering the block: drow at the read rows, zero elsewhere (no fill, no scatter)
            LAUNCH(launch_ln_bwd_init(w.x_in[(size_t)l], w.dln, w.ks_in, part, F + lw.ln1_g, w.drow, read_rows, w.S, w.dx, w.dxh, w.M, d, s));
            continue;
        }
        GemmArgs a{};
        a.rot_rows = 1;           // (backward GEMMs: train mode by definition)
        // d(pre-activation) = (dx @ W_proj) * quickgelu'(h_pre)
        a.A = w.dxh; a.W = W + lw.proj_wT; a.M = w.M; a.m_pad = w.Mp; a.N = 4 * d; a.K = d; a.aux = w.hpre_l[(size_t)l]; a.out = w.dh; a.ldc = 4 * d;
        LAUNCH(launch_gemm(EPI_GELUGRAD_F16, a, s));
        a = GemmArgs{};
        a.rot_rows = 1;
        a.A = w.dh; a.W = W + lw.fc_wT; a.M = w.M; a.m_pad = w.Mp; a.N = d; a.K = 4 * d; a.out = w.dln; a.ldc = d;
        a.ksplit = w.ks_fc; a.split_stride = part;
        LAUNCH(launch_gemm(EPI_F32, a, s));
        LAUNCH(launch_ln_bwd_add(w.x_mid[(size_t)l], w.dln, w.ks_fc, part, F + lw.ln2_g, w.dx, w.dxh, w.M, d, s));
        a = GemmArgs{};
        a.rot_rows = 1;
        a.A = w.dxh; a.W = W + lw.out_wT; a.M = w.M; a.m_pad = w.Mp; a.N = d; a.K = d; a.out = w.datt; a.ldc = d;
        LAUNCH(launch_gemm(EPI_F16, a, s));
        LAUNCH(launch_attention_bwd(w.qkv_l[(size_t)l], w.att_l[(size_t)l], w.datt, w.dqkv, w.batch, w.S, H, causal, s, w.Ps, w.kv_part));
        a = GemmArgs{};
        a.rot_rows = 1;
        a.A = w.dqkv; a.W = W + lw.in_wT; a.M = w.M; a.m_pad = w.Mp; a.N = d; a.K = 3 * d; a.out = w.dln; a.ldc = d;
        a.ksplit = w.ks_in; a.split_stride = part;
        LAUNCH(launch_gemm(EPI_F32, a, s));
        LAUNCH(launch_ln_bwd_add(w.x_in[(size_t)l], w.dln, w.ks_in, part, F + lw.ln1_g, w.dx, w.dxh, w.M, d, s));
    }
    return GRIP_OK;
}

static int backward_head_of_tower(grip_tower* t, Workspace& w, const float* grad_emb, const int32_t* index, hipStream_t s) {
    const grip_dims& D = t->D;
    const int d = D.width;
    // scale + f16 cast of dL/d(emb); d(ln output) = g @ proj^T  (W = proj [d, E] as stored: N = d, K = E)
    LAUNCH(launch_grad_scale_cast(grad_emb, w.gemb16, w.scale, w.batch * D.embed_dim, s));
    GemmArgs a{};
    a.A = w.gemb16; a.W = t->w16 + t->L.proj; a.M = w.batch; a.N = d; a.K = D.embed_dim; a.out = w.dcls; a.ldc = d;
    LAUNCH(launch_gemm(EPI_F32, a, s));
    if (w.rows_last) {    // compact: the final stream exists for the read rows only (run_blocks)
        LAUNCH(launch_ln_bwd_scatter(w.row_xout, w.dcls, nullptr, 1, t->w32 + t->L.lnpost_g, w.drow, w.drow_h, w.batch, d, s));
        return GRIP_OK;
    }
    // row of (sequence b, position index[b]): b * rs + index[b] in either layout (shared-prefix: Ps + b*(S-Ps) + index - Ps); every other row of the
    // stream gradient starts at zero (written by the same kernel)
    LAUNCH(launch_ln_bwd_scatter_fill(w.x_in[(size_t)D.layers], w.dcls, index, w.rs, w.Ps, t->w32 + t->L.lnpost_g, w.dx, w.dxh, w.batch, (int)w.M, d, s));
    return GRIP_OK;
}

// Finds the pending train-mode forward of `workspace`.  generation != 0 must equal the number that forward handed out: a later
// train-mode forward on the same workspace has overwritten the activations, and the gradients would silently be those of
// the wrong forward.  The entry is marked consumed (one backward per forward) and stays until the workspace's next forward.
static int check_bwd(grip_tower* t, void* workspace, size_t workspace_bytes, uint64_t generation, grip_tower::TrainState& st) {
    GRIP_REQUIRE(t && workspace, "backward: null pointer");
    auto it = t->pending.find(workspace);
    if (it == t->pending.end() || !it->second.w.train) {
        grip_set_error("backward without a matching train-mode forward on this workspace");
        return GRIP_ERR_STATE;
    }
    if (generation != 0 && it->second.generation != generation) {
        grip_set_error("backward: the activations of forward #%llu were overwritten by forward #%llu on the same workspace "
                       "(two train-mode forwards before a backward need two workspaces)",
                       (unsigned long long)generation, (unsigned long long)it->second.generation);
        return GRIP_ERR_STATE;
    }
    if (it->second.consumed) {      // kept until the workspace's next forward so that this is not reported as "no matching forward"
        grip_set_error("backward: forward #%llu has already been back-propagated (one backward per forward: the backward works in place on the "
                       "saved activations, so retain_graph / a second backward needs a second forward)", (unsigned long long)it->second.generation);
        return GRIP_ERR_STATE;
    }
    if (it->second.w.bytes > workspace_bytes) { grip_set_error("backward: workspace too small"); return GRIP_ERR_WORKSPACE; }
    st = it->second;
    it->second.consumed = true;
    return GRIP_OK;
}

extern "C" int grip_vit_backward_prefix(grip_tower* t, const float* grad_emb, const float* prefix, float* grad_prefix,
                                        void* workspace, size_t workspace_bytes, uint64_t generation, void* stream) {
    PassScope pass_scope;
    try {
        GRIP_REQUIRE(t && t->D.kind == 0 && grad_emb && prefix && grad_prefix, "vit_backward_prefix: bad arguments");
        auto it = t->pending.find(workspace);
        if (it != t->pending.end() && it->second.n_deep > 0 && !it->second.consumed) {
            grip_set_error("vit_backward_prefix: the forward on this workspace ran with %d deep prompts: its backward is grip_vit_backward_deep", it->second.n_deep);
            return GRIP_ERR_STATE;
        }
        grip_tower::TrainState st;
        RUN(check_bwd(t, workspace, workspace_bytes, generation, st));
        Workspace& w = st.w;
        GRIP_REQUIRE(w.P > 0, "vit_backward_prefix: forward had no prompt tokens");
        hipStream_t s = (hipStream_t)stream;
        RUN(backward_head_of_tower(t, w, grad_emb, nullptr, s));
        RUN(run_blocks_backward(t, w, 0, nullptr, s));
        if (st.per_image)     // one prompt per image: grad_prefix [batch, n_prefix, width], image b's rows only
            LAUNCH(launch_vit_prefix_grad_per_image(w.dx, prefix, t->w32 + t->L.lnpre_g, w.scale, grad_prefix, w.batch, w.S, w.P, t->D.width, s));
        else
            LAUNCH(launch_vit_prefix_grad(w.dx, prefix, t->w32 + t->L.lnpre_g, w.scale, grad_prefix, w.batch, w.S, w.P, t->D.width, s));
        return GRIP_OK;
    } catch (...) { grip_set_error("vit_backward_prefix: exception"); return GRIP_ERR_ARG; }
}

extern "C" int grip_vit_backward_deep(grip_tower* t, const float* grad_emb, const float* prefix, float* grad_prefix, float* grad_deep,
                                      void* workspace, size_t workspace_bytes, uint64_t generation, void* stream) {
    PassScope pass_scope;
    try {
        GRIP_REQUIRE(t && t->D.kind == 0 && grad_emb && prefix && grad_prefix, "vit_backward_deep: bad arguments");
        auto it = t->pending.find(workspace);
        GRIP_REQUIRE(it == t->pending.end() || it->second.n_deep == 0 || grad_deep, "vit_backward_deep: null grad_deep (the forward ran with %d deep prompts)",
                     it == t->pending.end() ? 0 : it->second.n_deep);
        grip_tower::TrainState st;
        RUN(check_bwd(t, workspace, workspace_bytes, generation, st));
        Workspace& w = st.w;
        GRIP_REQUIRE(w.P > 0, "vit_backward_deep: forward had no prompt tokens");
        hipStream_t s = (hipStream_t)stream;
        RUN(backward_head_of_tower(t, w, grad_emb, nullptr, s));
        RUN(run_blocks_backward(t, w, 0, nullptr, s, st.n_deep ? grad_deep : nullptr));
        if (st.per_image)
            LAUNCH(launch_vit_prefix_grad_per_image(w.dx, prefix, t->w32 + t->L.lnpre_g, w.scale, grad_prefix, w.batch, w.S, w.P, t->D.width, s));
        else
            LAUNCH(launch_vit_prefix_grad(w.dx, prefix, t->w32 + t->L.lnpre_g, w.scale, grad_prefix, w.batch, w.S, w.P, t->D.width, s));
        return GRIP_OK;
    } catch (...) { grip_set_error("vit_backward_deep: exception"); return GRIP_ERR_ARG; }
}

// (who: the entry point's name for the messages; grad_deep is only read when the forward ran with deep prompts)
static int text_backward(const char* who, grip_tower* t, const float* grad_emb, float* grad_prefix, float* grad_deep,
                         void* workspace, size_t workspace_bytes, uint64_t generation, void* stream) {
    PassScope pass_scope;
    GRIP_REQUIRE(t && t->D.kind == 1 && grad_emb && grad_prefix, "%s: bad arguments", who);
    grip_tower::TrainState st;
    RUN(check_bwd(t, workspace, workspace_bytes, generation, st));
    Workspace& w = st.w;
    GRIP_REQUIRE(w.P > 0, "%s: forward had no prompt tokens", who);
    hipStream_t s = (hipStream_t)stream;
    RUN(backward_head_of_tower(t, w, grad_emb, st.eot, s));
    RUN(run_blocks_backward(t, w, 1, st.eot, s, st.n_deep ? grad_deep : nullptr));
    if (w.Ps)   // shared-prefix layout: every class's share already met in the shared rows (rows 1 .. P)
        LAUNCH(launch_text_prefix_grad(w.dx, w.scale, grad_prefix, 1, w.S, w.P, 1, t->D.width, s));
    else
        LAUNCH(launch_text_prefix_grad(w.dx, w.scale, grad_prefix, w.batch, w.S, w.P, st.prefix_classes, t->D.width, s));
    return GRIP_OK;
}

extern "C" int grip_text_backward_prefix(grip_tower* t, const float* grad_emb, float* grad_prefix,
                                         void* workspace, size_t workspace_bytes, uint64_t generation, void* stream) {
    try {
        if (t && t->D.kind == 1) {
            auto it = t->pending.find(workspace);
            if (it != t->pending.end() && it->second.n_deep > 0 && !it->second.consumed) {
                grip_set_error("text_backward_prefix: the forward on this workspace ran with %d deep prompts: its backward is grip_text_backward_deep", it->second.n_deep);
                return GRIP_ERR_STATE;
            }
        }
        return text_backward("text_backward_prefix", t, grad_emb, grad_prefix, nullptr, workspace, workspace_bytes, generation, stream);
    } catch (...) { grip_set_error("text_backward_prefix: exception"); return GRIP_ERR_ARG; }
}

extern "C" int grip_text_backward_deep(grip_tower* t, const float* grad_emb, float* grad_prefix, float* grad_deep,
                                       void* workspace, size_t workspace_bytes, uint64_t generation, void* stream) {
    try {
        if (t && t->D.kind == 1) {
            auto it = t->pending.find(workspace);
            GRIP_REQUIRE(it == t->pending.end() || it->second.n_deep == 0 || grad_deep, "text_backward_deep: null grad_deep (the forward ran with %d deep prompts)",
                         it == t->pending.end() ? 0 : it->second.n_deep);
        }
        return text_backward("text_backward_deep", t, grad_emb, grad_prefix, grad_deep, workspace, workspace_bytes, generation, stream);
    } catch (...) { grip_set_error("text_backward_deep: exception"); return GRIP_ERR_ARG; }
}

extern "C" int grip_debug_attention_bwd(const void* qkv, const void* o, const void* d_out, void* dqkv, int B, int S, int H, int causal, void* stream) {
    return launch_attention_bwd((const half_t*)qkv, (const half_t*)o, (const half_t*)d_out, (half_t*)dqkv, B, S, H, causal, (hipStream_t)stream);
}
extern "C" int grip_debug_attention_bwd_shared(const void* qkv, const void* o, const void* d_out, void* dqkv, float* kv_part, int B, int S, int H, int shared_rows,
                                               void* stream) {
    return launch_attention_bwd((const half_t*)qkv, (const half_t*)o, (const half_t*)d_out, (half_t*)dqkv, B, S, H, 1, (hipStream_t)stream, shared_rows, kv_part);
}
extern "C" int grip_debug_attention_row_bwd(const void* qkv, const void* o_rows, const void* do_rows, const int32_t* row_index, void* dqkv, int B, int S, int H,
                                            int causal, void* stream) {
    return launch_attention_row_bwd((const half_t*)qkv, (const half_t*)o_rows, (const half_t*)do_rows, row_index, (half_t*)dqkv, B, S, H, causal, (hipStream_t)stream);
}
