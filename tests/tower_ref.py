"""The launches of a tower pass (csrc/tower.hip) in order, each mapped to the float64 reference of its operation and the derived bound on
|kernel - value| per element ("Tower pass tests").  Plain torch; nothing here calls the library.

steps(p) returns, for a pass description p (class Pass), one Step per kernel launch:
  label   block and operation, "b1.qkv"
  call    how the stringified launch begins that the launch budget names (grip_debug_launch_budget), "launch_gemm(EPI_LNFOLD_F16"
  reads   the buffers the launch reads
  owns    the regions it may write, Region(slot, rows, ld, col0, ncols): `rows` rows of `ld` elements from the start of the slot, columns col0 .. col0 + ncols
  ref     ref(before, after, fault=None) -> {name: (got, value, bound)}: `value` is float64 of the operation on the buffers `before` the launch as the
          kernel reads them, `got` what the launch left in `after` (a region, or a quantity derived from two: hi + lo of a compensated stream)
  exact   exact(before) -> {Region: tensor}, the outputs that are determined in bits (gathers, im2col, f16 copies of f32 inputs), or None
  emu     emu(before) -> {Region: tensor}: the same operation in float32 arithmetic with the tower's f16 stores, a CPU stand-in for the kernel
          (tests/test_host_tower_ref.py: the float32 chain stays inside every bound, every fault leaves it)

A buffer set (`before`, `after`) maps a slot name to a FLAT tensor in the slot's storage type: the workspace slots by the names
grip_debug_tower_slot reports, "out:emb", the call's arguments "in:images" / "in:prefix" / "in:deep" / "in:ids" / "in:eot", and the weights
"w:<name of grip_layout_slot>" as [rows, ld] tensors.  In the float64 chain of the host test every tensor is float64 and nothing is rounded.

The map is written from the model's equations (pre-LN blocks x += out_proj(MHSA(ln_1 x)); x += c_proj(QuickGELU(c_fc(ln_2 x))), CLS / EOT read rows,
ln_post, projection) and DESIGN.md: the statistics travel with the stream (section 4: ln_1 / ln_2 folded into the QKV / c_fc GEMMs,
y = rstd (x W'^T - mean colsum(W')) + (W beta + b), W' = f16(gamma o W); each residual epilogue emits per-tile (sum, sum of squares) of the values it
stores, ln_stats_finalize turns them into (mean, rstd)); the last block of an inference pass runs K and V for every row and everything else for the
read row of each sequence alone; the shared-prefix layout holds positions 0 .. P once; deep prompts replace rows 1 .. P of the input of blocks
1 .. n_deep.

Bounds come from the reference modules (gemm_ref, attention_ref, rowops_fwd_ref) with their counting rules, u = 2^-24, h = 2^-11, q = 2^-25.  The
launches that had no bound yet are exact: im2col and the deep rows are f16 roundings of f32 inputs (bit-equal to torch's rounding), the row gathers
copy bits.  Nothing in a bound is measured.

This module covers the inference passes of the f16 towers (folded LayerNorm, read-rows-only last block, compensated stream, shared-prefix layout,
deep and per-image prompts), of the exact f32 tower and the split-f16 tower (_steps_f32) and the train-mode forwards of the f16 towers (per-layer saves,
partial statistics read by the consumer, the compact last block, cooperative split-K), and -- backward_steps -- the backward of every train-mode forward
down to grad_prefix and grad_deep.  `fault` names ONE deliberate error
applied to the value (never to the bound): FAULT_SITES.

A train-mode folded GEMM of block l >= 1 reads the partial sums its producer took from unrounded values, while the saved stream holds their f16
rounding.  No allowance for that rounding is needed here: a step's reference is evaluated on the buffers as they stood when the launch ran, and
stat_part then still holds the very sums the kernel read (`stat_in` of gemm_ref)."""
from collections import namedtuple

import torch

import attention_ref as AR
import gemm_ref as G
import rowops_fwd_ref as FR

Region = namedtuple("Region", "slot rows ld col0 ncols row0", defaults=(0,))          # rows row0 .. row0 + rows of pitch ld, columns col0 .. col0 + ncols
Step = namedtuple("Step", "label call reads owns ref exact emu")
F16_SLOTS = ("x", "x_lo", "xn", "qkv", "att", "h", "cls16", "row_x", "row_x_lo", "row_att", "row_xn", "row_h", "patches")
F16_SLOTS += ("x_in", "x_mid", "qkv_l", "att_l", "hpre_l", "row_hpre", "row_xmid", "row_xout")          # train mode; per-layer slots are "<name>.<layer>"
F16_SLOTS += ("dxh", "dh", "dqkv", "datt", "gemb16", "drow_h", "row_dh", "row_datt")          # the backward's f16 scratch
F32_SLOTS = ("stat_part", "rowstat", "patch_out", "out:emb", "coop_scratch", "coop_cnt", "dx", "dln", "dcls", "scale", "kv_part", "drow", "row_dln",
             "out:grad_prefix", "out:grad_deep")          # (coop_cnt holds ints: zero is zero in either reading)


def f16slot(slot):
    return slot.split(".")[0] in F16_SLOTS


class Pass:
    """One forward pass of a tower.  kind 0 vision (batch images, S = 1 + P + G2), 1 text (batch classes, S = seq_len, eot [batch]); precision 0 the f16
    tower (inference, or train = True), 1 the exact f32 tower (inference)."""

    def __init__(self, kind, width, layers, embed_dim, batch, P=0, resolution=32, patch=8, vocab=0, seq0=0, seq_len=0, eot=None, prefix_classes=1,
                 n_deep=0, hilo=False, no_pos=False, per_image=False, shared=False, precision=0, train=False, coop_ks=1, w_grid=False):
        # 1: the exact tower, every activation f32, literal LayerNorm (inference only).  2: the split-f16 tower: the same pass with the four block GEMMs and
        # the attention on split operands (hi = f16(x), lo = f16(x - hi)); their A operands (LayerNorm output, attention output, MLP hidden) live in the
        # split layout.  w_grid: every block weight is an f16 number, so grip_tower_finalize picks the two-pass form (w_exact = 1)
        self.precision, self.f32, self.split, self.w_grid = precision, precision != 0, precision == 2, w_grid
        self.coop_ks = coop_ks      # text tower, train: what grip_debug_coop_split(M, d, 4 d) gives (asserted against the library by the tests)
        self.train = train          # GRIP_FWD_TRAIN: every block saves what its backward needs (x_in, x_mid, qkv_l, att_l, hpre_l per layer)
        self.kind, self.d, self.layers, self.E, self.B, self.P = kind, width, layers, embed_dim, batch, P
        self.H = width // 64
        self.resolution, self.patch, self.vocab = resolution, patch, vocab
        self.n_deep, self.hilo, self.no_pos, self.per_image = n_deep, hilo, no_pos, per_image
        self.prefix_classes = prefix_classes
        if kind == 0:
            self.G2 = (resolution // patch) ** 2
            self.seq0 = self.G2 + 1
            self.S = self.seq0 + P
            self.kpad = (3 * patch * patch + 63) // 64 * 64
            self.eot = None
            shared = False
        else:
            self.seq0 = seq0
            self.S = seq_len or seq0
            self.eot = list(eot)
            shared = bool(shared and P > 0 and prefix_classes == 1 and not precision)
        self.Ps = P + 1 if shared else 0
        self.rs = self.S - self.Ps
        self.M = self.Ps + batch * self.rs
        self.causal = kind
        # the last block runs for the read rows alone unless the rows of a sequence are not contiguous (shared-prefix layout)
        self.rows_only = not self.Ps
        assert not (train and (hilo or precision)), "train mode: the f16 towers, no compensated stream"

    def key(self):
        tier = "split.grid." if (self.split and self.w_grid) else "split." if self.split else "f32." if self.f32 else "train." if self.train else ""
        t = tier + f"text.C{self.B}.P{self.P}.pc{self.prefix_classes}.T{self.S}" if self.kind else tier + f"vit.B{self.B}.P{self.P}"
        t += f".d{self.d}.coop{self.coop_ks}" if self.coop_ks > 1 else ""
        return t + (".shared" if self.Ps else "") + (".hilo" if self.hilo else "") + (".nopos" if self.no_pos else "") + \
            (".perimage" if self.per_image else "") + (f".deep{self.n_deep}" if self.n_deep else "")

    def read_rows(self, dev="cpu"):
        """Stream row of the read position of each sequence: CLS, or the EOT position, in either row layout."""
        pos = torch.zeros(self.B, dtype=torch.long) if self.kind == 0 else torch.tensor(self.eot, dtype=torch.long)
        return (torch.arange(self.B) * self.rs + pos).to(dev)          # shared layout: Ps + b (S - Ps) + (pos - Ps)

    def is16(self, slot):
        return not self.f32 and f16slot(slot)

    def split_layout(self, r):
        """The region holds the split layout (split-f16 tower): 4-byte elements that are pairs of f16, meaningless read as f32."""
        return self.split and (r.slot, r.ld) in {("xn", self.d), ("att", self.d), ("h", 4 * self.d), ("row_xn", self.d), ("row_att", self.d), ("row_h", 4 * self.d)}

    def lw(self, l, name):
        return f"w:transformer.resblocks.{l}.{name}"

    def final(self, name):
        return "w:" + (("ln_post." if self.kind == 0 else "ln_final.") + name if name in ("weight", "bias") else name)


# ------------------------------------------------------------------------------------------------ buffers
def view(bufs, r):
    return bufs[r.slot][r.row0 * r.ld:(r.row0 + r.rows) * r.ld].view(r.rows, r.ld)[:, r.col0:r.col0 + r.ncols]


def is64(bufs):
    return bufs["w:positional_embedding"].dtype == torch.float64


def store(value, slot, like64):
    """A float32 / float64 value as the tower stores it in `slot` (the float64 chain rounds nothing)."""
    if like64:
        return value.double()
    return value.float().half() if f16slot(slot) else value.float()


def _h(ref, e):
    return e + FR.half_bound(ref, e)


def _deep_rows(p, bufs, l):
    """(stream rows, source rows [n, d]) of the deep prompt entering block l, 1 <= l <= n_deep."""
    d, P = p.d, p.P
    if p.kind == 0:
        deep = bufs["in:deep"].view(p.n_deep, P, d)[l - 1]
        rows = (torch.arange(p.B)[:, None] * p.S + 1 + torch.arange(P)[None]).reshape(-1)
        return rows, deep.repeat(p.B, 1)
    deep = bufs["in:deep"].view(p.n_deep, p.prefix_classes, P, d)[l - 1]
    if p.Ps:
        return 1 + torch.arange(P), deep[0]
    rows = (torch.arange(p.B)[:, None] * p.S + 1 + torch.arange(P)[None]).reshape(-1)
    return rows, (deep if p.prefix_classes == p.B else deep.expand(p.B, P, d)).reshape(-1, d)


# ------------------------------------------------------------------------------------------------ float32 stand-ins of the kernels
def _emu_acc(A, W, bias=None):
    acc = A.float() @ W.float().T
    return acc if bias is None else acc + bias.float()


def _emu_fold(A, W, bias, cs, stat):
    return (_emu_acc(A, W) - cs.float() * stat[:, :1].float()) * stat[:, 1:].float() + bias.float()


def _emu_gelu(y):
    return y * torch.sigmoid(y * 1.702)


def _emu_ln(x, g, b):
    x = x.float()
    c = x - x.mean(-1, keepdim=True)
    return c * ((c * c).mean(-1, keepdim=True) + FR.LN_EPS).rsqrt() * g.float() + b.float()


def _emu_onepass(s1, s2, d):
    mean = s1 / d
    var = (s2 / d - mean * mean).clamp_min(0)
    return torch.cat([mean, (var + FR.LN_EPS).rsqrt()], -1)


def _emu_tiles(v):
    M, N = v.shape
    t = v.reshape(M, N // 64, 64)
    return torch.stack([t.sum(-1).T, (t * t).sum(-1).T], -1).contiguous()          # [N / 64, M, 2]


def _emu_attention(qkv, B, S, H, causal, rows=None, qrows=None):
    q, k, v = (t.float() for t in AR.unpack(qkv, B, S, H))
    vis = torch.ones(S, S, dtype=torch.bool).tril() if causal else torch.ones(S, S, dtype=torch.bool)
    if rows is None:
        s = (q @ k.transpose(-1, -2) / 8.0).masked_fill(~vis, float("-inf"))
        return AR.rows(torch.softmax(s, -1) @ v)
    qr = qrows.float().reshape(B, H, 64)
    s = torch.einsum("bhd,bhjd->bhj", qr, k) / 8.0
    s = s.masked_fill(~vis[rows][:, None, :], float("-inf"))
    return torch.einsum("bhj,bhjd->bhd", torch.softmax(s, -1), v).reshape(B, H * 64)


# ------------------------------------------------------------------------------------------------ the schedule
def steps(p):
    if p.f32:
        return _steps_f32(p)
    d, B, S, M, P, H, E = p.d, p.B, p.S, p.M, p.P, p.H, p.E
    parts = d // 64
    out = []
    X = Region("x_in.0" if p.train else "x", M, d, 0, d)          # the stream the assembly writes; xin(l) / xmid(l) below
    XLO = Region("x_lo", M, d, 0, d)
    STAT = Region("rowstat", M, 2, 0, 2)

    def add(label, call, reads, owns, ref, exact=None, emu=None):
        out.append(Step(label, call, tuple(reads), tuple(owns), ref, exact, emu))

    # cooperative split-K of the train-mode c_proj GEMM (text tower): `coop_ks` partial 64 x 128 tiles of 8192 floats per output tile, 4 tickets per tile
    coop_tiles = (M + 63) // 64 * (d // 128)
    COOP_SCRATCH = Region("coop_scratch", coop_tiles * p.coop_ks * 8192, 1, 0, 1)
    COOP_CNT = Region("coop_cnt", coop_tiles * 4, 1, 0, 1)

    def gemm_step(label, call, epi, a, w, o, bias=None, resid=None, lo=None, colsum=None, stat=None, stats_to=None, wrows=None, fault_site=None,
                  stat_in=None, out2=None, ksplit=1):
        """One GEMM launch.  a / o / resid / lo: Regions; w, bias, colsum: weight names (wrows: the rows of W and entries of bias / colsum used);
        stat: Region of (mean, rstd); stats_to: Region [parts * rows, 2] that receives the per-tile sums of the stored values."""
        lo_ = wrows or slice(None)

        def operands(b, fault):
            W, bs, cs = b[w][lo_], (b[bias].reshape(-1)[lo_] if bias else None), (b[colsum].reshape(-1)[lo_] if colsum else None)
            if fault_site:
                W, bs, cs = fault_site(b, fault, W, bs, cs)
            inp = {"A": view(b, a), "W": W[:, :a.ncols]}
            if bs is not None:
                inp["bias"] = bs
            if cs is not None:
                inp["colsum"] = cs
            if stat is not None:
                st = view(b, stat)
                if fault == "stats_row_minus_256" and st.shape[0] > 256:
                    st = torch.cat([st[:256], st[:-256]])
                inp["rowstat"] = st
            if stat_in is not None:          # train mode: the consumer adds the producer's partial sums itself
                part = view(b, stat_in).reshape(parts, a.rows, 2)
                if fault == "stats_row_minus_256" and a.rows > 256:
                    part = torch.cat([part[:, :256], part[:, :-256]], 1)
                inp["stat_in"] = part
            if resid is not None:
                inp["resid"] = view(b, resid)
                if fault == "c_proj_resid_from_x_in" and resid.slot.startswith("x_mid."):
                    inp["resid"] = view(b, resid._replace(slot="x_in." + resid.slot[6:]))
                if lo is not None:
                    inp["resid_lo"] = torch.zeros_like(view(b, lo)) if fault == "hilo_lo_dropped" else view(b, lo)
            return inp

        def ref(before, after, fault=None):
            inp = operands(before, fault)
            hi = view(after, o) if lo is not None else None
            res = G.reference(inp, epi, ksplit=ksplit, stats=stats_to is not None, hi_stored=hi)
            if fault == "hilo_lo_dropped" and lo is not None:          # the bound stays that of the unfaulted operands
                clean = G.reference(operands(before, None), epi, stats=stats_to is not None, hi_stored=hi)
                res = {k: (v[0], clean[k][1]) for k, v in res.items()}
            got = {"out": (view(after, o),) + res["out"]}
            if ksplit > 1:          # cooperative split-K: the tickets are zero again when the launch ends (the partial tiles in coop_scratch are its own business)
                z = torch.zeros(COOP_CNT.rows, 1, dtype=torch.float64)
                got["tickets"] = (view(after, COOP_CNT), z, z)
            if out2 is not None:
                got["out2"] = (view(after, out2),) + res["out2"]
            if stats_to is not None:
                got["stat_part"] = (view(after, stats_to).reshape(parts, o.rows, 2),) + res["stat_part"]
            if lo is not None:
                got["hilo"] = (view(after, o).double() + view(after, lo).double(),) + res["hilo"]
                got["lo"] = (view(after, lo),) + res["lo"]
            return got

        def emu(before):
            inp = operands(before, None)
            k64 = is64(before)
            if epi in G.FOLD:
                if stat_in is not None:
                    part = inp["stat_in"]
                    inp["rowstat"] = torch.cat(FR.stats_finalize(part, d)[0::2], -1) if k64 else \
                        _emu_onepass(part[..., 0].sum(0)[:, None], part[..., 1].sum(0)[:, None], d)
                y = _emu_fold(inp["A"], inp["W"], inp["bias"], inp["colsum"], inp["rowstat"]) if not k64 else \
                    (inp["A"] @ inp["W"].T - inp["colsum"] * inp["rowstat"][:, :1]) * inp["rowstat"][:, 1:] + inp["bias"]
                res = {o: store(_emu_gelu(y) if epi == G.EPI_LNFOLD_GELU_F16 else y, o.slot, k64)}
                if out2 is not None:
                    res[out2] = store(y, out2.slot, k64)
                return res
            acc = _emu_acc(inp["A"], inp["W"], inp.get("bias")) if not k64 else inp["A"] @ inp["W"].T + (inp["bias"] if "bias" in inp else 0.0)
            res = {}
            if epi == G.EPI_BIAS_GELU_F16:
                if out2 is not None:
                    res[out2] = store(acc, out2.slot, k64)
                acc = _emu_gelu(acc)
            if resid is not None:
                acc = acc + (inp["resid"] if k64 else inp["resid"].float() + (inp["resid_lo"].float() if lo is not None else 0.0))
                if stats_to is not None:
                    res[stats_to] = _emu_tiles(acc).reshape(-1, 2)
                if lo is not None:
                    hi = store(acc, o.slot, k64)
                    res[lo] = store(acc - (hi if k64 else hi.float()), lo.slot, k64)
            res[o] = store(acc, o.slot, k64)
            return res

        reads = [a.slot, w] + [n for n in (bias, colsum) if n] + [r.slot for r in (stat, stat_in, resid, lo) if r is not None]
        # (a stat_in launch on the persistent GEMM kernel would finalise the sums into rowstat first, csrc/gemm_plan.cpp: no launch at these shapes is,
        # so rowstat is NOT owned and must keep its bits)
        owns = [o] + [r for r in (stats_to, lo, out2) if r is not None]
        if ksplit > 1:
            owns += [COOP_SCRATCH, COOP_CNT]
        add(label, call, reads, owns, ref, None, emu)

    def row_op(label, call, reads, o, fn, fn32, exact=None):
        """A row kernel with one output region: fn(before, fault) -> (value, bound of the f32 result); the store adds its own rounding."""
        def ref(before, after, fault=None):
            v, e = fn(before, fault)
            v0, e0 = fn(before, None) if fault else (v, e)
            return {"out": (view(after, o), v, _h(v0, e0) if f16slot(o.slot) else e0)}

        def emu(before):
            return {o: store(fn(before, None)[0] if is64(before) else fn32(before), o.slot, is64(before))}
        add(label, call, reads, [o], ref, exact, emu)

    # -------------------------------------------------------------------------------------------- stream assembly
    pos_name = "w:positional_embedding"
    if p.kind == 0:
        G2, kpad = p.G2, p.kpad
        PATCH = Region("patches", B * G2, kpad, 0, kpad)
        POUT = Region("patch_out", B * G2, d, 0, d)

        def im2col(b, dtype):
            return FR.im2col(b["in:images"].view(B, 3, p.resolution, p.resolution), p.patch, kpad, dtype)
        add("im2col", "launch_im2col(", ["in:images"], [PATCH],
            lambda before, after, fault=None: {"out": (view(after, PATCH), im2col(before, torch.float64), FR.half_bound(im2col(before, torch.float64), 0.0))},
            lambda before: {PATCH: im2col(before, torch.float16)},
            lambda before: {PATCH: im2col(before, torch.float64 if is64(before) else torch.float16)})
        gemm_step("patch_embed", "launch_gemm(EPI_F32", G.EPI_F32, PATCH, "w:conv1.weight", POUT)

        def assemble(b, fault):
            pos = None if (p.no_pos and fault != "pos_under_no_pos") else b[pos_name]
            pre = b["in:prefix"].view(-1, d) if P else None
            if fault == "prompt_rows_shifted" and P:
                pre = pre.view(-1, P, d).roll(1, 1).reshape(-1, d)
            return FR.vit_assemble(view(b, POUT), b["w:class_embedding"], pos, pre, b["w:ln_pre.weight"].reshape(-1), b["w:ln_pre.bias"].reshape(-1),
                                   B, P, G2, p.per_image)

        def assemble_ref(before, after, fault=None):
            y, e_y, (mean, e_mean, rstd, e_rstd) = assemble(before, fault)
            y0, e0, (_, e_mean, _, e_rstd) = assemble(before, None)
            st = view(after, STAT)
            res = {"x": (view(after, X), y, _h(y0, e0)), "mean": (st[:, :1], mean, e_mean), "rstd": (st[:, 1:], rstd, e_rstd)}
            if p.hilo:
                res["x_lo"] = (view(after, XLO),) + FR.x_lo(y, e0, view(after, X))
            return res

        def assemble_emu(before):
            k64 = is64(before)
            if k64:
                y, _, (mean, _, rstd, _) = assemble(before, None)
            else:
                v = torch.zeros(B, S, d)
                v[:, 0] = before["w:class_embedding"].reshape(-1)
                v[:, 1 + P:] = view(before, POUT).view(B, G2, d)
                if P:
                    v[:, 1:1 + P] = before["in:prefix"].view(-1, P, d)
                if not p.no_pos:
                    v[:, 0] += before[pos_name][0]
                    v[:, 1 + P:] += before[pos_name][1:1 + G2]
                y = _emu_ln(v.reshape(M, d), before["w:ln_pre.weight"].reshape(-1), before["w:ln_pre.bias"].reshape(-1))
                c = y - y.mean(-1, keepdim=True)
                mean, rstd = y.mean(-1, keepdim=True), ((c * c).mean(-1, keepdim=True) + FR.LN_EPS).rsqrt()
            res = {X: store(y, "x", k64), STAT: store(torch.cat([mean, rstd], -1), "rowstat", k64)}
            if p.hilo:
                res[XLO] = store(y - (res[X] if k64 else res[X].float()), "x_lo", k64)
            return res
        add("assemble", "launch_vit_assemble_ln(", ["patch_out", "w:class_embedding", pos_name, "in:prefix", "w:ln_pre.weight", "w:ln_pre.bias"],
            [X, STAT] + ([XLO] if p.hilo else []), assemble_ref, None, assemble_emu)
    else:
        def embed(b, fault):
            pos = None if (p.no_pos and fault != "pos_under_no_pos") else b[pos_name]
            pre = b["in:prefix"].view(-1, d) if P else None
            if fault == "prompt_rows_shifted" and P:
                pre = pre.view(-1, P, d).roll(1, 1).reshape(-1, d)
            return FR.text_embed(b["in:ids"].view(B, p.seq0), b["w:token_embedding.weight"], pos, pre, P, p.prefix_classes, B, S, p.Ps)

        def embed_ref(before, after, fault=None):
            v, e_v, (mean, _, rstd, _) = embed(before, fault)
            v0, e0, (_, e_mean, _, e_rstd) = embed(before, None)
            st = view(after, STAT)
            res = {"x": (view(after, X), v, _h(v0, e0) + 1e-300), "mean": (st[:, :1], mean, e_mean), "rstd": (st[:, 1:], rstd, e_rstd)}
            if p.coop_ks > 1:          # the forward zeroes the tickets (a memset, no launch) before its first launch
                z = torch.zeros(COOP_CNT.rows, 1, dtype=torch.float64)
                res["tickets"] = (view(after, COOP_CNT), z, z)
            return res

        def embed_emu(before):
            k64 = is64(before)
            v, _, (mean, _, rstd, _) = embed(before, None)
            if not k64:
                v = v.float()          # (one f32 add of f32 operands: float64 rounded once is the same number)
                mean, rstd = _emu_onepass(v.sum(-1, keepdim=True), (v * v).sum(-1, keepdim=True), d).split(1, -1)
            res = {X: store(v, "x", k64), STAT: store(torch.cat([mean, rstd], -1), "rowstat", k64)}
            if p.coop_ks > 1:
                res[COOP_CNT] = torch.zeros(COOP_CNT.rows, 1, dtype=torch.float64 if k64 else torch.float32)
            return res
        add("embed", "launch_text_embed(", ["in:ids", "w:token_embedding.weight", pos_name, "in:prefix"], [X, STAT] + ([COOP_CNT] if p.coop_ks > 1 else []),
            embed_ref, None, embed_emu)

    # -------------------------------------------------------------------------------------------- blocks
    def deep_step(l):
        def values(b, fault):
            rows, src = _deep_rows(p, b, l)
            if fault == "deep_one_block_late":
                src = _deep_rows(p, b, l - 1)[1] if l >= 2 else view(b, X)[rows]
            if fault == "deep_image0_only" and p.kind == 0 and B > 1:
                src = torch.cat([src[:P].double(), view(b, X)[rows[P:]].double()])
            return rows, src

        def ref(before, after, fault=None):
            rows, src = values(before, fault)
            _, src0 = _deep_rows(p, before, l)
            _, _, _, (mean, e_mean, rstd, e_rstd) = FR.deep_insert(src0.float(), p.hilo)
            st = view(after, STAT)[rows]
            res = {"x": (view(after, X)[rows], src.double(), FR.half_bound(src0.double(), 0.0)),
                   "mean": (st[:, :1], mean, e_mean), "rstd": (st[:, 1:], rstd, e_rstd)}
            if p.hilo:
                res["x_lo"] = (view(after, XLO)[rows], src0.double() - view(after, X)[rows].double(), FR.half_bound(src0.double() - view(after, X)[rows].double(), 0.0))
            # the launch owns the prompt rows alone: every other row of what it writes into keeps its value (the stream: `exact`)
            kept = torch.ones(M, dtype=torch.bool)
            kept[rows] = False
            for name, reg in (("rowstat kept", STAT),) + ((("x_lo kept", XLO),) if p.hilo else ()):
                res[name] = (view(after, reg)[kept], view(before, reg)[kept].double(), torch.zeros_like(view(before, reg)[kept], dtype=torch.float64))
            return res

        def emu(before):
            k64 = is64(before)
            rows, src = _deep_rows(p, before, l)
            x, st = view(before, X).clone(), view(before, STAT).clone()
            x[rows] = store(src, "x", k64)
            v = src.double() if k64 else x[rows].float()
            res = {}
            if p.hilo:
                xl = view(before, XLO).clone()
                xl[rows] = store(src - (x[rows] if k64 else x[rows].float()), "x_lo", k64)
                res[XLO] = xl
                v = v if k64 else v + xl[rows].float()
            if k64:
                c = v - v.mean(-1, keepdim=True)
                st[rows] = torch.cat([v.mean(-1, keepdim=True), ((c * c).mean(-1, keepdim=True) + FR.LN_EPS).rsqrt()], -1)
            else:
                st[rows] = _emu_onepass(v.sum(-1, keepdim=True), (v * v).sum(-1, keepdim=True), d)
            res.update({X: x, STAT: st})
            return res

        def exact(before):
            rows, src = _deep_rows(p, before, l)
            x = view(before, X).clone()
            x[rows] = src.float().half()
            return {X: x}
        add(f"b{l}.deep_insert", "launch_vit_deep_insert(" if p.kind == 0 else "launch_text_deep_insert(", ["in:deep", "x", "rowstat"],
            [X, STAT] + ([XLO] if p.hilo else []), ref, exact, emu)

    def gamma_swap(l):
        """`ln2` gamma used for `ln1`: the folded operand f16(ln_2.weight o W) in place of f16(ln_1.weight o W)."""
        def site(b, fault, W, bs, cs):
            if fault == "ln2_gamma_for_ln1":
                Wg, _, _ = FR.fold_weights(b[p.lw(l, "attn.in_proj_weight")], b[p.lw(l, "ln_2.weight")].reshape(-1), b[p.lw(l, "ln_1.bias")].reshape(-1),
                                           b[p.lw(l, "attn.in_proj_bias")].reshape(-1))
                W = Wg[-W.shape[0]:] if W.shape[0] != Wg.shape[0] else Wg
            if fault == "kv_bias_no_offset" and W.shape[0] == 2 * d:
                bs = b[p.lw(l, "attn.in_proj#bias")].reshape(-1)[:2 * d]
            if fault == "colsum_q_for_k" and W.shape[0] == 2 * d:
                cs = b[p.lw(l, "attn.in_proj#colsum")].reshape(-1)[:2 * d]
            return W, bs, cs
        return site

    def finalize_step(label):
        def fin(b, fault):
            return FR.stats_finalize(view(b, Region("stat_part", parts * M, 2, 0, 2)).reshape(parts, M, 2), d)

        def ref(before, after, fault=None):
            mean, e_mean, rstd, e_rstd = fin(before, fault)
            st = view(after, STAT)
            return {"mean": (st[:, :1], mean, e_mean), "rstd": (st[:, 1:], rstd, e_rstd)}

        def emu(before):
            k64 = is64(before)
            part = view(before, Region("stat_part", parts * M, 2, 0, 2)).reshape(parts, M, 2)
            if k64:
                mean, _, rstd, _ = fin(before, None)
                return {STAT: torch.cat([mean, rstd], -1)}
            return {STAT: _emu_onepass(part[..., 0].sum(0)[:, None], part[..., 1].sum(0)[:, None], d)}
        add(label, "launch_ln_stats_finalize(", ["stat_part"], [STAT], ref, None, emu)

    QKV = Region("qkv", M, 3 * d, 0, 3 * d)
    ATT = Region("att", M, d, 0, d)
    HID = Region("h", M, 4 * d, 0, 4 * d)
    SP = Region("stat_part", parts * M, 2, 0, 2)
    lo = XLO if p.hilo else None
    rr = p.read_rows()
    xin = lambda l: Region(f"x_in.{l}", M, d, 0, d)          # noqa: E731
    final_stream = None

    def deep_step_train(l):
        """Train mode: the rows go into x_in[l], their per-tile sums into stat_part (the consumer adds them itself); rowstat is not touched."""
        XL = xin(l)

        def values(b, fault):
            rows, src = _deep_rows(p, b, l)
            if fault == "deep_one_block_late":
                src = _deep_rows(p, b, l - 1)[1] if l >= 2 else view(b, XL)[rows]
            if fault == "deep_image0_only" and p.kind == 0 and B > 1:
                src = torch.cat([src[:P].double(), view(b, XL)[rows[P:]].double()])
            return rows, src

        def ref(before, after, fault=None):
            rows, src = values(before, fault)
            _, src0 = _deep_rows(p, before, l)
            _, _, (ts, e_ts, tq, e_tq), _ = FR.deep_insert(src0.float(), False)
            part = view(after, SP).reshape(parts, M, 2)
            kept = torch.ones(M, dtype=torch.bool)
            kept[rows] = False
            old = view(before, SP).reshape(parts, M, 2)[:, kept].double()
            return {"x": (view(after, XL)[rows], src.double(), FR.half_bound(src0.double(), 0.0)),
                    "tile sum": (part[:, rows, 0].T, ts, e_ts), "tile sum of squares": (part[:, rows, 1].T, tq, e_tq),
                    "stat_part kept": (part[:, kept], old, torch.zeros_like(old))}

        def emu(before):
            k64 = is64(before)
            rows, src = _deep_rows(p, before, l)
            x, part = view(before, XL).clone(), view(before, SP).reshape(parts, M, 2).clone()
            x[rows] = store(src, XL.slot, k64)
            t = (src.double() if k64 else x[rows].float()).reshape(-1, parts, 64)
            part[:, rows, 0], part[:, rows, 1] = t.sum(-1).T.to(part.dtype), (t * t).sum(-1).T.to(part.dtype)
            return {XL: x, SP: part.reshape(-1, 2)}

        def exact(before):
            rows, src = _deep_rows(p, before, l)
            x = view(before, XL).clone()
            x[rows] = src.float().half()
            return {XL: x}
        add(f"b{l}.deep_insert", "launch_vit_deep_insert(" if p.kind == 0 else "launch_text_deep_insert(", ["in:deep", XL.slot, "stat_part"], [XL, SP], ref, exact, emu)

    def ln_step(label, src, dst, l, which, fault_swap=False):
        def fn(b, fault):
            g = b[p.lw(l, "ln_2.weight" if (which == 2 or (fault_swap and fault == "ln2_gamma_for_ln1")) else "ln_1.weight")].reshape(-1)
            return FR.ln_fwd(view(b, src).double(), g, b[p.lw(l, f"ln_{which}.bias")].reshape(-1))
        row_op(label, "launch_layernorm_f16(", [src.slot, p.lw(l, f"ln_{which}.weight"), p.lw(l, f"ln_{which}.bias")], dst, fn,
               lambda b: _emu_ln(view(b, src), b[p.lw(l, f"ln_{which}.weight")].reshape(-1), b[p.lw(l, f"ln_{which}.bias")].reshape(-1)))

    for l in range(p.layers if p.train else 0):
        last = l + 1 == p.layers
        XI, XM, XO = xin(l), Region(f"x_mid.{l}", M, d, 0, d), xin(l + 1)
        QL, AL, HP = Region(f"qkv_l.{l}", M, 3 * d, 0, 3 * d), Region(f"att_l.{l}", M, d, 0, d), Region(f"hpre_l.{l}", M, 4 * d, 0, 4 * d)
        if 1 <= l <= p.n_deep:
            deep_step_train(l)
        if last and p.rows_only:
            # the read rows alone, everything its backward needs saved in compact [B, .] buffers; Q of every row comes with K and V (one GEMM, literal ln_1)
            XN = Region("xn", M, d, 0, d)
            RX, RMID, ROUT = Region("row_x", B, d, 0, d), Region("row_xmid", B, d, 0, d), Region("row_xout", B, d, 0, d)
            RXN, RATT, RH, RHP = Region("row_xn", B, d, 0, d), Region("row_att", B, d, 0, d), Region("row_h", B, 4 * d, 0, 4 * d), Region("row_hpre", B, 4 * d, 0, 4 * d)
            ln_step(f"b{l}.ln1", XI, XN, l, 1)
            gemm_step(f"b{l}.qkv", "launch_gemm(EPI_BIAS_F16", G.EPI_BIAS_F16, XN, p.lw(l, "attn.in_proj_weight"), QL, bias=p.lw(l, "attn.in_proj_bias"))

            def attn_row_train(before, after, fault=None, QL=QL):
                res = AR.attention_row(view(before, QL), B, S, H, p.causal, row_index=(rr - torch.arange(B) * S))
                return {"out": (view(after, RATT), res["out"], AR.bound(res, "o", "fwd_row"))}
            add(f"b{l}.attention_row", "launch_attention_row(", [QL.slot, "in:eot"], [RATT], attn_row_train, None,
                lambda before, QL=QL: {RATT: store(_emu_attention(view(before, QL), B, S, H, p.causal, rows=(rr - torch.arange(B) * S),
                                                                  qrows=view(before, QL)[rr][:, :d]) if not is64(before)
                                                   else attn_row_train(before, before)["out"][1], "row_att", is64(before))})

            def g_rows(b, fault, XI=XI):
                at = rr
                if fault == "eot_of_previous_class" and p.kind == 1:
                    at = torch.arange(B) * p.rs + torch.tensor(p.eot).roll(1)
                return view(b, XI)[at]
            add(f"b{l}.gather_row_x", "launch_gather_rows(", [XI.slot, "in:eot"], [RX],
                lambda before, after, fault=None: {"out": (view(after, RX), g_rows(before, fault).double(), torch.zeros(B, d, dtype=torch.float64))},
                lambda before: {RX: g_rows(before, None)}, lambda before: {RX: g_rows(before, None)})
            gemm_step(f"b{l}.out_proj", "launch_gemm(EPI_BIAS_RESID", G.EPI_BIAS_RESID, RATT, p.lw(l, "attn.out_proj.weight"), RMID, bias=p.lw(l, "attn.out_proj.bias"),
                      resid=RX)
            ln_step(f"b{l}.ln2", RMID, RXN, l, 2)
            gemm_step(f"b{l}.c_fc", "launch_gemm(EPI_BIAS_GELU_F16", G.EPI_BIAS_GELU_F16, RXN, p.lw(l, "mlp.c_fc.weight"), RH, bias=p.lw(l, "mlp.c_fc.bias"), out2=RHP)
            gemm_step(f"b{l}.c_proj", "launch_gemm(EPI_BIAS_RESID", G.EPI_BIAS_RESID, RH, p.lw(l, "mlp.c_proj.weight"), ROUT, bias=p.lw(l, "mlp.c_proj.bias"),
                      resid=RMID)
            final_stream = ROUT
            break
        # block 0 reads the (mean, rstd) the assembly wrote; a later block adds the partial sums of the epilogue that produced its input
        gemm_step(f"b{l}.qkv", "launch_gemm(EPI_LNFOLD_F16", G.EPI_LNFOLD_F16, XI, p.lw(l, "attn.in_proj_weight#G"), QL, bias=p.lw(l, "attn.in_proj#bias"),
                  colsum=p.lw(l, "attn.in_proj#colsum"), stat=STAT if l == 0 else None, stat_in=SP if l > 0 else None, fault_site=gamma_swap(l))

        def attn_train(before, after, fault=None, QL=QL, AL=AL):
            res = AR.attention_shared(view(before, QL), B, S, H, p.Ps) if p.Ps else AR.attention(view(before, QL), B, S, H, p.causal)
            return {"out": (view(after, AL), res["out"], AR.bound(res, "o", "fwd_mfma"))}

        def attn_train_emu(before, QL=QL, AL=AL, ref=attn_train):
            if is64(before):
                return {AL: ref(before, before)["out"][1]}
            q = AR.from_shared(view(before, QL), B, S, p.Ps) if p.Ps else view(before, QL)
            o = _emu_attention(q, B, S, H, p.causal)
            return {AL: store(AR.to_shared(o, B, S, p.Ps) if p.Ps else o, AL.slot, False)}
        add(f"b{l}.attention", "launch_attention_fwd(", [QL.slot], [AL], attn_train, None, attn_train_emu)
        gemm_step(f"b{l}.out_proj", "launch_gemm(EPI_BIAS_RESID", G.EPI_BIAS_RESID, AL, p.lw(l, "attn.out_proj.weight"), XM, bias=p.lw(l, "attn.out_proj.bias"),
                  resid=XI, stats_to=SP)
        gemm_step(f"b{l}.c_fc", "launch_gemm(EPI_LNFOLD_GELU_F16", G.EPI_LNFOLD_GELU_F16, XM, p.lw(l, "mlp.c_fc.weight#G"), HID, bias=p.lw(l, "mlp.c_fc#bias"),
                  colsum=p.lw(l, "mlp.c_fc#colsum"), stat_in=SP, out2=HP)
        gemm_step(f"b{l}.c_proj", "launch_gemm(EPI_BIAS_RESID", G.EPI_BIAS_RESID, HID, p.lw(l, "mlp.c_proj.weight"), XO, bias=p.lw(l, "mlp.c_proj.bias"),
                  resid=XM, stats_to=None if last else SP, ksplit=p.coop_ks)
        final_stream = XO
    for l in range(0 if p.train else p.layers):
        last = l + 1 == p.layers
        if 1 <= l <= p.n_deep:
            deep_step(l)
        if last and p.rows_only:
            KV = Region("qkv", M, 3 * d, d, 2 * d)
            RX, RLO = Region("row_x", B, d, 0, d), Region("row_x_lo", B, d, 0, d)
            RXN, RATT = Region("row_xn", B, d, 0, d), Region("row_att", B, d, 0, d)
            RQ, RH = Region("row_h", B, d, 0, d), Region("row_h", B, 4 * d, 0, 4 * d)
            RSP = Region("stat_part", parts * B, 2, 0, 2)
            rlo = RLO if p.hilo else None
            gemm_step(f"b{l}.kv", "launch_gemm(EPI_LNFOLD_F16", G.EPI_LNFOLD_F16, X, p.lw(l, "attn.in_proj_weight#G"), KV, bias=p.lw(l, "attn.in_proj#bias"),
                      colsum=p.lw(l, "attn.in_proj#colsum"), stat=STAT, wrows=slice(d, 3 * d), fault_site=gamma_swap(l))

            def gather(src, dst):
                def rows(b, fault):
                    at = rr
                    if fault == "eot_of_previous_class" and p.kind == 1:
                        at = torch.arange(B) * p.rs + torch.tensor(p.eot).roll(1)
                    return view(b, src)[at]
                add(f"b{l}.gather_{dst.slot}", "launch_gather_rows(", [src.slot, "in:eot"], [dst],
                    lambda before, after, fault=None: {"out": (view(after, dst), rows(before, fault).double(), torch.zeros(B, d, dtype=torch.float64))},
                    lambda before: {dst: rows(before, None)}, lambda before: {dst: rows(before, None)})
            gather(X, RX)
            if p.hilo:
                gather(XLO, RLO)

            def ln_rows(which, src):
                def fn(b, fault):
                    g = b[p.lw(l, "ln_2.weight" if (fault == "ln2_gamma_for_ln1" or which == 2) else "ln_1.weight")].reshape(-1)
                    return FR.ln_fwd(view(b, src).double(), g, b[p.lw(l, f"ln_{which}.bias")].reshape(-1))
                row_op(f"b{l}.ln{which}", "launch_layernorm_f16(", [src.slot, p.lw(l, f"ln_{which}.weight"), p.lw(l, f"ln_{which}.bias")], RXN, fn,
                       lambda b: _emu_ln(view(b, src), b[p.lw(l, f"ln_{which}.weight")].reshape(-1), b[p.lw(l, f"ln_{which}.bias")].reshape(-1)))
            ln_rows(1, RX)
            gemm_step(f"b{l}.q", "launch_gemm(EPI_BIAS_F16", G.EPI_BIAS_F16, RXN, p.lw(l, "attn.in_proj_weight"), RQ, bias=p.lw(l, "attn.in_proj_bias"), wrows=slice(0, d))

            def attn_row_ref(before, after, fault=None):
                res = AR.attention_row(view(before, QKV), B, S, H, p.causal, row_index=(rr - torch.arange(B) * S), qrows=view(before, RQ))
                return {"out": (view(after, RATT), res["out"], AR.bound(res, "o", "fwd_row"))}
            add(f"b{l}.attention_row", "launch_attention_row(", ["qkv", "row_h", "in:eot"], [RATT], attn_row_ref, None,
                lambda before: {RATT: store(_emu_attention(view(before, QKV), B, S, H, p.causal, rows=(rr - torch.arange(B) * S), qrows=view(before, RQ))
                                            if not is64(before) else attn_row_ref(before, before)["out"][1], "row_att", is64(before))})
            gemm_step(f"b{l}.out_proj", "launch_gemm(EPI_BIAS_RESID", G.EPI_BIAS_RESID, RATT, p.lw(l, "attn.out_proj.weight"), RX, bias=p.lw(l, "attn.out_proj.bias"),
                      resid=RX, lo=rlo, stats_to=RSP if p.hilo else None)
            ln_rows(2, RX)
            gemm_step(f"b{l}.c_fc", "launch_gemm(EPI_BIAS_GELU_F16", G.EPI_BIAS_GELU_F16, RXN, p.lw(l, "mlp.c_fc.weight"), RH, bias=p.lw(l, "mlp.c_fc.bias"))
            gemm_step(f"b{l}.c_proj", "launch_gemm(EPI_BIAS_RESID", G.EPI_BIAS_RESID, RH, p.lw(l, "mlp.c_proj.weight"), RX, bias=p.lw(l, "mlp.c_proj.bias"),
                      resid=RX, lo=rlo, stats_to=RSP if p.hilo else None)
            break
        gemm_step(f"b{l}.qkv", "launch_gemm(EPI_LNFOLD_F16", G.EPI_LNFOLD_F16, X, p.lw(l, "attn.in_proj_weight#G"), QKV, bias=p.lw(l, "attn.in_proj#bias"),
                  colsum=p.lw(l, "attn.in_proj#colsum"), stat=STAT, fault_site=gamma_swap(l))

        def attn_ref(before, after, fault=None):
            res = AR.attention_shared(view(before, QKV), B, S, H, p.Ps) if p.Ps else AR.attention(view(before, QKV), B, S, H, p.causal)
            return {"out": (view(after, ATT), res["out"], AR.bound(res, "o", "fwd_mfma"))}

        def attn_emu(before):
            if is64(before):
                return {ATT: attn_ref(before, before)["out"][1]}
            q = AR.from_shared(view(before, QKV), B, S, p.Ps) if p.Ps else view(before, QKV)
            o = _emu_attention(q, B, S, H, p.causal)
            return {ATT: store(AR.to_shared(o, B, S, p.Ps) if p.Ps else o, "att", False)}
        add(f"b{l}.attention", "launch_attention_fwd(", ["qkv"], [ATT], attn_ref, None, attn_emu)
        gemm_step(f"b{l}.out_proj", "launch_gemm(EPI_BIAS_RESID", G.EPI_BIAS_RESID, ATT, p.lw(l, "attn.out_proj.weight"), X, bias=p.lw(l, "attn.out_proj.bias"),
                  resid=X, lo=lo, stats_to=SP)
        finalize_step(f"b{l}.stats_mid")
        gemm_step(f"b{l}.c_fc", "launch_gemm(EPI_LNFOLD_GELU_F16", G.EPI_LNFOLD_GELU_F16, X, p.lw(l, "mlp.c_fc.weight#G"), HID, bias=p.lw(l, "mlp.c_fc#bias"),
                  colsum=p.lw(l, "mlp.c_fc#colsum"), stat=STAT)
        # the last block's sums have no reader (ln_post reads the stream's read rows); the compensated epilogue emits them all the same
        gemm_step(f"b{l}.c_proj", "launch_gemm(EPI_BIAS_RESID", G.EPI_BIAS_RESID, HID, p.lw(l, "mlp.c_proj.weight"), X, bias=p.lw(l, "mlp.c_proj.bias"),
                  resid=X, lo=lo, stats_to=SP if (not last or p.hilo) else None)
        if not last:
            finalize_step(f"b{l}.stats_out")

    # -------------------------------------------------------------------------------------------- head
    CLS = Region("cls16", B, d, 0, d)
    compact = p.rows_only
    src = final_stream if p.train else (Region("row_x", B, d, 0, d) if compact else X)

    def post(b, fault):
        at = torch.arange(B) if compact else rr
        if fault == "shared_row_map_off_by_one_class" and p.Ps and B > 1:
            at = at.roll(1)
        return FR.ln_fwd(view(b, src)[at].double(), b[p.final("weight")].reshape(-1), b[p.final("bias")].reshape(-1), None,
                         "drop_beta" if fault == "ln_post_beta_dropped" else None)
    row_op("ln_post", "launch_gather_ln_f16(", [src.slot, p.final("weight"), p.final("bias"), "in:eot"], CLS, post,
           lambda b: _emu_ln(view(b, src)[torch.arange(B) if compact else rr], b[p.final("weight")].reshape(-1), b[p.final("bias")].reshape(-1)))
    gemm_step("projection", "launch_gemm(EPI_F32", G.EPI_F32, CLS, "w:proj#T" if p.kind == 0 else "w:text_projection#T", Region("out:emb", B, E, 0, E))
    return out


def _steps_f32(p):
    """The exact (precision 1) tower: every buffer f32, LayerNorm a launch of its own in front of the QKV and c_fc GEMMs, the f32 GEMM and attention
    kernels (tests/tier_ref.py), no statistics buffers, no compensated stream, the plain row layout.  The last block: ln_1 and K / V for every row, then the
    read rows alone."""
    import tier_ref as TR
    d, B, S, M, P, H, E = p.d, p.B, p.S, p.M, p.P, p.H, p.E
    out = []
    X, XN = Region("x", M, d, 0, d), Region("xn", M, d, 0, d)
    st = lambda v, k64: v.double() if k64 else v.float()          # noqa: E731
    tier = 2 if p.split else 1
    # the split tower's split-layout buffers ([rows, K / 32, 32 hi | 32 lo] f16, 4 bytes per element): what feeds a block GEMM
    in_split = p.split_layout

    def rd(b, r):
        """The region's values: a split-layout buffer decoded as hi + lo (the float64 chain keeps plain values everywhere)."""
        v = view(b, r)
        return FR.unsplit(v.contiguous(), r.rows, r.ncols) if (in_split(r) and not is64(b)) else v

    def enc(v, r, k64):
        if k64 or not in_split(r):
            return st(v, k64)
        return TR.to_layout(*TR.split(v.float())).view(torch.float32)

    def add(label, call, reads, owns, ref, exact=None, emu=None):
        out.append(Step(label, call, tuple(reads), tuple(owns), ref, exact, emu))

    def one(label, call, reads, o, fn, fn32, exact=None, copy=False):
        """One output region: fn(before, fault) -> (value, bound); fn32(before) the float32 stand-in (copy: the stand-in is `exact`, a copy of bits)."""
        def ref(before, after, fault=None):
            v, _ = fn(before, fault)
            return {"out": (rd(after, o), v, fn(before, None)[1])}
        add(label, call, reads, [o], ref, exact, exact if copy else lambda before: {o: enc(fn(before, None)[0] if is64(before) else fn32(before), o, is64(before))})

    def gemm(label, epi, a, w, o, bias=None, resid=None, wrows=None, tier=1):
        rows_ = wrows or slice(None)

        def operands(b):
            inp = {"A": rd(b, a), "W": b[w][rows_][:, :a.ncols]}
            if bias:
                inp["bias"] = b[bias].reshape(-1)[rows_]
            if resid is not None:
                inp["resid"] = view(b, resid)
            return inp

        def fn(b, fault):
            return TR.gemm_reference(operands(b), tier, epi, w_exact=(tier == 2 and p.w_grid))["out"]

        def fn32(b):
            inp = operands(b)
            acc = _emu_acc(inp["A"], inp["W"], inp.get("bias"))
            if epi == TR.EPI_GELU:
                acc = _emu_gelu(acc)
            return acc + inp["resid"] if resid is not None else acc
        call = {TR.EPI_F32: "EPI_F32", TR.EPI_BIAS: "EPI_BIAS_F16", TR.EPI_GELU: "EPI_BIAS_GELU_F16", TR.EPI_RESID: "EPI_BIAS_RESID"}[epi]
        one(label, "launch_gemm(" + call, [a.slot, w] + ([bias] if bias else []) + ([resid.slot] if resid is not None else []), o, fn, fn32)

    def ln(label, call, src, dst, g, b_, rows=None):
        def fn(b, fault):
            x = rd(b, src)
            gamma = b[g.replace("ln_1", "ln_2") if fault == "ln2_gamma_for_ln1" else g].reshape(-1)
            y, e = FR.ln_fwd((x if rows is None else x[rows]).double(), gamma, b[b_].reshape(-1), None, "drop_beta" if fault == "ln_post_beta_dropped" else None)
            return y, (e + FR.split_bound(y, e) if in_split(dst) else e)
        one(label, call, [src.slot, g, b_], dst, fn, lambda b: _emu_ln(view(b, src) if rows is None else view(b, src)[rows], b[g].reshape(-1), b[b_].reshape(-1)))

    pos_name = "w:positional_embedding"
    if p.kind == 0:
        G2, kpad = p.G2, p.kpad
        PATCH, POUT = Region("patches", B * G2, kpad, 0, kpad), Region("patch_out", B * G2, d, 0, d)
        im = lambda b, dt: FR.im2col(b["in:images"].view(B, 3, p.resolution, p.resolution), p.patch, kpad, dt)          # noqa: E731
        one("im2col", "launch_im2col(", ["in:images"], PATCH, lambda b, fault: (im(b, torch.float64), torch.zeros(B * G2, kpad, dtype=torch.float64)),
            lambda b: im(b, torch.float32), lambda b: {PATCH: im(b, torch.float32)})
        gemm("patch_embed", TR.EPI_F32, PATCH, "w:conv1.weight", POUT)

        def assemble(b, fault):
            pos = None if (p.no_pos and fault != "pos_under_no_pos") else b[pos_name]
            pre = b["in:prefix"].view(-1, d) if P else None
            if fault == "prompt_rows_shifted" and P:
                pre = pre.view(-1, P, d).roll(1, 1).reshape(-1, d)
            y, e_y, _ = FR.vit_assemble(view(b, POUT), b["w:class_embedding"], pos, pre, b["w:ln_pre.weight"].reshape(-1), b["w:ln_pre.bias"].reshape(-1), B, P, G2,
                                        p.per_image)
            return y, e_y

        def assemble32(b):
            v = torch.zeros(B, S, d)
            v[:, 0] = b["w:class_embedding"].reshape(-1)
            v[:, 1 + P:] = view(b, POUT).view(B, G2, d)
            if P:
                v[:, 1:1 + P] = b["in:prefix"].view(-1, P, d)
            if not p.no_pos:
                v[:, 0] += b[pos_name][0]
                v[:, 1 + P:] += b[pos_name][1:1 + G2]
            return _emu_ln(v.reshape(M, d), b["w:ln_pre.weight"].reshape(-1), b["w:ln_pre.bias"].reshape(-1))
        one("assemble", "launch_vit_assemble_ln(", ["patch_out", "w:class_embedding", pos_name, "in:prefix", "w:ln_pre.weight", "w:ln_pre.bias"], X, assemble, assemble32)
    else:
        def embed(b, fault):
            pos = None if (p.no_pos and fault != "pos_under_no_pos") else b[pos_name]
            pre = b["in:prefix"].view(-1, d) if P else None
            if fault == "prompt_rows_shifted" and P:
                pre = pre.view(-1, P, d).roll(1, 1).reshape(-1, d)
            v, e_v, _ = FR.text_embed(b["in:ids"].view(B, p.seq0), b["w:token_embedding.weight"], pos, pre, P, p.prefix_classes, B, S, 0)
            return v, e_v + 1e-300
        one("embed", "launch_text_embed(", ["in:ids", "w:token_embedding.weight", pos_name, "in:prefix"], X, embed, lambda b: embed(b, None)[0].float())

    QKV, ATT, HID = Region("qkv", M, 3 * d, 0, 3 * d), Region("att", M, d, 0, d), Region("h", M, 4 * d, 0, 4 * d)
    rr = p.read_rows()
    for l in range(p.layers):
        last = l + 1 == p.layers
        if 1 <= l <= p.n_deep:
            def deep(b, fault, l=l):
                rows, src = _deep_rows(p, b, l)
                if fault == "deep_one_block_late":
                    src = _deep_rows(p, b, l - 1)[1] if l >= 2 else view(b, X)[rows]
                if fault == "deep_image0_only" and p.kind == 0 and B > 1:
                    src = torch.cat([src[:P].double(), view(b, X)[rows[P:]].double()])
                x = view(b, X).double().clone()
                x[rows] = src.double()
                return x, torch.zeros(M, d, dtype=torch.float64)
            one(f"b{l}.deep_insert", "launch_vit_deep_insert(" if p.kind == 0 else "launch_text_deep_insert(", ["in:deep", "x"], X, deep,
                lambda b, deep=deep: deep(b, None)[0].float(), lambda b, deep=deep: {X: deep(b, None)[0].float()})
        ln(f"b{l}.ln1", "launch_layernorm_f16(", X, XN, p.lw(l, "ln_1.weight"), p.lw(l, "ln_1.bias"))
        if last:
            KV = Region("qkv", M, 3 * d, d, 2 * d)
            RX, RXN, RATT = Region("row_x", B, d, 0, d), Region("row_xn", B, d, 0, d), Region("row_att", B, d, 0, d)
            RQ, RH = Region("row_h", B, d, 0, d), Region("row_h", B, 4 * d, 0, 4 * d)

            def kv_fn(b, fault, l=l):
                inp = {"A": rd(b, XN), "W": b[p.lw(l, "attn.in_proj_weight")][d:3 * d], "bias": b[p.lw(l, "attn.in_proj_bias")].reshape(-1)[d:3 * d]}
                clean = TR.gemm_reference(inp, tier, TR.EPI_BIAS, w_exact=(p.split and p.w_grid))["out"]
                if fault == "kv_bias_no_offset":
                    inp["bias"] = b[p.lw(l, "attn.in_proj_bias")].reshape(-1)[:2 * d]
                return TR.gemm_reference(inp, tier, TR.EPI_BIAS, w_exact=(p.split and p.w_grid))["out"][0], clean[1]
            one(f"b{l}.kv", "launch_gemm(EPI_BIAS_F16", ["xn", p.lw(l, "attn.in_proj_weight"), p.lw(l, "attn.in_proj_bias")], KV, kv_fn,
                lambda b, l=l: _emu_acc(rd(b, XN), b[p.lw(l, "attn.in_proj_weight")][d:3 * d], b[p.lw(l, "attn.in_proj_bias")].reshape(-1)[d:3 * d]))
            for src, dst in ((X, RX), (XN, RXN)):
                def rows(b, fault, src=src):
                    at = rr
                    if fault == "eot_of_previous_class" and p.kind == 1:
                        at = torch.arange(B) * p.rs + torch.tensor(p.eot).roll(1)
                    return rd(b, src)[at].double(), torch.zeros(B, d, dtype=torch.float64)
                one(f"b{l}.gather_{dst.slot}", "launch_gather_rows4(", [src.slot, "in:eot"], dst, rows, lambda b, src=src: rd(b, src)[rr],
                    lambda b, src=src, dst=dst: {dst: view(b, src)[rr]}, copy=True)
            gemm(f"b{l}.q", TR.EPI_BIAS, RXN, p.lw(l, "attn.in_proj_weight"), RQ, bias=p.lw(l, "attn.in_proj_bias"), wrows=slice(0, d), tier=tier)

            def attn_row(b, fault):
                res = AR.attention_row(view(b, QKV), B, S, H, p.causal, row_index=(rr - torch.arange(B) * S), qrows=view(b, RQ))
                return res["out"], (TR.split_store(res["out"], AR.bound_exact(res)) if p.split else AR.bound_exact(res))
            one(f"b{l}.attention_row", "launch_attention_row_f32(", ["qkv", "row_h", "in:eot"], RATT, attn_row,
                lambda b: _emu_attention(view(b, QKV), B, S, H, p.causal, rows=(rr - torch.arange(B) * S), qrows=view(b, RQ)))
            gemm(f"b{l}.out_proj", TR.EPI_RESID, RATT, p.lw(l, "attn.out_proj.weight"), RX, bias=p.lw(l, "attn.out_proj.bias"), resid=RX, tier=tier)
            ln(f"b{l}.ln2", "launch_layernorm_f16(", RX, RXN, p.lw(l, "ln_2.weight"), p.lw(l, "ln_2.bias"))
            gemm(f"b{l}.c_fc", TR.EPI_GELU, RXN, p.lw(l, "mlp.c_fc.weight"), RH, bias=p.lw(l, "mlp.c_fc.bias"), tier=tier)
            gemm(f"b{l}.c_proj", TR.EPI_RESID, RH, p.lw(l, "mlp.c_proj.weight"), RX, bias=p.lw(l, "mlp.c_proj.bias"), resid=RX, tier=tier)
            break
        gemm(f"b{l}.qkv", TR.EPI_BIAS, XN, p.lw(l, "attn.in_proj_weight"), QKV, bias=p.lw(l, "attn.in_proj_bias"), tier=tier)

        def attn(b, fault):
            res = TR.attention_terms(view(b, QKV), B, S, H, p.causal)
            return res["out"], (TR.bound_attention_split(res) if p.split else TR.bound_attention_f32(res))
        one(f"b{l}.attention", "launch_attention_fwd_split(" if p.split else "launch_attention_fwd_f32(", ["qkv"], ATT, attn, lambda b: _emu_attention(view(b, QKV), B, S, H, p.causal))
        gemm(f"b{l}.out_proj", TR.EPI_RESID, ATT, p.lw(l, "attn.out_proj.weight"), X, bias=p.lw(l, "attn.out_proj.bias"), resid=X, tier=tier)
        ln(f"b{l}.ln2", "launch_layernorm_f16(", X, XN, p.lw(l, "ln_2.weight"), p.lw(l, "ln_2.bias"))
        gemm(f"b{l}.c_fc", TR.EPI_GELU, XN, p.lw(l, "mlp.c_fc.weight"), HID, bias=p.lw(l, "mlp.c_fc.bias"), tier=tier)
        gemm(f"b{l}.c_proj", TR.EPI_RESID, HID, p.lw(l, "mlp.c_proj.weight"), X, bias=p.lw(l, "mlp.c_proj.bias"), resid=X, tier=tier)
    CLS = Region("cls16", B, d, 0, d)
    ln("ln_post", "launch_gather_ln_f16(", Region("row_x", B, d, 0, d), CLS, p.final("weight"), p.final("bias"))
    gemm("projection", TR.EPI_F32, CLS, "w:proj#T" if p.kind == 0 else "w:text_projection#T", Region("out:emb", B, E, 0, E))
    return out


def _saved_o_full(res, qkv, d_out, o_saved, B, S, H, causal):
    """attention_ref forms delta_i = dO_i . O_i from ITS OWN float64 output; a backward launch of a tower pass reads the O the forward SAVED (att_l), which
    carries the forward kernel's error.  The value of the operation on the buffers the launch read is therefore the reference's with
    dS_ij -= p_ij dO_i . (O_saved - O)_i: dq and dk move, dv does not.  The bounds stay those of attention_ref (they allow one f16 rounding of an exact O)."""
    q, k, v = AR.unpack(qkv, B, S, H)
    vis = torch.ones(S, S, dtype=torch.bool).tril() if causal else torch.ones(S, S, dtype=torch.bool)
    pr = torch.softmax((q @ k.transpose(-1, -2) / 8.0).masked_fill(~vis, float("-inf")), -1)
    delta = (AR.heads(d_out, B, S, H) * (AR.heads(o_saved, B, S, H) - AR.heads(res["out"], B, S, H))).sum(-1, keepdim=True)
    adj = pr * delta
    return res["dq"] - AR.rows(adj @ k / 8.0), res["dk"] - AR.rows(adj.transpose(-1, -2) @ q / 8.0), res["dv"]


def _q_eighth_terms(qkv, d_out, B, S, H, causal):
    """What attention_ref's count leaves out of attn_bwd_kernel: the kernel forms Q / 8 IN f16 before both of its uses (`q *= (half_t)0.125f`).  That is
    exact while q / 8 is a normal f16 number and one rounding onto the subnormal grid, 2^-25 absolute, where |q| < 2^-11.  Through dK_jd = sum_i dS_ij
    (q_id / 8) it is 2^-25 sum_i |dS_ij| [|q_id| < 2^-11]: nothing at unit-size gradients, visible under a loss scale that puts |dS| in the tens.  Through
    the scores it is eps_i = 2^-25 sum_d [|q_id| < 2^-11] |k_jd| absolute in an exponent, at most r = 2 max eps relative in a probability (numerator and
    row sum), which dS = p (dP - delta) carries as r (|dS| + p Gbar) and dV as r p |dO|.  -> (the dK term [B*S, D], r)."""
    q, k, v = AR.unpack(qkv, B, S, H)
    vis = torch.ones(S, S, dtype=torch.bool).tril() if causal else torch.ones(S, S, dtype=torch.bool)
    pr = torch.softmax((q @ k.transpose(-1, -2) / 8.0).masked_fill(~vis, float("-inf")), -1)
    dp = AR.heads(d_out, B, S, H) @ v.transpose(-1, -2)
    ds = pr * (dp - (pr * dp).sum(-1, keepdim=True))
    sub = (q.abs() < 2.0 ** -11).double()
    return AR.SUB16 * AR.rows(ds.abs().transpose(-1, -2) @ sub), 2 * AR.SUB16 * float((sub @ k.abs().transpose(-1, -2)).max())


def _bwd_mfma_bound(res, kind, extra_k, r):
    b = {x: AR.bound(res, x, kind) + r * res["scale_" + x] for x in "qkv"}
    for x in "qk":
        b[x] = b[x] + r * res["scale2_" + x]
    b["k"] = b["k"] + extra_k
    return torch.cat([b[x] for x in "qkv"], 1)


def _saved_o_row(res, qkv, do_rows, o_saved, B, S, H, causal, r):
    """The same for the one-row backward: query row r[b] of sequence b alone."""
    q, k, _ = AR.unpack(qkv, B, S, H)
    ar = torch.arange(B)
    qr = q[ar, :, r]                                                                     # [B, H, 64]
    vis = (torch.arange(S)[None] <= r[:, None]) if causal else torch.ones(B, S, dtype=torch.bool)
    pr = torch.softmax((torch.einsum("bhd,bhjd->bhj", qr, k) / 8.0).masked_fill(~vis[:, None], float("-inf")), -1)
    delta = (do_rows.double().reshape(B, H, 64) * (o_saved.double() - res["out"]).reshape(B, H, 64)).sum(-1)      # [B, H]
    adj = pr * delta[..., None]                                                          # [B, H, S]
    full = torch.zeros(B, H, S, 64, dtype=torch.float64)
    full[ar, :, r] = torch.einsum("bhj,bhjd->bhd", adj, k) / 8.0
    return res["dq"] - AR.rows(full), res["dk"] - AR.rows(adj[..., None] * qr[:, :, None, :] / 8.0), res["dv"]


def pick_ksplit(M, N, K):
    """The split factor of an EPI_F32 input-gradient GEMM with default tuning (csrc/gemm_plan.cpp gemm_pick_ksplit restated: 64 x 128 tiles, 64-wide K slices;
    tests/test_gpu_tower_passes.py holds it to the partial buffers the carve-up reserves)."""
    cdiv = lambda a, b: (a + b - 1) // b          # noqa: E731
    tiles, nk = cdiv(M, 64) * (N // 128), K // 64
    if tiles >= 512:
        return 1
    t128 = cdiv(M, 128) * (N // 128)
    if tiles > 256 and t128 <= 256:
        f128 = 1
        for f in (2, 3, 4):
            if nk % f == 0 and nk // f >= 8 and t128 * f <= 512:
                f128 = f
        if f128 > 1:
            return f128
    best, t32 = 1, cdiv(M, 32) * (N // 128)
    for f in (2, 3, 4, 6, 8):
        if nk % f or nk // f < 3:
            continue
        best = f
        wgs = t32 * f if (tiles * f <= 128 and t32 * f <= 256) else tiles * f
        if nk // f >= 4 and wgs >= 224:
            break
    return best


def backward_steps(p):
    """The launches of the backward of a train-mode forward (grip_vit_backward_prefix / _deep, grip_text_backward_prefix / _deep), in order.  The pass
    differentiates dL / d(embedding) = in:grad_emb down to the prompt rows: the loss scale (grad_scale_cast), the projection, ln_post at the read rows,
    then per block from the last to the first  d h_pre = (dx W_proj) QuickGELU'(h_pre),  dx += LNbwd(d h_pre W_fc; x_mid),  d att = dx W_out,
    d qkv = attention backward,  dx += LNbwd(d qkv W_in; x_in), the split-K partial products summed inside the LayerNorm backward; before block l's
    backward the rows a deep prompt replaced give grad_deep[l] and are zeroed; at the end the prompt rows of dx give grad_prefix (the vision tower through
    ln_pre), times the inverse loss scale.  The last block of the plain layout ran for the read rows alone and so does its backward (drow, row_*)."""
    import rowops_ref as RR
    assert p.train
    d, B, S, M, P, H, E, L = p.d, p.B, p.S, p.M, p.P, p.H, p.E, p.layers
    Mp, Bp = (M + 255) // 256 * 256, (B + 255) // 256 * 256
    ks_fc, ks_in, ks_row = pick_ksplit(M, d, 4 * d), pick_ksplit(M, d, 3 * d), pick_ksplit(B, d, 4 * d)
    out = []
    rr = p.read_rows()
    index = None if p.kind == 0 else torch.tensor(p.eot, dtype=torch.long)
    DX, DXH = Region("dx", M, d, 0, d), Region("dxh", M, d, 0, d)
    DROW, DROWH = Region("drow", B, d, 0, d), Region("drow_h", B, d, 0, d)
    hb = lambda v, e: e + FR.half_bound(v, e)          # noqa: E731
    Z = lambda *sh: torch.zeros(*sh, dtype=torch.float64)          # noqa: E731

    def step(label, call, owns, fn, exact=None, free=()):
        """fn(before, fault) -> {Region: (value, bound)}; `free`: owned scratch regions whose content is the kernel's own business."""
        def ref(before, after, fault=None):
            v = fn(before, fault)
            v0 = fn(before, None) if fault else v
            return {f"{r.slot}@{r.row0}": (view(after, r), v[r][0], v0[r][1]) for r in v}

        def emu(before):
            res = {r: store(val, r.slot, is64(before)) for r, (val, _) in fn(before, None).items()}
            res.update({r: torch.zeros(r.rows, r.ncols, dtype=torch.float64 if is64(before) else torch.float32) for r in free})
            return res
        out.append(Step("bwd." + label, call, (), tuple(owns) + tuple(free), ref, exact, emu))

    def gemm(label, epi, call, a, w, o, aux=None):
        def fn(b, fault):
            inp = {"A": view(b, a), "W": b[w]}
            if aux is not None:
                inp["aux"] = view(b, aux)
            return {o: G.reference(inp, epi)["out"]}
        step(label, "launch_gemm(" + call, [o], fn)

    def parts(slot, rows, pad, ks):
        return [Region(slot, rows, d, 0, d, row0=q * pad) for q in range(ks)]

    def splitk(label, a, w, slot, rows, pad, ks):
        """EPI_F32 split-K: ks partial [rows, d] products, `pad` rows apart; their sum is the product (each partial's own K range is the launcher's business)."""
        regs = parts(slot, rows, pad, ks)

        def ref(before, after, fault=None):
            v, e = G.reference({"A": view(before, a), "W": before[w]}, G.EPI_F32)["out"]
            return {"sum of the partials": (sum(view(after, r).double() for r in regs), v, e)}

        def emu(before):
            v = G.reference({"A": view(before, a), "W": before[w]}, G.EPI_F32)["out"][0]
            res = {r: torch.zeros(rows, d, dtype=v.dtype if is64(before) else torch.float32) for r in regs[1:]}
            res[regs[0]] = store(v, slot, is64(before))
            return res
        out.append(Step("bwd." + label, "launch_gemm(EPI_F32", (), tuple(regs), ref, None, emu))

    def dyp(b, slot, rows, pad, ks):
        return torch.stack([view(b, r) for r in parts(slot, rows, pad, ks)])

    # -------------------------------------------------------------------------------------------- head of the tower
    GE, SC, DCLS = Region("gemb16", B, E, 0, E), Region("scale", 1, 2, 0, 2), Region("dcls", B, d, 0, d)

    def cast(b, fault):
        g = b["in:grad_emb"].view(B, E).double()
        s0, s1, _ = RR.grad_scale_cast(g)
        return {GE: (g * s0, FR.half_bound(g * s0, 0.0)), SC: (torch.tensor([[s0, s1]], dtype=torch.float64), Z(1, 2))}
    step("grad_scale_cast", "launch_grad_scale_cast(", [GE, SC], cast,
         lambda b: {GE: RR.grad_scale_cast(b["in:grad_emb"].view(B, E))[2]})
    gemm("projection", G.EPI_F32, "EPI_F32", GE, "w:proj" if p.kind == 0 else "w:text_projection", DCLS)
    gpost = p.final("weight")
    if p.rows_only:
        ROUT = Region("row_xout", B, d, 0, d)

        def post(b, fault):
            v, e = RR.ln_bwd(view(b, ROUT), view(b, DCLS)[None], b[gpost].reshape(-1))
            return {DROW: (v, e), DROWH: (v, hb(v, e))}
        step("ln_post", "launch_ln_bwd_scatter(", [DROW, DROWH], post)
    else:
        XL = Region(f"x_in.{L}", M, d, 0, d)

        def post_fill(b, fault):
            v, e, _ = RR.ln_bwd_scatter(view(b, XL), view(b, DCLS), b[gpost].reshape(-1), index, p.rs, M)
            return {DX: (v, e), DXH: (v, hb(v, e))}
        step("ln_post", "launch_ln_bwd_scatter_fill(", [DX, DXH], post_fill)

    # -------------------------------------------------------------------------------------------- blocks, last to first
    def deep_grad(l):
        """Before block l's backward dx is the gradient of x_in[l + 1], whose rows 1 .. P the forward overwrote with deep[l]."""
        dc = p.prefix_classes if p.kind else 1
        GD = Region("out:grad_deep", dc * P, d, 0, d, row0=l * dc * P)
        if p.Ps:
            rows = 1 + torch.arange(P)
        else:
            rows = (torch.arange(B)[:, None] * S + 1 + torch.arange(P)[None]).reshape(-1)

        def fn(b, fault):
            dx, inv = view(b, DX).double(), float(view(b, SC)[0, 1])
            f = "skip_image" if fault == "grad_deep_one_image_short" else None
            if p.kind == 0:
                g, e = RR.vit_prefix_grad(dx, None, None, inv, B, S, P, 2, f)
                g0e = RR.vit_prefix_grad(dx, None, None, inv, B, S, P, 2)[1]
            elif p.Ps:
                g, e = RR.text_prefix_grad(dx[:S], inv, 1, S, P, 1)
                g0e = e
            else:
                g, e = RR.text_prefix_grad(dx, inv, B, S, P, dc, f)
                g0e = RR.text_prefix_grad(dx, inv, B, S, P, dc)[1]
            z = dx.clone()
            z[rows] = 0
            return {GD: (g.reshape(-1, d), g0e.reshape(-1, d)), DX: (z, Z(M, d)), DXH: (_zero_rows(view(b, DXH).double(), rows), Z(M, d))}
        step(f"b{l}.deep_grad", "launch_vit_deep_grad(" if p.kind == 0 else "launch_text_deep_grad(", [GD, DX, DXH], fn)

    def _zero_rows(t, rows):
        t = t.clone()
        t[rows] = 0
        return t

    for l in range(L - 1, -1, -1):
        w = lambda n: p.lw(l, n)          # noqa: E731
        if l + 1 <= p.n_deep:
            deep_grad(l)
        QL = Region(f"qkv_l.{l}", M, 3 * d, 0, 3 * d)
        DQKV = Region("dqkv", M, 3 * d, 0, 3 * d)
        XI = Region(f"x_in.{l}", M, d, 0, d)
        if l == L - 1 and p.rows_only:
            RDH, RDATT, RMID = Region("row_dh", B, 4 * d, 0, 4 * d), Region("row_datt", B, d, 0, d), Region("row_xmid", B, d, 0, d)
            gemm(f"b{l}.gelu_grad", G.EPI_GELUGRAD_F16, "EPI_GELUGRAD_F16", DROWH, w("mlp.c_proj.weight#T"), RDH, aux=Region("row_hpre", B, 4 * d, 0, 4 * d))
            splitk(f"b{l}.c_fc_dgrad", RDH, w("mlp.c_fc.weight#T"), "row_dln", B, Bp, ks_row)

            def add2(b, fault, l=l, RMID=RMID):
                v, e = RR.ln_bwd_add(view(b, RMID), dyp(b, "row_dln", B, Bp, ks_row), b[p.lw(l, "ln_2.weight")].reshape(-1), view(b, DROW))
                return {DROW: (v, e), DROWH: (v, hb(v, e))}
            step(f"b{l}.ln2_bwd", "launch_ln_bwd_add(", [DROW, DROWH], add2)
            gemm(f"b{l}.out_proj_dgrad", G.EPI_F16, "EPI_F16", DROWH, w("attn.out_proj.weight#T"), RDATT)

            def row_bwd(b, fault, QL=QL, RDATT=RDATT):
                r = rr - torch.arange(B) * S
                res = AR.attention_row(view(b, QL), B, S, H, p.causal, row_index=r, do_rows=view(b, RDATT))
                vals = _saved_o_row(res, view(b, QL), view(b, RDATT), view(b, Region("row_att", B, d, 0, d)), B, S, H, p.causal, r)
                return {DQKV: (torch.cat(vals, 1), torch.cat([AR.bound(res, x, "bwd_row") for x in "qkv"], 1))}
            step(f"b{l}.attention_row_bwd", "launch_attention_row_bwd(", [DQKV], row_bwd)
            splitk(f"b{l}.qkv_dgrad", DQKV, w("attn.in_proj_weight#T"), "dln", M, Mp, ks_in)

            def init(b, fault, l=l, XI=XI):
                v, e = RR.ln_bwd_init(view(b, XI), dyp(b, "dln", M, Mp, ks_in), b[p.lw(l, "ln_1.weight")].reshape(-1), view(b, DROW), index, S)
                return {DX: (v, e), DXH: (v, hb(v, e))}
            step(f"b{l}.ln1_bwd", "launch_ln_bwd_init(", [DX, DXH], init)
            continue
        DH, DATT, XM = Region("dh", M, 4 * d, 0, 4 * d), Region("datt", M, d, 0, d), Region(f"x_mid.{l}", M, d, 0, d)
        gemm(f"b{l}.gelu_grad", G.EPI_GELUGRAD_F16, "EPI_GELUGRAD_F16", DXH, w("mlp.c_proj.weight#T"), DH, aux=Region(f"hpre_l.{l}", M, 4 * d, 0, 4 * d))
        splitk(f"b{l}.c_fc_dgrad", DH, w("mlp.c_fc.weight#T"), "dln", M, Mp, ks_fc)

        def add_mid(b, fault, l=l, XM=XM):
            v, e = RR.ln_bwd_add(view(b, XM), dyp(b, "dln", M, Mp, ks_fc), b[p.lw(l, "ln_2.weight")].reshape(-1), view(b, DX))
            return {DX: (v, e), DXH: (v, hb(v, e))}
        step(f"b{l}.ln2_bwd", "launch_ln_bwd_add(", [DX, DXH], add_mid)
        gemm(f"b{l}.out_proj_dgrad", G.EPI_F16, "EPI_F16", DXH, w("attn.out_proj.weight#T"), DATT)

        def att_bwd(b, fault, QL=QL, DATT=DATT, l=l):
            o_saved = view(b, Region(f"att_l.{l}", M, d, 0, d))
            if p.Ps:          # the plain reference on the expanded rows, as attention_ref.attention_shared does: the shared query rows are sequence 0's
                res, kind = AR.attention_shared(view(b, QL), B, S, H, p.Ps, view(b, DATT)), "bwd_shared"
                do = AR.from_shared(view(b, DATT).double(), B, S, p.Ps).reshape(B, S, -1).clone()
                do[1:, :p.Ps] = 0
                full = AR.attention(AR.from_shared(view(b, QL), B, S, p.Ps), B, S, H, 1, do.reshape(B * S, -1))
                vals = _saved_o_full(full, AR.from_shared(view(b, QL), B, S, p.Ps), do.reshape(B * S, -1), AR.from_shared(o_saved.double(), B, S, p.Ps), B, S, H, 1)
                vals = tuple(AR.to_shared(v, B, S, p.Ps, f) for v, f in zip(vals, ("first", "sum", "sum")))
                extra_k, r = _q_eighth_terms(AR.from_shared(view(b, QL), B, S, p.Ps), do.reshape(B * S, -1), B, S, H, 1)
                extra_k = AR.to_shared(extra_k, B, S, p.Ps, "sum")
            else:
                res, kind = AR.attention(view(b, QL), B, S, H, p.causal, view(b, DATT)), "bwd_mfma"
                vals = _saved_o_full(res, view(b, QL), view(b, DATT), o_saved, B, S, H, p.causal)
                extra_k, r = _q_eighth_terms(view(b, QL), view(b, DATT), B, S, H, p.causal)
            return {DQKV: (torch.cat(vals, 1), _bwd_mfma_bound(res, kind, extra_k, r))}
        step(f"b{l}.attention_bwd", "launch_attention_bwd(", [DQKV], att_bwd,
             free=[Region("kv_part", B * p.Ps * 2, d, 0, d)] if p.Ps else [])
        splitk(f"b{l}.qkv_dgrad", DQKV, w("attn.in_proj_weight#T"), "dln", M, Mp, ks_in)

        def add_in(b, fault, l=l, XI=XI):
            v, e = RR.ln_bwd_add(view(b, XI), dyp(b, "dln", M, Mp, ks_in), b[p.lw(l, "ln_1.weight")].reshape(-1), view(b, DX))
            return {DX: (v, e), DXH: (v, hb(v, e))}
        step(f"b{l}.ln1_bwd", "launch_ln_bwd_add(", [DX, DXH], add_in)

    # -------------------------------------------------------------------------------------------- the prompt rows
    pc = (B if p.per_image else 1) if p.kind == 0 else p.prefix_classes
    GP = Region("out:grad_prefix", pc * P, d, 0, d)

    def prefix_grad(b, fault):
        dx = view(b, DX).double()
        inv = 1.0 if fault == "loss_scale_not_undone" else float(view(b, SC)[0, 1])
        inv0 = float(view(b, SC)[0, 1])
        if p.kind == 0:
            args = (b["in:prefix"].view(-1, d).double(), b["w:ln_pre.weight"].reshape(-1))
            g = RR.vit_prefix_grad(dx, *args, inv, B, S, P, 1 if p.per_image else 0)[0]
            e = RR.vit_prefix_grad(dx, *args, inv0, B, S, P, 1 if p.per_image else 0)[1]
        elif p.Ps:
            g, e = RR.text_prefix_grad(dx[:S], inv, 1, S, P, 1)[0], RR.text_prefix_grad(dx[:S], inv0, 1, S, P, 1)[1]
        else:
            g, e = RR.text_prefix_grad(dx, inv, B, S, P, pc)[0], RR.text_prefix_grad(dx, inv0, B, S, P, pc)[1]
        return {GP: (g.reshape(-1, d), e.reshape(-1, d))}
    call = ("launch_vit_prefix_grad_per_image(" if p.per_image else "launch_vit_prefix_grad(") if p.kind == 0 else "launch_text_prefix_grad("
    step("prefix_grad", call, [GP], prefix_grad)
    return out


# fault -> (label of the step it is an error of (first match by suffix), the passes that have the edge it needs: elsewhere the fault is the identity)
FAULT_SITES = {
    "ln2_gamma_for_ln1": (("b0.qkv", "b0.ln1"), lambda p: True),
    "kv_bias_no_offset": (".kv", lambda p: p.rows_only and not p.train),          # (a train-mode last block forms Q, K and V in one GEMM)
    "colsum_q_for_k": (".kv", lambda p: p.rows_only and not p.f32 and not p.train),
    "stats_row_minus_256": ("b1.qkv", lambda p: p.M > 256 and not p.f32),
    "deep_one_block_late": ("b1.deep_insert", lambda p: p.n_deep > 0),
    "deep_image0_only": ("b1.deep_insert", lambda p: p.n_deep > 0 and p.kind == 0 and p.B > 1),
    "eot_of_previous_class": (".gather_row_x", lambda p: p.kind == 1 and p.rows_only and len(set(p.eot)) > 1),
    "shared_row_map_off_by_one_class": ("ln_post", lambda p: p.Ps > 0 and p.B > 1),
    "prompt_rows_shifted": (("assemble", "embed"), lambda p: p.P > 1),
    "pos_under_no_pos": (("assemble", "embed"), lambda p: p.no_pos),
    "hilo_lo_dropped": ("b0.out_proj", lambda p: p.hilo),
    "c_proj_resid_from_x_in": ("b0.c_proj", lambda p: p.train),
    "ln_post_beta_dropped": ("ln_post", lambda p: True),
    # the backward (backward_steps)
    "grad_deep_one_image_short": ("bwd.b0.deep_grad", lambda p: p.train and p.n_deep > 0 and not p.Ps and p.B > 1 and (p.kind == 0 or p.prefix_classes == 1)),
    "loss_scale_not_undone": ("bwd.prefix_grad", lambda p: p.train),
}
FAULTS = tuple(FAULT_SITES)


def all_steps(p):
    """Forward, then (train mode) backward: the order the host chains run them in."""
    return steps(p) + (backward_steps(p) if p.train else [])


def fault_step(p, sched, fault):
    site, has_edge = FAULT_SITES[fault]
    sites = (site,) if isinstance(site, str) else site
    hit = [i for i, s in enumerate(sched) if any(s.label == t or (t.startswith(".") and s.label.endswith(t)) for t in sites)]
    return (hit[0] if hit else None), has_edge(p)


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def worst_ratio(got, value, bound):
    err = (got.double() - value).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ weights and inputs of the host chains
FAMILIES = ("randn", "outlier")


def weight_shapes(p):
    """{layout slot name: (rows, cols, f16?)} of the primary weights of the pass's tower, by the names grip_layout_slot gives them."""
    d, E = p.d, p.E
    sh = {}
    if p.kind == 0:
        sh.update({"conv1.weight": (d, p.kpad, 1), "class_embedding": (1, d, 0), "positional_embedding": (p.seq0, d, 0), "ln_pre.weight": (1, d, 0),
                   "ln_pre.bias": (1, d, 0)})
    else:
        sh.update({"token_embedding.weight": (p.vocab, d, 0), "positional_embedding": (p.seq0, d, 0)})
    for l in range(p.layers):
        pre = f"transformer.resblocks.{l}."
        sh.update({pre + "ln_1.weight": (1, d, 0), pre + "ln_1.bias": (1, d, 0), pre + "attn.in_proj_weight": (3 * d, d, 1), pre + "attn.in_proj_bias": (1, 3 * d, 0),
                   pre + "attn.out_proj.weight": (d, d, 1), pre + "attn.out_proj.bias": (1, d, 0), pre + "ln_2.weight": (1, d, 0), pre + "ln_2.bias": (1, d, 0),
                   pre + "mlp.c_fc.weight": (4 * d, d, 1), pre + "mlp.c_fc.bias": (1, 4 * d, 0), pre + "mlp.c_proj.weight": (d, 4 * d, 1),
                   pre + "mlp.c_proj.bias": (1, d, 0)})
    fin = "ln_post" if p.kind == 0 else "ln_final"
    sh.update({fin + ".weight": (1, d, 0), fin + ".bias": (1, d, 0), ("proj" if p.kind == 0 else "text_projection"): (d, E, 1)})
    return sh


OUTLIER_CHANNELS = (3, 40, 77, 126)


def make_weights(p, family, seed=5):
    """Primary weights {name: float32 [rows, cols]} (f16 operands already on the f16 grid) from grip_amd.rng.  randn: matrices at K^-1/2, LayerNorm gamma
    +-2^U(-2, 2) (a factor of 16, mixed signs), biases and beta 0.5 randn.  outlier: the same with four stream channels at |x| ~ 50 (ln_pre beta /
    the positional embedding), so that the folded acc - colsum mean cancels hard."""
    import grip_amd  # noqa: F401
    from grip_amd import rng
    w = {}
    for name, (rows, cols, f16) in weight_shapes(p).items():
        sid = rng.stream_id("tower_passes." + name)
        if name.endswith(("ln_1.weight", "ln_2.weight", "ln_pre.weight", "ln_post.weight", "ln_final.weight")):
            mag = torch.from_numpy(rng.uniform_range(seed, sid, (rows, cols), -2.0, 2.0)).float()
            sign = torch.from_numpy(rng.uniform_range(seed + 1, sid, (rows, cols), -1.0, 1.0)).float().sign()
            t = sign * 2.0 ** mag
        elif f16:
            k = 3 * p.patch * p.patch if name == "conv1.weight" else (rows if name in ("proj", "text_projection") else cols)
            t = torch.from_numpy(rng.normal(seed, sid, (rows, cols))).float() * k ** -0.5
            if name == "conv1.weight":
                t[:, 3 * p.patch * p.patch:] = 0          # the padding columns of the patch operand
            t = t if (p.f32 and not p.w_grid) else t.half().float()          # an exact tower's operands are f32 numbers off the f16 grid (w_grid: on it)
        elif name in ("class_embedding", "positional_embedding", "token_embedding.weight"):
            t = torch.from_numpy(rng.normal(seed, sid, (rows, cols))).float()
        else:
            t = 0.5 * torch.from_numpy(rng.normal(seed, sid, (rows, cols))).float()
        w[name] = t.contiguous()
    if family == "outlier":
        ch = list(OUTLIER_CHANNELS)
        signs = torch.tensor([50.0, -50.0, 50.0, -50.0])
        if p.kind == 0:
            w["ln_pre.bias"][0, ch] = signs
        else:
            w["positional_embedding"][:, ch] += signs
    return w


def derive(w, p, exact):
    """The derived slots grip_tower_finalize writes, {"w:" + name: tensor}.  exact: float64, nothing rounded (the float64 chain); else as the kernels
    produce them up to their own (separately tested) rounding: W' = f16(gamma o W), colsum of the rounded W', W beta + b, and the transposed projection."""
    out = {}
    for name, t in w.items():
        f16 = weight_shapes(p)[name][2]
        out["w:" + name] = t.double() if exact else (t.half() if (f16 and not p.f32) else t.float())
    for l in range(0 if p.f32 else p.layers):
        pre = f"transformer.resblocks.{l}."
        for W, g, b, bias, stem in ((pre + "attn.in_proj_weight", pre + "ln_1.weight", pre + "ln_1.bias", pre + "attn.in_proj_bias", pre + "attn.in_proj"),
                                    (pre + "mlp.c_fc.weight", pre + "ln_2.weight", pre + "ln_2.bias", pre + "mlp.c_fc.bias", pre + "mlp.c_fc")):
            if exact:
                Wg = w[g].double().reshape(1, -1) * w[W].double()
                cs, bo = Wg.sum(-1), w[bias].double().reshape(-1) + w[W].double() @ w[b].double().reshape(-1)
            else:
                Wg, (cs, _), (bo, _) = FR.fold_weights(w[W].half(), w[g].reshape(-1), w[b].reshape(-1), w[bias].reshape(-1))
                cs, bo = cs.float(), bo.float()
            out["w:" + W + "#G"], out["w:" + stem + "#colsum"], out["w:" + stem + "#bias"] = Wg, cs.reshape(1, -1), bo.reshape(1, -1)
    pj = "proj" if p.kind == 0 else "text_projection"
    out[f"w:{pj}#T"] = out["w:" + pj].T.contiguous()
    if p.train:          # the transposed block weights the input-gradient GEMMs read
        for l in range(p.layers):
            for n in ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight"):
                out[p.lw(l, n) + "#T"] = out[p.lw(l, n)].T.contiguous()
    return out


def make_inputs(p, seed=9):
    """The call's arguments {"in:...": float32 / int tensors}: images, prompts at 0.5 randn (LayerNorm sees them raw in the text tower), deep prompts, token ids."""
    import grip_amd  # noqa: F401
    from grip_amd import rng
    n = lambda name, shape, std=1.0: torch.from_numpy(rng.normal(seed, rng.stream_id("tower_passes.in." + name), shape, 0.0, std)).float().contiguous()  # noqa: E731
    inp = {}
    if p.kind == 0:
        inp["in:images"] = n("images", (p.B, 3, p.resolution, p.resolution)).reshape(-1)
        if p.P:
            inp["in:prefix"] = n("prefix", (p.B if p.per_image else 1, p.P, p.d), 0.5).reshape(-1)
    else:
        ids = torch.from_numpy(rng.integers(seed, rng.stream_id("tower_passes.in.ids"), (p.B, p.seq0), 0, p.vocab)).to(torch.int32)
        if p.Ps:
            ids[:, :p.Ps] = ids[0, :p.Ps].clone()          # the caller vouches for identical tokens at positions 0 .. P
        inp["in:ids"] = ids.reshape(-1).contiguous()
        inp["in:eot"] = torch.tensor(p.eot, dtype=torch.int32)
        if p.P:
            inp["in:prefix"] = n("prefix", (p.prefix_classes, p.P, p.d), 0.5).reshape(-1)
    if p.train:          # dL / d(embedding) of a loss at 1e-3: the loss scale is 2^k with k > 0, so a scale that is not undone shows
        inp["in:grad_emb"] = n("grad_emb", (p.B, p.E), 1e-3).reshape(-1)
    if p.n_deep:
        inp["in:deep"] = n("deep", (p.n_deep, p.prefix_classes if p.kind else 1, p.P, p.d), 0.5).reshape(-1)
    return inp


def empty_buffers(p, sched, like64):
    """Zero-size-exact host buffers for every region the schedule owns (the host chains; the GPU test views the workspace instead)."""
    size = {}
    for s in sched:
        for r in s.owns:
            size[r.slot] = max(size.get(r.slot, 0), (r.row0 + r.rows) * r.ld)
    return {slot: torch.full((n,), float("nan"), dtype=torch.float64 if like64 else (torch.float16 if p.is16(slot) else torch.float32)) for slot, n in size.items()}


def write(bufs, region, value):
    view(bufs, region).copy_(value)


# ------------------------------------------------------------------------------------------------ the required passes
def vision_cases():
    base = dict(kind=0, width=128, layers=3, embed_dim=128)
    cases = [Pass(batch=B, P=P, **base) for P in (0, 3) for B in (1, 3, 16)]
    cases += [Pass(batch=3, P=3, hilo=True, **base), Pass(batch=3, P=0, no_pos=True, **base), Pass(batch=3, P=3, per_image=True, **base),
              Pass(batch=3, P=3, n_deep=2, **base), Pass(batch=3, P=3, n_deep=2, hilo=True, **base)]
    return cases


def text_cases():
    base = dict(kind=1, width=128, layers=3, embed_dim=128, vocab=64, seq0=16)
    eot5, cases = [7, 11, 5, 9, 11], []
    for C in (1, 5):
        eot = eot5[:C]
        for pc in sorted({1, C}):
            for n_deep in (0, 2):
                cases.append(Pass(batch=C, P=3, eot=eot, seq_len=max(eot) + 1, prefix_classes=pc, n_deep=n_deep, **base))
                if pc == 1:
                    cases.append(Pass(batch=C, P=3, eot=eot, seq_len=max(eot) + 1, prefix_classes=1, n_deep=n_deep, shared=True, **base))
    cases.append(Pass(batch=5, P=0, eot=eot5, seq_len=12, **base))
    cases.append(Pass(batch=5, P=3, eot=[7, 15, 5, 9, 11], seq_len=0, **base))          # the untruncated sequence
    cases.append(Pass(batch=5, P=3, eot=eot5, seq_len=12, no_pos=True, **base))
    return cases


def split_cases():
    """The split-f16 tower (width 256: its GEMM tiles are 256 x 256): vision on f32-valued weights and on f16-grid weights (w_exact 0 and 1), and the exact
    text features the screen uses."""
    vis = dict(kind=0, width=256, layers=3, embed_dim=128, precision=2, batch=3)
    txt = dict(kind=1, width=256, layers=3, embed_dim=128, vocab=64, seq0=16, precision=2, batch=5, P=3, eot=[7, 11, 5, 9, 11], seq_len=12)
    return [Pass(P=P, w_grid=g, **vis) for P in (0, 3) for g in (False, True)] + [Pass(**txt), Pass(w_grid=True, prefix_classes=5, n_deep=2, **txt)]


def f32_cases():
    vis = dict(kind=0, width=128, layers=3, embed_dim=128, precision=1)
    txt = dict(kind=1, width=128, layers=3, embed_dim=128, vocab=64, seq0=16, precision=1)
    return [Pass(batch=3, P=0, **vis), Pass(batch=3, P=3, **vis), Pass(batch=3, P=3, n_deep=2, **vis),
            Pass(batch=5, P=3, eot=[7, 11, 5, 9, 11], seq_len=12, **txt), Pass(batch=5, P=3, eot=[7, 11, 5, 9, 11], seq_len=12, prefix_classes=5, n_deep=2, **txt)]


def train_cases():
    vis = dict(kind=0, width=128, layers=3, embed_dim=128, train=True)
    txt = dict(kind=1, width=128, layers=3, embed_dim=128, vocab=64, seq0=16, train=True, eot=[7, 11, 5, 9, 11], seq_len=12)
    cases = [Pass(batch=3, P=3, n_deep=n, **vis) for n in (0, 2)] + [Pass(batch=3, P=3, per_image=True, **vis), Pass(batch=16, P=3, **vis)]
    for pc in (1, 5):
        for n in (0, 2):
            cases.append(Pass(batch=5, P=3, prefix_classes=pc, n_deep=n, **txt))
            if pc == 1:
                cases.append(Pass(batch=5, P=3, prefix_classes=1, n_deep=n, shared=True, **txt))
    # cooperative split-K of c_proj: no M has it at width 128 (K = 512 is 8 slices, the form needs 16); width 256 is the smallest width that does, for every
    # M up to 64 tiles, with factor 4 (tests/test_host_tower_ref.py asserts both against grip_debug_coop_split).  The shared layout keeps a full last block.
    wide = dict(txt, width=256, coop_ks=4)
    cases += [Pass(batch=5, P=3, **wide), Pass(batch=5, P=3, shared=True, n_deep=2, **wide)]
    return cases


CASES = vision_cases() + text_cases() + f32_cases() + split_cases() + train_cases()
