"""Float64 attention on the values a kernel is given (head dim 64, scores scaled by 1/8), with out, dQ, dK, dV in closed form and, per output
element, the float64 sums of absolute terms that the element-wise error bounds of tests/test_gpu_attention_kernels.py are built from (DESIGN.md,
"Attention kernel tests").  Plain helper module: no fixtures, runs on whatever device its inputs live on.

Layouts: qkv [B*S, 3*D] (D = H*64, columns [q | k | v]), out / d_out [B*S, D].  The shared-prefix layout of the text tower (csrc/common.h seq_row) holds
the first Ps positions once and then the S - Ps own positions of every sequence: Ps + B (S - Ps) rows.

Every result is a dict.  Values: out, dq, dk, dv.  Sums (same shape as the value they bound):
  scale_o = sum_j p_j |v_j|          scale_v = sum_i p_ij |dO_i|
  scale_k = sum_i |dS_ij| |q_i| / 8  scale_q = sum_j |dS_ij| |k_j| / 8
  scale2_k / scale2_q: the same with |dS_ij| replaced by T_ij = p_ij (C1 G_ij + (1 + C1) Gbar_i), the error of dS_ij that does NOT shrink with dS_ij itself:
      G_ij = sum_d |dO_id| |v_jd| (f32 accumulation of dP over 64 dims, C1 = 66 * 2^-13 in units of 2^-11) and Gbar_i = sum_j p_ij G_ij (delta_i = dO_i . O_i
      with O saved in f16: one 2^-11 per term, plus its own f32 accumulation)
  sub_o, sub_q, sub_k, sub_v: sum of the |co-factors| of the f16-rounded intermediates (P, dS), for the f16 subnormal quantum (2^-25 absolute per rounding)
and `A` = the largest sum_d |q_d k_d| / 8 over visible (query, key) pairs, `S`."""
import torch

U16 = 2.0 ** -11          # unit roundoff of f16 (round to nearest), normal numbers
SUB16 = 2.0 ** -25        # half the spacing of f16 below 2^-14
U32 = 2.0 ** -24
C1 = 66 * 2.0 ** -13      # an f32 dot product of length 64 (+ 2 for the order / fma freedom), in units of U16


def unpack(qkv, B, S, H):
    """[B*S, 3*H*64] -> q, k, v, each [B, H, S, 64] float64."""
    x = qkv.double().reshape(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def heads(x, B, S, H):
    """[B*S, H*64] -> [B, H, S, 64] float64."""
    return x.double().reshape(B, S, H, 64).permute(0, 2, 1, 3)


def rows(x):
    """[B, H, S, 64] -> [B*S, H*64]."""
    B, H, S, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, H * 64)


def attention(qkv, B, S, H, causal, d_out=None):
    q, k, v = unpack(qkv, B, S, H)
    vis = torch.ones(S, S, dtype=torch.bool, device=qkv.device)
    if causal:
        vis = vis.tril()
    visf = vis.double()
    s = (q @ k.transpose(-1, -2)) / 8.0
    s = s.masked_fill(~vis, float("-inf"))
    p = torch.softmax(s, dim=-1)
    out = p @ v
    res = {"S": S, "A": ((q.abs() @ k.abs().transpose(-1, -2)) / 8.0 * visf).max().item(),
           "out": rows(out), "scale_o": rows(p @ v.abs()),
           "sub_o": rows(visf @ v.abs() + visf.sum(-1)[:, None] * out.abs())}
    if d_out is None:
        return res
    do = heads(d_out, B, S, H)
    dp = do @ v.transpose(-1, -2)
    G = do.abs() @ v.abs().transpose(-1, -2)
    # dS_ij = p_ij (dP_ij - delta_i), delta_i = sum_j p_ij dP_ij = dO_i . O_i, with dP taken relative to the row's most probable key: a row whose
    # dominant probability rounds to 1 would otherwise lose its whole dS to cancellation, in float64 too
    dp = dp - dp.gather(-1, p.argmax(-1, keepdim=True))
    delta = (p * dp).sum(-1, keepdim=True)
    gbar = (p * G).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    T = p * (C1 * G + (1 + C1) * gbar)
    res.update({
        "dq": rows(ds @ k / 8.0), "scale_q": rows(ds.abs() @ k.abs() / 8.0), "scale2_q": rows(T @ k.abs() / 8.0), "sub_q": rows(visf @ k.abs() / 8.0),
        "dk": rows(ds.transpose(-1, -2) @ q / 8.0), "scale_k": rows(ds.abs().transpose(-1, -2) @ q.abs() / 8.0),
        "scale2_k": rows(T.transpose(-1, -2) @ q.abs() / 8.0), "sub_k": rows(visf.t() @ q.abs() / 8.0),
        "dv": rows(p.transpose(-1, -2) @ do), "scale_v": rows(p.transpose(-1, -2) @ do.abs()), "sub_v": rows(visf.t() @ do.abs()),
    })
    return res


def attention_row(qkv, B, S, H, causal, row_index=None, qrows=None, do_rows=None):
    """ONE query row per sequence: row row_index[b] (None: row 0) of the packed qkv or, qrows [B, D] given, row b of qrows; causal: keys 0 .. r.
    out [B, D]; with do_rows [B, D]: dq / dk / dv as the whole packed [B*S, D] pieces (dq zero outside row r, causal dk / dv zero after it)."""
    q, k, v = unpack(qkv, B, S, H)
    dev = qkv.device
    r = torch.zeros(B, dtype=torch.long, device=dev) if row_index is None else row_index.long().to(dev)
    qr = q[torch.arange(B, device=dev), :, r] if qrows is None else qrows.double().reshape(B, H, 64)          # [B, H, 64]
    j = torch.arange(S, device=dev)
    vis = (j[None, :] <= r[:, None]) if causal else torch.ones(B, S, dtype=torch.bool, device=dev)          # [B, S]
    s = torch.einsum("bhd,bhjd->bhj", qr, k) / 8.0
    s = s.masked_fill(~vis[:, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    out = torch.einsum("bhj,bhjd->bhd", p, v)
    A = (torch.einsum("bhd,bhjd->bhj", qr.abs(), k.abs()) / 8.0 * vis[:, None, :]).max().item()
    res = {"S": S, "A": A, "out": out.reshape(B, H * 64), "scale_o": torch.einsum("bhj,bhjd->bhd", p, v.abs()).reshape(B, H * 64)}
    if do_rows is None:
        return res
    do = do_rows.double().reshape(B, H, 64)
    dp = torch.einsum("bhd,bhjd->bhj", do, v)
    G = torch.einsum("bhd,bhjd->bhj", do.abs(), v.abs())
    # dS_ij = p_ij (dP_ij - delta_i), delta_i = sum_j p_ij dP_ij = dO_i . O_i, with dP taken relative to the row's most probable key: a row whose
    # dominant probability rounds to 1 would otherwise lose its whole dS to cancellation, in float64 too
    dp = dp - dp.gather(-1, p.argmax(-1, keepdim=True))
    delta = (p * dp).sum(-1, keepdim=True)
    gbar = (p * G).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    T = p * (C1 * G + (1 + C1) * gbar)

    def at_row(x):      # [B, H, 64] -> [B, H, S, 64], zero outside row r
        full = torch.zeros(B, H, S, 64, dtype=torch.float64, device=dev)
        full[torch.arange(B, device=dev), :, r] = x
        return rows(full)
    res.update({
        "dq": at_row(torch.einsum("bhj,bhjd->bhd", ds, k) / 8.0), "scale_q": at_row(torch.einsum("bhj,bhjd->bhd", ds.abs(), k.abs()) / 8.0),
        "scale2_q": at_row(torch.einsum("bhj,bhjd->bhd", T, k.abs()) / 8.0),
        "dk": rows(ds[..., None] * qr[:, :, None, :] / 8.0), "scale_k": rows(ds.abs()[..., None] * qr.abs()[:, :, None, :] / 8.0),
        "scale2_k": rows(T[..., None] * qr.abs()[:, :, None, :] / 8.0),
        "dv": rows(p[..., None] * do[:, :, None, :]), "scale_v": rows(p[..., None] * do.abs()[:, :, None, :]),
    })
    for n in ("sub_q", "sub_k", "sub_v"):      # no f16 intermediate in the one-row kernels
        res[n] = torch.zeros_like(res["dq"])
    return res


# ------------------------------------------------------------------------------------------------ shared-prefix layout
def to_shared(x, B, S, Ps, fold="first"):
    """Plain [B*S, C] -> [Ps + B (S - Ps), C].  The shared rows: sequence 0's (fold = "first") or the sum over sequences (fold = "sum")."""
    x3 = x.reshape(B, S, -1)
    head = x3[0, :Ps] if fold == "first" else x3[:, :Ps].sum(0)
    return torch.cat((head, x3[:, Ps:].reshape(B * (S - Ps), -1)))


def from_shared(xs, B, S, Ps):
    """[Ps + B (S - Ps), C] -> plain [B*S, C] with the shared rows repeated for every sequence."""
    C = xs.shape[-1]
    return torch.cat((xs[:Ps].expand(B, Ps, C), xs[Ps:].reshape(B, S - Ps, C)), dim=1).reshape(B * S, C)


def attention_shared(qkv_s, B, S, H, Ps, d_out_s=None):
    """Causal attention in the shared-prefix layout: the plain reference on the expanded rows.  The shared query rows belong to sequence 0 alone (the
    other sequences' copies carry no output gradient); dK / dV of the shared keys are summed over sequences."""
    d_out = None
    if d_out_s is not None:
        d_out = from_shared(d_out_s, B, S, Ps).reshape(B, S, -1).clone()
        d_out[1:, :Ps] = 0
        d_out = d_out.reshape(B * S, -1)
    full = attention(from_shared(qkv_s, B, S, Ps), B, S, H, 1, d_out)
    res = {"S": S, "A": full["A"], "B": B}
    for n, x in full.items():
        if torch.is_tensor(x):
            res[n] = to_shared(x, B, S, Ps, "sum" if n.endswith(("k", "v")) else "first")
    return res


# ------------------------------------------------------------------------------------------------ bounds ("Attention kernel tests")
def k_of(kind, A, S, B=1):
    """The factor k of |err| <= k 2^-11 scale + 2^-11 |ref| (+ the terms of bound()), from the rounding steps of each kernel.  In units of 2^-11:
    cs = a probability's relative error from the f32 score (66 2^-24 A, twice: numerator and row sum), acc = an f32 sum of S terms, 0.1 = exp2 / rcp /
    the 1/8 and log2(e) products.  mfma: P (or dS) rounded to f16 once more; bwd_shared: the class sum of B f32 shares."""
    cs, acc = 66 * A * 2.0 ** -13, S * 2.0 ** -13
    return {"fwd_mfma": 2 * (1 + cs) + 2 * acc + 0.1,          # f16 P in the numerator AND in the row sum it is divided by
            "fwd_row": 2 * cs + 2 * acc + 0.1,                 # f32 probabilities
            "bwd_mfma": 2 * cs + 1 + 2 * acc + 0.1,            # p (2 cs + acc), P / dS to f16 (1), the MFMA accumulation (acc)
            "bwd_row": 2 * cs + 2 * acc + 0.1,
            "bwd_shared": 2 * cs + 1 + 2 * acc + 0.1 + B * 2.0 ** -13}[kind]


def bound(res, what, kind):
    """Element-wise bound of output `what` in {"o", "q", "k", "v"} of a kernel of class `kind` (k_of)."""
    k = k_of(kind, res["A"], res["S"], res.get("B", 1))
    ref = res["out" if what == "o" else "d" + what]
    b = k * U16 * res["scale_" + what] + U16 * ref.abs() + SUB16
    if what in "qk":
        b = b + U16 * res["scale2_" + what]
    if "mfma" in kind or "shared" in kind:
        b = b + SUB16 * res["sub_" + what]
    return b


def bound_exact(res):
    """The f32 one-row kernel on f32 inputs: the same count with 2^-24 for 2^-11 and no f16 anywhere."""
    return (2 * 66 * res["A"] + 2 * res["S"] + 8) * U32 * res["scale_o"] + U32 * res["out"].abs()


# ------------------------------------------------------------------------------------------------ input families
FAMILIES = ("randn", "peaked", "leak")


def make_inputs(family, B, S, H, causal, seed, device="cpu"):
    """(qkv [B*S, 3D] f16, d_out [B*S, D] f16).  randn: unit normal.  peaked: scores span tens of units; row i's dominant key is its last visible one
    (S - 1, causal: i) for even i, else the 32-key chunk boundary at or below it (i % 4 == 1) or the key before that boundary (i % 4 == 3); |v| and |dO|
    stay in [0.5, 4] so that no sum of absolute terms vanishes.  leak: unit normal with K and V of every odd sequence scaled by 64."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, S, 64, generator=g)
    k = torch.randn(B, H, S, 64, generator=g)
    v = torch.randn(B, H, S, 64, generator=g)
    do = torch.randn(B, H, S, 64, generator=g)
    if family == "peaked":
        i = torch.arange(S)
        last = i if causal else torch.full((S,), S - 1)
        cb = (last // 32) * 32
        t = torch.where(i % 2 == 0, last, torch.where(i % 4 == 1, cb, (cb - 1).clamp_min(0)))
        q = 3.0 * q + 3.0 * k[:, :, t]          # score of the target ~ 3 |k|^2 / 8 = 24, the others ~ N(0, 4.2^2)
        v = torch.sign(v) * (0.5 + v.abs()).clamp_max(4.0)
        do = torch.sign(do) * (0.5 + do.abs()).clamp_max(4.0)
    elif family == "leak":
        k[1::2] *= 64.0
        v[1::2] *= 64.0
    else:
        assert family == "randn"
    qkv = torch.cat((rows(q), rows(k), rows(v)), dim=1).half().to(device)
    return qkv, rows(do).half().to(device)
