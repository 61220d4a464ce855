"""float64 references of the forward row kernels (csrc/rowops.hip) with a derived bound on |f32 kernel - value| per element ("Row forward
and head kernel tests").  Plain torch float64 on whatever device the inputs live on; nothing here calls the library.

The conventions are those of tests/rowops_ref.py: every function returns (value, bound) pairs, float64; the bound is first-order forward error
propagation through the kernel's own sequence of operations with u = 2^-24 (an add, multiply or divide u |result|; a row reduction (4 NV + 6) u sum|terms|;
p terms added in index order (p - 1) u sum|terms|; rsqrtf 2 u), the inputs exact as the kernel reads them.  Nothing in a bound is measured.  Where a
statistic is formed by the one-pass formula sum v^2 / d - mean^2 the cancellation is carried (it is large on `flat` rows) and rsqrt is bounded over the whole
interval [v - E(v), v + E(v)] instead of to first order, because E(v) / v is not small there.

`fault` names ONE deliberate error applied to the float64 value (never to the bound): tests/test_host_rowops_fwd_ref.py shows with them that the bound
is not vacuous."""
import numpy as np
import torch

from rowops_ref import DIV_REL, FAMILIES, HALF_U, LN_EPS, RSQRT_REL, U, WIDTHS, _red, half_bound, make_inputs, nv_of  # noqa: F401

SPLIT_LO_SCALE = 1.0      # csrc/common.h GRIP_SPLIT_LO_SCALE
FAULTS = ("no_eps", "d_plus_4", "gamma_tail_one", "drop_beta", "pos_on_prompt", "pos_j_for_1_plus_j", "prompt_of_image_0", "class_0_context",
          "token_off_by_one", "read_row_off_by_one", "deep_stats_of_unrounded", "embed_stats_of_stored", "x_lo_of_unrounded_hi", "drop_tile",
          "colsum_unrounded")


def _sm(t):
    return t.sum(-1, keepdim=True)


# ------------------------------------------------------------------------------------------------ LayerNorm (ln_normalize + ln_apply, contraction off)
def ln_stats(x, e_x=None, fault=None):
    """ln_normalize on rows x (float64) known to within e_x: (mean, E(mean), c, E(c), rstd, E(rstd)), the first six lines of the backward bound."""
    d = x.shape[-1]
    R = _red(d)
    e_x = torch.zeros_like(x) if e_x is None else e_x
    dd = d + 4 if fault == "d_plus_4" else d
    eps = 0.0 if fault == "no_eps" else LN_EPS
    mean = _sm(x) / dd
    e_mean = (_sm(e_x) + R * _sm(x.abs())) / d + DIV_REL * mean.abs()
    c = x - mean
    e_c = e_x + e_mean + U * c.abs()
    q = _sm(c * c)
    e_q = _sm(2 * c.abs() * e_c + U * c * c) + R * q
    var = q / dd
    e_var = e_q / d + DIV_REL * var
    v = var + eps
    e_v = e_var + U * v
    rstd = v.rsqrt()
    e_rstd = 0.5 * rstd / v * e_v + RSQRT_REL * rstd
    return mean, e_mean, c, e_c, rstd, e_rstd


def ln_fwd(x, gamma, beta, e_x=None, fault=None):
    """y = ((c rstd) gamma) + beta with three roundings.  x [M, d] float64 (the values the kernel holds in f32, within e_x) -> (y, E(y))."""
    gamma, beta = gamma.double(), beta.double()
    if fault == "gamma_tail_one":
        gamma = gamma.clone()
        gamma[-4:] = 1.0
    if fault == "drop_beta":
        beta = torch.zeros_like(beta)
    mean, e_mean, c, e_c, rstd, e_rstd = ln_stats(x, e_x, fault)
    t1 = c * rstd
    e1 = rstd * e_c + c.abs() * e_rstd + U * t1.abs()
    t2 = t1 * gamma
    e2 = gamma.abs() * e1 + U * t2.abs()
    y = t2 + beta
    return y, e2 + U * y.abs()


def split_bound(ref, bound):
    """What split_f16x4 adds to an f32 value within `bound` of `ref`, decoded as hi + lo' / SPLIT_LO_SCALE: x - hi is exact in f32 and at most half an f16
    ulp of x, |x - hi| <= 2^-11 |x| + 2^-25; its own rounding to f16 (subnormals kept) is what the pair drops."""
    r = HALF_U * (ref.abs() + bound) + 2.0 ** -25
    return HALF_U * r + 2.0 ** -25 / SPLIT_LO_SCALE


def unsplit(buf, rows, d):
    """Split layout [rows, d / 32, (32 hi | 32 lo')] f16 -> hi + lo' / SPLIT_LO_SCALE (as tests/test_gpu_split.py decodes it)."""
    v = buf.view(torch.float16).reshape(rows, d // 32, 2, 32).double()
    return (v[:, :, 0] + v[:, :, 1] / SPLIT_LO_SCALE).reshape(rows, d)


def read_rows(n, stride, index, device, fault=None):
    pos = torch.zeros(n, dtype=torch.long, device=device) if index is None else index.to(device).long()
    at = torch.arange(n, device=device) * stride + pos
    return at + 1 if fault == "read_row_off_by_one" else at


def ln_gather(x, index, stride, n, gamma, beta, fault=None):
    """LayerNorm of rows r stride + index[r] (index None: position 0) of x, r < n."""
    at = read_rows(n, stride, index, x.device, fault) % x.shape[0]
    return ln_fwd(x[at].double(), gamma, beta, None, fault)


# ------------------------------------------------------------------------------------------------ vit_assemble_ln
def vit_assemble(patch, cls, pos, prefix, gamma, beta, B, P, G2, per_image, fault=None):
    """Rows (b, 0) = cls + pos[0], (b, 1 .. P) = prefix[(b,) s - 1] (no positional term), (b, 1 + P + j) = patch[b G2 + j] + pos[1 + j]; then LayerNorm; then
    ln_normalize once more on the f32 LayerNorm output (rowstat).  -> (y, E(y), (mean, E(mean), rstd, E(rstd)) of y), rows in stream order.  The add is
    one rounding (none for a prompt row or with pos None)."""
    d = patch.shape[-1]
    S = 1 + P + G2
    patch, cls = patch.double().reshape(B, G2, d), cls.double().reshape(1, 1, d)
    v = torch.zeros(B, S, d, dtype=torch.float64, device=patch.device)
    added = torch.zeros(B, S, 1, dtype=torch.bool, device=patch.device)
    v[:, :1] = cls
    v[:, 1 + P:] = patch
    if P:
        pre = prefix.double().reshape(B if per_image else 1, P, d)
        if fault == "prompt_of_image_0":
            pre = pre[:1]
        v[:, 1:1 + P] = pre
    if pos is not None:
        pos = pos.double()
        v[:, 0] += pos[0]
        v[:, 1 + P:] += pos[:G2] if fault == "pos_j_for_1_plus_j" else pos[1:1 + G2]
        added[:, 0] = True
        added[:, 1 + P:] = True
        if fault == "pos_on_prompt" and P:
            v[:, 1:1 + P] += pos[1:1 + P]
    v = v.reshape(B * S, d)
    e_v = U * v.abs() * added.reshape(B * S, 1)
    y, e_y = ln_fwd(v, gamma, beta, e_v, fault)
    mean, e_mean, _, _, rstd, e_rstd = ln_stats(y, e_y)
    return y, e_y, (mean, e_mean, rstd, e_rstd)


def x_lo(y, e_y, hi_stored, fault=None):
    """x_lo = f16(v - f16(v)) with v the f32 LayerNorm output, GIVEN the hi the kernel stored: the subtraction is exact, so the value is y - hi within
    E(y), and one rounding to f16."""
    ref = y - (y if fault == "x_lo_of_unrounded_hi" else hi_stored.double())
    true = y - hi_stored.double()
    return ref, e_y + half_bound(true, e_y)


# ------------------------------------------------------------------------------------------------ one-pass statistics
def _onepass_tail(S1, e1, S2, e2, d, inv_mul):
    """mean = S1 / d, var = max(S2 / d - mean^2, 0), rstd = rsqrt(var + eps).  inv_mul: the kernel multiplies by fl(1 / d) (two roundings) instead of
    dividing (one).  The cancellation in S2 / d - mean^2 is carried: E(var) is relative to S2 / d, not to var.  rsqrt over the whole interval: the
    computed argument is at least eps (1 - u) (the clamp), and within E(v) of v."""
    k = 2 * U if inv_mul else DIV_REL
    mean = S1 / d
    e_mean = e1 / d + k * mean.abs()
    m2 = S2 / d
    e_m2 = e2 / d + k * m2
    mm = mean * mean
    e_mm = 2 * mean.abs() * e_mean + e_mean * e_mean + U * mm
    var = (m2 - mm).clamp_min(0.0)
    e_var = e_m2 + e_mm + U * (m2 - mm).abs()            # (the clamp is a contraction towards the true, non-negative value)
    v = var + LN_EPS
    e_v = e_var + U * v
    rstd = v.rsqrt()
    lo = torch.maximum(v - e_v, torch.full_like(v, LN_EPS * (1 - 2 * U)))
    e_rstd = (lo.rsqrt() - rstd).clamp_min(0.0) + RSQRT_REL * lo.rsqrt()
    return mean, e_mean, rstd, e_rstd


def seq_rows(C, T, Ps, device):
    """(class, position) of every stream row: plain layout (Ps = 0) c T + t; shared-prefix layout rows 0 .. Ps - 1 once (class 0), then T - Ps per class."""
    cs = [0] * Ps + [c for c in range(C) for _ in range(Ps, T)]
    ts = list(range(Ps)) + [t for _ in range(C) for t in range(Ps, T)]
    return torch.tensor(cs, device=device), torch.tensor(ts, device=device)


def text_embed(ids, tok, pos, prefix, P, prefix_classes, C, T, Ps, fault=None):
    """x[c, t] = (1 <= t <= P ? prefix[c or 0, t - 1] : tok[clamp(ids[c, t])]) (+ pos[t]).  ids [C, ld_ids].  -> (v, E(v), (mean, E, rstd, E)): the statistics are
    one-pass (sum v, sum v^2 with (4 NV + 6)-deep reductions, contraction allowed: fewer roundings) of the UNROUNDED f32 row, whatever the stream stores."""
    d, vocab = tok.shape[-1], tok.shape[0]
    cs, ts = seq_rows(C, T, Ps, tok.device)
    idv = ids.long()[cs, ts] + (1 if fault == "token_off_by_one" else 0)
    v = tok.double()[idv.clamp(0, vocab - 1)]
    if P:
        pre = prefix.double().reshape(prefix_classes, P, d)
        pc = torch.zeros_like(cs) if (prefix_classes == 1 or fault == "class_0_context") else cs
        isp = (ts >= 1) & (ts <= P)
        v = torch.where(isp[:, None], pre[pc, (ts - 1).clamp(0, P - 1)], v)
    e_v = torch.zeros_like(v)
    if pos is not None:
        v = v + pos.double()[ts]
        e_v = U * v.abs()
    s = v.half().double() if fault == "embed_stats_of_stored" else v
    R = _red(d)
    S1, S2 = _sm(s), _sm(s * s)
    e1 = _sm(e_v) + R * _sm(v.abs())
    e2 = _sm(2 * v.abs() * e_v + U * v * v) + R * _sm(v * v)
    return v, e_v, _onepass_tail(S1, e1, S2, e2, d, inv_mul=False)


def deep_insert(deep, compensated, fault=None):
    """Rows deep [n, d] f32 as vit_deep_insert_kernel stores them in an f16 stream: hi = f16(deep) (exact), x_lo = f16(deep - hi) (exact: the subtraction
    is), and the statistics of the values AS STORED, v = hi or fl32(hi + f16(lo)): per 64-column tile ts = (v0 + v1) + (v2 + v3) then four DPP levels
    (6 adds deep), tq a four-term fma chain then four levels (8 roundings deep), the tiles then added in tile order (tiles - 1 more), contraction off;
    mean = sm * fl(1 / d).  -> (hi f16, lo f16, (ts, E, tq, E) [n, d / 64], (mean, E, rstd, E))."""
    d = deep.shape[-1]
    tiles = d // 64
    hi = deep.float().half()
    lo = (deep.float() - hi.float()).half()
    v = hi.double() + lo.double() if compensated else hi.double()
    e_v = U * v.abs() if compensated else torch.zeros_like(v)
    if fault == "deep_stats_of_unrounded":
        v = deep.double()
    vt = v.reshape(-1, tiles, 64)
    et = e_v.reshape(-1, tiles, 64)
    ts, tq = vt.sum(-1), (vt * vt).sum(-1)
    a1, a2 = vt.abs().sum(-1), tq
    e_ts = et.sum(-1) + 6 * U * a1
    e_tq = (2 * vt.abs() * et).sum(-1) + 8 * U * a2
    keep = slice(0, tiles - 1) if fault == "drop_tile" else slice(0, tiles)
    S1, S2 = _sm(ts[:, keep]), _sm(tq[:, keep])
    e1 = _sm(e_ts) + (tiles - 1) * U * _sm(a1)
    e2 = _sm(e_tq) + (tiles - 1) * U * _sm(a2)
    return hi, lo, (ts, e_ts, tq, e_tq), _onepass_tail(S1, e1, S2, e2, d, inv_mul=True)


def stats_finalize(part, d, fault=None):
    """ln_stats_finalize on part [parts, M, 2] f32 (exact inputs): `parts` sequential adds, then the same tail."""
    part = part.double()
    p = part.shape[0]
    used = part[:-1] if fault == "drop_tile" else part
    S1, S2 = used[..., 0].sum(0)[:, None], used[..., 1].sum(0)[:, None]
    e1 = (p - 1) * U * part[..., 0].abs().sum(0)[:, None]
    e2 = (p - 1) * U * part[..., 1].abs().sum(0)[:, None]
    return _onepass_tail(S1, e1, S2, e2, d, inv_mul=True)


def fold_weights(W, gamma, beta, bias, fault=None):
    """Wg = f16(fl32(gamma W)) exactly (one f32 multiply, one rounding: torch reproduces it); colsum = sum of the ROUNDED Wg, K / 64 in-lane adds and wave_sum;
    bias_out = bias + sum beta W.  W [N, K] f16.  -> (Wg f16, (colsum, E), (bias_out, E))."""
    K = W.shape[-1]
    depth = ((K + 63) // 64 + 6) * U
    prod = gamma.float() * W.float()
    Wg = prod.half()
    cs_terms = prod.double() if fault == "colsum_unrounded" else Wg.double()
    colsum = cs_terms.sum(-1)
    e_cs = depth * Wg.double().abs().sum(-1)
    t = beta.double() * W.double()
    sb = t.sum(-1)
    e_sb = (depth + U) * t.abs().sum(-1)
    out = bias.double() + sb
    return Wg, (colsum, e_cs), (out, e_sb + U * out.abs())


# ------------------------------------------------------------------------------------------------ exact kernels
def im2col(img, p, Kpad, out_dtype):
    """out[(b G + py) G + px][c p p + kh p + kw] = img[b][c][py p + kh][px p + kw], zero-padded to Kpad: the header's formula as an index expression."""
    B, _, R, _ = img.shape
    G, K = R // p, 3 * p * p
    k = torch.arange(K, device=img.device)
    c, kh, kw = k // (p * p), (k % (p * p)) // p, k % p
    row = torch.arange(B * G * G, device=img.device)
    b, py, px = row // (G * G), (row // G) % G, row % G
    vals = img[b[:, None], c[None], (py[:, None] * p + kh[None]), (px[:, None] * p + kw[None])]
    out = torch.zeros(B * G * G, Kpad, dtype=out_dtype, device=img.device)
    out[:, :K] = vals.float().to(out_dtype)
    return out


def make_rows(family, M, d, seed, device="cpu"):
    """(rows f32 [M, d] that are NOT f16 numbers, gamma, beta): the family's f16 rows times (1 + 1e-4 randn)."""
    x, _, gamma = make_inputs(family, M, d, 1, seed)
    g = torch.Generator().manual_seed(seed + 1)
    rows = (x.float() * (1 + 1e-4 * torch.randn(M, d, generator=g))).contiguous()
    beta = 0.2 * torch.randn(d, generator=g)
    return rows.to(device), gamma.to(device), beta.to(device)
