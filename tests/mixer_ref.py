"""float64 references of the UPT prompt-mixer launches (csrc/mixer.hip), one function per operation of a launch, each with a derived bound on
|f32 kernel - value| per element ("Mixer kernel tests").  Plain torch on whatever device and dtype the inputs have; nothing here calls
the library.

The conventions are those of tests/rowops_ref.py and tests/rowops_fwd_ref.py.  Every function takes the image of the f32 buffers the launch READS
(in float64 for a reference; in float32 the same statements are the CPU restatement tests/test_host_mixer_ref.py uses) and returns a dict
{buffer: (value, bound)} of what it writes.  A bound is first-order forward error propagation through the kernel's own sequence of operations with
u = 2^-24: the inputs are exact, an f32 add, multiply or divide contributes u |result|, a sum of K terms over lanes striding K and wave_sum
(ceil(K / 64) + 6) u sum|terms|, rsqrtf 2 u, a rounding to fp16 2^-11 |v| + 2^-25, and an error propagates through every later operation with the
absolute value of its partial derivative.  A Linear is bounded by (K + 2) u sum|x w| (the bias one more term), which holds for any order of the sum
with or without FMA.  TINY = 2^-126 is added wherever a result may be flushed.  Nothing in a bound is measured.

`__expf`, the fast intrinsic, is the one operation IEEE rules do not cover.  The compiler's own header (clang's __clang_hip_math.h) defines it as the
hardware exp2 of the f32 product t * log2(e): that product is |t| u relative to exp(t) and derivable.  No accuracy statement for the hardware exp2 or
for the intrinsic is installed with the toolchain's documentation or headers, so the allowance is BORROWED from the one this project already uses
for an f32 exponential, (2 |t| + 4) u relative (tests/test_gpu_cache_head.py): it is not a documented figure for the intrinsic.

A buffer named `<name>#f16` is not a buffer: it is the residual v - fp16(v) of buffer <name>, whose value and bound are zero where the kernel rounds
to fp16 (the result must be an fp16 number exactly).

`fault` names ONE deliberate error applied to the value (never to the bound); tests/test_host_mixer_ref.py shows with them that no bound is vacuous."""
import math

import numpy as np
import torch

from rowops_ref import DIV_REL, HALF_U, LN_EPS, RSQRT_REL, U

TINY = 2.0 ** -126
GELU_C = float(np.float32(1.702))          # the kernel's `1.702f`
EXPF_T, EXPF_C = 2.0, 4.0                  # exp(t) to (EXPF_T |t| + EXPF_C) u relative: borrowed from tests/test_gpu_cache_head.py (module docstring)
MIXER_TENSORS = ("coop", "vpt", "coop_pre_w", "coop_pre_b", "vpt_pre_w", "vpt_pre_b", "ln1_g", "ln1_b", "in_w", "in_b", "out_w", "out_b",
                 "ln2_g", "ln2_b", "fc_w", "fc_b", "proj_w", "proj_b", "coop_post_w", "coop_post_b", "vpt_post_w", "vpt_post_b")
FAMILIES = ("randn", "large")
# (P, text_width, vision_width, dim, n_deep): the smallest shapes that reach each edge of the kernels (tests/test_gpu_mixer_kernels.py)
SHALLOW_CASES = ((1, 64, 64, 64, 0), (3, 65, 130, 192, 0), (5, 100, 1280, 128, 0), (16, 1280, 1279, 256, 0), (4, 512, 768, 128, 0))
DEEP_CASES = ((1, 64, 64, 64, 1), (3, 65, 130, 192, 2), (7, 200, 136, 64, 5), (4, 512, 768, 128, 11), (16, 320, 1280, 256, 31))
CASES = SHALLOW_CASES + DEEP_CASES
FORWARD_SLOTS = ("x0", "st1", "y1", "qkv", "o", "x1", "st2", "z", "h", "g", "x2", "out16", "pm", "xv")
BACKWARD_SLOTS = ("d_x2", "dh", "dz", "d_x1", "d_o", "dqkv", "dy", "d_x0", "T_cq", "T_vq", "T_pr", "T_fc", "T_o", "T_in", "T_cp", "T_vp", "dsm", "dv_all")
DEEP_SLOTS = ("pm", "dsm", "xv", "dv_all")


def _applies_always(case):
    return True


# fault -> (the step it is an error of, the family it is shown on, the cases that have the edge it needs: elsewhere the fault is the identity)
FAULT_SITES = {
    "tile_last_row": ("in_proj", "randn", _applies_always),                                     # the last row of an 8-row tile reads the row before it
    "k_tail": ("pre", "randn", lambda c: c[1] % 64 != 0 or c[2] % 64 != 0),                     # the K % 64 tail not summed
    "n_tail": ("post", "randn", lambda c: c[1] % 4 != 0 or c[2] % 4 != 0),                      # the last N % 4 columns dropped
    "no_scale": ("attn", "randn", _applies_always),                                             # softmax without 1 / sqrt(dim)
    "rows_ps_l": ("attn", "randn", lambda c: c[0] > 1),                                         # rows indexed p S + l instead of l P + p
    "pm_transposed": ("attn", "randn", lambda c: c[4] > 0),                                     # pm stored [P, m, l]
    "gelu_1p7": ("gelu", "large", _applies_always),                                             # 1.7 for 1.702
    "gelugrad_1p7": ("dh", "large", _applies_always),
    "skip_round_d_x2": ("d_x2", "randn", _applies_always),                                      # the fp16 rounding of d_x2 skipped
    "lnbwd_no_c2": ("d_x1", "randn", _applies_always),                                          # c2 dropped from the LayerNorm backward
    "deep_stats_first_token": ("d_x0", "large", lambda c: c[4] > 0),                            # the deep rows use the first token's (mean, rstd)
    "bias_skip_row0": ("param_grads", "randn", _applies_always),                                # a bias gradient skips row 0
    "dgamma_unnormalised": ("param_grads", "randn", _applies_always),                           # d gamma from x instead of x^
    "transpose_tail": ("transpose", "randn", lambda c: c[1] % 32 != 0 or c[2] % 32 != 0),       # a transpose tail (N % 32) left unwritten
}
FAULTS = tuple(FAULT_SITES)


def _sm(t):
    return t.sum(-1, keepdim=True)


def _red(K):
    """Lanes striding K (ceil(K / 64) adds in a lane) and the six levels of wave_sum."""
    return ((K + 63) // 64 + 6) * U


def r16(t):
    return t.half().to(t.dtype)


def f16_pair(name, value, bound, skip=False):
    """A result the kernel rounds to fp16: it lies within the bound of the UNROUNDED result plus one fp16 rounding of what the kernel held
    (2^-11 (|v| + bound) + 2^-25), and its residual v - fp16(v) is zero exactly (`run` chains the rounded value).  skip: the fault, the rounding left
    out -- only the residual can tell."""
    v = value if skip else r16(value)
    return {name: (value, bound + HALF_U * (value.abs() + bound) + 2.0 ** -25), name + "#f16": (v - r16(v), torch.zeros_like(v))}


# ------------------------------------------------------------------------------------------------ the Linear and its epilogues
def linear(X, W, b=None, fault=None):
    """Y = X W^T + b, X [R, K], W [N, K]: |err| <= (K + 2) u (|X| |W|^T + |b|)."""
    R, K = X.shape
    N = W.shape[0]
    Xv = X
    if fault == "tile_last_row":
        last = [min(t + 7, R - 1) for t in range(0, R, 8)]
        last = [r for r in last if r > 0]
        Xv = X.clone()
        Xv[last] = X[[r - 1 for r in last]]
    if fault == "k_tail" and K % 64:
        Xv = X.clone()
        Xv[:, K - K % 64:] = 0
    Y = Xv @ W.T
    T = X.abs() @ W.abs().T
    if b is not None:
        Y, T = Y + b, T + b.abs()
    if fault == "n_tail" and N % 4:
        Y = Y.clone()
        Y[:, N - N % 4:] = 0
    return Y, (K + 2) * U * T


def resid(e0, X, W, b):
    """MEPI_RESID: e0 + (X W^T + b), one more rounded add."""
    y, e = linear(X, W, b)
    v = e0 + y
    return v, e + U * v.abs()


def _sigmoid_terms(h, c):
    """s = 1 / (1 + __expf(-c h)) as quick_gelu / quick_gelu_grad form it: (e, d = 1 + e, E(d)).  t = fl(c) h is one rounding, u |t| of the exponent."""
    t = -c * h
    e = torch.exp(t)
    rel_e = U * t.abs() + (EXPF_T * t.abs() + EXPF_C) * U
    d = 1 + e
    return e, d, e * rel_e + TINY + U * d


def gelu(h, fault=None, c=GELU_C):
    """MEPI_GELU on the h the kernel stored: g = h / (1 + __expf(-1.702f h))."""
    e, d, e_d = _sigmoid_terms(h, c)
    g = h / d
    bound = h.abs() * e_d / (d * d) + DIV_REL * g.abs() + TINY
    if fault == "gelu_1p7":
        g = h / (1 + torch.exp(-1.7 * h))
    return g, bound


def gelugrad(X, W, h, fault=None, c=GELU_C):
    """MEPI_GELUGRAD: (X W^T) d(h), d = s (1 + (1.702f h)(1 - s)), s = 1 / (1 + __expf(-1.702f h))."""
    y, e_y = linear(X, W)
    _, d, e_d = _sigmoid_terms(h, c)
    s = 1 / d
    e_s = e_d / (d * d) + DIV_REL * s
    a = 1 - s
    e_a = e_s + U * a.abs()
    b = c * h
    m = b * a
    e_m = b.abs() * e_a + a.abs() * U * b.abs() + U * m.abs()
    n = 1 + m
    e_n = e_m + U * n.abs()
    q = s * n
    e_q = n.abs() * e_s + s * e_n + U * q.abs()
    if fault == "gelugrad_1p7":
        s7 = 1 / (1 + torch.exp(-1.7 * h))
        q = s7 * (1 + 1.7 * h * (1 - s7))
    v = y * q
    return v, q.abs() * e_y + y.abs() * e_q + e_y * e_q + U * v.abs() + TINY


# ------------------------------------------------------------------------------------------------ LayerNorm, forward and backward
def ln_pro(x, gamma, beta, eps=LN_EPS):
    """PRO_LN (ln_row): two-pass statistics, y = ((x - mean) rstd) gamma + beta.  -> (y, E), (stats [R, 2] = (mean, rstd), E)."""
    d = x.shape[-1]
    R = _red(d)
    mean = _sm(x) / d
    e_mean = R * _sm(x.abs()) / d + DIV_REL * mean.abs()
    c = x - mean
    e_c = e_mean + U * c.abs()
    q = _sm(c * c)
    e_q = _sm(2 * c.abs() * e_c + U * c * c) + R * q
    var = q / d
    e_var = e_q / d + DIV_REL * var
    v = var + eps
    e_v = e_var + U * v
    rstd = v.rsqrt()
    e_rstd = 0.5 * rstd / v * e_v + RSQRT_REL * rstd
    t1 = c * rstd
    e1 = rstd * e_c + c.abs() * e_rstd + U * t1.abs()
    t2 = t1 * gamma
    e2 = gamma.abs() * e1 + U * t2.abs()
    y = t2 + beta
    return (y, e2 + U * y.abs()), (torch.cat((mean, rstd), -1), torch.cat((e_mean, e_rstd), -1))


def ln_bwd_add(dz, x, gamma, stats, p3, rows_of_stats=None, fault=None):
    """PRO_LNBWD_ADD (lnbwd_row): dx = p3 + rstd (g - c1 - x^ c2), g = dz gamma, x^ = (x - mean) rstd from the SAVED (mean, rstd) (exact inputs),
    c1 = sum g / K, c2 = sum g x^ / K."""
    K = x.shape[-1]
    R = _red(K)
    if rows_of_stats is not None:
        stats = stats[rows_of_stats]
    mean, rstd = stats[:, :1], stats[:, 1:]
    g = dz * gamma
    e_g = U * g.abs()
    c = x - mean
    xh = c * rstd
    e_xh = rstd.abs() * U * c.abs() + U * xh.abs()
    c1 = _sm(g) / K
    e_c1 = (_sm(e_g) + R * _sm(g.abs())) / K + DIV_REL * c1.abs()
    t = g * xh
    e_t = xh.abs() * e_g + g.abs() * e_xh + U * t.abs()
    c2 = _sm(t) / K
    e_c2 = (_sm(e_t) + R * _sm(t.abs())) / K + DIV_REL * c2.abs()
    m = xh * c2
    e_m = c2.abs() * e_xh + xh.abs() * e_c2 + U * m.abs()
    if fault == "lnbwd_no_c2":
        m = torch.zeros_like(m)
    r1 = g - c1
    e_r1 = e_g + e_c1 + U * r1.abs()
    r2 = r1 - m
    e_r2 = e_r1 + e_m + U * r2.abs()
    w = rstd * r2
    e_w = rstd.abs() * e_r2 + U * w.abs()
    dx = p3 + w
    return dx, e_w + U * dx.abs()


# ------------------------------------------------------------------------------------------------ attention over the S tokens of column p
def _tokens(t, S, P, fault=None):
    """Rows (token l, column p) -> l P + p of a [S P, n] buffer as [S, P, n] (the fault: rows p S + l)."""
    n = t.shape[-1]
    return t.reshape(P, S, n).transpose(0, 1) if fault == "rows_ps_l" else t.reshape(S, P, n)


def _rows(t, S, P, fault=None):
    """[S, P, n] back to rows."""
    n = t.shape[-1]
    return (t.transpose(0, 1) if fault == "rows_ps_l" else t).reshape(S * P, n)


def _softmax(q, k, Dh, fault=None):
    """p[n, l, m] = softmax_m(q[l, n] . k[m, n] rsqrtf(Dh)) with the kernels' max, __expf and division.  -> (p, E(p))."""
    scale = 1.0 if fault == "no_scale" else Dh ** -0.5
    dot = torch.einsum("lnd,mnd->nlm", q, k)
    T = torch.einsum("lnd,mnd->nlm", q.abs(), k.abs())
    s = dot * scale
    e_s = (_red(Dh) + U) * T * Dh ** -0.5 + (RSQRT_REL + U) * s.abs()
    mx = s.max(-1, keepdim=True).values
    z = s - mx
    e_z = e_s + e_s.max(-1, keepdim=True).values + U * z.abs()                 # the maximum of the computed scores is within max E(s) of the true one
    e = torch.exp(z)
    e_e = e * (torch.expm1(e_z) + (EXPF_T * z.abs() + EXPF_C) * U) + TINY
    den = _sm(e)
    e_den = _sm(e_e) + 6 * U * den                                               # wave_sum (one add for two tokens)
    p = e / den
    return p, e_e / den + e * e_den / (den * den) + DIV_REL * p + TINY


def attention(qkv, S, P, Dh, fault=None):
    """mixer_attn_kernel and PRO_ATTN (S = 2): o[l] = sum_m p[l, m] v[m] in token order, pm [P, S, S] = p.  qkv [S P, 3 Dh]."""
    t = _tokens(qkv, S, P, fault)
    q, k, v = t[..., :Dh], t[..., Dh:2 * Dh], t[..., 2 * Dh:]
    p, e_p = _softmax(q, k, Dh, fault)
    o = torch.einsum("nlm,mnd->lnd", p, v)
    e_o = torch.einsum("nlm,mnd->lnd", e_p, v.abs()) + (S + 1) * U * torch.einsum("nlm,mnd->lnd", p, v.abs())
    pm = p.transpose(1, 2) if fault == "pm_transposed" else p
    return {"o": (_rows(o, S, P, fault), _rows(e_o, S, P, fault) + TINY), "pm": (pm.reshape(-1), e_p.reshape(-1))}


def _ds(p, e_p, g, v, Dh):
    """dS[n, l, m] = p (dP - sum_m' p dP) rsqrtf(Dh), dP[l, m] = d o[l] . v[m].  e_p: what p carries (zero for the saved pm)."""
    dP = torch.einsum("lnd,mnd->nlm", g, v)
    e_dP = (_red(Dh) + U) * torch.einsum("lnd,mnd->nlm", g.abs(), v.abs())
    pd = p * dP
    t = _sm(pd)
    e_t = _sm(e_p * dP.abs() + p * e_dP + U * pd.abs()) + 6 * U * _sm(pd.abs())
    diff = dP - t
    e_diff = e_dP + e_t + U * diff.abs()
    scale = Dh ** -0.5
    ds = p * diff * scale
    return ds, (e_p * diff.abs() + p * e_diff) * scale + (2 * U + RSQRT_REL) * ds.abs() + TINY


def _dqkv(p, e_p, ds, e_ds, q, k, g, S):
    """dq[j] = sum_m dS[j, m] k[m], dk[j] = sum_l dS[l, j] q[l], dv[j] = sum_l p[l, j] d o[l], each S terms in token order."""
    out, err = [], []
    for a, e_a, pat, x in ((ds, e_ds, "njm,mnd->jnd", k), (ds, e_ds, "nlj,lnd->jnd", q), (p, e_p, "nlj,lnd->jnd", g)):
        out.append(torch.einsum(pat, a, x))
        err.append(torch.einsum(pat, e_a, x.abs()) + (S + 1) * U * torch.einsum(pat, a.abs(), x.abs()) + TINY)
    return torch.cat(out, -1), torch.cat(err, -1)


def attention_bwd_two(qkv, d_o, P, Dh):
    """PRO_ATTNBWD: dqkv of the two-token case, the softmax recomputed from qkv."""
    t, g = _tokens(qkv, 2, P), _tokens(d_o, 2, P)
    q, k, v = t[..., :Dh], t[..., Dh:2 * Dh], t[..., 2 * Dh:]
    p, e_p = _softmax(q, k, Dh)
    ds, e_ds = _ds(p, e_p, g, v, Dh)
    val, err = _dqkv(p, e_p, ds, e_ds, q, k, g, 2)
    return _rows(val, 2, P), _rows(err, 2, P)


def attention_ds(qkv, d_o, pm, S, P, Dh):
    """mixer_attn_ds_kernel: dsm [P, S, S] from the saved pm."""
    t, g = _tokens(qkv, S, P), _tokens(d_o, S, P)
    p = pm.reshape(P, S, S)
    ds, e_ds = _ds(p, torch.zeros_like(p), g, t[..., 2 * Dh:], Dh)
    return ds.reshape(-1), e_ds.reshape(-1)


def attention_bwd(qkv, d_o, pm, dsm, S, P, Dh):
    """mixer_attn_bwd_kernel: dqkv from the saved pm and dsm."""
    t, g = _tokens(qkv, S, P), _tokens(d_o, S, P)
    p, ds = pm.reshape(P, S, S), dsm.reshape(P, S, S)
    z = torch.zeros_like(p)
    val, err = _dqkv(p, z, ds, z, t[..., :Dh], t[..., Dh:2 * Dh], g, S)
    return _rows(val, S, P), _rows(err, S, P)


# ------------------------------------------------------------------------------------------------ parameter gradients, transposes
def param_grad(dY, X, fault=None):
    """mixer_param_grad_kernel, kind 0: dW = dY^T X and db = sum_r dY[r], R rows in index order: (R + 1) u sum|.|."""
    R = dY.shape[0]
    dW = dY.T @ X
    db = (dY[1:] if fault == "bias_skip_row0" else dY).sum(0)
    return (dW, (R + 1) * U * (dY.abs().T @ X.abs()) + TINY), (db, (R + 1) * U * dY.abs().sum(0))


def affine_grad(dY, X, stats, fault=None):
    """kind 1: dgamma[k] = sum_r (dY (X - mean)) rstd (three roundings a term), dbeta[k] = sum_r dY."""
    R = dY.shape[0]
    mean, rstd = stats[:, :1], stats[:, 1:]
    t = dY * (X - mean) * rstd
    dg = (dY * X if fault == "dgamma_unnormalised" else t).sum(0)
    return (dg, (R + 3) * U * t.abs().sum(0) + TINY), (dY.sum(0), (R + 1) * U * dY.abs().sum(0))


def transpose(W, fault=None):
    """mixer_transpose_kernel: W [N, K] -> [K, N], exact."""
    N, K = W.shape
    WT = W.T.contiguous()
    if fault == "transpose_tail":
        if N % 32:
            WT[:, N - N % 32:] = 0
        if K % 32:
            WT[K - K % 32:] = 0
    return WT, torch.zeros_like(WT)


# ------------------------------------------------------------------------------------------------ the launches in order
def shapes(case):
    """Every buffer of a case: name -> shape (workspace slots, operands, upstream gradients, outputs, gradient buffers)."""
    P, dt, dv, D, nd = case
    S = 2 + nd
    R = S * P
    sh = {"x0": (R, D), "st1": (R, 2), "y1": (R, D), "qkv": (R, 3 * D), "o": (R, D), "x1": (R, D), "st2": (R, 2), "z": (R, D), "h": (R, 4 * D),
          "g": (R, 4 * D), "x2": (R, D), "out16": (R, D), "d_x2": (R, D), "dh": (R, 4 * D), "dz": (R, D), "d_x1": (R, D), "d_o": (R, D),
          "dqkv": (R, 3 * D), "dy": (R, D), "d_x0": (R, D), "T_cq": (D, dt), "T_vq": (D, dv), "T_pr": (4 * D, D), "T_fc": (D, 4 * D), "T_o": (D, D),
          "T_in": (D, 3 * D), "T_cp": (dt, D), "T_vp": (dv, D),
          "coop": (P, dt), "vpt": (P, dv), "coop_pre_w": (D, dt), "coop_pre_b": (D,), "vpt_pre_w": (D, dv), "vpt_pre_b": (D,), "ln1_g": (D,), "ln1_b": (D,),
          "in_w": (3 * D, D), "in_b": (3 * D,), "out_w": (D, D), "out_b": (D,), "ln2_g": (D,), "ln2_b": (D,), "fc_w": (4 * D, D), "fc_b": (4 * D,),
          "proj_w": (D, 4 * D), "proj_b": (D,), "coop_post_w": (dt, D), "coop_post_b": (dt,), "vpt_post_w": (dv, D), "vpt_post_b": (dv,),
          "d_coop": (P, dt), "d_vpt": (P, dv), "coop_out": (P, dt), "vpt_out": (P, dv)}
    if nd:
        sh.update({"pm": (P * S * S,), "dsm": (P * S * S,), "xv": ((S - 1) * P, dv), "dv_all": ((S - 1) * P, dv), "deep": (nd * P, dv), "d_deep": (nd * P, dv),
                   "deep_out": (nd * P, dv), "g:deep": (nd * P, dv)})
    sh.update({"g:" + n: sh[n] for n in MIXER_TENSORS})
    return sh


TRANSPOSES = (("T_cq", "coop_post_w"), ("T_vq", "vpt_post_w"), ("T_pr", "proj_w"), ("T_fc", "fc_w"), ("T_o", "out_w"), ("T_in", "in_w"), ("T_cp", "coop_pre_w"),
              ("T_vp", "vpt_pre_w"))


def steps(case, hl, eps=LN_EPS, c=GELU_C, round_prompt_grads=True):
    """The operations of one forward and backward in launch order: [(step, direction, fn)], fn(b, fault) -> {buffer: (value, bound)} with b the dict of
    the buffers written so far (a launch with a prologue is two steps: the prologue's saved result, then the Linear on that SAVED result).  hl: the
    fp16 Linears (grip_upt_mixer.half_linears).  eps, c: the kernel's f32 constants (tests/test_host_mixer_ref.py passes the exact ones of the
    module graph); round_prompt_grads: the rounding of the prompt gradients with hl, which a graph with float64 leaves does not have."""
    P, dt, dv, D, nd = case
    S = 2 + nd
    deep = nd > 0
    Z = torch.zeros_like

    def cat(*parts):
        return tuple(torch.cat(x) for x in zip(*parts))

    def exact(t):
        return t, Z(t)

    def rounded(name, vb, on):
        return f16_pair(name, *vb) if on else {name: vb}

    def pre(b, f):
        parts = [linear(b["coop"], b["coop_pre_w"], b["coop_pre_b"], f), linear(b["vpt"], b["vpt_pre_w"], b["vpt_pre_b"], f)]
        if deep:
            parts.append(linear(b["deep"], b["vpt_pre_w"], b["vpt_pre_b"], f))
        out = rounded("x0", cat(*parts), hl)
        if deep:
            out["xv"] = exact(torch.cat((b["vpt"], b["deep"])))
        return out

    def ln(src, g_, b_, y, st):
        def fn(b, f):
            yv, sv = ln_pro(b[src], b[g_], b[b_], eps)
            return {y: yv, st: sv}
        return fn

    def attn(b, f):
        out = attention(b["qkv"], S, P, D, f)
        if not deep:
            del out["pm"]
        return out

    def post(b, f):
        o16 = b["out16"]
        out = rounded("coop_out", linear(o16[:P], b["coop_post_w"], b["coop_post_b"], f), hl)
        out.update(rounded("vpt_out", linear(o16[P:2 * P], b["vpt_post_w"], b["vpt_post_b"], f), hl))
        if deep:
            out.update(rounded("deep_out", linear(o16[2 * P:], b["vpt_post_w"], b["vpt_post_b"], f), hl))
        return out

    def d_x2(b, f):
        parts = [linear(b["d_coop"], b["T_cq"]), linear(b["d_vpt"], b["T_vq"])]
        if deep:
            parts.append(linear(b["d_deep"], b["T_vq"]))
        out = f16_pair("d_x2", *cat(*parts), skip=f == "skip_round_d_x2")
        if deep:
            out["dv_all"] = exact(torch.cat((b["d_vpt"], b["d_deep"])))
        return out

    def d_x0(b, f):
        rows = None
        if f == "deep_stats_first_token":
            rows = torch.arange(S * P, device=b["dy"].device)
            rows = torch.where(rows >= 2 * P, rows % P, rows)
        return rounded("d_x0", ln_bwd_add(b["dy"], b["x0"], b["ln1_g"], b["st1"], b["d_x1"], rows), hl)

    def prompt_grads(b, f):
        on = hl and round_prompt_grads
        d = b["d_x0"]
        out = rounded("g:coop", linear(d[:P], b["T_cp"]), on)
        out.update(rounded("g:vpt", linear(d[P:2 * P], b["T_vp"]), on))
        if deep:
            out.update(rounded("g:deep", linear(d[2 * P:], b["T_vp"]), on))
        return out

    def param_grads(b, f):
        out = {}
        dv_rows, xv = (b["dv_all"], b["xv"]) if deep else (b["d_vpt"], b["vpt"])
        for w, dY, X in (("coop_post", b["d_coop"], b["out16"][:P]), ("vpt_post", dv_rows, b["out16"][P:]), ("proj", b["d_x2"], b["g"]),
                         ("fc", b["dh"], b["z"]), ("out", b["d_x1"], b["o"]), ("in", b["dqkv"], b["y1"]), ("coop_pre", b["d_x0"][:P], b["coop"]),
                         ("vpt_pre", b["d_x0"][P:], xv)):
            out["g:" + w + "_w"], out["g:" + w + "_b"] = param_grad(dY, X, f)
        out["g:ln2_g"], out["g:ln2_b"] = affine_grad(b["dz"], b["x1"], b["st2"], f)
        out["g:ln1_g"], out["g:ln1_b"] = affine_grad(b["dy"], b["x0"], b["st1"], f)
        return out

    def dqkv(b, f):
        if deep:
            return {"dqkv": attention_bwd(b["qkv"], b["d_o"], b["pm"], b["dsm"], S, P, D)}
        return {"dqkv": attention_bwd_two(b["qkv"], b["d_o"], P, D)}

    fwd = [("pre", pre),
           ("ln1", ln("x0", "ln1_g", "ln1_b", "y1", "st1")),
           ("in_proj", lambda b, f: {"qkv": linear(b["y1"], b["in_w"], b["in_b"], f)}),
           ("attn", attn),
           ("out_proj", lambda b, f: {"x1": resid(b["x0"], b["o"], b["out_w"], b["out_b"])}),
           ("ln2", ln("x1", "ln2_g", "ln2_b", "z", "st2")),
           ("fc", lambda b, f: {"h": linear(b["z"], b["fc_w"], b["fc_b"])}),
           ("gelu", lambda b, f: {"g": gelu(b["h"], f, c)}),
           ("proj", lambda b, f: {"x2": resid(b["x1"], b["g"], b["proj_w"], b["proj_b"])}),
           ("out16", lambda b, f: {"out16": exact(r16(b["x2"]))}),
           ("post", post)]
    bwd = [("transpose", lambda b, f: {t: transpose(b[w], f) for t, w in TRANSPOSES}),
           ("d_x2", d_x2),
           ("dh", lambda b, f: {"dh": gelugrad(b["d_x2"], b["T_pr"], b["h"], f, c)}),
           ("dz", lambda b, f: {"dz": linear(b["dh"], b["T_fc"])}),
           ("d_x1", lambda b, f: {"d_x1": ln_bwd_add(b["dz"], b["x1"], b["ln2_g"], b["st2"], b["d_x2"], None, f)}),
           ("d_o", lambda b, f: {"d_o": linear(b["d_x1"], b["T_o"])})]
    if deep:
        bwd.append(("dsm", lambda b, f: {"dsm": attention_ds(b["qkv"], b["d_o"], b["pm"], S, P, D)}))
    bwd += [("dqkv", dqkv),
            ("dy", lambda b, f: {"dy": linear(b["dqkv"], b["T_in"])}),
            ("d_x0", d_x0),
            ("prompt_grads", prompt_grads),
            ("param_grads", param_grads)]
    def guarded(fn):
        """A fault reaches the values only: the bounds are those of the fault-free evaluation."""
        def g(b, f=None):
            clean = fn(b, None)
            if f is None:
                return clean
            faulty = fn(b, f)
            return {n: (faulty[n][0], clean[n][1]) for n in clean}
        return g

    return [(n, "forward", guarded(fn)) for n, fn in fwd] + [(n, "backward", guarded(fn)) for n, fn in bwd]


def run(case, hl, b, **kw):
    """Chain the steps: every step reads what the earlier ones wrote.  b: the operands and upstream gradients; returns b with every buffer added."""
    b = dict(b)
    for _, _, fn in steps(case, hl, **kw):
        out = fn(b, None)
        for name, (v, _) in out.items():
            if not name.endswith("#f16"):
                b[name] = r16(v) if name + "#f16" in out else v
    return b


def worst_ratio(got, value, bound):
    """max |got - value| / bound over the elements (0 where both vanish; inf where a zero bound is exceeded or got is not finite)."""
    err = (got - value).abs()
    inf = torch.full_like(err, math.inf)
    err = torch.where(torch.isfinite(err), err, inf)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), inf)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    return ratio.max().item() if ratio.numel() else 0.0


def residual16(t):
    return t - r16(t)


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(case, family, hl, seed=0):
    """The 22 tensors, deep prompts and upstream gradients (float32, CPU).  randn: init-like, weights at K^-1/2, prompts at 0.02.  large: in_proj and c_fc
    scaled up so that the softmax is peaked and |h| reaches about 10, gamma spread over a factor of 16, biases 0.5.  hl: every value an fp16 number."""
    P, dt, dv, D, nd = case
    sh = shapes(case)
    g = torch.Generator().manual_seed(1000 * seed + 7 * P + dt + dv + D + nd)
    big = family == "large"
    if family not in FAMILIES:
        raise ValueError(family)
    b = {}
    for n in MIXER_TENSORS:
        s = sh[n]
        if n in ("coop", "vpt"):
            t = 0.02 * torch.randn(s, generator=g)
        elif n.endswith("_w"):
            t = torch.randn(s, generator=g) * s[-1] ** -0.5 * (3.0 if big and n in ("in_w", "fc_w") else 1.0)
        elif n.endswith("_g"):
            t = torch.exp2(4 * torch.rand(s, generator=g) - 2) * (1 - 2 * (torch.rand(s, generator=g) < 0.25).float()) if big else 1 + 0.1 * torch.randn(s, generator=g)
        else:
            t = (0.5 if big else 0.1) * torch.randn(s, generator=g)
        b[n] = t
    names = ["d_coop", "d_vpt"] + (["d_deep"] if nd else [])
    for n in names:
        b[n] = torch.randn(sh[n], generator=g)
    if nd:
        b["deep"] = 0.02 * torch.randn(sh["deep"], generator=g)
    if hl:
        b = {n: t.half().float() for n, t in b.items()}
    return {n: t.float().contiguous() for n, t in b.items()}
