"""float64 references of the backward row kernels (csrc/rowops_bwd.hip) with a derived bound on |f32 kernel - value| per element
("Row backward kernel tests").  Plain torch float64 on whatever device the inputs live on; nothing here calls the library.

Every function returns (value, bound), both float64 and of the output's shape.  The bound is first-order forward error propagation through the
kernel's own sequence of operations with u = 2^-24: the inputs are exact (x f16 or f32, everything else f32, as the kernel reads them), each f32 add,
multiply and divide contributes u |result|, a row reduction (4 NV + 6) u sum|terms| (4 NV in-lane adds, six levels of wave_sum), a sum of p partials in
index order (p - 1) u sum|partials|, rsqrtf one ulp (2 u), and errors propagate through every later operation with the absolute value of its partial
derivative.  Nothing in a bound is measured.

`fault` names ONE deliberate error applied to the float64 value (never to the bound): tests/test_host_rowops_ref.py shows with them that the
bound is not vacuous."""
import math

import numpy as np
import torch

U = 2.0 ** -24
LN_EPS = float(np.float32(1e-5))       # the kernel's `1e-5f`
DIV_REL = U                            # f32 division: correctly rounded (hipcc's default, no fast-math): half an ulp
RSQRT_REL = 2.0 * U                    # rsqrtf: 1 ulp (HIP math API accuracy table)
HALF_U = 2.0 ** -11
FAMILIES = ("randn", "flat", "spiky")
WIDTHS = (128, 256, 320, 512, 768, 1024, 1280, 1792, 2048)
FAULTS = ("no_eps", "d_plus_4", "drop_last_partial", "drop_a", "drop_b", "gamma_tail_one", "read_row_off_by_one", "add_every_row", "skip_image",
          "scale_exponent_off_by_one")


def nv_of(d):
    """The register-vector count DISPATCH_NV_B instantiates for width d (5 is served by 6, 7 by 8)."""
    nv = (d // 4 + 63) // 64
    assert d % 4 == 0 and 1 <= nv <= 8, d
    return {5: 6, 7: 8}.get(nv, nv)


def _red(d):
    return (4 * nv_of(d) + 6) * U


def half_bound(ref, bound):
    """What the f16 copy of an f32 value within `bound` of `ref` adds: one rounding to f16 (relative above 2^-14, 2^-25 absolute below)."""
    return HALF_U * (ref.abs() + bound) + 2.0 ** -25


def ln_bwd(x, dyp, gamma, fault=None):
    """LNbwd(sum_p dyp[p]; x) per row, as ln_bwd_row computes it.  x [M, d], dyp [p, M, d], gamma [d] -> (value, bound) [M, d]."""
    x, dyp, gamma = x.double(), dyp.double(), gamma.double()
    d = x.shape[-1]
    R = _red(d)
    p = dyp.shape[0]
    if fault == "drop_last_partial":
        dyp = dyp[:-1]
    if fault == "gamma_tail_one":
        gamma = gamma.clone()
        gamma[-4:] = 1.0
    dd = d + 4 if fault == "d_plus_4" else d
    eps = 0.0 if fault == "no_eps" else LN_EPS
    sm = lambda t: t.sum(-1, keepdim=True)

    dy = dyp.sum(0)
    e_dy = (p - 1) * U * dyp.abs().sum(0)
    mean = sm(x) / dd
    e_mean = R * sm(x.abs()) / d + DIV_REL * mean.abs()
    c = x - mean
    e_c = e_mean + U * c.abs()                                   # the cancellation: e_mean is relative to |x|, not to |c|
    q = sm(c * c)
    e_q = sm(2 * c.abs() * e_c + U * c * c) + R * q
    var = q / dd
    e_var = e_q / d + DIV_REL * var
    v = var + eps
    e_v = e_var + U * v
    rstd = v.rsqrt()
    e_rstd = 0.5 * rstd / v * e_v + RSQRT_REL * rstd
    xh = c * rstd
    e_xh = rstd * e_c + c.abs() * e_rstd + U * xh.abs()
    g = dy * gamma
    e_g = gamma.abs() * e_dy + U * g.abs()
    a = sm(g) / dd
    e_a = (sm(e_g) + R * sm(g.abs())) / d + DIV_REL * a.abs()
    t = g * xh
    e_t = xh.abs() * e_g + g.abs() * e_xh + U * t.abs()
    b = sm(t) / dd
    e_b = (sm(e_t) + R * sm(t.abs())) / d + DIV_REL * b.abs()
    if fault == "drop_a":
        a = torch.zeros_like(a)
    if fault == "drop_b":
        b = torch.zeros_like(b)
    m = xh * b
    e_m = b.abs() * e_xh + xh.abs() * e_b + U * m.abs()
    r1 = g - a
    e_r1 = e_g + e_a + U * r1.abs()
    r2 = r1 - m
    e_r2 = e_r1 + e_m + U * r2.abs()
    out = r2 * rstd
    e_out = rstd * e_r2 + r2.abs() * e_rstd + U * out.abs()
    return out, e_out


def ln_bwd_add(x, dyp, gamma, old, fault=None):
    """dx = old + LNbwd(...): one more rounded add."""
    out, e = ln_bwd(x, dyp, gamma, fault)
    ref = old.double() + out
    return ref, e + U * ref.abs()


def read_rows(n, stride, index, device):
    """Row b * stride + index[b] of each of the n sequences (index None: position 0)."""
    pos = torch.zeros(n, dtype=torch.long, device=device) if index is None else index.to(device).long()
    return torch.arange(n, device=device) * stride + pos


def ln_bwd_init(x, dyp, gamma, rows_add, index, stride, fault=None):
    """dx[r] = LNbwd(...)[r] + (r is the read row of sequence r // stride ? rows_add[r // stride] : 0)."""
    out, e = ln_bwd(x, dyp, gamma, fault)
    M = x.shape[0]
    n = (M + stride - 1) // stride
    at = read_rows(n, stride, index, x.device)
    if fault == "read_row_off_by_one":
        at = at + 1
    add = torch.zeros_like(out)
    if fault == "add_every_row":
        add = rows_add.double()[torch.arange(M, device=x.device) // stride]
    else:
        keep = at < M
        add[at[keep]] = rows_add.double()[:n][keep]
    ref = out + add
    return ref, e + U * ref.abs() * (add != 0)


def ln_bwd_scatter(x, dy, gamma, index, stride, M, fault=None):
    """dx[b * stride + index[b]] = LNbwd(dy[b]; x[that row]) for b < n; (value, bound, rows) with value zero and bound zero on every other row of the M."""
    n = dy.shape[0]
    at = read_rows(n, stride, index, x.device)
    if fault == "read_row_off_by_one":
        at = (at + 1) % M
    out, e = ln_bwd(x[at], dy[None], gamma, fault)
    ref = torch.zeros(M, x.shape[-1], dtype=torch.float64, device=x.device)
    bound = torch.zeros_like(ref)
    ref[at], bound[at] = out, e
    return ref, bound, at


def vit_prefix_grad(dx, prefix, gamma, inv, B, S, P, mode, fault=None):
    """mode 0: grad[s] = inv sum_b LNbwd(dx[b S + 1 + s]; prefix[s]); 1: grad[b, s] = inv LNbwd(dx[b S + 1 + s]; prefix[b, s]); 2: grad[s] = inv sum_b dx[b S + 1 + s].
    The batch sum adds (B - 1) u sum|terms| (B - 1 adds of non-zero partial sums, in whatever tree), the scale one rounded multiply."""
    d = dx.shape[-1]
    rows = dx.reshape(B, S, d)[:, 1:1 + P]                        # [B, P, d]
    if mode == 2:
        terms, e = rows.double(), torch.zeros(B, P, d, dtype=torch.float64, device=dx.device)
    else:
        pre = prefix.reshape(1, P, d).expand(B, P, d) if mode == 0 else prefix.reshape(B, P, d)
        terms, e = ln_bwd(pre.reshape(B * P, d), rows.reshape(1, B * P, d), gamma, fault)
        terms, e = terms.reshape(B, P, d), e.reshape(B, P, d)
    if mode == 1:
        ref = terms * inv
        return ref, e * inv + U * ref.abs()
    used = terms[:-1] if fault == "skip_image" else terms
    ref = used.sum(0) * inv
    return ref, (e.sum(0) + (B - 1) * U * terms.abs().sum(0)) * inv + U * ref.abs()


def text_prefix_grad(dx, inv, C, T, P, prefix_classes, fault=None):
    """grad[pc, p] = inv x (sum_c dx[c T + 1 + p] when prefix_classes == 1, dx[pc T + 1 + p] when == C)."""
    d = dx.shape[-1]
    rows = dx.reshape(C, T, d)[:, 1:1 + P].double()
    if prefix_classes != 1:
        ref = rows * inv
        return ref, U * ref.abs()
    used = rows[:-1] if fault == "skip_image" else rows
    ref = used.sum(0, keepdim=True) * inv
    return ref, (C - 1) * U * rows.abs().sum(0, keepdim=True) * inv + U * ref.abs()


def grad_scale_cast(g, fault=None):
    """(scale[0], scale[1], g16): everything exact.  scale[0] = 2^k, amax 2^k in [32, 64), |k| <= 40; k = 0 for a zero or non-finite amax."""
    amax = g.abs().max().item() if g.numel() else 0.0
    k = 0
    if amax > 0 and math.isfinite(amax):
        k = max(-40, min(40, 6 - math.frexp(amax)[1]))
    if fault == "scale_exponent_off_by_one":
        k += 1
    return 2.0 ** k, 2.0 ** -k, (g.float() * (2.0 ** k)).half()


def make_inputs(family, M, d, parts, seed, device="cpu"):
    """(x f16 [M, d], dyp f32 [parts, M, d], gamma f32 [d]).  randn; flat: x = c + 0.01 randn, 1 <= |c| <= 8 per row (variance ~1e-4: LN_EPS and the
    cancellation in x - mean matter); spiky: one element per row 100 x the others and a sign-alternating dy (a and b are sums that cancel)."""
    g = torch.Generator().manual_seed(seed)
    gamma = 1 + 0.3 * torch.randn(d, generator=g)
    dyp = torch.randn(parts, M, d, generator=g)
    if family == "randn":
        x = torch.randn(M, d, generator=g)
    elif family == "flat":
        c = (1 + 7 * torch.rand(M, 1, generator=g)) * (1 - 2 * (torch.arange(M)[:, None] % 2))
        x = c + 0.01 * torch.randn(M, d, generator=g)
        dyp = 0.25 * dyp                      # rstd ~ 100: keeps the f16 copy of dx far inside the f16 range
    elif family == "spiky":
        x = torch.randn(M, d, generator=g)
        j = torch.randint(0, d, (M,), generator=g)
        x[torch.arange(M), j] *= 100
        dyp = (1 - 2 * (torch.arange(d) % 2)) * (1 + 0.1 * dyp)
    else:
        raise ValueError(family)
    return x.half().to(device), dyp.float().to(device), gamma.float().to(device)
