"""float64 reference, bound and inputs for the soft-target cross-entropy kernel (csrc/soft_ce.hip, grip_soft_ce), shared by the GPU tests and checked against
an independent oracle on the host (tests/test_host_soft_ce_ref.py).  Everything works on torch tensors of any device.  Conventions of tests/head_ref.py:
(value, bound) per element, first-order forward error propagation through the kernel's own sequence of operations, u = 2^-24, expf and logf 1 ulp = 2 u
relative (the HIP math API accuracy table), inputs exact, every result that can underflow carries 2^-126 absolute; nothing in the bound is measured.  The
reference runs in float64 on the SAME f32 operands (logits, weights, the matrix, float(1 / temperature), float(smoothing)): only the arithmetic differs.

THE RECURSION (include/grip_amd.h).  Row i with 0 <= soft_row[i] < soft_rows is SOFT: a_j = inv_t log max(soft[r, j], 2^-126), s[col_map[j]] = softmax_j(a),
0 elsewhere.  Any other row is HARD: s = onehot(labels[i]), or 0 for a label outside [0, c).  Every row: t = (1 - eps) s + eps / c, T = sum_k t_k,
term_i = w_i (T lse_i - sum_k t_k x_ik), loss = sum of the terms of the rows with w_i != 0 that are soft or carry a label in [0, c);
grad_i = w_i (T softmax(x_i) - t_i).  A hard row with a label outside [0, c) keeps grip_weighted_ce's rule: out of the loss, s = 0 and T := 1 exactly (the whole
softmax stays; with eps = 0 the gradient is w_i softmax(x_i)).

THE BOUND.
    a        logf 2 u, the product u:                                                e_a = 3 u |a|
    softmax  over the cz matrix columns as tests/head_ref.py bounds the one over the logits: the kernel's maximum is that of its own a (within max e_a),
             zz = a - mx rounds once:  e_zz = e_a + max_j e_a + u |zz|;  expf:  e_ex = ex expm1(e_zz) + 2 u ex e^{e_zz} + 2^-126;  the sum of ceil(cz / 64)
             in-lane terms and six wave levels:  e_ss = sum e_ex + (ceil(cz / 64) + 6) u ss;  the division:  e_s = e_ex / ss + ex e_ss / ss^2 + u s + 2^-126
             a hard row's s is exact.  The scatter moves values, it rounds nothing.
    t        keep = 1 - eps and floor = eps / c round once each, the product and the sum once each:
             e_t = keep e_s + 2 u keep s + u floor + u t + 2^-126
    T, dot   sums of ceil(c / 64) in-lane terms + six wave levels:  e_T = sum e_t + (ceil(c / 64) + 6) u T;
             e_dot = sum (e_t |x| + u |t x|) + (ceil(c / 64) + 6) u sum |t x|
    lse, p   as head_ref.weighted_ce
    term     tl = T lse, d = tl - dot, term = w d:  e_term = |w| (e_T |lse| + T e_lse + u |tl| + e_dot + u |d|) + u |term|
    loss     ceil(n / 4) in-wave adds and three across the waves:  e_loss = sum e_term + (ceil(n / 4) + 3) u sum |term|
    grad     tp = T p, d = tp - t, g = w d:  e_g = |w| (e_T p + T e_p + u |tp| + e_t + u |d|) + u |g| + 2^-126
A hard row without smoothing runs grip_weighted_ce's shorter sequence (w (lse - x[label]), w (p - onehot)): each of its roundings is one of the above with
T = 1, t = onehot exact, so the same bound covers it."""
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
EXP_REL = 2.0 * U
LOG_REL = 2.0 * U


def _sm(t):
    return t.sum(-1, keepdim=True)


def _depth(c):
    return (c + 63) // 64 + 6


def sharpen64(z, inv_t):
    """(s, e_s) of softmax_j(inv_t log max(z, 2^-126)) over the last dim, in float64 with the bound of the module docstring."""
    cz = z.shape[-1]
    a = inv_t * torch.log(z.double().clamp_min(TINY))
    e_a = (LOG_REL + U) * a.abs()
    mx = a.max(-1, keepdim=True).values
    zz = a - mx
    e_zz = e_a + e_a.max(-1, keepdim=True).values + U * zz.abs()
    ex = zz.exp()
    e_ex = ex * torch.expm1(e_zz) + EXP_REL * ex * e_zz.exp() + TINY
    ss = _sm(ex)
    e_ss = _sm(e_ex) + _depth(cz) * U * ss
    s = ex / ss
    return s, e_ex / ss + ex * e_ss / ss ** 2 + U * s + TINY


def soft_ce64(logits, labels, weight, soft=None, soft_row=None, col_map=None, inv_t=1.0, smoothing=0.0):
    """dict of the float64 values and bounds: loss, e_loss (0-d); grad, e_grad, target, e_target [n, c]; term, e_term [n] and counted [n] (the rows in the
    loss); is_soft [n].  inv_t and smoothing are taken as the f32 numbers the kernel receives."""
    x, w = logits.double(), weight.double()[:, None]
    n, c = x.shape
    dev = x.device
    inv_t = float(torch.tensor(inv_t, dtype=torch.float32))
    eps = float(torch.tensor(smoothing, dtype=torch.float32))
    lab = labels.long()
    valid = (lab >= 0) & (lab < c)
    cols = torch.arange(c, device=dev)
    s = ((cols[None] == lab[:, None]) & valid[:, None]).double()
    e_s = torch.zeros_like(s)
    is_soft = torch.zeros(n, dtype=torch.bool, device=dev)
    if soft is not None:
        r = soft_row.long()
        is_soft = (r >= 0) & (r < soft.shape[0])
        if bool(is_soft.any()):
            sz, e_sz = sharpen64(soft[r[is_soft]], inv_t)
            full, e_full = torch.zeros(sz.shape[0], c, dtype=torch.float64, device=dev), torch.zeros(sz.shape[0], c, dtype=torch.float64, device=dev)
            full[:, col_map.long()] = sz
            e_full[:, col_map.long()] = e_sz
            s[is_soft], e_s[is_soft] = full, e_full
    keep, floor_ = 1.0 - eps, eps / c
    t = keep * s + floor_
    e_t = keep * e_s + 2 * U * keep * s + U * floor_ + U * t + TINY
    T = _sm(t)
    e_T = _sm(e_t) + _depth(c) * U * T
    out_of_range = (~is_soft & ~valid)[:, None]
    T = torch.where(out_of_range, torch.ones_like(T), T)
    e_T = torch.where(out_of_range, torch.zeros_like(e_T), e_T)
    tx = t * x
    dot = _sm(tx)
    e_dot = _sm(e_t * x.abs() + U * tx.abs()) + _depth(c) * U * _sm(tx.abs())
    # lse and p: tests/head_ref.py, weighted_ce
    m = x.max(-1, keepdim=True).values
    z = x - m
    e_z = U * z.abs()
    ex = z.exp()
    e_ex = ex * torch.expm1(e_z) + EXP_REL * ex * e_z.exp() + TINY
    sm = _sm(ex)
    e_sm = _sm(e_ex) + _depth(c) * U * sm
    lg = sm.log()
    lse = m + lg
    e_lse = e_sm / sm + LOG_REL * lg.abs() + U * lse.abs()
    p = ex / sm
    e_p = e_ex / sm + ex * e_sm / sm ** 2 + U * p + TINY
    tl = T * lse
    d = tl - dot
    term = w * d
    e_term = w.abs() * (e_T * lse.abs() + T * e_lse + U * tl.abs() + e_dot + U * d.abs()) + U * term.abs()
    counted = ((w[:, 0] != 0) & (is_soft | valid))[:, None]
    loss = (term * counted).sum()
    e_loss = (e_term * counted).sum() + ((n + 3) // 4 + 3) * U * (term.abs() * counted).sum() + TINY
    tp = T * p
    dg = tp - t
    grad = w * dg
    e_grad = w.abs() * (e_T * p + T * e_p + U * tp.abs() + e_t + U * dg.abs()) + U * grad.abs() + TINY
    return dict(loss=loss, e_loss=e_loss, grad=grad, e_grad=e_grad, target=t, e_target=e_t, term=term[:, 0], e_term=e_term[:, 0], counted=counted[:, 0],
                is_soft=is_soft)


def check(ref, loss, grad=None, target=None):
    """Assert every element of the kernel's outputs against `ref` (soft_ce64); returns the worst |err| / bound."""
    worst = 0.0
    for name, got, want, b in (("loss", loss, ref["loss"], ref["e_loss"]), ("grad", grad, ref["grad"], ref["e_grad"]),
                               ("target", target, ref["target"], ref["e_target"])):
        if got is None:
            continue
        err = (got.double().reshape(want.shape) - want).abs()
        ratio = float((err / b).max())
        assert bool(torch.isfinite(got).all()) and bool((err <= b).all()), f"soft_ce: |{name} - {name}64| is {ratio:.2f} x its bound"
        worst = max(worst, ratio)
    return worst


def soft_ce_f32(logits, labels, weight, soft=None, soft_row=None, col_map=None, inv_t=1.0, smoothing=0.0):
    """An f32 emulation of the kernel in torch (no fused multiply-add, torch's own summation order): what the checker must accept.  (loss, grad, target)."""
    x, w = logits.float(), weight.float()[:, None]
    n, c = x.shape
    lab = labels.long()
    valid = (lab >= 0) & (lab < c)
    s = ((torch.arange(c)[None] == lab[:, None]) & valid[:, None]).float()
    is_soft = torch.zeros(n, dtype=torch.bool)
    if soft is not None:
        r = soft_row.long()
        is_soft = (r >= 0) & (r < soft.shape[0])
        a = torch.tensor(inv_t, dtype=torch.float32) * torch.log(soft[r[is_soft]].clamp_min(TINY))
        e = torch.exp(a - a.max(-1, keepdim=True).values)
        full = torch.zeros(e.shape[0], c)
        full[:, col_map.long()] = e / _sm(e)
        s[is_soft] = full
    eps = torch.tensor(smoothing, dtype=torch.float32)
    t = (1 - eps) * s + eps / c
    m = x.max(-1, keepdim=True).values
    ex = torch.exp(x - m)
    sm = _sm(ex)
    lse = m + torch.log(sm)
    T = torch.where((~is_soft & ~valid)[:, None], torch.ones(n, 1), _sm(t))
    term = w * (T * lse - _sm(t * x))
    counted = ((w[:, 0] != 0) & (is_soft | valid))[:, None]
    return (term * counted).sum(), w * (T * (ex / sm) - t), t


# ------------------------------------------------------------------------------------------ inputs and cases
CS = (1, 63, 64, 65, 102, 129, 300)
NS = (1, 4, 5, 67)
TEMPERATURES = (0.5, 1.0, 2.0)
SMOOTHINGS = (0.0, 0.1)
SOFT_ROWS = 9
_ROW_PATTERN = (2, -1, 0, 1, SOFT_ROWS, 3, -1, 4, 5, -7, 6, 7, 8)        # matrix row of batch row i (cycled): < 0 and SOFT_ROWS mark hard rows


def czs(c):
    """The matrix widths of the case table: 1, c - 1 and c where they exist."""
    return sorted({v for v in (1, c - 1, c) if 1 <= v <= c})


def matrix(cz, seed):
    """soft [SOFT_ROWS, cz] f32: row 0 all zeros, row 1 with exact zeros inside, row 3 saturated (logits x 30: most entries underflow), the others softmax rows."""
    g = torch.Generator().manual_seed(seed)
    z = torch.softmax(2 * torch.randn(SOFT_ROWS, cz, generator=g), dim=1)
    z[3] = torch.softmax(30 * torch.randn(cz, generator=g), dim=0)
    z[1][torch.rand(cz, generator=g) < 0.4] = 0.0
    z[0] = 0.0
    return z.float()


def operands(n, c, cz, seed=None):
    """(logits [n, c], labels [n] int32, weight [n], soft [SOFT_ROWS, cz], soft_row [n] int32, col_map [cz] int32) on the CPU: hard and soft rows, zero weights
    (i = 3 mod 5), labels outside [0, c) on a hard row (i = 6 mod 13: label c) and on a soft one (i = 7 mod 13: -3, never read), a matrix row index
    outside the matrix, zeros inside a matrix row and an all-zero matrix row; col_map is the head of a permutation of the c columns."""
    g = torch.Generator().manual_seed(1000 * n + 10 * c + cz if seed is None else seed)
    i = torch.arange(n)
    logits = (4 * torch.randn(n, c, generator=g)).float()
    labels = torch.randint(0, c, (n,), generator=g).to(torch.int32)
    labels[i % 13 == 6] = c
    labels[i % 13 == 7] = -3
    weight = (0.25 + torch.rand(n, generator=g)).float() * torch.where(torch.rand(n, generator=g) < 0.2, -1.0, 1.0)
    weight[i % 5 == 3] = 0.0
    soft_row = torch.tensor([_ROW_PATTERN[k % len(_ROW_PATTERN)] for k in range(n)], dtype=torch.int32)
    col_map = torch.randperm(c, generator=g)[:cz].to(torch.int32)
    return logits, labels, weight.float(), matrix(cz, seed=7 * c + cz), soft_row, col_map


SHAPES = [(n, c) for n in NS for c in CS]
SETTINGS = [(t, e) for t in TEMPERATURES for e in SMOOTHINGS]


def inv_temperature(t):
    """The f32 the engine hands the kernel for a temperature."""
    return float(torch.tensor(1.0 / float(t), dtype=torch.float32))
