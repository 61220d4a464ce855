"""float64 references of the head kernels (csrc/head.hip: cosine_head, cosine_head_backward, weighted_ce) with a derived bound on |f32 kernel - value|
per element ("Row forward and head kernel tests").  Same conventions as tests/rowops_ref.py: (value, bound), first-order forward error propagation
through the kernel's own sequence of operations, u = 2^-24, inputs exact; nothing measured.

Unit costs beyond those of rowops_ref: sqrtf correctly rounded (u; hipcc's default), expf and logf 1 ulp = 2 u relative (the HIP math API accuracy table,
where rsqrtf's figure came from); a head row reduction over e columns (4 EV + 6) u sum|terms| with EV = ceil(e / 256) register vectors per lane (four adds per
vector, six levels of wave_sum), plus u per product; l2norm_rows_kernel walks scalars (`i += 64`): e / 64 in-lane adds + 6.  exp(z + dz) - exp(z) is bounded with
expm1(dz), not to first order; every result that can underflow (expf, a probability, a gradient) carries 2^-126 absolute.

`fault` names ONE deliberate error applied to the float64 value only (tests/test_host_head_ref.py)."""
import torch

from rowops_ref import U

SQRT_REL = U
EXP_REL = 2.0 * U
LOG_REL = 2.0 * U
TINY = 2.0 ** -126                     # an f32 result below the smallest normal number: gradual underflow or a flush to zero moves it by less than this
FAULTS = ("scale_twice", "text_not_normalised", "last_class_dropped", "drop_projection", "drop_rows_3_mod_4", "count_zero_weight_row", "one_hot_at_label_plus_1")
E_LIST = (4, 252, 256, 260, 512, 1024, 1028, 2048)


def _ev(e):
    return (e // 4 + 63) // 64


def _sm(t):
    return t.sum(-1, keepdim=True)


def _norm(x, depth):
    """(nrm, E(nrm)) of rows x: q = sum x^2 through a reduction `depth` u deep (+ u per product), sqrtf."""
    q = _sm(x * x)
    e_q = (depth + 1) * U * q
    nrm = q.sqrt()
    return nrm, 0.5 * e_q / nrm + SQRT_REL * nrm, q, e_q


def first_argmax(v):
    """Index of the first maximum of every row."""
    j = torch.arange(v.shape[-1], device=v.device).expand_as(v)
    return torch.where(v == v.max(-1, keepdim=True).values, j, torch.full_like(j, v.shape[-1])).min(-1).values


def cosine_head(img, txt, scale, fault=None):
    """logits = (scale (x / |x|)) . (t / |t|), probs = softmax.  img [n, e], txt [c, e] f32 -> ((logits, E), (probs, E))."""
    x, t = img.double(), txt.double()
    e, c = x.shape[-1], t.shape[0]
    R = (4 * _ev(e) + 6) * U
    tn_nrm, e_tn_nrm, _, _ = _norm(t, (e + 63) // 64 + 6)
    tn = t / tn_nrm
    e_tn = t.abs() * e_tn_nrm / tn_nrm ** 2 + U * tn.abs()
    if fault == "text_not_normalised":
        tn = t
    nrm, e_nrm, _, _ = _norm(x, 4 * _ev(e) + 6)
    xn = x / nrm
    e_xn = x.abs() * e_nrm / nrm ** 2 + U * xn.abs()
    xs = scale * xn
    e_xs = scale * e_xn + U * xs.abs()
    if fault == "scale_twice":
        xs = scale * xs
    lg = xs @ tn.T
    a_tn = (t / tn_nrm).abs()
    a_xs = (scale * xn).abs()
    e_lg = e_xs @ a_tn.T + a_xs @ e_tn.T + (U + R) * (a_xs @ a_tn.T)
    # softmax: m the row max of the computed logits (within max E of the true one), z = lg - m, expf, sum of ceil(c / 64) in-lane terms + wave_sum, one divide
    m = lg.max(-1, keepdim=True).values
    z = lg - m
    e_z = e_lg + e_lg.max(-1, keepdim=True).values + U * z.abs()
    ex = z.exp()
    e_ex = ex * torch.expm1(e_z) + EXP_REL * ex * e_z.exp() + TINY
    used = ex[:, :-1] if (fault == "last_class_dropped" and c > 1) else ex
    sm = _sm(used)
    true_sm = _sm(ex)
    e_sm = _sm(e_ex) + ((c + 63) // 64 + 6) * U * true_sm
    p = ex / sm
    e_p = e_ex / true_sm + ex * e_sm / true_sm ** 2 + U * (ex / true_sm) + TINY
    return (lg, e_lg), (p, e_p)


def cosine_head_bwd(self_rows, other, scale, dl, fault=None):
    """grad[r] = (acc - x proj) / |x| with acc = sum_j other[j] (scale dl[r, j] / |other[j]|), proj = <x, acc> / |x|^2.  dl [n_self, n_other] (the text side passes the
    transposed view).  Wave w adds the rows j = w, w + 8, ... and w + 4, w + 12, ... interleaved (all j = w mod 4 in index order: at most ceil(n_other / 4) adds),
    the four waves are added ((a0 + p0) + p1) + p2: a sum ceil(n_other / 4) + 3 adds deep."""
    x, o, dl = self_rows.double(), other.double(), dl.double()
    e, n_other = x.shape[-1], o.shape[0]
    ev = _ev(e)
    R = (4 * ev + 6) * U
    _, _, qo, e_qo = _norm(o, 4 * ev + 6)
    g = scale * dl / qo.sqrt().T                                     # [n_self, n_other]: one multiply, sqrtf, one divide
    e_g = g.abs() * (U + 0.5 * (e_qo / qo).T + SQRT_REL + U)
    if fault == "drop_rows_3_mod_4":
        keep = (torch.arange(n_other, device=x.device) % 4 != 3).double()
        acc = (g * keep) @ o
    else:
        acc = g @ o
    a_terms = g.abs() @ o.abs()
    e_acc = e_g @ o.abs() + U * a_terms + ((n_other + 3) // 4 + 3) * U * a_terms
    q = _sm(x * x)
    e_q = (4 * ev + 7) * U * q
    dot = _sm(x * acc)
    e_dot = _sm(x.abs() * e_acc + U * (x * acc).abs()) + R * _sm((x * acc).abs())
    inv = q.rsqrt()
    e_inv = inv * (0.5 * e_q / q + SQRT_REL + U)
    proj = dot / q
    e_proj = e_dot / q + dot.abs() * e_q / q ** 2 + U * proj.abs()
    m = x * proj
    e_m = x.abs() * e_proj + U * m.abs()
    if fault == "drop_projection":
        m = torch.zeros_like(m)
    r = acc - m
    e_r = e_acc + e_m + U * (acc - x * proj).abs()
    out = r * inv
    return out, inv * e_r + (acc - x * proj).abs() * e_inv + U * (r * inv).abs()


def weighted_ce(logits, labels, weight, fault=None):
    """loss = sum_i w_i (lse_i - x_i[label_i]) over the rows with w_i != 0 and 0 <= label_i < c; grad_i = w_i (softmax_i - onehot(label_i)), no one-hot for a label
    outside [0, c).  lse = m + logf(sum expf(x - m)); rows walked w, w + 4, ... per wave (ceil(n / 4) adds), the four partials ((p0 + p1) + p2) + p3."""
    x, w = logits.double(), weight.double()[:, None]
    n, c = x.shape
    lab = labels.long()
    m = x.max(-1, keepdim=True).values
    z = x - m
    e_z = U * z.abs()
    ex = z.exp()
    e_ex = ex * torch.expm1(e_z) + EXP_REL * ex * e_z.exp() + TINY
    sm = _sm(ex)
    e_sm = _sm(e_ex) + ((c + 63) // 64 + 6) * U * sm
    lg = sm.log()
    lse = m + lg
    e_lse = e_sm / sm + LOG_REL * lg.abs() + U * lse.abs()
    valid = ((lab >= 0) & (lab < c))[:, None]
    xl = x.gather(1, lab.clamp(0, c - 1)[:, None])
    diff = lse - xl
    e_diff = e_lse + U * diff.abs()
    term = w * diff
    e_term = w.abs() * e_diff + U * term.abs()
    counted = valid & (w != 0)
    if fault == "count_zero_weight_row":
        term = torch.where(w == 0, diff, term)
        counted = valid
    loss = (term * counted).sum()
    e_loss = (e_term * counted).sum() + ((n + 3) // 4 + 3) * U * (term.abs() * counted).sum()
    p = ex / sm
    e_p = e_ex / sm + ex * e_sm / sm ** 2 + U * p + TINY
    hot_at = lab + 1 if fault == "one_hot_at_label_plus_1" else lab
    hot = (torch.arange(c, device=x.device)[None] == hot_at[:, None]).double()
    d = p - hot
    grad = w * d
    true_d = p - (torch.arange(c, device=x.device)[None] == lab[:, None]).double()
    e_grad = w.abs() * (e_p + U * true_d.abs()) + U * (w * true_d).abs() + TINY
    return (loss, e_loss), (grad, e_grad)


def head_inputs(n, c, e, seed, device="cpu"):
    """Un-normalised embeddings with some structure: image rows lean towards one text row each, so that a softmax at scale 100 has a clear winner on most rows."""
    g = torch.Generator().manual_seed(seed)
    txt = torch.randn(c, e, generator=g) * (0.5 + torch.rand(c, 1, generator=g))
    img = torch.randn(n, e, generator=g) * (0.5 + 2 * torch.rand(n, 1, generator=g)) + 0.5 * txt[torch.randint(0, c, (n,), generator=g)]
    return img.float().to(device), txt.float().to(device)


def excluded_share(ref, bound):
    """Share of rows whose float64 top-two gap is within twice the bound (the arg-max is not compared there)."""
    if ref.shape[-1] < 2:
        return 0.0, torch.ones(ref.shape[0], dtype=torch.bool, device=ref.device)
    top = ref.topk(2, dim=-1)
    clear = (top.values[:, 0] - top.values[:, 1]) > 2 * bound.max(-1).values
    return 1.0 - clear.double().mean().item(), clear


# (n, c, e, scale, seed) of tests/test_gpu_head_kernels.py: the 16-wave form runs n <= 64 and e <= 1024, the 4-wave form everything else.  Every n, c and e of the
# issue's lists appears with both forms where the form allows it (n = 65, e = 1028 and e = 2048 exist in the 4-wave form only).
HEAD_CASES = ((1, 1, 4, 1.0), (3, 3, 252, 100.0), (64, 4, 256, 1.0), (1, 5, 260, 100.0), (3, 63, 512, 1.0), (64, 64, 1024, 100.0), (3, 65, 4, 100.0),
              (1, 102, 512, 100.0), (3, 1023, 256, 1.0), (64, 1024, 260, 100.0),
              (65, 1, 4, 100.0), (65, 3, 252, 1.0), (65, 4, 256, 100.0), (65, 5, 260, 1.0), (65, 63, 512, 100.0), (65, 64, 1024, 1.0), (1, 65, 1028, 1.0),
              (3, 102, 2048, 100.0), (64, 1023, 1028, 100.0), (65, 1024, 2048, 1.0), (64, 102, 2048, 100.0))


def head_case_seed(n, c, e):
    return 1000 * n + 10 * c + e
