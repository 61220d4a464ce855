"""CPU: the derived bounds of tests/head_ref.py hold for f32 arithmetic in three reduction orders and are not vacuous (what makes
tests/test_gpu_head_kernels.py meaningful).  No GPU, no library call.

(a) The formulas of csrc/head.hip in numpy float32, every row sum formed as a wave forms it (the lane's own vectors in index order, then the 64 lane sums
    sequentially, pairwise and in reverse), at every e of the GPU test: every element is within the bound.  tests/_out/head_ref_host.json keeps the worst ratios.
(b) Seven single faults applied to the float64 value: each leaves the bound on at least one element at every e.
(c) The arg-max comparison of the GPU test leaves out the rows whose float64 top-two gap is within twice the bound: for every case and seed of the GPU test that
    share is at most 1 % on the reference alone."""
import numpy as np
import pytest
import torch

import head_ref as HR
from conftest import write_report
from test_host_rowops_fwd_ref import _ratio, _wsum
from test_host_rowops_ref import F, ORDERS

_REPORT = {}


def _head_f32(img, txt, scale, order):
    x, t = img.numpy().astype(F), txt.numpy().astype(F)
    tn = t / np.sqrt(_wsum(t * t, order, 1))
    xs = F(scale) * (x / np.sqrt(_wsum(x * x, order)))
    lg = np.stack([_wsum(xs * tn[j], order)[:, 0] for j in range(t.shape[0])], -1)
    ex = np.exp(lg - lg.max(-1, keepdims=True))
    assert ex.dtype == F
    p = ex / _wsum(ex, order, 1)
    return lg, p


def _bwd_f32(x, o, scale, dl, order):
    x, o, dl = x.numpy().astype(F), o.numpy().astype(F), dl.numpy().astype(F)
    g = F(scale) * dl / np.sqrt(_wsum(o * o, order))[:, 0]
    waves = []
    for w in range(4):
        acc = np.zeros_like(x)
        for j in range(w, o.shape[0], 4):
            acc = acc + o[j] * g[:, j:j + 1]
        waves.append(acc)
    acc = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    q = _wsum(x * x, order)
    proj = _wsum(x * acc, order) / q
    return (acc - x * proj) * (F(1) / np.sqrt(q))


def _ce_f32(x, lab, w, order):
    x, w = x.numpy().astype(F), w.numpy().astype(F)
    n, c = x.shape
    m = x.max(-1, keepdims=True)
    ex = np.exp(x - m)
    sm = _wsum(ex, order, 1)
    lse = m + np.log(sm)
    part = [F(0)] * 4
    for r in range(n):
        if w[r] != 0 and 0 <= lab[r] < c:
            part[r % 4] = part[r % 4] + w[r] * (lse[r, 0] - x[r, lab[r]])
    hot = (np.arange(c)[None] == lab.numpy()[:, None]).astype(F)
    return ((part[0] + part[1]) + part[2]) + part[3], w[:, None] * (ex / sm - hot)


def _ce_inputs(n, c, seed, spread):
    g = torch.Generator().manual_seed(seed)
    x = spread * torch.randn(n, c, generator=g)
    lab = torch.randint(0, c, (n,), generator=g).int()
    w = torch.rand(n, generator=g) * (torch.arange(n) % 3 != 1)
    return x.float(), lab, w.float()


@pytest.mark.parametrize("e", HR.E_LIST)
def test_bound_holds_for_f32_in_three_reduction_orders(e):
    n, c = 6, 70
    img, txt = HR.head_inputs(n, c, e, seed=e)
    worst = {}
    for scale in (1.0, 100.0):
        (lg, e_lg), (p, e_p) = HR.cosine_head(img, txt, scale)
        dl = (p - torch.nn.functional.one_hot(torch.arange(n) % c, c)).float() / n
        gi, e_gi = HR.cosine_head_bwd(img, txt, scale, dl)
        gt, e_gt = HR.cosine_head_bwd(txt, img, scale, dl.T)
        for order in ORDERS:
            l32, p32 = _head_f32(img, txt, scale, order)
            k = f"{order}.scale{scale:g}."
            worst[k + "logits"] = _ratio(l32, lg, e_lg)
            worst[k + "probs"] = _ratio(p32, p, e_p)
            worst[k + "grad_img"] = _ratio(_bwd_f32(img, txt, scale, dl, order), gi, e_gi)
            worst[k + "grad_txt"] = _ratio(_bwd_f32(txt, img, scale, dl.T.contiguous(), order), gt, e_gt)
    for spread in (1.0, 30.0):
        x, lab, w = _ce_inputs(9, e if e > 4 else 5, e, spread)
        (loss, e_loss), (grad, e_grad) = HR.weighted_ce(x, lab, w)
        for order in ORDERS:
            l32, g32 = _ce_f32(x, lab, w, order)
            worst[f"{order}.spread{spread:g}.loss"] = float(abs(float(l32) - loss.item()) / e_loss.item())
            worst[f"{order}.spread{spread:g}.ce_grad"] = _ratio(g32, grad, e_grad)
    per = {}
    for k, v in worst.items():
        per[k.rsplit(".", 1)[1]] = max(per.get(k.rsplit(".", 1)[1], 0.0), round(v, 4))
    _REPORT[f"e{e}"] = per
    write_report("head_ref_host.json", _REPORT)
    print(f"e={e}: {per}")
    assert max(worst.values()) <= 1.0, worst


def _exceeds(value, ref, bound):
    return bool(((value - ref).abs() > bound).any())


@pytest.mark.parametrize("fault", HR.FAULTS)
def test_each_single_fault_exceeds_the_bound(fault):
    caught = []
    for e in HR.E_LIST:
        n, c = 6, 70
        img, txt = HR.head_inputs(n, c, e, seed=3 * e)
        (lg, e_lg), (p, e_p) = HR.cosine_head(img, txt, 100.0)
        if fault in ("scale_twice", "text_not_normalised"):
            hit = _exceeds(HR.cosine_head(img, txt, 100.0, fault)[0][0], lg, e_lg)
        elif fault == "last_class_dropped":
            (p1, e_p1) = HR.cosine_head(img, txt, 1.0)[1]
            hit = _exceeds(HR.cosine_head(img, txt, 1.0, fault)[1][0], p1, e_p1)
        elif fault in ("drop_projection", "drop_rows_3_mod_4"):
            dl = (p - torch.nn.functional.one_hot(torch.arange(n) % c, c)).float() / n
            ref, bound = HR.cosine_head_bwd(img, txt, 100.0, dl)
            hit = _exceeds(HR.cosine_head_bwd(img, txt, 100.0, dl, fault)[0], ref, bound)
        else:
            x, lab, w = _ce_inputs(9, e if e > 4 else 5, e, 1.0)
            (loss, e_loss), (grad, e_grad) = HR.weighted_ce(x, lab, w)
            (floss, _), (fgrad, _) = HR.weighted_ce(x, lab, w, fault)
            hit = abs(floss - loss) > e_loss if fault == "count_zero_weight_row" else _exceeds(fgrad, grad, e_grad)
        if hit:
            caught.append(e)
    _REPORT.setdefault("faults", {})[fault] = "every e" if caught == list(HR.E_LIST) else caught
    write_report("head_ref_host.json", _REPORT)
    assert caught == list(HR.E_LIST), caught


@pytest.mark.parametrize("n,c,e,scale", HR.HEAD_CASES)
def test_argmax_exclusion_cap_on_the_reference(n, c, e, scale):
    img, txt = HR.head_inputs(n, c, e, HR.head_case_seed(n, c, e))
    (lg, e_lg), (p, e_p) = HR.cosine_head(img, txt, scale)
    s_l, s_p = HR.excluded_share(lg, e_lg)[0], HR.excluded_share(p, e_p)[0]
    _REPORT.setdefault("excluded share", {})[f"n{n}.c{c}.e{e}.scale{scale:g}"] = [s_l, s_p]
    write_report("head_ref_host.json", _REPORT)
    assert s_l <= 0.01 and s_p <= 0.01, (s_l, s_p)
