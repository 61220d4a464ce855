"""CPU: the derived bounds of tests/rowops_ref.py hold for f32 arithmetic in three reduction orders and are not vacuous (what makes
tests/test_gpu_rowops_bwd.py meaningful).  No GPU, no library call.

(a) The formulas of csrc/rowops_bwd.hip evaluated in numpy float32 with the row sums taken sequentially, pairwise and in reverse: every element of every
    family and width is within the bound.  The worst |err| / bound is printed and written to tests/_out/rowops_ref_host.json.
(b) Ten single faults applied to the float64 value: each exceeds the bound on at least one element."""
import numpy as np
import pytest
import torch

import rowops_ref as RR
from conftest import write_report

F = np.float32
ORDERS = ("sequential", "pairwise", "reversed")
_REPORT = {}


def _rsum(v, order):
    """f32 sum over the last axis in a stated order, kept as [..., 1]."""
    v = v.astype(F)
    if order == "sequential":
        return np.cumsum(v, axis=-1, dtype=F)[..., -1:]
    if order == "reversed":
        return np.cumsum(v[..., ::-1], axis=-1, dtype=F)[..., -1:]
    while v.shape[-1] > 1:
        if v.shape[-1] % 2:
            v = np.concatenate([v, np.zeros(v.shape[:-1] + (1,), F)], axis=-1)
        v = v[..., 0::2] + v[..., 1::2]
    return v


def _ln_bwd_f32(x, dyp, gamma, order):
    """ln_bwd_row in float32: the same operations in the same sequence, each rounded to f32."""
    x, dyp, gamma = x.numpy().astype(F), dyp.numpy().astype(F), gamma.numpy().astype(F)
    d = F(x.shape[-1])
    dy = dyp[0]
    for p in range(1, dyp.shape[0]):
        dy = dy + dyp[p]
    mean = _rsum(x, order) / d
    c = x - mean
    rstd = F(1) / np.sqrt(_rsum(c * c, order) / d + F(1e-5))
    xh = c * rstd
    g = dy * gamma
    a = _rsum(g, order) / d
    b = _rsum(g * xh, order) / d
    out = (g - a - xh * b) * rstd
    assert out.dtype == F
    return out


def _ratio(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref.numpy()) / bound.numpy()).max())


@pytest.mark.parametrize("family", RR.FAMILIES)
@pytest.mark.parametrize("d", RR.WIDTHS)
def test_bound_holds_for_f32_in_three_reduction_orders(d, family):
    M, parts, B, P = 24, 3, 8, 3
    x, dyp, gamma = RR.make_inputs(family, M, d, parts, seed=d + len(family))
    old = torch.randn(M, d, generator=torch.Generator().manual_seed(d)).float()
    ref, bound = RR.ln_bwd_add(x, dyp, gamma, old)
    hb = bound + RR.half_bound(ref, bound)
    # the prompt slice on the same rows: B images x P tokens, prefix = the first P rows of x (f32), summed over the batch in index order
    dx = torch.zeros(B, 1 + P, d)
    dx[:, 1:] = dyp[0].reshape(B, P, d)
    pre = x[:P].float()
    pref, pbound = RR.vit_prefix_grad(dx.reshape(-1, d), pre, gamma, 2.0 ** -7, B, 1 + P, P, 0)
    worst = {}
    for order in ORDERS:
        got = _ln_bwd_f32(x, dyp, gamma, order) + old.numpy()
        worst[order + ".dx"] = _ratio(got, ref, bound)
        worst[order + ".dxh"] = _ratio(got.astype(np.float16), ref, hb)
        rows = _ln_bwd_f32(pre.repeat(B, 1, 1).reshape(B * P, d), dx[:, 1:].reshape(1, B * P, d), gamma, order).reshape(B, P, d)
        acc = np.zeros((P, d), F)
        for i in range(B):
            acc = acc + rows[i]
        worst[order + ".prefix_grad"] = _ratio(acc * F(2.0 ** -7), pref, pbound)
    _REPORT[f"{family}.d{d}"] = {k: round(v, 4) for k, v in worst.items()}
    write_report("rowops_ref_host.json", _REPORT)
    print(f"{family} d={d}: worst |err| / bound = {max(worst.values()):.3f} ({max(worst, key=worst.get)})")
    assert max(worst.values()) <= 1.0, worst


def _exceeds(value, ref, bound):
    return bool(((value - ref).abs() > bound).any())


def _fault_case(fault, family, d):
    """Does the faulted float64 value leave the bound of the unfaulted one on at least one element?"""
    M, parts = 10, 3
    x, dyp, gamma = RR.make_inputs(family, M, d, parts, seed=7 * d + len(family))
    g = torch.Generator().manual_seed(d)
    if fault in ("read_row_off_by_one", "add_every_row"):
        stride = 5
        index = torch.tensor([2, 4], dtype=torch.int32)
        add = torch.randn(M // stride, d, generator=g)
        ref, bound = RR.ln_bwd_init(x, dyp, gamma, add, index, stride)
        hit = _exceeds(RR.ln_bwd_init(x, dyp, gamma, add, index, stride, fault)[0], ref, bound)
        if fault == "read_row_off_by_one":      # the scatter forms take the same decision
            sref, sbound, _ = RR.ln_bwd_scatter(x, dyp[0, :2], gamma, index, stride, M)
            hit = hit and _exceeds(RR.ln_bwd_scatter(x, dyp[0, :2], gamma, index, stride, M, fault)[0], sref, sbound)
        return hit
    if fault == "skip_image":
        B, S, P = 5, 2, 1                        # dyp[0] as the stream gradient of 5 sequences of 2 rows, one prompt row each
        dx, pre = dyp[0], x[:P].float()
        ref, bound = RR.vit_prefix_grad(dx, pre, gamma, 0.5, B, S, P, 0)
        hit = _exceeds(RR.vit_prefix_grad(dx, pre, gamma, 0.5, B, S, P, 0, fault)[0], ref, bound)
        tref, tbound = RR.text_prefix_grad(dx, 0.5, B, S, P, 1)
        return hit and _exceeds(RR.text_prefix_grad(dx, 0.5, B, S, P, 1, fault)[0], tref, tbound)
    if fault == "scale_exponent_off_by_one":
        s0, s1, g16 = RR.grad_scale_cast(dyp[0] * 1e-3)
        f0, f1, fg16 = RR.grad_scale_cast(dyp[0] * 1e-3, fault)
        return f0 != s0 and f1 != s1 and not torch.equal(g16, fg16)          # the bound is zero: everything about this kernel is exact
    old = torch.randn(M, d, generator=g)
    ref, bound = RR.ln_bwd_add(x, dyp, gamma, old)
    return _exceeds(RR.ln_bwd_add(x, dyp, gamma, old, fault)[0], ref, bound)


NAMED_FAMILY = {"no_eps": "flat", "drop_b": "spiky"}


@pytest.mark.parametrize("fault", RR.FAULTS)
def test_each_single_fault_exceeds_the_bound(fault):
    """Asserted at every width on the family the fault is named for (randn where none is named); the other families are recorded."""
    caught = {fam: [d for d in RR.WIDTHS if _fault_case(fault, fam, d)] for fam in RR.FAMILIES}
    _REPORT.setdefault("faults", {})[fault] = {fam: ("all widths" if len(ds) == len(RR.WIDTHS) else ds) for fam, ds in caught.items()}
    write_report("rowops_ref_host.json", _REPORT)
    print(f"{fault}: caught at widths {caught}")
    assert caught[NAMED_FAMILY.get(fault, "randn")] == list(RR.WIDTHS), caught
