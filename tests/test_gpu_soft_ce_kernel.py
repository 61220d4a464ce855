"""grip_soft_ce (csrc/soft_ce.hip) through the C ABI: every element of loss, grad_logits and target_out against float64 on the same operands under the
bound that tests/soft_ce_ref.py derives (nothing in it comes from a measurement), bit-equality with grip_weighted_ce for soft = NULL and smoothing 0 at
every (n, c), two calls bit-equal, a row's bits equal between the full batch and a permuted subset, the refusals with nothing written, the optional
outputs absent.  NaN guard rows sit behind every operand and output: a write past an output or a read past an operand would show.  The worst
|err| / bound per case goes to tests/_out/soft_ce.json."""
import ctypes

import pytest
import torch

import soft_ce_ref as R
from conftest import write_report

pytestmark = pytest.mark.gpu
GUARD = 8
_REPORT = {}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native, native.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(x):
    """x on the device with GUARD rows of NaN (integers: a large negative number) behind it."""
    fill = float("nan") if x.dtype.is_floating_point else -(2 ** 30)
    buf = torch.full((x.shape[0] + GUARD,) + tuple(x.shape[1:]), fill, device="cuda", dtype=x.dtype)
    buf[:x.shape[0]] = x
    return buf[:x.shape[0]]


def _soft_ce(x, lab, w, soft=None, soft_row=None, col_map=None, inv_t=1.0, eps=0.0, want_grad=True, want_target=True):
    """(loss [1], grad or None, target or None) of one call on guarded operands; asserts that nothing outside the outputs was written."""
    native, lib = _lib()
    n, c = x.shape
    xg, lg, wg = _guarded(x), _guarded(lab), _guarded(w)
    sg, rg, mg = (_guarded(t) if t is not None else None for t in (soft, soft_row, col_map))
    loss = torch.full((1 + GUARD,), float("nan"), device="cuda")
    grad = torch.full((n + GUARD, c), float("nan"), device="cuda")
    target = torch.full((n + GUARD, c), float("nan"), device="cuda")
    rows, cz = (0, 0) if soft is None else soft.shape
    native.check(lib.grip_soft_ce(_p(xg), _p(lg), _p(wg), n, c, _p(sg), rows, cz, _p(rg), _p(mg), inv_t, eps, _p(loss), _p(grad if want_grad else None),
                                  _p(target if want_target else None), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(loss[1:]).all() and torch.isnan(grad[n:]).all() and torch.isnan(target[n:]).all(), "a guard row was written"
    assert torch.isfinite(grad[:n]).all() if want_grad else torch.isnan(grad).all()
    assert torch.isfinite(target[:n]).all() if want_target else torch.isnan(target).all()
    return loss[:1], grad[:n] if want_grad else None, target[:n] if want_target else None


def _weighted_ce(x, lab, w):
    native, lib = _lib()
    loss = torch.full((1,), float("nan"), device="cuda")
    grad = torch.full_like(x, float("nan"))
    native.check(lib.grip_weighted_ce(_p(x), _p(lab), _p(w), x.shape[0], x.shape[1], _p(loss), _p(grad), _stream()))
    torch.cuda.synchronize()
    return loss, grad


@pytest.mark.parametrize("n,c", R.SHAPES, ids=[f"{n}x{c}" for n, c in R.SHAPES])
def test_every_element_against_float64(n, c):
    for cz in R.czs(c):
        x, lab, w, soft, row, cmap = (t.cuda() for t in R.operands(n, c, cz))
        for temperature, eps in R.SETTINGS:
            inv_t = R.inv_temperature(temperature)
            loss, grad, target = _soft_ce(x, lab, w, soft, row, cmap, inv_t, eps)
            ref = R.soft_ce64(x, lab, w, soft, row, cmap, inv_t, eps)
            case = f"{n}x{c}-cz{cz}-T{temperature:g}-eps{eps:g}"
            ratio = R.check(ref, loss, grad, target)
            _REPORT[case] = round(ratio, 4)
            print(f"soft_ce {case}: worst |err| / bound = {ratio:.3f}")
            hard = ~ref["is_soft"]
            if eps == 0.0:
                unmapped = torch.ones(c, dtype=torch.bool, device="cuda")
                unmapped[cmap.long()] = False
                assert (target[~hard][:, unmapped] == 0).all(), "an unmapped column of a soft target must be exactly 0"
                onehot = (torch.arange(c, device="cuda")[None] == lab[:, None]).float()
                assert torch.equal(target[hard], onehot[hard]), "a hard row's target is its one-hot"
            again = _soft_ce(x, lab, w, soft, row, cmap, inv_t, eps)
            assert all(torch.equal(a, b) for a, b in zip(again, (loss, grad, target))), "two calls differ"
    write_report("soft_ce.json", _REPORT)


@pytest.mark.parametrize("n,c", R.SHAPES, ids=[f"{n}x{c}" for n, c in R.SHAPES])
def test_hard_rows_without_smoothing_are_weighted_ce_bit_for_bit(n, c):
    x, lab, w, soft, row, cmap = (t.cuda() for t in R.operands(n, c, R.czs(c)[-1]))
    want_loss, want_grad = _weighted_ce(x, lab, w)
    loss, grad, target = _soft_ce(x, lab, w)                                        # soft = NULL
    assert torch.equal(loss, want_loss) and torch.equal(grad, want_grad)
    loss, grad, _ = _soft_ce(x, lab, w, inv_t=0.5, want_target=False)               # (the temperature touches no hard row)
    assert torch.equal(loss, want_loss) and torch.equal(grad, want_grad)
    all_hard = torch.full_like(row, -1)
    loss, grad, _ = _soft_ce(x, lab, w, soft, all_hard, cmap)                       # a matrix nobody points into
    assert torch.equal(loss, want_loss) and torch.equal(grad, want_grad)
    _, mixed, _ = _soft_ce(x, lab, w, soft, row, cmap)                              # the hard rows of a mixed batch
    hard = (row < 0) | (row >= soft.shape[0])
    assert torch.equal(mixed[hard], want_grad[hard])


@pytest.mark.parametrize("c", [64, 102, 300])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_a_rows_bits_do_not_depend_on_n_or_on_its_place(c, eps):
    n = 67
    x, lab, w, soft, row, cmap = (t.cuda() for t in R.operands(n, c, c - 1))
    _, grad, target = _soft_ce(x, lab, w, soft, row, cmap, 2.0, eps)
    rows = torch.tensor([n - 1, 3, 16, 39, 0, 2, 4, 1, 6], device="cuda")            # other waves, other places, another n
    _, gs, ts = _soft_ce(x[rows].contiguous(), lab[rows].contiguous(), w[rows].contiguous(), soft, row[rows].contiguous(), cmap, 2.0, eps)
    assert torch.equal(gs, grad[rows]) and torch.equal(ts, target[rows])
    l1, g1, t1 = _soft_ce(x[2:3].contiguous(), lab[2:3].contiguous(), w[2:3].contiguous(), soft, row[2:3].contiguous(), cmap, 2.0, eps)      # n = 1
    assert torch.equal(g1, grad[2:3]) and torch.equal(t1, target[2:3])


def test_optional_outputs_can_be_absent():
    n, c = 5, 102
    x, lab, w, soft, row, cmap = (t.cuda() for t in R.operands(n, c, c - 1))
    full = _soft_ce(x, lab, w, soft, row, cmap, 1.0, 0.1)
    for want_grad, want_target in ((False, True), (True, False), (False, False)):
        loss, grad, target = _soft_ce(x, lab, w, soft, row, cmap, 1.0, 0.1, want_grad, want_target)
        assert torch.equal(loss, full[0])
        assert grad is None or torch.equal(grad, full[1])
        assert target is None or torch.equal(target, full[2])


def test_an_all_zero_matrix_row_is_uniform_over_the_mapped_columns():
    n, c, cz = 5, 65, 64
    x, lab, w, soft, row, cmap = (t.cuda() for t in R.operands(n, c, cz))
    _, _, target = _soft_ce(x, lab, w, soft, row, cmap, 0.5, 0.0)
    zero_rows = (row == 0)
    assert zero_rows.any()
    want = torch.zeros(c, device="cuda")
    want[cmap.long()] = 1.0 / cz
    assert torch.allclose(target[zero_rows], want.expand(int(zero_rows.sum()), c), rtol=1e-6, atol=0)


def test_refusals():
    native, lib = _lib()
    n, c, cz = 5, 64, 63
    x, lab, w, soft, row, cmap = (t.cuda() for t in R.operands(n, c, cz))
    loss = torch.full((1,), float("nan"), device="cuda")
    grad, target = (torch.full((n, c), float("nan"), device="cuda") for _ in range(2))

    def refused(word, n=n, c=c, cz=cz, inv_t=1.0, eps=0.0, xx=x, ll=lab, ww=w, ss=soft, rr=row, mm=cmap, out=loss):
        rc = lib.grip_soft_ce(_p(xx), _p(ll), _p(ww), n, c, _p(ss), soft.shape[0], cz, _p(rr), _p(mm), inv_t, eps, _p(out), _p(grad), _p(target), _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("null pointer", xx=None)
    refused("null pointer", ll=None)
    refused("null pointer", ww=None)
    refused("null pointer", out=None)
    refused("null pointer", rr=None)
    refused("null pointer", mm=None)
    refused("n = 0", n=0)
    refused("c = 0", c=0)
    refused("n = -1", n=-1)
    refused("cz = 0", cz=0)
    refused("cz = 65", cz=65)
    refused("inv_temperature = 0", inv_t=0.0)
    refused("inv_temperature = -1", inv_t=-1.0)
    refused("inv_temperature = inf", inv_t=float("inf"))
    refused("inv_temperature = nan", inv_t=float("nan"))
    refused("smoothing = -0.1", eps=-0.1)
    refused("smoothing = 1", eps=1.0)
    refused("smoothing = nan", eps=float("nan"))
    torch.cuda.synchronize()
    assert torch.isnan(loss).all() and torch.isnan(grad).all() and torch.isnan(target).all()
    assert lib.grip_soft_ce(_p(x), _p(lab), _p(w), n, c, None, 0, 0, None, None, 1.0, 0.0, _p(loss), None, None, _stream()) == 0      # soft = NULL needs neither
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()


def test_engine_call_checks_its_operands():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    n, c, cz = 5, 102, 101
    x, lab, w, soft, row, cmap = (t.cuda() for t in R.operands(n, c, cz))
    loss, grad, target = engine.soft_ce(x, lab, w, soft, row, cmap, temperature=0.5, smoothing=0.1, want_target=True)
    assert loss.dim() == 0
    R.check(R.soft_ce64(x, lab, w, soft, row, cmap, R.inv_temperature(0.5), 0.1), loss, grad, target)
    l0, g0 = engine.soft_ce(x, lab.long(), w)                                          # defaults: grip_weighted_ce's bits
    wl, wg = _weighted_ce(x, lab, w)
    assert torch.equal(l0.reshape(1), wl) and torch.equal(g0, wg)
    xr = x.clone().requires_grad_(True)
    out = engine.SoftCEFn.apply(xr, lab, w, soft, row, cmap, 0.5, 0.1)
    (3.0 * out).backward()
    assert torch.equal(out.detach(), loss) and torch.equal(xr.grad, grad * 3.0)
    dup = cmap.clone()
    dup[1] = dup[0]
    big = cmap.clone()
    big[0] = c
    for bad, word in ((dict(logits=x[0]), "logits must be"), (dict(labels=lab[:3]), "labels must be"), (dict(labels=w), "labels must be"),
                      (dict(row_weight=w[:3]), "row_weight must be"), (dict(soft=soft.double()), "soft must be"), (dict(soft=soft.cpu()), "soft must be"),
                      (dict(soft=soft[:, :5]), "soft must be"), (dict(soft_row=row.long()), "soft_row must be"), (dict(soft_row=row[:3]), "soft_row must be"),
                      (dict(col_map=cmap.long()), "col_map must be"), (dict(col_map=cmap[:7]), "col_map must be"), (dict(col_map=dup), "distinct"),
                      (dict(col_map=big), "distinct"), (dict(temperature=0.0), "temperature = 0"), (dict(temperature=float("inf")), "temperature = inf"),
                      (dict(smoothing=1.0), "smoothing = 1"), (dict(smoothing=-0.5), "smoothing = -0.5")):
        args = dict(logits=x, labels=lab, row_weight=w, soft=soft, soft_row=row, col_map=cmap)
        with pytest.raises(native.GripError, match=word):
            engine.soft_ce(**{**args, **bad})
    with pytest.raises(native.GripError):
        engine.soft_ce(x.cpu(), lab.cpu(), w.cpu())
