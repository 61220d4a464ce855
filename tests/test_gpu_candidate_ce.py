"""grip_candidate_ce (csrc/candidate.hip) through the C ABI: every element of loss and grad_logits against float64 on the same operands under the bound
that tests/candidate_ref.py derives (nothing in it comes from a measurement) over soft_ce_ref's grid, with cz < c, a permuting col_map and mixed hard /
candidate / empty rows; bit-equality with grip_weighted_ce for cand = NULL at every (n, c); a singleton set gives the hard row's bits; two calls
bit-equal; a row's bits equal between the full batch and a permuted subset; the refusals with nothing written; the engine's operand checks and
CandidateCEFn.  NaN guard rows sit behind every operand and output.  The worst |err| / bound per case goes to tests/_out/candidate_ce.json."""
import ctypes

import numpy as np
import pytest
import torch

import candidate_ref as R
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


def _candidate_ce(x, lab, w, cand=None, cand_row=None, col_map=None, want_grad=True):
    """(loss [1], grad or None) of one call on guarded operands; asserts that nothing outside the outputs was written."""
    native, lib = _lib()
    n, c = x.shape
    xg, lg, wg = _guarded(x), _guarded(lab), _guarded(w)
    cg, rg, mg = (_guarded(t) if t is not None else None for t in (cand, cand_row, col_map))
    loss = torch.full((1 + GUARD,), float("nan"), device="cuda")
    grad = torch.full((n + GUARD, c), float("nan"), device="cuda")
    rows, cz = (0, 0) if cand is None else (cand.shape[0], col_map.shape[0])
    native.check(lib.grip_candidate_ce(_p(xg), _p(lg), _p(wg), n, c, _p(cg), rows, cz, _p(rg), _p(mg), _p(loss), _p(grad if want_grad else None), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(loss[1:]).all() and torch.isnan(grad[n:]).all(), "a guard row was written"
    assert torch.isfinite(grad[:n]).all() if want_grad else torch.isnan(grad).all()
    return loss[:1], grad[:n] if want_grad else None


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
        x, lab, w, cand, row, cmap = (t.cuda() for t in R.operands(n, c, cz))
        loss, grad = _candidate_ce(x, lab, w, cand, row, cmap)
        ref = R.candidate_ce64(x, lab, w, cand, row, cmap)
        case = f"{n}x{c}-cz{cz}"
        ratio = R.check(ref, loss, grad)
        _REPORT[case] = round(ratio, 4)
        print(f"candidate_ce {case}: worst |err| / bound = {ratio:.3f}")
        assert (grad[ref["empty"]] == 0).all(), "an empty set must leave a zero gradient row"
        _, member = R.members(cand, row, cmap, n, c)
        live = ref["is_cand"] & ~ref["empty"]
        onehot = torch.arange(c, device="cuda")[None] == lab[:, None]
        pull = torch.where(ref["is_cand"][:, None], member, onehot)          # the columns whose gradient carries a subtracted target
        positive = (w > 0)[:, None] & ~pull & ~ref["empty"][:, None]
        assert (grad[positive] >= 0).all(), "outside its set a row's gradient is w softmax >= 0"
        assert int(live.sum()) + int(ref["empty"].sum()) == int(ref["is_cand"].sum())
        again = _candidate_ce(x, lab, w, cand, row, cmap)
        assert torch.equal(again[0], loss) and torch.equal(again[1], grad), "two calls differ"
        only_loss, none = _candidate_ce(x, lab, w, cand, row, cmap, want_grad=False)
        assert none is None and torch.equal(only_loss, loss)
    write_report("candidate_ce.json", _REPORT)


@pytest.mark.parametrize("n,c", R.SHAPES, ids=[f"{n}x{c}" for n, c in R.SHAPES])
def test_without_sets_it_is_weighted_ce_bit_for_bit(n, c):
    x, lab, w, cand, row, cmap = (t.cuda() for t in R.operands(n, c, R.czs(c)[-1]))
    want_loss, want_grad = _weighted_ce(x, lab, w)
    loss, grad = _candidate_ce(x, lab, w)                                           # cand = NULL
    assert torch.equal(loss, want_loss) and torch.equal(grad, want_grad)
    all_hard = torch.full_like(row, -1)
    loss, grad = _candidate_ce(x, lab, w, cand, all_hard, cmap)                     # a matrix nobody points into
    assert torch.equal(loss, want_loss) and torch.equal(grad, want_grad)
    _, mixed = _candidate_ce(x, lab, w, cand, row, cmap)                            # the hard rows of a mixed batch
    hard = (row < 0) | (row >= cand.shape[0])
    assert torch.equal(mixed[hard], want_grad[hard])


@pytest.mark.parametrize("n,c", R.SHAPES, ids=[f"{n}x{c}" for n, c in R.SHAPES])
def test_a_singleton_set_is_the_hard_rows_bits(n, c):
    x, lab, w, _, _, _ = (t.cuda() for t in R.operands(n, c, c))
    lab = lab.clamp(0, c - 1)                                                       # every row carries a label a set can hold
    want_loss, want_grad = _weighted_ce(x, lab, w)
    cmap = torch.randperm(c, generator=torch.Generator().manual_seed(c)).to(torch.int32)
    inverse = torch.empty(c, dtype=torch.long)
    inverse[cmap.long()] = torch.arange(c)
    single = np.zeros((n, c), dtype=bool)
    single[np.arange(n), inverse[lab.cpu().long()].numpy()] = True                  # mask column j with col_map[j] = label
    cand = torch.from_numpy(R.pack(single).copy()).cuda()
    rows = torch.arange(n, dtype=torch.int32, device="cuda")
    loss, grad = _candidate_ce(x, torch.full_like(lab, -1), w, cand, rows, cmap.cuda())
    assert torch.equal(grad, want_grad) and torch.equal(loss, want_loss)


@pytest.mark.parametrize("c", [64, 102, 300])
def test_a_rows_bits_do_not_depend_on_n_or_on_its_place(c):
    n = 67
    x, lab, w, cand, row, cmap = (t.cuda() for t in R.operands(n, c, c - 1))
    _, grad = _candidate_ce(x, lab, w, cand, row, cmap)
    rows = torch.tensor([n - 1, 3, 16, 39, 0, 2, 4, 1, 6, 5, 7, 8], device="cuda")      # other waves, other places, another n
    _, gs = _candidate_ce(x[rows].contiguous(), lab[rows].contiguous(), w[rows].contiguous(), cand, row[rows].contiguous(), cmap)
    assert torch.equal(gs, grad[rows])
    _, g1 = _candidate_ce(x[2:3].contiguous(), lab[2:3].contiguous(), w[2:3].contiguous(), cand, row[2:3].contiguous(), cmap)      # n = 1
    assert torch.equal(g1, grad[2:3])


def test_a_col_map_entry_outside_the_logits_is_skipped():
    n, c, cz = 5, 65, 64
    x, lab, w, cand, row, cmap = (t.cuda() for t in R.operands(n, c, cz))
    cmap = cmap.clone()
    cmap[0], cmap[cz // 2] = -1, c                                                  # row 3 of sets() holds exactly these two mask columns: now empty
    loss, grad = _candidate_ce(x, lab, w, cand, row, cmap)
    ref = R.candidate_ce64(x, lab, w, cand, row, cmap)
    R.check(ref, loss, grad)
    assert bool(ref["empty"][row == 3].all()) and (grad[row == 3] == 0).all()


def test_refusals():
    native, lib = _lib()
    n, c, cz = 5, 64, 63
    x, lab, w, cand, row, cmap = (t.cuda() for t in R.operands(n, c, cz))
    loss = torch.full((1,), float("nan"), device="cuda")
    grad = torch.full((n, c), float("nan"), device="cuda")

    def refused(word, n=n, c=c, cz=cz, xx=x, ll=lab, ww=w, cc=cand, rr=row, mm=cmap, out=loss):
        rc = lib.grip_candidate_ce(_p(xx), _p(ll), _p(ww), n, c, _p(cc), cand.shape[0], cz, _p(rr), _p(mm), _p(out), _p(grad), _stream())
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
    refused("c = 16001", c=16001, cz=1)
    torch.cuda.synchronize()
    assert torch.isnan(loss).all() and torch.isnan(grad).all()
    assert lib.grip_candidate_ce(_p(x), _p(lab), _p(w), n, c, None, 0, 0, None, None, _p(loss), None, _stream()) == 0      # cand = NULL needs neither
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()


def test_engine_call_checks_its_operands_and_autograd():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    n, c, cz = 5, 102, 101
    x, lab, w, cand, row, cmap = (t.cuda() for t in R.operands(n, c, cz))
    loss, grad = engine.candidate_ce(x, lab, w, cand, row, cmap)
    assert loss.dim() == 0
    ref = R.candidate_ce64(x, lab, w, cand, row, cmap)
    R.check(ref, loss, grad)
    l0, g0 = engine.candidate_ce(x, lab.long(), w)                                   # defaults: grip_weighted_ce's bits
    wl, wg = _weighted_ce(x, lab, w)
    assert torch.equal(l0.reshape(1), wl) and torch.equal(g0, wg)
    xr = x.clone().requires_grad_(True)
    out = engine.CandidateCEFn.apply(xr, lab, w, cand, row, cmap)
    (3.0 * out).backward()
    assert torch.equal(out.detach(), loss) and torch.equal(xr.grad, grad * 3.0)
    # the gradient autograd returns is the reference's: a central difference of the float64 loss along a random direction agrees with <grad, direction>
    d = torch.randn(n, c, generator=torch.Generator().manual_seed(1)).cuda().double()
    h = 1e-6
    up = R.candidate_ce64((x.double() + h * d), lab, w, cand, row, cmap)["loss"]
    down = R.candidate_ce64((x.double() - h * d), lab, w, cand, row, cmap)["loss"]
    in_loss = (ref["counted"] | ref["empty"])[:, None]                               # (a hard row outside the loss keeps w softmax: no loss term behind it)
    slope = float(((xr.grad.double() / 3.0) * d * in_loss).sum())
    assert abs(float((up - down) / (2 * h)) - slope) <= 1e-5 * max(1.0, abs(slope))
    dup = cmap.clone()
    dup[1] = dup[0]
    big = cmap.clone()
    big[0] = c
    for bad, word in ((dict(logits=x[0]), "logits must be"), (dict(labels=lab[:3]), "labels must be"), (dict(labels=w), "labels must be"),
                      (dict(row_weight=w[:3]), "row_weight must be"), (dict(cand=cand.long()), "cand must be"), (dict(cand=cand.cpu()), "cand must be"),
                      (dict(cand=cand[:, :1]), "cand must be"), (dict(cand_row=row.long()), "cand_row must be"), (dict(cand_row=row[:3]), "cand_row must be"),
                      (dict(col_map=cmap.long()), "col_map must be"), (dict(col_map=None), "col_map must be"), (dict(col_map=dup), "distinct"),
                      (dict(col_map=big), "distinct")):
        args = dict(logits=x, labels=lab, row_weight=w, cand=cand, cand_row=row, col_map=cmap)
        with pytest.raises(native.GripError, match=word):
            engine.candidate_ce(**{**args, **bad})
    with pytest.raises(native.GripError):
        engine.candidate_ce(x.cpu(), lab.cpu(), w.cpu())
