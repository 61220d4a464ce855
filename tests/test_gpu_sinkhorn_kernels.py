"""grip_sinkhorn_balance (csrc/sinkhorn.hip) through the C ABI: every element of Q, mass and log_scale against float64 on the same inputs under the
bound that tests/sinkhorn_ref.py derives (nothing in it comes from a measurement), pred exactly the first maximum of the kernel's own row, two calls
bit-equal, a bare step's rows bit-equal between the full matrix and a row subset, zero columns and an all-zero P finite with unit rows, the refusals
with nothing written.  NaN guard rows sit behind every operand and output and the workspace starts as 0xFF bytes (NaNs): a read of anything the call
did not write itself would show.  The worst |err| / bound per case goes to tests/_out/sinkhorn.json."""
import ctypes

import pytest
import torch

import sinkhorn_ref as R
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
    """x on the device with GUARD rows of NaN behind it."""
    x = x.reshape(-1, 1) if x.dim() == 1 else x
    buf = torch.full((x.shape[0] + GUARD,) + tuple(x.shape[1:]), float("nan"), device="cuda", dtype=x.dtype)
    buf[:x.shape[0]] = x
    return buf[:x.shape[0]]


def _balance(p, lt, tau, iters, b0=None, want_pred=True):
    native, lib = _lib()
    n, c = p.shape
    pg, lg = _guarded(p), _guarded(lt)
    bg = _guarded(b0) if b0 is not None else None
    q = torch.full((n + GUARD, c), float("nan"), device="cuda")
    pred = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    mass = torch.full((c + GUARD,), float("nan"), device="cuda")
    b = torch.full((c + GUARD,), float("nan"), device="cuda")
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_sinkhorn_workspace(n, c, ctypes.byref(nbytes)))
    ws = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device="cuda")
    native.check(lib.grip_sinkhorn_balance(_p(pg), _p(lg), _p(bg), tau, iters, n, c, _p(q), _p(pred) if want_pred else None, _p(mass), _p(b), _p(ws),
                                           ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(q[n:]).all() and (pred[n:] == -1).all() and torch.isnan(mass[c:]).all() and torch.isnan(b[c:]).all(), "a guard row was written"
    assert torch.isfinite(q[:n]).all() and torch.isfinite(mass[:c]).all() and torch.isfinite(b[:c]).all(), "an owned output element was not written (or is not finite)"
    assert (pred[:n] >= 0).all() if want_pred else (pred == -1).all()
    return q[:n], pred[:n], mass[:c], b[:c]


@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_every_element_against_float64(case):
    p, lt, tau, iters, b0 = (t.cuda() if torch.is_tensor(t) else t for t in R.case_operands(case))
    q, pred, mass, b = _balance(p, lt, tau, iters, b0)
    ratio = R.check_balance(p, lt, tau, iters, b0, q, pred, mass, b)
    _REPORT[R.case_id(case)] = round(ratio, 4)
    write_report("sinkhorn.json", _REPORT)
    print(f"balance {R.case_id(case)}: worst |err| / bound = {ratio:.3f}")
    if iters == 0:
        assert torch.equal(b, b0 if b0 is not None else torch.zeros_like(b)), "a bare step must hand the start vector back"
    again = _balance(p, lt, tau, iters, b0)
    assert all(torch.equal(x, y) for x, y in zip(again, (q, pred, mass, b))), "two calls differ"


@pytest.mark.parametrize("c", [64, 102, 129])        # one and two classes per lane in registers / waiting in the output row
def test_a_bare_steps_rows_do_not_depend_on_n_or_on_their_place(c):
    n = 8 * R.ROWS + 5
    p = R.inputs(n, c, "plain", seed=5).cuda()
    lt = R.log_target_of(c, device="cuda")
    b0 = R.advanced_start(p, lt, 1.0).cuda()
    q, pred, _, _ = _balance(p, lt, 1.0, 0, b0)
    rows = torch.tensor([n - 1, 3, R.ROWS, 2 * R.ROWS + 7, 0], device="cuda")       # other places in other chunks, another n
    qs, ps, _, _ = _balance(p[rows].contiguous(), lt, 1.0, 0, b0)
    assert torch.equal(qs, q[rows]) and torch.equal(ps, pred[rows])
    q1, _, m1, _ = _balance(p[7:8].contiguous(), lt, 1.0, 0, b0, want_pred=False)      # n = 1; pred is optional
    assert torch.equal(q1, q[7:8]) and torch.equal(m1, q[7])


@pytest.mark.parametrize("c", [65, 300])
def test_pred_takes_the_first_maximum(c):
    """Classes 7 and c - 1 (two different lane passes) are bit-equal in P, in the prior and in the start vector: their Q columns are bit-equal and, where
    they carry the row's maximum, pred is the lower index."""
    n = 37
    p = R.inputs(n, c, "plain", seed=12)
    p[:, 7] = p[:, c - 1] = 2 * p.max(dim=1).values * (torch.arange(n) % 2)       # the twins win every other row
    p = p.cuda()
    lt = R.log_target_of(c, device="cuda")
    q, pred, mass, b = _balance(p, lt, 1.0, 0)
    assert torch.equal(q[:, 7], q[:, c - 1])
    twins_win = q[:, 7] == q.max(dim=1).values
    assert twins_win.sum() == n // 2 and (pred[twins_win] == 7).all()
    R.check_balance(p, lt, 1.0, 0, None, q, pred, mass, b)


@pytest.mark.parametrize("c", [102, 300])
@pytest.mark.parametrize("kind", ["zerocol", "allzero"])
def test_zero_columns_stay_finite_with_unit_rows(c, kind):
    """A column of P that is zero in every row is legal: its b_c rises until the class has its share, filled with arbitrary rows.  Nothing is claimed
    about those values beyond: finite, non-negative, rows summing to 1 within (c + 8) u."""
    n = 2 * R.ROWS + 1
    p = R.inputs(n, c, "plain", seed=21)
    if kind == "zerocol":
        p[:, c // 2] = 0.0
    else:
        p[:] = 0.0
    p = p.cuda()
    lt = R.log_target_of(c, device="cuda")
    for iters in (0, 3, 10):
        q, pred, mass, b = _balance(p, lt, 1.0, iters)        # (asserts every output finite)
        assert (q >= 0).all() and ((q.double().sum(1) - 1).abs() <= (c + 8) * R.U).all()
        assert (pred.long() == torch.from_numpy(q.cpu().numpy().argmax(1)).cuda()).all()
    if kind == "zerocol":
        assert mass[c // 2] > 0.5 * n / c, "ten iterations must have given the empty class a share"
    else:
        assert torch.allclose(q, torch.full_like(q, 1.0 / c), rtol=1e-5)


def test_refusals():
    native, lib = _lib()
    n, c = 5, 64
    p = R.inputs(n, c, "plain", seed=9).cuda()
    lt = R.log_target_of(c, device="cuda")
    q = torch.full((n, c), float("nan"), device="cuda")
    mass, b = (torch.full((c,), float("nan"), device="cuda") for _ in range(2))
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def refused(word, tau=1.0, iters=3, n=n, c=c, pp=p, qq=q, mm=mass, ws_bytes=None):
        rc = lib.grip_sinkhorn_balance(_p(pp), _p(lt), None, tau, iters, n, c, _p(qq), None, _p(mm), _p(b), _p(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                       _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("tau = 0", tau=0.0)
    refused("tau = -1", tau=-1.0)
    refused("tau = inf", tau=float("inf"))
    refused("tau = nan", tau=float("nan"))
    refused("iters = -1", iters=-1)
    refused("n = 0", n=0)
    refused("c = 0", c=0)
    refused("null pointer", pp=None)
    refused("alias", qq=p)
    refused("alias", mm=b)
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_sinkhorn_workspace(n, c, ctypes.byref(nbytes)))
    refused("workspace too small", ws_bytes=nbytes.value - 1)
    torch.cuda.synchronize()
    assert torch.isnan(q).all() and torch.isnan(mass).all() and torch.isnan(b).all() and torch.isfinite(p).all()


def test_engine_call_checks_its_operands_and_normalises_the_prior():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    n, c = 2 * R.ROWS + 1, 102
    p = R.inputs(n, c, "plain", seed=3).cuda()
    prior = torch.arange(1, c + 1, dtype=torch.float32)
    q, pred, mass, b = engine.sinkhorn_balance(p, tau=0.5, iters=3, prior=7 * prior)          # (an un-normalised prior on the CPU)
    lt = R.log_target_of(c, prior, device="cuda")
    R.check_balance(p, lt, 0.5, 3, None, q, pred, mass, b)
    q2, pred2, mass2, b2 = engine.sinkhorn_balance(p, tau=0.5, iters=0, prior=prior.cuda(), log_scale=b)       # the returned vector continues the recursion
    assert torch.equal(q2, q) and torch.equal(pred2, pred) and torch.equal(mass2, mass) and torch.equal(b2, b)
    q3, _, _, _ = engine.sinkhorn_balance(p.half(), iters=0)                                    # (any floating-point probabilities; defaults: uniform, tau 1)
    R.check_balance(p.half().float(), R.log_target_of(c, device="cuda"), 1.0, 0, None, q3, None, q3.sum(0), torch.zeros(c, device="cuda"))
    for bad, word in ((dict(probs=p[0]), "probs must be"), (dict(probs=p.long()), "probs must be"), (dict(prior=prior[:5]), "prior must be"),
                      (dict(prior=-prior), "finite positive"), (dict(prior=prior * float("nan")), "finite positive"), (dict(log_scale=b[:5]), "log_scale must be"),
                      (dict(log_scale=b.cpu()), "log_scale must be"), (dict(log_scale=b.double()), "log_scale must be"), (dict(tau=0.0), "tau = 0"),
                      (dict(iters=-1), "iters = -1")):
        with pytest.raises(native.GripError, match=word):
            engine.sinkhorn_balance(**{"probs": p, **bad})
    with pytest.raises(native.GripError):
        engine.sinkhorn_balance(p.cpu())
