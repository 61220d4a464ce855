"""grip_probe_objective / grip_probe_fit (csrc/linear_probe.hip) through the C ABI: every element of loss, grad_w and grad_b against float64 on the same
inputs with the bounds that tests/probe_ref.py derives (nothing in them comes from a measurement), twin classes and two calls bit-equal, ignored NaN rows
never read, fit(3) = fit(1) three times, fit(1) = objective + the written update, fit(iters) against the float64 recursion, a captured graph replayed,
and the refusals with nothing written.  NaN guard rows sit behind every operand and output and the workspace starts as 0xFF bytes (NaNs): a read of
anything the call did not write itself would show.  The worst |err| / bound per family goes to tests/_out/probe.json."""
import ctypes

import numpy as np
import pytest
import torch

import probe_ref as R
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


def _guarded(x, fill=float("nan")):
    """x on the device with GUARD rows of `fill` behind it."""
    if x is None:
        return None
    x2 = x.reshape(-1, 1) if x.dim() == 1 else x
    buf = torch.full((x2.shape[0] + GUARD,) + tuple(x2.shape[1:]), fill, device="cuda", dtype=x.dtype)
    buf[:x2.shape[0]] = x2
    return buf[:x2.shape[0]]


def _guards_intact(t):
    return torch.isnan(t._base[t.shape[0]:]).all()


def _ws(query, *dims):
    native, _ = _lib()
    nbytes = ctypes.c_size_t()
    native.check(query(*dims, ctypes.byref(nbytes)))
    return torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device="cuda")


def _operands(inp):
    return dict(F=_guarded(inp["F"]), W=_guarded(inp["W"].float()), b=_guarded(None if inp["b"] is None else inp["b"].float()), base=_guarded(inp["base"]),
                y=_guarded(inp["y"], 1 << 30), soft=_guarded(inp["soft"]), r=_guarded(inp["r"]))


def _objective(inp, ops=None):
    native, lib = _lib()
    (n, e), c = inp["F"].shape, inp["W"].shape[0]
    d = ops or _operands(inp)      # (held: a freed block would be handed to the next operand)
    loss = torch.full((1 + GUARD,), float("nan"), device="cuda")
    gw = torch.full((c + GUARD, e), float("nan"), device="cuda")
    gb = torch.full((c + GUARD,), float("nan"), device="cuda")
    ws = _ws(lib.grip_probe_objective_workspace, n, c, e)
    native.check(lib.grip_probe_objective(_p(d["F"]), _p(d["W"]), _p(d["b"]), _p(d["base"]), _p(d["y"]), _p(d["soft"]), _p(d["r"]), inp["scale"], inp["norm"],
                                          n, c, e, _p(loss), _p(gw), _p(gb), _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(loss[1:]).all() and torch.isnan(gw[c:]).all() and torch.isnan(gb[c:]).all(), "a guard row of the outputs was written"
    assert torch.isfinite(loss[:1]).all() and torch.isfinite(gw[:c]).all() and torch.isfinite(gb[:c]).all(), "an owned output element is missing or not finite"
    return loss[0].cpu(), gw[:c].cpu(), gb[:c].cpu()


def _fit(inp, l2, lr, mu, iters, start=None, want_trace=True):
    """(W, b, mom_w, mom_b, trace) on the CPU after `iters` iterations from `start` = (W, b, mom_w, mom_b) (None: inp's W and b, zero momentum)."""
    native, lib = _lib()
    (n, e), c = inp["F"].shape, inp["W"].shape[0]
    d = _operands(inp)
    if start is None:
        start = (inp["W"].float(), torch.zeros(c) if inp["b"] is None else inp["b"].float(), torch.zeros(c, e), torch.zeros(c))
    g = [_guarded(t) for t in start]
    tr = torch.full((iters + GUARD,), float("nan"), device="cuda") if want_trace else None
    ws = _ws(lib.grip_probe_fit_workspace, n, c, e)
    native.check(lib.grip_probe_fit(_p(d["F"]), _p(d["base"]), _p(d["y"]), _p(d["soft"]), _p(d["r"]), inp["scale"], inp["norm"], l2, lr, mu, iters, n, c, e,
                                    _p(g[0]), _p(g[1]), _p(g[2]), _p(g[3]), _p(tr), _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert all(_guards_intact(t) and torch.isfinite(t).all() for t in g), "a guard row of an in/out operand was written, or an element is not finite"
    assert tr is None or (torch.isnan(tr[iters:]).all() and torch.isfinite(tr[:iters]).all())
    return tuple(t.reshape(s.shape).cpu() for t, s in zip(g, start)) + (None if tr is None else tr[:iters].cpu(),)


def _seed(case):
    n, c, e, _ = case
    return n * 1000 + c * 10 + e


def _note(family, key, ratios):
    _REPORT.setdefault(family, {})[key] = [round(float(v), 4) for v in ratios]
    _REPORT["worst." + family] = round(max(max(v) for v in _REPORT[family].values()), 4)
    write_report("probe.json", _REPORT)


# ------------------------------------------------------------------------------------------ objective
@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_objective_every_element_against_float64(case):
    n, c, e, kind = case
    inp = R.probe_inputs(n, c, e, kind, _seed(case))
    ops = _operands(inp)
    loss, gw, gb = _objective(inp, ops)
    l64, w64, b64 = R.objective64(inp)
    bl, bw, bb = R.objective_bound(inp)
    print(f"objective {R.case_id(case)}: |err| / bound = loss {abs(float(loss) - l64) / bl:.3f}, grad_w {(np.abs(R.f64(gw) - w64) / bw).max():.3f}, "
          f"grad_b {(np.abs(R.f64(gb) - b64) / bb).max():.3f}")
    ratios = R.check_objective(inp, loss, gw, gb)
    _note("objective", R.case_id(case), ratios)
    loss2, gw2, gb2 = _objective(inp, ops)
    assert torch.equal(loss2, loss) and torch.equal(gw2, gw) and torch.equal(gb2, gb), "two calls differ"


@pytest.mark.parametrize("shape", [(70, 129, 64), (40, 300, 36)], ids=["c129", "c300"])
def test_twin_classes_get_bit_equal_gradients(shape):
    """Classes 7 and c - 1 (different sixteens, class tiles and -- at c = 129 -- contraction tiles) are bit-equal in W, b, the base column and the targets."""
    n, c, e = shape
    inp = R.probe_inputs(n, c, e, "mixed", 11)
    inp["W"][c - 1] = inp["W"][7]
    inp["b"][c - 1] = inp["b"][7]
    inp["base"][:, c - 1] = inp["base"][:, 7]
    inp["soft"][:, c - 1] = inp["soft"][:, 7]
    inp["y"][inp["y"] == c - 1] = 3
    inp["y"][inp["y"] == 7] = 3
    _, gw, gb = _objective(inp)
    assert torch.equal(gw[7], gw[c - 1]) and torch.equal(gb[7], gb[c - 1]) and not torch.equal(gw[7], gw[8])


@pytest.mark.parametrize("how", ["label", "weight"])
def test_an_ignored_nan_row_leaves_every_output_finite_and_unchanged(how):
    n, c, e = 70, 65, 36
    inp = R.probe_inputs(n, c, e, "mixed", 12)
    for i in (0, 33, 69):
        if how == "label":
            inp["y"][i] = c
        else:
            inp["r"][i] = 0.0
    inp["norm"] = float(np.float32(1.0 / R._prep(inp)["r"].sum()))
    ref = _objective(inp)
    for i in (0, 33, 69):
        inp["F"][i] = float("nan")
        inp["base"][i] = float("nan")
        inp["soft"][i] = float("nan")
    out = _objective(inp)      # (asserts that every output is finite)
    assert all(torch.equal(a, b) for a, b in zip(out, ref))


def test_objective_refusals_leave_the_outputs_untouched():
    native, lib = _lib()
    inp = R.probe_inputs(5, 3, 16, "mixed", 9)
    d = _operands(inp)
    loss, gw, gb = torch.full((1,), float("nan"), device="cuda"), torch.full((3, 16), float("nan"), device="cuda"), torch.full((3,), float("nan"), device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def refused(word, n=5, c=3, e=16, scale=100.0, norm=0.2, ff=d["F"], o=gw, ws_bytes=None):
        rc = lib.grip_probe_objective(_p(ff), _p(d["W"]), _p(d["b"]), _p(d["base"]), _p(d["y"]), _p(d["soft"]), _p(d["r"]), scale, norm, n, c, e, _p(loss), _p(o),
                                      _p(gb), _p(ws), ws.numel() if ws_bytes is None else ws_bytes, _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("n = 0", n=0)
    refused("c = 0", c=0)
    refused("c = 1025", c=1025)
    refused("e = 6", e=6)
    refused("e = 1028", e=1028)
    refused("scale = 0", scale=0.0)
    refused("norm = inf", norm=float("inf"))
    refused("nan", norm=float("nan"))
    refused("null pointer", ff=None)
    refused("alias", o=d["F"])
    refused("16-byte aligned", ff=d["F"].reshape(-1)[1:])
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_probe_objective_workspace(5, 3, 16, ctypes.byref(nbytes)))
    refused("workspace too small", ws_bytes=nbytes.value - 1)
    torch.cuda.synchronize()
    assert torch.isnan(loss).all() and torch.isnan(gw).all() and torch.isnan(gb).all() and torch.isfinite(d["F"]).all()


# ------------------------------------------------------------------------------------------ fit
@pytest.mark.parametrize("case", R.FIT_CASES, ids=[R.case_id(c) for c in R.FIT_CASES])
def test_fit_three_is_fit_one_three_times_and_follows_the_float64_recursion(case):
    n, c, e, kind = case
    inp = R.probe_inputs(n, c, e, kind, _seed(case))
    l2, mu = R.FIT_HYPER["l2"], R.FIT_HYPER["mu"]
    lr = R.default_lr(inp["scale"], l2)
    three = _fit(inp, l2, lr, mu, 3)
    state, traces = None, []
    for _ in range(3):
        *state, tr = _fit(inp, l2, lr, mu, 1, start=state)
        traces.append(tr)
    assert all(torch.equal(a, b) for a, b in zip(three[:4], state)) and torch.equal(three[4], torch.cat(traces)), "fit(3) is not fit(1) three times"
    assert all(torch.equal(a, b) for a, b in zip(_fit(inp, l2, lr, mu, 3, want_trace=False)[:4], three[:4])), "loss_trace = NULL changes the fit"
    for iters in (1, R.FIT_TIGHT_ITERS, R.FIT_GROSS_ITERS):
        out = three if iters == 3 else _fit(inp, l2, lr, mu, iters)
        ratios = R.check_fit(inp, l2, lr, mu, iters, *out)
        _note(f"fit{iters}", R.case_id(case), ratios)
        print(f"fit({iters}) {R.case_id(case)}: worst |err| / bound (W, b, mom_w, mom_b, trace) = {[round(v, 3) for v in ratios]}")


def test_fit_one_without_momentum_is_the_objective_and_the_written_update():
    """G = fmaf(l2, W, gw), m = fmaf(0, 0, G) = G, W = fmaf(-lr, m, W) on the objective's own bits: in float64 each fmaf is an exact product and sum, rounded once
    to f32 -- bit-equal unless the float64 sum itself rounds (a double rounding, which moves the result by at most one f32 ulp)."""
    inp = R.probe_inputs(130, 65, 36, "mixed", 13)
    l2, lr = np.float32(0.5), np.float32(R.default_lr(inp["scale"], 0.5))
    loss, gw, gb = _objective(inp)
    W1, b1, mw1, mb1, tr = _fit(inp, float(l2), float(lr), 0.0, 1)
    W0, b0 = inp["W"].double().numpy(), inp["b"].double().numpy()
    G = (float(l2) * W0 + gw.double().numpy()).astype(np.float32)
    assert torch.equal(tr[0], loss) and np.array_equal(mb1.numpy(), gb.numpy())
    for got, want in ((mw1.numpy(), G), (W1.numpy(), (W0 - float(lr) * G.astype(np.float64)).astype(np.float32)),
                      (b1.numpy(), (b0 - float(lr) * gb.double().numpy()).astype(np.float32))):
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()
        assert (got == want).mean() > 0.99


def test_fit_through_the_engine_eager_captured_and_continued():
    import grip_amd  # noqa: F401
    from grip_amd import engine
    inp = R.probe_inputs(257, 102, 64, "mixed", 14)
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}
    l2, mu, iters = 1.0, 0.9, 5
    lr = R.default_lr(inp["scale"], l2)
    norm = engine.probe_norm(dev["y"], dev["soft"], dev["r"], 102)
    assert norm == pytest.approx(inp["norm"], rel=1e-6)
    args = (dev["F"], dev["base"], dev["y"], dev["soft"], dev["r"], inp["scale"], l2, lr, mu)
    W, b, state, trace = engine.probe_fit(*args, iters, dev["W"], dev["b"], want_trace=True, norm=inp["norm"])
    ref = _fit(inp, l2, lr, mu, iters)
    assert torch.equal(W.cpu(), ref[0]) and torch.equal(b.cpu(), ref[1]) and torch.equal(state[0].cpu(), ref[2]) and torch.equal(trace.cpu(), ref[4])
    assert torch.equal(dev["W"].cpu(), inp["W"]), "probe_fit modified its start"
    # continued: 2 + 3 = 5
    W2, b2, st2, tr2 = engine.probe_fit(*args, 2, dev["W"], dev["b"], want_trace=True, norm=inp["norm"])
    W5, b5, st5, tr3 = engine.probe_fit(*args, 3, W2, b2, state=st2, want_trace=True)
    assert torch.equal(W5, W) and torch.equal(b5, b) and torch.equal(st5[0], state[0]) and torch.equal(st5[1], state[1]) and torch.equal(torch.cat([tr2, tr3]), trace)
    # captured in a graph and replayed twice
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Wg, bg, stg, trg = engine.probe_fit(*args, iters, dev["W"], dev["b"], want_trace=True, norm=inp["norm"])
    for _ in range(2):
        Wg.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(Wg, W) and torch.equal(bg, b) and torch.equal(stg[0], state[0]) and torch.equal(trg, trace), "a replay differs from the eager call"
    lo, gw, gb = engine.probe_objective(dev["F"], dev["W"], dev["b"], dev["base"], dev["y"], dev["soft"], dev["r"], inp["scale"], inp["norm"])
    o = _objective(inp)
    assert torch.equal(lo.cpu(), o[0]) and torch.equal(gw.cpu(), o[1]) and torch.equal(gb.cpu(), o[2]) and torch.equal(lo.cpu(), trace[0].cpu())


def test_fit_refusals_leave_the_operands_untouched():
    native, lib = _lib()
    inp = R.probe_inputs(5, 3, 16, "mixed", 9)
    d = _operands(inp)
    w, b = inp["W"].cuda(), inp["b"].cuda()
    mw, mb = torch.zeros(3, 16, device="cuda"), torch.zeros(3, device="cuda")
    tr = torch.full((4,), float("nan"), device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def refused(word, n=5, c=3, e=16, scale=100.0, norm=0.2, l2=1.0, lr=1e-4, mu=0.9, iters=2, ww=w, m=mw, ws_bytes=None):
        rc = lib.grip_probe_fit(_p(d["F"]), _p(d["base"]), _p(d["y"]), _p(d["soft"]), _p(d["r"]), scale, norm, l2, lr, mu, iters, n, c, e, _p(ww), _p(b), _p(m),
                                _p(mb), _p(tr), _p(ws), ws.numel() if ws_bytes is None else ws_bytes, _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("n = -1", n=-1)
    refused("c = 1025", c=1025)
    refused("e = 2", e=2)
    refused("lr = 0", lr=0.0)
    refused("scale = -1", scale=-1.0)
    refused("l2 = -1", l2=-1.0)
    refused("momentum = 1", mu=1.0)
    refused("momentum = -0.5", mu=-0.5)
    refused("iters = 0", iters=0)
    refused("null pointer", ww=None)
    refused("alias", m=w)
    refused("alias", ww=d["F"])
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_probe_fit_workspace(5, 3, 16, ctypes.byref(nbytes)))
    refused("workspace too small", ws_bytes=nbytes.value - 1)
    torch.cuda.synchronize()
    assert torch.equal(w.cpu(), inp["W"]) and torch.equal(b.cpu(), inp["b"]) and (mw == 0).all() and (mb == 0).all() and torch.isnan(tr).all()
