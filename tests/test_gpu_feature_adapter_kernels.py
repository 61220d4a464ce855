"""The feature adapter (csrc/feature_adapter.hip: grip_feature_adapter_forward / _backward) through the C ABI, element by element against float64 on
the same f32 inputs, under the bounds of tests/feature_adapter_ref.py (nothing in them comes from a measurement).  Every element is asserted; the
worst |err| / bound per case and output goes to tests/_out/feature_adapter.json.

Every operand is followed by NaN guard rows and every output is NaN-prefilled with guard rows of its own: the guard rows must stay NaN and every
owned element must be finite.  The backward is given the float64 reference's hidden and act rounded to f32 (exact zeros where ReLU clipped) and the
reference reads those same f32 values, so no mask is ever in doubt.  Shapes: feature_adapter_ref.CASES (relative to the forward's 64-row tile, its
five accumulator counts and the 16 x 16 wave tiles of the backward)."""
import ctypes

import pytest
import torch

import feature_adapter_ref as R
from conftest import write_report

pytestmark = pytest.mark.gpu
GUARD = 8
ZERO_ROW_CASE, ZERO_ROW = (70, 64, 16), 66      # an all-zero feature row in the ragged second tile
_REPORT, _REF = {}, {}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native, native.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _padded(x):
    """x followed by GUARD rows of NaN in one allocation: the view of the owned rows."""
    buf = torch.full((x.shape[0] + GUARD,) + tuple(x.shape[1:]), float("nan"), device="cuda", dtype=torch.float32)
    buf[:x.shape[0]] = x
    return buf[:x.shape[0]]


def _out(rows, cols):
    buf = torch.full((rows + GUARD, cols), float("nan"), device="cuda", dtype=torch.float32)
    return buf, buf[:rows]


def _owned(what, buf, rows):
    assert torch.isfinite(buf[:rows]).all(), f"{what}: an owned element was not written (or is not finite)"
    assert torch.isnan(buf[rows:]).all(), f"{what}: a guard row was written"
    return buf[:rows]


def _forward(f, w1, w2, r, train):
    """(out, hidden_out, act_out) of one forward call; the last two None at inference."""
    native, lib = _lib()
    (n, e), h = f.shape, w1.shape[0]
    obuf, out = _out(n, e)
    hbuf, hid = _out(n, h) if train else (None, None)
    abuf, act = _out(n, e) if train else (None, None)
    fv, av, bv = _padded(f), _padded(w1), _padded(w2)      # (named: a temporary would be freed, and its memory reused, before the call)
    native.check(lib.grip_feature_adapter_forward(_p(fv), _p(av), _p(bv), r, n, e, h, _p(out), _p(hid), _p(act), _stream()))
    torch.cuda.synchronize()
    _owned("out", obuf, n)
    if train:
        _owned("hidden_out", hbuf, n), _owned("act_out", abuf, n)
    return out, hid, act


def _backward(f, w2, hidden, act, G, r, ws_shift=0):
    """(grad_w1, grad_w2); the workspace is NaN-prefilled and starts ws_shift bytes into its allocation."""
    native, lib = _lib()
    (n, e), h = f.shape, w2.shape[1]
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_feature_adapter_workspace(n, e, h, ctypes.byref(nbytes)))
    ws = torch.full(((nbytes.value + ws_shift + 3) // 4,), float("nan"), device="cuda", dtype=torch.float32)
    b1, g1 = _out(h, e)
    b2, g2 = _out(e, h)
    fv, bv, hv, av, gv = _padded(f), _padded(w2), _padded(hidden), _padded(act), _padded(G)
    native.check(lib.grip_feature_adapter_backward(_p(fv), _p(bv), _p(hv), _p(av), _p(gv), r, n, e, h, _p(g1), _p(g2),
                                                   ctypes.c_void_p(ws.data_ptr() + ws_shift), nbytes.value, _stream()))
    torch.cuda.synchronize()
    return _owned("grad_w1", b1, h), _owned("grad_w2", b2, e)


def _case(n, e, h, r):
    """Inputs on the GPU and the float64 reference of a case, computed once and shared by the tests (never modified)."""
    key = (n, e, h, r)
    if key not in _REF:
        f, w1, w2, G = (t.cuda() for t in R.inputs(n, e, h, n * 1000 + e, zero_row=ZERO_ROW if (n, e, h) == ZERO_ROW_CASE else None))
        fwd = R.forward(f, w1, w2, r)
        hid32, act32 = fwd["H"].float(), fwd["x"].float()
        _REF[key] = dict(f=f, w1=w1, w2=w2, G=G, fwd=fwd, hid32=hid32, act32=act32, bwd=R.backward(f, w2, hid32, act32, G, r))
    return _REF[key]


def _check(case, what, got, ref, bound):
    ratio = R.worst_ratio(got, ref, bound)
    _REPORT.setdefault(case, {})[what] = round(ratio, 4)
    write_report("feature_adapter.json", _REPORT)
    print(f"{case} {what}: worst |err| / bound = {ratio:.3f}")
    assert torch.isfinite(got).all() and ((got.double() - ref).abs() <= bound).all(), f"{case} {what}: |err| is {ratio:.2f} x its bound"


RUNS = [(n, e, h, 0.2) for n, e, h in R.CASES] + [(130, 256, 64, 0.7)]


@pytest.mark.parametrize("n,e,h,r", RUNS, ids=[f"n{n}-e{e}-h{h}-r{r:g}" for n, e, h, r in RUNS])
def test_forward_and_backward_against_float64(n, e, h, r):
    c = _case(n, e, h, r)
    case, fwd, bwd = f"n{n}.e{e}.h{h}.r{r:g}", c["fwd"], c["bwd"]
    out, hid, act = _forward(c["f"], c["w1"], c["w2"], r, True)
    _check(case, "out", out, fwd["out"], fwd["b_out"])
    _check(case, "hidden_out", hid, fwd["H"], fwd["du"])
    _check(case, "act_out", act, fwd["x"], fwd["dz"])
    inf, none_h, none_a = _forward(c["f"], c["w1"], c["w2"], r, False)
    assert none_h is None and none_a is None and torch.equal(inf, out), "the inference call's out differs from the training call's"
    g1, g2 = _backward(c["f"], c["w2"], c["hid32"], c["act32"], c["G"], r)
    _check(case, "grad_w2", g2, bwd["grad_w2"], bwd["b_w2"])
    _check(case, "grad_w1", g1, bwd["grad_w1"], bwd["b_w1"])
    assert (g1 != 0).any() and (g2 != 0).any()


def test_zero_feature_row_is_exact():
    n, e, h = ZERO_ROW_CASE
    c = _case(n, e, h, 0.2)
    assert (c["f"][ZERO_ROW] == 0).all()
    out, hid, act = _forward(c["f"], c["w1"], c["w2"], 0.2, True)
    assert (out[ZERO_ROW] == 0).all() and (hid[ZERO_ROW] == 0).all() and (act[ZERO_ROW] == 0).all()
    assert (out[ZERO_ROW - 1] != 0).any() and (out[ZERO_ROW + 1] != 0).any()
    # its contribution to both gradients is exactly 0: whatever its row of grad_out and of act holds, no bit of either gradient moves ...
    g1, g2 = _backward(c["f"], c["w2"], c["hid32"], c["act32"], c["G"], 0.2)
    G2, act2 = c["G"].clone(), c["act32"].clone()
    G2[ZERO_ROW] = 1e6 * (1 + torch.rand(e, device="cuda"))
    act2[ZERO_ROW] = 1.0
    h1, h2 = _backward(c["f"], c["w2"], c["hid32"], act2, G2, 0.2)
    assert torch.equal(h1, g1) and torch.equal(h2, g2)
    # ... and the gradients are those of the batch without the row (a zero product leaves an fmaf chain's value as it is)
    keep = [i for i in range(n) if i != ZERO_ROW]
    k1, k2 = _backward(c["f"][keep], c["w2"], c["hid32"][keep], c["act32"][keep], c["G"][keep], 0.2)
    assert torch.equal(k1, g1) and torch.equal(k2, g2)


@pytest.mark.parametrize("n,e,h", [(70, 64, 16), (130, 256, 64)])
def test_forward_exact_statements(n, e, h):
    c = _case(n, e, h, 0.2)
    f, w1, w2 = c["f"], c["w1"], c["w2"]
    full = _forward(f, w1, w2, 0.2, False)[0]
    assert torch.equal(_forward(f, w1, w2, 0.0, False)[0], f), "ratio = 0 does not return img_emb"
    one, _, act = _forward(f, w1, w2, 1.0, True)
    assert torch.equal(one, act), "ratio = 1 does not return x"
    assert torch.equal(act, _forward(f, w1, w2, 0.2, True)[2]) and (act > 0).any() and (act == 0).any()
    assert torch.equal(_forward(f, w1, w2, 0.2, False)[0], full), "two runs differ"
    # a row's bits depend on the row and the weights only: not on n, on the row's place in a tile or on the call
    assert torch.equal(_forward(f[:16], w1, w2, 0.2, False)[0], full[:16]), "rows 0 .. 15 alone differ"
    assert torch.equal(_forward(f[64:], w1, w2, 0.2, False)[0], full[64:]), "rows 64 .. end alone differ (they sat in the second tile)"
    for i in (0, 37, n - 1):
        assert torch.equal(_forward(f[i:i + 1], w1, w2, 0.2, False)[0], full[i:i + 1]), f"row {i} alone differs"


@pytest.mark.parametrize("n,e,h", [(70, 64, 16), (67, 768, 192)])
def test_backward_is_reproducible_and_owns_its_workspace(n, e, h):
    c = _case(n, e, h, 0.2)
    args = (c["f"], c["w2"], c["hid32"], c["act32"], c["G"], 0.2)
    g1, g2 = _backward(*args)
    a1, a2 = _backward(*args)
    assert torch.equal(a1, g1) and torch.equal(a2, g2), "two runs differ"
    s1, s2 = _backward(*args, ws_shift=4096 + 16)      # another address (not 256-byte aligned), NaN-prefilled like the first
    assert torch.equal(s1, g1) and torch.equal(s2, g2), "the gradients depend on the workspace"


def test_refusals():
    """Bad arguments return an error and a message before any launch (the output buffers keep their NaNs)."""
    native, lib = _lib()
    n, e, h = 4, 64, 16
    f, w1, w2, G = (t.cuda() for t in R.inputs(n, e, h, 1))
    out, hid, act = (torch.full(s, float("nan"), device="cuda") for s in ((n, e), (n, h), (n, e)))
    g1, g2 = torch.full((h, e), float("nan"), device="cuda"), torch.full((e, h), float("nan"), device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def refused(rc, word):
        assert rc != 0
        msg = lib.grip_last_error().decode()
        assert word in msg, msg

    fwd = lambda *a: lib.grip_feature_adapter_forward(*a, _stream())      # noqa: E731
    refused(fwd(_p(f), _p(w1), _p(w2), 0.2, n, 96, h, _p(out), None, None), "e = 96")
    refused(fwd(_p(f), _p(w1), _p(w2), 0.2, n, e, 24, _p(out), None, None), "h = 24")
    refused(fwd(_p(f), _p(w1), _p(w2), 0.2, n, 1024, 272, _p(out), None, None), "h = 272")
    refused(fwd(_p(f), _p(w1), _p(w2), 0.2, 0, e, h, _p(out), None, None), "n = 0")
    refused(fwd(_p(f), _p(w1), None, 0.2, n, e, h, _p(out), None, None), "null pointer")
    refused(fwd(_p(f), _p(w1), _p(w2), 0.2, n, e, h, _p(out), _p(hid), None), "given together")
    refused(fwd(_p(f), _p(w1), _p(w2), 0.2, n, e, h, _p(f), None, None), "alias")
    refused(fwd(ctypes.c_void_p(f.data_ptr() + 4), _p(w1), _p(w2), 0.2, n - 1, e, h, _p(out), None, None), "16-byte aligned")
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_feature_adapter_workspace(n, e, h, ctypes.byref(nbytes)))
    bwd = lambda *a: lib.grip_feature_adapter_backward(*a, _stream())      # noqa: E731
    hid32, act32 = torch.rand(n, h, device="cuda"), torch.rand(n, e, device="cuda")
    refused(bwd(_p(f), _p(w2), _p(hid32), _p(act32), _p(G), 0.2, n, e, h, _p(g1), _p(g2), _p(ws), nbytes.value - 1), "workspace too small")
    refused(bwd(_p(f), _p(w2), _p(hid32), _p(act32), _p(G), 0.2, n, e, h, _p(g1), None, _p(ws), ws.numel()), "null pointer")
    refused(bwd(_p(f), _p(w2), _p(hid32), _p(act32), _p(G), 0.2, n, 96, h, _p(g1), _p(g2), _p(ws), ws.numel()), "e = 96")
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in (out, hid, act, g1, g2))
