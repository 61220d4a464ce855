"""grip_class_scatter / grip_spd_solve / grip_linear_head (csrc/gda_head.hip) through the C ABI: every output element against float64 on the same inputs
with the bounds that tests/gda_ref.py derives (nothing in them comes from a measurement), two calls bit-equal, S bit-symmetric, the Cholesky
backward-error inequalities with the kernel's own factor, the first arg-max, a row's bits alone and inside a batch, the refusals with nothing written.
NaN guard rows sit behind every operand and output and the workspace starts as 0xFF bytes (NaNs): a read of anything the call did not write itself
would show.  The worst |err| / bound per case goes to tests/_out/gda.json."""
import ctypes

import pytest
import torch

import gda_ref as R
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


def _ws(query, *dims):
    native, _ = _lib()
    nbytes = ctypes.c_size_t()
    native.check(query(*dims, ctypes.byref(nbytes)))
    return torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device="cuda")


def _scatter(F, y, r, mean):
    native, lib = _lib()
    (n, e), c = F.shape, mean.shape[0]
    out = torch.full((e + GUARD, e), float("nan"), device="cuda")
    ws = _ws(lib.grip_class_scatter_workspace, n, c, e)
    assert ws.numel() <= R.SCATTER_SLICES * e * e * 4 + 256, "the workspace must not grow with n"
    Fg, yg, rg, mg = _guarded(F), _guarded(y, 1 << 30), _guarded(r), _guarded(mean)      # (held: a freed block would be handed to the next operand)
    native.check(lib.grip_class_scatter(_p(Fg), _p(yg), _p(rg), _p(mg), n, c, e, _p(out), _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(out[e:]).all(), "a guard row of the output was written"
    assert torch.isfinite(out[:e]).all(), "an owned output element was not written"
    return out[:e]


def _solve(a, a_scale, ridge_rel, rhs, want_factor=True, x_fill=float("nan")):
    native, lib = _lib()
    e, c = a.shape[0], rhs.shape[0]
    x = torch.full((c + GUARD, e), x_fill, device="cuda")
    L = torch.full((e + GUARD, e), float("nan"), device="cuda") if want_factor else None
    info = torch.full((1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    ws = _ws(lib.grip_spd_solve_workspace, e, c)
    ag, bg = _guarded(a), _guarded(rhs)
    native.check(lib.grip_spd_solve(_p(ag), a_scale, ridge_rel, _p(bg), e, c, _p(x), _p(L), _p(info), _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(x[c:]).all() and (info[1:] == -7).all() and (L is None or torch.isnan(L[e:]).all()), "a guard row of the outputs was written"
    return x[:c], (None if L is None else L[:e]), int(info[0])


def _head(f, w, bias, alpha, base, mode, want_argmax=True):
    """mode: nobase (base NULL), base (base read, another buffer written), inplace (logits_out IS base_logits)."""
    native, lib = _lib()
    (n, e), c = f.shape, w.shape[0]
    out = torch.full((n + GUARD, c), float("nan"), device="cuda")
    bg = None
    if mode == "base":
        bg = _guarded(base)
    elif mode == "inplace":
        out[:n] = base
        bg = out
    am = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    ws = _ws(lib.grip_linear_head_workspace, n, c, e)
    fg, wg, sg = _guarded(f), _guarded(w), _guarded(bias)
    native.check(lib.grip_linear_head(_p(fg), _p(wg), _p(sg), alpha, _p(bg), n, c, e, _p(out), _p(am) if want_argmax else None, _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(out[n:]).all() and (am[n:] == -1).all(), "a guard row of the outputs was written"
    assert (am[:n] >= 0).all() if want_argmax else (am == -1).all()
    return out[:n], am[:n]


# ------------------------------------------------------------------------------------------ scatter
@pytest.mark.parametrize("case", R.S_CASES, ids=[R.case_id(c) for c in R.S_CASES])
def test_scatter_every_element_against_float64(case):
    n, c, e, kind = case
    F, y, r, mean = R.scatter_inputs(n, c, e, kind, seed=n * 1000 + c * 10 + e)
    if n >= 5:      # a label outside 0 .. c - 1 contributes nothing (R.centred drops it too); its feature row is a NaN row: it must not be read
        y = y.clone()
        y[3] = c + 5
        y[1] = -1
        F = F.clone()
        F[3] = float("nan")
    ops = tuple(None if t is None else t.cuda() for t in (F, y, r, mean))
    S = _scatter(*ops)
    ratio = R.check_scatter(F, y, r, mean, S)
    _REPORT["scatter." + R.case_id(case)] = round(ratio, 4)
    write_report("gda.json", _REPORT)
    print(f"scatter {R.case_id(case)}: worst |err| / bound = {ratio:.3f}")
    assert torch.equal(S, S.T), "S is not bit-symmetric"
    if kind == "samerows":
        assert (S == 0).all(), "identical rows around their own mean must give S = 0 exactly"
    assert torch.equal(_scatter(*ops), S), "two calls differ"


def test_scatter_refusals():
    native, lib = _lib()
    F, y, r, mean = (t.cuda() for t in R.scatter_inputs(5, 3, 16, "weighted", seed=9))
    out = torch.full((16, 16), float("nan"), device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def refused(word, n=5, c=3, e=16, ff=F, o=out, ws_bytes=None):
        rc = lib.grip_class_scatter(_p(ff), _p(y), _p(r), _p(mean), n, c, e, _p(o), _p(ws), ws.numel() if ws_bytes is None else ws_bytes, _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("n = 0", n=0)
    refused("c = 0", c=0)
    refused("e = 6", e=6)
    refused("e = 1028", e=1028)
    refused("null pointer", ff=None)
    refused("alias", o=F)
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_class_scatter_workspace(5, 3, 16, ctypes.byref(nbytes)))
    refused("workspace too small", ws_bytes=nbytes.value - 1)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isfinite(F).all()


# ------------------------------------------------------------------------------------------ SPD solve
@pytest.mark.parametrize("case", R.V_CASES, ids=[R.case_id(c) for c in R.V_CASES])
def test_solve_backward_error_inequalities(case):
    e, c, ridge, kind = case
    a, a_scale, rhs = R.solve_inputs(e, c, kind, seed=e * 10 + c)
    ad, bd = a.cuda(), rhs.cuda()
    x, L, info = _solve(ad, a_scale, ridge, bd)
    assert info == 0
    assert torch.isfinite(x).all() and torch.isfinite(L).all(), "an owned output element was not written"
    ratios = R.check_solve(a, a_scale, ridge, rhs, x, L)
    _REPORT["solve." + R.case_id(case)] = [round(v, 4) for v in ratios]
    write_report("gda.json", _REPORT)
    print(f"solve {R.case_id(case)}: worst |err| / bound = factor {ratios[0]:.3f}, residual {ratios[1]:.3f}, solution {ratios[2]:.3f}")
    x2, L2, _ = _solve(ad, a_scale, ridge, bd)
    assert torch.equal(x2, x) and torch.equal(L2, L), "two calls differ"
    x3, none, info3 = _solve(ad, a_scale, ridge, bd, want_factor=False)
    assert none is None and info3 == 0 and torch.equal(x3, x), "factor_out = NULL changes the solution"
    poisoned = ad.clone()
    poisoned[torch.triu(torch.ones(e, e, dtype=torch.bool, device="cuda"), 1)] = float("nan")
    x4, L4, info4 = _solve(poisoned, a_scale, ridge, bd)
    assert info4 == 0 and torch.equal(x4, x) and torch.equal(L4, L), "the upper triangle of a was read"


@pytest.mark.parametrize("e", [4, 132])
def test_solve_reports_the_first_bad_pivot_and_returns(e):
    rhs = torch.ones(3, e, device="cuda")
    _, _, info = _solve(torch.zeros(e, e, device="cuda"), 1.0, 0.0, rhs)
    assert info == 1
    a = torch.eye(e, device="cuda")
    a[e - 2, e - 2] = -1.0
    _, _, info = _solve(a, 1.0, 0.0, rhs)
    assert info == e - 1, "info must be j + 1 of the FIRST pivot j that is not > 0"


def test_solve_through_the_engine_raises_and_names_the_pivot():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    with pytest.raises(native.GripError, match="pivot 0 of 8"):
        engine.spd_solve(torch.zeros(8, 8, device="cuda"), torch.ones(2, 8, device="cuda"))
    a = torch.eye(8, device="cuda") * 4
    x, L = engine.spd_solve(a, torch.ones(2, 8, device="cuda"), a_scale=0.5, ridge_rel=1.0, want_factor=True)       # M = 2 I + 2 I
    assert torch.equal(x, torch.full((2, 8), 0.25, device="cuda")) and torch.equal(L, torch.eye(8, device="cuda") * 2)


def test_solve_refusals():
    native, lib = _lib()
    a, a_scale, rhs = R.solve_inputs(16, 3, "scatter", seed=4)
    a, rhs = a.cuda(), rhs.cuda()
    x = torch.full((3, 16), float("nan"), device="cuda")
    info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def refused(word, e=16, c=3, s=a_scale, ridge=1.0, aa=a, xx=x, ws_bytes=None):
        rc = lib.grip_spd_solve(_p(aa), s, ridge, _p(rhs), e, c, _p(xx), None, _p(info), _p(ws), ws.numel() if ws_bytes is None else ws_bytes, _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("c = 0", c=0)
    refused("e = 6", e=6)
    refused("e = 2048", e=2048)
    refused("a_scale = 0", s=0.0)
    refused("ridge_rel = -1", ridge=-1.0)
    refused("null pointer", aa=None)
    refused("alias", xx=a)
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_spd_solve_workspace(16, 3, ctypes.byref(nbytes)))
    refused("workspace too small", ws_bytes=nbytes.value - 1)
    torch.cuda.synchronize()
    assert torch.isnan(x).all() and int(info[0]) == -7 and torch.isfinite(a).all()


# ------------------------------------------------------------------------------------------ linear head
@pytest.mark.parametrize("case", R.H_CASES, ids=[R.case_id(c) for c in R.H_CASES])
def test_head_every_element_against_float64(case):
    n, c, e, mode = case
    f, w, bias, base, alpha = R.head_inputs(n, c, e, seed=n * 1000 + c * 10 + e)
    ops = tuple(t.cuda() for t in (f, w, bias))
    out, am = _head(*ops, alpha, base.cuda(), mode)
    assert torch.isfinite(out).all(), "an owned output element was not written (or is not finite)"
    ratio = R.check_head(f, w, bias, alpha, None if mode == "nobase" else base, out)
    _REPORT["head." + R.case_id(case)] = round(ratio, 4)
    write_report("gda.json", _REPORT)
    print(f"head {R.case_id(case)}: worst |err| / bound = {ratio:.3f}")
    assert torch.equal(am.long(), out.argmax(1)) or all(out[i, am[i]] == out[i].max() and (out[i, :am[i]] < out[i].max()).all() for i in range(n))
    out2, am2 = _head(*ops, alpha, base.cuda(), mode)
    assert torch.equal(out2, out) and torch.equal(am2, am), "two calls differ"
    out3, _ = _head(*ops, alpha, base.cuda(), mode, want_argmax=False)
    assert torch.equal(out3, out), "argmax_out = NULL changes the logits"


def test_head_first_argmax_with_twin_classes_and_the_zero_row():
    """Classes 7 and c - 1 (two different class tiles) are bit-equal in w, bias and base: their logits are bit-equal in every row and, where they carry
    the row's maximum, the arg-max is the lower index.  A zero row follows grip_cache_head_forward's rule: 1 / sqrt(0) = inf scales a zero score, the
    whole row is NaN and its arg-max is 0; the rows around it do not see it."""
    n, c, e = 70, 129, 64
    f, w, bias, base, alpha = R.head_inputs(n, c, e, seed=5)
    w[7] = w[c - 1] = f[:n // 2].mean(0) * 3
    bias[7] = bias[c - 1] = -50.0
    base[:, 7] = base[:, c - 1]
    ref, _ = _head(f.cuda(), w.cuda(), bias.cuda(), alpha, base.cuda(), "base")
    f[41] = 0
    out, am = _head(f.cuda(), w.cuda(), bias.cuda(), alpha, base.cuda(), "base")
    assert torch.equal(out[:, 7], out[:, c - 1]) or (torch.equal(out[:41, 7], out[:41, c - 1]) and torch.equal(out[42:, 7], out[42:, c - 1]))
    assert torch.isnan(out[41]).all() and int(am[41]) == 0
    keep = torch.arange(n, device="cuda") != 41
    assert torch.equal(out[keep], ref[keep])
    assert (am[keep] == 7).sum() > n // 4 and not (am == c - 1).any()


def test_head_row_bits_alone_and_inside_a_batch():
    n, c, e = 200, 102, 512
    f, w, bias, base, alpha = (t.cuda() if torch.is_tensor(t) else t for t in R.head_inputs(n, c, e, seed=6))
    out, am = _head(f, w, bias, alpha, base, "base")
    for i in (0, 63, 64, 199):
        oi, ai = _head(f[i:i + 1].clone(), w, bias, alpha, base[i:i + 1].clone(), "base")
        assert torch.equal(oi[0], out[i]) and int(ai[0]) == int(am[i]), f"row {i} differs alone"
    shifted, _ = _head(f[37:150].clone(), w, bias, alpha, base[37:150].clone(), "inplace")
    assert torch.equal(shifted, out[37:150]), "a row's bits depend on its place in a tile"


def test_head_refusals():
    native, lib = _lib()
    f, w, bias, base, alpha = (t.cuda() if torch.is_tensor(t) else t for t in R.head_inputs(5, 3, 16, seed=7))
    out = torch.full((5, 3), float("nan"), device="cuda")
    am = torch.full((5,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 12, dtype=torch.uint8, device="cuda")

    def refused(word, n=5, c=3, e=16, al=alpha, ff=f, o=out, ws_bytes=None):
        rc = lib.grip_linear_head(_p(ff), _p(w), _p(bias), al, _p(base), n, c, e, _p(o), _p(am), _p(ws), ws.numel() if ws_bytes is None else ws_bytes, _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("n = 0", n=0)
    refused("c = 0", c=0)
    refused("e = 6", e=6)
    refused("e = 2048", e=2048)
    refused("finite", al=float("inf"))
    refused("null pointer", ff=None)
    refused("alias", o=f)
    refused("workspace too small", ws_bytes=0)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and (am == -1).all() and torch.isfinite(f).all()
