"""grip_gmm_mstep / grip_gmm_estep (csrc/gmm_transduce.hip) through the C ABI: every output element against float64 on the same inputs with the bounds
that tests/gmm_ref.py derives (nothing in them comes from a measurement), two calls bit-equal, the first-maximum arg-max, bit-equal classes staying
bit-equal, the refusals with nothing written.  NaN guard rows sit behind every operand and output and the workspace starts as 0xFF bytes (NaNs): a read
of anything the call did not write itself would show.  The worst |err| / bound per case goes to tests/_out/gmm.json."""
import ctypes

import pytest
import torch

import gmm_ref as R
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
    x = x.reshape(-1, 1) if x.dim() == 1 else x
    buf = torch.full((x.shape[0] + GUARD,) + tuple(x.shape[1:]), fill, device="cuda", dtype=x.dtype)
    buf[:x.shape[0]] = x
    return buf[:x.shape[0]]


def _mstep(z, f, var_floor=1e-8):
    native, lib = _lib()
    (n, c), e = z.shape, f.shape[1]
    zg, fg = _guarded(z), _guarded(f)
    cnt = torch.full((c + GUARD,), float("nan"), device="cuda")
    mean = torch.full((c + GUARD, e), float("nan"), device="cuda")
    var = torch.full((e + GUARD,), float("nan"), device="cuda")
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_gmm_mstep_workspace(n, c, e, ctypes.byref(nbytes)))
    ws = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device="cuda")
    native.check(lib.grip_gmm_mstep(_p(zg), _p(fg), n, c, e, var_floor, _p(cnt), _p(mean), _p(var), _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(cnt[c:]).all() and torch.isnan(mean[c:]).all() and torch.isnan(var[e:]).all(), "a guard row of the outputs was written"
    assert torch.isfinite(cnt[:c]).all() and torch.isfinite(mean[:c]).all() and torch.isfinite(var[:e]).all(), "an owned output element was not written"
    return cnt[:c], mean[:c], var[:e]


def _estep(f, mean, var, probs, idx, sim, z_in, lam, z_iters, want_argmax=True):
    native, lib = _lib()
    (n, e), c, k = f.shape, mean.shape[0], idx.shape[1]
    fg, mg, vg, pg, sg, zg = (_guarded(t) for t in (f, mean, var, probs, sim, z_in))
    ig = _guarded(idx, 1 << 30)
    obuf = torch.full((n + GUARD, c), float("nan"), device="cuda")
    abuf = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_gmm_estep_workspace(n, c, e, k, ctypes.byref(nbytes)))
    ws = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device="cuda")
    native.check(lib.grip_gmm_estep(_p(fg), _p(mg), _p(vg), _p(pg), _p(ig), _p(sg), _p(zg), lam, z_iters, n, c, e, k, _p(obuf), _p(abuf) if want_argmax else None,
                                    _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(obuf[n:]).all() and (abuf[n:] == -1).all(), "a guard row of the outputs was written"
    assert torch.isfinite(obuf[:n]).all(), "an owned output element was not written (or is not finite)"
    assert (abuf[:n] >= 0).all() if want_argmax else (abuf == -1).all()
    return obuf[:n], abuf[:n]


# ------------------------------------------------------------------------------------------ M-step
@pytest.mark.parametrize("case", R.M_CASES, ids=[R.case_id(c) for c in R.M_CASES])
def test_mstep_every_element_against_float64(case):
    n, c, e, kind = case
    z, f = (t.cuda() for t in R.mstep_inputs(n, c, e, kind, seed=n * 1000 + c * 10 + e))
    cnt, mean, var = _mstep(z, f)
    ratio = R.check_mstep(z, f, 1e-8, cnt, mean, var)
    _REPORT["mstep." + R.case_id(case)] = round(ratio, 4)
    write_report("gmm.json", _REPORT)
    print(f"M-step {R.case_id(case)}: worst |err| / bound = {ratio:.3f}")
    if kind == "zerocol":
        assert cnt[c // 2] == 0 and (mean[c // 2] == 0).all(), "a class of exactly zero weight must give N_c = 0 and a zero centre"
    if kind == "samerows":
        assert (var == torch.tensor(1e-8, device="cuda")).all(), "identical rows must give var_floor exactly"
    again = _mstep(z, f)
    assert all(torch.equal(a, b) for a, b in zip(again, (cnt, mean, var))), "two calls differ"


def test_mstep_refusals():
    native, lib = _lib()
    z, f = (t.cuda() for t in R.mstep_inputs(5, 64, 16, "plain", seed=9))
    cnt, mean, var = (torch.full(s, float("nan"), device="cuda") for s in ((64,), (64, 16), (16,)))
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def refused(word, n=5, c=64, e=16, var_floor=1e-8, zz=z, m=mean, ws_bytes=None):
        rc = lib.grip_gmm_mstep(_p(zz), _p(f), n, c, e, var_floor, _p(cnt), _p(m), _p(var), _p(ws), ws.numel() if ws_bytes is None else ws_bytes, _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("var_floor = 0", var_floor=0.0)
    refused("var_floor = -1", var_floor=-1.0)
    refused("n = 0", n=0)
    refused("c = 0", c=0)
    refused("e = 6", e=6)
    refused("null pointer", zz=None)
    refused("alias", m=f)
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_gmm_mstep_workspace(5, 64, 16, ctypes.byref(nbytes)))
    refused("workspace too small", ws_bytes=nbytes.value - 1)
    torch.cuda.synchronize()
    assert torch.isnan(cnt).all() and torch.isnan(mean).all() and torch.isnan(var).all() and torch.isfinite(f).all()


# ------------------------------------------------------------------------------------------ E-step
@pytest.mark.parametrize("case", R.E_CASES, ids=[R.case_id(c) for c in R.E_CASES])
def test_estep_every_element_against_float64(case):
    n, c, e, k, zi, lam, kind = case
    ops = tuple(t.cuda() for t in R.estep_inputs(n, c, e, k, kind, seed=n * 1000 + c * 10 + k))
    out, am = _estep(*ops, lam, zi)
    ratio = R.check_estep(*ops, lam, zi, out, am)
    _REPORT["estep." + R.case_id(case)] = round(ratio, 4)
    write_report("gmm.json", _REPORT)
    print(f"E-step {R.case_id(case)}: worst |err| / bound = {ratio:.3f}")
    again, am2 = _estep(*ops, lam, zi)
    assert torch.equal(again, out) and torch.equal(am2, am), "two calls differ"


@pytest.mark.parametrize("c", [65, 300])        # classes in registers / waiting in the output row
def test_argmax_is_optional_and_takes_the_first_maximum(c):
    """Classes 7 and c - 1 (two different lane passes) are bit-equal in the centres, in P and in the neighbours' Z: their Z columns stay bit-equal
    through every sweep and, where they carry the row's maximum, the arg-max is the lower index."""
    n, e, k = 37, 64, 3
    f, mean, var, probs, idx, sim, z_in = R.estep_inputs(n, c, e, k, "plain", seed=12)
    var = var * 10                                       # (soft assignments: ties are visible, not 0 == 0)
    mean[7] = mean[c - 1] = f[:n // 2].mean(0)           # the twin classes win the rows near this centre
    probs[:] = 1.0 / c
    z_in[:, c - 1] = z_in[:, 7]
    ops = tuple(t.cuda() for t in (f, mean, var, probs, idx, sim, z_in))
    out, am = _estep(*ops, 1.0, 5)
    assert torch.equal(out[:, 7], out[:, c - 1]) and (out[:, 7] > 0).all()
    twins_win = out[:, 7] == out.max(dim=1).values
    assert twins_win.any() and (am[twins_win] == 7).all()
    R.check_estep(*ops, 1.0, 5, out, am)
    out2, _ = _estep(*ops, 1.0, 5, want_argmax=False)
    assert torch.equal(out2, out)


def test_estep_refusals():
    native, lib = _lib()
    f, mean, var, probs, idx, sim, z_in = (t.cuda() for t in R.estep_inputs(5, 64, 16, 3, "plain", seed=9))
    out = torch.full((5, 64), float("nan"), device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def refused(word, lam=1.0, z_iters=5, n=5, c=64, e=16, k=3, p=probs, o=out, ws_bytes=None):
        rc = lib.grip_gmm_estep(_p(f), _p(mean), _p(var), _p(p), _p(idx), _p(sim), _p(z_in), lam, z_iters, n, c, e, k, _p(o), None, _p(ws),
                                ws.numel() if ws_bytes is None else ws_bytes, _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("lam = -1", lam=-1.0)
    refused("z_iters = 0", z_iters=0)
    refused("k = 0", k=0)
    refused("k = 33", k=33)
    refused("n = 0", n=0)
    refused("c = 0", c=0)
    refused("e = 6", e=6)
    refused("null pointer", p=None)
    refused("alias", o=z_in)
    refused("alias", o=probs)
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_gmm_estep_workspace(5, 64, 16, 3, ctypes.byref(nbytes)))
    refused("workspace too small", ws_bytes=nbytes.value - 1)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isfinite(z_in).all() and torch.isfinite(probs).all()
