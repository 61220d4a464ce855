"""grip_view_mode (csrc/view_mode.hip) through the C ABI: every element of mode, y and h2 against float64 on the same inputs under the bound that
tests/view_mode_ref.py derives (nothing in it comes from a measurement).  The tight checks are the forced single steps (outer = 1, inner = 1 from every
state of the float64 trajectory under the defaults) and outer = 0; a free run at the defaults is held to the carried bound, whose vacuous share is
reported, and GENTLE keeps that bound non-vacuous for the whole run.  Two calls bit-equal; an image alone bit-equal to itself at other places of a
17-image launch; the refusals with nothing written.  NaN guard rows sit behind every operand and output.  The worst |err| / bound per group goes to
tests/_out/view_mode.json."""
import ctypes

import pytest
import torch

import view_mode_ref as R
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
    if x is None:
        return None
    buf = torch.full((x.shape[0] + GUARD,) + tuple(x.shape[1:]), float("nan"), device="cuda", dtype=x.dtype)
    buf[:x.shape[0]] = x
    return buf[:x.shape[0]]


def _mode(f, s, params, mode_in=None, y_in=None, want_h2=True):
    native, lib = _lib()
    n, v, e = f.shape
    c = 1 if s is None else s.shape[2]
    fg, sg, mg, yg = _guarded(f), _guarded(s), _guarded(mode_in), _guarded(y_in)
    mode = torch.full((n + GUARD, e), float("nan"), device="cuda")
    y = torch.full((n + GUARD, v), float("nan"), device="cuda")
    h2 = torch.full((n + GUARD, v), float("nan"), device="cuda")
    nbytes = ctypes.c_size_t(7)
    native.check(lib.grip_view_mode_workspace(n, v, c, e, ctypes.byref(nbytes)))
    ws = torch.full((max(nbytes.value, 1),), 0xFF, dtype=torch.uint8, device="cuda")
    native.check(lib.grip_view_mode(_p(fg), _p(sg), n, v, c, e, params["rho"], params["lam"], params["lam_y"], params["h2_floor"], params["outer"],
                                    params["inner"], _p(mg), _p(yg), _p(mode), _p(y), _p(h2) if want_h2 else None, _p(ws), nbytes.value, _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(mode[n:]).all() and torch.isnan(y[n:]).all() and torch.isnan(h2[n:]).all(), "a guard row was written"
    assert torch.isfinite(mode[:n]).all() and torch.isfinite(y[:n]).all(), "an owned output element was not written (or is not finite)"
    assert torch.isfinite(h2[:n]).all() if want_h2 else torch.isnan(h2).all()
    return mode[:n], y[:n], h2[:n] if want_h2 else None


def _note(group, key, ratio):
    _REPORT.setdefault(group, {})[key] = round(ratio, 4)
    worst = _REPORT.setdefault("worst", {})
    worst[group] = max(worst.get(group, 0.0), round(ratio, 4))
    write_report("view_mode.json", _REPORT)


@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_forced_single_steps_against_float64(case):
    f, s = (t.cuda() if t is not None else None for t in R.case_inputs(case))
    start = dict(R.DEFAULTS, outer=0)
    got = _mode(f, s, start)
    worst, vac = R.check_run(f, s, start, None, None, *got)
    assert vac == 0.0
    assert torch.equal(got[1], torch.full_like(got[1], 1.0) / f.shape[1]), "outer = 0 must hand the start weights back"
    states = R.run64(f, s, trajectory=True, **R.DEFAULTS)[-1]
    one = dict(R.DEFAULTS, outer=1, inner=1)
    for t, (m0, y0) in enumerate(states):
        got = _mode(f, s, one, m0, y0)
        ratio, vac = R.check_run(f, s, one, m0, y0, *got)
        print(f"view_mode {R.case_id(case)} forced step {t}: worst |err| / bound = {ratio:.3f}, vacuous share {vac:.3f}")
        worst = max(worst, ratio)
    _note("forced_steps", R.case_id(case), worst)
    again = _mode(f, s, one, *states[-1])
    assert all(torch.equal(a, b) for a, b in zip(again, got)), "two calls differ"
    m_only, y_only, none = _mode(f, s, one, *states[-1], want_h2=False)       # h2_out is optional
    assert none is None and torch.equal(m_only, got[0]) and torch.equal(y_only, got[1])


@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_free_runs_against_float64(case):
    f, s = (t.cuda() if t is not None else None for t in R.case_inputs(case))
    for group, params in (("free_defaults", R.DEFAULTS), ("free_gentle", R.GENTLE)):
        got = _mode(f, s, params)
        ratio, vac = R.check_run(f, s, params, None, None, *got)
        print(f"view_mode {R.case_id(case)} {group}: worst |err| / bound = {ratio:.3f}, vacuous share {vac:.3f}")
        _note(group, R.case_id(case), ratio)
        _REPORT.setdefault(group + "_vacuous_share", {})[R.case_id(case)] = round(vac, 4)
        if group == "free_gentle" and case[4] in ("plain", "outlier"):
            assert vac == 0.0, "GENTLE must keep the bound non-vacuous for the whole run"
        again = _mode(f, s, params)
        assert all(torch.equal(a, b) for a, b in zip(again, got)), "two calls differ"
    write_report("view_mode.json", _REPORT)


@pytest.mark.parametrize("shape", [(16, 512, 102), (33, 1024, None), (64, 64, 5)], ids=str)
def test_an_images_bits_do_not_depend_on_n_or_on_its_place(shape):
    v, e, c = shape
    f, s = (t.cuda() if t is not None else None for t in R.inputs(17, v, e, c, "outlier", seed=77))
    mode, y, h2 = _mode(f, s, R.DEFAULTS)
    for i in (0, 5, 16):
        alone = _mode(f[i:i + 1].contiguous(), None if s is None else s[i:i + 1].contiguous(), R.DEFAULTS)
        assert torch.equal(alone[0], mode[i:i + 1]) and torch.equal(alone[1], y[i:i + 1]) and torch.equal(alone[2], h2[i:i + 1])
    perm = torch.tensor([16, 3, 0, 9, 5, 1, 2, 4, 6, 7, 8, 10, 11, 12, 13, 14, 15], device="cuda")      # the same images at other places
    moved = _mode(f[perm].contiguous(), None if s is None else s[perm].contiguous(), R.DEFAULTS)
    assert torch.equal(moved[0], mode[perm]) and torch.equal(moved[1], y[perm]) and torch.equal(moved[2], h2[perm])


def test_a_start_state_may_be_the_output_it_continues_into():
    native, lib = _lib()
    f, s = (t.cuda() for t in R.inputs(3, 16, 512, 102, "plain", seed=8))
    two = _mode(f, s, dict(R.DEFAULTS, outer=2))
    m, y, _ = _mode(f, s, dict(R.DEFAULTS, outer=1))
    d = R.DEFAULTS
    native.check(lib.grip_view_mode(_p(f), _p(s), 3, 16, 102, 512, d["rho"], d["lam"], d["lam_y"], d["h2_floor"], 1, d["inner"], _p(m), _p(y), _p(m), _p(y),
                                    None, None, 0, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(m, two[0]) and torch.equal(y, two[1]), "two single steps in place must be one call of two steps"


def test_refusals():
    native, lib = _lib()
    n, v, c, e = 3, 16, 5, 64
    f, s = (t.cuda() for t in R.inputs(n, v, e, c, "plain", seed=9))
    mode = torch.full((n, e), float("nan"), device="cuda")
    y, h2 = (torch.full((n, v), float("nan"), device="cuda") for _ in range(2))
    d = R.DEFAULTS

    def refused(word, n=n, v=v, c=c, e=e, ff=f, ss=s, mm=mode, yy=y, hh=h2, m0=None, y0=None, **kw):
        p = dict(d, **kw)
        rc = lib.grip_view_mode(_p(ff), _p(ss), n, v, c, e, p["rho"], p["lam"], p["lam_y"], p["h2_floor"], p["outer"], p["inner"], _p(m0), _p(y0), _p(mm),
                                _p(yy), _p(hh), None, 0, _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("n = 0", n=0)
    refused("c = 0", c=0)
    refused("v = 1", v=1)
    refused("v = 65", v=65)
    refused("e = 32", e=32)
    refused("e = 96", e=96)
    refused("e = 1088", e=1088)
    refused("rho = 0", rho=0.0)
    refused("rho = 1.5", rho=1.5)
    refused("rho = nan", rho=float("nan"))
    refused("lam = -1", lam=-1.0)
    refused("lam = inf", lam=float("inf"))
    refused("lam_y = 0", lam_y=0.0)
    refused("lam_y = nan", lam_y=float("nan"))
    refused("h2_floor = 0", h2_floor=0.0)
    refused("outer = -1", outer=-1)
    refused("inner = -1", inner=-1)
    refused("null pointer", ff=None)
    refused("null pointer", mm=None)
    refused("null pointer", yy=None)
    refused("alias", mm=f)
    refused("alias", yy=s)
    refused("alias", hh=y)
    refused("alias", y0=h2)
    refused("aligned", ff=f.reshape(-1)[1:], n=n - 1)
    nbytes = ctypes.c_size_t(7)
    assert lib.grip_view_mode_workspace(n, 65, c, e, ctypes.byref(nbytes)) == 1 and nbytes.value == 7
    assert lib.grip_view_mode_workspace(n, v, c, e, None) == 1
    torch.cuda.synchronize()
    assert torch.isnan(mode).all() and torch.isnan(y).all() and torch.isnan(h2).all() and torch.isfinite(f).all()


def test_engine_call_validates_on_the_host_and_matches_the_abi():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    f, s = (t.cuda() for t in R.inputs(3, 16, 512, 102, "outlier", seed=5))
    mode, y, h2 = engine.view_mode(f, s, want_h2=True)
    want = _mode(f, s, R.DEFAULTS)
    assert torch.equal(mode, want[0]) and torch.equal(y, want[1]) and torch.equal(h2, want[2])
    assert engine.VIEW_MODE_DEFAULTS == R.DEFAULTS
    m2, y2 = engine.view_mode(f, s, outer=1, mode_in=mode, y_in=y)       # the returned state continues the recursion
    six = _mode(f, s, dict(R.DEFAULTS, outer=6))
    assert torch.equal(m2, six[0]) and torch.equal(y2, six[1])
    m3, _ = engine.view_mode(f[:, :, :64].contiguous(), None, **R.GENTLE)
    R.check_run(f[:, :, :64].contiguous(), None, R.GENTLE, None, None, m3, None, None)
    for bad, word in ((dict(view_emb=f[0]), "view_emb must be"), (dict(view_emb=f.double()), "view_emb must be"), (dict(view_emb=f[:, :1]), "v = 1"),
                      (dict(view_emb=f[:, :, :96]), "e = 96"), (dict(view_probs=s[:2]), "view_probs must be"), (dict(view_probs=s.cpu()), "view_probs must be"),
                      (dict(mode_in=mode[:2]), "mode_in must be"), (dict(y_in=y.double()), "y_in must be"), (dict(rho=0.0), "rho = 0"), (dict(rho=2.0), "rho = 2"),
                      (dict(lam=-1.0), "lam = -1"), (dict(lam_y=0.0), "lam_y = 0"), (dict(h2_floor=float("nan")), "h2_floor = nan"),
                      (dict(outer=-1), "outer = -1"), (dict(inner=1.5), "inner = 1.5")):
        with pytest.raises(native.GripError, match=word):
            engine.view_mode(**{"view_emb": f, "view_probs": s, **bad})
    with pytest.raises(native.GripError):
        engine.view_mode(f.cpu())
