"""grip_view_entropy (csrc/view_entropy.hip) through the C ABI: the loss, every gradient element, every entropy and every element of the marginal against
float64 on the same logits, evaluated ON THE KERNEL'S selection, under the bounds tests/view_entropy_ref.py derives (nothing in them is measured); the
selection itself against the selection statement of the reference (equal to the float64 one wherever the entropy gap decides it, a valid one elsewhere,
bit-identical views lower index first -- no case is left out); unselected gradient rows exactly +0.0; two calls bit-equal; an image's outputs bit-equal at
n = 1 and as image 0 / 2 of n = 3 (the gradient after the one multiplication by fl(1 / 3)); the two forms of the mean over images bit-equal; v = keep = 1
gives loss_i = H_0 within the bounds; every refusal with nothing written.  NaN / sentinel guard rows sit behind every output.  The worst |err| / bound per
output goes to tests/_out/view_entropy_kernel.json."""
import ctypes

import numpy as np
import pytest
import torch

import view_entropy_ref as R
from conftest import write_report

pytestmark = pytest.mark.gpu
GUARD = 4
SENTINEL = -7
_REPORT = {}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native, native.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(x, keep, grad=True, ent=True, sel=True, mean=True):
    """x np f32 [n, v, c] -> dict(loss, grad, H, sel, mean) of numpy arrays (None where an output was not asked for), guards checked."""
    native, lib = _lib()
    n, v, c = x.shape
    xd = torch.from_numpy(x).cuda().reshape(n * v, c).contiguous()
    loss = torch.full((1 + GUARD,), float("nan"), device="cuda")
    g = torch.full((n * v + GUARD, c), float("nan"), device="cuda") if grad else None
    h = torch.full((n + GUARD, v), float("nan"), device="cuda") if ent else None
    s = torch.full((n + GUARD, v), SENTINEL, dtype=torch.int32, device="cuda") if sel else None
    m = torch.full((n + GUARD, c), float("nan"), device="cuda") if mean else None
    native.check(lib.grip_view_entropy(_p(xd), n, v, c, keep, _p(loss), _p(g), _p(h), _p(s), _p(m), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(loss[1:]).all() and torch.isfinite(loss[0]), "the loss, or a guard behind it"
    for t, rows in ((g, n * v), (h, n), (m, n)):
        if t is not None:
            assert torch.isnan(t[rows:]).all(), "a guard row was written"
            assert torch.isfinite(t[:rows]).all(), "an owned output element was not written (or is not finite)"
    if s is not None:
        assert (s[n:] == SENTINEL).all() and ((s[:n] == 0) | (s[:n] == 1)).all()
    host = lambda t, rows, shape: None if t is None else t[:rows].cpu().numpy().reshape(shape)
    return dict(loss=loss[:1].cpu().numpy()[0], grad=host(g, n * v, (n, v, c)), H=host(h, n, (n, v)), sel=None if s is None else host(s, n, (n, v)).astype(bool),
                mean=host(m, n, (n, c)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]) if a[k].dtype == np.float32 else a[k], _bits(b[k]) if b[k].dtype == np.float32 else b[k])
               for k in ("grad", "H", "sel", "mean")) and _bits(np.float32(a["loss"])) == _bits(np.float32(b["loss"]))


def _check(x, keep, got, worst):
    n, v, c = x.shape
    R.check_selection(x, keep, got["sel"])
    ref = R.run64(x, keep, selection=got["sel"])
    for name, bname in (("loss", "bloss"), ("grad", "bgrad"), ("H", "bH"), ("mean", "bmean")):
        err = np.abs(np.asarray(got[name], dtype=np.float64) - ref[name])
        bound = np.asarray(ref[bname], dtype=np.float64)
        assert (err <= bound).all(), (name, (n, v, c, keep), float(err.max()), float(np.max(err - bound)))
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
        worst[name] = max(worst.get(name, 0.0), ratio)
    assert (_bits(got["grad"][~got["sel"]]) == 0).all(), "an unselected gradient row must be exactly +0.0"
    if v == keep == 1:      # the marginal of one view is the view: loss_i is H_0, so the loss is the mean of the kernel's own entropies within the sum of
        # the two bounds (2^-100: what the floor of the logarithm may take from a class below 2^-126)
        assert abs(float(got["loss"]) - float(got["H"][:, 0].astype(np.float64).mean())) <= ref["bloss"] + float(ref["bH"][:, 0].mean()) + 2.0 ** -100, (n, c)
    return ref


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n", R.NS)
def test_every_output_against_float64(kind, n):
    worst = {}
    for case in R.cases():
        if case[0] != kind or case[1] != n or case[3] == R.C_LIMIT:
            continue
        _, _, v, c = case
        x = R.logits(*case)
        for keep in R.keeps(v):
            got = _run(x, keep)
            _check(x, keep, got, worst)
            assert _same(_run(x, keep), got), f"two calls differ at {case}, keep = {keep}"
    print(f"view_entropy {kind} n = {n}: worst |err| / bound " + ", ".join(f"{k} {r:.3f}" for k, r in sorted(worst.items())))
    _REPORT[f"{kind}-n{n}"] = {k: round(r, 4) for k, r in worst.items()}
    top = _REPORT.setdefault("worst", {})
    for k, r in worst.items():
        top[k] = max(top.get(k, 0.0), round(r, 4))
    write_report("view_entropy_kernel.json", _REPORT)


def test_the_class_limit():
    case = R.cases()[-1]
    x = R.logits(*case)
    worst = {}
    for keep in R.keeps(case[2]):
        _check(x, keep, _run(x, keep), worst)
    print("view_entropy at c = 16000: worst |err| / bound " + ", ".join(f"{k} {r:.3f}" for k, r in sorted(worst.items())))
    _REPORT["c-limit"] = {k: round(r, 4) for k, r in worst.items()}
    write_report("view_entropy_kernel.json", _REPORT)


@pytest.mark.parametrize("kind", ["normal", "saturated", "duplicates"])
@pytest.mark.parametrize("v,c", [(5, 65), (17, 102), (64, 1000)])
def test_an_images_outputs_do_not_depend_on_n_or_on_its_place(kind, v, c):
    x = R.logits(kind, 3, v, c, seed=5)
    f = np.float32
    inv3 = f(1.0) / f(3.0)
    for keep in R.keeps(v):
        three = _run(x, keep)
        alone = [_run(x[i:i + 1].copy(), keep) for i in range(3)]
        for i in (0, 2):
            for k in ("H", "sel", "mean"):      # these carry no 1 / n
                a, b = alone[i][k][0], three[k][i]
                assert np.array_equal(_bits(a) if a.dtype == f else a, _bits(b) if b.dtype == f else b), (k, i, keep)
            assert np.array_equal(_bits((alone[i]["grad"][0] * inv3).astype(f)), _bits(three["grad"][i])), "the gradient differs by more than the factor 1 / n"
        li = [f(a["loss"]) for a in alone]      # (n = 1: loss_0 * 1.0f)
        assert _bits(f(f(f(li[0] + li[1]) + li[2]) * inv3)) == _bits(f(three["loss"])), "the mean adds the per-image losses in ascending i, then 1 / n"
        # the mean over images without mean_probs_out (one workgroup walks the images again) has the same bits; so has a call with no optional output
        for kw in (dict(mean=False), dict(grad=False, ent=False, sel=False, mean=False)):
            assert _bits(f(_run(x, keep, **kw)["loss"])) == _bits(f(three["loss"])), kw
        part = _run(x, keep, ent=False, mean=False)
        assert np.array_equal(_bits(part["grad"]), _bits(three["grad"])) and np.array_equal(part["sel"], three["sel"])


def test_refusals_leave_the_outputs_untouched():
    native, lib = _lib()
    n, v, c = 3, 5, 7
    x = torch.from_numpy(R.logits("normal", n, v, c)).cuda().reshape(n * v, c)
    loss = torch.full((1,), float("nan"), device="cuda")
    g = torch.full((n * v, c), float("nan"), device="cuda")
    h = torch.full((n, v), float("nan"), device="cuda")
    s = torch.full((n, v), SENTINEL, dtype=torch.int32, device="cuda")
    m = torch.full((n, c), float("nan"), device="cuda")

    def refused(word, n=n, v=v, c=c, keep=2, xx=x, ll=loss, gg=g, hh=h, ss=s, mm=m):
        rc = lib.grip_view_entropy(_p(xx), n, v, c, keep, _p(ll), _p(gg), _p(hh), _p(ss), _p(mm), _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("null pointer", xx=None)
    refused("null pointer", ll=None)
    refused("n = 0", n=0)
    refused("n = -1", n=-1)
    refused("c = 0", c=0)
    refused("v = 0", v=0)
    refused("v = 65", v=65)
    refused("keep = 0", keep=0)
    refused("keep = 6", keep=6)
    refused("c = 16001", c=16001)
    refused("alias", gg=x)
    refused("alias", mm=g)
    refused("alias", hh=loss)
    torch.cuda.synchronize()
    assert torch.isnan(loss).all() and torch.isnan(g).all() and torch.isnan(h).all() and torch.isnan(m).all() and (s == SENTINEL).all()
    assert torch.isfinite(x).all()


def test_engine_call_validates_on_the_host_and_matches_the_abi():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    x = R.logits("normal", 3, 16, 102, seed=3)
    want = _run(x, 4)
    xd = torch.from_numpy(x).cuda().reshape(48, 102)
    loss, grad, ent, sel, mean = engine.view_entropy(xd, 16, 4, want_entropy=True, want_selected=True, want_mean=True)
    assert loss.dim() == 0 and _bits(np.float32(loss.item())) == _bits(np.float32(want["loss"]))
    assert np.array_equal(_bits(grad.cpu().numpy().reshape(3, 16, 102)), _bits(want["grad"])) and np.array_equal(_bits(ent.cpu().numpy()), _bits(want["H"]))
    assert np.array_equal(sel.cpu().numpy().astype(bool), want["sel"]) and np.array_equal(_bits(mean.cpu().numpy()), _bits(want["mean"]))
    only = engine.view_entropy(xd, 16, 4, want_grad=False)
    assert torch.is_tensor(only) and torch.equal(only, loss)
    # the autograd twin: the gradient of the forward, scaled by the incoming scalar in the backward
    leaf = xd.clone().requires_grad_(True)
    (2.5 * engine.ViewEntropyFn.apply(leaf, 16, 4)).backward()
    assert torch.equal(leaf.grad, grad * 2.5)
    for bad, word in ((dict(logits=xd.double()), "logits must be"), (dict(logits=xd[:, ::2]), "logits must be"), (dict(logits=xd[0]), "logits must be"),
                      (dict(views=5), "multiple of views"), (dict(views=0), "views = 0"), (dict(views=65), "views = 65"), (dict(keep=0), "keep = 0"),
                      (dict(keep=17), "keep = 17"), (dict(keep=1.5), "keep = 1.5"), (dict(views=True), "views = True")):
        with pytest.raises(native.GripError, match=word):
            engine.view_entropy(**{"logits": xd, "views": 16, "keep": 4, **bad})
    with pytest.raises(native.GripError):
        engine.view_entropy(xd.cpu(), 16, 4)
    with pytest.raises(native.GripError, match="c <= 16000"):
        engine.view_entropy(torch.zeros(2, 16001, device="cuda"), 2, 1)
