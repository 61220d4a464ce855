"""grip_label_propagate (csrc/knn_graph.hip) through the C ABI, every element against the float64 recursion on the same idx / sim with the bound that
tests/knn_ref.py carries through it (nothing in it comes from a measurement), row sums, the first-maximum arg-max, alpha = 0 bit-equal to probs, two
calls bit-equal; NaN guard rows behind every operand and output.  One planted-cluster case carries the meaning: propagation over the graph of
grip_knn_graph repairs 20 % wrong labels.  The worst |err| / bound per case goes to tests/_out/label_propagate.json."""
import ctypes
import itertools

import pytest
import torch

import knn_ref as R
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


def _guarded(x, fill):
    buf = torch.full((x.shape[0] + GUARD,) + tuple(x.shape[1:]), fill, device="cuda", dtype=x.dtype)
    buf[:x.shape[0]] = x
    return buf[:x.shape[0]]


def _propagate(probs, idx, sim, alpha, gamma, iters, want_argmax=True):
    native, lib = _lib()
    (n, c), k = probs.shape, idx.shape[1]
    p, ix, sm = _guarded(probs, float("nan")), _guarded(idx, 1 << 30), _guarded(sim, float("nan"))
    obuf = torch.full((n + GUARD, c), float("nan"), device="cuda")
    abuf = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_label_propagate_workspace(n, c, k, ctypes.byref(nbytes)))
    ws = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device="cuda")
    native.check(lib.grip_label_propagate(_p(p), _p(ix), _p(sm), alpha, gamma, iters, n, c, k, _p(obuf), _p(abuf) if want_argmax else None, _p(ws),
                                          ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(obuf[n:]).all() and (abuf[n:] == -1).all(), "a guard row of the outputs was written"
    assert torch.isfinite(obuf[:n]).all(), "an owned output element was not written (or is not finite)"
    assert (abuf[:n] >= 0).all() if want_argmax else (abuf == -1).all()
    return obuf[:n], abuf[:n]


def _inputs(n, c, k, seed):
    """Softmax rows, a random directed graph (self-loops and repeated neighbours included: n = 1 is nothing else) and sorted similarities."""
    g = torch.Generator().manual_seed(seed)
    probs = torch.softmax(4 * torch.randn(n, c, generator=g), dim=1)
    idx = torch.randint(0, n, (n, k), generator=g, dtype=torch.int32)
    idx[0, 0] = 0                                                   # a self-loop for certain
    if k > 1:
        idx[n - 1, 1] = idx[n - 1, 0]                               # ... and a repeated neighbour
    sim = torch.sort(1.2 * torch.rand(n, k, generator=g) - 0.2, dim=1, descending=True).values
    return probs.cuda(), idx.cuda(), sim.cuda()


HYPER = [(a, g) for a in (0.0, 0.5, 0.8) for g in (0.0, 10.0, 50.0)]
CASES = [(n, c, k, (1, 2, 10)[(i + i // 3) % 3], *HYPER[(i + i // 9) % 9])
         for i, (n, c, k) in enumerate(itertools.product((1, 5, 257), (1, 2, 64, 65, 102, 300), (1, 16, 32)))]
assert {c[3] for c in CASES} == {1, 2, 10} and {c[4:] for c in CASES} == set(HYPER)


@pytest.mark.parametrize("n,c,k,iters,alpha,gamma", CASES, ids=[f"n{a[0]}-c{a[1]}-k{a[2]}-it{a[3]}-a{a[4]:g}-g{a[5]:g}" for a in CASES])
def test_every_element_against_float64(n, c, k, iters, alpha, gamma):
    probs, idx, sim = _inputs(n, c, k, seed=n * 1000 + c * 10 + k)
    out, am = _propagate(probs, idx, sim, alpha, gamma, iters)
    ratio = R.check_propagation(probs, idx, sim, alpha, gamma, iters, out, am)
    _REPORT[f"n{n}.c{c}.k{k}.it{iters}.a{alpha:g}.g{gamma:g}"] = round(ratio, 4)
    write_report("label_propagate.json", _REPORT)
    print(f"n{n} c{c} k{k} it{iters} a{alpha:g} g{gamma:g}: worst |err| / bound = {ratio:.3f}")
    if alpha == 0.0:
        assert torch.equal(out, probs), "alpha = 0 changed a probability"
    again, am2 = _propagate(probs, idx, sim, alpha, gamma, iters)
    assert torch.equal(again, out) and torch.equal(am2, am), "two calls differ"


def test_argmax_is_optional_and_takes_the_first_maximum():
    probs, idx, sim = _inputs(5, 65, 16, seed=3)
    probs[:] = 0
    probs[:, 7] = probs[:, 64] = 0.5                    # two equal maxima in every row, in two different lane passes, and they stay equal
    out, am = _propagate(probs, idx, sim, 0.8, 10.0, 10)
    assert torch.equal(out[:, 7], out[:, 64]) and (am == 7).all()
    out2, _ = _propagate(probs, idx, sim, 0.8, 10.0, 10, want_argmax=False)
    assert torch.equal(out2, out)


def test_planted_clusters_are_repaired_over_the_kernels_own_graph():
    """n = 512, c = 8, e = 64, k = 8, alpha = 0.8, gamma = 10, iters = 10, seed 0: unit centres, per-dimension noise 0.25 / sqrt(e), row scales
    0.1 .. 30; probs put 0.6 on the true class -- on a wrong one for a random 20 % of the rows -- plus 0.02 U noise, renormalised.  The graph is
    grip_knn_graph's and the float64 recursion runs on THAT graph (the gap between the k-th and the (k + 1)-th neighbour can be smaller than the score
    bound: a float64 graph of its own could differ from the kernel's in a neighbour).  Preconditions on the REFERENCE: its smallest top-2 margin exceeds
    100 x the largest bound, and its accuracy is 1.0 (a float64 trial on an exact graph: accuracy 0.795 before, 1.000 after, smallest margin 0.108).
    Then the kernel's argmax_out equals the reference's on every row."""
    from test_gpu_knn_graph import _knn, _padded
    n, c, e, k = 512, 8, 64, 8
    g = torch.Generator().manual_seed(0)
    centres = torch.nn.functional.normalize(torch.randn(c, e, generator=g), dim=1)
    y = torch.randint(0, c, (n,), generator=g)
    emb = (centres[y] + 0.25 / e ** 0.5 * torch.randn(n, e, generator=g)) * (0.1 + 29.9 * torch.rand(n, 1, generator=g))
    wrong = torch.rand(n, generator=g) < 0.2
    shown = torch.where(wrong, (y + torch.randint(1, c, (n,), generator=g)) % c, y)
    probs = 0.4 / (c - 1) * torch.ones(n, c)
    probs[torch.arange(n), shown] = 0.6
    probs = probs + 0.02 * torch.rand(n, c, generator=g)
    probs = (probs / probs.sum(1, keepdim=True)).cuda()
    x = _padded(emb.cuda())
    idx, sim = _knn(x, x, k, 0)
    R.check_graph(x, x, idx, sim, 0)
    out, am = _propagate(probs, idx, sim, 0.8, 10.0, 10)
    ratio = R.check_propagation(probs, idx, sim, 0.8, 10.0, 10, out, am)
    _REPORT["planted_clusters"] = round(ratio, 4)
    z, b = R.propagate64(probs, idx, sim, 0.8, 10.0, 10)
    top2 = z.topk(2, dim=1).values
    margin, ref = float((top2[:, 0] - top2[:, 1]).min()), z.argmax(dim=1)
    before, after = float((probs.argmax(1).cpu() == y).float().mean()), float((ref.cpu() == y).float().mean())
    _REPORT["planted_clusters_reference"] = {"accuracy_before": before, "accuracy_after": after, "smallest_margin": margin, "largest_bound": float(b.max())}
    write_report("label_propagate.json", _REPORT)
    print(f"planted clusters: reference accuracy {before:.3f} -> {after:.3f}, smallest margin {margin:.3g}, largest bound {float(b.max()):.3g}")
    assert margin > 100 * float(b.max()), "precondition: the reference's margins do not dominate the bound"
    assert after == 1.0, "precondition: the float64 reference does not repair every label"
    assert before < 0.85
    assert torch.equal(am.long(), ref), "the kernel's argmax_out differs from the float64 reference's"


def test_refusals():
    native, lib = _lib()
    probs, idx, sim = _inputs(5, 64, 16, seed=9)
    out = torch.full((5, 64), float("nan"), device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def refused(word, alpha=0.8, gamma=10.0, iters=10, n=5, c=64, k=16, p=probs, o=out, ws_bytes=None):
        rc = lib.grip_label_propagate(_p(p), _p(idx), _p(sim), alpha, gamma, iters, n, c, k, _p(o), None, _p(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                      _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("alpha = 1", alpha=1.0)
    refused("alpha = -0.5", alpha=-0.5)
    refused("gamma = -1", gamma=-1.0)
    refused("iters = 0", iters=0)
    refused("k = 0", k=0)
    refused("k = 33", k=33)
    refused("n = 0", n=0)
    refused("c = 0", c=0)
    refused("null pointer", p=None)
    refused("alias", o=probs)
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_label_propagate_workspace(5, 64, 16, ctypes.byref(nbytes)))
    refused("workspace too small", ws_bytes=nbytes.value - 1)
    assert lib.grip_label_propagate_workspace(5, 64, 33, ctypes.byref(nbytes)) == 1 and "k = 33" in lib.grip_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
