"""grip_candidate_select (csrc/candidate.hip) through the C ABI: threshold, mask, count and label EQUAL to the NumPy reference of tests/candidate_ref.py --
zero tolerance -- at every n x c of the table, for every claim in {1, 2, n, ceil(2 n / c)}, tau in {0.5, 0.99, 1.0}, all four combine modes and four
kinds of pool, three of which force ties (probabilities quantised to multiples of 2^-6; duplicated columns and rows with an all-zero column; uniform
rows).  Then: a row's bits independent of n and of its place given the threshold, two calls bit-equal, the optional outputs absent, the refusals with
nothing written, and the engine's operand checks.  Guard rows of a sentinel sit behind every output: a write past one would show."""
import ctypes

import numpy as np
import pytest
import torch

import candidate_ref as R

pytestmark = pytest.mark.gpu
GUARD = 8
SENTINEL = -(2 ** 30) - 12345


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native, native.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_COMBINE = {name: i for i, name in enumerate(R.COMBINE)}


def _select(p, claim, tau, combine, want=(True, True, True)):
    """(threshold, mask, count, label) of one call on a device tensor p [n, c] (each optional output None when not wanted); asserts the guards."""
    native, lib = _lib()
    n, c = p.shape
    w = R.words(c)
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_candidate_select_workspace(n, c, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    thr = torch.full((c + GUARD,), float("nan"), device="cuda")
    mask = torch.full((n + GUARD, w), SENTINEL, dtype=torch.int32, device="cuda")
    count = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    label = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    native.check(lib.grip_candidate_select(_p(p), n, c, claim, tau, _COMBINE[combine], _p(thr if want[0] else None), _p(mask), _p(count if want[1] else None),
                                           _p(label if want[2] else None), _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(thr[c:]).all() and (mask[n:] == SENTINEL).all() and (count[n:] == SENTINEL).all() and (label[n:] == SENTINEL).all(), "a guard was written"
    for out, wanted in ((thr, want[0]), (count, want[1]), (label, want[2])):
        assert wanted or bool(((out != out) | (out == SENTINEL)).all()), "an output that was not asked for was written"
    return thr[:c] if want[0] else None, mask[:n], count[:n] if want[1] else None, label[:n] if want[2] else None


SHAPES = [(n, c) for n in R.SEL_NS for c in R.SEL_CS]


@pytest.mark.parametrize("n,c", SHAPES, ids=[f"{n}x{c}" for n, c in SHAPES])
def test_equal_to_the_reference(n, c):
    for kind in R.SEL_KINDS:
        host = R.pool(n, c, kind)
        rank = R.Ranking(host)
        p = torch.from_numpy(host).cuda()
        pos, order = torch.from_numpy(rank.pos).cuda(), torch.from_numpy(rank.order).cuda()
        intra = {tau: torch.from_numpy(rank.intra(tau)).cuda() for tau in R.SEL_TAUS}
        for claim in R.claims(n, c):
            want_thr = torch.from_numpy(rank.threshold(claim)).cuda()
            inter = torch.from_numpy(rank.inter(claim)).cuda()
            for tau in R.SEL_TAUS:
                for combine in R.COMBINE:
                    thr, mask, count, label = _select(p, claim, tau, combine)
                    want = R.outputs_t(R.combine_sets(intra[tau], inter, combine), pos, order)
                    case = f"{kind} {n}x{c} claim {claim} tau {tau} {combine}"
                    assert torch.equal(thr.view(torch.int32), want_thr.view(torch.int32)), f"{case}: threshold"
                    assert torch.equal(mask, want[0]), f"{case}: mask"
                    assert torch.equal(count, want[1]), f"{case}: count"
                    assert torch.equal(label, want[2]), f"{case}: label"


def test_the_torch_side_of_the_comparison_is_the_numpy_reference():
    """outputs_t (used above so that a large case needs no host pass per mode) against the all-NumPy select()."""
    n, c = 65, 33
    for kind in R.SEL_KINDS:
        rank = R.Ranking(R.pool(n, c, kind))
        pos, order = torch.from_numpy(rank.pos).cuda(), torch.from_numpy(rank.order).cuda()
        for claim in R.claims(n, c):
            for combine in R.COMBINE:
                member = R.combine_sets(torch.from_numpy(rank.intra(0.99)).cuda(), torch.from_numpy(rank.inter(claim)).cuda(), combine)
                got = R.outputs_t(member, pos, order)
                want = R.select(rank, claim, 0.99, combine)
                assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want[:3]))


@pytest.mark.parametrize("c", [33, 102, 129, 300])
def test_a_rows_bits_do_not_depend_on_n_or_on_its_place(c):
    """Given the threshold: a subset of the rows, permuted, is selected with a claim that reproduces the same thresholds (the rows that define them kept)."""
    n = 1000
    host = R.pool(n, c, "softmax")
    host[:, 0] = np.float32(0.5)                            # a tied column: its threshold is 0.5 for any claim and any subset
    p = torch.from_numpy(host).cuda()
    for combine in R.COMBINE:
        thr, mask, count, label = _select(p, n, 0.99, combine)           # claim = n: the thresholds are the column minima
        low = torch.unique(p.argmin(dim=0))                              # the rows that hold them
        rows = torch.cat([torch.tensor([n - 1, 3, 516, 0, 64], device="cuda"), low]).unique()
        rows = rows[torch.randperm(len(rows), generator=torch.Generator().manual_seed(c)).cuda()]
        sub = p[rows].contiguous()
        thr2, mask2, count2, label2 = _select(sub, len(rows), 0.99, combine)
        assert torch.equal(thr2, thr) and torch.equal(mask2, mask[rows]) and torch.equal(count2, count[rows]) and torch.equal(label2, label[rows])
    one = p[7:8].contiguous()                                            # n = 1 with tau alone deciding
    _, m1, c1, l1 = _select(one, 1, 0.5, "intra")
    _, mf, cf, lf = _select(p, 3, 0.5, "intra")
    assert torch.equal(m1, mf[7:8]) and torch.equal(c1, cf[7:8]) and torch.equal(l1, lf[7:8])


def test_two_calls_are_bit_equal_and_optional_outputs_can_be_absent():
    n, c = 1000, 102
    p = torch.from_numpy(R.pool(n, c, "quantised")).cuda()
    full = _select(p, 20, 0.99, "intersection")
    again = _select(p, 20, 0.99, "intersection")
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        got = _select(p, 20, 0.99, "intersection", want)
        assert all(g is None or torch.equal(g, f) for g, f in zip(got, full))


def test_refusals():
    native, lib = _lib()
    n, c = 17, 33
    p = torch.from_numpy(R.pool(n, c, "softmax")).cuda()
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_candidate_select_workspace(n, c, ctypes.byref(nbytes)))
    assert nbytes.value >= c * 256 * 4
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    thr = torch.full((c,), float("nan"), device="cuda")
    mask = torch.full((n, R.words(c)), SENTINEL, dtype=torch.int32, device="cuda")
    count, label = (torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2))

    def refused(word, n=n, c=c, claim=2, tau=0.99, combine=0, pp=p, mm=mask, ww=ws, nb=None):
        rc = lib.grip_candidate_select(_p(pp), n, c, claim, tau, combine, _p(thr), _p(mm), _p(count), _p(label), _p(ww), ws.numel() if nb is None else nb,
                                       _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("null pointer", pp=None)
    refused("null pointer", mm=None)
    refused("null pointer", ww=None)
    refused("n = 0", n=0)
    refused("n = -1", n=-1)
    refused("c = 0", c=0)
    refused("claim = 0", claim=0)
    refused("claim = 18", claim=n + 1)
    refused("claim = -3", claim=-3)
    refused("tau = 0", tau=0.0)
    refused("tau = -0.5", tau=-0.5)
    refused("tau = 1.5", tau=1.5)
    refused("tau = nan", tau=float("nan"))
    refused("combine = 4", combine=4)
    refused("combine = -1", combine=-1)
    refused("workspace too small", nb=nbytes.value - 1)
    assert lib.grip_candidate_select_workspace(0, c, ctypes.byref(nbytes)) == 1
    assert lib.grip_candidate_select_workspace(n, c, None) == 1
    torch.cuda.synchronize()
    assert torch.isnan(thr).all() and (mask == SENTINEL).all() and (count == SENTINEL).all() and (label == SENTINEL).all()


def test_engine_call_checks_its_operands():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    n, c = 65, 102
    host = R.pool(n, c, "duplicates")
    p = torch.from_numpy(host).cuda()
    for combine in R.COMBINE:
        mask, count, label, thr = engine.candidate_select(p, 3, 0.99, combine)
        want = R.select(host, 3, 0.99, combine)
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((mask, count, label, thr), want))
    assert all(torch.equal(a, b) for a, b in zip(engine.candidate_select(p, 3), engine.candidate_select(p.double(), 3, tau=0.99, combine="intersection")))
    for bad, word in ((dict(probs=p[0]), "probs must be"), (dict(probs=p.int()), "probs must be"), (dict(claim=0), "claim = 0"), (dict(claim=n + 1), "claim = 66"),
                      (dict(claim=2.0), "claim = 2.0"), (dict(tau=0.0), "tau = 0"), (dict(tau=1.01), "tau = 1.01"), (dict(combine="both"), "combine = 'both'")):
        with pytest.raises(native.GripError, match=word):
            engine.candidate_select(**{**dict(probs=p, claim=3), **bad})
    with pytest.raises(native.GripError):
        engine.candidate_select(p.cpu(), 3)
