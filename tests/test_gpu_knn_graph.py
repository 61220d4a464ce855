"""grip_knn_graph (csrc/knn_graph.hip) through the C ABI, every row against float64 with the checker of tests/knn_ref.py: indices distinct / in range /
not the excluded row, every score within r = (2 e + 12) u T, the list sorted by (sim descending, index ascending), the selection right up to the
two bounds, planted bit-identical base rows in index order with equal bits.  Nothing in the bound comes from a measurement (knn_ref's docstring).

Every operand is followed by NaN guard rows, idx_out / sim_out are -1 / NaN prefilled and followed by guard rows that must keep their fill.  Shapes
are relative to the kernel's 64 x 64 tiles and 32-float stages.  The worst |err| / bound per case goes to tests/_out/knn_graph.json."""
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


def _padded(x):
    """x followed by GUARD rows of NaN in one allocation: the view of the owned rows."""
    buf = torch.full((x.shape[0] + GUARD,) + tuple(x.shape[1:]), float("nan"), device="cuda", dtype=torch.float32)
    buf[:x.shape[0]] = x
    return buf[:x.shape[0]]


def _knn(q, x, k, self_offset):
    """The ABI call on guarded buffers.  q may be a view of x's rows (pool on pool, a window): it is passed as it is."""
    native, lib = _lib()
    (n, e), m = q.shape, x.shape[0]
    ibuf = torch.full((n + GUARD, k), -1, dtype=torch.int32, device="cuda")
    sbuf = torch.full((n + GUARD, k), float("nan"), device="cuda")
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_knn_graph_workspace(n, m, e, k, ctypes.byref(nbytes)))
    ws = torch.full((nbytes.value,), 0xFF, dtype=torch.uint8, device="cuda")      # (NaN bit patterns: nothing may rely on a zeroed workspace)
    native.check(lib.grip_knn_graph(_p(q), _p(x), n, m, e, k, self_offset, _p(ibuf), _p(sbuf), _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    assert (ibuf[n:] == -1).all() and torch.isnan(sbuf[n:]).all(), "a guard row of the outputs was written"
    assert (ibuf[:n] >= 0).all() and torch.isfinite(sbuf[:n]).all(), "an owned output element was not written (or is not finite)"
    return ibuf[:n], sbuf[:n]


DUPS = ((3, 67), (10, 11))      # across the boundary of the first two base tiles / inside one tile


def _base(m, e, seed):
    x = R.embeddings(m, e, seed, "cuda")
    dups = tuple((lo, hi) for lo, hi in DUPS if hi < m)
    for lo, hi in dups:
        x[hi] = x[lo]
    return _padded(x), dups


def _operands(mode, n, m, e, seed):
    x, dups = _base(m, e, seed)
    if mode == "pool":
        return x[:n], x, 0, dups
    if mode == "window":
        return x[37:37 + n], x, 37, dups
    return _padded(R.embeddings(n, e, seed + 1, "cuda")), x, -1, dups


def _cases():
    """m x e x k in full, n and the query mode dealt round-robin (a mode that does not fit m falls back to a smaller n, then to foreign queries)."""
    ns, modes, out = (1, 63, 65, 130), ("pool", "window", "foreign"), []
    for i, (mname, e, k) in enumerate(itertools.product(("k+1", 64, 65, 200, 1000), (4, 36, 64, 512), (1, 5, 16, 32))):
        m = k + 1 if mname == "k+1" else mname
        n, mode = ns[(i + i // 4) % 4], modes[(i + i // 16) % 3]
        if m - (mode != "foreign") < k:
            mode = "foreign"
        room = {"pool": m, "window": m - 37, "foreign": 1 << 30}[mode]
        if n > room:
            fits = [v for v in ns if v <= room]
            n, mode = (max(fits), mode) if fits else (n, "foreign")
        out.append((mode, n, m, e, k))
    assert {c[0] for c in out} == set(modes) and {c[1] for c in out} == set(ns)
    return out


CASES = _cases()


@pytest.mark.parametrize("mode,n,m,e,k", CASES, ids=[f"{c[0]}-n{c[1]}-m{c[2]}-e{c[3]}-k{c[4]}" for c in CASES])
def test_every_row_against_float64(mode, n, m, e, k):
    q, x, off, dups = _operands(mode, n, m, e, seed=n * 7919 + m * 31 + e + k)
    idx, sim = _knn(q, x, k, off)
    ratio = R.check_graph(q, x, idx, sim, off, dups)
    _REPORT[f"{mode}.n{n}.m{m}.e{e}.k{k}"] = round(ratio, 4)
    write_report("knn_graph.json", _REPORT)
    print(f"{mode} n{n} m{m} e{e} k{k}: worst |err| / bound = {ratio:.3f}")


def test_duplicates_are_listed_in_index_order():
    """Queries close to the planted duplicates, so that every list holds both pairs (the checker's tie property is exercised on every row)."""
    x, dups = _base(200, 64, seed=11)
    g = torch.Generator().manual_seed(12)
    q = _padded(torch.cat([x[3] + 0.01 * x[3].norm() * torch.randn(33, 64, generator=g).cuda() / 8,
                           x[10] + 0.01 * x[10].norm() * torch.randn(32, 64, generator=g).cuda() / 8]))
    idx, sim = _knn(q, x, 5, -1)
    R.check_graph(q, x, idx, sim, -1, dups)
    assert (idx[:33, :2] == torch.tensor([3, 67], device="cuda", dtype=torch.int32)).all()
    assert (idx[33:, :2] == torch.tensor([10, 11], device="cuda", dtype=torch.int32)).all()


WALK_N = {1: 200000, 6: 33000}      # query rows at which knn_shares deals the 16 base tiles of m = 1 000 (4 of m = 200) to 1 / 6 (1 / 4) workgroups per query tile


def _walked(q, x, k, shares):
    """The call with the query block `q` repeated to WALK_N[shares] rows, so that ONE workgroup walks several base tiles (all of them at shares = 1:
    the accumulator reset, the compare with the list's current k-th entry, the ballot skip, the stage / tile advance of the main loop -- the path of
    the pool shape); with the few rows of `q` alone every base tile has a workgroup of its own and all cross-tile work is the merge kernel's.
    Returns the rows of `q`."""
    n = q.shape[0]
    big = _padded(q.repeat(-(-WALK_N[shares] // n), 1)[:WALK_N[shares]])
    idx, sim = _knn(big, x, k, -1)
    assert torch.equal(idx[n:2 * n], idx[:n]) and torch.equal(sim[n:2 * n], sim[:n]), "the same query rows in another query tile give other bits"
    return idx[:n].clone(), sim[:n].clone()


@pytest.mark.parametrize("m,e,k", [(m, e, k) for m in (200, 1000) for e in (36, 64, 512) for k in (1, 5, 32)])
def test_one_workgroup_walks_many_tiles_against_float64(m, e, k):
    """Random bases with the planted duplicates, 130 foreign queries: the lists of a one-share call (a workgroup walks every base tile, e / 32 stages
    each) and of a call with a few tiles per workgroup, every row against float64 and bit-equal to the fully split call."""
    x, dups = _base(m, e, seed=51 + m + e + k)
    q = _padded(R.embeddings(130, e, 52, "cuda"))
    split_i, split_s = _knn(q, x, k, -1)
    for shares in (1, 6):
        idx, sim = _walked(q, x, k, shares)
        _REPORT[f"walk{shares}.m{m}.e{e}.k{k}"] = round(R.check_graph(q, x, idx, sim, -1, dups), 4)
        assert torch.equal(idx, split_i) and torch.equal(sim, split_s), f"{shares} share(s): the lists differ from the fully split call's"
    write_report("knn_graph.json", _REPORT)


@pytest.mark.parametrize("e,k", [(e, k) for e in (64, 512) for k in (1, 16, 32)])
def test_ascending_and_descending_scores_select_the_same_rows(e, k):
    """x_j = cos(theta_j) d + sin(theta_j) d_perp_j with theta monotone in j and the queries near d.  theta descending in j: the scores ascend along the
    base, so a workgroup that walks the base finds k insertions in every tile; theta ascending: none after the first tile.  Run with one share (one
    workgroup walks all 16 tiles: the LDS list takes every insertion), with six, and fully split (one tile per workgroup: the merge kernel takes
    them).  One base in the two orders: the same rows, the same bits, however the base is split."""
    m, n = 1000, 65
    g = torch.Generator().manual_seed(21)
    d = torch.nn.functional.normalize(torch.randn(e, generator=g, dtype=torch.float64), dim=0)
    perp = torch.randn(m, e, generator=g, dtype=torch.float64)
    perp = torch.nn.functional.normalize(perp - (perp @ d)[:, None] * d, dim=1)
    theta = torch.linspace(0.2, 1.2, m, dtype=torch.float64)
    scale = 0.1 + 29.9 * torch.rand(m, 1, generator=g, dtype=torch.float64)
    x_desc = _padded(((torch.cos(theta)[:, None] * d + torch.sin(theta)[:, None] * perp) * scale).float().cuda())      # scores descending in j
    x_asc = _padded(x_desc.flip(0))                                                                                  # scores ascending in j
    q = _padded(((d + 0.16 / e ** 0.5 * torch.randn(n, e, generator=g, dtype=torch.float64)) * (0.1 + 29.9 * torch.rand(n, 1, generator=g, dtype=torch.float64))).float().cuda())
    i_d, s_d = _walked(q, x_desc, k, 1)
    i_a, s_a = _walked(q, x_asc, k, 1)
    _REPORT[f"descending.e{e}.k{k}"] = round(R.check_graph(q, x_desc, i_d, s_d), 4)
    _REPORT[f"ascending.e{e}.k{k}"] = round(R.check_graph(q, x_asc, i_a, s_a), 4)
    write_report("knn_graph.json", _REPORT)
    for name, x, want in (("descending", x_desc, (i_d, s_d)), ("ascending", x_asc, (i_a, s_a))):
        for how, got in (("six shares", _walked(q, x, k, 6)), ("fully split", _knn(q, x, k, -1))):
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{name}, {how}: the lists differ from the one-share call's"
    assert (i_d < 64).float().mean() > 0.9 and (i_a >= m - 64).float().mean() > 0.9      # the construction does what it says: the best rows sit in one end tile
    if k > 1:
        assert (s_d[:, :-1] != s_d[:, 1:]).all(), "precondition: a list holds two equal scores (the index tie-break would differ between the orders)"
    # The same scores bit for bit, and the same rows -- except where the k-th place is an exact tie between two base rows in the kernel's own scores
    # (equal bits in s_a and s_d at that place): the total order gives it to the lower index, which is the other row once the base is flipped.  With no
    # equal scores inside a list (above) that can only be a list's last entry.
    assert torch.equal(s_a, s_d), "the two orders of one base do not select the same scores"
    differs = (m - 1 - i_a) != i_d
    print(f"e{e} k{k}: {int(differs.sum())} of {n} rows end in an exact tie for the k-th place")
    assert not differs[:, :-1].any() and int(differs.sum()) <= n // 8, "the two orders of one base do not select the same rows"


def test_a_rows_bits_do_not_depend_on_n_place_or_call():
    m, e, k, n = 1000, 36, 16, 130
    x, _ = _base(m, e, seed=31)
    fq = _padded(R.embeddings(n, e, 32, "cuda"))
    idx, sim = _knn(fq, x, k, -1)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(33)).cuda()
    pi, ps = _knn(_padded(fq[perm]), x, k, -1)
    assert torch.equal(pi, idx[perm]) and torch.equal(ps, sim[perm]), "a row's bits depend on its place in the query block"
    widx, wsim = _knn(x[37:37 + n], x, k, 37)
    for i in (0, 17, 64, 129):
        a, b = _knn(fq[i:i + 1].clone(), x, k, -1)
        assert torch.equal(a, idx[i:i + 1]) and torch.equal(b, sim[i:i + 1]), f"row {i} alone differs from row {i} of the n = {n} call"
        a, b = _knn(x[37 + i:38 + i], x, k, 37 + i)
        assert torch.equal(a, widx[i:i + 1]) and torch.equal(b, wsim[i:i + 1]), f"window row {i} alone differs from row {i} of the n = {n} call"
    # the queries as a copy (their norms computed in a launch of their own) instead of a view of the base (norms computed once)
    a, b = _knn(_padded(x[37:37 + n].clone()), x, k, 37)
    assert torch.equal(a, widx) and torch.equal(b, wsim), "a window's bits depend on whether it aliases the base"
    a, b = _knn(x[37:37 + n], x, k, 37)
    assert torch.equal(a, widx) and torch.equal(b, wsim), "two runs differ"


def test_a_score_is_an_ascending_chain_over_e():
    """An f32 MFMA is a k-ordered fmaf chain, and the staging hands consecutive fours of e to consecutive MFMAs: a score is fmaf over e ascending.
    Rows on which the order decides the result exactly (q = ones, so |q| = 8 and its reciprocal is exact):
      A_o: x[o] = 2^24, x[o + 1] = -2^24, x[o + 4] = 1   ascending: (2^24 - 2^24) + 1 = 1;  with x[o + 4] between the two: (2^24 + 1 -> 2^24) - 2^24 = 0
      B_o: x[o] = 1, x[o + 1] = 2^24, x[o + 4] = -2^24   ascending: (1 + 2^24 -> 2^24) - 2^24 = 0;  any order that adds the 1 last: 1
    at o = 0 (inside a four-by-four block of the staging), 15 (across two blocks) and 32 (the second 32-float stage).  Both sums of squares are
    2^49 in f32 in any order."""
    e, big = 64, 2.0 ** 24
    x = torch.zeros(6, e)
    for i, o in enumerate((0, 15, 32)):
        x[2 * i, o], x[2 * i, o + 1], x[2 * i, o + 4] = big, -big, 1.0
        x[2 * i + 1, o], x[2 * i + 1, o + 1], x[2 * i + 1, o + 4] = 1.0, big, -big
    idx, sim = _knn(_padded(torch.ones(1, e).cuda()), _padded(x.cuda()), 6, -1)
    want = float((1.0 / torch.sqrt(torch.tensor(2.0 ** 49, dtype=torch.float32))) * 0.125)
    got = dict(zip(idx[0].tolist(), sim[0].tolist()))
    assert idx[0].tolist() == [0, 2, 4, 1, 3, 5], idx          # the three A rows (equal scores: by index), then the three B rows
    for j in (0, 2, 4):
        assert abs(got[j] - want) <= 3e-7 * want, (j, got[j], want)
    for j in (1, 3, 5):
        assert got[j] == 0.0, (j, got[j])


def test_rows_do_not_depend_on_the_base_split():
    """With few query tiles the base tiles are dealt to several workgroups per query tile and the shares' lists are merged (csrc/knn_graph.hip,
    knn_shares: 16 shares -- one per base tile -- at n = 130, 6 at n = 33 000, 1 at n = 200 000 for these 16 base tiles).  The same rows come out
    with the same bits; e = 4 keeps the large calls small."""
    m, e, k = 1000, 4, 16
    x, dups = _base(m, e, seed=41)
    q = _padded(R.embeddings(200000, e, 42, "cuda"))
    whole_i, whole_s = _knn(q, x, k, -1)
    for n in (130, 33000):
        a, b = _knn(_padded(q[:n].clone()), x, k, -1)
        assert torch.equal(a, whole_i[:n]) and torch.equal(b, whole_s[:n]), f"rows 0 .. {n - 1} differ from the same rows of the 200 000-row call"
    _REPORT["split.n200000"] = round(R.check_graph(q[:130], x, whole_i[:130], whole_s[:130], -1, dups), 4)
    write_report("knn_graph.json", _REPORT)


def test_refusals():
    """Each constraint of include/grip_amd.h returns status 1 and a message; nothing is launched (the outputs keep their fill)."""
    native, lib = _lib()
    big = torch.randn(64, 4096, device="cuda")
    idx = torch.full((64, 32), -1, dtype=torch.int32, device="cuda")
    sim = torch.full((64, 32), float("nan"), device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def refused(word, n=4, m=40, e=64, k=5, off=-1, q=True, ws_bytes=None, shift=0):
        x = big[:, :e].contiguous() if e <= 4096 else big
        qp = ctypes.c_void_p(x.data_ptr() + shift) if q else None
        rc = lib.grip_knn_graph(qp, _p(x), n, m, e, k, off, _p(idx), _p(sim), _p(ws), ws.numel() if ws_bytes is None else ws_bytes, _stream())
        msg = lib.grip_last_error().decode()
        assert rc == 1 and word in msg, (rc, msg)

    refused("e = 6", e=6)
    refused("e = 0", e=0)
    refused("e = 2052", e=2052)
    refused("k = 0", k=0)
    refused("k = 33", k=33)
    refused("n = 0", n=0)
    refused("m = 0", m=0)
    refused("k = 5 neighbours out of 4", m=4)                 # m >= k ...
    refused("k = 5 neighbours out of 4", m=5, off=0)          # ... after the row itself is excluded
    refused("runs past", n=4, m=40, off=37)                   # self_offset + n <= m
    refused("self_offset = -2", off=-2)
    refused("null pointer", q=False)
    refused("16-byte aligned", shift=4)
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_knn_graph_workspace(4, 40, 64, 5, ctypes.byref(nbytes)))
    refused("workspace too small", ws_bytes=nbytes.value - 1)
    for args, word in (((4, 40, 6, 5), "e = 6"), ((0, 40, 64, 5), "n = 0"), ((4, 40, 64, 33), "k = 33")):
        assert lib.grip_knn_graph_workspace(*args, ctypes.byref(nbytes)) == 1 and word in lib.grip_last_error().decode()
    torch.cuda.synchronize()
    assert (idx == -1).all() and torch.isnan(sim).all()
