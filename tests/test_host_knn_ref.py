"""The checkers of tests/knn_ref.py have teeth (CPU): they accept an f32 torch emulation of the two kernels (f32 matmul, stable sort; f32 gather
recursion) and reject planted faults -- a neighbour swapped for a worse one by 4 bounds, the self row included, a tie in the wrong order, one sim
off by 4 bounds, one Z element off by 4 bounds."""
import pytest
import torch

import knn_ref as R

N, M, E, K = 130, 1000, 64, 16
DUPS = ((3, 67), (10, 11))


@pytest.fixture(scope="module")
def graph():
    x = R.embeddings(M, E, seed=1)
    for lo, hi in DUPS:
        x[hi] = x[lo]
    q = x[37:37 + N]
    idx, sim = R.knn_f32(q, x, K, self_offset=37)
    return q, x, idx, sim


def test_graph_checker_accepts_the_f32_emulation(graph):
    q, x, idx, sim = graph
    assert R.check_graph(q, x, idx, sim, 37, DUPS) <= 1.0
    assert any((idx == hi).any() for _, hi in DUPS), "no list holds a planted duplicate: the tie check is not exercised"
    fq = R.embeddings(65, E, seed=2)
    assert R.check_graph(fq, x, *R.knn_f32(fq, x, 5), -1, DUPS) <= 1.0


def test_graph_checker_rejects_a_worse_neighbour(graph):
    q, x, idx, sim = graph
    s64, r = R.cosine64(q, x)
    i = 5
    worst = int(torch.argmin(s64[i]))
    last = int(idx[i, -1])
    assert s64[i, last] - s64[i, worst] > 4 * (r[i, last] + r[i, worst])       # worse by more than 4 bounds
    idx, sim = idx.clone(), sim.clone()
    idx[i, -1], sim[i, -1] = worst, s64[i, worst].float()                      # (its own score is right and the list stays sorted: only the selection is wrong)
    with pytest.raises(AssertionError, match=r"\(d\) selection"):
        R.check_graph(q, x, idx, sim, 37, DUPS)


def test_graph_checker_rejects_the_self_row(graph):
    q, x, idx, sim = graph
    idx, sim = idx.clone(), sim.clone()
    idx[7] = torch.cat([torch.tensor([37 + 7], dtype=torch.int32), idx[7, :-1]])
    sim[7] = torch.cat([torch.ones(1), sim[7, :-1]])
    with pytest.raises(AssertionError, match=r"\(a\) self"):
        R.check_graph(q, x, idx, sim, 37, DUPS)


def test_graph_checker_rejects_a_tie_in_the_wrong_order(graph):
    q, x, idx, sim = graph
    row, pos = [(i, int(torch.nonzero(idx[i] == 67)[0])) for i in range(N) if (idx[i] == 67).any()][0]
    assert int(idx[row, pos - 1]) == 3
    idx = idx.clone()
    idx[row, pos - 1], idx[row, pos] = 67, 3
    with pytest.raises(AssertionError, match=r"\((c|e)\)"):
        R.check_graph(q, x, idx, sim, 37, DUPS)


def test_graph_checker_rejects_a_score_off_by_four_bounds(graph):
    q, x, idx, sim = graph
    _, r = R.cosine64(q, x)
    sim = sim.clone()
    sim[9, 0] = (sim[9, 0].double() + 4 * r[9, idx[9, 0].long()]).float()       # (the first entry: the list stays sorted)
    with pytest.raises(AssertionError, match=r"\(b\) score"):
        R.check_graph(q, x, idx, sim, 37, DUPS)


@pytest.mark.parametrize("alpha,gamma,iters", [(0.8, 10.0, 10), (0.5, 50.0, 2), (0.0, 0.0, 1)])
def test_propagation_checker_accepts_the_f32_emulation_and_rejects_an_element(graph, alpha, gamma, iters):
    _, x, _, _ = graph
    pool = x[:257]
    idx, sim = R.knn_f32(pool, pool, K, self_offset=0)
    probs = torch.softmax(3 * torch.randn(257, 102, generator=torch.Generator().manual_seed(4)), dim=1)
    z, pred = R.propagate_f32(probs, idx, sim, alpha, gamma, iters)
    assert R.check_propagation(probs, idx, sim, alpha, gamma, iters, z, pred) <= 1.0
    if alpha == 0.0:
        assert torch.equal(z, probs)
    _, b = R.propagate64(probs, idx, sim, alpha, gamma, iters)
    bad = z.clone()
    bad[100, 50] = (bad[100, 50].double() + 4 * b[100, 50]).float()
    with pytest.raises(AssertionError, match="propagation: .Z - Z64."):
        R.check_propagation(probs, idx, sim, alpha, gamma, iters, bad, None)
    wrong = pred.clone()
    wrong[3] = (wrong[3] + 1) % 102
    with pytest.raises(AssertionError, match="argmax_out"):
        R.check_propagation(probs, idx, sim, alpha, gamma, iters, z, wrong)
