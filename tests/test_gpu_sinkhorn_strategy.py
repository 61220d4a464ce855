"""BALANCED_PSEUDOLABELS through the strategies (`small` towers, the synthetic pool of test_gpu_pool_cache: 6 classes, 108 unlabeled images).  With the
switch on, a textual strategy's assign_pseudo_labels returns the leaderboard over the FLOAT64 recursion (tests/sinkhorn_ref.py) on the same
probabilities -- on the head's, or with TRANSDUCTIVE_GMM as well on the assignments Z of engine.gmm_transduce -- wherever the float64 ranking is
separated by more than the derived bound; the rows left out for that reason are counted and may be at most 2 % of the pool.  Every class receives its k
entries, each with that class as its arg-max: what the balance is for.  The pickles are named `_ot_` / `_ot_gmm_`.  With the switch absent nothing
moves: the lists and file names are those of the plain head -> scan and no balance call is made."""
import glob
import os

import numpy as np
import pytest
import torch

import sinkhorn_ref as R
from test_gpu_pool_cache import _strategy

pytestmark = pytest.mark.gpu
OT = dict(BALANCED_PSEUDOLABELS=True, OT_TAU=1.0, OT_ITERS=3)          # (the defaults, spelled out)
GMM = dict(TRANSDUCTIVE_GMM=True, GMM_K=4, GMM_LAMBDA=2.0, GMM_ITERS=1, GMM_Z_ITERS=1)
K = 4
# The pool of test_gpu_pool_cache._strategy is synthetic_pool(6, 20, 64, seed 23).  On it the FLOAT64 reference alone leaves too many rows undecided for
# these checks (4 of 108 on the head's probabilities at tau 1, iters 3; 105 of 108 on the GMM's Z, most of whose rows are 1.0 to the last bit after three
# rounds), so the two balanced passes draw the same pool from other seeds, on which it leaves none: 2 for the head, 1 for one GMM round of one sweep.
HEAD_SEED, GMM_SEED = 2, 1


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("GRIP_PSEUDOLABEL_MODE", "GRIP_SPLIT_TIER", "GRIP_SCREEN_STREAM"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture
def calls(monkeypatch):
    """calls() -> [(n, c, tau, iters)] of every engine.sinkhorn_balance call so far."""
    import grip_amd  # noqa: F401
    from grip_amd import engine
    seen, real = [], engine.sinkhorn_balance

    def balance(probs, tau=1.0, iters=3, prior=None, log_scale=None):
        seen.append((*probs.shape, tau, iters))
        return real(probs, tau, iters, prior, log_scale)
    monkeypatch.setattr(engine, "sinkhorn_balance", balance)
    return lambda: list(seen)


def _pool_seed(monkeypatch, seed):
    """_strategy builds its pool with methods.main.synthetic_pool: the same call with another seed."""
    from grip_amd.methods import main
    real = main.synthetic_pool
    monkeypatch.setattr(main, "synthetic_pool", lambda classes, per_class, res, _seed: real(classes, per_class, res, seed))


def _pickles(root):
    return sorted(os.path.basename(f) for f in glob.glob(os.path.join(str(root), "pseudolabels", "*_pseudolabels_*split_*.pickle")))


def _undecided_rows(q64, bq, k):
    """Rows that take part in a comparison of the scan which the bound does not decide.  The scan (csrc/leaderboard.cpp: a board is an append list until
    its first overflow sorts it; a row its arg-max board rejects is offered to every other board) is walked here on the float64 values, and both rows
    of a comparison are marked when their values are within the two bounds plus the f32 rounding of both (u q each: the scan reads f32): the row
    against the board's last entry, the row against the entries of a board it enters (the sort or the insertion may compare it with any of them; at the
    first overflow the entries also with one another), and a row's largest value against its runner-up (the arg-max)."""
    q, slack = q64.numpy(), (bq + R.U * q64).numpy()
    n, c = q.shape
    amb = np.zeros(n, dtype=bool)
    boards, is_sorted = [[] for _ in range(c)], [False] * c

    def close(a, b, j):
        if abs(q[a, j] - q[b, j]) <= slack[a, j] + slack[b, j]:
            amb[a] = amb[b] = True

    def admits(i, j):
        b = boards[j]
        if len(b) < k:
            return True
        close(i, b[-1], j)
        return q[b[-1], j] < q[i, j]

    def offer(i, j):
        b = boards[j]
        if len(b) < k:
            b.append(i)
            return
        if not admits(i, j):
            return
        for a in b:
            close(i, a, j)
        if not is_sorted[j]:
            for x in range(len(b)):
                for y in range(x):
                    close(b[x], b[y], j)
            is_sorted[j] = True
        b.append(i)
        b.sort(key=lambda a: -q[a, j])
        b.pop()

    for i in range(n):
        order = np.argsort(-q[i], kind="stable")
        js = int(order[0])
        if c > 1 and q[i, js] - q[i, order[1]] <= slack[i, js] + slack[i, order[1]]:
            amb[i] = True
        if admits(i, js):
            offer(i, js)
        else:
            for j in range(c):
                if j != js:
                    offer(i, j)
    return torch.from_numpy(amb)


def _check_lists(got, z, labels, paths, tau, iters, name):
    """`got` (the strategy's dataset) against the leaderboard over the float64 recursion on z, outside the undecided rows; every class k entries of its own."""
    from grip_amd import engine, pseudolabels as pl
    n, c = z.shape
    lt = R.log_target_of(c, device=z.device)
    q64, _, _, bq, _, _, rho = R.balance64(z, lt, tau, iters, bounds=True)
    assert rho < 0.5
    amb = _undecided_rows(q64.cpu(), bq.cpu(), K)
    left_out = int(amb.sum())
    want = pl.leaderboard(q64.float().cpu().numpy(), q64.argmax(1).int().cpu().numpy(), paths, labels, K)
    skip = {paths[i] for i in np.flatnonzero(amb.numpy())}
    pairs_got = {(f, l) for f, l in zip(got.filepaths, got.labels) if f not in skip}
    pairs_want = {(f, l) for f, l in zip(*want) if f not in skip}
    _, pred, mass, _ = engine.sinkhorn_balance(z, tau, iters)       # (the kernel's own arg-max: bit-identical from call to call)
    own = dict(zip(paths, (labels[int(j)] for j in pred.cpu())))
    entries = {lab: [f for f, l in zip(got.filepaths, got.labels) if l == lab] for lab in labels}
    of_own = {lab: sum(own[f] == lab for f in mine) for lab, mine in entries.items()}
    print(f"{name}: {left_out} of {n} rows are not separated by the bound in float64 (largest bound {float(bq.max()):.2e}); {len(pairs_got ^ pairs_want)} entries "
          f"differ outside them; entries per class {[len(v) for v in entries.values()]}, of the class's own arg-max {list(of_own.values())}; arg-max rows per "
          f"class before {torch.bincount(z.argmax(1), minlength=c).tolist()} and after {torch.bincount(pred.long(), minlength=c).tolist()}")
    assert left_out <= 0.02 * n, f"{name}: the float64 reference leaves {left_out} of {n} rows undecided on this pool"
    assert pairs_got == pairs_want and len(pairs_want) >= c * K - 2 * left_out
    for lab in labels:      # every class receives k entries whose arg-max is that class
        assert len(entries[lab]) == K and of_own[lab] == K, (name, lab, entries[lab])
    return mass


def test_textual_pass_is_the_leaderboard_over_the_balanced_head(tmp_path, monkeypatch, calls):
    from grip_amd import engine, pseudolabels as pl
    _pool_seed(monkeypatch, HEAD_SEED)
    m, train, unlabeled = _strategy("TextualFPL", tmp_path, monkeypatch, **OT)
    b = m.balanced
    assert isinstance(b, pl.BalancedAssignment) and (b.tau, b.iters, b.prior, b.inner) == (1.0, 3, None, None) and m.transduction() is b
    m.define_model(m.classes)
    images, paths = unlabeled.images, list(unlabeled.filepaths)
    labels = [m.label_to_idx[c] for c in m.classes]
    emb, txt = m.trained_features(images, m.classes)
    _, probs, _, _ = engine.cosine_head(emb, txt.detach(), m.scale())
    n0 = len(calls())
    got = m.assign_pseudo_labels(K, unlabeled)      # (identical mode is the default: with a transduction installed the pass takes its plain branch)
    assert calls()[n0:] == [(len(paths), len(labels), 1.0, 3)] and pl.propagation() is None
    mass = _check_lists(got, probs, labels, paths, 1.0, 3, "head")
    assert torch.equal(m.balanced.state[0], mass) and m.gmm_state is None
    unlabeled.filepaths, unlabeled.labels = list(paths), None
    m.create_training_dataset(train, unlabeled)
    names = _pickles(tmp_path)
    assert len(names) == 1 and "_pseudolabels_ot_split_" in names[0], names


def test_textual_pass_balances_the_gmm_assignments(tmp_path, monkeypatch, calls):
    from grip_amd import engine, pseudolabels as pl
    _pool_seed(monkeypatch, GMM_SEED)
    m, train, unlabeled = _strategy("TextualFPL", tmp_path, monkeypatch, **OT, **GMM)
    assert m.balanced.inner is m.gmm and m.transduction() is m.balanced and m.balanced.infix == "ot_gmm_" and m.label_prop is None
    m.define_model(m.classes)
    images, paths = unlabeled.images, list(unlabeled.filepaths)
    labels = [m.label_to_idx[c] for c in m.classes]
    emb, txt = m.trained_features(images, m.classes)
    _, probs, _, _ = engine.cosine_head(emb, txt.detach(), m.scale())
    idx, sim = engine.knn_graph(emb, k=4)
    z, _, mean, var, _ = engine.gmm_transduce(emb, probs, idx, sim, lam=2.0, iters=1, z_iters=1, var_floor=1e-8)
    n0 = len(calls())
    got = m.assign_pseudo_labels(K, unlabeled)
    assert calls()[n0:] == [(len(paths), len(labels), 1.0, 3)]
    _check_lists(got, z, labels, paths, 1.0, 3, "gmm")
    assert torch.equal(m.gmm_state[0], mean) and torch.equal(m.gmm_state[1], var)       # gmm_state keeps its meaning under the wrapper
    unlabeled.filepaths, unlabeled.labels = list(paths), None
    m.create_training_dataset(train, unlabeled)
    names = _pickles(tmp_path)
    assert len(names) == 1 and "_pseudolabels_ot_gmm_split_" in names[0], names


def test_switch_absent_changes_nothing(tmp_path, monkeypatch, calls):
    from grip_amd import engine, pseudolabels as pl
    monkeypatch.setenv("GRIP_PSEUDOLABEL_MODE", "f16")
    m, train, unlabeled = _strategy("TextualFPL", tmp_path, monkeypatch)
    assert m.balanced is None and m.transduction() is None
    m.define_model(m.classes)
    images, paths = unlabeled.images, list(unlabeled.filepaths)
    labels = [m.label_to_idx[c] for c in m.classes]
    emb, txt = m.trained_features(images, m.classes)
    _, probs, am_l, _ = engine.cosine_head(emb, txt.detach(), m.scale())
    want = pl.leaderboard(probs.cpu().numpy(), am_l.cpu().numpy(), paths, labels, K)       # the plain head -> scan
    plain = m.assign_pseudo_labels(K, unlabeled)
    assert (list(plain.filepaths), list(plain.labels)) == (list(want[0]), list(want[1])) and len(want[0]) > 0
    unlabeled.filepaths, unlabeled.labels = list(paths), None
    m.create_training_dataset(train, unlabeled)
    names = _pickles(tmp_path)
    assert calls() == [] and len(names) == 1 and "_ot_" not in names[0] and "_gmm_" not in names[0] and "_lp_" not in names[0], names
