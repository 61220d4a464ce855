"""The references of tests/candidate_ref.py against independent oracles on the host: the float64 loss and gradient against torch.autograd on
-log sum_S softmax, the algebra of the sets, the f32 emulation inside the derived bound, and the planted experiment behind the feature."""
import numpy as np
import pytest
import torch

import candidate_ref as R


def _autograd(x, lab, w, cand, row, cmap):
    """(loss, grad) in float64 by autograd: hard rows w CE(x, label), candidate rows -w log sum_S softmax(x), empty sets and bad labels left out."""
    n, c = x.shape
    xr = x.double().clone().requires_grad_(True)
    is_cand, member = R.members(cand, row, cmap, n, c)
    logp = torch.log_softmax(xr, dim=-1)
    total = xr.sum() * 0
    for i in range(n):
        if bool(is_cand[i]):
            if bool(member[i].any()):
                total = total + w[i].double() * -torch.log(torch.exp(logp[i][member[i]]).sum())
        elif 0 <= int(lab[i]) < c:
            total = total + w[i].double() * -logp[i, int(lab[i])]
        else:
            total = total + (w[i].double() * torch.softmax(xr[i], -1).detach() * xr[i]).sum() * 0      # (weighted_ce's rule is checked below)
    total.backward()
    return total.detach(), xr.grad


@pytest.mark.parametrize("n,c", [(5, 1), (5, 65), (67, 102), (4, 300)])
def test_reference_matches_autograd(n, c):
    for cz in R.czs(c):
        x, lab, w, cand, row, cmap = R.operands(n, c, cz)
        ref = R.candidate_ce64(x, lab, w, cand, row, cmap)
        loss, grad = _autograd(x, lab, w, cand, row, cmap)
        assert torch.allclose(ref["loss"], loss, rtol=1e-12, atol=1e-12)
        in_range = ((lab >= 0) & (lab < c)) | ref["is_cand"]
        assert torch.allclose(ref["grad"][in_range], grad[in_range], rtol=1e-11, atol=1e-13)
        out = ~in_range                                     # a hard row with a label outside [0, c): the whole softmax stays
        assert torch.allclose(ref["grad"][out], (w[out].double()[:, None] * torch.softmax(x[out].double(), -1)), rtol=1e-12, atol=1e-15)
        assert bool(ref["empty"].any()) or n < 3


def test_f32_emulation_is_inside_the_bound():
    for n, c in R.SHAPES:
        for cz in R.czs(c):
            ops = R.operands(n, c, cz)
            loss, grad = R.candidate_ce_f32(*ops)
            R.check(R.candidate_ce64(*ops), loss, grad)


def test_singleton_is_cross_entropy_full_is_zero_empty_is_nothing():
    n, c = 6, 33
    g = torch.Generator().manual_seed(3)
    x = (3 * torch.randn(n, c, generator=g)).float()
    w = (0.5 + torch.rand(n, generator=g)).float()
    y = torch.randint(0, c, (n,), generator=g).to(torch.int32)
    cmap = torch.arange(c, dtype=torch.int32)
    rows = torch.arange(n, dtype=torch.int32)
    single = np.zeros((n, c), dtype=bool)
    single[np.arange(n), y.numpy()] = True
    ref = R.candidate_ce64(x, torch.full_like(y, -1), w, torch.from_numpy(R.pack(single).copy()), rows, cmap)
    hard = R.candidate_ce64(x, y, w)
    assert torch.allclose(ref["loss"], hard["loss"], rtol=1e-13) and torch.allclose(ref["grad"], hard["grad"], rtol=1e-12, atol=1e-15)
    ce = (w.double() * torch.nn.functional.cross_entropy(x.double(), y.long(), reduction="none")).sum()
    assert torch.allclose(hard["loss"], ce, rtol=1e-12)
    full = R.candidate_ce64(x, y, w, torch.from_numpy(R.pack(np.ones((n, c), dtype=bool)).copy()), rows, cmap)
    assert abs(float(full["loss"])) <= 1e-12 and float(full["grad"].abs().max()) <= 1e-15
    none = R.candidate_ce64(x, y, w, torch.zeros(n, R.words(c), dtype=torch.int32), rows, cmap)
    assert float(none["loss"]) == 0.0 and float(none["grad"].abs().max()) == 0.0 and not bool(none["counted"].any())


def test_cumsum_float32_is_the_sequential_sum():
    g = np.random.default_rng(5)
    for c in (1, 7, 102, 1024):
        p = np.sort(g.random(c).astype(np.float32))[::-1]
        s = np.float32(0)
        seq = []
        for v in p:
            s = np.float32(s + v)
            seq.append(s)
        assert np.array_equal(np.cumsum(p, dtype=np.float32), np.array(seq, dtype=np.float32))


@pytest.mark.parametrize("kind", R.SEL_KINDS)
def test_set_algebra(kind):
    n, c = 65, 33
    p = R.pool(n, c, kind)
    for claim in R.claims(n, c):
        for tau in R.SEL_TAUS:
            sets = {name: R.unpack(R.select(p, claim, tau, name)[0], c) for name in R.COMBINE}
            assert np.array_equal(sets["intersection"], sets["intra"] & sets["inter"]) and np.array_equal(sets["union"], sets["intra"] | sets["inter"])
            assert not (sets["intersection"] & ~sets["intra"]).any() and not (sets["inter"] & ~sets["union"]).any()
            assert sets["intra"][np.arange(n), R.select(p, claim, tau, "intra")[2]].all()        # rank 0 is always in
            assert (sets["inter"].sum(0) >= claim).all()                                         # every class claims at least `claim` rows (ties: more)
            for name in R.COMBINE:
                mask, count, label, thr = R.select(p, claim, tau, name)
                assert np.array_equal(R.pack(R.unpack(mask, c)), mask) and np.array_equal(count, sets[name].sum(1))
                assert ((label == -1) == (count == 0)).all()
                best = np.where(sets[name], p, -1).max(1)
                assert all(label[i] == -1 or (p[i, label[i]] == best[i] and not sets[name][i, :label[i]][p[i, :label[i]] == best[i]].any()) for i in range(n))


# ------------------------------------------------------------------------------------------ the planted experiment
# A planted pool, not a dataset.  Per seed: 20 unit class prototypes in 64 dimensions; 2 000 pool features proto[y] + 2.2 N(0, I) / sqrt(e), normalised (and
# 2 000 fresh ones for the held-out accuracy); text prototypes proto + 1.0 N(0, I) / sqrt(e), normalised; zero-shot logits 10 f . t_c + bias_c with
# bias ~ N(0, 1.5^2) -- a head biased for and against classes.  A residual linear head (logits + 10 f W^T + b) is trained from zero by the linear probe's
# recursion (_fit: 300 heavy-ball iterations, l2 = 0.1):
#   hard:       the product's leaderboard scan (an image competes on its arg-max board only; what does not make it spills onto the other classes'
#               boards), cross-entropy on the (row, class) pairs;
#   candidate:  R.select(probs, claim, tau = 0.99), -log sum_S softmax on every row with a non-empty set.
N_POOL, N_CLASSES, DIM = 2000, 20, 64


def _planted(seed):
    g = np.random.default_rng(seed)
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    proto = unit(g.standard_normal((N_CLASSES, DIM)))
    text = unit(proto + 1.0 * g.standard_normal((N_CLASSES, DIM)) / np.sqrt(DIM))
    bias = 1.5 * g.standard_normal(N_CLASSES)

    def draw():
        y = g.integers(0, N_CLASSES, N_POOL)
        f = unit(proto[y] + 2.2 * g.standard_normal((N_POOL, DIM)) / np.sqrt(DIM))
        return f, y, 10.0 * f @ text.T + bias

    return draw(), draw()


def _softmax(z):
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


SCALE, L2, MOMENTUM, ITERS = 10.0, 0.1, 0.9, 300


def _fit(f, base, target_of):
    """W, b of the head base + SCALE f W^T + b after ITERS heavy-ball iterations from zero, the linear probe's recursion (include/grip_amd.h, grip_probe_fit):
    G = L2 W + gw, m = MOMENTUM m + G, W -= lr m with lr = 1 / (1/2 (SCALE^2 + 1) + L2) on the mean loss.  target_of(p) -> the [rows, c] target the
    gradient p - target is taken against (a one-hot, or the model's own softmax over the set: the partial-label loss's moving target)."""
    W, b = np.zeros((N_CLASSES, DIM)), np.zeros(N_CLASSES)
    mW, mb = np.zeros_like(W), np.zeros_like(b)
    lr = 1.0 / (0.5 * (SCALE * SCALE + 1.0) + L2)
    for _ in range(ITERS):
        q = _softmax(base + SCALE * f @ W.T + b)
        d = (q - target_of(q)) / len(f)
        mW = MOMENTUM * mW + (L2 * W + SCALE * d.T @ f)
        mb = MOMENTUM * mb + d.sum(0)
        W, b = W - lr * mW, b - lr * mb
    return W, b


def _hard_lists(p, k):
    """The hard lists of the product's leaderboard scan (oracle/leaderboard.py), in pool order: an image competes on the board of its arg-max class; when it
    does not make that board it is offered to every other class's board with that class's probability."""
    board = [[] for _ in range(N_CLASSES)]

    def offer(c, score, i):
        if len(board[c]) < k:
            board[c].append((score, i))
            return True
        if board[c][-1][0] < score:
            board[c] = sorted(board[c] + [(score, i)], reverse=True)[:k]
            return True
        return False

    for i in range(len(p)):
        c = int(p[i].argmax())
        if len(board[c]) < k or board[c][-1][0] < p[i, c]:
            offer(c, float(p[i, c]), i)
        else:
            for j in np.argsort(-p[i], kind="stable"):
                if j != c:
                    offer(int(j), float(p[i, j]), i)
    rows = [i for b in board for _, i in b]
    labs = [c for c, b in enumerate(board) for _ in b]
    return np.array(rows), np.array(labs)


def planted_accuracies(seed, k=N_POOL // N_CLASSES, claim=N_POOL // N_CLASSES, tau=0.99):
    (f, y, z), (fh, yh, zh) = _planted(seed)
    p = _softmax(z).astype(np.float32)
    acc = lambda W, b: float(((zh + SCALE * fh @ W.T + b).argmax(1) == yh).mean())
    rows, labs = _hard_lists(p, k)
    onehot = np.eye(N_CLASSES)[labs]
    hard = acc(*_fit(f[rows], z[rows], lambda q: onehot))
    mask, count, _, _ = R.select(p, claim, tau)
    keep = count > 0
    member = R.unpack(mask, N_CLASSES)[keep].astype(np.float64)
    cand = acc(*_fit(f[keep], z[keep], lambda q: q * member / (q * member).sum(1, keepdims=True)))
    return dict(zero_shot=float((zh.argmax(1) == yh).mean()), hard=hard, candidate=cand, mean_set=float(count[keep].mean()),
                wrong_hard=float((y[rows] != labs).mean()))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_candidate_sets_beat_hard_lists(seed):
    r = planted_accuracies(seed)
    print(f"planted seed {seed}: zero-shot {r['zero_shot']:.3f}, hard top-K (K = 100) {r['hard']:.3f} ({r['wrong_hard']:.2f} of its labels wrong), "
          f"candidate sets (tau 0.99, claim 100, mean set size {r['mean_set']:.2f}) {r['candidate']:.3f}")
    assert r["candidate"] > r["hard"]
