"""The float64 reference and bound of tests/soft_ce_ref.py on the host (CPU): the reference equals an independent oracle (torch.nn.functional.cross_entropy
on probability targets with label_smoothing, torch.autograd for the gradient); sharpening is monotone in the temperature and the one-hot is its limit
T -> 0; an f32 emulation of the kernel stays under the derived bound on the GPU tests' own operands (and a planted fault of four bounds does not), so the
bound is honest before a GPU sees it; a float64 planted experiment trains a linear head on the hard labels and on the soft rows of a propagated matrix
and records both accuracies; the ABI lists the call and its argument checks need no device."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import knn_ref
import sinkhorn_ref
import soft_ce_ref as R
from conftest import REPO, write_report


def _oracle(x, lab, w, soft, row, cmap, inv_t, eps):
    """(per-row CE [n], grad [n, c], probability targets [n, c]) from torch's own cross-entropy in float64: the sharpened rows are built from
    torch.softmax / torch.pow (not from the reference's code), label_smoothing is torch's."""
    n, c = x.shape
    inv_t = float(torch.tensor(inv_t, dtype=torch.float32))
    eps = float(torch.tensor(eps, dtype=torch.float32))
    valid = (lab >= 0) & (lab < c)
    t = torch.zeros(n, c, dtype=torch.float64)
    t[valid, lab.long()[valid]] = 1.0
    is_soft = (row >= 0) & (row < soft.shape[0])
    for i in torch.nonzero(is_soft).flatten().tolist():
        z = soft[row[i]].double().clamp_min(R.TINY)
        t[i] = 0.0
        t[i, cmap.long()] = torch.softmax(inv_t * z.log(), dim=0)
    xd = x.double().requires_grad_(True)
    ce = F.cross_entropy(xd, t, reduction="none", label_smoothing=eps)
    (w.double() * ce).sum().backward()
    return ce.detach(), xd.grad, t, is_soft, valid


@pytest.mark.parametrize("n,c", [(5, 1), (5, 65), (67, 102), (67, 300)])
@pytest.mark.parametrize("temperature,eps", R.SETTINGS)
def test_reference_equals_torch_cross_entropy_on_probability_targets(n, c, temperature, eps):
    for cz in R.czs(c):
        x, lab, w, soft, row, cmap = R.operands(n, c, cz)
        inv_t = R.inv_temperature(temperature)
        ref = R.soft_ce64(x, lab, w, soft, row, cmap, inv_t, eps)
        ce, grad, t, is_soft, valid = _oracle(x, lab, w, soft, row, cmap, inv_t, eps)
        counted = (w != 0) & (is_soft | valid)
        assert torch.equal(counted, ref["counted"]) and torch.equal(is_soft, ref["is_soft"])
        assert torch.allclose(ref["term"][counted], (w.double() * ce)[counted], rtol=1e-11, atol=1e-12)
        assert torch.allclose(ref["loss"], (w.double() * ce)[counted].sum(), rtol=1e-11, atol=1e-12)
        smoothed = (1 - float(torch.tensor(eps, dtype=torch.float32))) * t + float(torch.tensor(eps, dtype=torch.float32)) / c
        assert torch.allclose(ref["target"], smoothed, rtol=1e-12, atol=1e-300)
        keeps_rule = ~is_soft & ~valid                      # a label outside [0, c): the whole softmax stays (grip_weighted_ce's rule), torch knows no such row
        assert torch.allclose(ref["grad"][~keeps_rule], grad[~keeps_rule], rtol=1e-10, atol=1e-13)
        p = torch.softmax(x.double(), dim=1)
        assert torch.allclose(ref["grad"][keeps_rule], (w.double()[:, None] * (p - smoothed))[keeps_rule], rtol=1e-12, atol=1e-15)
        if n == 67:
            assert keeps_rule.any() and (is_soft & ~valid).any() and (w == 0).any() and (soft[row[is_soft].long()] == 0).all(1).any()


def test_hard_rows_are_the_weighted_ce_reference():
    import head_ref
    x, lab, w, *_ = R.operands(67, 102, 102)
    ref = R.soft_ce64(x, lab, w)
    (loss, e_loss), (grad, e_grad) = head_ref.weighted_ce(x, lab, w)
    assert torch.allclose(ref["loss"], loss, rtol=1e-13) and torch.allclose(ref["grad"], grad, rtol=1e-13, atol=1e-300)
    assert ref["e_loss"] >= e_loss and (ref["e_grad"] >= e_grad).all()        # the shorter sequence's bound lies inside this one


def test_sharpening_is_monotone_in_the_temperature_and_one_hot_in_the_limit():
    z = R.matrix(102, seed=3)[4:]                                                  # (the plain rows: no zeros, not saturated)
    top = z.argmax(1)
    assert ((z == z.max(1, keepdim=True).values).sum(1) == 1).all()              # rows with a unique maximum
    last_top, last_entropy = None, None
    for temperature in (4.0, 2.0, 1.0, 0.5, 0.25, 0.1):
        s, _ = R.sharpen64(z, 1.0 / temperature)
        assert torch.allclose(s.sum(1), torch.ones(len(s), dtype=torch.float64), rtol=1e-13)
        assert torch.equal(s.argmax(1), top)
        peak = s.max(1).values
        entropy = -(s * s.clamp_min(1e-300).log()).sum(1)
        if last_top is not None:
            assert (peak > last_top).all() and (entropy < last_entropy).all()   # a lower temperature: a higher peak, a lower entropy, on every row
        last_top, last_entropy = peak, entropy
    s1, _ = R.sharpen64(z, 1.0)
    assert torch.allclose(s1, z.double() / z.double().sum(1, keepdim=True), rtol=1e-12, atol=1e-300)       # T = 1: the row itself, renormalised
    s0, _ = R.sharpen64(z, 1.0 / 1e-3)
    clear = z.topk(2, dim=1).values[:, 1] <= 0.9 * z.max(1).values                                         # the runner-up at 0.9 of the maximum at most:
    assert clear.sum() >= 3                                                                               # 0.9 ^ 1000 < 1e-45 is left of it at T = 1e-3
    assert torch.allclose(s0[clear], F.one_hot(top, z.shape[1]).double()[clear], rtol=0, atol=1e-40)      # T -> 0: the one-hot
    zero, _ = R.sharpen64(torch.zeros(2, 7), 2.0)
    assert torch.equal(zero, torch.full((2, 7), 1.0 / 7, dtype=torch.float64))                            # an all-zero row: uniform


# ------------------------------------------------------------------------------------------ the bound holds for an f32 emulation
@pytest.mark.parametrize("n,c", R.SHAPES, ids=[f"{n}x{c}" for n, c in R.SHAPES])
def test_f32_emulation_stays_under_the_bound(n, c):
    for cz in R.czs(c):
        ops = R.operands(n, c, cz)
        for temperature, eps in R.SETTINGS:
            inv_t = R.inv_temperature(temperature)
            loss, grad, target = R.soft_ce_f32(*ops, inv_t, eps)
            assert R.check(R.soft_ce64(*ops, inv_t, eps), loss, grad, target) <= 1.0
    ops = R.operands(n, c, c)[:3]
    loss, grad, target = R.soft_ce_f32(*ops)
    assert R.check(R.soft_ce64(*ops), loss, grad, target) <= 1.0


def test_checker_rejects_an_element_off_by_four_bounds():
    ops = R.operands(67, 102, 101)
    inv_t = R.inv_temperature(0.5)
    ref = R.soft_ce64(*ops, inv_t, 0.1)
    loss, grad, target = R.soft_ce_f32(*ops, inv_t, 0.1)
    assert R.check(ref, loss, grad, target) <= 1.0
    for name, t, at in (("loss", loss, ()), ("grad", grad, (2, 17)), ("target", target, (0, int(ops[5][3])))):
        bad = t.clone()
        bad[at] = (bad[at].double() + 4 * ref["e_" + name][at] + 1e-6 * bad[at].abs().double() + 1e-30).float()
        args = {"loss": loss, "grad": grad, "target": target, name: bad}
        with pytest.raises(AssertionError, match=f"soft_ce: .{name} - "):
            R.check(ref, args["loss"], args["grad"], args["target"])


# ------------------------------------------------------------------------------------------ what the soft targets are for
PLANTED_SEEDS = (0, 1, 2)       # the first three seeds, chosen before anything was run; every one is recorded


def _planted(seed, n=2000, c=20, e=32, n_test=2000, spread=0.2):
    """A pool of unit features around c class centres (noise of about the centre's own norm: 0.2 sqrt(32)), a head that is right about the images and
    wrong about the marginal (sinkhorn_ref.planted_pool: its noise does not depend on the features), and the head's probabilities propagated over the
    pool's own kNN graph (knn_ref.propagate64 with the strategy's defaults: k 16, alpha 0.8, gamma 10, 10 steps)."""
    g = torch.Generator().manual_seed(1000 + seed)
    centres = F.normalize(torch.randn(c, e, generator=g, dtype=torch.float64), dim=1)
    p, labels = sinkhorn_ref.planted_pool(n, c, seed=seed)
    feats = F.normalize(centres[labels] + spread * torch.randn(n, e, generator=g, dtype=torch.float64), dim=1)
    test_labels = torch.arange(n_test) % c
    test = F.normalize(centres[test_labels] + spread * torch.randn(n_test, e, generator=g, dtype=torch.float64), dim=1)
    cos = feats @ feats.T
    cos.fill_diagonal_(-2.0)
    sim, idx = cos.topk(16, dim=1)
    z, _ = knn_ref.propagate64(p, idx, sim.float(), 0.8, 10.0, 10)
    return feats, labels, test, test_labels, p, z


def _train_head(feats, targets, steps=300, lr=2.0, scale=10.0):
    """A linear head from zeros, full-batch gradient descent on the mean cross-entropy against `targets` [n, c] in float64."""
    w = torch.zeros(targets.shape[1], feats.shape[1], dtype=torch.float64)
    for _ in range(steps):
        g = (torch.softmax(scale * feats @ w.T, dim=1) - targets) / feats.shape[0]
        w -= lr * scale * g.T @ feats
    return w


def test_planted_pool_soft_rows_against_hard_labels():
    """Both heads start from the same noisy pool: one trains on onehot(arg-max Z) of every row, the other on the row of Z itself (temperature 1,
    sharpen64).  Seen in float64 on the CPU, held-out accuracy hard -> soft: seed 0  0.626 -> 0.615, seed 1  0.143 -> 0.527, seed 2  0.616 -> 0.663
    (tests/_out/soft_ce_planted.json keeps every figure).  Where the propagation helped the arg-max (seeds 0 and 2: 0.44 -> 0.62, 0.45 -> 0.62 on the pool) the
    two heads are within five points of each other, either way round; where it amplified the head's biased marginal (seed 1: 0.27 -> 0.13) the hard
    labels pass the damage on and the soft rows keep what the head knew.  Asserted: what these runs showed, no more."""
    report = {}
    for seed in PLANTED_SEEDS:
        feats, labels, test, test_labels, p, z = _planted(seed)
        c = z.shape[1]
        acc = {"head_argmax_on_pool": float((p.argmax(1) == labels).double().mean()), "propagated_argmax_on_pool": float((z.argmax(1) == labels).double().mean())}
        for name, targets in (("hard", F.one_hot(z.argmax(1), c).double()), ("soft", R.sharpen64(z, 1.0)[0])):
            w = _train_head(feats, targets)
            acc[name + "_pool"] = float(((feats @ w.T).argmax(1) == labels).double().mean())
            acc[name + "_held_out"] = float(((test @ w.T).argmax(1) == test_labels).double().mean())
        report[f"seed_{seed}"] = acc
        print(f"planted 2000 x 20, seed {seed}: {acc}")
        assert acc["soft_held_out"] >= acc["hard_held_out"] - 0.05
    write_report("soft_ce_planted.json", report)
    assert report["seed_1"]["propagated_argmax_on_pool"] < report["seed_1"]["head_argmax_on_pool"]
    assert report["seed_1"]["soft_held_out"] >= report["seed_1"]["hard_held_out"] + 0.3


# ------------------------------------------------------------------------------------------ plumbing
def test_abi_lists_the_entry_point_and_its_checks_need_no_device():
    import grip_amd  # noqa: F401
    from grip_amd import native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "grip_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(grip_[a-z_0-9]+)\s*\(", text))
    assert "grip_soft_ce" in declared and "grip_soft_ce" in native.EXPORTS and native.ABI_VERSION == 9
    lib = native.lib()
    one = 1        # (any non-null address: the checks below fail before anything is read)
    for args, word in (((None, one, one, 5, 2, None, 0, 0, None, None, 1.0, 0.0, one), "null pointer"),
                       ((one, one, one, 0, 2, None, 0, 0, None, None, 1.0, 0.0, one), "n = 0"),
                       ((one, one, one, 5, 0, None, 0, 0, None, None, 1.0, 0.0, one), "c = 0"),
                       ((one, one, one, 5, 2, None, 0, 0, None, None, 0.0, 0.0, one), "inv_temperature = 0"),
                       ((one, one, one, 5, 2, None, 0, 0, None, None, float("nan"), 0.0, one), "inv_temperature = nan"),
                       ((one, one, one, 5, 2, None, 0, 0, None, None, 1.0, 1.0, one), "smoothing = 1"),
                       ((one, one, one, 5, 2, one, 3, 3, one, one, 1.0, 0.0, one), "cz = 3"),
                       ((one, one, one, 5, 2, one, 3, 1, None, one, 1.0, 0.0, one), "null pointer"),
                       ((one, one, one, 5, 20000, one, 3, 5, one, one, 1.0, 0.0, one), "at most 16000")):
        rc = lib.grip_soft_ce(*args, None, None, None)
        assert rc == 1 and word in lib.grip_last_error().decode(), (args, lib.grip_last_error().decode())
