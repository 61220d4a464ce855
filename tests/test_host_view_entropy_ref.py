"""CPU: the float64 reference and the bounds of tests/view_entropy_ref.py hold water before any GPU is involved -- the reference agrees with float64 torch
autograd on the paper's formulation written independently, an f32 emulation of the kernel's operation order stays inside the derived bounds at every
shape the GPU test runs (and its selection, like the float64 one, satisfies the selection statement), and the planted pool of the issue is written out:
its figures are reproduced, no ranking is asserted."""
import numpy as np
import pytest
import torch

import view_entropy_ref as R


def _paper(x, sel, keep):
    """The paper's formulation in float64 torch with autograd: per image logsumexp_p(log_softmax(x_p)) - log keep over the selected views, its entropy;
    the mean over the images.  Returns (loss, grad [n, v, c])."""
    xt = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    total = 0.0
    for i in range(xt.shape[0]):
        lp = torch.log_softmax(xt[i][torch.tensor(np.flatnonzero(sel[i]))], dim=1)
        avg = torch.logsumexp(lp, dim=0) - float(np.log(keep))
        total = total - (avg.exp() * avg).sum()
    loss = total / xt.shape[0]
    loss.backward()
    return float(loss.detach()), xt.grad.numpy()


@pytest.mark.parametrize("kind", ["normal", "duplicates", "uniform"])
@pytest.mark.parametrize("n,v,c", [(1, 1, 5), (3, 5, 63), (2, 16, 102), (1, 64, 102), (3, 17, 1000)])
def test_reference_agrees_with_autograd_on_the_papers_formulation(kind, n, v, c):
    x = R.logits(kind, n, v, c, seed=1)
    for keep in R.keeps(v):
        ref = R.run64(x, keep)
        loss, grad = _paper(x, ref["sel"], keep)
        tol = R.agree_rel(keep, c)
        assert abs(loss - ref["loss"]) <= tol * ref["lscale"] + 1e-300, (keep, loss, ref["loss"])
        assert (np.abs(grad - ref["grad"]) <= tol * ref["gscale"] + 1e-300).all(), keep
        assert (grad[~ref["sel"]] == 0).all() and (ref["grad"][~ref["sel"]] == 0).all()


def test_gradient_on_a_given_selection_is_that_selections_gradient():
    x = R.logits("normal", 2, 5, 7, seed=2)
    sel = np.array([[0, 1, 0, 0, 1], [1, 0, 0, 1, 0]], dtype=bool)      # not the float64 selection: any selection is a constant of the gradient
    ref = R.run64(x, 2, selection=sel)
    loss, grad = _paper(x, sel, 2)
    tol = R.agree_rel(2, 7)
    assert abs(loss - ref["loss"]) <= tol * ref["lscale"] and (np.abs(grad - ref["grad"]) <= tol * ref["gscale"]).all()


def test_selection_order():
    H = np.array([0.5, np.nan, 0.25, 0.5, np.inf, 0.25])
    assert R.select(H, 1).tolist() == [False, False, True, False, False, False]      # ties to the lower index
    assert R.select(H, 3).tolist() == [True, False, True, False, False, True]
    assert R.select(H, 5).tolist() == [True, True, True, True, False, True]          # a non-finite entropy after every finite one, index ascending


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n", R.NS)
def test_f32_emulation_stays_inside_the_bounds(kind, n):
    """Every shape of the GPU test (the case at the c limit: below)."""
    worst = {}
    for case in R.cases():
        if case[0] != kind or case[1] != n or case[3] == R.C_LIMIT:
            continue
        _, _, v, c = case
        x = R.logits(*case)
        for keep in R.keeps(v):
            got = R.run_f32(x, keep)
            R.check_selection(x, keep, got["sel"])
            R.check_selection(x, keep, R.run64(x, keep)["sel"])      # the inputs keep the float64 reference itself inside the statement
            for k, r in R.worst_ratios(got, x, keep).items():
                worst[k] = max(worst.get(k, 0.0), r)
            if v == keep == 1:
                ref = R.run64(x, 1)
                assert (np.abs(got["loss_i"].astype(np.float64) - ref["H"][:, 0]) <= ref["bloss_i"] + ref["bH"][:, 0]).all()
    print(f"f32 emulation {kind} n = {n}: worst |err| / bound " + ", ".join(f"{k} {r:.3f}" for k, r in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, worst


def test_f32_emulation_at_the_class_limit():
    case = R.cases()[-1]
    assert case[3] == R.C_LIMIT
    x = R.logits(*case)
    for keep in R.keeps(case[2]):
        got = R.run_f32(x, keep)
        R.check_selection(x, keep, got["sel"])
        worst = R.worst_ratios(got, x, keep)
        assert max(worst.values()) <= 1.0, worst


def test_saturated_pools_exercise_the_floor():
    x = R.logits("saturated", 1, 5, 1000)
    ref = R.run64(x, 1)
    assert (ref["mean"] < R.TINY).any() and np.isfinite(ref["grad"]).all() and np.isfinite(ref["loss"])


# the planted pool (a planted pool, not a dataset), float64, seeds 0 / 1 / 2: single view, mean of the views' probabilities, MTA mode, TPT (rho 0.5)
PLANTED = {0: (0.5485, 0.8895, 0.8680, 0.5805), 1: (0.5445, 0.9075, 0.8770, 0.5775), 2: (0.5340, 0.8720, 0.8385, 0.5590)}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_pool_figures_are_reproduced(seed):
    """No ranking is asserted: the figures are written out and must be the recorded ones, to two images of the 2 000 (an arg-max between two classes a
    rounding apart may fall either way on another host's float64 matrix products)."""
    a = R.planted_accuracies(seed)
    print(f"planted pool seed {seed}: single view {a['single']:.4f}, mean of the views' probabilities {a['mean_probability']:.4f}, "
          f"MTA mode {a['mode']:.4f}, TPT {a['tpt']:.4f}")
    got = (a["single"], a["mean_probability"], a["mode"], a["tpt"])
    assert all(abs(g - w) <= 2 / 2000 + 1e-12 for g, w in zip(got, PLANTED[seed])), (got, PLANTED[seed])
