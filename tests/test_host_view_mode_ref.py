"""CPU: the float64 reference and the bound of tests/view_mode_ref.py hold water before any GPU is involved -- an f32 emulation of the recursion (torch's
own summation orders, no fused multiply-add) stays inside the derived bound on every case the GPU test runs, the vectorised float64 recursion agrees with
a plain-loop restatement, GENTLE keeps the bound non-vacuous for a whole run, and the planted pool of the issue is written out (all four columns
reported; the one assertion is mode > single view on each seed)."""
import pytest
import torch

import view_mode_ref as R


@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_f32_emulation_stays_inside_the_bound(case):
    f, s = R.case_inputs(case)
    for params in (dict(R.DEFAULTS, outer=0), dict(R.DEFAULTS, outer=1, inner=1), R.DEFAULTS, R.GENTLE):
        mode, y, h2 = R.run_f32(f, s, **params)
        worst, vac = R.check_run(f, s, params, None, None, mode, y, h2)
        print(f"f32 emulation {R.case_id(case)} outer {params['outer']} inner {params['inner']}: worst |err| / bound = {worst:.3f}, vacuous share {vac:.3f}")
    # the forced single steps of the GPU test: from every state of the float64 trajectory under the defaults
    states = R.run64(f, s, trajectory=True, **R.DEFAULTS)[-1]
    one = dict(R.DEFAULTS, outer=1, inner=1)
    for m0, y0 in states:
        mode, y, h2 = R.run_f32(f, s, mode_in=m0, y_in=y0, **one)
        worst, vac = R.check_run(f, s, one, m0, y0, mode, y, h2)
        assert worst <= 1.0


@pytest.mark.parametrize("case", [c for c in R.CASES if c[4] in ("plain", "outlier")], ids=R.case_id)
def test_gentle_parameters_keep_the_bound_non_vacuous(case):
    f, s = R.case_inputs(case)
    m64, _, _, bm, by, _ = R.run64(f, s, **R.GENTLE)
    assert R.vacuous_share(m64, bm, by) == 0.0
    assert float(by.max()) < 1e-2 and float(bm.max()) < 1e-2, (float(by.max()), float(bm.max()))      # it still says something: y and m to two digits at least


@pytest.mark.parametrize("c", [5, None])
def test_float64_recursion_agrees_with_plain_loops(c):
    f, s = R.inputs(2, 5, 64, c, "outlier", seed=3)
    m64, y64, h64 = R.run64(f, s, **R.DEFAULTS)[:3]
    m, y, h2 = (torch.tensor(x, dtype=torch.float64) for x in R.run_loops(f, s, **R.DEFAULTS))
    assert (m - m64).abs().max() < 1e-12 and (y - y64).abs().max() < 1e-12 and (h2 - h64).abs().max() < 1e-12


def test_outer_zero_returns_the_start_state():
    f, s = R.inputs(2, 5, 64, 5, "plain", seed=4)
    m64, y64 = R.run64(f, s, **dict(R.DEFAULTS, outer=0))[:2]
    u0 = f[:, 0].double() / f[:, 0].double().norm(dim=1, keepdim=True)
    assert torch.equal(m64, u0) and torch.equal(y64, torch.full((2, 5), 0.2, dtype=torch.float64))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_pool_mode_beats_the_single_view(seed):
    """A planted pool, not a dataset: 2 000 images, 20 classes, e = 64, V = 16, half the views of an image miss, view 0 is clean, imperfect text."""
    a = R.planted_accuracies(seed)
    print(f"planted pool seed {seed}: single view {a['single']:.3f}, mean of the unit view embeddings {a['mean_embedding']:.3f}, "
          f"the mode {a['mode']:.3f}, mean of the views' probabilities {a['mean_probability']:.3f}")
    assert a["mode"] > a["single"]
