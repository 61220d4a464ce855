"""CPU tests of the Gaussian discriminant head's references and plumbing (no GPU): the float64 references of tests/gda_ref.py equal naive loops at tiny
sizes; an f32 torch / numpy emulation of each step stays under its bound on every input of the GPU tests and a planted fault of four bounds is
rejected; the three head switches exclude each other and visual strategies ignore the new one; the head file round-trips; the ABI names are exported;
and the planted experiment of the README: the GDA head at alpha = 1 beats zero-shot and the diagonal variant on every seed at both shapes."""
import os
import types

import numpy as np
import pytest
import torch

import gda_ref as R


# ------------------------------------------------------------------------------------------ references against naive loops
def test_references_equal_naive_loops_at_tiny_sizes():
    F, y, r, mean = R.scatter_inputs(7, 3, 4, "weighted", seed=1)
    S = np.zeros((4, 4))
    for i in range(7):
        d = (F[i] - mean[int(y[i])]).double().numpy()       # one f32 rounding
        S += float(r[i]) * np.outer(d, d)
    assert np.allclose(R.scatter64(F, y, r, mean), S, rtol=1e-14, atol=0)
    a, a_scale, rhs = R.solve_inputs(4, 2, "scatter", seed=2)
    M, _ = R.spd_matrix64(a, a_scale, 0.5)
    A = a.double().numpy()
    s = float(np.float32(a_scale))
    naive = np.array([[s * A[max(i, j), min(i, j)] + (0.5 * s * sum(A[k, k] for k in range(4)) / 4 if i == j else 0.0) for j in range(4)] for i in range(4)])
    assert np.allclose(M, naive, rtol=1e-14, atol=0)
    x = R.solve64(a, a_scale, 0.5, rhs)
    assert np.allclose(M @ x.T, rhs.double().numpy().T, rtol=1e-10, atol=1e-13)
    f, w, bias, base, alpha = R.head_inputs(3, 2, 4, seed=3)
    al = float(np.float32(alpha))
    naive = np.array([[float(base[i, c]) + al * (sum(float(f[i, d]) * float(w[c, d]) for d in range(4)) / sum(float(f[i, d]) ** 2 for d in range(4)) ** 0.5
                                                  - float(bias[c])) for c in range(2)] for i in range(3)])
    assert np.allclose(R.head64(f, w, bias, alpha, base), naive, rtol=1e-13, atol=0)
    # fit64: three rows, two classes + an empty one, by hand
    F = torch.nn.functional.normalize(torch.tensor([[1.0, 0.2], [0.8, -0.1], [0.1, 1.0]]), dim=1)
    y = torch.tensor([0, 0, 2])
    mu, w, bias = R.fit64(F, y, None, 3, shrink=0.5)
    Fd = F.double().numpy()
    m0 = (Fd[0] + Fd[1]) / 2
    S = np.outer(Fd[0] - m0, Fd[0] - m0) + np.outer(Fd[1] - m0, Fd[1] - m0)
    A = S / 3 + 0.5 * np.trace(S) / (3 * 2) * np.eye(2)
    assert np.allclose(mu[0], m0) and (mu[1] == 0).all() and np.allclose(mu[2], Fd[2])
    assert np.allclose(w[0], np.linalg.solve(A, m0)) and (w[1] == 0).all() and bias[1] == 0 and np.isclose(bias[2], 0.5 * Fd[2] @ np.linalg.solve(A, Fd[2]))


# ------------------------------------------------------------------------------------------ emulations under the bounds, planted faults rejected
@pytest.mark.parametrize("case", R.S_CASES, ids=[R.case_id(c) for c in R.S_CASES])
def test_f32_emulation_of_the_scatter_stays_under_its_bound(case):
    n, c, e, kind = case
    F, y, r, mean = R.scatter_inputs(n, c, e, kind, seed=n * 1000 + c * 10 + e)
    S = R.emulate_scatter(F, y, r, mean)
    ratio = R.check_scatter(F, y, r, mean, S)
    assert ratio < 1
    if kind == "samerows":
        assert (S == 0).all()
    bound = R.scatter_bound(F, y, r, mean)
    i, j = np.unravel_index(bound.argmax(), bound.shape)
    bad = S.clone().double()
    bad[i, j] += 4 * bound[i, j]
    with pytest.raises(AssertionError, match="scatter"):
        R.check_scatter(F, y, r, mean, bad)


def test_scatter_cases_cover_what_the_kernel_branches_on():
    assert {c[0] for c in R.S_CASES} >= {1, 5, 255, 257, 549} and {c[1] for c in R.S_CASES} >= {1, 2, 65, 102}
    assert {c[2] for c in R.S_CASES} == {4, 64, 68, 192, 512} and {c[3] for c in R.S_CASES} == {"plain", "weighted", "empty", "samerows"}
    rows, slices = R.scatter_split(R.S_CASES[-1][0])
    assert rows == 2 * R.SCATTER_ROWS and slices == 9 and R.S_CASES[-1][0] % rows not in (0,), "more than one chunk per slice and a ragged last slice"
    assert R.scatter_split(257) == (256, 2) and R.scatter_split(256) == (256, 1) and R.scatter_split(50000)[1] <= R.SCATTER_SLICES
    F, y, r, mean = R.scatter_inputs(549, 65, 192, "empty", seed=0)
    assert not (y == 32).any() and (mean[32] == 0).all()
    assert float(R.scatter_inputs(5, 2, 4, "weighted", seed=0)[2][0]) == 0.0


@pytest.mark.parametrize("case", R.V_CASES, ids=[R.case_id(c) for c in R.V_CASES])
def test_f32_emulation_of_the_solve_passes_the_three_inequalities(case):
    e, c, ridge, kind = case
    a, a_scale, rhs = R.solve_inputs(e, c, kind, seed=e * 10 + c)
    x, L = R.emulate_solve(a, a_scale, ridge, rhs)
    ratios = R.check_solve(a, a_scale, ridge, rhs, x, L)
    assert max(ratios) < 1
    if e <= 132:       # planted faults: four bounds on one element of the factor, of the solution
        M, E = R.spd_matrix64(a, a_scale, ridge)
        Ld = L.double().numpy()
        fb = R.gamma(e + 1) * (np.abs(Ld) @ np.abs(Ld).T) + E
        badL = L.clone().double()
        badL[e - 1, e - 1] += 4 * fb[e - 1, e - 1] / (2 * abs(Ld[e - 1, e - 1])) + 4 * np.sqrt(fb[e - 1, e - 1])
        with pytest.raises(AssertionError, match="solve"):
            R.check_solve(a, a_scale, ridge, rhs, x, badL)
        x64 = R.solve64(a, a_scale, ridge, rhs)
        res = (R.gamma(3 * e + 1) * (np.abs(Ld) @ np.abs(Ld).T) + E) @ np.abs(x64).T
        sb = np.abs(np.linalg.inv(M)) @ res
        badx = x.clone().double()
        badx[0, 0] = x64[0, 0] + 4 * sb[0, 0]
        with pytest.raises(AssertionError, match="solve"):
            R.check_solve(a, a_scale, ridge, rhs, badx, L)


def test_solve_cases_cover_one_ragged_and_eight_panels():
    assert {c[0] for c in R.V_CASES} == {4, 64, 68, 132, 512} and {c[1] for c in R.V_CASES} == {1, 2, 65, 102}
    assert {c[2] for c in R.V_CASES if c[3] == "scatter"} == {1.0, 0.1} and any(c[3] == "diag" for c in R.V_CASES)


@pytest.mark.parametrize("case", R.H_CASES, ids=[R.case_id(c) for c in R.H_CASES])
def test_f32_emulation_of_the_head_stays_under_its_bound(case):
    n, c, e, mode = case
    f, w, bias, base, alpha = R.head_inputs(n, c, e, seed=n * 1000 + c * 10 + e)
    b = None if mode == "nobase" else base
    out = R.emulate_head(f, w, bias, alpha, b)
    assert R.check_head(f, w, bias, alpha, b, out) < 1
    bound = R.head_bound(f, w, bias, alpha, b)
    bad = out.clone().double()
    bad[n - 1, c - 1] += 4 * bound[n - 1, c - 1]
    with pytest.raises(AssertionError, match="head"):
        R.check_head(f, w, bias, alpha, b, bad)


def test_head_cases_cover_the_tile_edges():
    assert {(c[0], c[1]) for c in R.H_CASES} == {(n, c) for n in (1, 63, 65, 200) for c in (1, 64, 65, 102, 129)}
    assert {c[2] for c in R.H_CASES} == {4, 64, 512, 1024} and {c[3] for c in R.H_CASES} == {"nobase", "base", "inplace"}


# ------------------------------------------------------------------------------------------ plumbing
def _conf(**kw):
    return types.SimpleNamespace(MODALITY="text", VIS_ENCODER="ViT-B/16", DATASET_NAME="Synthetic", LEARNING_PARADIGM="ssl", MODEL="textual_fpl",
                                 OPTIM_SEED=1, SPLIT_SEED=500, **kw)


def _strategy(modality, **conf):
    import grip_amd  # noqa: F401
    from grip_amd.methods.training_strategies import TrainingStrategy
    s = object.__new__(TrainingStrategy)
    s.config = types.SimpleNamespace(**conf)
    s.modality = modality
    return s


def test_the_three_head_switches_exclude_each_other_and_visual_strategies_ignore_it():
    from grip_amd.methods.main import DEFAULTS
    assert "GDA_HEAD" not in DEFAULTS or DEFAULTS["GDA_HEAD"] is False
    assert not _strategy("text").gda_head() and not _strategy("text", GDA_HEAD=False).gda_head()
    assert _strategy("text", GDA_HEAD=True).gda_head() and _strategy("text", GDA_HEAD=True, TIP_ADAPTER=False, CLIP_ADAPTER=False).gda_head()
    for modality in ("image", "multi"):
        assert not _strategy(modality, GDA_HEAD=True).gda_head()
        assert not _strategy(modality, GDA_HEAD=True, TIP_ADAPTER=True).gda_head()      # both ignored there: nothing to refuse
    for other in ("TIP_ADAPTER", "CLIP_ADAPTER"):
        with pytest.raises(ValueError, match="GDA_HEAD, TIP_ADAPTER and CLIP_ADAPTER"):
            _strategy("text", GDA_HEAD=True, **{other: True}).gda_head()
    with pytest.raises(ValueError, match="CLIP_ADAPTER and TIP_ADAPTER"):
        _strategy("text", CLIP_ADAPTER=True, TIP_ADAPTER=True).clip_adapter()
    assert _strategy("text", TIP_ADAPTER=True).tip_adapter() and not _strategy("text", TIP_ADAPTER=True).gda_head()


def test_gda_file_round_trips(tmp_path, monkeypatch):
    import grip_amd  # noqa: F401
    from grip_amd.models import GdaHeadModel
    from grip_amd.utils import compute_metrics as cm, gda_head_path
    monkeypatch.chdir(tmp_path)
    conf = _conf()
    g = torch.Generator().manual_seed(3)
    m = GdaHeadModel(torch.randn(5, 8, generator=g), torch.randn(5, 8, generator=g), torch.randn(5, generator=g), 5, alpha=0.3)
    prompt = [torch.zeros(1, 4, 8).numpy()]
    plain = cm.save_parameters(prompt, conf, iteration=3)
    with open(plain, "rb") as f:
        plain_bytes = f.read()
    fn = cm.save_parameters(prompt, conf, iteration=3, gda=m)
    path = gda_head_path(conf, 3)
    assert fn == plain and path == fn[:-len(".pickle")] + "_gda.pickle"
    assert sorted(os.listdir("trained_prompts")) == sorted([os.path.basename(fn), os.path.basename(path)])
    with open(fn, "rb") as f:
        assert f.read() == plain_bytes      # the prompt file is what it is without the head
    back = GdaHeadModel.load(path)
    assert torch.equal(back.mean, m.mean) and torch.equal(back.w, m.w) and torch.equal(back.bias, m.bias) and (back.n_class, back.alpha) == (5, 0.3)
    assert sorted(m.state()) == ["alpha", "bias", "mean", "n_class", "w"]
    cm.save_parameters(prompt, conf)      # no head: the prompt file alone
    assert not os.path.exists(gda_head_path(conf))
    with pytest.raises(ValueError):
        GdaHeadModel(torch.zeros(5, 8), torch.zeros(4, 8), torch.zeros(5), 5)


def test_fit_validates_its_labels_on_the_host():
    import grip_amd  # noqa: F401
    from grip_amd.models import GdaHeadModel
    f = torch.randn(4, 8)
    for labels in ([0, 1, 2, 3], [0, -1, 0, 0], [0.0, 1.0, 0.0, 1.0]):
        with pytest.raises(ValueError):
            GdaHeadModel.fit(f, labels, [False] * 4, 3)
    with pytest.raises(ValueError):
        GdaHeadModel.fit(f, [0, 1, 2], [False] * 4, 3)


def test_abi_names_are_exported_with_their_signatures():
    import ctypes

    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    names = ("grip_class_scatter", "grip_spd_solve", "grip_linear_head")
    for n in names:
        assert n in native.EXPORTS and n + "_workspace" in native.EXPORTS
        assert getattr(native.lib(), n) is not None
    lib = native.lib()
    assert len(lib.grip_class_scatter.argtypes) == 11 and len(lib.grip_spd_solve.argtypes) == 12
    assert len(lib.grip_linear_head.argtypes) == 13 and native.ABI_VERSION == 9
    lib, nbytes = native.lib(), ctypes.c_size_t()
    # the workspace calls need no device; the scatter's is bounded by a constant x e^2 floats whatever n is
    native.check(lib.grip_class_scatter_workspace(50000, 102, 512, ctypes.byref(nbytes)))
    big = nbytes.value
    native.check(lib.grip_class_scatter_workspace(5000000, 102, 512, ctypes.byref(nbytes)))
    assert nbytes.value == big == engine.GDA_SCATTER_SLICES * 512 * 512 * 4 + 256
    native.check(lib.grip_class_scatter_workspace(257, 102, 512, ctypes.byref(nbytes)))
    assert nbytes.value == 2 * 512 * 512 * 4 + 256
    assert (engine.GDA_SCATTER_ROWS, engine.GDA_SCATTER_SLICES) == (R.SCATTER_ROWS, R.SCATTER_SLICES)
    native.check(lib.grip_spd_solve_workspace(512, 102, ctypes.byref(nbytes)))
    assert nbytes.value >= 2 * (512 + 102) * 512 * 4
    assert lib.grip_spd_solve_workspace(1028, 102, ctypes.byref(nbytes)) == 1 and b"e = 1028" in lib.grip_last_error()
    assert lib.grip_linear_head_workspace(5, 0, 16, ctypes.byref(nbytes)) == 1 and b"c = 0" in lib.grip_last_error()


# ------------------------------------------------------------------------------------------ the planted experiment (README)
@pytest.mark.parametrize("shape", R.PLANTED_SHAPES, ids=[f"C{c}-e{e}" for c, e in R.PLANTED_SHAPES])
def test_planted_pool_gda_beats_zero_shot_and_the_diagonal_variant(shape):
    """A planted pool, not a dataset (see R.planted_pool); float64 on the CPU.  Only the ordering is asserted; the accuracies are printed (README)."""
    C, e = shape
    for seed in R.PLANTED_SEEDS:
        acc = R.planted_accuracies(C, e, seed)
        print(f"planted C = {C}, e = {e}, seed {seed}: zero-shot {acc['zero_shot']:.3f}, GDA alpha=1 {acc['gda']:.3f}, diagonal {acc['diagonal']:.3f}, "
              f"GDA alpha=3 {acc['gda3']:.3f}")
        assert acc["gda"] > acc["zero_shot"] and acc["gda"] > acc["diagonal"], (seed, acc)
