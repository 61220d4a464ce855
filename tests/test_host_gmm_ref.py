"""The float64 references and bounds of tests/gmm_ref.py on the host (CPU): the vectorised references equal a naive loop form at tiny sizes; an f32
emulation of both steps stays under the derived bounds on the GPU tests' own inputs (and a planted fault of four bounds does not), so the bounds are
honest before a GPU sees them; and the plumbing of the switch: TransductiveGMM validates its settings, label_propagation() takes both classes and
nothing else, the pickle carries the installed object's infix, TRANSDUCTIVE_GMM and LABEL_PROPAGATION exclude each other, the ABI lists the four calls."""
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import gmm_ref as R
from conftest import REPO

NEW_EXPORTS = ("grip_gmm_mstep_workspace", "grip_gmm_mstep", "grip_gmm_estep_workspace", "grip_gmm_estep")


def _pl():
    import grip_amd  # noqa: F401
    from grip_amd import pseudolabels as pl
    return pl


# ------------------------------------------------------------------------------------------ references against the naive loops
def _naive_mstep(z, f, var_floor):
    n, c = len(z), len(z[0])
    e = len(f[0])
    cnt = [sum(z[i][j] for i in range(n)) for j in range(c)]
    mean = [[(sum(z[i][j] * f[i][d] for i in range(n)) / cnt[j]) if cnt[j] != 0 else 0.0 for d in range(e)] for j in range(c)]
    var = [max(var_floor, sum(z[i][j] * (f[i][d] - mean[j][d]) ** 2 for i in range(n) for j in range(c)) / n) for d in range(e)]
    return cnt, mean, var


def _naive_estep(f, mean, var, p, idx, sim, z, lam, z_iters):
    n, c, e, k = len(f), len(mean), len(var), len(idx[0])
    g = [[sum(f[i][d] * mean[j][d] / var[d] for d in range(e)) - 0.5 * sum(mean[j][d] ** 2 / var[d] for d in range(e)) for j in range(c)] for i in range(n)]
    for _ in range(z_iters):
        new = []
        for i in range(n):
            a = [g[i][j] + lam * math.log(max(p[i][j], R.TINY)) + sum(max(0.0, sim[i][t]) * z[idx[i][t]][j] for t in range(k)) for j in range(c)]
            m = max(a)
            x = [math.exp(v - m) for v in a]
            new.append([v / sum(x) for v in x])
        z = new
    return z


def test_references_equal_the_naive_loops():
    n, c, e, k = 7, 3, 8, 2
    z, f = R.mstep_inputs(n, c, e, "zerocol", seed=1)
    cnt, mean, var = R.mstep64(z, f, 0.04)
    ncnt, nmean, nvar = _naive_mstep(z.double().tolist(), f.double().tolist(), float(torch.tensor(0.04).float()))
    assert torch.allclose(cnt, torch.tensor(ncnt, dtype=torch.float64), rtol=1e-13, atol=0)
    assert torch.allclose(mean, torch.tensor(nmean, dtype=torch.float64), rtol=1e-12, atol=1e-300) and (mean[c // 2] == 0).all() and cnt[c // 2] == 0
    assert torch.allclose(var, torch.tensor(nvar, dtype=torch.float64), rtol=1e-12, atol=0)
    assert (var == float(torch.tensor(0.04).float())).any() and (var > 0.041).any()       # the floor binds in some dimensions only
    f, mu, v, p, idx, sim, z_in = R.estep_inputs(n, c, e, k, "zeroprob", seed=2)
    v = v * 30                                                                             # (soft assignments: every class keeps a visible share)
    for lam, zi in ((0.0, 1), (1.0, 3)):
        got, _ = R.estep64(f, mu, v, p, idx, sim, z_in, lam, zi)
        want = _naive_estep(f.double().tolist(), mu.double().tolist(), v.double().tolist(), p.double().tolist(), idx.tolist(), sim.double().tolist(),
                            z_in.double().tolist(), lam, zi)
        assert torch.allclose(got, torch.tensor(want, dtype=torch.float64), rtol=1e-9, atol=1e-300)
    assert (sim < 0).any() and (p == 0).any()


# ------------------------------------------------------------------------------------------ the bounds hold for an f32 emulation
@pytest.mark.parametrize("case", R.M_CASES, ids=[R.case_id(c) for c in R.M_CASES])
def test_mstep_f32_emulation_stays_under_the_bound(case):
    n, c, e, kind = case
    z, f = R.mstep_inputs(n, c, e, kind, seed=n * 1000 + c * 10 + e)
    cnt, mean, var = R.mstep_f32(z, f, 1e-8)
    assert R.check_mstep(z, f, 1e-8, cnt, mean, var) <= 1.0
    if kind == "zerocol":
        assert cnt[c // 2] == 0 and (mean[c // 2] == 0).all()
    if kind == "samerows":
        assert (var == torch.tensor(1e-8)).all()


def test_mstep_checker_rejects_an_element_off_by_four_bounds():
    z, f = R.mstep_inputs(257, 65, 64, "plain", seed=3)
    cnt, mean, var = R.mstep_f32(z, f, 1e-8)
    _, _, _, bc, bm, bv = R.mstep64(z, f, 1e-8, bounds=True)
    for name, t, b, at in (("count", cnt, bc, (7,)), ("mean", mean, bm, (7, 9)), ("var", var, bv, (9,))):
        bad = t.clone()
        bad[at] = (bad[at].double() + 4 * b[at]).float()
        args = {"count": cnt, "mean": mean, "var": var, name: bad}
        with pytest.raises(AssertionError, match=f"M-step: .{name} - "):
            R.check_mstep(z, f, 1e-8, args["count"], args["mean"], args["var"])


@pytest.mark.parametrize("case", R.E_CASES, ids=[R.case_id(c) for c in R.E_CASES])
def test_estep_f32_emulation_stays_under_the_bound(case):
    n, c, e, k, zi, lam, kind = case
    ops = R.estep_inputs(n, c, e, k, kind, seed=n * 1000 + c * 10 + k)
    z, pred = R.estep_f32(*ops, lam, zi)
    assert R.check_estep(*ops, lam, zi, z, pred) <= 1.0


def test_estep_checker_rejects_an_element_and_a_wrong_argmax():
    ops = R.estep_inputs(257, 102, 64, 3, "plain", seed=4)
    z, pred = R.estep_f32(*ops, 1.0, 2)
    z64, b = R.estep64(*ops, 1.0, 2)
    i, j = 100, int(z64[100].argmax())
    bad = z.clone()
    bad[i, j] = (bad[i, j].double() - 4 * b[i, j] - 1e-6).float()
    with pytest.raises(AssertionError, match="E-step: .Z - Z64."):
        R.check_estep(*ops, 1.0, 2, bad, None)
    wrong = pred.clone()
    wrong[3] = (wrong[3] + 1) % 102
    with pytest.raises(AssertionError, match="argmax_out"):
        R.check_estep(*ops, 1.0, 2, z, wrong)


# ------------------------------------------------------------------------------------------ plumbing
def test_transductive_gmm_defaults_and_validation():
    pl = _pl()
    t = pl.TransductiveGMM()
    assert (t.k, t.lam, t.iters, t.z_iters, t.var_floor, t.keep_graphs, t.state, t.infix) == (3, 1.0, 10, 5, 1e-8, False, None, "gmm_")
    pl.TransductiveGMM(k=32, lam=0.0, iters=1, z_iters=1, var_floor=1e-30, keep_graphs=True)
    for bad in (dict(k=0), dict(k=33), dict(lam=-0.1), dict(lam=float("inf")), dict(iters=0), dict(z_iters=0), dict(var_floor=0.0), dict(var_floor=-1.0),
                dict(var_floor=float("inf"))):
        with pytest.raises(ValueError, match="TransductiveGMM"):
            pl.TransductiveGMM(**bad)
    assert issubclass(pl.TransductiveGMM, pl._PoolGraph) and issubclass(pl.LabelPropagation, pl._PoolGraph)      # one graph-keeping, not two
    assert pl.LabelPropagation().infix == "lp_"


def test_label_propagation_installs_both_classes_and_refuses_others():
    pl = _pl()
    a, b = pl.LabelPropagation(), pl.TransductiveGMM()
    with pl.label_propagation(b) as got:
        assert got is b and pl.propagation() is b
        with pl.label_propagation(a):
            assert pl.propagation() is a
        assert pl.propagation() is b
    assert pl.propagation() is None
    for other in (16, "gmm", object(), pl.TransductiveGMM):
        with pytest.raises(TypeError):
            with pl.label_propagation(other):
                pass
    assert pl.propagation() is None


def test_pickle_infix_is_the_installed_objects(tmp_path, monkeypatch):
    """pseudolabel_top_k reads `..._pseudolabels_split_...`, `..._lp_split_...` or `..._gmm_split_...` by what is installed: a cached list of one kind is
    never taken for another (the files are planted: nothing is computed)."""
    import pickle

    pl = _pl()
    from grip_amd.utils.clip_pseudolabels import pseudolabel_top_k
    monkeypatch.chdir(tmp_path)
    os.makedirs("pseudolabels")
    cfg = SimpleNamespace(LEARNING_PARADIGM="ul", MODEL="textual_fpl")
    for tag in ("", "lp_", "gmm_"):
        with open(f"pseudolabels/D_ViT-B32_ul_textual_fpl_2_pseudolabels_{tag}split_7.pickle", "wb") as f:
            pickle.dump({"filepaths": [tag or "plain"], "labels": [0]}, f)

    def load():
        ds = SimpleNamespace(filepaths=["x"], labels=[1])
        return pseudolabel_top_k(cfg, "D", 2, "", ds, [], None, None, {}, "cpu", "ViT-B/32", 7).filepaths
    assert load() == ["plain"]
    with pl.label_propagation(pl.TransductiveGMM()):
        assert load() == ["gmm_"]
        with pl.label_propagation(pl.LabelPropagation()):
            assert load() == ["lp_"]
    assert load() == ["plain"]


def test_the_two_transductions_exclude_each_other(monkeypatch):
    """TrainingStrategy.__init__ reads the switches before it builds any encoder: the constructor runs here without a model, up to that point."""
    import grip_amd  # noqa: F401
    from grip_amd.methods import training_strategies as ts

    class Stop(Exception):
        pass

    class Probe(ts.TrainingStrategy):
        def declare_custom_encoder(self):
            raise Stop(self)

    monkeypatch.setattr(ts.clip, "load", lambda *a, **k: (None, None))

    def make(**kw):
        cfg = SimpleNamespace(VIS_ENCODER="small", PROMPT_TEMPLATE="", MODALITY="text", CACHE_POOL_FEATURES=False, **kw)
        with pytest.raises(Stop) as stop:
            Probe(cfg, {}, [], [], [], "cpu")
        return stop.value.args[0]

    with pytest.raises(ValueError, match="TRANSDUCTIVE_GMM and LABEL_PROPAGATION"):
        make(TRANSDUCTIVE_GMM=True, LABEL_PROPAGATION=True)
    s = make(TRANSDUCTIVE_GMM=True, GMM_K=5, GMM_LAMBDA=2.0, GMM_ITERS=3, GMM_Z_ITERS=2)
    g = s.gmm
    assert (g.k, g.lam, g.iters, g.z_iters, g.keep_graphs) == (5, 2.0, 3, 2, True) and s.label_prop is None and s.transduction() is g and s.gmm_state is None
    s = make(LABEL_PROPAGATION=True)
    assert s.gmm is None and s.label_prop is not None and s.transduction() is s.label_prop
    s = make()
    assert s.gmm is None and s.label_prop is None and s.transduction() is None and s.gmm_state is None


def test_abi_lists_the_four_entry_points():
    import grip_amd  # noqa: F401
    from grip_amd import native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "grip_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(grip_[a-z_0-9]+)\s*\(", text))
    for name in NEW_EXPORTS:
        assert name in declared and name in native.EXPORTS, name
    assert native.ABI_VERSION == 9
    lib = native.lib()
    for name in NEW_EXPORTS:
        assert getattr(lib, name) is not None


def test_workspace_calls_need_no_device_and_refuse_bad_sizes():
    import ctypes

    import grip_amd  # noqa: F401
    from grip_amd import native
    lib = native.lib()
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_gmm_mstep_workspace(50000, 102, 512, ctypes.byref(nbytes)))
    chunks = -(-50000 // R.ROWS)
    assert nbytes.value >= 4 * chunks * 102 * 512
    native.check(lib.grip_gmm_estep_workspace(50000, 102, 512, 3, ctypes.byref(nbytes)))
    assert nbytes.value >= 4 * (102 * 512 + 2 * 50000 * 102)
    for args, word in (((0, 2, 8), "n = 0"), ((5, 0, 8), "c = 0"), ((5, 2, 6), "e = 6"), ((5, 2, 2052), "e = 2052")):
        assert lib.grip_gmm_mstep_workspace(*args, ctypes.byref(nbytes)) == 1 and word in lib.grip_last_error().decode()
        assert lib.grip_gmm_estep_workspace(*args, 3, ctypes.byref(nbytes)) == 1 and word in lib.grip_last_error().decode()
    assert lib.grip_gmm_estep_workspace(5, 2, 8, 33, ctypes.byref(nbytes)) == 1 and "k = 33" in lib.grip_last_error().decode()
    assert lib.grip_gmm_estep_workspace(5, 2, 8, 0, ctypes.byref(nbytes)) == 1 and "k = 0" in lib.grip_last_error().decode()
