"""The float64 reference and bound of tests/sinkhorn_ref.py on the host (CPU): the vectorised reference equals a naive loop form at a tiny size; an f32
emulation of the recursion stays under the derived bound on the GPU tests' own inputs (and a planted fault of four bounds, or a wrong arg-max, does
not), so the bound is honest before a GPU sees it; on a planted pool with a biased marginal the float64 recursion raises the arg-max accuracy and fills
the smallest class; and the plumbing of the switch: BalancedAssignment validates its settings, names its three infixes, label_propagation() takes it as
a third class and nothing else, BALANCED_PSEUDOLABELS wraps the transduction that is on, the ABI lists the two calls."""
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import sinkhorn_ref as R
from conftest import REPO

NEW_EXPORTS = ("grip_sinkhorn_workspace", "grip_sinkhorn_balance")


def _pl():
    import grip_amd  # noqa: F401
    from grip_amd import pseudolabels as pl
    return pl


# ------------------------------------------------------------------------------------------ the reference against the naive loops
def test_reference_equals_the_naive_loops():
    n, c, tau, iters = 5, 3, 0.5, 2
    p = R.inputs(n, c, "zeros", seed=1)
    lt = R.log_target_of(c, [1.0, 2.0, 3.0])
    b0 = torch.tensor([0.25, -0.5, 0.0])
    q, mass, b = R.balance64(p, lt, tau, iters, b0)
    P, LT, B = p.double().tolist(), lt.double().tolist(), b0.double().tolist()

    def rows(B):
        out = []
        for i in range(n):
            a = [tau * math.log(max(P[i][j], R.TINY)) + B[j] for j in range(c)]
            x = [math.exp(v - max(a)) for v in a]
            out.append([v / sum(x) for v in x])
        return out
    for _ in range(iters):
        qq = rows(B)
        B = [B[j] + LT[j] + math.log(n) - math.log(max(sum(qq[i][j] for i in range(n)), R.TINY)) for j in range(c)]
    qq = rows(B)
    assert torch.allclose(q, torch.tensor(qq, dtype=torch.float64), rtol=1e-12, atol=1e-300)
    assert torch.allclose(b, torch.tensor(B, dtype=torch.float64), rtol=1e-12, atol=1e-15)
    assert torch.allclose(mass, torch.tensor([sum(qq[i][j] for i in range(n)) for j in range(c)], dtype=torch.float64), rtol=1e-12, atol=0)
    assert (p == 0).any() and torch.allclose(q.sum(1), torch.ones(n, dtype=torch.float64), rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------ the bound holds for an f32 emulation
@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_f32_emulation_stays_under_the_bound(case):
    p, lt, tau, iters, b0 = R.case_operands(case)
    q, pred, mass, b = R.balance_f32(p, lt, tau, iters, b0)
    assert R.check_balance(p, lt, tau, iters, b0, q, pred, mass, b) <= 1.0


def test_checker_rejects_an_element_off_by_four_bounds_and_a_wrong_argmax():
    case = (2 * R.ROWS + 1, 102, "plain", 1, "advanced", 1.0, None)
    p, lt, tau, iters, b0 = R.case_operands(case)
    q, pred, mass, b = R.balance_f32(p, lt, tau, iters, b0)
    q64, _, _, bq, bs, beta, _ = R.balance64(p, lt, tau, iters, b0, bounds=True)
    for name, t, bound, at in (("Q", q, bq, (7, int(q64[7].argmax()))), ("mass", mass, bs, (9,)), ("log_scale", b, beta, (9,))):
        bad = t.clone()
        bad[at] = (bad[at].double() + 4 * bound[at] + 1e-6 * bad[at].abs().double()).float()
        args = {"Q": q, "mass": mass, "log_scale": b, name: bad}
        with pytest.raises(AssertionError, match=f"balance: .{name} - "):
            R.check_balance(p, lt, tau, iters, b0, args["Q"], None, args["mass"], args["log_scale"])
    wrong = pred.clone()
    wrong[3] = (wrong[3] + 1) % 102
    with pytest.raises(AssertionError, match="pred is not the first maximum"):
        R.check_balance(p, lt, tau, iters, b0, q, wrong, mass, b)


# ------------------------------------------------------------------------------------------ what the balance is for
@pytest.mark.parametrize("n,c,gain,grow", [(2000, 20, 0.2, 50), (5100, 102, 0.2, 20)])
def test_planted_pool_gains_accuracy_and_fills_the_smallest_class(n, c, gain, grow):
    """A head that is right about the images and wrong about the marginal (per-class bias N(0, 1.5^2)): three iterations at tau = 1 raise the arg-max
    accuracy by at least `gain` and the smallest arg-max class by at least `grow` rows (float64 on the CPU; seen with seed 0: 0.442 -> 0.699 and 1 -> 89
    of 100 at 2 000 x 20, 0.137 -> 0.500 and 0 -> 34 of 50 at 5 100 x 102); the column residual falls with the iterations."""
    p, labels = R.planted_pool(n, c, seed=0)
    lt = R.log_target_of(c)
    acc, smallest, resid = {}, {}, {}
    for iters in (0, 3, 10):
        q, mass, _ = R.balance64(p, lt, 1.0, iters)
        pred = q.argmax(1)
        acc[iters] = float((pred == labels).double().mean())
        smallest[iters] = int(torch.bincount(pred, minlength=c).min())
        resid[iters] = float((mass / (n / c) - 1).abs().max())
    print(f"planted {n} x {c}: accuracy {acc}, smallest arg-max class {smallest}, column residual {resid}")
    assert acc[3] >= acc[0] + gain and smallest[3] >= smallest[0] + grow
    assert resid[10] < resid[3] < resid[0] and resid[10] < 1e-5


# ------------------------------------------------------------------------------------------ plumbing
def test_balanced_assignment_defaults_validation_and_infixes():
    pl = _pl()
    t = pl.BalancedAssignment()
    assert (t.tau, t.iters, t.prior, t.inner, t.state, t.infix) == (1.0, 3, None, None, None, "ot_")
    lp, gmm = pl.LabelPropagation(), pl.TransductiveGMM()
    assert pl.BalancedAssignment(inner=lp).infix == "ot_lp_" and pl.BalancedAssignment(inner=gmm).infix == "ot_gmm_"
    ok = pl.BalancedAssignment(tau=0.5, iters=0, prior=[1, 2, 3], inner=gmm)
    assert ok.prior.tolist() == [1.0, 2.0, 3.0] and ok.inner is gmm and "BalancedAssignment" in repr(ok)
    for bad in (dict(tau=0.0), dict(tau=-1.0), dict(tau=float("inf")), dict(tau=float("nan")), dict(iters=-1), dict(prior=[1.0, 0.0]), dict(prior=[1.0, -2.0]),
                dict(prior=[1.0, float("nan")]), dict(prior=[[1.0, 2.0]]), dict(prior=[]), dict(inner=3), dict(inner=pl.BalancedAssignment())):
        with pytest.raises(ValueError, match="BalancedAssignment"):
            pl.BalancedAssignment(**bad)


def test_label_propagation_takes_the_third_class_and_refuses_others():
    pl = _pl()
    a, b = pl.BalancedAssignment(), pl.BalancedAssignment(inner=pl.TransductiveGMM())
    with pl.label_propagation(a) as got:
        assert got is a and pl.propagation() is a
        with pl.label_propagation(b):
            assert pl.propagation() is b
        assert pl.propagation() is a
    assert pl.propagation() is None
    for other in (16, "ot", object(), pl.BalancedAssignment):
        with pytest.raises(TypeError):
            with pl.label_propagation(other):
                pass
    assert pl.propagation() is None


def test_pickle_infix_is_the_installed_objects(tmp_path, monkeypatch):
    """pseudolabel_top_k reads `..._ot_split_...`, `..._ot_lp_split_...` or `..._ot_gmm_split_...` by what is installed: a cached list of one kind is never
    taken for another (the files are planted: nothing is computed)."""
    import pickle

    pl = _pl()
    from grip_amd.utils.clip_pseudolabels import pseudolabel_top_k
    monkeypatch.chdir(tmp_path)
    os.makedirs("pseudolabels")
    cfg = SimpleNamespace(LEARNING_PARADIGM="ul", MODEL="textual_fpl")
    for tag in ("", "lp_", "gmm_", "ot_", "ot_lp_", "ot_gmm_"):
        with open(f"pseudolabels/D_ViT-B32_ul_textual_fpl_2_pseudolabels_{tag}split_7.pickle", "wb") as f:
            pickle.dump({"filepaths": [tag or "plain"], "labels": [0]}, f)

    def load():
        ds = SimpleNamespace(filepaths=["x"], labels=[1])
        return pseudolabel_top_k(cfg, "D", 2, "", ds, [], None, None, {}, "cpu", "ViT-B/32", 7).filepaths
    assert load() == ["plain"]
    with pl.label_propagation(pl.BalancedAssignment()):
        assert load() == ["ot_"]
        with pl.label_propagation(pl.BalancedAssignment(inner=pl.LabelPropagation())):
            assert load() == ["ot_lp_"]
        with pl.label_propagation(pl.BalancedAssignment(inner=pl.TransductiveGMM())):
            assert load() == ["ot_gmm_"]
        with pl.label_propagation(pl.TransductiveGMM()):
            assert load() == ["gmm_"]
    assert load() == ["plain"]


def test_the_switch_wraps_the_transduction_that_is_on(monkeypatch):
    """TrainingStrategy.__init__ reads the switches before it builds any encoder: the constructor runs here without a model, up to that point."""
    import grip_amd  # noqa: F401
    from grip_amd import pseudolabels as pl
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

    s = make()
    assert s.balanced is None and s.transduction() is None
    s = make(BALANCED_PSEUDOLABELS=False, OT_TAU=0.0)              # (the settings are not even read with the switch off)
    assert s.balanced is None and s.transduction() is None
    s = make(BALANCED_PSEUDOLABELS=True)
    b = s.balanced
    assert isinstance(b, pl.BalancedAssignment) and (b.tau, b.iters, b.prior, b.inner, b.infix) == (1.0, 3, None, None, "ot_")
    assert s.transduction() is b and s.gmm is None and s.label_prop is None and s.gmm_state is None
    s = make(BALANCED_PSEUDOLABELS=True, OT_TAU=0.5, OT_ITERS=7, OT_PRIOR=[1.0, 3.0], TRANSDUCTIVE_GMM=True, GMM_K=5)
    b = s.balanced
    assert (b.tau, b.iters, b.prior.tolist(), b.infix) == (0.5, 7, [1.0, 3.0], "ot_gmm_") and b.inner is s.gmm and s.gmm.k == 5
    assert s.transduction() is b and s.label_prop is None and s.gmm_state is None
    s = make(BALANCED_PSEUDOLABELS=True, LABEL_PROPAGATION=True)
    assert s.balanced.inner is s.label_prop and s.balanced.infix == "ot_lp_" and s.transduction() is s.balanced and s.gmm is None
    with pytest.raises(ValueError, match="TRANSDUCTIVE_GMM and LABEL_PROPAGATION"):
        make(BALANCED_PSEUDOLABELS=True, TRANSDUCTIVE_GMM=True, LABEL_PROPAGATION=True)
    with pytest.raises(ValueError, match="BalancedAssignment"):
        make(BALANCED_PSEUDOLABELS=True, OT_ITERS=-1)
    s = make(TRANSDUCTIVE_GMM=True)                                 # the other switches keep their meaning
    assert s.balanced is None and s.transduction() is s.gmm


def test_abi_lists_the_two_entry_points():
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


def test_workspace_call_needs_no_device_and_refuses_bad_sizes():
    import ctypes

    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    lib = native.lib()
    nbytes = ctypes.c_size_t()
    native.check(lib.grip_sinkhorn_workspace(50000, 102, ctypes.byref(nbytes)))
    assert engine.SINKHORN_ROWS == R.ROWS and nbytes.value >= 4 * -(-50000 // R.ROWS) * 102
    native.check(lib.grip_sinkhorn_workspace(2 ** 31 - 1, 1000, ctypes.byref(nbytes)))       # (64-bit sizes)
    assert nbytes.value >= 4 * (2 ** 31 // R.ROWS) * 1000
    for args, word in (((0, 2), "n = 0"), ((5, 0), "c = 0"), ((-1, 2), "n = -1")):
        assert lib.grip_sinkhorn_workspace(*args, ctypes.byref(nbytes)) == 1 and word in lib.grip_last_error().decode()
    # the argument checks of the call itself come before anything touches a device
    rc = lib.grip_sinkhorn_balance(None, None, None, 0.0, 3, 5, 2, None, None, None, None, None, 0, None)
    assert rc == 1 and "tau = 0" in lib.grip_last_error().decode()
    rc = lib.grip_sinkhorn_balance(None, None, None, float("nan"), 3, 5, 2, None, None, None, None, None, 0, None)
    assert rc == 1 and "tau = nan" in lib.grip_last_error().decode()
    rc = lib.grip_sinkhorn_balance(None, None, None, 1.0, -1, 5, 2, None, None, None, None, None, 0, None)
    assert rc == 1 and "iters = -1" in lib.grip_last_error().decode()
    rc = lib.grip_sinkhorn_balance(None, None, None, 1.0, 3, 5, 2, None, None, None, None, None, 0, None)
    assert rc == 1 and "null pointer" in lib.grip_last_error().decode()
