"""CPU tests of the linear probe's references and plumbing (no GPU): the float64 gradients of tests/probe_ref.py equal float64 torch autograd of
F.cross_entropy with probability targets plus the ridge; an f32 torch emulation in the kernel's order stays under the bound on every input of the GPU
tests and a planted fault of four bounds in one element is rejected; with momentum 0 and the default step the float64 loss never increases; the ABI
names are exported and the workspace calls need no device; the switch excludes the other heads and the head file round-trips; and the planted experiment of DESIGN 21: the probe beats zero-shot at every seed."""
import ctypes

import numpy as np
import pytest
import torch

import gda_ref
import probe_ref as R


def _seed(case):
    n, c, e, _ = case
    return n * 1000 + c * 10 + e


# ------------------------------------------------------------------------------------------ the reference against autograd
@pytest.mark.parametrize("case", [(5, 3, 4, "mixed"), (65, 102, 36, "zerosoft"), (63, 65, 64, "ignored"), (9, 1, 4, "soft"), (40, 7, 36, "null")],
                         ids=R.case_id)
def test_reference_gradients_equal_float64_autograd(case):
    """T_i CE(x_i, t_i / T_i) with probability targets is T_i lse - t_i . x_i; rows that do not contribute are dropped before autograd sees them."""
    n, c, e, kind = case
    inp = R.probe_inputs(n, c, e, kind, _seed(case))
    p = R._prep(inp)
    keep = torch.from_numpy(p["ok"])
    F = torch.from_numpy(p["F"])[keep]
    W = torch.from_numpy(p["W"]).clone().requires_grad_(True)
    b = torch.from_numpy(p["b"]).clone().requires_grad_(True)
    t, r = torch.from_numpy(p["t"])[keep], torch.from_numpy(p["r"])[keep]
    x = torch.from_numpy(p["base"])[keep] + p["s"] * F @ W.T + b
    T = t.sum(1)
    ce = torch.nn.functional.cross_entropy(x, t / T.clamp(min=1e-300)[:, None], reduction="none")
    l2 = 0.7
    J = p["nu"] * (r * T * ce).sum() + 0.5 * l2 * (W * W).sum()
    J.backward()
    loss, gw, gb = R.objective64(inp)
    assert np.isclose(loss + 0.5 * l2 * (p["W"] ** 2).sum(), float(J.detach()), rtol=1e-12, atol=1e-14)
    assert np.allclose(gw + l2 * p["W"], W.grad.numpy(), rtol=1e-10, atol=1e-14) and np.allclose(gb, b.grad.numpy(), rtol=1e-10, atol=1e-14)


def test_partition_and_step_helpers_match_the_engine():
    import grip_amd  # noqa: F401
    from grip_amd import engine
    assert (engine.PROBE_SCORE_ROWS, engine.PROBE_ROWS) == (R.SCORE_ROWS, R.ROWS)
    for n, c, e, _ in R.CASES + [(50000, 102, 512, ""), (1632, 102, 512, "")]:
        per, slices = engine.probe_slices(n, c, e)
        assert (per * R.ROWS, slices) == R.split(n, c, e) and engine.probe_slice_cap(c, e) == R.slice_cap(c, e)
    assert R.split(4097, 3, 36) == (128, 33) and R.split(513, 1000, 1024) == (128, 5) and R.split(50000, 102, 512) == (13 * 64, 61)


# ------------------------------------------------------------------------------------------ emulation under the bound, a planted fault rejected
@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_f32_emulation_of_the_objective_stays_under_its_bound(case):
    n, c, e, kind = case
    inp = R.probe_inputs(n, c, e, kind, _seed(case))
    loss, gw, gb = R.emulate_objective(inp)
    ratios = R.check_objective(inp, loss, gw, gb)
    assert max(ratios) < 1 and np.isfinite(gw.numpy()).all()


def test_a_planted_fault_of_four_bounds_in_one_element_is_rejected():
    inp = R.probe_inputs(65, 102, 36, "mixed", 7)
    loss, gw, gb = R.objective64(inp)
    bl, bw, bb = R.objective_bound(inp)
    R.check_objective(inp, loss, torch.from_numpy(gw), torch.from_numpy(gb))
    i, j = np.unravel_index(bw.argmin(), bw.shape)
    bad = gw.copy()
    bad[i, j] += 4 * bw[i, j]
    with pytest.raises(AssertionError, match="grad_w"):
        R.check_objective(inp, loss, torch.from_numpy(bad), torch.from_numpy(gb))
    badb = gb.copy()
    badb[bb.argmin()] -= 4 * bb.min()
    with pytest.raises(AssertionError, match="grad_b"):
        R.check_objective(inp, loss, torch.from_numpy(gw), torch.from_numpy(badb))
    with pytest.raises(AssertionError, match="loss"):
        R.check_objective(inp, loss + 4 * bl, torch.from_numpy(gw), torch.from_numpy(gb))


@pytest.mark.parametrize("case", R.FIT_CASES, ids=[R.case_id(c) for c in R.FIT_CASES])
def test_f32_emulation_of_the_fit_stays_under_the_carried_bound(case):
    n, c, e, kind = case
    inp = R.probe_inputs(n, c, e, kind, _seed(case))
    lr = R.default_lr(inp["scale"], R.FIT_HYPER["l2"])
    for iters in (1, R.FIT_TIGHT_ITERS, R.FIT_GROSS_ITERS):
        out = R.emulate_fit(inp, R.FIT_HYPER["l2"], lr, R.FIT_HYPER["mu"], iters)
        ratios = R.check_fit(inp, R.FIT_HYPER["l2"], lr, R.FIT_HYPER["mu"], iters, *out)
        *_, (dW, _, _, _, _) = R.fit64(inp, R.FIT_HYPER["l2"], lr, R.FIT_HYPER["mu"], iters, want_bound=True)
        print(f"fit({iters}) {R.case_id(case)}: worst |err| / bound {max(ratios):.3f}; the bound on W is {dW.max() / R.U:.3g} u wide at most")
    W, *_ = R.emulate_fit(inp, R.FIT_HYPER["l2"], lr, R.FIT_HYPER["mu"], 2)
    W[0, 0] = -W[0, 0] + 1.0
    with pytest.raises(AssertionError):
        R.check_fit(inp, R.FIT_HYPER["l2"], lr, R.FIT_HYPER["mu"], 2, W, *R.emulate_fit(inp, R.FIT_HYPER["l2"], lr, R.FIT_HYPER["mu"], 2)[1:])


def test_update_follows_the_headers_sequence():
    """One step by hand: G = l2 W + gw, m = mu m + G, W = W - lr m; the bias without the ridge; state carried from call to call."""
    inp = R.probe_inputs(9, 3, 4, "mixed", 3)
    l2, lr, mu = 0.5, 0.01, 0.75
    _, gw, gb = R.objective64(inp)
    W1, b1, mw1, mb1, tr1 = R.fit64(inp, l2, lr, mu, 1)
    W0, b0 = inp["W"].double().numpy(), inp["b"].double().numpy()
    assert np.allclose(mw1, l2 * W0 + gw) and np.allclose(W1, W0 - lr * (l2 * W0 + gw)) and np.allclose(b1, b0 - lr * gb) and np.allclose(mb1, gb)
    W3, b3, mw3, mb3, tr3 = R.fit64(inp, l2, lr, mu, 3)
    nxt = dict(inp, W=torch.from_numpy(W1), b=torch.from_numpy(b1))
    W3b, b3b, mw3b, mb3b, tr2 = R.fit64(nxt, l2, lr, mu, 2, state=(mw1, mb1))
    assert np.array_equal(W3, W3b) and np.array_equal(b3, b3b) and np.array_equal(mw3, mw3b) and np.array_equal(tr3, np.concatenate([tr1, tr2]))


@pytest.mark.parametrize("l2", R.PLANTED_L2)
def test_loss_never_increases_without_momentum_at_the_default_step(l2):
    """The default step is the reciprocal of a Lipschitz bound of the gradient, so plain gradient descent (mu = 0) descends monotonically in exact
    arithmetic: the float64 trace of J = data term + (l2 / 2) |W|^2 must never go up."""
    C, e = gda_ref.PLANTED_SHAPES[0]
    Ftr, ytr, *_ = gda_ref.planted_pool(C, e, 0)
    inp = dict(F=Ftr, W=torch.zeros(C, e), b=torch.zeros(C), base=R.planted_train_logits(C, e, 0), y=ytr.to(torch.int32), soft=None, r=None,
               scale=R.PROBE_SCALE, norm=1.0 / Ftr.shape[0])
    lr = R.default_lr(R.PROBE_SCALE, l2)
    W = inp["W"].double().numpy()
    b = np.zeros(C)
    J = []
    for _ in range(60):
        cur = dict(inp, W=torch.from_numpy(W), b=torch.from_numpy(b))
        J.append(R.objective64(cur)[0] + 0.5 * float(np.float32(l2)) * (W * W).sum())
        W, b, *_ = R.fit64(cur, l2, lr, 0.0, 1)
    assert all(b_ <= a_ for a_, b_ in zip(J, J[1:])), J
    assert J[-1] < J[0]


# ------------------------------------------------------------------------------------------ plumbing
def test_abi_names_are_exported_and_the_workspace_calls_need_no_device():
    import grip_amd  # noqa: F401
    from grip_amd import native
    lib, nbytes = native.lib(), ctypes.c_size_t()
    for name in ("grip_probe_objective", "grip_probe_fit"):
        assert name in native.EXPORTS and name + "_workspace" in native.EXPORTS
    assert len(lib.grip_probe_objective.argtypes) == 18 and len(lib.grip_probe_fit.argtypes) == 22 and native.ABI_VERSION == 9
    native.check(lib.grip_probe_objective_workspace(50000, 102, 512, ctypes.byref(nbytes)))
    floats = 50000 * 102 + 61 * 102 * 512 + 61 * 102 + 1563
    assert floats * 4 <= nbytes.value <= floats * 4 + 4 * 256 + 256
    native.check(lib.grip_probe_fit_workspace(50000, 102, 512, ctypes.byref(nbytes)))
    assert floats * 4 <= nbytes.value
    for n, c, e, word in ((0, 3, 16, b"n = 0"), (5, 0, 16, b"c = 0"), (5, 1025, 16, b"c = 1025"), (5, 3, 6, b"e = 6"), (5, 3, 1028, b"e = 1028")):
        assert lib.grip_probe_objective_workspace(n, c, e, ctypes.byref(nbytes)) == 1 and word in lib.grip_last_error()
        assert lib.grip_probe_fit_workspace(n, c, e, ctypes.byref(nbytes)) == 1 and word in lib.grip_last_error()


def _strategy(modality, **conf):
    import types

    import grip_amd  # noqa: F401
    from grip_amd.methods.training_strategies import TrainingStrategy
    s = object.__new__(TrainingStrategy)
    s.config = types.SimpleNamespace(**conf)
    s.modality = modality
    return s


def test_the_switch_is_refused_beside_the_other_heads_and_ignored_by_visual_strategies():
    from grip_amd.methods.main import DEFAULTS
    assert "LINEAR_PROBE" not in DEFAULTS or DEFAULTS["LINEAR_PROBE"] is False
    assert not _strategy("text").linear_probe() and not _strategy("text", LINEAR_PROBE=False, GDA_HEAD=True).linear_probe()
    assert _strategy("text", LINEAR_PROBE=True).linear_probe() and _strategy("text", LINEAR_PROBE=True, PROBE_INIT="gda", GDA_HEAD=False).linear_probe()
    for modality in ("image", "multi"):
        assert not _strategy(modality, LINEAR_PROBE=True).linear_probe()
        assert not _strategy(modality, LINEAR_PROBE=True, GDA_HEAD=True).linear_probe()      # both ignored there: nothing to refuse
    for other in ("TIP_ADAPTER", "CLIP_ADAPTER", "GDA_HEAD"):
        with pytest.raises(ValueError, match=f"LINEAR_PROBE and {other} are different heads"):
            _strategy("text", LINEAR_PROBE=True, **{other: True}).linear_probe()
    with pytest.raises(ValueError, match="PROBE_INIT"):
        _strategy("text", LINEAR_PROBE=True, PROBE_INIT="ones").linear_probe()
    # the existing methods and their messages are what they were
    with pytest.raises(ValueError, match="GDA_HEAD, TIP_ADAPTER and CLIP_ADAPTER"):
        _strategy("text", GDA_HEAD=True, TIP_ADAPTER=True, LINEAR_PROBE=True).gda_head()
    assert _strategy("text", GDA_HEAD=True, LINEAR_PROBE=True).gda_head()


def test_probe_file_round_trips_beside_an_unchanged_prompt_file(tmp_path, monkeypatch):
    import os
    import types

    import grip_amd  # noqa: F401
    from grip_amd.models import LinearProbeModel
    from grip_amd.utils import compute_metrics as cm, linear_probe_path
    monkeypatch.chdir(tmp_path)
    conf = types.SimpleNamespace(MODALITY="text", VIS_ENCODER="ViT-B/16", DATASET_NAME="Synthetic", LEARNING_PARADIGM="ssl", MODEL="textual_fpl", OPTIM_SEED=1,
                                 SPLIT_SEED=500)
    g = torch.Generator().manual_seed(3)
    m = LinearProbeModel(torch.randn(5, 8, generator=g), torch.randn(5, generator=g), 5, scale=30.0, alpha=0.3)
    prompt = [torch.zeros(1, 4, 8).numpy()]
    plain = cm.save_parameters(prompt, conf, iteration=3)
    with open(plain, "rb") as f:
        plain_bytes = f.read()
    fn = cm.save_parameters(prompt, conf, iteration=3, probe=m)
    path = linear_probe_path(conf, 3)
    assert fn == plain and path == fn[:-len(".pickle")] + "_probe.pickle"
    assert sorted(os.listdir("trained_prompts")) == sorted([os.path.basename(fn), os.path.basename(path)])
    with open(fn, "rb") as f:
        assert f.read() == plain_bytes      # the prompt file is what it is without the head
    back = LinearProbeModel.load(path)
    assert torch.equal(back.w, m.w) and torch.equal(back.b, m.b) and (back.n_class, back.scale, back.alpha) == (5, 30.0, 0.3)
    cm.save_parameters(prompt, conf)      # no head: the prompt file alone
    assert not os.path.exists(linear_probe_path(conf))
    for labels in ([0, 1, 2, 3], [0, -1, 0, 0], [0.0, 1.0, 0.0, 1.0]):      # out of range; -1 without a soft matrix; not integers: refused on the host, before any device call
        with pytest.raises(ValueError):
            LinearProbeModel.fit(torch.randn(4, 8), None, labels, [False] * 4, 3)


# ------------------------------------------------------------------------------------------ the planted experiment
def test_planted_pool_probe_beats_zero_shot_at_every_seed():
    """A planted pool, not a dataset (gda_ref.planted_pool); float64 on the CPU.  Only this ordering is asserted: the probe (from zero, the default l2) above
    zero-shot at every seed.  GDA, the probe from zero and the probe from the GDA start are printed side by side without an asserted order."""
    C, e = gda_ref.PLANTED_SHAPES[0]
    for seed in gda_ref.PLANTED_SEEDS:
        acc = R.planted_accuracies(C, e, seed)
        print(f"planted C = {C}, e = {e}, seed {seed}: zero-shot {acc['zero_shot']:.3f}, GDA {acc['gda']:.3f}, probe {acc['probe']:.3f}, "
              f"probe from GDA {acc['probe_from_gda']:.3f}; loss {acc['probe_loss'][0]:.3f} -> {acc['probe_loss'][1]:.3f}")
        assert acc["probe"] > acc["zero_shot"], (seed, acc)
