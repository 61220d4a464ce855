"""The trained linear probe end to end on the device (models/probe_models.py LinearProbeModel; LINEAR_PROBE of the textual strategies): the planted pool
at C = 20, e = 64 keeps the float64 experiment's ordering; the model's logits are clip_logits + alpha (scale u . W + b) in float64 under the linear
head's own bound; the file round-trips; search picks the first best alpha; a tiny textual strategy predicts CLIP logits + the head's term, its pseudolabel
lists and prompt file do not move with the switch, the switch is refused beside the other heads and ignored by a visual strategy, and with
SOFT_PSEUDOLABELS the probe's soft rows are engine.soft_ce's targets."""
import logging
import os

import numpy as np
import pytest
import torch

import gda_ref
import probe_ref as R
import test_gpu_soft_strategy as S
import test_gpu_tip_adapter as T
from conftest import write_report

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", gda_ref.PLANTED_SEEDS)
def test_planted_pool_on_the_device(seed):
    """C = 20, e = 64, the default ridge, 300 iterations: the device's probe is above zero-shot, as the float64 experiment is.  Only the ordering is asserted (300 f32
    iterations are not bit-comparable with float64; the kernels' own bounds are tests/test_gpu_probe_kernels.py's); accuracies and losses are printed."""
    import grip_amd  # noqa: F401
    from grip_amd.models import LinearProbeModel
    C, e = gda_ref.PLANTED_SHAPES[0]
    Ftr, ytr, fte, yte, clip = gda_ref.planted_pool(C, e, seed)
    base = R.planted_train_logits(C, e, seed)
    acc64 = R.planted_accuracies(C, e, seed)
    m = LinearProbeModel.fit(Ftr.cuda(), base.cuda(), ytr, [False] * len(ytr), C)
    assert R.PROBE_L2 == 0.1      # (LinearProbeModel.fit's default)
    out = m(fte.cuda(), clip.cuda())
    acc = float((out.argmax(1).cpu() == yte).float().mean())
    trace = m.loss_trace.cpu()
    print(f"planted C = {C}, e = {e}, seed {seed}: device probe {acc:.3f} (float64 {acc64['probe']:.3f}), zero-shot {acc64['zero_shot']:.3f}, GDA {acc64['gda']:.3f}; "
          f"loss {float(trace[0]):.4f} -> {float(trace[-1]):.4f} (float64 {acc64['probe_loss'][0]:.4f} -> {acc64['probe_loss'][1]:.4f})")
    write_report(f"probe_planted_{seed}.json", {"accuracy": acc, "float64": acc64, "loss": [float(trace[0]), float(trace[-1])]})
    assert acc > acc64["zero_shot"] and acc64["probe"] > acc64["zero_shot"]      # the ordering, on the device as in float64
    assert trace.numel() == 300 and float(trace[-1]) < float(trace[0])


def test_model_logits_file_and_search():
    import grip_amd  # noqa: F401
    from grip_amd import engine
    from grip_amd.models import GdaHeadModel, LinearProbeModel
    g = torch.Generator().manual_seed(21)
    n, C, e = 200, 20, 64
    raw = (torch.randn(n, e, generator=g) * (0.5 + torch.rand(n, 1, generator=g)))
    y = torch.randint(0, C, (n,), generator=g)
    base = torch.randn(n, C, generator=g) * 10
    pseudo = (torch.rand(n, generator=g) < 0.4).tolist()
    m = LinearProbeModel.fit(raw.cuda(), base.cuda(), y, pseudo, C, pseudo_weight=0.25, scale=50.0, l2=0.5, iters=20, alpha=2.0)
    assert (m.n_class, m.scale, m.alpha) == (C, 50.0, 2.0) and m.loss_trace.numel() == 20 and float(m.loss_trace[-1]) < float(m.loss_trace[0])
    # the fit is engine.probe_fit on the unit rows, bit for bit, and reproducible
    unit = (raw.cuda() / raw.cuda().norm(dim=-1, keepdim=True)).contiguous()
    r = torch.where(torch.tensor(pseudo), torch.tensor(0.25), torch.tensor(1.0))
    lr = 1.0 / (0.5 * (50.0 ** 2 + 1) + 0.5)
    w, b, _ = engine.probe_fit(unit, base.cuda(), y.to(torch.int32).cuda(), None, r.cuda(), 50.0, 0.5, lr, 0.9, 20, torch.zeros(C, e, device="cuda"),
                               torch.zeros(C, device="cuda"), norm=1.0 / float(r.double().sum()))
    assert torch.equal(m.w, w) and torch.equal(m.b, b)
    # logits = clip_logits + alpha (scale u . W + b): float64, under the linear head's own bound with w = scale W, bias = -b
    out = m(raw.cuda(), base.cuda())
    ws, nb = (m.w * m.scale).cpu(), (-m.b).cpu()
    ratio = gda_ref.check_head(raw, ws, nb, 2.0, base, out)
    u64 = torch.nn.functional.normalize(raw.double(), dim=1).numpy()
    direct = base.double().numpy() + 2.0 * (u64 @ ws.double().numpy().T - nb.double().numpy()[None, :])
    assert np.abs(gda_ref.head64(raw, ws, nb, 2.0, base) - direct).max() < 1e-9
    print(f"probe logits: worst |err| / bound = {ratio:.3f}")
    by_hand, pred = engine.linear_head(raw.cuda(), m.w * 50.0, -m.b, 2.0, base.cuda(), want_argmax=True)
    assert torch.equal(out, by_hand) and out.data_ptr() != base.data_ptr()
    # search: the first best alpha of the grid
    best = m.search([0.0, 2.0, 2.0, 5.0], raw.cuda(), base.cuda(), out.argmax(1))
    assert best == (2.0, 1.0) and m.alpha == 2.0
    # soft rows, an init from a GDA head, and the label rules
    soft = torch.softmax(torch.randn(n, C, generator=g), 1)
    y2 = y.clone()
    y2[::3] = -1
    ms = LinearProbeModel.fit(raw.cuda(), None, y2, pseudo, C, soft=soft.cuda(), iters=3)
    gda = GdaHeadModel.fit(raw.cuda(), y, pseudo, C)
    mg = LinearProbeModel.fit(raw.cuda(), base.cuda(), y, pseudo, C, iters=1, init=(gda.w / 100.0, -gda.bias), lr=1e-30)
    assert torch.isfinite(ms.w).all() and torch.allclose(mg.w * 100.0, gda.w, rtol=1e-6, atol=1e-30) and torch.allclose(-mg.b, gda.bias, rtol=1e-6, atol=1e-30)
    for bad in (y2, [0.0] * n, [C] * n, [-2] * n):
        with pytest.raises(ValueError):
            LinearProbeModel.fit(raw.cuda(), base.cuda(), bad, pseudo, C, iters=1)


def test_file_round_trip(tmp_path):
    import grip_amd  # noqa: F401
    from grip_amd.models import LinearProbeModel
    g = torch.Generator().manual_seed(3)
    m = LinearProbeModel(torch.randn(5, 8, generator=g), torch.randn(5, generator=g), 5, scale=30.0, alpha=0.3)
    back = LinearProbeModel.load(m.save(str(tmp_path / "p.pickle")), device="cuda")
    assert torch.equal(back.w.cpu(), m.w) and torch.equal(back.b.cpu(), m.b) and (back.n_class, back.scale, back.alpha) == (5, 30.0, 0.3) and back.w.is_cuda
    assert sorted(m.state()) == ["alpha", "b", "n_class", "scale", "w"]
    with pytest.raises(ValueError):
        LinearProbeModel(torch.zeros(5, 8), torch.zeros(4), 5)


def test_strategy_linear_probe(tmp_path):
    from grip_amd.engine import cosine_head, linear_head
    from grip_amd.models import LinearProbeModel
    from grip_amd.utils import compute_metrics as cm
    off, on = T._run(tmp_path), T._run(tmp_path, LINEAR_PROBE=True, PROBE_ALPHA=2.0, PROBE_PSEUDO_WEIGHT=0.5, PROBE_ITERS=25, PROBE_L2=0.1)
    # the pseudolabel pass and the prompt training are untouched: same lists, same prompt, byte-identical prompt file
    assert (on["data"]["train"].filepaths, on["data"]["train"].labels) == (off["data"]["train"].filepaths, off["data"]["train"].labels)
    assert len(on["prompt"]) == len(off["prompt"]) and all(np.array_equal(a, b) for a, b in zip(on["prompt"], off["prompt"]))
    assert on["best"] == off["best"]
    m, other, train = on["m"], off["m"], on["data"]["train"]
    assert other.probe is None and isinstance(m.probe, LinearProbeModel) and m.probe.w.is_cuda and m.tip is None and m.adapter is None and m.gda is None
    assert m.probe.alpha == 2.0 and m.probe_classes == list(on["classes"]) and m.probe.loss_trace.numel() == 25 and m.probe.scale == float(m.scale())
    assert not torch.equal(on["logits"], off["logits"])
    # the probe is the fit of the training set's rows: frozen features, the trained prompt's CLIP logits, labels, pseudo rows at PROBE_PSEUDO_WEIGHT
    names = [p.split("/")[-1] for p in train.filepaths]
    with torch.no_grad():
        feats = m.frozen_image_features(train.images, names)
        text = m.features(train.images[:1], on["classes"])[1]
        clip_train = cosine_head(feats, text, m.scale(), want_probs=False)[0]
    pseudo = [p in m.check_unlabeled for p in names]
    assert 0 < sum(pseudo) == len(train) - 10
    again = LinearProbeModel.fit(feats, clip_train, [int(l) for l in train.labels], pseudo, len(on["classes"]), pseudo_weight=0.5, scale=float(m.scale()), l2=0.1,
                                 iters=25, alpha=2.0)
    assert torch.equal(again.w, m.probe.w) and torch.equal(again.b, m.probe.b)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        fn_off = cm.save_parameters(off["prompt"], off["conf"])
        with open(fn_off, "rb") as fh:
            bytes_off = fh.read()
        fn = cm.save_parameters(on["prompt"], on["conf"], probe=m.probe)
        path = cm.linear_probe_path(on["conf"])
        assert fn == fn_off and os.path.exists(path) and path == fn[:-len(".pickle")] + "_probe.pickle"
        with open(fn, "rb") as fh:
            assert fh.read() == bytes_off
        loaded = other.load_linear_probe(path, off["classes"])
        try:
            _, reloaded = other.predict(off["data"]["test"], off["classes"])
            test = off["data"]["test"]
            with torch.no_grad():
                tf = other.frozen_image_features(test.images)
                clip_logits = cosine_head(tf, other.features(test.images[:1], off["classes"])[1], other.scale(), want_probs=False)[0]
                manual = linear_head(tf, loaded.w * loaded.scale, -loaded.b, 2.0, clip_logits)
                term = linear_head(tf, loaded.w * loaded.scale, -loaded.b, 2.0)
            sub = list(off["classes"])[1:4]
            _, part = other.predict(off["data"]["test"], sub)
            with torch.no_grad():
                sub_clip = cosine_head(tf, other.features(test.images[:1], sub)[1], other.scale(), want_probs=False)[0]
        finally:
            other.probe = None
        _, plain = other.predict(off["data"]["test"], off["classes"])
    finally:
        os.chdir(cwd)
    # predict is the CLIP logits plus exactly the head's term
    assert torch.equal(reloaded, on["logits"]) and torch.equal(manual.cpu(), on["logits"]) and torch.equal(plain, off["logits"])
    assert torch.equal(part, (sub_clip + term[:, 1:4]).cpu())
    # building again gives the same probe and the global torch RNG is not read; PROBE_SEARCH picks from the grid; PROBE_INIT "gda" starts elsewhere
    first, state = (m.probe.w.clone(), m.probe.b.clone()), torch.get_rng_state()
    m.build_linear_probe(on["data"]["train"])
    assert torch.equal(torch.get_rng_state(), state), "the global torch RNG moved"
    assert torch.equal(m.probe.w, first[0]) and torch.equal(m.probe.b, first[1]) and m.probe_targets[1] is None
    m.config.PROBE_SEARCH, m.config.PROBE_ALPHA_GRID, m.config.PROBE_INIT = True, (0.5, 4.0), "gda"
    try:
        m.build_linear_probe(on["data"]["train"], on["data"]["val"])
        assert m.probe_search is not None and m.probe.alpha == m.probe_search[0] and m.probe.alpha in (0.5, 4.0) and not torch.equal(m.probe.w, first[0])
    finally:
        m.config.PROBE_SEARCH, m.config.PROBE_INIT = False, "zero"
        m.build_linear_probe(on["data"]["train"])
    assert m.probe.alpha == 2.0 and torch.equal(m.predict(on["data"]["test"], on["classes"])[1], on["logits"])


def test_switch_is_refused_beside_the_other_heads_and_ignored_by_a_visual_strategy(tmp_path, monkeypatch, caplog):
    for other in ("TIP_ADAPTER", "CLIP_ADAPTER", "GDA_HEAD"):
        with pytest.raises(ValueError, match=f"LINEAR_PROBE and {other}"):
            S._strategy(tmp_path / other, monkeypatch, LINEAR_PROBE=True, **{other: True})
    with pytest.raises(ValueError, match="PROBE_INIT"):
        S._strategy(tmp_path / "init", monkeypatch, LINEAR_PROBE=True, PROBE_INIT="ones")
    with caplog.at_level(logging.INFO):
        m, train, unlabeled = S._strategy(tmp_path / "visual", monkeypatch, paradigm="ul", cls_name="VisualFPL", LINEAR_PROBE=True, GDA_HEAD=True)
    assert sum("LINEAR_PROBE is ignored by the image strategies" in r.getMessage() for r in caplog.records) == 1
    assert not m.linear_probe() and m.probe is None


def test_soft_pseudolabels_give_the_probe_engine_soft_ces_targets(tmp_path, monkeypatch):
    from grip_amd import engine
    m, train, unlabeled = S._strategy(tmp_path, monkeypatch, LINEAR_PROBE=True, PROBE_ITERS=5, **S.LP, **S.SOFT)
    data = m.create_training_dataset(train, unlabeled)
    m.define_model(m.classes)
    probe = m.build_linear_probe(data)
    labels, targets = m.probe_targets
    classes, ids, lut = m._class_space(False)
    soft = m.soft_targets(classes)
    with torch.random.fork_rng(devices=[]):
        feats, clip_logits, labs, names = m._tip_inputs(data, classes, lut)
    rows = m.soft_rows(soft, ids[labs].tolist(), names)
    is_soft = rows >= 0
    assert 0 < int(is_soft.sum()) < len(names) and [n in m.check_unlabeled for n in names] == is_soft.tolist()
    assert torch.equal(labels[is_soft], torch.full_like(labels[is_soft], -1)) and torch.equal(labels[~is_soft], labs[~is_soft])
    _, _, want = engine.soft_ce(torch.randn_like(clip_logits), labs, torch.rand(len(names), device="cuda") + 0.5, soft.matrix, rows, soft.col_map, soft.temperature,
                                soft.smoothing, want_target=True)
    assert torch.equal(targets[is_soft], want[is_soft]) and torch.allclose(targets[is_soft].sum(1), torch.ones(int(is_soft.sum()), device="cuda"), atol=1e-5)
    # the fit read those rows: the same call by hand gives the same bits, and hard labels give other ones
    pseudo = [n in m.check_unlabeled for n in names]
    from grip_amd.models import LinearProbeModel
    again = LinearProbeModel.fit(feats, clip_logits, labels, pseudo, len(classes), soft=want, scale=float(m.scale()), iters=5)
    hard = LinearProbeModel.fit(feats, clip_logits, labs, pseudo, len(classes), scale=float(m.scale()), iters=5)
    assert torch.equal(again.w, probe.w) and torch.equal(again.b, probe.b) and not torch.equal(hard.w, probe.w)
