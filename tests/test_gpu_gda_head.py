"""The Gaussian discriminant head end to end on the device (models/gda_models.py GdaHeadModel; GDA_HEAD of the textual strategies): the fit is the
hand-rolled sequence of engine calls bit for bit; the planted pool at C = 20, e = 64 keeps its ordering and stays within the composed bound of
tests/gda_ref.py (fit64 + head64); a tiny textual strategy predicts CLIP logits + linear_head, its head file reloads to the same logits, and the
pseudolabel lists and the prompt file do not move with the switch."""
import os

import numpy as np
import pytest
import torch

import gda_ref as R
import test_gpu_tip_adapter as T
from conftest import write_report

pytestmark = pytest.mark.gpu


def test_fit_is_the_hand_rolled_sequence_of_engine_calls():
    import grip_amd  # noqa: F401
    from grip_amd import engine
    from grip_amd.models import GdaHeadModel
    g = torch.Generator().manual_seed(11)
    n, C, e = 300, 7, 68
    raw = (torch.randn(n, e, generator=g) * (0.5 + torch.rand(n, 1, generator=g))).cuda()
    y = torch.randint(0, C - 1, (n,), generator=g)        # class C - 1 owns no row
    pseudo = (torch.rand(n, generator=g) < 0.4).tolist()
    prior = torch.rand(C, generator=g) + 0.1
    m = GdaHeadModel.fit(raw, y, pseudo, C, pseudo_weight=0.25, shrink=0.5, alpha=2.0, prior=prior)
    unit = (raw / raw.norm(dim=-1, keepdim=True)).contiguous()
    r = torch.where(torch.tensor(pseudo), torch.tensor(0.25), torch.tensor(1.0))
    z = torch.zeros(n, C, device="cuda")
    z[torch.arange(n), y.cuda()] = r.cuda()
    count, mean, _ = engine.gmm_mstep(z, unit)
    S = engine.class_scatter(unit, y.to(torch.int32).cuda(), r.cuda(), mean)
    w = engine.spd_solve(S, mean, a_scale=1.0 / float(r.double().sum()), ridge_rel=0.5)
    bias = 0.5 * (mean * w).sum(1) - torch.log(prior.cuda())
    assert float(count[C - 1]) == 0 and (m.w[C - 1] == 0).all() and float(m.bias[C - 1]) == 0 and (m.mean[C - 1] == 0).all()
    assert torch.equal(m.mean, mean) and torch.equal(m.w[:C - 1], w[:C - 1]) and torch.equal(m.bias[:C - 1], bias[:C - 1])
    assert (m.n_class, m.alpha) == (C, 2.0)
    base = torch.randn(n, C, generator=g).cuda() * 20
    out = m(raw, base)
    by_hand, pred = engine.linear_head(raw, m.w, m.bias, 2.0, base, want_argmax=True)
    assert torch.equal(out, by_hand) and out.data_ptr() != base.data_ptr() and torch.equal(pred.long(), out.argmax(1))
    assert torch.equal(out[:, C - 1], base[:, C - 1]), "a class without rows must contribute nothing"
    # no weights at all (pseudo_weight 1) is the unweighted call, and the fit is bit-reproducible
    a, b = (GdaHeadModel.fit(raw, y, pseudo, C) for _ in range(2))
    assert torch.equal(a.w, b.w) and torch.equal(a.bias, b.bias)
    S1 = engine.class_scatter(unit, y.to(torch.int32).cuda(), None, a.mean)
    assert torch.equal(a.w[:C - 1], engine.spd_solve(S1, a.mean, a_scale=1.0 / n, ridge_rel=1.0)[:C - 1])
    # search: the first best alpha of the grid
    labels = out.argmax(1)
    best = m.search([0.0, 2.0, 2.0, 5.0], raw, base, labels)
    assert best == (2.0, 1.0) and m.alpha == 2.0


@pytest.mark.parametrize("seed", R.PLANTED_SEEDS)
def test_planted_pool_on_the_device(seed):
    """C = 20, e = 64: the device's head keeps the float64 ordering (GDA at alpha = 1 above zero-shot and above the diagonal variant) and every logit is
    within the composed bound of fit64 + head64."""
    import grip_amd  # noqa: F401
    from grip_amd.models import GdaHeadModel
    C, e = R.PLANTED_SHAPES[0]
    Ftr, ytr, fte, yte, clip = R.planted_pool(C, e, seed)
    m = GdaHeadModel.fit(Ftr.cuda(), ytr, [False] * len(ytr), C)
    out = m(fte.cuda(), clip.cuda())
    acc64 = R.planted_accuracies(C, e, seed)
    acc = float((out.argmax(1).cpu() == yte).float().mean())
    print(f"planted C = {C}, e = {e}, seed {seed}: device GDA alpha=1 {acc:.3f} (float64 {acc64['gda']:.3f}), zero-shot {acc64['zero_shot']:.3f}, "
          f"diagonal {acc64['diagonal']:.3f}")
    assert acc > acc64["zero_shot"] and acc > acc64["diagonal"]
    _, w64, b64 = R.fit64(Ftr, ytr, None, C)
    ref = R.head64(fte, torch.from_numpy(w64), torch.from_numpy(b64), 1.0, clip)
    dw, db = R.fit_bound(Ftr, ytr, None, C)
    assert (np.abs(R.f64(m.w) - w64) <= dw).all() and (np.abs(R.f64(m.bias) - b64) <= db).all()
    bound = R.composed_logit_bound(fte, m.w, m.bias, 1.0, clip, dw, db)
    ratio = np.abs(R.f64(out) - ref) / bound
    write_report(f"gda_planted_{seed}.json", {"accuracy": acc, "float64": acc64, "worst_ratio": float(ratio.max()),
                                              "w_ratio": float((np.abs(R.f64(m.w) - w64) / dw).max())})
    print(f"   worst |err| / bound: logits {ratio.max():.4f}, w {(np.abs(R.f64(m.w) - w64) / dw).max():.4f}")
    assert (ratio <= 1).all(), ratio.max()


def test_strategy_gda_head(tmp_path):
    from grip_amd.engine import cosine_head, linear_head
    from grip_amd.models import GdaHeadModel
    from grip_amd.utils import compute_metrics as cm
    off, on = T._run(tmp_path), T._run(tmp_path, GDA_HEAD=True, GDA_ALPHA=2.0, GDA_PSEUDO_WEIGHT=0.5)
    # the pseudolabel pass and the prompt training are untouched: same lists, same prompt, byte-identical prompt file
    assert (on["data"]["train"].filepaths, on["data"]["train"].labels) == (off["data"]["train"].filepaths, off["data"]["train"].labels)
    assert len(on["prompt"]) == len(off["prompt"]) and all(np.array_equal(a, b) for a, b in zip(on["prompt"], off["prompt"]))
    assert on["best"] == off["best"]
    m, other, train = on["m"], off["m"], on["data"]["train"]
    assert other.gda is None and other.tip is None and other.adapter is None and isinstance(m.gda, GdaHeadModel) and m.gda.w.is_cuda
    assert m.tip is None and m.adapter is None and m.gda.alpha == 2.0 and m.gda_classes == list(on["classes"])
    assert not torch.equal(on["logits"], off["logits"])
    # the head is the fit of the training set's rows: frozen features, labels, pseudo rows at GDA_PSEUDO_WEIGHT
    with torch.no_grad():
        feats = m.frozen_image_features(train.images, [p.split("/")[-1] for p in train.filepaths])
    pseudo = [p.split("/")[-1] in m.check_unlabeled for p in train.filepaths]
    assert 0 < sum(pseudo) == len(train) - 10
    again = GdaHeadModel.fit(feats, [int(l) for l in train.labels], pseudo, len(on["classes"]), pseudo_weight=0.5, alpha=2.0)
    assert torch.equal(again.w, m.gda.w) and torch.equal(again.bias, m.gda.bias) and torch.equal(again.mean, m.gda.mean)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        fn_off = cm.save_parameters(off["prompt"], off["conf"])
        with open(fn_off, "rb") as fh:
            bytes_off = fh.read()
        fn = cm.save_parameters(on["prompt"], on["conf"], gda=m.gda)
        path = cm.gda_head_path(on["conf"])
        assert fn == fn_off and os.path.exists(path) and path == fn[:-len(".pickle")] + "_gda.pickle"
        with open(fn, "rb") as fh:
            assert fh.read() == bytes_off
        # the head file round-trips through predict on the strategy that was trained without it ...
        loaded = other.load_gda_head(path, off["classes"])
        try:
            _, reloaded = other.predict(off["data"]["test"], off["classes"])
            # ... predict is CLIP logits + linear_head by hand ...
            test = off["data"]["test"]
            with torch.no_grad():
                tf = other.frozen_image_features(test.images)
                text = other.features(test.images[:1], off["classes"])[1]
                clip_logits = cosine_head(tf, text, other.scale(), want_probs=False)[0]
                manual = linear_head(tf, loaded.w, loaded.bias, 2.0, clip_logits)
            # ... and a class subset gathers the head's columns
            sub = list(off["classes"])[1:4]
            _, part = other.predict(off["data"]["test"], sub)
            with torch.no_grad():
                sub_clip = cosine_head(tf, other.features(test.images[:1], sub)[1], other.scale(), want_probs=False)[0]
                term = linear_head(tf, loaded.w, loaded.bias, 2.0)
        finally:
            other.gda = None
        _, plain = other.predict(off["data"]["test"], off["classes"])
    finally:
        os.chdir(cwd)
    assert torch.equal(reloaded, on["logits"]) and torch.equal(manual.cpu(), on["logits"]) and torch.equal(plain, off["logits"])
    assert torch.equal(part, (sub_clip + term[:, 1:4]).cpu())
    # another BATCH_SIZE: the same logits bit for bit; fitting again gives the same head and the global torch RNG is not read
    keep = m.config.BATCH_SIZE
    try:
        m.config.BATCH_SIZE = 4
        assert torch.equal(m.predict(on["data"]["test"], on["classes"])[1], on["logits"])
    finally:
        m.config.BATCH_SIZE = keep
    first, state = (m.gda.w.clone(), m.gda.bias.clone()), torch.get_rng_state()
    m.build_gda_head(on["data"]["train"])
    assert torch.equal(torch.get_rng_state(), state), "the global torch RNG moved"
    assert torch.equal(m.gda.w, first[0]) and torch.equal(m.gda.bias, first[1])
    # GDA_SEARCH picks from the grid on the validation set
    m.config.GDA_SEARCH, m.config.GDA_ALPHA_GRID = True, (0.5, 4.0)
    try:
        m.build_gda_head(on["data"]["train"], on["data"]["val"])
        assert m.gda_search is not None and m.gda.alpha == m.gda_search[0] and m.gda.alpha in (0.5, 4.0)
    finally:
        m.config.GDA_SEARCH = False
        m.build_gda_head(on["data"]["train"])
    assert m.gda.alpha == 2.0 and torch.equal(m.predict(on["data"]["test"], on["classes"])[1], on["logits"])
