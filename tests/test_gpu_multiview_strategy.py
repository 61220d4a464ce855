"""MULTIVIEW_PSEUDOLABELS through the strategies (`small` towers, the synthetic pool of test_gpu_pool_cache: 6 classes, 108 unlabeled images).  With the
switch on, the matrix a pass hands to pseudolabel_from_features is bit-equal to engine.view_mode of the views augment.views makes from the sampler's
boxes; view 0's embedding is the ordinary pool embedding, bit for bit; with every box the identity the mode is u_0 within the derived bound
(tests/view_mode_ref.py); the pickle carries `mv_`; a textual strategy encodes its views once over two iterations, a visual one every pass; MV_PREDICT
changes predict's features and nothing else; with the switches absent a pass makes today's calls."""
import glob
import os

import numpy as np
import pytest
import torch

import view_mode_ref as R
from test_gpu_pool_cache import _strategy

pytestmark = pytest.mark.gpu
MV = dict(MULTIVIEW_PSEUDOLABELS=True, MV_VIEWS=4)
K = 4


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("GRIP_PSEUDOLABEL_MODE", "GRIP_SPLIT_TIER", "GRIP_SCREEN_STREAM"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture
def spy(monkeypatch):
    """Records the matrix every pseudolabel_from_features call receives and every engine.view_mode / augment.views call."""
    import grip_amd  # noqa: F401
    from grip_amd import augment, engine, pseudolabels as pl
    seen = {"matrix": [], "view_mode": 0, "views": 0, "encode_pool": []}
    real_pff, real_vm, real_views, real_enc = pl.pseudolabel_from_features, engine.view_mode, augment.views, pl.encode_pool

    def pff(img_emb, *a, **kw):
        seen["matrix"].append(img_emb.clone())
        return real_pff(img_emb, *a, **kw)

    def vm(*a, **kw):
        seen["view_mode"] += 1
        return real_vm(*a, **kw)

    def views(*a, **kw):
        seen["views"] += 1
        return real_views(*a, **kw)

    def enc(tower, images, *a, **kw):
        seen["encode_pool"].append((images.shape[0] if torch.is_tensor(images) else images.n, kw.get("paths") is not None))
        return real_enc(tower, images, *a, **kw)
    monkeypatch.setattr(pl, "pseudolabel_from_features", pff)
    monkeypatch.setattr(engine, "view_mode", vm)
    monkeypatch.setattr(augment, "views", views)
    monkeypatch.setattr(pl, "encode_pool", enc)
    return seen


def _pickles(root):
    return sorted(os.path.basename(f) for f in glob.glob(os.path.join(str(root), "pseudolabels", "*_pseudolabels_*split_*.pickle")))


def _views_by_hand(images, paths, views, seed=0, scale=(0.5, 1.0)):
    """[n * V, 3, H, H]: view 0 the image, view p the box of ViewSampler(seed).box(base name, epoch 0, view p), made by augment.views."""
    from grip_amd import augment
    x = images.cuda().float().contiguous()
    n, _, H, W = x.shape
    sampler = augment.ViewSampler(seed=seed, scale=scale)
    boxes = [(0, 0, H, W, 0) if p == 0 else sampler.box(os.path.basename(f), 0, H, W, view=p) for f in paths for p in range(views)]
    return augment.views(x, np.array(boxes, dtype=np.int32), rows=np.repeat(np.arange(n), views), n_px=H)


def test_textual_pass_hands_on_the_modes_of_the_samplers_views(tmp_path, monkeypatch, spy):
    from grip_amd import engine, pseudolabels as pl
    m, train, unlabeled = _strategy("TextualFPL", tmp_path, monkeypatch, **MV)
    assert isinstance(m.multi_view, pl.MultiView) and m.mv_passes is m.multi_view and m.multi_view.views == 4 and m.multi_view.keep_bytes == 4 << 30
    m.define_model(m.classes)
    images, paths = unlabeled.images, list(unlabeled.filepaths)
    n, V = len(paths), 4
    tower = m.clip_model.visual.tower
    vw = _views_by_hand(images, paths, V)
    assert torch.equal(vw.view(n, V, *vw.shape[1:])[:, 0], images.cuda().float()), "view 0 is a bit-exact copy"
    view_emb = pl.encode_pool(tower, vw, chunk=440).view(n, V, -1)
    assert torch.equal(view_emb[:, 0], pl.encode_pool(tower, images, chunk=440)), "view 0's embedding is the ordinary pool embedding"
    txt = m.trained_features(images, m.classes)[1].detach()      # (no MultiView is installed out here: the pass's own text features, inference kernels)
    _, probs, _, _ = engine.cosine_head(view_emb.reshape(n * V, -1), txt, m.scale())
    want, y = engine.view_mode(view_emb, probs.view(n, V, -1))
    spy["matrix"].clear()
    spy["encode_pool"].clear()
    got = m.assign_pseudo_labels(K, unlabeled)       # (identical mode is the default: with a MultiView installed the pass takes its plain branch)
    assert len(spy["matrix"]) == 1 and torch.equal(spy["matrix"][0], want) and pl.multiview() is None
    assert torch.equal(m.multi_view.last_y, y) and len(got.filepaths) > 0
    assert not any(keyed for _, keyed in spy["encode_pool"]), "the views go through encode_pool without a cache key"
    # a second iteration over the same pool encodes nothing: the frozen tower's view embeddings were kept
    unlabeled.filepaths, unlabeled.labels = list(paths), None
    before = len(spy["encode_pool"])
    m.assign_pseudo_labels(K, unlabeled)
    assert m.multi_view.encodes == 1 and len(spy["encode_pool"]) == before and torch.equal(spy["matrix"][1], want)
    unlabeled.filepaths, unlabeled.labels = list(paths), None
    m.create_training_dataset(train, unlabeled)
    names = _pickles(tmp_path)
    assert len(names) == 1 and "_pseudolabels_mv_split_" in names[0], names


def test_visual_strategy_encodes_its_views_every_pass_under_its_prompt(tmp_path, monkeypatch, spy):
    from grip_amd import engine, pseudolabels as pl
    m, train, unlabeled = _strategy("VisualFPL", tmp_path, monkeypatch, **MV)
    assert m.multi_view.keep_bytes == 0
    m.define_model(m.classes)
    images, paths = unlabeled.images, list(unlabeled.filepaths)
    n, V = len(paths), 4
    vw = _views_by_hand(images, paths, V)
    view_emb = pl.encode_pool(m.clip_model.visual.tower, vw, chunk=440, prefix=m.model.prefix.detach(), deep=m.deep_prompts()).view(n, V, -1)
    txt = m.fixed_text_features(m.classes)
    _, probs, _, _ = engine.cosine_head(view_emb.reshape(n * V, -1), txt, m.scale())
    want, _ = engine.view_mode(view_emb, probs.view(n, V, -1))
    spy["matrix"].clear()
    m.assign_pseudo_labels(K, unlabeled)
    unlabeled.filepaths, unlabeled.labels = list(paths), None
    m.assign_pseudo_labels(K, unlabeled)
    assert m.multi_view.encodes == 2 and torch.equal(spy["matrix"][0], want) and torch.equal(spy["matrix"][1], want)


def test_identity_boxes_give_the_single_view_within_the_bound(tmp_path, monkeypatch):
    from grip_amd import engine, pseudolabels as pl
    m, _, unlabeled = _strategy("TextualFPL", tmp_path, monkeypatch, **MV, MV_SCALE=(1.0, 1.0), MV_RATIO=(1.0, 1.0), MV_FLIP=0.0)
    m.define_model(m.classes)
    images, paths = unlabeled.images, list(unlabeled.filepaths)
    mv = m.multi_view
    view_emb = mv.encode_views(m.clip_model.visual.tower, images, paths, chunk=440)
    assert all(torch.equal(view_emb[:, p], view_emb[:, 0]) for p in range(1, 4))
    m.model.classes = m.classes
    txt = m.model(m.classes).detach()
    mode = mv.aggregate(view_emb, txt, m.scale())
    n, V, e = view_emb.shape
    _, probs, _, _ = engine.cosine_head(view_emb.reshape(n * V, e), txt, m.scale())
    probs = probs.view(n, V, -1)
    m64, _, _, bm, _, _ = R.run64(view_emb, probs, **R.DEFAULTS)
    u0 = view_emb[:, 0].double() / view_emb[:, 0].double().norm(dim=1, keepdim=True)
    assert (m64 - u0).abs().max() < 1e-12, "in float64 the mode of identical views is the view"
    worst, vac = R.check_run(view_emb, probs, R.DEFAULTS, None, None, mode, mv.last_y, None)      # (h2 sits on the floor: the carried bound is vacuous here)
    # identical views: m_d = (sum_p w_p u_0d) / (sum_p w_p) with the SAME weights in both sums, so whatever the weights are the quotient is u_0d up to
    # the rounding of u_0 itself (eu, tests/view_mode_ref.py), two sums of V terms and one division: (eu + (2 V + 4) u) |u_0d|
    bound = ((e / 2 + 5) + 2 * V + 4) * R.U * u0.abs() + R.TINY
    err = (mode.double() - u0).abs()
    print(f"identity boxes: worst |mode - u_0| / bound = {float((err / bound).max()):.3f} (carried bound: vacuous share {vac:.3f})")
    assert (err <= bound).all()


def test_mv_predict_changes_predicts_features_and_nothing_else(tmp_path, monkeypatch, spy):
    from grip_amd import engine, pseudolabels as pl
    monkeypatch.setenv("GRIP_PSEUDOLABEL_MODE", "f16")
    m, train, unlabeled = _strategy("TextualFPL", tmp_path, monkeypatch, MV_PREDICT=True, MV_VIEWS=4)
    assert m.mv_predict and m.multi_view is not None and m.mv_passes is None
    m.define_model(m.classes)
    _, plain_logits = _plain_predict(m, train)
    handed, real_agg = [], m.multi_view.aggregate

    def aggregate(view_emb, txt, scale):
        handed.append((view_emb.clone(), txt.detach().clone(), real_agg(view_emb, txt, scale)))
        return handed[-1][2]
    monkeypatch.setattr(m.multi_view, "aggregate", aggregate)
    pred, logits = m.predict(train, m.classes)
    assert len(handed) == 1 and len(train) <= 16       # one batch
    view_emb, txt, mode = handed[0]
    files = list(train.filepaths)
    vw = _views_by_hand(train.images, files, 4)
    assert torch.equal(view_emb, m.clip_model.encode_image(vw).float().view(len(files), 4, -1)), "predict encodes the sampler's views of its batch"
    _, probs, _, _ = engine.cosine_head(view_emb.reshape(len(files) * 4, -1), txt, m.scale())
    assert torch.equal(mode, engine.view_mode(view_emb, probs.view(len(files), 4, -1))[0])
    want = engine.cosine_head(mode, txt, m.scale(), want_probs=False)[0]       # no head is on: the logits are the cosine head of the modes
    assert torch.equal(logits, want.cpu()) and not torch.equal(logits, plain_logits)
    assert torch.equal(pred, torch.tensor([m.label_to_idx[c] for c in m.classes])[want.cpu().argmax(1)])
    # the pseudolabel pass is the plain one: encode_pool's rows, no view_mode call, a pickle without mv_
    images, paths = unlabeled.images, list(unlabeled.filepaths)
    emb = pl.encode_pool(m.clip_model.visual.tower, images, chunk=440)
    spy["matrix"].clear()
    n_vm = spy["view_mode"]
    m.assign_pseudo_labels(K, unlabeled)
    assert torch.equal(spy["matrix"][0], emb) and spy["view_mode"] == n_vm
    unlabeled.filepaths, unlabeled.labels = list(paths), None
    m.create_training_dataset(train, unlabeled)
    assert "_mv_" not in _pickles(tmp_path)[0]


def _plain_predict(m, data):
    on, m.mv_predict = m.mv_predict, False
    try:
        return m.predict(data, m.classes)
    finally:
        m.mv_predict = on


def test_switches_absent_change_nothing(tmp_path, monkeypatch, spy):
    from grip_amd import engine, pseudolabels as pl
    monkeypatch.setenv("GRIP_PSEUDOLABEL_MODE", "f16")
    m, train, unlabeled = _strategy("TextualFPL", tmp_path, monkeypatch)
    assert m.multi_view is None and m.mv_passes is None and not m.mv_predict
    m.define_model(m.classes)
    images, paths = unlabeled.images, list(unlabeled.filepaths)
    labels = [m.label_to_idx[c] for c in m.classes]
    emb, txt = m.trained_features(images, m.classes)
    _, probs, am_l, _ = engine.cosine_head(emb, txt.detach(), m.scale())
    want = pl.leaderboard(probs.cpu().numpy(), am_l.cpu().numpy(), paths, labels, K)       # the plain head -> scan
    spy["matrix"].clear()
    spy["encode_pool"].clear()
    plain = m.assign_pseudo_labels(K, unlabeled)
    assert (list(plain.filepaths), list(plain.labels)) == (list(want[0]), list(want[1])) and len(want[0]) > 0
    assert spy["encode_pool"] == [(len(paths), True)] and torch.equal(spy["matrix"][0], emb)      # one keyed pool encode, its rows handed on
    m.predict(train, m.classes)
    unlabeled.filepaths, unlabeled.labels = list(paths), None
    m.create_training_dataset(train, unlabeled)
    names = _pickles(tmp_path)
    assert spy["view_mode"] == 0 and spy["views"] == 0 and len(names) == 1 and "_mv_" not in names[0], names
