"""TPT through the strategies (`small` towers, the synthetic pool of test_gpu_pool_cache: 6 classes; the 12 labelled shots stand in for a test set, V = 8).
With the switch absent `predict` is the parent's, bit for bit (against a second strategy built without the key, and with the tuner class made unusable);
with it on, an item's row does not depend on BATCH_SIZE, equals the tuner's episode on the sampler's views of the item, and the prompt is what it was;
the validation inside `train` runs no episode unless TPT_VALIDATION is set; TPT with MV_PREDICT or CLIP_ADAPTER is refused; a visual strategy logs and
ignores the switch."""
import logging

import pytest
import torch

from test_gpu_pool_cache import _strategy

pytestmark = pytest.mark.gpu
TPT = dict(TPT=True, TPT_VIEWS=8, TPT_RHO=0.5)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("GRIP_PSEUDOLABEL_MODE", "GRIP_SPLIT_TIER", "GRIP_SCREEN_STREAM"):
        monkeypatch.delenv(k, raising=False)


def test_switch_absent_is_the_parents_predict(tmp_path, monkeypatch):
    from grip_amd import tpt
    m, train, _ = _strategy("TextualFPL", tmp_path / "a", monkeypatch)
    m.define_model(m.classes)
    assert m.tpt_settings is None and m.test_time_tuner(m.classes) is None
    pred, logits = m.predict(train, m.classes)
    off, _, _ = _strategy("TextualFPL", tmp_path / "b", monkeypatch, TPT=False)
    off.define_model(off.classes)

    def boom(*a, **kw):
        raise AssertionError("a strategy without TPT built a tuner")
    monkeypatch.setattr(tpt, "TestTimeTuner", boom)
    pred2, logits2 = off.predict(train, off.classes)
    assert torch.equal(pred, pred2) and torch.equal(logits, logits2)
    # the parent's predict, written out: the cosine head of the frozen features and the inference text features
    from grip_amd.engine import cosine_head
    with torch.no_grad():
        img, txt = m.features(train.images.cuda(), m.classes)
        want = cosine_head(img, txt, m.scale(), want_probs=False)[0]
    assert torch.equal(logits, want.cpu()) and len(train) <= 24


def test_predict_with_tpt_does_not_depend_on_the_batch_size_and_restores_the_prompt(tmp_path, monkeypatch):
    from grip_amd import pseudolabels as pl
    m, train, _ = _strategy("TextualFPL", tmp_path, monkeypatch, **TPT)
    m.define_model(m.classes)
    assert m.tpt_settings["views"] == 8 and len(train) == 12
    before = m.model.prefix.detach().clone()
    out = {}
    for bs in (4, 8):
        m.config.BATCH_SIZE = bs
        out[bs] = m.predict(train, m.classes)
        assert torch.equal(m.model.prefix.detach(), before) and m.model.prefix.grad is None
    assert torch.equal(out[4][0], out[8][0]) and torch.equal(out[4][1], out[8][1])
    tuner = m.test_time_tuner(m.classes)
    assert tuner.episodes == 24 and tuner.keep == 4 and tuner.model is m.model
    # an item's row is the tuner's episode on the sampler's views of the item, alone
    files = list(train.filepaths)
    x = train.images.cuda().float().contiguous()
    for i in (0, 7, 11):
        vw = tuner.make_views(x[i:i + 1], files[i:i + 1])
        assert torch.equal(vw[0], x[i]), "view 0 is a bit-exact copy"
        feats = pl.encode_pool(m.clip_model.visual.tower, vw)
        assert torch.equal(tuner.tune(feats).cpu(), out[4][1][i])
    plain = _plain_predict(m, train)
    assert not torch.equal(plain[1], out[4][1]), "the episodes changed nothing"
    ids = torch.tensor([m.label_to_idx[c] for c in m.classes])
    assert torch.equal(out[4][0], ids[out[4][1].argmax(1)])


def _plain_predict(m, data):
    m._tpt_plain = True
    try:
        return m.predict(data, m.classes)
    finally:
        m._tpt_plain = False


@pytest.mark.parametrize("validate", [False, True])
def test_validation_inside_train_runs_episodes_only_on_request(tmp_path, monkeypatch, validate):
    m, train, unlabeled = _strategy("TextualFPL", tmp_path, monkeypatch, **TPT, **({"TPT_VALIDATION": True} if validate else {}))
    from grip_amd import tpt
    made = []
    real = tpt.TestTimeTuner

    def spy(*a, **kw):
        made.append(real(*a, **kw))
        return made[-1]
    monkeypatch.setattr(tpt, "TestTimeTuner", spy)
    m.train(train, train, only_seen=True)      # two epochs, each validated on the 12 shots
    episodes = sum(t.episodes for t in made)
    assert episodes == (2 * len(train) if validate else 0), episodes
    names, pred, _ = m.evaluation(train)       # evaluation uses TPT either way
    assert sum(t.episodes for t in made) == episodes + len(train) and len(pred) == len(names) == len(train)


@pytest.mark.parametrize("other", [dict(MV_PREDICT=True), dict(CLIP_ADAPTER=True)])
def test_tpt_with_mv_predict_or_clip_adapter_is_refused(tmp_path, monkeypatch, other):
    with pytest.raises(ValueError, match="TPT and " + next(iter(other))):
        _strategy("TextualFPL", tmp_path, monkeypatch, **TPT, **other)


def test_a_visual_strategy_logs_and_ignores_the_switch(tmp_path, monkeypatch, caplog):
    with caplog.at_level(logging.INFO):
        m, train, _ = _strategy("VisualFPL", tmp_path / "on", monkeypatch, **TPT)
    assert any("TPT is ignored by the image strategies" in r.getMessage() for r in caplog.records)
    assert m.tpt_settings is None
    m.define_model(m.classes)
    off, _, _ = _strategy("VisualFPL", tmp_path / "off", monkeypatch)
    off.define_model(off.classes)
    a, b = m.predict(train, m.classes), off.predict(train, off.classes)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
