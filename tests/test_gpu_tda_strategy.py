"""The test-time streaming cache through the strategies (`small` towers, the synthetic pool of test_gpu_pool_cache: 6 classes; the 12 labelled shots stand
in for a test set).  With TDA: True `predict` is, bit for bit, engine.stream_cache on the logits and the image features of the plain `predict` in dataset
order, whatever BATCH_SIZE; with TDA: False or the switch absent it is the plain `predict` and no cache object exists; the validation inside `train` runs
a stream only with TDA_VALIDATION.  One textual and one visual strategy."""
import pytest
import torch

from test_gpu_pool_cache import _strategy

pytestmark = pytest.mark.gpu
# queues that see evictions on 12 items of 6 classes, and windows that admit the small towers' near-uniform predictions
TDA = dict(TDA=True, TDA_POS_CAP=1, TDA_NEG_CAP=1, TDA_NEG_ENTROPY=(0.0, 1.0), TDA_NEG_MASK=(0.01, 1.0))


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("GRIP_PSEUDOLABEL_MODE", "GRIP_SPLIT_TIER", "GRIP_SCREEN_STREAM"):
        monkeypatch.delenv(k, raising=False)


def _plain(m, data):
    m._tda_plain = True
    try:
        return m.predict(data, m.classes)
    finally:
        m._tda_plain = False


@pytest.mark.parametrize("cls_name", ["TextualFPL", "VisualFPL"])
def test_predict_is_the_stream_over_the_plain_rows(tmp_path, monkeypatch, cls_name):
    from grip_amd import engine, tda
    m, train, _ = _strategy(cls_name, tmp_path / "on", monkeypatch, **TDA)
    m.define_model(m.classes)
    assert isinstance(m.tda, tda.StreamCache) and m.tda.settings["pos_cap"] == 1 and len(train) == 12
    plain_pred, plain = _plain(m, train)
    assert m.tda.streams == 0
    with torch.no_grad():
        feats = m.features(train.images.cuda(), m.classes)[0].detach().float().contiguous()
    want, plan = engine.stream_cache(plain.cuda().contiguous(), feats, **m.tda.settings)
    assert int(plan["counts"][0]) > 0 and not torch.equal(want.cpu(), plain), "the stream changed nothing"
    ids = torch.tensor([m.label_to_idx[c] for c in m.classes])
    for bs in (16, 5):
        m.config.BATCH_SIZE = bs
        pred, logits = m.predict(train, m.classes)
        assert torch.equal(logits, want.cpu()) and torch.equal(pred, ids[want.cpu().argmax(1)]), bs
    assert m.tda.streams == 2 and torch.equal(m.tda.plan["pos_leave"], plan["pos_leave"])
    # the switch off, or absent: the plain rows, bit for bit, and no cache object
    for name, kw in (("false", dict(TDA=False)), ("absent", {})):
        off, train2, _ = _strategy(cls_name, tmp_path / name, monkeypatch, **kw)
        off.define_model(off.classes)
        assert off.tda is None

        def boom(*a, **k):
            raise AssertionError("a strategy without TDA ran a stream")
        with monkeypatch.context() as mp:
            mp.setattr(engine, "stream_cache", boom)
            pred2, logits2 = off.predict(train2, off.classes)
        assert torch.equal(logits2, plain) and torch.equal(pred2, plain_pred), name


@pytest.mark.parametrize("validate", [False, True])
def test_validation_inside_train_runs_a_stream_only_on_request(tmp_path, monkeypatch, validate):
    m, train, _ = _strategy("TextualFPL", tmp_path, monkeypatch, **TDA, **({"TDA_VALIDATION": True} if validate else {}))
    m.train(train, train, only_seen=True)      # two epochs, each validated on the 12 shots
    assert m.tda.streams == (2 if validate else 0)
    names, pred, _ = m.evaluation(train)       # evaluation streams either way
    assert m.tda.streams == (3 if validate else 1) and len(pred) == len(names) == len(train)


def test_bad_settings_fail_when_the_strategy_is_built(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="pos_cap"):
        _strategy("TextualFPL", tmp_path, monkeypatch, TDA=True, TDA_POS_CAP=0)
