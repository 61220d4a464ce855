"""SOFT_PSEUDOLABELS and LABEL_SMOOTHING through the strategies (`small` towers, a synthetic pool of 6 classes: 12 labelled shots, 60 unlabeled images).
With the switch on and each of the three transductions, the lists are the switch-off lists, the soft_row of every batch points at the rows the store
recorded for those file names (-1 for the labelled shots), and the first step's logits gradient is the float64 gradient on those targets under the bound
of tests/soft_ce_ref.py.  In TRZSL the seen columns of a soft target are exactly 0.  SOFT_PSEUDOLABELS without a transduction raises, a duplicated base
name raises when it is asked about, LABEL_SMOOTHING works alone, the graphed and the eager loop agree bit for bit, and with both switches absent nothing
moves: lists, pickle name and trained prompt are those of the parent's code path and grip_soft_ce is never called.

The pool is methods.main.synthetic_pool(6, 12, 64, seed 23), the seed of test_gpu_pool_cache._strategy: every check here compares two runs of the same
deterministic kernels, or a kernel with float64 on its own operands, so no seed had to be looked for (test_gpu_sinkhorn_strategy.py chose its seeds for
a float64 RANKING to be decided; nothing is ranked in float64 here)."""
import glob
import os

import pytest
import torch

import soft_ce_ref as R

pytestmark = pytest.mark.gpu
LP = dict(LABEL_PROPAGATION=True, LP_K=8)
GMM = dict(TRANSDUCTIVE_GMM=True, GMM_K=4, GMM_LAMBDA=2.0, GMM_ITERS=1, GMM_Z_ITERS=1)
OT = dict(BALANCED_PSEUDOLABELS=True)
SOFT = dict(SOFT_PSEUDOLABELS=True, SOFT_TEMPERATURE=0.5)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("GRIP_PSEUDOLABEL_MODE", "GRIP_SPLIT_TIER", "GRIP_SCREEN_STREAM"):
        monkeypatch.delenv(k, raising=False)


def _strategy(tmp_path, monkeypatch, paradigm="ssl", cls_name="TextualFPL", **kw):
    import grip_amd  # noqa: F401
    from grip_amd import methods
    from grip_amd.data import ImagePool, TensorPoolDataset
    from grip_amd.methods.main import synthetic_pool
    from test_gpu_strategies import _conf
    os.makedirs(tmp_path, exist_ok=True)
    monkeypatch.chdir(tmp_path)
    classes, files, images, names = synthetic_pool(6, 12, 64, 23)
    l2i = {c: i for i, c in enumerate(classes)}
    seen, unseen = (classes[:3], classes[3:]) if paradigm == "trzsl" else (classes, classes)
    shots = [i for i in range(len(files)) if i % 12 < 2 and names[i] in seen]
    rest = [i for i in range(len(files)) if i % 12 >= 2]
    pool = ImagePool(files, images.cuda())
    train = TensorPoolDataset([files[i] for i in shots], pool, labels=[names[i] for i in shots], label_map=l2i)
    unlabeled = TensorPoolDataset([files[i] for i in rest], pool, labels=None, label_map=l2i)
    conf = _conf(MODEL="grip_" + cls_name.lower(), LEARNING_PARADIGM=paradigm, EPOCHS=2, BATCH_SIZE=16, N_PSEUDOSHOTS=3, TEXT_PREFIX_SIZE=4, VISION_PREFIX_SIZE=4,
                 **kw)
    m = getattr(methods, cls_name)(conf, l2i, "", classes, seen, unseen, "cuda")
    return m, train, unlabeled


def _pickles(root):
    return sorted(os.path.basename(f) for f in glob.glob(os.path.join(str(root), "pseudolabels", "*_pseudolabels_*split_*.pickle")))


@pytest.fixture
def soft_calls(monkeypatch):
    """[(operands of the call, (loss, grad))] of every engine.soft_ce call, tensors cloned."""
    import grip_amd  # noqa: F401
    from grip_amd import engine
    seen, real = [], engine.soft_ce

    def soft_ce(logits, labels, row_weight, soft=None, soft_row=None, col_map=None, temperature=1.0, smoothing=0.0, want_target=False):
        out = real(logits, labels, row_weight, soft, soft_row, col_map, temperature, smoothing, want_target)
        keep = lambda t: t.detach().clone() if torch.is_tensor(t) else t      # noqa: E731
        seen.append((tuple(keep(t) for t in (logits, labels, row_weight, soft, soft_row, col_map)) + (temperature, smoothing), tuple(keep(t) for t in out)))
        return out
    monkeypatch.setattr(engine, "soft_ce", soft_ce)
    return seen


@pytest.mark.parametrize("name,trans", [("lp", LP), ("gmm", GMM), ("ot", OT)])
def test_switch_on_keeps_the_lists_and_trains_on_the_recorded_rows(tmp_path, monkeypatch, soft_calls, name, trans):
    from grip_amd import pseudolabels as pl
    m_off, train_off, unl_off = _strategy(tmp_path / "off", monkeypatch, **trans)
    assert m_off.soft_store is None and m_off.soft_targets(m_off.classes) is None
    data_off = m_off.create_training_dataset(train_off, unl_off)
    lists_off = (list(data_off.filepaths), list(data_off.labels))
    m, train, unlabeled = _strategy(tmp_path / "on", monkeypatch, GRAPH_STEPS=False, **trans, **SOFT)
    pool_paths = list(unlabeled.filepaths)
    assert isinstance(m.soft_store, pl.SoftTargetStore) and m.soft_store.matrix is None
    data = m.create_training_dataset(train, unlabeled)
    assert (list(data.filepaths), list(data.labels)) == lists_off and _pickles(tmp_path / "on") == _pickles(tmp_path / "off") and len(lists_off[0]) > 12
    store = m.soft_store
    assert store.records == 1 and tuple(store.matrix.shape) == (len(pool_paths), 6) and store.class_labels == tuple(m.label_to_idx[c] for c in m.classes)
    assert pl.soft_target_store() is None and soft_calls == []
    # a second pass does not read the pickle it finds (a loaded list has no matrix): it runs, records again into the same buffer and rewrites the file
    at, before = store.matrix.data_ptr(), store.matrix.clone()
    m2, train2, unl2 = _strategy(tmp_path / "on", monkeypatch, GRAPH_STEPS=False, **trans, **SOFT)
    m2.soft_store = store
    data2 = m2.create_training_dataset(train2, unl2)
    assert store.records == 2 and store.matrix.data_ptr() == at and torch.equal(store.matrix, before) and list(data2.filepaths) == lists_off[0]
    # the batches: pseudolabelled rows point at their pool row, labelled shots are hard rows
    m2.define_model(m2.classes)
    classes, ids, lut = m2._class_space(False)
    soft = m2.soft_targets(classes)
    assert soft.matrix is store.matrix and soft.temperature == 0.5 and soft.smoothing == 0.0 and soft.col_map.tolist() == list(range(6))
    n_pseudo = 0
    for _, _, _, label, names in m2._loader(data2, True):
        rows = m2.soft_rows(soft, label.tolist(), names).tolist()
        for n, r in zip(names, rows):
            assert r == (pool_paths.index(n) if n in m2.check_unlabeled else -1), (n, r)
            n_pseudo += r >= 0
    assert n_pseudo == sum(f in m2.check_unlabeled for f in data2.filepaths) >= len(m2.check_unlabeled) > 0      # (the scan may list an image under two classes)
    # the first step's gradient against float64 on those targets
    m2._train_epoch(m2._loader(data2, True))
    assert len(soft_calls) == len(m2._loader(data2, True))
    (logits, labels, w, z, row, cmap, temperature, eps), (loss, grad) = soft_calls[0]
    _, _, _, label0, names0 = next(iter(m2._loader(data2, True)))
    assert row.tolist() == m2.soft_rows(soft, label0.tolist(), names0).tolist() and (row >= 0).any() and (row < 0).any()
    assert z.data_ptr() != store.matrix.data_ptr() and torch.equal(z, store.matrix) and temperature == 0.5 and eps == 0.0
    ratio = R.check(R.soft_ce64(logits, labels, w, z, row, cmap, R.inv_temperature(temperature), eps), loss, grad)
    print(f"{name}: first step, worst |err| / bound = {ratio:.3f} over {tuple(grad.shape)} gradient elements, {int((row >= 0).sum())} soft rows")
    hard = R.soft_ce64(logits, labels, w)["grad"]
    assert (grad.double() - hard).abs().max() > 1e-4, "the soft rows must have moved the gradient away from the hard-label one"


def test_trzsl_soft_targets_are_exactly_zero_on_the_seen_columns(tmp_path, monkeypatch):
    from grip_amd import engine
    m, train, unlabeled = _strategy(tmp_path, monkeypatch, paradigm="trzsl", **LP, **SOFT)
    data = m.create_training_dataset(train, unlabeled)
    unseen_ids = [m.label_to_idx[c] for c in m.unseen_classes]
    assert tuple(m.soft_store.matrix.shape) == (60, 3) and m.soft_store.class_labels == tuple(unseen_ids)
    m.define_model(m.classes)
    classes, ids, lut = m._class_space(False)
    soft = m.soft_targets(classes)
    assert soft.col_map.tolist() == [classes.index(c) for c in m.unseen_classes]
    seen_cols = [classes.index(c) for c in m.seen_classes]
    checked = 0
    for img, _, _, label, names in m._loader(data, True):
        rows = m.soft_rows(soft, label.tolist(), names)
        is_pseudo = torch.tensor([int(l) in unseen_ids for l in label.tolist()], device="cuda")
        assert torch.equal(rows >= 0, is_pseudo)                      # trzsl: a pseudolabelled row is one with an unseen label
        logits = torch.randn(len(names), len(classes), device="cuda")
        w = m.row_weights(label.tolist(), names).cuda()
        _, _, target = engine.soft_ce(logits, lut[label.cuda()], w, soft.matrix, rows, soft.col_map, soft.temperature, soft.smoothing, want_target=True)
        assert (target[is_pseudo][:, seen_cols] == 0).all() and torch.allclose(target[is_pseudo].sum(1), torch.ones(int(is_pseudo.sum()), device="cuda"), atol=1e-5)
        onehot = torch.nn.functional.one_hot(lut[label.cuda()], len(classes)).float()
        assert torch.equal(target[~is_pseudo], onehot[~is_pseudo])      # labelled rows keep their one-hot
        checked += int(is_pseudo.sum())
    assert checked == sum(f in m.check_unlabeled for f in data.filepaths) >= len(m.check_unlabeled) > 0
    assert m.soft_targets(m.seen_classes, only_seen=True) is None        # only_seen training has no pseudo rows: the hard path


def test_soft_pseudolabels_need_a_transduction_and_valid_settings(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="SOFT_PSEUDOLABELS needs"):
        _strategy(tmp_path, monkeypatch, SOFT_PSEUDOLABELS=True)
    with pytest.raises(ValueError, match="SOFT_TEMPERATURE"):
        _strategy(tmp_path, monkeypatch, SOFT_PSEUDOLABELS=True, SOFT_TEMPERATURE=0.0, **LP)
    with pytest.raises(ValueError, match="LABEL_SMOOTHING"):
        _strategy(tmp_path, monkeypatch, LABEL_SMOOTHING=1.0)


def test_a_duplicated_base_name_raises_when_it_is_asked_about(tmp_path, monkeypatch):
    m, train, unlabeled = _strategy(tmp_path, monkeypatch, **LP, **SOFT)
    paths = ["a/one.jpg", "b/one.jpg", "a/two.jpg"]
    m.soft_store.record(paths, [m.label_to_idx[c] for c in m.classes], torch.full((3, 6), 1 / 6, device="cuda"))
    m.check_unlabeled = {"one.jpg", "two.jpg"}
    soft = m.soft_targets(m.classes)
    assert m.soft_rows(soft, [0, 1], ["two.jpg", "shot.jpg"]).tolist() == [2, -1]
    with pytest.raises(ValueError, match="names two rows"):
        m.soft_rows(soft, [0, 1], ["two.jpg", "one.jpg"])


@pytest.mark.parametrize("cls_name,paradigm,kw", [("TextualFPL", "ssl", {**LP, **SOFT}), ("VisualFPL", "ul", {**LP, **SOFT, "LABEL_SMOOTHING": 0.1}),
                                                  ("MultimodalFPL", "trzsl", {**OT, **SOFT}), ("TextualFPL", "ssl", {"LABEL_SMOOTHING": 0.1})])
def test_graphed_loop_equals_eager_loop(tmp_path, monkeypatch, soft_calls, cls_name, paradigm, kw):
    """_train_epoch with the step replayed from a HIP graph (batches of 16 and a ragged last one through the eager fallback) against GRAPH_STEPS False:
    the same losses, accuracies and trained parameters, with soft rows, with smoothing on top, and with LABEL_SMOOTHING alone."""
    out = []
    for graph in (True, False):
        m, train, unlabeled = _strategy(tmp_path / str(graph), monkeypatch, paradigm=paradigm, cls_name=cls_name, GRAPH_STEPS=graph, **kw)
        data = m.create_training_dataset(train, unlabeled)
        m.define_model(m.classes)
        loader = m._loader(data, True)
        n0 = len(soft_calls)
        stats = [m._train_epoch(loader, epoch=e) for e in range(2)]
        assert len(soft_calls) > n0 and all(c[0][7] == kw.get("LABEL_SMOOTHING", 0.0) for c in soft_calls[n0:])
        assert all((c[0][3] is None) == ("SOFT_PSEUDOLABELS" not in kw) for c in soft_calls[n0:])
        out.append((stats, [p.detach().clone() for p in m.model.parameters() if p.requires_grad]))
    (s_g, p_g), (s_e, p_e) = out
    assert s_g == s_e and all(torch.equal(a, b) for a, b in zip(p_g, p_e)) and all(torch.isfinite(torch.tensor(s[0])) for s in s_g)


def test_switches_absent_change_nothing(tmp_path, monkeypatch, soft_calls):
    """The first GRIP iteration (pseudolabels from frozen CLIP, two epochs) with both switches absent, against the same iteration with the new plumbing
    taken out (steps.step_loss := the parent's WeightedCEFn call, pl.soft_targets := a context that installs nothing): lists, pickle name and
    trained prompt are bit-equal, no store exists and grip_soft_ce is never called."""
    import contextlib

    from grip_amd import pseudolabels as pl, steps
    out = []
    for parent in (False, True):
        if parent:
            monkeypatch.setattr(steps, "step_loss", lambda logits, labels, row_weight, soft=None, soft_row=None: steps.WeightedCEFn.apply(logits, labels, row_weight))
            monkeypatch.setattr(pl, "soft_targets", lambda store: contextlib.nullcontext())
        m, train, unlabeled = _strategy(tmp_path / str(parent), monkeypatch, **LP)
        assert m.soft_store is None and m.label_smoothing == 0.0
        data = m.create_training_dataset(train, unlabeled)
        m.define_model(m.classes)
        loader = m._loader(data, True)
        stats = [m._train_epoch(loader, epoch=e) for e in range(2)]
        out.append((list(data.filepaths), list(data.labels), _pickles(tmp_path / str(parent)), stats, m.unwrap_model().prefix.detach().clone()))
    assert out[0][:4] == out[1][:4] and torch.equal(out[0][4], out[1][4]) and soft_calls == []
    assert len(out[0][2]) == 1 and "_pseudolabels_lp_split_" in out[0][2][0]
