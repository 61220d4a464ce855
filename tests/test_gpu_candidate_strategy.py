"""CANDIDATE_PSEUDOLABELS through the strategies (`small` towers, the synthetic pool of test_gpu_soft_strategy.py: 6 classes, 12 labelled shots, 60 unlabeled
images).  With the switch on, the training list is the pool rows with a non-empty candidate set -- the NumPy reference's sets on the matrix the kernel was
given -- each once, in pool order, labelled with the set's first member; the pickle is named `_cpl_`; a later pass overwrites the store in place and the
next graph replay trains on it; the graphed and the eager loop agree bit for bit; in TRZSL the sets live on the unseen columns; the first step's loss and
gradient are the float64 ones under the bound of tests/candidate_ref.py.  The switch raises together with SOFT_PSEUDOLABELS or LABEL_SMOOTHING, composes
with BALANCED_PSEUDOLABELS, and with the switch absent nothing moves: lists, pickle name and trained prompt are those of the parent's code path."""
import numpy as np
import pytest
import torch

import candidate_ref as R
from test_gpu_soft_strategy import _env, _pickles, _strategy  # noqa: F401  (_env: the autouse environment fixture)

pytestmark = pytest.mark.gpu
CPL = dict(CANDIDATE_PSEUDOLABELS=True)
OT = dict(BALANCED_PSEUDOLABELS=True)


@pytest.fixture
def cand_calls(monkeypatch):
    """{"select": [(probs, claim, tau, combine, outputs)], "ce": [(operands, (loss, grad))]} of every engine.candidate_select / candidate_ce call."""
    import grip_amd  # noqa: F401
    from grip_amd import engine
    seen = {"select": [], "ce": []}
    real_select, real_ce = engine.candidate_select, engine.candidate_ce
    keep = lambda t: t.detach().clone() if torch.is_tensor(t) else t      # noqa: E731

    def candidate_select(probs, claim, tau=0.99, combine="intersection"):
        out = real_select(probs, claim, tau, combine)
        seen["select"].append((keep(probs), claim, tau, combine, tuple(keep(t) for t in out)))
        return out

    def candidate_ce(logits, labels, row_weight, cand=None, cand_row=None, col_map=None):
        out = real_ce(logits, labels, row_weight, cand, cand_row, col_map)
        seen["ce"].append((tuple(keep(t) for t in (logits, labels, row_weight, cand, cand_row, col_map)), tuple(keep(t) for t in out)))
        return out
    monkeypatch.setattr(engine, "candidate_select", candidate_select)
    monkeypatch.setattr(engine, "candidate_ce", candidate_ce)
    return seen


def _expected_lists(call, pool_paths, class_ids):
    """The lists the reference selection gives on the operands of a recorded candidate_select call; asserts the kernel's outputs on the way."""
    probs, claim, tau, combine, (mask, count, label, thr) = call
    want = R.select(probs.cpu().numpy(), claim, tau, combine)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip((mask, count, label, thr), want))
    keep = [i for i in range(len(pool_paths)) if want[1][i] > 0]
    return [pool_paths[i] for i in keep], [class_ids[int(want[2][i])] for i in keep], want


@pytest.mark.parametrize("cls_name,paradigm", [("TextualFPL", "ssl"), ("VisualFPL", "ul")])
def test_the_training_list_is_the_rows_with_a_set_and_the_steps_train_on_the_sets(tmp_path, monkeypatch, cand_calls, cls_name, paradigm):
    from grip_amd import pseudolabels as pl, steps
    m, train, unlabeled = _strategy(tmp_path, monkeypatch, paradigm=paradigm, cls_name=cls_name, GRAPH_STEPS=False, **CPL)
    pool_paths = list(unlabeled.filepaths)
    n_shots = len(train.filepaths)
    assert isinstance(m.candidate_store, pl.CandidateStore) and m.candidate_store.mask is None and m.soft_targets(m.classes) is None
    data = m.create_training_dataset(train, unlabeled)
    ids = [m.label_to_idx[c] for c in m.classes]
    (call,) = cand_calls["select"]
    assert call[1:4] == (min(60, 2 * 3), 0.99, "intersection") and tuple(call[0].shape) == (60, 6)       # claim = CPL_SLOTS x N_PSEUDOSHOTS
    files, labels, want = _expected_lists(call, pool_paths, ids)
    n_pseudo = len(files)
    assert 0 < n_pseudo <= 60 and len(set(files)) == n_pseudo                                              # each image once
    assert list(data.filepaths)[:n_pseudo] == files and [int(l) for l in data.labels[:n_pseudo]] == labels
    assert len(data.filepaths) == n_pseudo + (0 if paradigm == "ul" else n_shots)
    store = m.candidate_store
    assert store.records == 1 and np.array_equal(store.mask.cpu().numpy(), want[0]) and store.class_labels == tuple(ids) and pl.candidates() is None
    names = _pickles(tmp_path)
    assert len(names) == 1 and "_pseudolabels_cpl_split_" in names[0]
    # the steps: pseudolabelled rows point at their mask row, labelled shots are hard rows; the first step against float64
    m.define_model(m.classes)
    classes, idx, lut = m._class_space(False)
    soft = m.soft_targets(classes)
    assert isinstance(soft, steps.CandidateTargets) and soft.mask is store.mask and soft.col_map.tolist() == list(range(6))
    m._train_epoch(m._loader(data, True))
    assert len(cand_calls["ce"]) == len(m._loader(data, True))
    (logits, labs, w, cand, row, cmap), (loss, grad) = cand_calls["ce"][0]
    _, _, _, label0, names0 = next(iter(m._loader(data, True)))
    assert row.tolist() == [pool_paths.index(n) if n in m.check_unlabeled else -1 for n in names0] and (row >= 0).any()
    assert torch.equal(cand, store.mask)
    ref = R.candidate_ce64(logits, labs, w, cand, row, cmap)
    ratio = R.check(ref, loss, grad)
    print(f"{cls_name}: first step, worst |err| / bound = {ratio:.3f} over {tuple(grad.shape)} gradient elements, {int((row >= 0).sum())} candidate rows, "
          f"mean set size {float(want[1][want[1] > 0].mean()):.2f}")
    assert not bool(ref["empty"].any())                                                                    # a listed row has a set
    # a second pass does not read the pickle it finds: it runs, records into the same buffer and rewrites the file
    at = store.mask.data_ptr()
    m2, train2, unl2 = _strategy(tmp_path, monkeypatch, paradigm=paradigm, cls_name=cls_name, GRAPH_STEPS=False, **CPL)
    m2.candidate_store = store
    data2 = m2.create_training_dataset(train2, unl2)
    assert store.records == 2 and store.mask.data_ptr() == at and list(data2.filepaths)[:n_pseudo] == files and len(cand_calls["select"]) == 2


@pytest.mark.parametrize("cls_name,paradigm,kw", [("TextualFPL", "ssl", {}), ("VisualFPL", "ul", {"CPL_COMBINE": "union", "CPL_TAU": 0.9}),
                                                  ("MultimodalFPL", "trzsl", OT)])
def test_graphed_loop_equals_eager_loop_and_a_replay_trains_on_the_overwritten_sets(tmp_path, monkeypatch, cand_calls, cls_name, paradigm, kw):
    """Two epochs with the step replayed from a HIP graph (batches of 16 and a ragged last one through the eager fallback) against GRAPH_STEPS False.
    Between the epochs the store is overwritten in place with other sets (every class for every image: the pseudolabelled rows then carry no loss): the
    graph is not rebuilt, and its next replays give what the eager loop gives on the new sets."""
    out = []
    for graph in (True, False):
        m, train, unlabeled = _strategy(tmp_path / str(graph), monkeypatch, paradigm=paradigm, cls_name=cls_name, GRAPH_STEPS=graph, **CPL, **kw)
        pool_paths = list(unlabeled.filepaths)
        data = m.create_training_dataset(train, unlabeled)
        m.define_model(m.classes)
        loader = m._loader(data, True)
        n0 = len(cand_calls["ce"])
        stats = [m._train_epoch(loader, epoch=0)]
        store = m.candidate_store
        at, step = store.mask.data_ptr(), getattr(m, "_gstep", None)
        cz = len(store.class_labels)
        store.record(pool_paths, list(store.class_labels), torch.from_numpy(R.pack(np.ones((len(pool_paths), cz), dtype=bool)).copy()).cuda())
        stats.append(m._train_epoch(loader, epoch=1))
        assert store.mask.data_ptr() == at and getattr(m, "_gstep", None) is step and (step is not None) == graph
        assert len(cand_calls["ce"]) > n0 and all(c[0][3] is not None for c in cand_calls["ce"][n0:])
        out.append((stats, [p.detach().clone() for p in m.model.parameters() if p.requires_grad]))
    (s_g, p_g), (s_e, p_e) = out
    assert s_g == s_e and all(torch.equal(a, b) for a, b in zip(p_g, p_e)) and all(np.isfinite(s[0]) for s in s_g)
    assert s_g[1][0] < s_g[0][0]          # full sets: only the labelled rows (none in ul) still carry a loss


def test_trzsl_sets_live_on_the_unseen_columns(tmp_path, monkeypatch, cand_calls):
    m, train, unlabeled = _strategy(tmp_path, monkeypatch, paradigm="trzsl", GRAPH_STEPS=False, **CPL)
    pool_paths = list(unlabeled.filepaths)
    data = m.create_training_dataset(train, unlabeled)
    unseen_ids = [m.label_to_idx[c] for c in m.unseen_classes]
    store = m.candidate_store
    assert tuple(store.mask.shape) == (60, 1) and store.class_labels == tuple(unseen_ids) and tuple(cand_calls["select"][0][0].shape) == (60, 3)
    files, labels, _ = _expected_lists(cand_calls["select"][0], pool_paths, unseen_ids)
    assert list(data.filepaths)[:len(files)] == files and [int(l) for l in data.labels[:len(files)]] == labels and set(labels) <= set(unseen_ids)
    m.define_model(m.classes)
    classes, ids, lut = m._class_space(False)
    soft = m.soft_targets(classes)
    assert soft.col_map.tolist() == [classes.index(c) for c in m.unseen_classes]
    seen_cols = [classes.index(c) for c in m.seen_classes]
    m._train_epoch(m._loader(data, True))
    checked = 0
    for (_, _, _, label, names), ((logits, labs, w, cand, row, cmap), (loss, grad)) in zip(m._loader(data, True), cand_calls["ce"]):
        is_pseudo = torch.tensor([int(l) in unseen_ids for l in label.tolist()], device="cuda")
        assert torch.equal(row >= 0, is_pseudo)                           # trzsl: a pseudolabelled row is one with an unseen label
        R.check(R.candidate_ce64(logits, labs, w, cand, row, cmap), loss, grad)
        _, member = R.members(cand, row, cmap, *logits.shape)
        assert not bool(member[:, seen_cols].any())                       # no set holds a seen class ...
        assert (grad[is_pseudo][:, seen_cols] >= 0).all()                 # ... so nothing pulls a pseudolabelled row towards one
        checked += int(is_pseudo.sum())
    assert checked == len(files) > 0
    assert m.soft_targets(m.seen_classes, only_seen=True) is None         # only_seen training has no pseudo rows: the hard path


def test_the_switch_raises_with_soft_rows_or_smoothing_and_checks_its_settings(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="CANDIDATE_PSEUDOLABELS"):
        _strategy(tmp_path, monkeypatch, SOFT_PSEUDOLABELS=True, LABEL_PROPAGATION=True, LP_K=8, **CPL)
    with pytest.raises(ValueError, match="CANDIDATE_PSEUDOLABELS"):
        _strategy(tmp_path, monkeypatch, LABEL_SMOOTHING=0.1, **CPL)
    with pytest.raises(ValueError, match="tau = 0"):
        _strategy(tmp_path, monkeypatch, CPL_TAU=0.0, **CPL)
    with pytest.raises(ValueError, match="slots = 0"):
        _strategy(tmp_path, monkeypatch, CPL_SLOTS=0, **CPL)
    with pytest.raises(ValueError, match="combine = 'both'"):
        _strategy(tmp_path, monkeypatch, CPL_COMBINE="both", **CPL)


def test_it_composes_with_balanced_pseudolabels(tmp_path, monkeypatch, cand_calls):
    m, train, unlabeled = _strategy(tmp_path, monkeypatch, GRAPH_STEPS=False, CPL_SLOTS=3, **CPL, **OT)
    pool_paths = list(unlabeled.filepaths)
    data = m.create_training_dataset(train, unlabeled)
    (call,) = cand_calls["select"]
    assert call[1] == 9 and torch.allclose(call[0].sum(1), torch.ones(60, device="cuda"), atol=1e-5)
    mass, _ = m.balanced.state
    assert torch.allclose(call[0].sum(0), mass, rtol=1e-4)                # the selection ran on the balanced Q, not on the head's probabilities
    files, labels, _ = _expected_lists(call, pool_paths, [m.label_to_idx[c] for c in m.classes])
    assert list(data.filepaths)[:len(files)] == files and [int(l) for l in data.labels[:len(files)]] == labels
    names = _pickles(tmp_path)
    assert len(names) == 1 and "_pseudolabels_cpl_ot_split_" in names[0]
    m.define_model(m.classes)
    loss, acc = m._train_epoch(m._loader(data, True))
    assert np.isfinite(loss) and len(cand_calls["ce"]) == len(m._loader(data, True))


def test_switch_absent_changes_nothing(tmp_path, monkeypatch, cand_calls):
    """The first GRIP iteration (pseudolabels from frozen CLIP, two epochs) with the switch absent, against the same iteration with the new plumbing taken
    out (steps.step_loss := the parent's WeightedCEFn call, pl.candidate_sets := a context that installs nothing): lists, pickle name and trained prompt
    are bit-equal, no store exists and neither candidate kernel is ever called."""
    import contextlib

    from grip_amd import pseudolabels as pl, steps
    out = []
    for parent in (False, True):
        if parent:
            monkeypatch.setattr(steps, "step_loss", lambda logits, labels, row_weight, soft=None, soft_row=None: steps.WeightedCEFn.apply(logits, labels, row_weight))
            monkeypatch.setattr(pl, "candidate_sets", lambda selection, store: contextlib.nullcontext())
        m, train, unlabeled = _strategy(tmp_path / str(parent), monkeypatch)
        assert m.candidate_store is None and m.candidate_selection is None
        data = m.create_training_dataset(train, unlabeled)
        m.define_model(m.classes)
        loader = m._loader(data, True)
        stats = [m._train_epoch(loader, epoch=e) for e in range(2)]
        out.append((list(data.filepaths), list(data.labels), _pickles(tmp_path / str(parent)), stats, m.unwrap_model().prefix.detach().clone()))
    assert out[0][:4] == out[1][:4] and torch.equal(out[0][4], out[1][4]) and cand_calls == {"select": [], "ce": []}
    assert len(out[0][2]) == 1 and "_pseudolabels_split_" in out[0][2][0]
