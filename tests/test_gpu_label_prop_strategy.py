"""LABEL_PROPAGATION through the strategies (`small` towers, the synthetic pool of test_gpu_pool_cache: 6 classes, 108 unlabeled images).  With the
switch on, a textual strategy's assign_pseudo_labels returns exactly the leaderboard over engine.label_propagate(head, knn_graph(embeddings)) of the
same embeddings, builds the graph once over two GRIP iterations and names its pickle `_lp_`; a visual strategy rebuilds the graph every pass.  With
the switch absent nothing moves: the lists are those of the plain head -> scan, with or without label_propagation(None) around the call."""
import glob
import os

import pytest
import torch

from test_gpu_pool_cache import _strategy

pytestmark = pytest.mark.gpu
LP = dict(LABEL_PROPAGATION=True, LP_K=8, LP_ALPHA=0.7, LP_GAMMA=20.0, LP_ITERS=5)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("GRIP_PSEUDOLABEL_MODE", "GRIP_SPLIT_TIER", "GRIP_SCREEN_STREAM"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture
def graphs(monkeypatch):
    """graphs() -> [(n, k)] of every engine.knn_graph call so far."""
    import grip_amd  # noqa: F401
    from grip_amd import engine
    calls, real = [], engine.knn_graph

    def counting(queries, base=None, k=16, self_offset=None):
        calls.append((queries.shape[0], k))
        return real(queries, base, k, self_offset)
    monkeypatch.setattr(engine, "knn_graph", counting)
    return lambda: list(calls)


def test_settings_reach_the_strategy(tmp_path, monkeypatch):
    from grip_amd import pseudolabels as pl
    m, _, _ = _strategy("TextualFPL", tmp_path / "a", monkeypatch, **LP)
    lp = m.label_prop
    assert isinstance(lp, pl.LabelPropagation) and (lp.k, lp.alpha, lp.gamma, lp.iters, lp.keep_graphs) == (8, 0.7, 20.0, 5, True)
    v, _, _ = _strategy("VisualFPL", tmp_path / "b", monkeypatch, LABEL_PROPAGATION=True)
    lp = v.label_prop
    assert (lp.k, lp.alpha, lp.gamma, lp.iters, lp.keep_graphs) == (16, 0.8, 10.0, 10, False)
    off, _, _ = _strategy("TextualFPL", tmp_path / "c", monkeypatch)
    assert off.label_prop is None and pl.propagation() is None


def test_textual_pass_is_the_leaderboard_over_the_propagated_probabilities(tmp_path, monkeypatch, graphs):
    from grip_amd import engine, pseudolabels as pl
    m, _, unlabeled = _strategy("TextualFPL", tmp_path, monkeypatch, **LP)
    m.define_model(m.classes)
    images, paths = unlabeled.images, list(unlabeled.filepaths)
    labels = [m.label_to_idx[c] for c in m.classes]
    emb, txt = m.trained_features(images, m.classes)
    _, probs, _, _ = engine.cosine_head(emb, txt.detach(), m.scale())
    idx, sim = engine.knn_graph(emb, k=8)
    z, pred = engine.label_propagate(probs, idx, sim, 0.7, 20.0, 5)
    assert idx.shape == (len(paths), 8) and not torch.equal(z, probs)
    want = pl.leaderboard(z.cpu().numpy(), pred.cpu().numpy(), paths, labels, 4)
    n0 = len(graphs())
    got = m.assign_pseudo_labels(4, unlabeled)      # (identical mode is the default: with a propagation installed the pass takes its plain branch)
    assert (list(got.filepaths), list(got.labels)) == (list(want[0]), list(want[1])) and len(want[0]) > 0
    assert graphs()[n0:] == [(len(paths), 8)] and pl.propagation() is None
    # the second pass over the same pool finds the graph
    unlabeled.filepaths, unlabeled.labels = list(paths), None
    again = m.assign_pseudo_labels(4, unlabeled)
    assert (list(again.filepaths), list(again.labels)) == (list(want[0]), list(want[1])) and len(graphs()) == n0 + 1
    # other features behind the same paths do not meet the kept graph: it is rebuilt from them, once
    other = emb.flip(0).contiguous()
    fresh = engine.knn_graph(other, k=8)
    n1 = len(graphs())
    assert torch.equal(m.label_prop.graph(other, paths)[0], fresh[0]) and len(graphs()) == n1 + 1
    assert torch.equal(m.label_prop.graph(other, paths)[0], fresh[0]) and len(graphs()) == n1 + 1


def _pickles(root):
    return sorted(os.path.basename(f) for f in glob.glob(os.path.join(str(root), "pseudolabels", "*_pseudolabels_*split_*.pickle")))


def test_textual_grip_builds_the_graph_once_and_names_its_pickle(tmp_path, monkeypatch, graphs):
    m, train, unlabeled = _strategy("TextualFPL", tmp_path, monkeypatch, STEP_QUANTILE=50, **LP)
    n = len(unlabeled)
    m.grip_train(train, None, unlabeled)           # two iterations: the frozen-CLIP pass, then a pass with the trained prompt
    assert graphs() == [(n, 8)] and m.label_prop.graphs_built == 1
    names = _pickles(tmp_path)
    assert len(names) == 1 and "_pseudolabels_lp_split_" in names[0], names


def test_visual_grip_rebuilds_the_graph_every_pass(tmp_path, monkeypatch, graphs):
    m, train, unlabeled = _strategy("VisualFPL", tmp_path, monkeypatch, STEP_QUANTILE=50, **LP)
    n = len(unlabeled)
    m.grip_train(train, None, unlabeled)
    assert graphs() == [(n, 8), (n, 8)] and m.label_prop.graphs_built == 2
    assert all("_pseudolabels_lp_split_" in f for f in _pickles(tmp_path)) and len(_pickles(tmp_path)) == 1


def test_switch_absent_changes_nothing(tmp_path, monkeypatch, graphs):
    from grip_amd import engine, pseudolabels as pl
    monkeypatch.setenv("GRIP_PSEUDOLABEL_MODE", "f16")
    m, train, unlabeled = _strategy("TextualFPL", tmp_path, monkeypatch)
    m.define_model(m.classes)
    images, paths = unlabeled.images, list(unlabeled.filepaths)
    labels = [m.label_to_idx[c] for c in m.classes]
    emb, txt = m.trained_features(images, m.classes)
    _, probs, am_l, _ = engine.cosine_head(emb, txt.detach(), m.scale())
    want = pl.leaderboard(probs.cpu().numpy(), am_l.cpu().numpy(), paths, labels, 4)       # the plain head -> scan
    plain = m.assign_pseudo_labels(4, unlabeled)
    got = (list(plain.filepaths), list(plain.labels))
    unlabeled.filepaths, unlabeled.labels = list(paths), None
    with pl.label_propagation(None):
        none = m.assign_pseudo_labels(4, unlabeled)
    assert got == (list(none.filepaths), list(none.labels)) == (list(want[0]), list(want[1])) and len(want[0]) > 0
    unlabeled.filepaths, unlabeled.labels = list(paths), None
    m.create_training_dataset(train, unlabeled)
    names = _pickles(tmp_path)
    assert graphs() == [] and len(names) == 1 and "_lp_" not in names[0], names
