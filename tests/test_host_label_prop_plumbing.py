"""Host plumbing of the label-propagation switch (CPU): the context manager nests and restores, LabelPropagation validates its settings, the
pickle of a propagated pass carries its own name, and the four new entry points are part of the ABI on both sides."""
import os
import re

import pytest

from conftest import REPO

NEW_EXPORTS = ("grip_knn_graph_workspace", "grip_knn_graph", "grip_label_propagate_workspace", "grip_label_propagate")


def _pl():
    import grip_amd  # noqa: F401
    from grip_amd import pseudolabels as pl
    return pl


def test_context_manager_nests_and_restores():
    pl = _pl()
    assert pl.propagation() is None
    a, b = pl.LabelPropagation(), pl.LabelPropagation(k=4, alpha=0.5, gamma=0.0, iters=1)
    with pl.label_propagation(a) as got:
        assert got is a and pl.propagation() is a
        with pl.label_propagation(b):
            assert pl.propagation() is b
            with pl.label_propagation(None) as none:        # None: a no-op, like pool_cache(None)
                assert none is None and pl.propagation() is b
        assert pl.propagation() is a
        with pytest.raises(RuntimeError):
            with pl.label_propagation(b):
                raise RuntimeError("inside")
        assert pl.propagation() is a
    assert pl.propagation() is None
    with pytest.raises(TypeError):
        with pl.label_propagation(16):
            pass
    assert pl.propagation() is None


def test_defaults_and_validation():
    pl = _pl()
    lp = pl.LabelPropagation()
    assert (lp.k, lp.alpha, lp.gamma, lp.iters, lp.keep_graphs) == (16, 0.8, 10.0, 10, False)
    pl.LabelPropagation(k=32, alpha=0.0, gamma=0.0, iters=1)
    for bad in (dict(alpha=1.0), dict(alpha=1.5), dict(alpha=-0.1), dict(k=33), dict(k=0), dict(iters=0), dict(gamma=-1.0), dict(gamma=float("inf"))):
        with pytest.raises(ValueError):
            pl.LabelPropagation(**bad)


def test_pickle_name_carries_lp_only_while_installed(tmp_path, monkeypatch):
    """pseudolabel_top_k reads `..._pseudolabels_lp_split_...` while a propagation is installed and the reference's name otherwise: a cached list of one
    kind is never taken for the other (the files are planted: nothing is computed)."""
    import pickle
    from types import SimpleNamespace

    pl = _pl()
    from grip_amd.utils.clip_pseudolabels import pseudolabel_top_k
    monkeypatch.chdir(tmp_path)
    os.makedirs("pseudolabels")
    cfg = SimpleNamespace(LEARNING_PARADIGM="ul", MODEL="textual_fpl")
    plain, prop = "pseudolabels/D_ViT-B32_ul_textual_fpl_2_pseudolabels_split_7.pickle", "pseudolabels/D_ViT-B32_ul_textual_fpl_2_pseudolabels_lp_split_7.pickle"
    for name, tag in ((plain, "plain"), (prop, "lp")):
        with open(name, "wb") as f:
            pickle.dump({"filepaths": [tag], "labels": [0]}, f)

    def load():
        ds = SimpleNamespace(filepaths=["x"], labels=[1])
        return pseudolabel_top_k(cfg, "D", 2, "", ds, [], None, None, {}, "cpu", "ViT-B/32", 7).filepaths
    assert load() == ["plain"]
    with pl.label_propagation(pl.LabelPropagation()):
        assert load() == ["lp"]
    assert load() == ["plain"]


def test_abi_lists_the_four_entry_points():
    import grip_amd  # noqa: F401
    from grip_amd import native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "grip_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(grip_[a-z_]+)\s*\(", text))
    for name in NEW_EXPORTS:
        assert name in declared and name in native.EXPORTS, name
    assert declared == set(native.EXPORTS)
    assert native.ABI_VERSION == 9
    lib = native.lib()
    for name in NEW_EXPORTS:
        assert getattr(lib, name) is not None
