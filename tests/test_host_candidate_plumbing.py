"""Host plumbing of the candidate-set switch (CPU): CandidateStore keeps SoftTargetStore's contract (it owns its buffer, rows by base name, column maps per
class list) on a shared base class, the candidate_sets context manager nests and restores, CandidateSelection and steps.CandidateTargets validate their
settings, the pickle of a candidate pass carries its own name and is never read, and the three new entry points are part of the ABI on both sides."""
import os
import re

import pytest
import torch

from conftest import REPO

NEW_EXPORTS = ("grip_candidate_select_workspace", "grip_candidate_select", "grip_candidate_ce")


def _pl():
    import grip_amd  # noqa: F401
    from grip_amd import pseudolabels as pl
    return pl


def test_store_owns_its_buffer_and_keys_rows_by_base_name():
    pl = _pl()
    store = pl.CandidateStore()
    assert isinstance(store, pl._PoolRowStore) and isinstance(pl.SoftTargetStore(), pl._PoolRowStore) and store.mask is None
    for call in (lambda: store.rows(["a.jpg"]), lambda: store.col_map([0])):
        with pytest.raises(ValueError, match="no pass has recorded a mask"):
            call()
    paths = ["p/a.jpg", "p/b.jpg", "q/c.jpg"]
    first = torch.tensor([[1, 0], [2, 0], [-1, 1]], dtype=torch.int32)                # 33 classes: two words per row
    labels = list(range(100, 133))
    store.record(paths, labels, first)
    assert store.mask is not first and torch.equal(store.mask, first) and store.mask is store.matrix and store.records == 1
    at = store.mask.data_ptr()
    store.record(paths, labels, first + 4)                                               # the same shape: in place
    assert store.mask.data_ptr() == at and torch.equal(store.mask, first + 4) and store.records == 2
    store.record(paths[:2], labels, first[:2])                                           # another shape: another buffer
    assert store.mask.data_ptr() != at and tuple(store.mask.shape) == (2, 2)
    assert store.rows(["b.jpg", "x/a.jpg", "c.jpg", "b.jpg"], hard=[False, False, False, True]).tolist() == [1, 0, -1, -1] and store.rows([]).dtype == torch.int32
    for bad in (first.float()[:2], first[:2, :1], first):                                # dtype, words, rows
        with pytest.raises(ValueError, match=r"CandidateStore.record: a int32 \[2, 2\] mask was expected"):
            store.record(paths[:2], labels, bad)
    train = list(range(140, 90, -1))                                                     # a training class list that holds the ranked classes, in another order
    cmap = store.col_map(train)
    assert cmap.dtype == torch.int32 and cmap.tolist() == [train.index(c) for c in labels] and store.col_map(train) is cmap
    with pytest.raises(ValueError, match="does not hold"):
        store.col_map(labels[1:])
    store.record(["p/a.jpg", "q/a.jpg"], labels, first[:2])
    with pytest.raises(ValueError, match="CandidateStore: the base name 'a.jpg' names two rows of the pool: candidate sets are keyed"):
        store.rows(["a.jpg"])
    store.forget()
    assert store.rows(["a.jpg"]).tolist() == [-1]
    soft = pl.SoftTargetStore()                                                          # the messages of the float store are its own
    with pytest.raises(ValueError, match=r"SoftTargetStore.record: a float32 \[2, 3\] matrix was expected"):
        soft.record(paths[:2], [0, 1, 2], first[:2])


def test_context_manager_nests_and_restores():
    pl = _pl()
    assert pl.candidates() is None and pl.list_infix() == ""
    a, b = (pl.CandidateSelection(), pl.CandidateStore()), (pl.CandidateSelection(tau=0.5, slots=1, combine="union"), pl.CandidateStore())
    with pl.candidate_sets(*a) as got:
        assert got is a[1] and pl.candidates() == a and pl.list_infix() == "cpl_"
        with pl.candidate_sets(*b):
            assert pl.candidates() == b
            with pl.candidate_sets(None, None) as none:          # None, None: a no-op, like label_propagation(None)
                assert none is None and pl.candidates() == b
            with pl.label_propagation(pl.BalancedAssignment(inner=pl.LabelPropagation())):
                assert pl.list_infix() == "cpl_ot_lp_"
        assert pl.candidates() == a
        with pytest.raises(RuntimeError):
            with pl.candidate_sets(*b):
                raise RuntimeError("inside")
        assert pl.candidates() == a
    assert pl.candidates() is None
    with pl.label_propagation(pl.TransductiveGMM()):
        assert pl.list_infix() == "gmm_"
    for bad in ((a[0], None), (None, a[1]), (a[0], pl.SoftTargetStore()), (0.99, a[1])):
        with pytest.raises(TypeError):
            with pl.candidate_sets(*bad):
                pass
    assert pl.candidates() is None


def test_defaults_and_validation():
    pl = _pl()
    from grip_amd import steps
    sel = pl.CandidateSelection()
    assert (sel.tau, sel.slots, sel.combine, sel.infix) == (0.99, 2, "intersection", "cpl_")
    assert (sel.claim(1000, 16), sel.claim(20, 16), sel.claim(1000, pl.K_ALL), pl.CandidateSelection(slots=3).claim(1000, 16)) == (32, 20, 1000, 48)
    pl.CandidateSelection(tau=1.0, slots=1, combine="inter")
    for bad in (dict(tau=0.0), dict(tau=1.5), dict(tau=-0.1), dict(tau=float("nan")), dict(slots=0), dict(slots=1.5), dict(slots=True), dict(combine="both"),
                dict(combine=0)):
        with pytest.raises(ValueError):
            pl.CandidateSelection(**bad)
    mask, cmap = torch.zeros(4, 2, dtype=torch.int32), torch.arange(33, dtype=torch.int32)
    t = steps.CandidateTargets(mask, cmap)
    assert t.matrix is mask and t.key() == ("candidates", mask.data_ptr(), (4, 2), cmap.data_ptr()) and t.key() != steps.CandidateTargets(mask.clone(), cmap).key()
    for bad in ((mask.float(), cmap), (mask[:, :1], cmap), (mask[0], cmap), (mask, cmap[None]), (None, cmap)):
        with pytest.raises(ValueError, match="CandidateTargets"):
            steps.CandidateTargets(*bad)
    with pytest.raises(ValueError, match="needs the batch's soft_row"):
        steps.step_loss(torch.zeros(4, 40), torch.zeros(4, dtype=torch.long), torch.ones(4), t, None)


def test_pickle_name_carries_cpl_and_an_existing_file_is_not_read(tmp_path, monkeypatch):
    """pseudolabel_top_k names the pickle of a candidate pass `..._pseudolabels_cpl_split_...` (in front of a transduction's infix) and, while the store is
    installed, runs the pass even when that file exists -- a loaded list has no sets behind it (the pass is a stub here: nothing is computed)."""
    import pickle
    from types import SimpleNamespace

    pl = _pl()
    from grip_amd.utils import clip_pseudolabels as cp
    monkeypatch.chdir(tmp_path)
    os.makedirs("pseudolabels")
    cfg = SimpleNamespace(LEARNING_PARADIGM="ul", MODEL="textual_fpl")
    stem = "pseudolabels/D_ViT-B32_ul_textual_fpl_2_pseudolabels_{}split_7.pickle"
    for infix in ("", "cpl_", "cpl_lp_"):
        with open(stem.format(infix), "wb") as f:
            pickle.dump({"filepaths": ["file:" + infix], "labels": [0]}, f)
    ran = []

    def compute(k, template, dataset, classnames, transform, clip_model, label_to_idx, device, filename, chunk=880):
        ran.append(filename)
        dataset.filepaths = ["pass"]
        return dataset
    monkeypatch.setattr(cp, "compute_pseudo_labels", compute)

    def load():
        ds = SimpleNamespace(filepaths=["x"], labels=[1])
        return cp.pseudolabel_top_k(cfg, "D", 2, "", ds, [], None, None, {}, "cpu", "ViT-B/32", 7).filepaths
    assert load() == ["file:"] and ran == []
    with pl.candidate_sets(pl.CandidateSelection(), pl.CandidateStore()):
        assert load() == ["pass"] and ran == [stem.format("cpl_")]
        with pl.label_propagation(pl.LabelPropagation()):
            assert load() == ["pass"] and ran[-1] == stem.format("cpl_lp_")
    assert load() == ["file:"] and len(ran) == 2


def test_abi_lists_the_three_entry_points():
    import grip_amd  # noqa: F401
    from grip_amd import native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "grip_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(grip_[a-z_]+)\s*\(", text))
    for name in NEW_EXPORTS:
        assert name in declared and name in native.EXPORTS, name
    assert declared == set(native.EXPORTS) and native.ABI_VERSION == 9
    lib = native.lib()
    for name in NEW_EXPORTS:
        assert getattr(lib, name) is not None
    nbytes = native.c_size_t()
    assert lib.grip_candidate_select_workspace(50000, 102, native.ctypes.byref(nbytes)) == 0 and nbytes.value >= 102 * 256 * 4      # (needs no device)
    assert lib.grip_candidate_select_workspace(0, 102, native.ctypes.byref(nbytes)) == 1 and b"n = 0" in lib.grip_last_error()
