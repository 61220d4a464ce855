"""CPU: the host side of the Tip-Adapter cache head -- grouping of the keys by class, the configuration switch, the ctypes signatures, and the
workspace entry point (host-only: it answers and refuses without a GPU)."""
import ctypes
import os
import types

import pytest
import torch


def test_grouping_and_class_start():
    import grip_amd  # noqa: F401
    from grip_amd.models import TipAdapterModel, group_keys_by_class
    labels = [3, 1, 3, 0, 1, 3, 5]                      # classes 2, 4 and 6 own no key
    order, start = group_keys_by_class(labels, 7)
    assert order.tolist() == [3, 1, 4, 0, 2, 5, 6]      # stable: within a class the given order is kept
    assert start.dtype == torch.int32 and start.tolist() == [0, 1, 3, 3, 6, 6, 7, 7]
    keys = torch.arange(7.0)[:, None] * torch.ones(1, 8)      # key j is the constant j
    weight = torch.arange(7.0) + 10
    m = TipAdapterModel(keys, labels, 7, key_weight=weight, alpha=2.0, beta=3.0)
    assert m.keys[:, 0].tolist() == [3, 1, 4, 0, 2, 5, 6] and not isinstance(m.keys, torch.nn.Parameter)
    assert m.key_weight.tolist() == [13, 11, 14, 10, 12, 15, 16]      # permuted with the keys
    assert m.key_class.tolist() == [0, 1, 1, 3, 3, 3, 5] and m.order.tolist() == order.tolist()
    assert m.class_start.tolist() == start.tolist() and (m.alpha, m.beta, m.n_class) == (2.0, 3.0, 7)
    t = TipAdapterModel(keys, labels, 7, train_keys=True)
    assert isinstance(t.keys, torch.nn.Parameter) and t.keys.requires_grad and [p is t.keys for p in t.parameters()] == [True]
    assert t.key_weight is None
    assert group_keys_by_class([0, 0, 0], 1)[1].tolist() == [0, 3]
    assert group_keys_by_class(torch.tensor([2]), 3)[1].tolist() == [0, 0, 0, 1]


def test_labels_are_validated():
    import grip_amd  # noqa: F401
    from grip_amd.models import TipAdapterModel, group_keys_by_class
    with pytest.raises(ValueError, match="outside"):
        group_keys_by_class([0, 7], 7)
    with pytest.raises(ValueError, match="outside"):
        group_keys_by_class([-1, 2], 7)
    with pytest.raises(ValueError, match="integer"):
        group_keys_by_class([0.5, 2.0], 7)
    with pytest.raises(ValueError, match="at least one"):
        group_keys_by_class([], 7)
    with pytest.raises(ValueError, match="key_weight"):
        TipAdapterModel(torch.ones(3, 4), [0, 1, 2], 3, key_weight=torch.ones(2))
    with pytest.raises(ValueError, match="expected"):
        TipAdapterModel(torch.ones(3, 4), [0, 1], 3)


def test_from_lists_normalises_and_weighs_the_pseudolabelled_rows():
    import grip_amd  # noqa: F401
    from grip_amd.models import TipAdapterModel
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(5, 16, generator=g) * 7
    m = TipAdapterModel.from_lists(feats, [1, 0, 1, 0, 2], [False, True, True, False, False], 3, pseudo_weight=0.25, alpha=1.5)
    assert m.order.tolist() == [1, 3, 0, 2, 4] and m.class_start.tolist() == [0, 2, 4, 5]
    assert torch.allclose(m.keys.norm(dim=1), torch.ones(5), atol=1e-6)
    assert torch.equal(m.keys, (feats / feats.norm(dim=-1, keepdim=True))[m.order])
    assert m.key_weight.tolist() == [0.25, 1.0, 1.0, 0.25, 1.0] and m.alpha == 1.5 and m.beta == 5.5
    assert TipAdapterModel.from_lists(feats, [1, 0, 1, 0, 2], [False, True, True, False, False], 3).key_weight is None      # weight 1: no array


def test_cache_file_round_trips(tmp_path, monkeypatch):
    import grip_amd  # noqa: F401
    from grip_amd.models import TipAdapterModel
    from grip_amd.utils import compute_metrics as cm
    monkeypatch.chdir(tmp_path)
    conf = types.SimpleNamespace(MODALITY="text", VIS_ENCODER="ViT-B/16", DATASET_NAME="Synthetic", LEARNING_PARADIGM="ssl", MODEL="textual_fpl",
                                 OPTIM_SEED=1, SPLIT_SEED=500)
    m = TipAdapterModel(torch.randn(6, 8), [2, 0, 2, 1, 0, 2], 4, key_weight=torch.rand(6), alpha=2.0, beta=4.0)
    prompt = [torch.zeros(1, 4, 8).numpy()]
    fn = cm.save_parameters(prompt, conf, iteration=3, cache=m)
    assert fn.endswith("_spl_500.pickle") and sorted(os.listdir("trained_prompts")) == sorted([os.path.basename(fn), os.path.basename(cm.tip_cache_path(conf, 3))])
    assert (cm.load_parameters(conf, iteration=3)[0] == prompt[0]).all()      # the prompt file is what it is without the cache
    back = TipAdapterModel.load(cm.tip_cache_path(conf, 3))
    assert torch.equal(back.keys, m.keys) and torch.equal(back.key_weight, m.key_weight) and torch.equal(back.class_start, m.class_start)
    assert torch.equal(back.key_class, m.key_class) and (back.alpha, back.beta, back.n_class) == (2.0, 4.0, 4)
    cm.save_parameters(prompt, conf)      # no cache: the prompt file alone
    assert not os.path.exists(cm.tip_cache_path(conf))


def _strategy(modality, **conf):
    import grip_amd  # noqa: F401
    from grip_amd.methods.training_strategies import TrainingStrategy
    s = object.__new__(TrainingStrategy)
    s.config = types.SimpleNamespace(**conf)
    s.modality = modality
    return s


def test_switch_defaults_off_and_is_textual_only():
    from grip_amd.methods.main import DEFAULTS
    assert "TIP_ADAPTER" not in DEFAULTS or DEFAULTS["TIP_ADAPTER"] is False
    assert not _strategy("text").tip_adapter() and not _strategy("text", TIP_ADAPTER=False).tip_adapter()
    assert _strategy("text", TIP_ADAPTER=True).tip_adapter()
    for modality in ("image", "multi"):
        assert not _strategy(modality, TIP_ADAPTER=True).tip_adapter()


def test_ctypes_signatures():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native, steps
    names = ("grip_cache_head_workspace", "grip_cache_head_forward", "grip_cache_head_backward")
    assert all(n in native.EXPORTS for n in names)
    assert len(native._SIGS["grip_cache_head_workspace"][1]) == 5
    assert len(native._SIGS["grip_cache_head_forward"][1]) == 14 and len(native._SIGS["grip_cache_head_backward"][1]) == 15
    assert native._SIGS["grip_cache_head_forward"][1][4:6] == [ctypes.c_float, ctypes.c_float]
    lib = native.lib()
    for n in names:
        assert getattr(lib, n).restype is ctypes.c_int
    assert issubclass(engine.CacheHeadFn, torch.autograd.Function) and callable(steps.tip_step) and issubclass(steps.GraphedTipStep, steps.GraphedStep)


def test_workspace_answers_and_refuses_without_a_gpu():
    import grip_amd  # noqa: F401
    from grip_amd import native
    lib = native.lib()
    nbytes = ctypes.c_size_t()
    assert lib.grip_cache_head_workspace(50000, 1632, 102, 512, ctypes.byref(nbytes)) == 0
    assert nbytes.value >= 50000 * 4
    small = ctypes.c_size_t()
    assert lib.grip_cache_head_workspace(1, 1, 1, 4, ctypes.byref(small)) == 0 and 4 <= small.value < nbytes.value
    for args, word in (((4, 4, 4, 6), "e = 6"), ((4, 4, 4, 4096), "e = 4096"), ((0, 4, 4, 64), "n = 0"), ((4, 0, 4, 64), "m = 0"), ((4, 4, -1, 64), "c = -1")):
        assert lib.grip_cache_head_workspace(*args, ctypes.byref(nbytes)) != 0
        assert word in lib.grip_last_error().decode()
    assert lib.grip_cache_head_workspace(4, 4, 4, 64, None) != 0 and "null" in lib.grip_last_error().decode()
    # the launching entry points refuse bad arguments before they touch the device
    assert lib.grip_cache_head_forward(None, None, None, None, 1.0, 5.5, 4, 4, 4, 64, None, None, 0, None) != 0
    assert "null pointer" in lib.grip_last_error().decode()
    assert lib.grip_cache_head_backward(None, None, None, None, 1.0, 5.5, 4, 4, 4, 6, None, None, None, 0, None) != 0
    assert "e = 6" in lib.grip_last_error().decode()
