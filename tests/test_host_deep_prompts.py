"""CPU: the host side of deep visual prompts (VPT-Deep): the two ABI additions are declared and exported, the engine's shape rules, and the
visual strategies' initialisation (the shallow prompt is drawn first and stays bit-identical with VPT_DEEP)."""
import os
import re
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_deep_calls():
    import grip_amd  # noqa: F401
    from grip_amd import native
    with open(os.path.join(REPO, "include", "grip_amd.h")) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = native.lib()
    for name in ("grip_vit_forward_deep", "grip_vit_backward_deep"):
        assert re.search(rf"\bint {name}\s*\(", h), name
        assert name in native.EXPORTS
        assert getattr(lib, name) is not None
    # the additions leave the ABI version where it was
    assert int(re.search(r"#define GRIP_ABI_VERSION (\d+)", h).group(1)) == native.ABI_VERSION == lib.grip_abi_version() == 9


def test_deep_prompt_shape_rules():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    check = engine.check_deep_prompts
    check(torch.zeros(1, 4, 8), 4, 8, 12)
    check(torch.zeros(11, 4, 8), 4, 8, 12)
    for bad, P in ((torch.zeros(12, 4, 8), 4),      # D > layers - 1
                   (torch.zeros(0, 4, 8), 4),       # D = 0 given explicitly
                   (torch.zeros(2, 3, 8), 4),       # not the shallow prompt's P
                   (torch.zeros(2, 4, 7), 4),       # width
                   (torch.zeros(4, 8), 4),          # not [D, P, d]
                   (torch.zeros(1, 1, 4, 8), 4),
                   (torch.zeros(1, 4, 8), 0)):      # no shallow prompt
        with pytest.raises(native.GripError, match="deep visual prompts"):
            check(bad, P, 8, 12)
    t = types.SimpleNamespace(width=8, dims=types.SimpleNamespace(layers=3))
    deep, D = engine.Tower.vit_deep(t, torch.ones(2, 4, 8, dtype=torch.float16).transpose(1, 2).contiguous().transpose(1, 2), 4)
    assert D == 2 and deep.dtype == torch.float32 and deep.is_contiguous()
    assert engine.Tower.vit_deep(t, None, 4) == (None, 0)
    with pytest.raises(native.GripError, match=r"1 <= D <= 2"):
        engine.Tower.vit_deep(t, torch.ones(3, 4, 8), 4)


def _strategy(deep):
    import grip_amd  # noqa: F401
    from grip_amd import config
    from grip_amd.methods.training_strategies import TrainingStrategy
    s = object.__new__(TrainingStrategy)
    conf = dict(OPTIM_SEED=3, PREFIX_SIZE=4, VAR_INIT=0.02)
    if deep is not None:
        conf["VPT_DEEP"] = deep
    s.config = types.SimpleNamespace(**conf)
    s.modality = "image"
    s.clip_model = types.SimpleNamespace(dims=config.get_dims("ViT-B/16"))
    s.initialize_prompts_parameters()
    return s


def test_vpt_deep_initialisation_keeps_the_shallow_prompt():
    plain, off, deep = _strategy(None), _strategy(False), _strategy(True)
    assert torch.equal(plain.initial_prefix, deep.initial_prefix) and torch.equal(plain.initial_prefix, off.initial_prefix)
    assert plain.initial_prefix.shape == (4, 768)
    assert plain.initial_deep_prefix is None and off.initial_deep_prefix is None
    assert deep.initial_deep_prefix.shape == (11, 4, 768)
    assert not torch.equal(deep.initial_deep_prefix[0], deep.initial_prefix)
    assert abs(float(deep.initial_deep_prefix.std()) - 0.02) < 2e-3
