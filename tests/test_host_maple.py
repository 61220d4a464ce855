"""CPU: the host side of the coupled deep multimodal prompts (MaPLe): the three ABI 9 additions of csrc/couple.hip are declared, exported and
check their arguments before touching a device; MaPLeModel registers the four trainable tensors and its framework path is the literal per-depth
nn.Linear; MAPLE draws its deep text prompts after the two shallow prompts; the MaPLe snapshot round-trips through save / load_parameters."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("grip_prompt_couple_workspace", "grip_prompt_couple_forward", "grip_prompt_couple_backward")


def test_header_declares_and_library_exports_the_coupling_calls():
    import grip_amd  # noqa: F401
    from grip_amd import native
    with open(os.path.join(REPO, "include", "grip_amd.h")) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    lib = native.lib()
    for name in CALLS:
        assert re.search(rf"\bint {name}\s*\(", h), name
        assert name in native.EXPORTS
        assert getattr(lib, name) is not None
    assert int(re.search(r"#define GRIP_ABI_VERSION (\d+)", h).group(1)) == native.ABI_VERSION == lib.grip_abi_version() == 9


def test_coupling_workspace_sizes_and_refusals():
    import grip_amd  # noqa: F401
    from grip_amd import native
    lib = native.lib()
    err = lib.grip_last_error
    n = ctypes.c_size_t()
    sizes = []
    for nd in (0, 1, 8, 11, 31):
        assert lib.grip_prompt_couple_workspace(16, nd, 512, 768, ctypes.byref(n)) == 0
        sizes.append(n.value)
    assert 0 < sizes[0] < sizes[1] < sizes[2] < sizes[3] < sizes[4]
    for P in (0, 17):
        assert lib.grip_prompt_couple_workspace(P, 2, 512, 768, ctypes.byref(n)) == 1 and b"n_prompt" in err()
    for nd in (-1, 32):
        assert lib.grip_prompt_couple_workspace(4, nd, 512, 768, ctypes.byref(n)) == 1 and b"n_deep" in err() and b"out of range" in err()
    for dt, dv in ((500, 768), (512, 700), (0, 768), (512, 32)):
        assert lib.grip_prompt_couple_workspace(4, 2, dt, dv, ctypes.byref(n)) == 1 and b"multiples of 64" in err()
    assert lib.grip_prompt_couple_workspace(4, 2, 512, 768, None) == 1 and b"null pointer" in err()
    # the compute calls refuse before they touch a device (host memory stands in for the buffers: nothing is launched)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    fwd, bwd = lib.grip_prompt_couple_forward, lib.grip_prompt_couple_backward
    assert fwd(p, p, 17, 2, 512, 768, p, p, p, p, None) == 1 and b"n_prompt = 17" in err()
    assert fwd(p, p, 4, 32, 512, 768, p, p, p, p, None) == 1 and b"n_deep = 32" in err()
    assert fwd(p, p, 4, 2, 520, 768, p, p, p, p, None) == 1 and b"multiples of 64" in err()
    assert fwd(None, p, 4, 2, 512, 768, p, p, p, p, None) == 1 and b"null pointer" in err()
    assert fwd(p, p, 4, 2, 512, 768, p, None, p, p, None) == 1 and b"null pointer" in err()
    assert fwd(p, None, 4, 2, 512, 768, p, p, p, p, None) == 1 and b"null deep_text" in err()
    assert fwd(p, p, 4, 2, 512, 768, p, p, p, None, None) == 1 and b"null deep_text" in err()
    assert bwd(p, p, 0, 2, 512, 768, p, p, p, p, p, p, p, p, 1 << 20, None) == 1 and b"n_prompt" in err()
    assert bwd(p, p, 4, -1, 512, 768, p, p, p, p, p, p, p, p, 1 << 20, None) == 1 and b"out of range" in err()
    assert bwd(p, p, 4, 2, 512, 768, p, p, p, p, p, None, p, p, 1 << 20, None) == 1 and b"null pointer" in err()
    assert bwd(p, p, 4, 2, 512, 768, p, p, p, p, p, p, p, None, 0, None) == 1 and b"null pointer" in err()
    assert bwd(p, p, 4, 2, 512, 768, p, p, None, p, p, p, p, p, 1 << 20, None) == 1 and b"null deep_text" in err()
    assert bwd(p, p, 4, 2, 512, 768, p, p, p, p, None, p, p, p, 1 << 20, None) == 1 and b"null deep_text" in err()
    assert bwd(p, p, 4, 2, 512, 768, p, p, p, p, p, p, p, p, 1024, None) == 1 and b"workspace too small" in err()


def _maple(D, P=4, dt=96, dv=80, seed=0):
    import grip_amd  # noqa: F401
    from grip_amd.models import MaPLeModel
    g = torch.Generator().manual_seed(seed)
    ctx = torch.randn(1, P, dt, generator=g) * 0.02
    deep = torch.randn(D, P, dt, generator=g) * 0.02 if D else None
    torch.manual_seed(seed + 1)
    return MaPLeModel(ctx, deep, None, None, ["a"], device="cpu", vision_width=dv)


def test_maple_model_registers_exactly_the_four_parameters():
    m = _maple(3)
    shapes = {n: tuple(p.shape) for n, p in m.named_parameters()}
    assert shapes == {"ctx": (1, 4, 96), "compound_prompts_text": (3, 4, 96), "proj_weight": (4, 80, 96), "proj_bias": (4, 80)}
    assert all(p.requires_grad and p.dtype == torch.float32 for p in m.parameters())
    assert m.module is m and m.classes == ["a"]
    # each slice is initialised as nn.Linear initialises its own
    torch.manual_seed(1)
    lin = [torch.nn.Linear(96, 80) for _ in range(4)]
    assert all(torch.equal(m.proj_weight[l], lin[l].weight) and torch.equal(m.proj_bias[l], lin[l].bias) for l in range(4))
    shallow = _maple(0)
    assert {n: tuple(p.shape) for n, p in shallow.named_parameters()} == {"ctx": (1, 4, 96), "proj_weight": (1, 80, 96), "proj_bias": (1, 80)}
    assert shallow.compound_prompts_text is None
    with pytest.raises(ValueError, match="compound_prompts_text"):
        from grip_amd.models import MaPLeModel
        MaPLeModel(torch.zeros(1, 4, 96), torch.zeros(2, 3, 96), None, None, ["a"], vision_width=80)


def test_framework_coupling_is_the_literal_per_depth_linear():
    m = _maple(3, seed=4)
    assert not m._native_couple_ok()              # a CPU model: the framework's linear
    ctx, deep, vis_prefix, vis_deep = m.couple()
    assert ctx is m.ctx and deep is m.compound_prompts_text
    assert vis_prefix.shape == (4, 80) and vis_deep.shape == (3, 4, 80)
    lins = []
    for l in range(4):
        lin = torch.nn.Linear(96, 80)
        with torch.no_grad():
            lin.weight.copy_(m.proj_weight[l])
            lin.bias.copy_(m.proj_bias[l])
        lins.append(lin)
    with torch.no_grad():
        assert torch.equal(vis_prefix, lins[0](m.ctx[0]))
        for l in range(3):
            assert torch.equal(vis_deep[l], lins[l + 1](m.compound_prompts_text[l]))
    g = torch.Generator().manual_seed(2)
    w0, w1 = torch.randn(4, 80, generator=g), torch.randn(3, 4, 80, generator=g)
    ((vis_prefix * w0).sum() + (vis_deep * w1).sum()).backward()
    (sum((lins[l + 1](m.compound_prompts_text[l].detach()) * w1[l]).sum() for l in range(3)) + (lins[0](m.ctx[0].detach()) * w0).sum()).backward()
    for l in range(4):
        assert torch.equal(m.proj_weight.grad[l], lins[l].weight.grad) and torch.equal(m.proj_bias.grad[l], lins[l].bias.grad)
    assert m.ctx.grad.abs().sum() > 0 and m.compound_prompts_text.grad.abs().sum() > 0
    # D = 0: the shallow pair only
    s = _maple(0)
    out = s.couple()
    assert out[1] is None and out[3] is None and out[2].shape == (4, 80)


def _strategy(modality="multi", **conf):
    import grip_amd  # noqa: F401
    from grip_amd import config
    from grip_amd.methods.training_strategies import TrainingStrategy
    s = object.__new__(TrainingStrategy)
    base = dict(OPTIM_SEED=3, TEXT_PREFIX_SIZE=4, VISION_PREFIX_SIZE=4, PREFIX_SIZE=4, VAR_INIT=0.02)
    base.update(conf)
    s.config = types.SimpleNamespace(**base)
    s.modality = modality
    s.clip_model = types.SimpleNamespace(dims=config.get_dims("ViT-B/16"))
    s.initialize_prompts_parameters()
    return s


def test_maple_initialisation_keeps_the_prompts():
    plain, off, on, nine = _strategy(), _strategy(MAPLE=False), _strategy(MAPLE=True), _strategy(MAPLE=True, MAPLE_DEPTH=8)
    for s in (off, on, nine):
        assert torch.equal(plain.coop_init, s.coop_init) and torch.equal(plain.vpt_init, s.vpt_init)
    assert not plain.maple() and not off.maple() and on.maple()
    assert plain.maple_deep_init is None and off.maple_deep_init is None
    assert on.maple_deep_init.shape == (11, 4, 512) and nine.maple_deep_init.shape == (8, 4, 512)
    assert abs(float(on.maple_deep_init.std()) - 0.02) < 2e-3
    assert on.vpt_deep_init is None
    assert _strategy(MAPLE=True, MAPLE_DEPTH=0).maple_deep_init is None
    with pytest.raises(ValueError, match="UPT_DEEP"):
        _strategy(MAPLE=True, UPT_DEEP=True)
    with pytest.raises(ValueError, match="MAPLE_DEPTH"):
        _strategy(MAPLE=True, MAPLE_DEPTH=12)
    with pytest.raises(ValueError, match="VISION_PREFIX_SIZE"):
        _strategy(MAPLE=True, VISION_PREFIX_SIZE=8)
    # textual and visual strategies ignore the switch
    for modality in ("text", "image"):
        a, b = _strategy(modality), _strategy(modality, MAPLE=True, UPT_DEEP=True)
        assert not b.maple() and torch.equal(a.initial_prefix, b.initial_prefix) and b.initial_deep_prefix is None


def test_maple_snapshot_round_trips(tmp_path, monkeypatch):
    import grip_amd  # noqa: F401
    from grip_amd.utils import compute_metrics as cm
    monkeypatch.chdir(tmp_path)
    conf = types.SimpleNamespace(MODALITY="multi", MAPLE=True, VIS_ENCODER="ViT-B/16", DATASET_NAME="Synthetic", LEARNING_PARADIGM="ssl",
                                 MODEL="multimodal_prompt", OPTIM_SEED=1, SPLIT_SEED=500)
    g = np.random.default_rng(0)
    snap = [g.standard_normal((1, 4, 96), dtype=np.float32), g.standard_normal((3, 4, 96), dtype=np.float32),
            g.standard_normal((4, 80, 96), dtype=np.float32), g.standard_normal((4, 80), dtype=np.float32)]
    fn = cm.save_parameters(snap, conf, iteration=2)
    assert fn.endswith("_maple.pickle") and os.path.exists(fn) and os.listdir("trained_prompts") == [os.path.basename(fn)]
    back = cm.load_parameters(conf, iteration=2)
    assert len(back) == 4 and all(np.array_equal(a, b) for a, b in zip(snap, back))
    shallow = [snap[0], None, snap[2][:1], snap[3][:1]]
    cm.save_parameters(shallow, conf)
    back = cm.load_parameters(conf)
    assert back[1] is None and np.array_equal(back[2], shallow[2])
    # without the switch the multimodal file set is UPT's
    conf.MAPLE = False
    with pytest.raises(FileNotFoundError):
        cm.load_parameters(conf, iteration=2)
