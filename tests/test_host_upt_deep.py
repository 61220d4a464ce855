"""CPU: the host side of deep UPT (vpt_embeddings_deep mixed with the prompts and fed to the image tower as deep prompts): the three ABI 9
additions are declared, exported and check their arguments before touching a device; UPT_DEEP draws the deep embeddings after the two
prompts; the framework mixer with mix_deep computes the reference's intended graph (models/prompts_models.py:129-146 with :133-134, :146)."""
import ctypes
import os
import re
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("grip_upt_mixer_deep_workspace", "grip_upt_mixer_forward_deep", "grip_upt_mixer_backward_deep")


def test_header_declares_and_library_exports_the_deep_mixer_calls():
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


def test_deep_workspace_sizes_and_refusals():
    import grip_amd  # noqa: F401
    from grip_amd import native
    lib = native.lib()
    n, n0 = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.grip_upt_mixer_workspace(16, 768, 1024, 128, ctypes.byref(n0)) == 0
    assert lib.grip_upt_mixer_deep_workspace(16, 0, 768, 1024, 128, ctypes.byref(n)) == 0 and n.value == n0.value
    sizes = []
    for nd in (1, 23, 31):
        assert lib.grip_upt_mixer_deep_workspace(16, nd, 768, 1024, 128, ctypes.byref(n)) == 0
        sizes.append(n.value)
    assert n0.value < sizes[0] < sizes[1] < sizes[2]
    for nd in (-1, 32):
        assert lib.grip_upt_mixer_deep_workspace(16, nd, 768, 1024, 128, ctypes.byref(n)) == 1
        assert b"n_deep" in lib.grip_last_error() and b"out of range" in lib.grip_last_error()
    assert lib.grip_upt_mixer_deep_workspace(40, 2, 768, 1024, 128, ctypes.byref(n)) == 1 and b"n_prompt" in lib.grip_last_error()
    assert lib.grip_upt_mixer_deep_workspace(4, 2, 512, 768, 128, None) == 1 and b"null pointer" in lib.grip_last_error()
    # the compute calls refuse before they touch a device
    m = native.UptMixer(4, 512, 768, 128, 0, 0)
    assert lib.grip_upt_mixer_forward_deep(ctypes.byref(m), None, 32, None, None, None, None, 0, None) == 1 and b"n_deep = 32" in lib.grip_last_error()
    assert lib.grip_upt_mixer_forward_deep(None, None, 1, None, None, None, None, 0, None) == 1 and b"null pointer" in lib.grip_last_error()
    assert lib.grip_upt_mixer_forward_deep(ctypes.byref(m), None, 2, None, None, None, None, 0, None) == 1 and b"null vpt_deep" in lib.grip_last_error()
    assert lib.grip_upt_mixer_backward_deep(ctypes.byref(m), None, -1, None, None, None, None, None, None, 0, None) == 1 \
        and b"out of range" in lib.grip_last_error()
    assert lib.grip_upt_mixer_backward_deep(ctypes.byref(m), None, 3, None, None, None, None, None, None, 0, None) == 1 \
        and b"null vpt_deep" in lib.grip_last_error()


def _strategy(upt_deep):
    import grip_amd  # noqa: F401
    from grip_amd import config
    from grip_amd.methods.training_strategies import TrainingStrategy
    s = object.__new__(TrainingStrategy)
    conf = dict(OPTIM_SEED=3, TEXT_PREFIX_SIZE=4, VISION_PREFIX_SIZE=4, VAR_INIT=0.02, VPT_DEEP=True)
    if upt_deep is not None:
        conf["UPT_DEEP"] = upt_deep
    s.config = types.SimpleNamespace(**conf)
    s.modality = "multi"
    s.clip_model = types.SimpleNamespace(dims=config.get_dims("ViT-B/16"))
    s.initialize_prompts_parameters()
    return s


def test_upt_deep_initialisation_keeps_the_prompts():
    plain, off, deep = _strategy(None), _strategy(False), _strategy(True)
    for s in (off, deep):
        assert torch.equal(plain.coop_init, s.coop_init) and torch.equal(plain.vpt_init, s.vpt_init)
    assert plain.coop_init.shape == (1, 4, 512) and plain.vpt_init.shape == (1, 4, 768)
    # off by default; VPT_DEEP keeps its meaning (visual strategies only)
    assert plain.vpt_deep_init is None and off.vpt_deep_init is None and not plain.vpt_deep()
    assert deep.upt_deep() and not plain.upt_deep()
    assert deep.vpt_deep_init.shape == (11, 4, 768)
    assert not torch.equal(deep.vpt_deep_init[0], deep.vpt_init[0])
    assert abs(float(deep.vpt_deep_init.std()) - 0.02) < 2e-3


def _upt(deep, mix_deep, seed=0):
    import grip_amd  # noqa: F401
    from grip_amd.models import UPTModel
    g = torch.Generator().manual_seed(seed)
    coop, vpt = torch.randn(1, 4, 96, generator=g) * 0.02, torch.randn(1, 4, 80, generator=g) * 0.02
    torch.manual_seed(seed + 1)
    return UPTModel(coop, vpt, deep, None, None, ["a"], 64, device="cpu", dtype=torch.float32, mix_deep=mix_deep)


def test_framework_mix_deep_is_the_intended_reference_graph():
    deep = torch.randn(3, 4, 80, generator=torch.Generator().manual_seed(9)) * 0.02
    m = _upt(deep.clone(), True)
    assert not m._native_mixer_ok()              # a CPU model: the framework's kernels
    ce, ve, de = m.mix()
    assert ce.shape == (1, 4, 96) and ve.shape == (1, 4, 80) and de.shape == (3, 4, 80)
    with torch.no_grad():
        coop_embds = m.proj_coop_pre(m.coop_embeddings)
        vpt_embds = m.proj_vpt_pre(torch.cat((m.vpt_embeddings, m.vpt_embeddings_deep)))        # [1 + D, P, dim]
        out = m.transformer(torch.cat((coop_embds, vpt_embds)).float()).to(torch.float16)          # sequence 2 + D, batch P
        coop_want = m.proj_coop_post(out[:1].float())
        vpt_all = m.proj_vpt_post(out[1:].float())
    assert torch.equal(ce.detach(), coop_want) and torch.equal(ve.detach(), vpt_all[:1]) and torch.equal(de.detach(), vpt_all[1:])
    (ce.square().sum() + ve.square().sum() + de.square().sum()).backward()
    assert m.vpt_embeddings_deep.grad is not None and m.vpt_embeddings_deep.grad.abs().sum() > 0
    # the deep rows take part in the attention: the shallow outputs differ from a model without them
    plain = _upt(None, False)
    assert not torch.equal(plain.mix()[1].detach(), ve.detach())


def test_mix_deep_off_ignores_the_deep_embeddings():
    deep = torch.randn(3, 4, 80, generator=torch.Generator().manual_seed(9)) * 0.02
    off, plain = _upt(deep, False), _upt(None, False)
    a, b = off.mix(), plain.mix()
    assert len(a) == len(b) == 2 and all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b))
    (a[0].sum() + a[1].sum()).backward()
    assert off.vpt_embeddings_deep.grad is None
    with pytest.raises(ValueError, match="mix_deep"):
        _upt(None, True)
