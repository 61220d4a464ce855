"""CPU: the host side of the CLIP-Adapter feature head -- the float64 helper of the GPU tests against torch autograd, the ctypes signatures, the
workspace entry point (host-only: it answers and refuses without a GPU), the model's seeded initialisation and file, and the configuration switch."""
import ctypes
import os
import types

import pytest
import torch

import feature_adapter_ref as R


def _torch_restatement(f, w1, w2, r):
    return r * torch.relu(torch.relu(f @ w1.T) @ w2.T) + (1 - r) * f


@pytest.mark.parametrize("seed", [0, 2])
def test_reference_helper_against_float64_autograd(seed):
    n, e, h, r = 16, 64, 16, 0.2
    f, w1, w2, G = R.inputs(n, e, h, seed)
    fwd = R.forward(f, w1, w2, r)
    assert R.doubtful(fwd) == 0, "a pre-activation lies within its forward bound of zero: another seed"
    a, b = w1.double().requires_grad_(True), w2.double().requires_grad_(True)
    out = _torch_restatement(f.double(), a, b, r)
    (out * G.double()).sum().backward()
    assert torch.allclose(fwd["out"], out.detach(), rtol=1e-12, atol=0)
    bwd = R.backward(f, w2, fwd["H"], fwd["x"], G, r)
    assert torch.allclose(bwd["grad_w1"], a.grad, rtol=1e-10, atol=1e-13 * float(a.grad.abs().max()))
    assert torch.allclose(bwd["grad_w2"], b.grad, rtol=1e-10, atol=1e-13 * float(b.grad.abs().max()))
    # the same statements in f32 on the CPU (another, equally valid summation order) are inside the bounds, and the bounds are not vacuous:
    # one dropped term of a sum leaves them
    o32 = _torch_restatement(f, w1, w2, r)
    assert R.worst_ratio(o32, fwd["out"], fwd["b_out"]) <= 1.0
    assert R.worst_ratio(torch.relu(f @ w1.T), fwd["H"], fwd["du"]) <= 1.0
    h32, x32 = fwd["H"].float(), fwd["x"].float()
    ref = R.backward(f, w2, h32, x32, G, r)
    dX = r * G * (x32 > 0)
    assert R.worst_ratio(dX.T @ h32, ref["grad_w2"], ref["b_w2"]) <= 1.0
    assert R.worst_ratio((((dX @ w2) * (h32 > 0)).T @ f), ref["grad_w1"], ref["b_w1"]) <= 1.0
    assert R.worst_ratio(dX[1:].T @ h32[1:], ref["grad_w2"], ref["b_w2"]) > 1.0
    w1_short = w1.clone()
    w1_short[:, -1] = 0
    assert R.worst_ratio(_torch_restatement(f, w1_short, w2, r), fwd["out"], fwd["b_out"]) > 1.0


def test_doubtful_masks_are_detected_and_a_zero_row_is_exact():
    assert R.doubtful(R.forward(*R.inputs(16, 64, 16, 1)[:3], 0.2)) > 0      # seed 1 of this draw has pre-activations within their bound of zero
    assert all(R.doubtful(R.forward(*R.inputs(16, 64, 16, s)[:3], 0.2)) == 0 for s in (0, 2, 3, 4))
    f, w1, w2, G = R.inputs(16, 64, 16, 0, zero_row=5)
    fwd = R.forward(f, w1, w2, 0.2)
    assert (fwd["out"][5] == 0).all() and (fwd["H"][5] == 0).all() and (fwd["du"][5] == 0).all()
    assert R.doubtful(fwd) > 0      # a zero pre-activation is "within its bound of zero": the kernel tests feed the backward exact masks instead


def test_ctypes_signatures():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native, steps
    names = ("grip_feature_adapter_workspace", "grip_feature_adapter_forward", "grip_feature_adapter_backward")
    assert all(n in native.EXPORTS for n in names)
    assert len(native._SIGS[names[0]][1]) == 4 and len(native._SIGS[names[1]][1]) == 11 and len(native._SIGS[names[2]][1]) == 14
    assert native._SIGS[names[1]][1][3] is ctypes.c_float and native._SIGS[names[2]][1][5] is ctypes.c_float
    lib = native.lib()
    for n in names:
        assert getattr(lib, n).restype is ctypes.c_int
    assert issubclass(engine.FeatureAdapterFn, torch.autograd.Function) and callable(engine.feature_adapter)
    assert callable(steps.adapter_step) and issubclass(steps.GraphedAdapterStep, steps.GraphedStep)


def test_workspace_answers_and_refuses_without_a_gpu():
    import grip_amd  # noqa: F401
    from grip_amd import native
    lib = native.lib()
    nbytes = ctypes.c_size_t()
    assert lib.grip_feature_adapter_workspace(64, 512, 128, ctypes.byref(nbytes)) == 0
    assert 64 * 128 * 4 <= nbytes.value <= 64 * 128 * 4 + 4096
    # the cap: n * h floats and a constant -- no e * h partial however many rows (a partial per 64 rows would be 205 MB here)
    assert lib.grip_feature_adapter_workspace(50000, 512, 128, ctypes.byref(nbytes)) == 0
    assert 50000 * 128 * 4 <= nbytes.value <= 50000 * 128 * 4 + 8 * 512 * 128 * 4
    for cfg in ((1, 64, 16), (7, 128, 32), (9, 256, 64), (3, 768, 192), (5, 1024, 256)):
        assert lib.grip_feature_adapter_workspace(*cfg, ctypes.byref(nbytes)) == 0, cfg
    for args, word in (((4, 96, 16), "e = 96"), ((4, 64, 24), "h = 24"), ((4, 1024, 272), "h = 272"), ((0, 64, 16), "n = 0"), ((4, 2048, 256), "e = 2048"),
                       ((4, 64, 0), "h = 0")):
        assert lib.grip_feature_adapter_workspace(*args, ctypes.byref(nbytes)) != 0
        assert word in lib.grip_last_error().decode(), lib.grip_last_error().decode()
    assert lib.grip_feature_adapter_workspace(4, 64, 16, None) != 0 and "null" in lib.grip_last_error().decode()
    # the launching entry points refuse bad arguments before they touch the device
    assert lib.grip_feature_adapter_forward(None, None, None, 0.2, 4, 64, 16, None, None, None, None) != 0
    assert "null pointer" in lib.grip_last_error().decode()
    assert lib.grip_feature_adapter_forward(None, None, None, 0.2, 4, 96, 16, None, None, None, None) != 0
    assert "e = 96" in lib.grip_last_error().decode()
    assert lib.grip_feature_adapter_backward(None, None, None, None, None, 0.2, 4, 64, 24, None, None, None, 0, None) != 0
    assert "h = 24" in lib.grip_last_error().decode()
    assert lib.grip_feature_adapter_backward(None, None, None, None, None, 0.2, 0, 64, 16, None, None, None, 0, None) != 0
    assert "n = 0" in lib.grip_last_error().decode()


def test_model_is_seeded_by_its_own_generator():
    import grip_amd  # noqa: F401
    from grip_amd.models import ClipAdapterModel
    torch.manual_seed(123)
    before = torch.get_rng_state()
    a, b, c = ClipAdapterModel(128, seed=7), ClipAdapterModel(128, seed=7), ClipAdapterModel(128, seed=8)
    assert torch.equal(torch.get_rng_state(), before), "the global torch RNG was read"
    assert torch.equal(a.w1, b.w1) and torch.equal(a.w2, b.w2) and not torch.equal(a.w1, c.w1)
    assert a.w1.shape == (32, 128) and a.w2.shape == (128, 32) and (a.hidden_dim, a.ratio, a.reduction) == (32, 0.2, 4)
    # nn.Linear(bias=False): U(+-1 / sqrt(fan_in))
    assert float(a.w1.detach().abs().max()) <= 128 ** -0.5 and float(a.w1.detach().abs().max()) > 0.9 * 128 ** -0.5
    assert float(a.w2.detach().abs().max()) <= 32 ** -0.5 and float(a.w2.detach().abs().max()) > 0.9 * 32 ** -0.5
    assert [p is q for p, q in zip(a.parameters(), (a.w1, a.w2))] == [True, True] and a.w1.requires_grad and a.w2.requires_grad
    assert ClipAdapterModel(768, reduction=4).hidden_dim == 192 and ClipAdapterModel(64, reduction=2, ratio=0.5).ratio == 0.5
    for kw in (dict(embed_dim=100), dict(embed_dim=128, reduction=3), dict(embed_dim=2048), dict(embed_dim=64, reduction=8), dict(embed_dim=1024, reduction=2)):
        with pytest.raises(ValueError):
            ClipAdapterModel(**kw)


def _conf(**kw):
    return types.SimpleNamespace(MODALITY="text", VIS_ENCODER="ViT-B/16", DATASET_NAME="Synthetic", LEARNING_PARADIGM="ssl", MODEL="textual_fpl",
                                 OPTIM_SEED=1, SPLIT_SEED=500, **kw)


def test_adapter_file_round_trips(tmp_path, monkeypatch):
    import grip_amd  # noqa: F401
    from grip_amd.models import ClipAdapterModel
    from grip_amd.utils import adapter_path, compute_metrics as cm
    monkeypatch.chdir(tmp_path)
    conf = _conf()
    m = ClipAdapterModel(128, reduction=2, ratio=0.35, seed=4)
    with torch.no_grad():
        m.w1.mul_(1.7)
    prompt = [torch.zeros(1, 4, 8).numpy()]
    plain = cm.save_parameters(prompt, conf, iteration=3)
    with open(plain, "rb") as f:
        plain_bytes = f.read()
    fn = cm.save_parameters(prompt, conf, iteration=3, adapter=m)
    path = adapter_path(conf, 3)
    assert fn == plain and path == cm.adapter_path(conf, 3) and path == fn[:-len(".pickle")] + "_adapter.pickle"
    assert sorted(os.listdir("trained_prompts")) == sorted([os.path.basename(fn), os.path.basename(path)])
    with open(fn, "rb") as f:
        assert f.read() == plain_bytes      # the prompt file is what it is without the adapter
    back = ClipAdapterModel.load(path)
    assert torch.equal(back.w1, m.w1) and torch.equal(back.w2, m.w2) and (back.ratio, back.reduction, back.seed) == (0.35, 2, 4)
    assert back.w1.requires_grad
    m.save(tmp_path / "direct.pickle")
    assert torch.equal(ClipAdapterModel.load(tmp_path / "direct.pickle").w2, m.w2)
    cm.save_parameters(prompt, conf)      # no adapter: the prompt file alone
    assert not os.path.exists(adapter_path(conf))


def _strategy(modality, **conf):
    import grip_amd  # noqa: F401
    from grip_amd.methods.training_strategies import TrainingStrategy
    s = object.__new__(TrainingStrategy)
    s.config = types.SimpleNamespace(**conf)
    s.modality = modality
    return s


def test_switch_defaults_off_is_textual_only_and_excludes_the_cache_head():
    from grip_amd.methods.main import DEFAULTS
    assert "CLIP_ADAPTER" not in DEFAULTS or DEFAULTS["CLIP_ADAPTER"] is False
    assert not _strategy("text").clip_adapter() and not _strategy("text", CLIP_ADAPTER=False).clip_adapter()
    assert _strategy("text", CLIP_ADAPTER=True).clip_adapter() and _strategy("text", CLIP_ADAPTER=True, TIP_ADAPTER=False).clip_adapter()
    for modality in ("image", "multi"):
        assert not _strategy(modality, CLIP_ADAPTER=True).clip_adapter()
        assert not _strategy(modality, CLIP_ADAPTER=True, TIP_ADAPTER=True).clip_adapter()      # both ignored there: nothing to refuse
    with pytest.raises(ValueError, match="CLIP_ADAPTER and TIP_ADAPTER"):
        _strategy("text", CLIP_ADAPTER=True, TIP_ADAPTER=True).clip_adapter()
    assert _strategy("text", TIP_ADAPTER=True).tip_adapter() and not _strategy("text", TIP_ADAPTER=True).clip_adapter()
