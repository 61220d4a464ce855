"""The CLIP-Adapter feature head above the kernel: engine.FeatureAdapterFn against float64 autograd, the graphed adapter step against the eager one,
the model over any split of its rows, and the CLIP_ADAPTER switch of the textual strategies on the synthetic pool (tiny towers).

FeatureAdapterFn's backward reads the hidden tensor of its OWN f32 forward, not the float64 one: within du of it (feature_adapter_ref: the forward
bound of the hidden activations) and, for a seed without a doubtful pre-activation (asserted), with the same masks.  grad_w2 = dX^T hidden inherits
sum_i |dX_ij| du_ik, which feature_adapter_ref.backward(hidden_err=du) adds to the kernel's own bound; grad_w1 reads hidden through its mask only and
keeps the kernel's bound."""
import os

import numpy as np
import pytest
import torch

import feature_adapter_ref as R
import test_gpu_feature_adapter_kernels as K
import test_gpu_tip_adapter as T

pytestmark = pytest.mark.gpu


def test_feature_adapter_fn_against_float64_autograd():
    import grip_amd  # noqa: F401
    from grip_amd import native
    from grip_amd.engine import FeatureAdapterFn, feature_adapter
    n, e, h, r = 16, 64, 16, 0.2
    f, w1, w2, G = (t.cuda() for t in R.inputs(n, e, h, 0))
    fwd = R.forward(f, w1, w2, r)
    assert R.doubtful(fwd) == 0, "a pre-activation lies within its forward bound of zero: another seed"
    a64, b64 = w1.double().requires_grad_(True), w2.double().requires_grad_(True)
    ref = r * torch.relu(torch.relu(f.double() @ a64.T) @ b64.T) + (1 - r) * f.double()
    (ref * G.double()).sum().backward()
    bwd = R.backward(f, w2, fwd["H"], fwd["x"], G, r, hidden_err=fwd["du"])
    assert torch.allclose(bwd["grad_w1"], a64.grad, rtol=1e-10, atol=1e-13 * float(a64.grad.abs().max()))      # the two float64 statements agree
    assert torch.allclose(bwd["grad_w2"], b64.grad, rtol=1e-10, atol=1e-13 * float(b64.grad.abs().max()))
    a, b = w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
    out = FeatureAdapterFn.apply(f, a, b, r)
    (out * G).sum().backward()
    K._check("FeatureAdapterFn", "out", out.detach(), ref.detach(), fwd["b_out"])
    K._check("FeatureAdapterFn", "w1.grad", a.grad, a64.grad, bwd["b_w1"])
    K._check("FeatureAdapterFn", "w2.grad", b.grad, b64.grad, bwd["b_w2"])
    assert a.grad.shape == w1.shape and b.grad.shape == w2.shape and f.grad is None
    assert torch.equal(feature_adapter(f, w1, w2, r), out.detach())      # the inference call: same bits, no hidden tensor in memory
    # one weight frozen: the other still gets its gradient
    a2 = w1.clone().requires_grad_(True)
    (FeatureAdapterFn.apply(f, a2, w2, r) * G).sum().backward()
    assert torch.equal(a2.grad, a.grad)
    with pytest.raises(native.GripError, match="img_emb requires grad"):
        FeatureAdapterFn.apply(f.clone().requires_grad_(True), a, b, r)
    with pytest.raises(native.GripError, match="expected"):
        feature_adapter(f, w2, w1, r)


def _batches(n, c, e, count, seed):
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(c, e, generator=g)
    out = []
    for _ in range(count):
        labels = torch.randint(0, c, (n,), generator=g)
        f = (centers[labels] + 0.8 * torch.randn(n, e, generator=g)) * (0.5 + 4 * torch.rand(n, 1, generator=g))
        out.append((f.cuda(), labels.cuda().to(torch.int32)))
    return centers.cuda(), out


def test_graphed_adapter_step_equals_eager():
    import grip_amd  # noqa: F401
    from grip_amd import steps
    from grip_amd.models import ClipAdapterModel
    n, c, e = 16, 5, 64
    text, batches = _batches(n, c, e, 3, 21)
    w = torch.full((n,), 1.0 / n, device="cuda")
    # capture, replay, a batch of another size (the eager step), replay again
    plan = [(batches[0][0], batches[0][1], w), (batches[1][0], batches[1][1], w), (batches[2][0][:5], batches[2][1][:5], w[:5] * n / 5),
            (batches[2][0], batches[2][1], w)]
    out = []
    for graphed in (False, True):
        model = ClipAdapterModel(e, reduction=4, ratio=0.2, seed=3, device="cuda")
        opt = torch.optim.AdamW([model.w1, model.w2], lr=1e-2, eps=1e-4)
        step = steps.GraphedAdapterStep(model, text, 30.0, opt) if graphed else None
        losses, traj = [], []
        for f, y, rw in plan:
            loss = step(f, y, rw) if graphed else steps.adapter_step(model, f, text, 30.0, y, rw, opt)
            losses.append(float(loss))
            traj.append((model.w1.detach().clone(), model.w2.detach().clone()))
        out.append((losses, traj))
    (l_e, t_e), (l_g, t_g) = out
    assert l_e == l_g, (l_e, l_g)
    assert all(torch.equal(a1, b1) and torch.equal(a2, b2) for (a1, a2), (b1, b2) in zip(t_e, t_g))
    assert not torch.equal(t_e[0][0], t_e[3][0]) and not torch.equal(t_e[0][1], t_e[3][1])


def test_model_rows_do_not_depend_on_the_split():
    import grip_amd  # noqa: F401
    from grip_amd.models import ClipAdapterModel
    model = ClipAdapterModel(128, seed=5, device="cuda")
    f = R.inputs(70, 128, 32, 9)[0].cuda()
    with torch.no_grad():
        whole = model(f)
        for cut in (16, 1):
            assert torch.equal(torch.cat([model(f[:cut]), model(f[cut:])]), whole), f"split {cut} / {70 - cut}"
    assert torch.equal(model(f).detach(), whole) and model(f).requires_grad      # the training forward returns the same bits
    assert whole.shape == f.shape and not torch.equal(whole, f)


# ---------------------------------------------------------------------------------------------------------------- strategy (tiny towers)
def test_strategy_clip_adapter(tmp_path):
    from grip_amd.engine import cosine_head
    from grip_amd.models import ClipAdapterModel
    from grip_amd.utils import compute_metrics as cm
    off, on = T._run(tmp_path), T._run(tmp_path, CLIP_ADAPTER=True)
    # the pseudolabel pass and the prompt training are untouched: same lists, same prompt, byte-identical prompt file
    assert (on["data"]["train"].filepaths, on["data"]["train"].labels) == (off["data"]["train"].filepaths, off["data"]["train"].labels)
    assert len(on["prompt"]) == len(off["prompt"]) and all(np.array_equal(a, b) for a, b in zip(on["prompt"], off["prompt"]))
    assert on["best"] == off["best"]
    m, other = on["m"], off["m"]
    assert other.adapter is None and isinstance(m.adapter, ClipAdapterModel) and m.adapter.w1.is_cuda
    assert (m.adapter.embed_dim, m.adapter.hidden_dim, m.adapter.ratio, m.adapter.seed) == (256, 64, 0.2, 1)      # OPTIM_SEED = 1
    assert len(m.adapter_losses) == 20 and m.adapter_losses[-1] < m.adapter_losses[0], m.adapter_losses
    fresh = ClipAdapterModel(256, seed=1)
    assert not torch.equal(m.adapter.w1.detach().cpu(), fresh.w1.detach()) and not torch.equal(m.adapter.w2.detach().cpu(), fresh.w2.detach())
    assert not torch.equal(on["logits"], off["logits"])
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        fn_off = cm.save_parameters(off["prompt"], off["conf"])
        with open(fn_off, "rb") as fh:
            bytes_off = fh.read()
        fn = cm.save_parameters(on["prompt"], on["conf"], adapter=m.adapter)
        path = cm.adapter_path(on["conf"])
        assert fn == fn_off and os.path.exists(path) and path == fn[:-len(".pickle")] + "_adapter.pickle"
        with open(fn, "rb") as fh:
            assert fh.read() == bytes_off
        # the adapter file round-trips through predict on the strategy that was trained without it ...
        loaded = other.load_feature_adapter(path)
        try:
            _, again = other.predict(off["data"]["test"], off["classes"])
            # ... and predict is cosine_head(adapter(frozen features), text features)
            test = off["data"]["test"]
            with torch.no_grad():
                tf = other.frozen_image_features(test.images)
                text = other.features(test.images[:1], off["classes"])[1]
                manual = cosine_head(loaded(tf), text, other.scale(), want_probs=False)[0]
        finally:
            other.adapter = None
        _, plain = other.predict(off["data"]["test"], off["classes"])
    finally:
        os.chdir(cwd)
    assert torch.equal(again, on["logits"]) and torch.equal(manual.cpu(), on["logits"]) and torch.equal(plain, off["logits"])
    # another BATCH_SIZE: the same logits bit for bit
    keep = m.config.BATCH_SIZE
    try:
        for bs in (4, 16):
            m.config.BATCH_SIZE = bs
            assert torch.equal(m.predict(on["data"]["test"], on["classes"])[1], on["logits"]), f"BATCH_SIZE {bs}"
    finally:
        m.config.BATCH_SIZE = keep
    # training it again gives the same adapter, and the global torch RNG is not read
    first = (m.adapter.w1.detach().clone(), m.adapter.w2.detach().clone(), list(m.adapter_losses))
    state = torch.get_rng_state()
    m.build_feature_adapter(on["data"]["train"])
    assert torch.equal(torch.get_rng_state(), state), "the global torch RNG moved"
    assert torch.equal(m.adapter.w1.detach(), first[0]) and torch.equal(m.adapter.w2.detach(), first[1]) and m.adapter_losses == first[2]
