"""The test-time episode (tpt.TestTimeTuner) on the small synthetic model the other step tests use: the context gradient of ViewEntropyFn through
CosineHeadFn and the text tower against the same chain under torch's log_softmax-based loss; an item's row the same with and without a host
synchronisation between episodes and whatever episodes ran before it; the context, its .grad and the strategy's SGD state untouched by an episode; a
deep-CoOp model's deep prompts frozen; steps = 2 differs from steps = 1; lr = 0 gives the plain row of view 0.  (The episode runs eagerly: a graphed
episode is not built, so there is no graphed row to compare.)"""
import numpy as np
import pytest
import torch

import view_entropy_ref as R

pytestmark = pytest.mark.gpu
C, V, KEEP = 5, 4, 2


def _setup(deep=False, views=V):
    import grip_amd  # noqa: F401
    from grip_amd import clip, rng
    from grip_amd.models import CustomTextEncoder, TextPrefixModel
    m, _ = clip.load("small", device="cuda")
    classes = [f"class {i}" for i in range(C)]
    N = lambda name, shape: torch.from_numpy(rng.normal(4, rng.stream_id(name), shape, 0.0, 0.02)).cuda()   # noqa: E731
    d = m.dims
    tm = TextPrefixModel(N("tpt.p", (1, 4, d.transformer_width)), CustomTextEncoder(m, "cuda", torch.float32), classes, device="cuda",
                         deep_prefix=N("tpt.d", (d.transformer_layers - 1, 4, d.transformer_width)) if deep else None)
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        feats = m.encode_image(torch.randn(3 * views, 3, 64, 64, device="cuda", generator=g)).float().view(3, views, -1)      # three items
    return m, tm, feats


def _prefix_grad(tm, m, x, loss_of_logits, grad_logits=None):
    """(the context gradient, the logits) of the chain context -> text tower -> cosine head -> loss_of_logits (or, with grad_logits, of <grad_logits, logits>)."""
    from grip_amd.engine import CosineHeadFn
    tm.prefix.grad = None
    logits = CosineHeadFn.apply(x, tm(tm.classes), m.logit_scale.exp().item())
    if grad_logits is None:
        loss_of_logits(logits).backward()
    else:
        logits.backward(gradient=grad_logits)
    g, tm.prefix.grad = tm.prefix.grad.detach().clone(), None
    return g, logits.detach()


def test_the_context_gradient_against_the_same_chain_under_torchs_loss():
    """The project states no bound for the whole chain text tower -> head, so (the second form the issue names) the reference is the SAME f32 chain under
    torch's log_softmax-based loss on the kernel's selection.  The backward of the chain is a linear map J^T of the logits gradient.  The two logits
    gradients differ by at most 2 bgrad (view_entropy_ref's bound of a gradient element against float64, once for each side), so the context gradients
    differ by at most |J|^T (2 bgrad) -- |J| is read off the chain itself, one backward per logits element (V C = 20 of them) -- plus what the backward's
    own rounding adds on either side (f16 towers): E, the largest element of Bwd(b1) + Bwd(b2) - Bwd(b1 + b2) for the torch gradient b split into its
    even and odd rows; a property of the existing backward on these inputs, not of the kernel under test.  Margin: |J|^T (2 bgrad) + 2 E.
    E is MEASURED here, at run time, so this last comparison is INFORMATIVE: it says the two chains agree to the backward's own noise and prints which
    term governs (carried / E).  What would catch a wrong kernel gradient are the two exact assertions before it: the kernel's logits gradient is within
    bgrad (derived, nothing measured) of float64 on the step's own logits, and ViewEntropyFn hands exactly that gradient to the chain (torch.equal of
    the context gradients)."""
    from grip_amd import engine
    m, tm, feats = _setup()
    x = feats[0].contiguous()
    ga, logits = _prefix_grad(tm, m, x, lambda lg: engine.ViewEntropyFn.apply(lg, V, KEEP))
    _, grad_k, sel = engine.view_entropy(logits, V, KEEP, want_selected=True)
    idx = torch.nonzero(sel[0]).flatten()

    def torch_loss(lg):
        lp = torch.log_softmax(lg[idx], dim=1)
        avg = torch.logsumexp(lp, dim=0) - float(np.log(KEEP))
        return -(avg.exp() * avg).sum()
    gb, _ = _prefix_grad(tm, m, x, torch_loss)
    leaf = logits.clone().requires_grad_(True)
    torch_loss(leaf).backward()
    b = leaf.grad
    # the autograd twin hands the kernel's gradient to the chain as it is
    assert torch.equal(_prefix_grad(tm, m, x, None, grad_k)[0], ga)
    ref = R.run64(logits.cpu().numpy().reshape(1, V, C), KEEP, selection=sel.cpu().numpy().astype(bool))
    assert (np.abs(grad_k.cpu().numpy().reshape(1, V, C).astype(np.float64) - ref["grad"]) <= ref["bgrad"]).all()
    beta = torch.from_numpy(2.0 * ref["bgrad"].reshape(V, C)).cuda()
    absj = torch.zeros(V, C, *tm.prefix.shape, dtype=torch.float64, device="cuda")
    for p in range(V):
        for j in range(C):
            one = torch.zeros(V, C, device="cuda")
            one[p, j] = 1.0
            absj[p, j] = _prefix_grad(tm, m, x, None, one)[0].double().abs()
    carried = (absj * beta[:, :, None, None, None]).sum((0, 1))
    even = b.clone()
    even[1::2] = 0
    noise = (_prefix_grad(tm, m, x, None, even)[0].double() + _prefix_grad(tm, m, x, None, b - even)[0].double() - _prefix_grad(tm, m, x, None, b)[0].double()).abs().max()
    err = (ga.double() - gb.double()).abs()
    print(f"context gradient vs torch's loss: worst |diff| {float(err.max()):.3e}, |grad| up to {float(gb.abs().max()):.3e}, carried bound up to "
          f"{float(carried.max()):.3e}, the backward's own noise E {float(noise):.3e}, carried / E {float(carried.max()) / max(float(noise), 1e-300):.3e}")
    assert float(gb.abs().max()) > 0 and (err <= carried + 2 * noise).all()


def _tuner(tm, m, **kw):
    from grip_amd import tpt
    return tpt.TestTimeTuner(tm, m, **{"views": V, "rho": 0.5, **kw})


def test_an_items_row_does_not_depend_on_the_episodes_around_it():
    m, tm, feats = _setup()
    before = tm.prefix.detach().clone()
    rows = {}
    for steps in (1, 2):
        t = _tuner(tm, m, steps=steps)
        synced = []
        for i in (0, 1, 2):
            synced.append(t.tune(feats[i]).clone())
            torch.cuda.synchronize()
        queued = [t.tune(feats[i % 3]).clone() for i in range(24)]      # enqueued back to back, no host synchronisation in between
        torch.cuda.synchronize()
        assert all(torch.equal(r, synced[i % 3]) for i, r in enumerate(queued)), f"an item's row depends on the episodes before it (steps = {steps})"
        assert t.episodes == 27 and torch.equal(tm.prefix.detach(), before)
        rows[steps] = synced
    assert not torch.equal(rows[1][0], rows[2][0]), "a second step changes nothing"
    assert rows[1][0].shape == (C,) and all(torch.isfinite(r).all() for r in rows[2])


def test_rows_at_vitb16_shapes_do_not_depend_on_the_episodes_around_them():
    """The shapes an episode has in use (BASELINE.json configs[1]: C = 102, P = 16, V = 64, the ViT-B/16 text tower, where other kernels run than on the
    small towers): rows of episodes enqueued back to back with no host synchronisation are the rows of episodes synchronised one by one."""
    import bench
    from grip_amd import clip, rng, tpt
    from grip_amd.models import CustomTextEncoder, TextPrefixModel
    Cb, Pb, Vb = 102, 16, 64
    m, _ = clip.load("ViT-B/16", device="cuda")
    classes = [f"class_{i}" for i in range(Cb)]
    enc = CustomTextEncoder(m, "cuda", torch.float32)
    enc._tok_cache[(Pb, tuple(classes))] = bench.synth_tokens(Cb, Pb).cuda()      # no tokenizer needed
    tm = TextPrefixModel(torch.from_numpy(rng.normal(1, rng.stream_id("bench.prefix"), (1, Pb, m.dims.transformer_width), 0.0, 0.02)).cuda(), enc, classes,
                         device="cuda")
    feats = torch.randn(4, Vb, m.dims.embed_dim, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    before = tm.prefix.detach().clone()
    t = tpt.TestTimeTuner(tm, m, views=Vb)
    synced = []
    for i in range(4):
        synced.append(t.tune(feats[i]).clone())
        torch.cuda.synchronize()
    queued = [t.tune(feats[i % 4]).clone() for i in range(24)]
    torch.cuda.synchronize()
    assert all(torch.equal(r, synced[i % 4]) for i, r in enumerate(queued)) and torch.equal(tm.prefix.detach(), before)
    assert t.keep == 6 and all(torch.isfinite(r).all() for r in synced) and not torch.equal(synced[0], synced[1])


def test_an_episode_leaves_the_context_its_grad_and_the_strategys_optimizer_alone():
    from grip_amd import engine, steps as gsteps
    m, tm, feats = _setup()
    opt = torch.optim.SGD([tm.prefix], lr=0.1, momentum=0.9, weight_decay=0.1)      # the strategy's optimizer, with a momentum buffer to disturb
    y, w = torch.arange(V, device="cuda", dtype=torch.int32) % C, torch.full((V,), 1 / V, device="cuda")
    gsteps.coop_step(tm, m, None, y, w, opt, image_features=feats[1])
    sentinel = torch.full_like(tm.prefix, 0.25)
    tm.prefix.grad = sentinel
    before = tm.prefix.detach().clone()
    state = {k: v.clone() if torch.is_tensor(v) else v for k, v in opt.state[tm.prefix].items()}
    assert "momentum_buffer" in state
    t = _tuner(tm, m)
    with torch.no_grad():      # (the inference forward, as `predict` runs it)
        plain = engine.cosine_head(feats[0][:1].contiguous(), tm(tm.classes), m.logit_scale.exp().item(), want_probs=False)[0][0]
    row = t.tune(feats[0])
    assert not torch.equal(row, plain), "the episode changed nothing"
    assert torch.equal(tm.prefix.detach(), before) and tm.prefix.requires_grad
    assert tm.prefix.grad is sentinel and torch.equal(sentinel, torch.full_like(sentinel, 0.25))
    after = opt.state[tm.prefix]
    assert set(after) == set(state) and all(torch.equal(after[k], v) if torch.is_tensor(v) else after[k] == v for k, v in state.items())
    assert len(opt.state) == 1 and t._optimizer is not opt
    # lr = 0: the row is the plain row of view 0, bit for bit (AdamW at lr 0 multiplies by 1 and adds -0)
    zero = _tuner(tm, m, lr=0.0)
    assert torch.equal(zero.tune(feats[0]), plain) and torch.equal(tm.prefix.detach(), before)
    # steps = 0 likewise
    assert torch.equal(_tuner(tm, m, steps=0).tune(feats[0]), plain)


def test_a_deep_coop_models_deep_prompts_stay_frozen():
    m, tm, feats = _setup(deep=True)
    deep_before, prefix_before = tm.deep_prefix.detach().clone(), tm.prefix.detach().clone()
    assert tm.deep_prefix.requires_grad and tm.deep_prefix.grad is None
    rows = [_tuner(tm, m).tune(feats[0]) for _ in range(2)]
    assert torch.equal(rows[0], rows[1]) and torch.isfinite(rows[0]).all()
    assert tm.deep_prefix.grad is None and tm.deep_prefix.requires_grad and torch.equal(tm.deep_prefix.detach(), deep_before)
    assert torch.equal(tm.prefix.detach(), prefix_before)


def test_the_tuner_refuses_features_of_another_shape():
    m, tm, feats = _setup()
    with pytest.raises(ValueError, match="view features"):
        _tuner(tm, m).tune(feats[0][:3])
