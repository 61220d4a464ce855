"""Deep UPT (grip_upt_mixer_*_deep): vpt_embeddings_deep [D, P, dv] joins the UPT mixer's sequence (length 2 + D) and the deep rows of its
output become the image tower's deep prompts -- the reference's models/prompts_models.py:129-146 as :133-134 and :146 intend.  The mixer's
outputs and all 23 gradients against a float64 restatement, the n_deep = 0 bits, the framework path, UPTModel end to end, the graphed step,
a multimodal strategy and the refusals."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(P, dt, dv, D, nd, dtype, seed=0, mix_deep=True):
    import grip_amd  # noqa: F401
    from grip_amd.models import UPTModel
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    coop = (torch.randn(1, P, dt, generator=g) * 0.02).to(dtype).cuda()
    vpt = (torch.randn(1, P, dv, generator=g) * 0.02).to(dtype).cuda()
    deep = (torch.randn(nd, P, dv, generator=g) * 0.02).to(dtype).cuda()
    m = UPTModel(coop, vpt, deep, None, None, ["a"], D, device="cuda", dtype=dtype, mix_deep=mix_deep)
    with torch.no_grad():     # LayerNorm affine and biases away from their init so that their gradients are exercised
        for n, p in m.named_parameters():
            if n.endswith("bias") or "ln_" in n:
                p.add_((torch.randn(p.shape, generator=g) * 0.1).to(p.dtype).cuda())
    return m


def _reference_mix_deep(m, dd=torch.float64):
    """The deep mix in float64 on the CPU: proj_vpt_pre(cat(vpt, deep)), the block over the sequence of 2 + D tokens, the fp16 round trip,
    proj_vpt_post of the visual rows.  The float16 branch rounds every projection's output to fp16 (and, through autograd, the gradient
    arriving there)."""
    sd = {k: v.detach().cpu().to(dd).requires_grad_(True) for k, v in m.named_parameters()}
    half = m.dtype == torch.float16
    r16 = (lambda t: t.to(torch.float16).to(dd)) if half else (lambda t: t)        # noqa: E731
    lin = lambda x, w, b: x @ sd[w].t() + sd[b]      # noqa: E731
    coop, vpt, deep = sd["coop_embeddings"], sd["vpt_embeddings"], sd["vpt_embeddings_deep"]
    x = torch.cat((r16(lin(coop, "proj_coop_pre.weight", "proj_coop_pre.bias")),
                   r16(lin(torch.cat((vpt, deep)), "proj_vpt_pre.weight", "proj_vpt_pre.bias"))), dim=0)     # [2 + D, P, dim]
    D = x.shape[-1]
    pre = "transformer.resblocks.0."
    ln = lambda t, w, b: torch.nn.functional.layer_norm(t, (D,), sd[pre + w], sd[pre + b], 1e-5)      # noqa: E731
    y = ln(x, "ln_1.weight", "ln_1.bias")
    q, k, v = lin(y, pre + "attn.in_proj_weight", pre + "attn.in_proj_bias").chunk(3, dim=-1)
    att = torch.einsum("lnd,mnd->nlm", q, k) / D ** 0.5
    o = torch.einsum("nlm,mnd->lnd", att.softmax(-1), v)
    x = x + lin(o, pre + "attn.out_proj.weight", pre + "attn.out_proj.bias")
    h = lin(ln(x, "ln_2.weight", "ln_2.bias"), pre + "mlp.c_fc.weight", pre + "mlp.c_fc.bias")
    x = x + lin(h * torch.sigmoid(1.702 * h), pre + "mlp.c_proj.weight", pre + "mlp.c_proj.bias")
    out = x.to(torch.float16).to(dd)
    vpt_all = r16(lin(out[1:], "proj_vpt_post.weight", "proj_vpt_post.bias"))
    return r16(lin(out[:1], "proj_coop_post.weight", "proj_coop_post.bias")), vpt_all[:1], vpt_all[1:], sd


def _check_against_reference(m, rtol, grad_cos, grad_rel):
    P, dt, dv, nd = m.coop_length, m.coop_dim, m.vpt_dim, m.vpt_embeddings_deep.shape[0]
    assert m._native_mixer_ok()
    ce, ve, de = m.mix()
    assert ce.shape == (1, P, dt) and ve.shape == (1, P, dv) and de.shape == (nd, P, dv)
    g = torch.Generator().manual_seed(5)
    ws = [torch.randn(t.shape, generator=g) for t in (ce, ve, de)]
    sum((t.float() * w.cuda()).sum() for t, w in zip((ce, ve, de), ws)).backward()
    ref = _reference_mix_deep(m)
    sum((t * w.double()).sum() for t, w in zip(ref[:3], ws)).backward()
    for got, want in zip((ce, ve, de), ref[:3]):
        want = want.detach()
        torch.testing.assert_close(got.detach().cpu().double(), want, rtol=rtol, atol=rtol * want.abs().max().item())
    seen = 0
    for name, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == p.dtype, name
        want = ref[3][name].grad
        got = p.grad.detach().cpu().double()
        cos = torch.nn.functional.cosine_similarity(got.reshape(-1), want.reshape(-1), dim=0).item()
        rel = ((got - want).norm() / want.norm().clamp_min(1e-30)).item()
        assert cos >= 1 - grad_cos and rel <= grad_rel, f"{name}: cos {cos:.6f} rel {rel:.2e}"
        seen += 1
    assert seen == 23


@pytest.mark.parametrize("P,dt,dv,D,nd", [(4, 512, 768, 128, 11), (16, 768, 1024, 128, 23), (1, 512, 768, 64, 1), (3, 192, 320, 256, 2)])
def test_deep_mixer_forward_and_all_gradients(P, dt, dv, D, nd):
    _check_against_reference(_model(P, dt, dv, D, nd, torch.float32), 2e-3, 1e-4, 1e-2)


def test_deep_mixer_float16_branch():
    """multimodal_prompt.py:46's float16 branch (half_linears) with deep embeddings, against the float64 graph with the same fp16 rounding points."""
    _check_against_reference(_model(4, 512, 768, 128, 11, torch.float16, seed=4), 4e-3, 1e-3, 3e-2)


def _struct(m, tensors):
    from grip_amd import native
    return native.UptMixer(m.coop_length, m.coop_dim, m.vpt_dim, m.transformer.width, 0, 0, *[t.data_ptr() for t in tensors])


def _mixer_tensors(m):
    b = m.transformer.resblocks[0]
    ts = [m.coop_embeddings, m.vpt_embeddings, m.proj_coop_pre.weight, m.proj_coop_pre.bias, m.proj_vpt_pre.weight, m.proj_vpt_pre.bias, b.ln_1.weight,
          b.ln_1.bias, b.attn.in_proj_weight, b.attn.in_proj_bias, b.attn.out_proj.weight, b.attn.out_proj.bias, b.ln_2.weight, b.ln_2.bias,
          b.mlp.c_fc.weight, b.mlp.c_fc.bias, b.mlp.c_proj.weight, b.mlp.c_proj.bias, m.proj_coop_post.weight, m.proj_coop_post.bias,
          m.proj_vpt_post.weight, m.proj_vpt_post.bias]
    return [t.detach().contiguous() for t in ts]


def test_n_deep_zero_gives_the_shallow_mixer_bits():
    from grip_amd import native
    lib = native.lib()
    m = _model(4, 512, 768, 128, 2, torch.float32, seed=7)
    ts = _mixer_tensors(m)
    P, dt, dv = 4, 512, 768
    n = ctypes.c_size_t()
    native.check(lib.grip_upt_mixer_deep_workspace(P, 0, dt, dv, 128, ctypes.byref(n)))
    g = torch.Generator(device="cuda").manual_seed(3)
    dc, dvv = torch.randn(P, dt, device="cuda", generator=g), torch.randn(P, dv, device="cuda", generator=g)
    res = []
    for deep_call in (False, True):
        ws = torch.zeros(n.value, dtype=torch.uint8, device="cuda")
        co, vo = torch.empty(P, dt, device="cuda"), torch.empty(P, dv, device="cuda")
        grads = [torch.full_like(t, float("nan")) for t in ts]
        s = torch.cuda.current_stream().cuda_stream
        mm, gg = _struct(m, ts), _struct(m, grads)
        if deep_call:
            native.check(lib.grip_upt_mixer_forward_deep(ctypes.byref(mm), None, 0, co.data_ptr(), vo.data_ptr(), None, ws.data_ptr(), n.value, s))
            native.check(lib.grip_upt_mixer_backward_deep(ctypes.byref(mm), None, 0, dc.data_ptr(), dvv.data_ptr(), None, ctypes.byref(gg), None,
                                                          ws.data_ptr(), n.value, s))
        else:
            native.check(lib.grip_upt_mixer_forward(ctypes.byref(mm), co.data_ptr(), vo.data_ptr(), ws.data_ptr(), n.value, s))
            native.check(lib.grip_upt_mixer_backward(ctypes.byref(mm), dc.data_ptr(), dvv.data_ptr(), ctypes.byref(gg), ws.data_ptr(), n.value, s))
        torch.cuda.synchronize()
        res.append((co, vo, grads))
    (a0, a1, ag), (b0, b1, bg) = res
    assert torch.equal(a0, b0) and torch.equal(a1, b1)
    assert all(torch.equal(x, y) for x, y in zip(ag, bg))


def test_deep_mixer_is_reproducible_and_equals_the_framework_path(monkeypatch):
    m = _model(4, 512, 768, 128, 11, torch.float32, seed=3)
    outs = []
    for native_on in ("1", "1", "0"):
        monkeypatch.setenv("GRIP_NATIVE_MIXER", native_on)
        assert m._native_mixer_ok() == (native_on == "1")
        m.zero_grad(set_to_none=True)
        ce, ve, de = m.mix()
        (ce.square().sum() + ve.square().sum() + de.square().sum()).backward()
        outs.append(((ce.detach().clone(), ve.detach().clone(), de.detach().clone()), {n: p.grad.clone() for n, p in m.named_parameters()}))
    a, b, t = outs
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(a[1][n], b[1][n]) for n in a[1])
    for x, y in zip(a[0], t[0]):
        torch.testing.assert_close(x, y, rtol=2e-3, atol=2e-3 * y.abs().max().item())
    assert len(a[1]) == 23
    for n in a[1]:
        cos = torch.nn.functional.cosine_similarity(a[1][n].reshape(-1), t[1][n].reshape(-1), dim=0).item()
        assert cos >= 1 - 1e-3, (n, cos)


def _small_upt(cm, classes, deep, mix_deep, seed=11):
    from grip_amd import rng
    from grip_amd.models import CustomImageEncoder, CustomTextEncoder, UPTModel
    N = lambda name, shape: torch.from_numpy(rng.normal(5, rng.stream_id(name), shape, 0.0, 0.02)).cuda()   # noqa: E731
    torch.manual_seed(seed)
    return UPTModel(N("ud.c", (1, 4, 256)), N("ud.v", (1, 4, 256)), None if deep is None else N("ud.d", (deep, 4, 256)), CustomImageEncoder(cm.visual),
                    CustomTextEncoder(cm, "cuda", torch.float32), classes, 128, device="cuda", dtype=torch.float32, mix_deep=mix_deep)


def _loss(um, x, classes):
    from grip_amd.engine import CosineHeadFn, WeightedCEFn
    t_out, v_out = um(x, classes)
    logits = CosineHeadFn.apply(v_out, t_out, 100.0)
    loss = WeightedCEFn.apply(logits, torch.arange(x.shape[0], device="cuda") % len(classes), torch.full((x.shape[0],), 1 / x.shape[0], device="cuda"))
    loss.backward()
    return t_out.detach(), v_out.detach()


def test_upt_model_mix_deep_end_to_end(monkeypatch):
    import grip_amd  # noqa: F401
    from grip_amd import clip
    from grip_amd.models import CustomImageEncoder
    cm, _ = clip.load("small", device="cuda")                # 3 vision blocks: D = 2 deep prompts
    classes = ["forest", "river", "sea lake", "highway"]
    x = torch.randn(6, 3, 64, 64, generator=torch.Generator().manual_seed(2)).cuda()
    trainable = lambda mod: {n: p for n, p in mod.named_parameters() if p.requires_grad}      # noqa: E731
    res = {}
    for native_mixer in ("1", "0"):
        monkeypatch.setenv("GRIP_NATIVE_MIXER", native_mixer)
        um = _small_upt(cm, classes, 2, True)
        assert um._native_mixer_ok() == (native_mixer == "1")
        t_out, v_out = _loss(um, x, classes)
        res[native_mixer] = {n: p.grad.detach().clone() for n, p in trainable(um).items()}
        if native_mixer == "1":
            _, vpt_all, deep_all = um.mix()      # the tower in train mode, as inside the model's forward
            want = CustomImageEncoder(cm.visual)(x, vpt_all.detach().requires_grad_(), deep_prompts=deep_all.detach().requires_grad_()).detach()
            assert torch.equal(v_out, want), "the image tower does not read the mixer's deep rows"
            assert um.vpt_embeddings_deep.grad is not None and um.vpt_embeddings_deep.grad.abs().sum() > 0
    assert len(res["1"]) == 23
    for n in res["0"]:
        cos = torch.nn.functional.cosine_similarity(res["1"][n].reshape(-1), res["0"][n].reshape(-1), dim=0).item()
        assert cos >= 1 - 1e-3, (n, cos)
    # mix_deep off: a given vpt_embeddings_deep changes nothing and gets no gradient
    monkeypatch.setenv("GRIP_NATIVE_MIXER", "1")
    off, plain = _small_upt(cm, classes, 2, False), _small_upt(cm, classes, None, False)
    a, b = _loss(off, x, classes), _loss(plain, x, classes)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert off.vpt_embeddings_deep.grad is None
    assert all(torch.equal(p.grad, trainable(plain)[n].grad) for n, p in trainable(off).items() if n != "vpt_embeddings_deep")


def test_graphed_deep_upt_step_equals_eager():
    import grip_amd  # noqa: F401
    from grip_amd import clip, steps
    cm, _ = clip.load("small", device="cuda")
    classes = [f"class {i}" for i in range(6)]
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(8, 3, 64, 64, device="cuda", generator=g) for _ in range(4)]
    ys = [torch.randint(0, 6, (8,), device="cuda", generator=g, dtype=torch.int32) for _ in range(4)]
    w = torch.full((8,), 1 / 8, device="cuda")
    res = {}
    for graphed in (False, True):
        um = _small_upt(cm, classes, 2, True)
        start = um.vpt_embeddings_deep.detach().clone()
        opt = torch.optim.SGD([p for p in um.parameters() if p.requires_grad], lr=0.1, weight_decay=0.1)
        step = steps.GraphedUptStep(um, 100.0, opt) if graphed else (lambda x, y, ww, _m=um, _o=opt: steps.upt_step(_m, 100.0, x, y, ww, _o))
        losses = [float(step(x, y, w)) for x, y in zip(xs, ys)]
        res[graphed] = (losses, [p.detach().clone() for p in um.parameters() if p.requires_grad], um.vpt_embeddings_deep.detach().clone())
    e, gr = res[False], res[True]
    assert e[0] == gr[0] and all(torch.equal(a, b) for a, b in zip(e[1], gr[1]))
    assert not torch.equal(gr[2], start), "the deep embeddings were not trained inside the graph"


def test_multimodal_strategy_with_upt_deep(tmp_path, monkeypatch):
    from test_gpu_strategies import _conf
    from grip_amd import pseudolabels as pl
    from grip_amd.data import TensorPoolDataset
    from grip_amd.methods import MultimodalPrompt
    from grip_amd.methods.main import synthetic_pool
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("GRIP_PSEUDOLABEL_MODE", raising=False)
    conf = _conf(MODEL="multimodal_prompt", LEARNING_PARADIGM="ssl", EPOCHS=2, LR=0.2, TEXT_PREFIX_SIZE=4, VISION_PREFIX_SIZE=4, UPT_DEEP=True)
    classes, files, images, names = synthetic_pool(4, 8, 64, 3)
    l2i = {c: i for i, c in enumerate(classes)}
    data = TensorPoolDataset(files, images.cuda(), labels=names, label_map=l2i)
    m = MultimodalPrompt(conf, l2i, classes, classes, classes, "cuda")
    m.define_model(classes)
    assert m.model.mix_deep and tuple(m.model.vpt_embeddings_deep.shape) == (2, 4, 256) and m.model._native_mixer_ok()
    before = m.model.vpt_embeddings_deep.detach().clone()
    loader = m._loader(data, True)
    for _ in range(2):
        m._train_epoch(loader)
    assert not torch.equal(m.model.vpt_embeddings_deep.detach(), before), "vpt_embeddings_deep did not change"
    snap = m.prompt_snapshot()
    assert snap[6] is not None and snap[6].shape == (2, 4, 256)
    pool = images.cuda()
    img, _ = m.trained_features(pool, classes)
    with torch.no_grad():
        _, vpt_all, deep_all = m.model.mix()
    want = pl.encode_pool(m.clip_model.visual.tower, pool, chunk=440, prefix=vpt_all, deep=deep_all)
    assert torch.equal(img, want), "the pool pass does not use the mixer's deep prompts"
    assert not torch.equal(img, pl.encode_pool(m.clip_model.visual.tower, pool, chunk=440, prefix=vpt_all))
    # the trained-prompt pseudolabel pass (identical mode): the f32 lists over the same prompts, deep ones included
    twin = m.clip_model.exact_twin()
    with torch.no_grad():
        txt, vprompt = m.trained_text_features(classes, twin)
        emb = pl.encode_pool(twin.visual.tower, pool, chunk=32, prefix=vprompt, deep=m.deep_prompts())
    want = pl.pseudolabel_from_features(emb, txt, m.scale(), list(files), [l2i[c] for c in classes], 3, argmax_on="logits")
    out = m.assign_pseudo_labels(3, TensorPoolDataset(files, pool, labels=None, label_map=l2i))
    assert (out.filepaths, out.labels) == want and len(want[0]) > 3


def test_deep_mixer_refusals():
    from grip_amd import native
    from grip_amd.engine import UptMixerFn
    lib = native.lib()
    m = _model(4, 512, 768, 128, 2, torch.float32, seed=1)
    ts = _mixer_tensors(m)
    mm = _struct(m, ts)
    n = ctypes.c_size_t()
    native.check(lib.grip_upt_mixer_deep_workspace(4, 2, 512, 768, 128, ctypes.byref(n)))
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    deep = m.vpt_embeddings_deep.detach()
    co, vo, do = torch.empty(4, 512, device="cuda"), torch.empty(4, 768, device="cuda"), torch.empty(2, 4, 768, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    fwd = lambda nd, dp=deep.data_ptr(), out=do.data_ptr(), nb=n.value: lib.grip_upt_mixer_forward_deep(      # noqa: E731
        ctypes.byref(mm), dp, nd, co.data_ptr(), vo.data_ptr(), out, ws.data_ptr(), nb, s)
    for nd in (-1, 32):
        assert fwd(nd) == 1 and b"out of range" in lib.grip_last_error()
    assert fwd(2, dp=None) == 1 and b"null vpt_deep" in lib.grip_last_error()
    assert fwd(2, out=None) == 1 and b"null vpt_deep" in lib.grip_last_error()
    assert fwd(2, nb=n.value - 4096) == 1 and b"workspace too small" in lib.grip_last_error()
    assert fwd(3) == 1 and b"workspace too small" in lib.grip_last_error()      # a workspace sized for n_deep = 2
    grads = [torch.empty_like(t) for t in ts]
    gg = _struct(m, grads)
    gd = torch.empty(2, 4, 768, device="cuda")
    bwd = lambda nd, gdp=gd.data_ptr(), g=gg, nb=n.value: lib.grip_upt_mixer_backward_deep(      # noqa: E731
        ctypes.byref(mm), deep.data_ptr(), nd, co.data_ptr(), vo.data_ptr(), do.data_ptr(), ctypes.byref(g), gdp, ws.data_ptr(), nb, s)
    assert bwd(40) == 1 and b"out of range" in lib.grip_last_error()
    assert bwd(2, gdp=None) == 1 and b"grad_vpt_deep" in lib.grip_last_error()
    bad = _struct(m, grads)
    bad.in_w = None
    assert bwd(2, g=bad) == 1 and b"every gradient buffer" in lib.grip_last_error()
    assert bwd(2, nb=1024) == 1 and b"workspace too small" in lib.grip_last_error()
    torch.cuda.synchronize()
    # the host: a deep tensor that is not [D, P, dv]
    wrong = torch.zeros(2, 3, 768, device="cuda")
    with pytest.raises(native.GripError, match="vpt_embeddings_deep"):
        UptMixerFn.apply(*ts, wrong)
    m.vpt_embeddings_deep = torch.nn.Parameter(wrong)
    assert not m._native_mixer_ok()          # never reaches the kernels; the framework's cat refuses it
    with pytest.raises(RuntimeError):
        m.mix()
