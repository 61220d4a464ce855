"""Coupled deep multimodal prompts (MaPLe) on the native coupling kernels (csrc/couple.hip): vis[l] = text_prompt[l] W[l]^T + b[l] per depth.
The kernels against float64 with a DERIVED bound, MaPLeModel end to end against the CPU oracle composed from the two pinned restatements
(tests/test_host_text_deep.py:oracle_text_deep_forward, tests/test_gpu_deep_prompts.py:oracle_deep_forward) plus torch.nn.functional.linear per
depth and CPU autograd, the framework path, the graphed step, a multimodal strategy and the D = 0 route.

The bound: an f32 dot product of length K, summed in any order, with or without fused multiply-adds, satisfies
|err| <= (K + 2) * 2^-24 * sum_k |x_k w_k| (the bias, where there is one, counts as one more term).  K = dt for the forward, dv for dX, P for dW
and db.  It is asserted element-wise; nothing in it comes from a measurement."""
import pytest
import torch

from test_gpu_deep_prompts import oracle_deep_forward
from test_host_text_deep import oracle_text_deep_forward

pytestmark = pytest.mark.gpu
SEED = 131
U = 2.0 ** -24
SHAPES = [(3, 1, 128, 128), (4, 1, 256, 256), (2, 8, 512, 768), (16, 11, 512, 768), (16, 11, 768, 1024), (4, 0, 512, 768)]


def _inputs(name, shape, std=1.0):
    import grip_amd  # noqa: F401
    from grip_amd import rng
    return torch.from_numpy(rng.normal(SEED, rng.stream_id(name), shape, 0.0, std))


def _operands(P, D, dt, dv):
    tag = f"{P}.{D}.{dt}.{dv}"
    ctx = _inputs(f"mp.ctx.{tag}", (P, dt))
    deep = _inputs(f"mp.deep.{tag}", (D, P, dt)) if D else None
    w = _inputs(f"mp.w.{tag}", (1 + D, dv, dt), dt ** -0.5)
    b = _inputs(f"mp.b.{tag}", (1 + D, dv), 0.1)
    dy = _inputs(f"mp.dy.{tag}", (1 + D, P, dv))
    return ctx, deep, w, b, dy


def _float64_products(ctx, deep, w, b, dy):
    """(value, magnitude sum) in float64 of Y, dX, dW, db; X / Y / dY stacked over the 1 + D depths."""
    X = (ctx[None] if deep is None else torch.cat((ctx[None], deep))).double()
    W, B, G = w.double(), b.double(), dy.double()
    Y = torch.einsum("lpk,lnk->lpn", X, W) + B[:, None, :]
    Ym = torch.einsum("lpk,lnk->lpn", X.abs(), W.abs()) + B.abs()[:, None, :]
    dX, dXm = torch.einsum("lpn,lnk->lpk", G, W), torch.einsum("lpn,lnk->lpk", G.abs(), W.abs())
    dW, dWm = torch.einsum("lpn,lpk->lnk", G, X), torch.einsum("lpn,lpk->lnk", G.abs(), X.abs())
    return (Y, Ym), (dX, dXm), (dW, dWm), (G.sum(1), G.abs().sum(1))


def _assert_within_bound(got, want, mag, K, what):
    err = (got.detach().cpu().double() - want).abs()
    bound = (K + 2) * U * mag
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: worst |err| / bound = {worst:.3f} (K = {K})")
    assert torch.isfinite(got).all() and (err <= bound).all(), f"{what}: |err| is {worst:.2f} x the (K + 2) 2^-24 sum|x w| bound, K = {K}"


def _run_couple(ctx, deep, w, b, dy):
    """(Y [1 + D, P, dv], dX [1 + D, P, dt], dW, db) of one forward + backward through MaPLeModel.couple()'s path for the current GRIP_NATIVE_COUPLE."""
    from grip_amd.models import MaPLeModel
    m = MaPLeModel(ctx[None].clone().cuda(), None if deep is None else deep.clone().cuda(), None, None, ["a"], device="cuda", vision_width=w.shape[1])
    with torch.no_grad():
        m.proj_weight.copy_(w.cuda())
        m.proj_bias.copy_(b.cuda())
    _, _, vis_prefix, vis_deep = m.couple()
    Y = vis_prefix[None] if deep is None else torch.cat((vis_prefix[None], vis_deep))
    (Y * dy.cuda()).sum().backward()
    dX = m.ctx.grad if deep is None else torch.cat((m.ctx.grad, m.compound_prompts_text.grad))
    return m, (Y.detach().clone(), dX.clone(), m.proj_weight.grad.clone(), m.proj_bias.grad.clone())


def _check_against_float64(P, D, dt, dv, outs, what):
    ctx, deep, w, b, dy = _operands(P, D, dt, dv)
    (Y, Ym), (dX, dXm), (dW, dWm), (db, dbm) = _float64_products(ctx, deep, w, b, dy)
    _assert_within_bound(outs[0], Y, Ym, dt, f"{what} forward")
    _assert_within_bound(outs[1], dX, dXm, dv, f"{what} dX")
    _assert_within_bound(outs[2], dW, dWm, P, f"{what} dW")
    _assert_within_bound(outs[3], db, dbm, P, f"{what} db")


@pytest.mark.parametrize("P,D,dt,dv", SHAPES)
def test_coupling_kernels_vs_float64(monkeypatch, P, D, dt, dv):
    monkeypatch.setenv("GRIP_NATIVE_COUPLE", "1")
    runs = []
    for _ in range(2):
        m, outs = _run_couple(*_operands(P, D, dt, dv))
        assert m._native_couple_ok()
        runs.append(outs)
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "the coupling kernels are not bit-reproducible"
    _check_against_float64(P, D, dt, dv, runs[0], f"native ({P}, {D}, {dt}, {dv})")


@pytest.mark.parametrize("P,D,dt,dv", SHAPES)
def test_framework_path_meets_the_same_bound(monkeypatch, P, D, dt, dv):
    """GRIP_NATIVE_COUPLE=0: the same f32 products of the same operands through torch.nn.functional.linear."""
    monkeypatch.setenv("GRIP_NATIVE_COUPLE", "0")
    m, outs = _run_couple(*_operands(P, D, dt, dv))
    assert not m._native_couple_ok()
    _check_against_float64(P, D, dt, dv, outs, f"framework ({P}, {D}, {dt}, {dv})")


def test_coupling_function_without_deep_prompts_and_no_grad():
    from grip_amd.engine import PromptCoupleFn, prompt_couple_forward
    ctx, deep, w, b, _ = _operands(2, 8, 512, 768)
    c, d, ww, bb = (t.cuda() for t in (ctx, deep, w, b))
    vp, vd = prompt_couple_forward(c, d, ww, bb)
    out = PromptCoupleFn.apply(c.clone().requires_grad_(True), d, ww, bb)
    assert torch.equal(out[0], vp) and torch.equal(out[1], vd)
    vp0, none = prompt_couple_forward(c[None], None, ww[:1], bb[:1])          # ctx as the model keeps it, [1, P, dt]
    assert none is None and torch.equal(vp0, vp)


@pytest.fixture(scope="module")
def models():
    import grip_amd  # noqa: F401
    from grip_amd import clip
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = clip.load(name, device="cuda")[0]
        return cache[name]
    return get


CLASSES = ["forest", "river", "sea lake", "annual crop land", "highway"]


def _maple_model(cm, name, P, D, classes=CLASSES):
    from grip_amd import config
    from grip_amd.models import CustomImageEncoder, CustomTextEncoder, MaPLeModel
    d = config.get_dims(name)
    ctx = _inputs(f"mm.ctx.{name}.{P}", (1, P, d.transformer_width), 0.02)
    deep = _inputs(f"mm.deep.{name}.{P}.{D}", (D, P, d.transformer_width), 0.02) if D else None
    torch.manual_seed(SEED)
    m = MaPLeModel(ctx.cuda(), None if deep is None else deep.cuda(), CustomImageEncoder(cm.visual), CustomTextEncoder(cm, "cuda", torch.float32), classes,
                   device="cuda")
    with torch.no_grad():        # biases away from nn.Linear's tiny init so that the visual prompts have the scale of trained ones
        m.proj_bias.add_(_inputs(f"mm.b.{name}.{D}", tuple(m.proj_bias.shape), 0.02).cuda())
    return m


@pytest.mark.parametrize("name,P,D", [("tiny", 3, 1), ("small", 4, 1), ("ViT-B/16", 4, 8), ("ViT-B/16", 16, 11)])
def test_maple_model_vs_oracle(models, monkeypatch, name, P, D):
    """Embeddings of both towers and the gradients of the four parameters of a fixed weighted sum of the logits, against the CPU oracle."""
    import numpy as np
    from conftest import oracle_clip
    from oracle import wrappers as W
    from test_gpu_backward import assert_grad_close
    from test_gpu_towers import assert_embeddings_close
    from grip_amd import config
    from grip_amd.engine import CosineHeadFn, text_prefix_forward
    monkeypatch.setenv("GRIP_NATIVE_COUPLE", "1")
    d = config.get_dims(name)
    om, _ = oracle_clip().load(name)
    cm = models(name)
    m = _maple_model(cm, name, P, D)
    assert m._native_couple_ok() and tuple(m.proj_weight.shape) == (1 + D, d.vision_width, d.transformer_width)
    B, C = 3, len(CLASSES)
    x = _inputs(f"mm.x.{name}", (B, 3, d.image_resolution, d.image_resolution))
    wts = _inputs(f"mm.w.{name}", (B, C))
    t_out, v_out = m(x.cuda(), CLASSES)
    logits = CosineHeadFn.apply(v_out, t_out, 100.0)
    (logits * wts.cuda()).sum().backward()
    # the oracle: nn.functional.linear per depth, the two block-by-block towers, the cosine head, CPU autograd
    lin = torch.nn.functional.linear
    trainable = {n: p for n, p in m.named_parameters() if p.requires_grad}       # (the frozen backbone is a registered sub-module)
    o = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in trainable.items()}
    ids = m.text_encoder._token_ids(P, CLASSES).cpu()
    vis_prefix = lin(o["ctx"][0], o["proj_weight"][0], o["proj_bias"][0])
    vis_deep = torch.stack([lin(o["compound_prompts_text"][l], o["proj_weight"][l + 1], o["proj_bias"][l + 1]) for l in range(D)])
    o_txt = oracle_text_deep_forward(om, ids, o["ctx"], o["compound_prompts_text"])
    o_img = oracle_deep_forward(om.visual, x, vis_prefix, vis_deep)
    o_logits, _ = W.cosine_head(o_img, o_txt, torch.tensor(np.log(100.0)))
    (o_logits * wts).sum().backward()
    assert_embeddings_close(t_out, o_txt.detach(), f"{name} MaPLe text embeddings D={D}")
    assert_embeddings_close(v_out, o_img.detach(), f"{name} MaPLe image embeddings D={D}")
    assert len(o) == 4
    for n, p in trainable.items():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32, n
        assert_grad_close(p.grad, o[n].grad, f"{name} MaPLe d loss / d {n}, D={D}")
    # the coupling's share arrived: ctx's gradient is not the text tower's alone
    ctx_only = m.ctx.detach().clone().requires_grad_(True)
    t_alone = text_prefix_forward(cm.text_tower, m.text_encoder._token_ids(P, CLASSES), ctx_only, deep=m.compound_prompts_text.detach())
    (CosineHeadFn.apply(v_out.detach(), t_alone, 100.0) * wts.cuda()).sum().backward()
    assert torch.isfinite(ctx_only.grad).all() and not torch.allclose(ctx_only.grad, m.ctx.grad, rtol=1e-3, atol=0.0)


def test_graphed_maple_step_equals_eager(models):
    from grip_amd import steps
    cm = models("small")
    classes = [f"class {i}" for i in range(6)]
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(8, 3, 64, 64, device="cuda", generator=g) for _ in range(3)]
    ys = [torch.randint(0, 6, (8,), device="cuda", generator=g, dtype=torch.int32) for _ in range(3)]
    w = torch.full((8,), 1 / 8, device="cuda")
    res = {}
    for graphed in (False, True):
        m = _maple_model(cm, "small", 4, 1, classes)
        assert m._native_couple_ok()
        params = [p for p in m.parameters() if p.requires_grad]
        start = [p.detach().clone() for p in params]
        opt = torch.optim.SGD(params, lr=0.1, weight_decay=0.1)
        step = steps.GraphedUptStep(m, 100.0, opt) if graphed else (lambda x, y, ww, _m=m, _o=opt: steps.upt_step(_m, 100.0, x, y, ww, _o))
        losses = [float(step(x, y, w)) for x, y in zip(xs, ys)]
        res[graphed] = (losses, [p.detach().clone() for p in params], start)
    e, gr = res[False], res[True]
    assert e[0] == gr[0] and all(torch.equal(a, b) for a, b in zip(e[1], gr[1]))
    assert len(gr[1]) == 4 and all(not torch.equal(a, b) for a, b in zip(gr[1], gr[2])), "a parameter did not move inside the graph"


def test_multimodal_strategy_with_maple(tmp_path, monkeypatch):
    from test_gpu_strategies import _conf
    from grip_amd import pseudolabels as pl
    from grip_amd.data import TensorPoolDataset
    from grip_amd.methods import MultimodalPrompt
    from grip_amd.methods.main import synthetic_pool
    from grip_amd.models import MaPLeModel
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("GRIP_PSEUDOLABEL_MODE", raising=False)
    monkeypatch.setenv("GRIP_NATIVE_COUPLE", "1")
    conf = _conf(MODEL="multimodal_prompt", LEARNING_PARADIGM="ssl", EPOCHS=2, LR=0.2, TEXT_PREFIX_SIZE=4, VISION_PREFIX_SIZE=4, MAPLE=True)
    classes, files, images, names = synthetic_pool(4, 8, 64, 3)
    l2i = {c: i for i, c in enumerate(classes)}
    data = TensorPoolDataset(files, images.cuda(), labels=names, label_map=l2i)
    m = MultimodalPrompt(conf, l2i, classes, classes, classes, "cuda")
    m.define_model(classes)
    assert isinstance(m.model, MaPLeModel) and m.model._native_couple_ok()
    assert tuple(m.model.compound_prompts_text.shape) == (1, 4, 256) and tuple(m.model.proj_weight.shape) == (2, 256, 256)
    params = [p for p in m.model.parameters() if p.requires_grad]
    before = [p.detach().clone() for p in params]
    assert len(params) == 4
    loader = m._loader(data, True)
    losses = [m._train_epoch(loader)[0] for _ in range(2)]
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses[1] < losses[0], losses
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, params)), "a MaPLe parameter did not change"
    snap = m.prompt_snapshot()
    assert [None if s is None else s.shape for s in snap] == [(1, 4, 256), (1, 4, 256), (2, 256, 256), (2, 256)]
    pool = images.cuda()
    img, txt = m.trained_features(pool, classes)
    with torch.no_grad():
        ctx, deep_text, vis_prefix, vis_deep = m.model.couple()
        t_want = m.model.text_encoder(ctx, classes, deep_prompts=deep_text)
    want = pl.encode_pool(m.clip_model.visual.tower, pool, chunk=440, prefix=vis_prefix, deep=vis_deep)
    assert torch.equal(img, want) and torch.equal(txt, t_want), "the pool pass does not read the coupled prompts"
    assert not torch.equal(img, pl.encode_pool(m.clip_model.visual.tower, pool, chunk=440, prefix=vis_prefix))
    assert torch.equal(m.deep_prompts(), vis_deep)
    # predict() goes through the model's own forward
    pred, logits = m.predict(data, classes)
    assert logits.shape == (len(files), len(classes)) and torch.isfinite(logits).all()
    # the trained-prompt pseudolabel pass (identical mode) returns the exact mode's lists over the same coupled prompts
    twin = m.clip_model.exact_twin()
    with torch.no_grad():
        e_txt, vprompt = m.trained_text_features(classes, twin)
        emb = pl.encode_pool(twin.visual.tower, pool, chunk=32, prefix=vprompt, deep=m.deep_prompts())
    want = pl.pseudolabel_from_features(emb, e_txt, m.scale(), list(files), [l2i[c] for c in classes], 3, argmax_on="logits")
    out = m.assign_pseudo_labels(3, TensorPoolDataset(files, pool, labels=None, label_map=l2i))
    assert (out.filepaths, out.labels) == want and len(want[0]) > 3


def test_depth_zero_launches_no_deep_tower_call(models, monkeypatch):
    from grip_amd import native
    from grip_amd.engine import CosineHeadFn
    cm = models("small")
    m = _maple_model(cm, "small", 4, 0)
    params = [p for p in m.parameters() if p.requires_grad]
    assert m.compound_prompts_text is None and len(params) == 3 and m._native_couple_ok()
    x = _inputs("mm.x0", (4, 3, 64, 64)).cuda()
    with torch.no_grad():
        vis_prefix = m.couple()[2]
    want_t = m.text_encoder(m.ctx.detach().clone().requires_grad_(True), CLASSES).detach()
    want_v = m.image_encoder(x, vis_prefix.detach().clone().requires_grad_(True)).detach()
    lib = native.lib()

    def refuse(*a):
        raise AssertionError("a deep tower call was made with D = 0")
    for name in ("grip_vit_forward_deep", "grip_vit_backward_deep", "grip_text_forward_deep", "grip_text_backward_deep"):
        monkeypatch.setattr(lib, name, refuse)
    t_out, v_out = m(x, CLASSES)
    CosineHeadFn.apply(v_out, t_out, 100.0).sum().backward()
    assert torch.equal(t_out.detach(), want_t) and torch.equal(v_out.detach(), want_v)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0 for p in params)
