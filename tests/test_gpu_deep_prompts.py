"""Deep visual prompts (VPT-Deep, grip_vit_forward_deep / grip_vit_backward_deep): before block l (1 <= l <= D) the prompt rows of the stream are
replaced by deep[l - 1], no LayerNorm and no positional embedding -- the reference's deep branch (models/clip_encoders.py:158-174) with its
projection and dropout as identity.  Forward and gradients against the CPU oracle composed here block by block, every tower precision, the
pool encode, the screen-and-refine pass, the graphed step, a visual strategy and the refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 101


def _inputs(name, shape, std=1.0):
    import grip_amd  # noqa: F401
    from grip_amd import rng
    return torch.from_numpy(rng.normal(SEED, rng.stream_id(name), shape, 0.0, std))


@pytest.fixture(scope="module")
def models():
    import grip_amd  # noqa: F401
    from grip_amd import clip
    cache = {}

    def get(name, exact=False):
        key = (name, bool(exact))
        if key not in cache:
            cache[key] = clip.load(name, device="cuda", exact=exact)[0]
        return cache[key]
    return get


def oracle_deep_forward(visual, x, prefix, deep):
    """oracle/wrappers.py:vision_forward with the transformer run block by block and the prompt rows replaced before blocks 1 .. D."""
    x = visual.conv1(x)
    x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
    cls = visual.class_embedding.to(x.dtype) + torch.zeros(x.shape[0], 1, x.shape[-1], dtype=x.dtype)
    x = torch.cat([cls, x], dim=1)
    x = x + visual.positional_embedding.to(x.dtype)
    B, P = x.shape[0], prefix.shape[-2]
    x = torch.cat([x[:, :1, :], prefix.reshape(1, P, -1).expand(B, -1, -1), x[:, 1:, :]], dim=1)
    x = visual.ln_pre(x).permute(1, 0, 2)                                          # LND
    for l, block in enumerate(visual.transformer.resblocks):
        if 1 <= l <= deep.shape[0]:
            x = torch.cat([x[:1], deep[l - 1][:, None, :].expand(-1, B, -1), x[1 + P:]], dim=0)
        x = block(x)
    x = visual.ln_post(x.permute(1, 0, 2)[:, 0, :])
    return x @ visual.proj


def _enc(tower, x, prefix, hilo=False, deep=None, chunk=None):
    out = torch.empty(x.shape[0], tower.embed_dim, device="cuda")
    tower.encode_chunks(x, out, 0, x.shape[0], chunk or x.shape[0], prefix, streams=1, hilo=hilo, deep=deep)
    return out


@pytest.mark.parametrize("name,B,P,D", [("tiny", 3, 3, 1), ("ViT-B/16", 4, 16, 11)])
def test_forward_deep_prompts_vs_oracle(models, name, B, P, D):
    from conftest import oracle_clip
    from test_gpu_exact import _close
    from test_gpu_towers import assert_embeddings_close
    from grip_amd import config
    from grip_amd.models import CustomImageEncoder
    d = config.get_dims(name)
    om, _ = oracle_clip().load(name)
    x = _inputs(f"dp.x.{name}", (B, 3, d.image_resolution, d.image_resolution))
    prefix = _inputs(f"dp.p.{name}", (P, d.vision_width), 0.05)
    deep = _inputs(f"dp.d.{name}", (D, P, d.vision_width), 0.05)
    with torch.no_grad():
        want = oracle_deep_forward(om.visual, x, prefix, deep)
        got = CustomImageEncoder(models(name).visual)(x.cuda(), prefix.cuda(), deep_prompts=deep.cuda())
        got_exact = CustomImageEncoder(models(name, exact=True).visual)(x.cuda(), prefix.cuda(), deep_prompts=deep.cuda())
        shallow = CustomImageEncoder(models(name).visual)(x.cuda(), prefix.cuda())
    assert_embeddings_close(got, want, f"{name} deep prompts")
    _close(got_exact, want, f"{name} deep prompts, exact tower", rel_tol=5e-5)
    assert not torch.equal(got, shallow), "deep prompts did not change the embedding"


def _towers(models):
    m = models("small")
    return {"f16": (m.visual.tower, False), "f16+hilo": (m.visual.tower, True), "split-f16": (m.split_twin().visual.tower, False),
            "f32": (m.exact_twin().visual.tower, False)}


@pytest.mark.parametrize("form", ["f16", "f16+hilo", "split-f16", "f32"])
def test_small_forms_vs_oracle_and_n_deep_zero_bits(models, form):
    """`small` (3 blocks, D = 1 and 2) on every stream form against the composed oracle; grip_vit_forward_deep with n_deep = 0 gives
    grip_vit_forward's bits; the deep encode is chunk-independent."""
    from conftest import oracle_clip
    from test_gpu_exact import _close
    from test_gpu_towers import assert_embeddings_close
    from grip_amd import native
    tower, hilo = _towers(models)[form]
    om, _ = oracle_clip().load("small")
    B, P = 5, 4
    x = _inputs("dp.small.x", (B, 3, 64, 64))
    prefix = _inputs("dp.small.p", (P, 256), 0.05)
    for D in (1, 2):
        deep = _inputs(f"dp.small.d{D}", (D, P, 256), 0.05)
        with torch.no_grad():
            want = oracle_deep_forward(om.visual, x, prefix, deep)
        got = _enc(tower, x.cuda(), prefix.cuda(), hilo, deep.cuda())
        if form in ("f16", "f16+hilo"):
            assert_embeddings_close(got, want, f"small {form} D={D}")
        else:
            _close(got, want, f"small {form} D={D}", rel_tol=5e-5)
        assert torch.equal(_enc(tower, x.cuda(), prefix.cuda(), hilo, deep.cuda(), chunk=2), got), f"{form}: deep encode depends on the chunking"
        assert not torch.equal(got, _enc(tower, x.cuda(), prefix.cuda(), hilo))
    # n_deep = 0 through the new entry point: the bits of grip_vit_forward
    xc, pc = x.cuda(), prefix.cuda().contiguous()
    ws = tower.workspace(B, P, False)
    p_, n_ = tower._aligned(ws)
    flags = native.FWD_STREAM_HILO if hilo else 0
    a = torch.empty(B, tower.embed_dim, device="cuda")
    b = torch.empty(B, tower.embed_dim, device="cuda")
    native.check(tower.lib.grip_vit_forward(tower.handle, xc.data_ptr(), 0, pc.data_ptr(), P, B, a.data_ptr(), p_, n_, flags, None, None))
    native.check(tower.lib.grip_vit_forward_deep(tower.handle, xc.data_ptr(), 0, pc.data_ptr(), P, None, 0, B, b.data_ptr(), p_, n_, flags, None, None))
    torch.cuda.synchronize()
    assert torch.equal(a, b), f"{form}: n_deep = 0 differs from grip_vit_forward"


@pytest.mark.parametrize("name,B,P,D", [("tiny", 3, 3, 1), ("ViT-B/16", 4, 16, 11)])
def test_deep_gradients_vs_oracle(models, name, B, P, D):
    """d loss / d prompt and d loss / d deep prompts against CPU-oracle autograd; the backward is bit-reproducible."""
    from conftest import oracle_clip
    from test_gpu_backward import assert_grad_close
    from grip_amd import config
    from grip_amd.engine import vit_prefix_forward
    d = config.get_dims(name)
    om, _ = oracle_clip().load(name)
    x = _inputs(f"dp.gx.{name}", (B, 3, d.image_resolution, d.image_resolution))
    prefix = _inputs(f"dp.gp.{name}", (P, d.vision_width), 0.05)
    deep = _inputs(f"dp.gd.{name}", (D, P, d.vision_width), 0.05)
    w = _inputs(f"dp.gw.{name}", (B, d.embed_dim))
    pc, dc = prefix.clone().requires_grad_(True), deep.clone().requires_grad_(True)
    (oracle_deep_forward(om.visual, x, pc, dc) * w).sum().backward()
    tower = models(name).visual.tower
    grads = []
    for _ in range(2):
        pg, dg = prefix.clone().cuda().requires_grad_(True), deep.clone().cuda().requires_grad_(True)
        (vit_prefix_forward(tower, x.cuda(), pg, deep=dg) * w.cuda()).sum().backward()
        assert pg.grad.shape == (P, d.vision_width) and dg.grad.shape == (D, P, d.vision_width) and dg.grad.dtype == torch.float32
        grads.append((pg.grad, dg.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1]), "deep backward is not bit-reproducible"
    assert_grad_close(grads[0][0], pc.grad, f"{name} shallow prompt gradient")
    for l in range(D):
        assert_grad_close(grads[0][1][l], dc.grad[l], f"{name} deep prompt gradient, block {l + 1}")
    # only the deep prompts require grad: still the train-mode path; f16 deep prompts get an f16 gradient
    dh = deep.clone().cuda().half().requires_grad_(True)
    (vit_prefix_forward(tower, x.cuda(), prefix.cuda(), deep=dh) * w.cuda()).sum().backward()
    assert dh.grad is not None and dh.grad.dtype == torch.float16 and dh.grad.shape == (D, P, d.vision_width)


def test_identical_lists_with_deep_prompts(models):
    """Screen-and-refine with deep prompts returns the f32 tower's lists over the same prompts (plain list equality with the exact mode)."""
    from conftest import structured_pool
    from grip_amd import clip, engine, pseudolabels as pl
    m = models("small")
    twin, split = m.exact_twin(), m.split_twin()
    n, P = 2000, 4
    pool = structured_pool(33, n, 64)
    prefix = _inputs("dp.refine.p", (P, 256), 0.05).cuda()
    deep = _inputs("dp.refine.d", (2, P, 256), 0.05).cuda()
    classes = ["annual crop land", "forest", "herbaceous vegetation", "highway", "industrial buildings", "pasture", "river"]
    tok = clip.tokenize([f"a photo of a {c}" for c in classes]).cuda()
    paths = [f"pool/{i:06d}.jpg" for i in range(n)]
    labels = list(range(len(classes)))
    scale = m.logit_scale.exp().item()
    with torch.no_grad():
        txt = twin.encode_text(tok)
        e32 = torch.empty(n, m.visual.tower.embed_dim, device="cuda")
        twin.visual.tower.encode_chunks(pool, e32, 0, n, 250, prefix, streams=1, deep=deep)
    _, p32, _, a32 = engine.cosine_head(e32, txt, scale)
    p32h, a32h = p32.cpu().numpy(), a32.cpu().numpy()
    for k in (16, pl.K_ALL):
        want = pl.leaderboard(p32h, a32h, paths, labels, k)
        got = pl.identical_lists(m.visual.tower, twin.visual.tower, pool, txt, scale, paths, labels, k, prefix=prefix,
                                 visual_mid=split.visual.tower, deep=deep)
        assert (list(got[0]), list(got[1])) == (list(want[0]), list(want[1])), f"k={k}: screen-and-refine lists differ from the f32 tower's"
    ref = pl.encode_pool(m.visual.tower, pool, chunk=440, prefix=prefix, deep=deep)
    assert torch.equal(pl.encode_pool(m.visual.tower, pool, chunk=333, prefix=prefix, deep=deep.cpu()), ref)
    assert not torch.equal(pl.encode_pool(m.visual.tower, pool, chunk=440, prefix=prefix), ref)


def test_graphed_deep_vpt_step_equals_eager(models):
    from grip_amd import clip, rng, steps
    from grip_amd.models import CustomImageEncoder, ImagePrefixModel
    m = models("small")
    classes = [f"class {i}" for i in range(6)]
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(8, 3, 64, 64, device="cuda", generator=g) for _ in range(4)]
    ys = [torch.randint(0, 6, (8,), device="cuda", generator=g, dtype=torch.int32) for _ in range(4)]
    w = torch.full((8,), 1 / 8, device="cuda")
    with torch.no_grad():
        txt = m.encode_text(clip.tokenize([f"a photo of a {c}" for c in classes]).cuda())
    N = lambda name, shape: torch.from_numpy(rng.normal(5, rng.stream_id(name), shape, 0.0, 0.02)).cuda()   # noqa: E731
    res = {}
    for graphed in (False, True):
        im = ImagePrefixModel(N("gd.p", (4, 256)), CustomImageEncoder(m.visual), device="cuda", deep_prefix=N("gd.d", (2, 4, 256)))
        opt = torch.optim.SGD([im.prefix, im.deep_prefix], lr=0.1, weight_decay=0.1)
        step = steps.GraphedVptStep(im, txt, 100.0, opt) if graphed else (lambda x, y, ww, _m=im, _o=opt: steps.vpt_step(_m, txt, 100.0, x, y, ww, _o))
        losses = [float(step(x, y, w)) for x, y in zip(xs, ys)]
        res[graphed] = (losses, im.prefix.detach().clone(), im.deep_prefix.detach().clone())
    e, gr = res[False], res[True]
    assert e[0] == gr[0] and torch.equal(e[1], gr[1]) and torch.equal(e[2], gr[2])
    assert not torch.equal(e[2], N("gd.d", (2, 4, 256))), "the deep prompts were not trained"


def test_visual_strategy_with_vpt_deep_trains(tmp_path, monkeypatch):
    from test_gpu_strategies import _conf
    from grip_amd.data import TensorPoolDataset
    from grip_amd.methods import VisualPrompt
    from grip_amd.methods.main import synthetic_pool
    monkeypatch.chdir(tmp_path)
    conf = _conf(MODEL="visual_prompt", LEARNING_PARADIGM="ssl", EPOCHS=2, LR=0.2, VPT_DEEP=True)
    classes, files, images, names = synthetic_pool(4, 8, 64, 3)
    l2i = {c: i for i, c in enumerate(classes)}
    data = TensorPoolDataset(files, images.cuda(), labels=names, label_map=l2i)
    m = VisualPrompt(conf, l2i, classes, classes, classes, "cuda")
    m.define_model(classes)
    assert m.model.deep_prefix is not None and tuple(m.model.deep_prefix.shape) == (2, 4, 256)
    before = m.model.deep_prefix.detach().clone()
    loader = m._loader(data, True)
    for _ in range(2):
        m._train_epoch(loader)
    assert not torch.equal(m.model.deep_prefix.detach(), before), "deep_prefix did not change"
    snap = m.prompt_snapshot()
    assert len(snap) == 2 and snap[0].shape == (4, 256) and snap[1].shape == (2, 4, 256)
    img, _ = m.trained_features(images.cuda(), classes)
    with torch.no_grad():
        want = m.model(images.cuda())
    assert torch.equal(img, want), "the pool pass does not use the trained deep prompts"


def test_deep_prompt_refusals(models):
    from grip_amd import native
    m = models("tiny")          # 2 blocks: D = 1 at most
    t = m.visual.tower
    x = torch.randn(3, 3, 32, 32, device="cuda")
    p = torch.randn(2, 128, device="cuda")
    for bad in (torch.zeros(2, 2, 128, device="cuda"), torch.zeros(1, 3, 128, device="cuda"), torch.zeros(1, 2, 64, device="cuda"), torch.zeros(2, 128, device="cuda")):
        with pytest.raises(native.GripError, match="deep visual prompts"):
            t.vit_forward(x, p, deep=bad)
    from grip_amd.models import CustomImageEncoder
    with pytest.raises(NotImplementedError):       # the reference-named keyword keeps raising (tests/test_gpu_errors.py)
        CustomImageEncoder(m.visual)(x, p, deep_embds=torch.zeros(1, 2, 128, device="cuda"))
    ws = t.workspace(3, 2, True)
    p_, n_ = t._aligned(ws)
    out = torch.empty(3, t.embed_dim, device="cuda")
    deep = torch.randn(1, 2, 128, device="cuda")
    pp = torch.randn(3, 2, 128, device="cuda")
    call = lambda prefix, P, dp, D, flags=0: native.check(t.lib.grip_vit_forward_deep(      # noqa: E731
        t.handle, x.data_ptr(), 0, prefix, P, dp, D, 3, out.data_ptr(), p_, n_, flags, None, None))
    for D, match in ((-1, "out of range"), (2, "out of range")):
        with pytest.raises(native.GripError, match=match):
            call(p.data_ptr(), 2, deep.data_ptr(), D)
    with pytest.raises(native.GripError, match="n_prefix must be positive"):
        call(None, 0, deep.data_ptr(), 1)
    with pytest.raises(native.GripError, match="null deep"):
        call(p.data_ptr(), 2, None, 1)
    with pytest.raises(native.GripError, match="PER_IMAGE"):
        call(pp.data_ptr(), 2, deep.data_ptr(), 1, native.FWD_PER_IMAGE_PREFIX)
    with pytest.raises(native.GripError, match="one prompt shared"):
        out2 = torch.empty(3, t.embed_dim, device="cuda")
        t.encode_chunks(x, out2, 0, 3, 3, pp, streams=1, deep=deep)
    tt = m.text_tower
    with pytest.raises(native.GripError, match="vision tower"):
        native.check(tt.lib.grip_vit_forward_deep(tt.handle, x.data_ptr(), 0, p.data_ptr(), 2, deep.data_ptr(), 1, 3, out.data_ptr(), p_, n_, 0, None, None))
    # a train-mode deep forward: grip_vit_backward_prefix refuses it and names the deep call, which then runs
    native.check(t.lib.grip_vit_forward_deep(t.handle, x.data_ptr(), 0, p.data_ptr(), 2, deep.data_ptr(), 1, 3, out.data_ptr(), p_, n_,
                                             native.FWD_TRAIN, None, None))
    ge = torch.randn(3, t.embed_dim, device="cuda")
    gp, gd = torch.empty(2, 128, device="cuda"), torch.empty(1, 2, 128, device="cuda")
    with pytest.raises(native.GripError, match="grip_vit_backward_deep"):
        native.check(t.lib.grip_vit_backward_prefix(t.handle, ge.data_ptr(), p.data_ptr(), gp.data_ptr(), p_, n_, 0, None))
    native.check(t.lib.grip_vit_backward_deep(t.handle, ge.data_ptr(), p.data_ptr(), gp.data_ptr(), gd.data_ptr(), p_, n_, 0, None))
    torch.cuda.synchronize()
    assert torch.isfinite(gp).all() and torch.isfinite(gd).all()
