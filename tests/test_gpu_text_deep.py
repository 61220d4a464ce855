"""Deep text prompts (deep CoOp, grip_text_forward_deep / grip_text_backward_deep): before block l (1 <= l <= D) positions 1 .. P of every class's
residual stream are replaced by deep[l - 1] (one set for every class, or one per class), no LayerNorm, no positional and no token embedding -- the
text-tower mirror of the deep visual prompts.  Forward and gradients against the CPU oracle composed block by block
(tests/test_host_text_deep.py:oracle_text_deep_forward, pinned there to oracle.wrappers.text_forward and the golden vectors), every tower
precision, both row layouts, truncated and full sequences, the graphed CoOp steps, a textual strategy and the refusals.

Tolerances are the project's helpers: test_gpu_towers.assert_embeddings_close (f16 towers), test_gpu_exact._close(rel_tol=5e-5) (f32 and split-f16
twins, the value the deep visual prompt tests use), test_gpu_backward.assert_grad_close (gradients), and for shared-vs-plain layout the figures of
tests/test_gpu_backward.py::test_shared_prefix_layout_equals_plain."""
import pytest
import torch

from test_host_text_deep import oracle_text_deep_forward

pytestmark = pytest.mark.gpu
SEED = 103


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
        key = (name, int(exact))      # 0 f16 towers, 1 f32 (the exact twin's arithmetic), 2 split-f16 with a text tower of its own
        if key not in cache:
            cache[key] = clip.load(name, device="cuda", exact=exact)[0]
        return cache[key]
    return get


def _tokens(d, P, lens, seed=0):
    """CustomTextEncoder's layout: SOT, P context placeholders, the class's own tokens (lens[c] of them), EOT (the largest id), zero padding."""
    gen = torch.Generator().manual_seed(seed * 131 + P)
    sot, eot = d.vocab_size - 2, d.vocab_size - 1
    tok = torch.zeros(len(lens), d.context_length, dtype=torch.int32)
    for c, n in enumerate(lens):
        row = [sot] + [7] * P + [int(v) for v in torch.randint(10, d.vocab_size - 2, (n,), generator=gen)] + [eot]
        tok[c, :len(row)] = torch.tensor(row, dtype=torch.int32)
    return tok


def _same_layout_tolerance(a, b, what):
    """Embeddings of one function in two row layouts / sequence lengths: tests/test_gpu_backward.py:269-273."""
    cos = torch.nn.functional.cosine_similarity(a, b, dim=1)
    assert (1 - cos).max().item() <= 2e-6, f"{what}: 1-cos {(1 - cos).max().item():.2e}"
    torch.testing.assert_close(a, b, rtol=2e-3, atol=2e-3 * b.abs().max().item())


# `tiny` and `small` have two text blocks, so D = 1 is their only depth (D = 2 is refused: n_deep <= layers - 1); the partial depth D = 2 runs on
# ViT-B/16 next to the full D = 11
CASES = [("tiny", 3, (2, 1, 4, 3, 1), (1,)), ("small", 4, (2, 1, 4, 3, 1), (1,)), ("ViT-B/16", 16, (1, 2, 3, 4, 5, 6, 2, 7, 3), (2, 11))]


@pytest.mark.parametrize("name,P,lens,depths", CASES)
def test_forward_deep_text_prompts_vs_oracle(models, name, P, lens, depths):
    from conftest import oracle_clip
    from test_gpu_exact import _close
    from test_gpu_towers import assert_embeddings_close
    from grip_amd import config, native
    from grip_amd.engine import text_prefix_forward
    d = config.get_dims(name)
    om, _ = oracle_clip().load(name)
    m, twin = models(name), models(name, exact=True)
    tok = _tokens(d, P, lens)
    prefix = _inputs(f"td.p.{name}", (1, P, d.transformer_width), 0.02)
    with torch.no_grad():
        shallow = text_prefix_forward(m.text_tower, tok.clone().cuda(), prefix.cuda())
    for D in depths:
        deep = _inputs(f"td.d.{name}.{D}", (D, P, d.transformer_width), 0.02)
        with torch.no_grad():
            want = oracle_text_deep_forward(om, tok, prefix, deep)
            got = text_prefix_forward(m.text_tower, tok.clone().cuda(), prefix.cuda(), deep=deep.cuda())
            assert m.text_tower.last_text_flags & native.FWD_SHARED_PREFIX, "the shared-prefix layout was not taken"
            got_exact = text_prefix_forward(twin.text_tower, tok.clone().cuda(), prefix.cuda(), deep=deep.cuda())
        assert_embeddings_close(got, want, f"{name} deep text prompts D={D}")
        _close(got_exact, want, f"{name} deep text prompts D={D}, exact tower", rel_tol=5e-5)
        assert not torch.equal(got, shallow), "deep prompts did not change the embedding"
        if name == "small":
            with torch.no_grad():
                got_split = text_prefix_forward(models("small", exact=2).text_tower, tok.clone().cuda(), prefix.cuda(), deep=deep.cuda())
            _close(got_split, want, f"small deep text prompts D={D}, split-f16 tower", rel_tol=5e-5)


def test_encoder_keyword_reaches_the_tower(models):
    """CustomTextEncoder.forward(..., deep_prompts=) on its own token ids, [D, P, d] and [D, 1, P, d] alike."""
    from conftest import oracle_clip
    from test_gpu_towers import assert_embeddings_close
    from grip_amd.models import CustomTextEncoder
    m = models("small")
    om, _ = oracle_clip().load("small")
    enc = CustomTextEncoder(m, "cuda", torch.float32)
    classes = ["forest", "annual crop land", "river"]
    prefix = _inputs("td.enc.p", (1, 4, 256), 0.02)
    deep = _inputs("td.enc.d", (1, 4, 256), 0.02)
    with torch.no_grad():
        got = enc(prefix.cuda(), classes, deep_prompts=deep.cuda())
        got4 = enc(prefix.cuda(), classes, deep_prompts=deep.cuda()[:, None])
        want = oracle_text_deep_forward(om, enc._token_ids(4, classes).cpu(), prefix, deep)
    assert_embeddings_close(got, want, "CustomTextEncoder deep_prompts")
    assert torch.equal(got, got4)


@pytest.mark.parametrize("name,P,lens,D", [("small", 3, (2, 1, 4, 3, 1), 1), ("ViT-B/16", 16, "ragged", 11)])
def test_shared_and_plain_layouts_and_sequence_lengths_agree(models, name, P, lens, D):
    """The same deep prompts in the shared-prefix layout and in the plain one: embeddings (train and inference forward) and both gradients agree to
    the shared-vs-plain tolerance of the shallow context; so do all 77 positions (seq_len = 0) against the EOT-truncated sequence."""
    from test_gpu_backward import assert_grad_close
    from grip_amd import config, native
    from grip_amd.engine import TextPrefixFn, text_prefix_forward
    m = models(name)
    d = config.get_dims(name)
    tower = m.text_tower
    if lens == "ragged":
        gen = torch.Generator().manual_seed(5)
        lens = [1 + int(v) for v in torch.randint(0, 9, (37,), generator=gen)]
    C = len(lens)
    tok = _tokens(d, P, lens, seed=1)
    prefix0 = _inputs(f"td.lay.p.{name}", (1, P, d.transformer_width), 0.02).cuda()
    deep0 = _inputs(f"td.lay.d.{name}", (D, P, d.transformer_width), 0.02).cuda()
    wout = _inputs(f"td.lay.w.{name}", (C, d.embed_dim)).cuda()
    res = {}
    for share, truncate in ((True, True), (False, True), (True, False), (False, False)):
        tower.share_text_prefix, tower.truncate_text_at_eot = share, truncate
        try:
            t = tok.clone().cuda()
            pf, df = prefix0.clone().requires_grad_(True), deep0.clone().requires_grad_(True)
            out = TextPrefixFn.apply(tower, t, pf, True, df)
            assert bool(tower.last_text_flags & native.FWD_SHARED_PREFIX) == share
            (out * wout).sum().backward()
            with torch.no_grad():
                inf = text_prefix_forward(tower, t, pf, deep=df)
            res[share, truncate] = (out.detach().clone(), inf.clone(), pf.grad.clone(), df.grad.clone())
        finally:
            tower.share_text_prefix, tower.truncate_text_at_eot = True, True
    ref = res[False, True]
    for key in ((True, True), (True, False), (False, False)):
        what = f"{'shared' if key[0] else 'plain'} layout, {'truncated' if key[1] else 'all positions'} vs plain truncated"
        _same_layout_tolerance(res[key][0], ref[0], f"train-mode embeddings, {what}")
        _same_layout_tolerance(res[key][1], ref[1], f"inference embeddings, {what}")
        assert_grad_close(res[key][2], ref[2].cpu().numpy(), f"context gradient, {what}", cos_tol=1e-4, rel_tol=1e-2)
        assert_grad_close(res[key][3], ref[3].cpu().numpy(), f"deep prompt gradient, {what}", cos_tol=1e-4, rel_tol=1e-2)


def test_no_positional_embedding_vs_oracle(models):
    from conftest import oracle_clip
    from test_gpu_exact import _close
    from test_gpu_towers import assert_embeddings_close
    from grip_amd import config
    from grip_amd.engine import text_prefix_forward
    d = config.get_dims("small")
    om, _ = oracle_clip().load("small")
    tok = _tokens(d, 4, (2, 1, 4, 3), seed=2)
    prefix = _inputs("td.np.p", (1, 4, 256), 0.02)
    deep = _inputs("td.np.d", (1, 4, 256), 0.02)
    with torch.no_grad():
        want = oracle_text_deep_forward(om, tok, prefix, deep, enable_pos_emb=False)
        assert not torch.allclose(want, oracle_text_deep_forward(om, tok, prefix, deep))
        got = text_prefix_forward(models("small").text_tower, tok.clone().cuda(), prefix.cuda(), pos_emb=False, deep=deep.cuda())
        got_exact = text_prefix_forward(models("small", exact=True).text_tower, tok.clone().cuda(), prefix.cuda(), pos_emb=False, deep=deep.cuda())
    assert_embeddings_close(got, want, "deep text prompts, enable_pos_emb=False")
    _close(got_exact, want, "deep text prompts, enable_pos_emb=False, exact tower", rel_tol=5e-5)


@pytest.mark.parametrize("name,P,lens,D", [("small", 3, (2, 1, 4, 3, 1), 1), ("ViT-B/16", 16, (1, 2, 3, 4, 5, 6, 2, 7), 11)])
def test_class_specific_deep_context_vs_oracle(models, name, P, lens, D):
    """One context and one set of deep prompts per class ([C, P, d], [D, C, P, d]): forward and both gradients against the oracle; given the same
    rows for every class it is the shared context's function, and its per-class gradients sum to the shared one."""
    from conftest import oracle_clip
    from test_gpu_backward import assert_grad_close
    from test_gpu_exact import _close
    from test_gpu_towers import assert_embeddings_close
    from grip_amd import config, native
    from grip_amd.engine import text_prefix_forward
    d = config.get_dims(name)
    om, _ = oracle_clip().load(name)
    tower = models(name).text_tower
    C, dt = len(lens), d.transformer_width
    tok = _tokens(d, P, lens, seed=3)
    prefix = _inputs(f"td.cs.p.{name}", (C, P, dt), 0.02)
    deep = _inputs(f"td.cs.d.{name}", (D, C, P, dt), 0.02)
    w = _inputs(f"td.cs.w.{name}", (C, d.embed_dim))
    pc, dc = prefix.clone().requires_grad_(True), deep.clone().requires_grad_(True)
    want = oracle_text_deep_forward(om, tok, pc, dc)
    (want * w).sum().backward()
    pg, dg = prefix.clone().cuda().requires_grad_(True), deep.clone().cuda().requires_grad_(True)
    got = text_prefix_forward(tower, tok.clone().cuda(), pg, deep=dg)
    assert not tower.last_text_flags & native.FWD_SHARED_PREFIX
    (got * w.cuda()).sum().backward()
    assert_embeddings_close(got, want.detach(), f"{name} class-specific deep context")
    with torch.no_grad():
        got_exact = text_prefix_forward(models(name, exact=True).text_tower, tok.clone().cuda(), prefix.cuda(), deep=deep.cuda())
    _close(got_exact, want.detach(), f"{name} class-specific deep context, exact tower", rel_tol=5e-5)
    assert pg.grad.shape == (C, P, dt) and dg.grad.shape == (D, C, P, dt)
    assert_grad_close(pg.grad, pc.grad, f"{name} class-specific context gradient")
    for l in range(D):
        assert_grad_close(dg.grad[l], dc.grad[l], f"{name} class-specific deep gradient, block {l + 1}")
    # every class given the same rows: the shared context's result, and gradients that sum to the shared context's
    ps, ds = prefix[:1].clone().cuda().requires_grad_(True), deep[:, 0].clone().cuda().requires_grad_(True)
    shared = text_prefix_forward(tower, tok.clone().cuda(), ps, deep=ds)
    (shared * w.cuda()).sum().backward()
    pe = prefix[:1].expand(C, -1, -1).contiguous().cuda().requires_grad_(True)
    de = deep[:, :1].expand(-1, C, -1, -1).contiguous().cuda().requires_grad_(True)
    same = text_prefix_forward(tower, tok.clone().cuda(), pe, deep=de)
    (same * w.cuda()).sum().backward()
    assert_embeddings_close(same, shared.detach().cpu(), f"{name} per-class copies of one context vs the shared context")
    assert_grad_close(pe.grad.sum(0, keepdim=True), ps.grad.cpu(), f"{name} summed per-class context gradient vs shared")
    assert_grad_close(de.grad.sum(1), ds.grad.cpu(), f"{name} summed per-class deep gradient vs shared")


@pytest.mark.parametrize("name,P,lens,D", [("tiny", 3, (2, 1, 4, 3, 1), 1), ("ViT-B/16", 16, (1, 2, 3, 4, 5, 6, 2, 7, 3), 11)])
def test_deep_text_gradients_vs_oracle(models, name, P, lens, D):
    """d loss / d context and d loss / d deep prompts against CPU-oracle autograd; the backward is bit-reproducible."""
    from conftest import oracle_clip
    from test_gpu_backward import assert_grad_close
    from grip_amd import config
    from grip_amd.engine import text_prefix_forward
    d = config.get_dims(name)
    om, _ = oracle_clip().load(name)
    C, dt = len(lens), d.transformer_width
    tok = _tokens(d, P, lens, seed=4)
    prefix = _inputs(f"td.g.p.{name}", (1, P, dt), 0.02)
    deep = _inputs(f"td.g.d.{name}", (D, P, dt), 0.02)
    w = _inputs(f"td.g.w.{name}", (C, d.embed_dim))
    pc, dc = prefix.clone().requires_grad_(True), deep.clone().requires_grad_(True)
    (oracle_text_deep_forward(om, tok, pc, dc) * w).sum().backward()
    tower = models(name).text_tower
    grads = []
    for _ in range(2):
        pg, dg = prefix.clone().cuda().requires_grad_(True), deep.clone().cuda().requires_grad_(True)
        (text_prefix_forward(tower, tok.clone().cuda(), pg, deep=dg) * w.cuda()).sum().backward()
        assert pg.grad.shape == (1, P, dt) and dg.grad.shape == (D, P, dt) and dg.grad.dtype == torch.float32
        grads.append((pg.grad, dg.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1]), "deep text backward is not bit-reproducible"
    assert_grad_close(grads[0][0], pc.grad, f"{name} context gradient")
    for l in range(D):
        assert_grad_close(grads[0][1][l], dc.grad[l], f"{name} deep text prompt gradient, block {l + 1}")
    # the shallow context's gradient flows through block 0 only: not the gradient without deep prompts
    p0 = prefix.clone().cuda().requires_grad_(True)
    (text_prefix_forward(tower, tok.clone().cuda(), p0) * w.cuda()).sum().backward()
    assert not torch.allclose(p0.grad, grads[0][0])
    # only the deep prompts require grad: still the train-mode path; f16 deep prompts [D, 1, P, d] get an f16 gradient of that shape
    dh = deep.clone().cuda().half()[:, None].requires_grad_(True)
    (text_prefix_forward(tower, tok.clone().cuda(), prefix.cuda(), deep=dh) * w.cuda()).sum().backward()
    assert dh.grad is not None and dh.grad.dtype == torch.float16 and dh.grad.shape == (D, 1, P, dt)
    assert_grad_close(dh.grad, dc.grad, f"{name} deep gradient with only the deep prompts trainable")


@pytest.mark.parametrize("form", ["f16", "split-f16", "f32"])
def test_n_deep_zero_is_grip_text_forward_bit_for_bit(models, form):
    """grip_text_forward_deep(deep = NULL, n_deep = 0) against grip_text_forward, plain and shared layout; the backward pair alike (f16)."""
    from grip_amd import config, native
    m = models("small")
    tower = {"f16": m.text_tower, "split-f16": models("small", exact=2).text_tower, "f32": m.exact_twin().text_tower}[form]
    d = config.get_dims("small")
    C, P = 5, 4
    tok = _tokens(d, P, (2, 1, 4, 3, 1), seed=6).cuda()
    eot = tok.argmax(-1).to(torch.int32)
    S = int(eot.max()) + 1
    prefix = _inputs("td.z.p", (1, P, 256), 0.02).cuda().contiguous()
    lib, h = tower.lib, tower.handle
    for train in ((False, True) if form == "f16" else (False,)):
        for shared in (0, native.FWD_SHARED_PREFIX):
            flags = shared | (native.FWD_TRAIN if train else 0)
            ws = tower.workspace(C, P, train, S)
            p_, n_ = tower._aligned(ws)
            a, b = torch.empty(C, tower.embed_dim, device="cuda"), torch.empty(C, tower.embed_dim, device="cuda")
            ge = _inputs("td.z.g", (C, tower.embed_dim)).cuda()
            ga, gb = torch.empty(1, P, 256, device="cuda"), torch.empty(1, P, 256, device="cuda")
            native.check(lib.grip_text_forward(h, tok.data_ptr(), eot.data_ptr(), prefix.data_ptr(), P, 1, C, S, a.data_ptr(), p_, n_, flags, None, None))
            if train:
                native.check(lib.grip_text_backward_prefix(h, ge.data_ptr(), ga.data_ptr(), p_, n_, 0, None))
            native.check(lib.grip_text_forward_deep(h, tok.data_ptr(), eot.data_ptr(), prefix.data_ptr(), P, 1, None, 0, C, S, b.data_ptr(), p_, n_, flags, None, None))
            if train:
                native.check(lib.grip_text_backward_deep(h, ge.data_ptr(), gb.data_ptr(), None, p_, n_, 0, None))
            torch.cuda.synchronize()
            assert torch.equal(a, b), f"{form} train={train} shared={shared}: n_deep = 0 differs from grip_text_forward"
            if train:
                assert torch.equal(ga, gb), f"{form} shared={shared}: grip_text_backward_deep after n_deep = 0 differs from grip_text_backward_prefix"
            tower.release(ws)


@pytest.mark.parametrize("kind", ["images", "features"])
def test_graphed_deep_coop_steps_equal_eager(models, kind):
    """GraphedCoopStep / GraphedCoopFeatureStep with a deep_prefix follow the eager coop_step exactly (tests/test_gpu_strategies.py:156-178), and
    both parameters move."""
    from grip_amd import rng, steps
    from grip_amd.models import CustomTextEncoder, TextPrefixModel
    m = models("small")
    classes = [f"class {i}" for i in range(7)]
    g = torch.Generator(device="cuda").manual_seed(0)
    if kind == "images":
        xs = [torch.randn(8, 3, 64, 64, device="cuda", generator=g) for _ in range(5)]
    else:
        xs = [torch.randn(8, m.dims.embed_dim, device="cuda", generator=g) for _ in range(5)]
    ys = [torch.randint(0, 7, (8,), device="cuda", generator=g, dtype=torch.int32) for _ in range(5)]
    w = torch.full((8,), 1 / 8, device="cuda")
    N = lambda name, shape: torch.from_numpy(rng.normal(3, rng.stream_id(name), shape, 0.0, 0.02)).cuda()   # noqa: E731
    out = []
    for graphed in (False, True):
        tm = TextPrefixModel(N("tdg.p", (1, 4, 256)), CustomTextEncoder(m, "cuda", torch.float32), classes, device="cuda", deep_prefix=N("tdg.d", (1, 4, 256)))
        opt = torch.optim.SGD([tm.prefix, tm.deep_prefix], lr=0.1, weight_decay=0.1)
        if kind == "images":
            eager = lambda x, y, ww, _tm=tm, _opt=opt: steps.coop_step(_tm, m, x, y, ww, _opt)                            # noqa: E731
            step = steps.GraphedCoopStep(tm, m, opt) if graphed else eager
        else:
            eager = lambda x, y, ww, _tm=tm, _opt=opt: steps.coop_step(_tm, m, None, y, ww, _opt, image_features=x)      # noqa: E731
            step = steps.GraphedCoopFeatureStep(tm, m, opt) if graphed else eager
        losses = [float(step(x, y, w)) for x, y in zip(xs, ys)]
        losses.append(float(step(xs[0][:5], ys[0][:5], w[:5] * 8 / 5)))       # another batch size: the graphed step falls back to eager
        out.append((losses, tm.prefix.detach().clone(), tm.deep_prefix.detach().clone()))
    (l_e, p_e, d_e), (l_g, p_g, d_g) = out
    assert l_e == l_g, (l_e, l_g)
    assert torch.equal(p_e, p_g) and torch.equal(d_e, d_g)
    assert not torch.equal(p_g, N("tdg.p", (1, 4, 256))) and not torch.equal(d_g, N("tdg.d", (1, 4, 256))), "a parameter was not trained"


def test_textual_strategy_with_coop_deep(tmp_path, monkeypatch):
    """A textual strategy with COOP_DEEP: trains both tensors, snapshots two arrays, labels the pool in both pseudolabel modes -- in the identical
    mode with the lists of the exact twin fed the same prompts -- and without the switch is today's strategy bit for bit."""
    from test_gpu_strategies import _conf
    import grip_amd  # noqa: F401
    from grip_amd import methods, pseudolabels as pl
    from grip_amd.data import TensorPoolDataset
    from grip_amd.engine import text_prefix_forward
    from grip_amd.methods.main import synthetic_pool
    from grip_amd.models import TextPrefixModel
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("GRIP_PSEUDOLABEL_MODE", raising=False)
    classes, files, images, names = synthetic_pool(5, 40, 64, 17)
    l2i = {c: i for i, c in enumerate(classes)}

    def trained(**kw):
        conf = _conf(MODEL="x", LEARNING_PARADIGM="ssl", LR=0.1, **kw)
        s = methods.TextualFPL(conf, l2i, "", classes, classes, classes, "cuda")
        s.define_model(classes)
        loader = s._loader(TensorPoolDataset(files, images.cuda(), labels=names, label_map=l2i), True)
        stats = [s._train_epoch(loader) for _ in range(2)]
        return s, stats

    s, _ = trained(COOP_DEEP=True)
    layers = s.clip_model.dims.transformer_layers
    assert tuple(s.model.deep_prefix.shape) == (layers - 1, 4, 256)
    assert not torch.equal(s.model.deep_prefix.detach().cpu(), s.initial_deep_prefix), "deep_prefix did not change"
    assert not torch.equal(s.model.prefix.detach().cpu(), s.initial_prefix), "prefix did not change"
    snap = s.prompt_snapshot()
    assert len(snap) == 2 and snap[0].shape == (1, 4, 256) and snap[1].shape == (layers - 1, 4, 256)
    # identical mode: the all-f32 lists with the same prompts
    twin = s.clip_model.exact_twin()
    ids = s.text_encoder._token_ids(4, classes)
    with torch.no_grad():
        txt = text_prefix_forward(twin.text_tower, ids, s.model.prefix.detach(), deep=s.model.deep_prefix.detach())
        assert torch.equal(s.trained_text_features(classes, twin)[0], txt)
        assert not torch.equal(text_prefix_forward(twin.text_tower, ids, s.model.prefix.detach()), txt)
        emb = pl.encode_pool(twin.visual.tower, images.cuda(), chunk=32)
    want = pl.pseudolabel_from_features(emb, txt, s.scale(), list(files), [l2i[c] for c in classes], 7, argmax_on="logits")
    pl.LAST_REFINE_STATS = None
    out = s.assign_pseudo_labels(7, TensorPoolDataset(files, images.cuda(), labels=None, label_map=l2i))
    assert (out.filepaths, out.labels) == want and pl.LAST_REFINE_STATS is not None and len(want[0]) > 7
    # f16 mode: the f16 towers' own lists, deep prompts included (trained_features == the model's forward)
    monkeypatch.setenv("GRIP_PSEUDOLABEL_MODE", "f16")
    img16, txt16 = s.trained_features(images.cuda(), classes)
    with torch.no_grad():
        assert torch.equal(txt16, s.model(classes))
    want16 = pl.pseudolabel_from_features(img16, txt16, s.scale(), list(files), [l2i[c] for c in classes], 7, argmax_on="logits")
    out16 = s.assign_pseudo_labels(7, TensorPoolDataset(files, images.cuda(), labels=None, label_map=l2i))
    assert (out16.filepaths, out16.labels) == want16 and len(want16[0]) > 7
    pred, _ = s.predict(TensorPoolDataset(files, images.cuda(), labels=names, label_map=l2i), classes)
    assert len(pred) == len(files)
    monkeypatch.delenv("GRIP_PSEUDOLABEL_MODE")
    # COOP_DEEP absent: the trajectory of a model built without deep_prefix (the parent's construction), bit for bit
    a, stats_a = trained()
    assert a.model.deep_prefix is None and len(a.prompt_snapshot()) == 1
    b, _ = trained()
    b.model = TextPrefixModel(b.initial_prefix.clone().cuda(), b.text_encoder, classes, device="cuda")
    b.optimizer = torch.optim.SGD([b.model.prefix], lr=float(b.config.LR), weight_decay=float(b.config.DECAY), momentum=float(getattr(b.config, "MOMENTUM", 0.0)))
    from grip_amd.methods.training_strategies import make_scheduler
    b.scheduler = make_scheduler(b.optimizer, b.config)
    b._model_gen += 1
    loader = b._loader(TensorPoolDataset(files, images.cuda(), labels=names, label_map=l2i), True)
    stats_b = [b._train_epoch(loader) for _ in range(2)]
    assert stats_a == stats_b and torch.equal(a.model.prefix.detach(), b.model.prefix.detach())
    assert torch.equal(a.initial_prefix, s.initial_prefix)


def test_deep_text_prompt_refusals(models):
    """Invalid arguments only: nothing is launched by the refused calls."""
    from grip_amd import native
    from grip_amd.engine import text_prefix_forward
    import os
    import re
    from conftest import REPO
    with open(os.path.join(REPO, "include", "grip_amd.h")) as f:
        header = f.read()
    ERR_ARG, ERR_STATE = (int(re.search(rf"\b{n}\s*=?\s*(-?\d+)", header).group(1)) for n in ("GRIP_ERR_ARG", "GRIP_ERR_STATE"))
    m = models("tiny")          # 2 blocks: D = 1 at most
    d = m.dims
    t = m.text_tower
    C, P = 3, 2
    tok = _tokens(d, P, (1, 2, 1), seed=7).cuda()
    eot = tok.argmax(-1).to(torch.int32)
    S = int(eot.max()) + 1
    p = torch.randn(1, P, 128, device="cuda")
    for bad in (torch.zeros(2, P, 128, device="cuda"), torch.zeros(1, 3, 128, device="cuda"), torch.zeros(1, P, 64, device="cuda"), torch.zeros(P, 128, device="cuda"),
                torch.zeros(1, C, P, 128, device="cuda")):
        with pytest.raises(native.GripError, match="deep text prompts"):
            t.text_forward(tok, p, deep=bad)
    with pytest.raises(native.GripError, match=r"expected \[D, 3, 2, 128\]"):
        text_prefix_forward(t, tok, p.expand(C, -1, -1).contiguous(), deep=torch.zeros(1, P, 128, device="cuda"))
    ws = t.workspace(C, P, True, S)
    p_, n_ = t._aligned(ws)
    out = torch.empty(C, t.embed_dim, device="cuda")
    deep = torch.randn(1, 1, P, 128, device="cuda")
    call = lambda prefix, n_prefix, dp, D, flags=0: native.check(t.lib.grip_text_forward_deep(      # noqa: E731
        t.handle, tok.data_ptr(), eot.data_ptr(), prefix, n_prefix, 1, dp, D, C, S, out.data_ptr(), p_, n_, flags, None, None))
    for D in (-1, 2):
        with pytest.raises(native.GripError, match=rf"\(status {ERR_ARG}\).*n_deep = -?\d out of range"):
            call(p.data_ptr(), P, deep.data_ptr(), D)
    with pytest.raises(native.GripError, match="n_prefix must be positive"):
        call(None, 0, deep.data_ptr(), 1)
    with pytest.raises(native.GripError, match="null deep"):
        call(p.data_ptr(), P, None, 1)
    v = m.visual.tower
    with pytest.raises(native.GripError, match="not a text tower.*grip_vit_forward_deep"):
        native.check(v.lib.grip_text_forward_deep(v.handle, tok.data_ptr(), eot.data_ptr(), p.data_ptr(), P, 1, deep.data_ptr(), 1, C, S, out.data_ptr(), p_, n_, 0, None, None))
    x = torch.randn(3, 3, 32, 32, device="cuda")
    with pytest.raises(native.GripError, match="vision tower"):      # the vision call on a text tower keeps its message
        native.check(t.lib.grip_vit_forward_deep(t.handle, x.data_ptr(), 0, p.data_ptr(), P, deep.data_ptr(), 1, 3, out.data_ptr(), p_, n_, 0, None, None))
    # a train-mode deep forward: grip_text_backward_prefix refuses it (GRIP_ERR_STATE) and names the deep call, which then runs
    call(p.data_ptr(), P, deep.data_ptr(), 1, native.FWD_TRAIN)
    ge = torch.randn(C, t.embed_dim, device="cuda")
    gp, gd = torch.empty(1, P, 128, device="cuda"), torch.empty(1, 1, P, 128, device="cuda")
    rc = t.lib.grip_text_backward_prefix(t.handle, ge.data_ptr(), gp.data_ptr(), p_, n_, 0, None)
    assert rc == ERR_STATE
    with pytest.raises(native.GripError, match="grip_text_backward_deep"):
        native.check(rc)
    with pytest.raises(native.GripError, match="null grad_deep"):
        native.check(t.lib.grip_text_backward_deep(t.handle, ge.data_ptr(), gp.data_ptr(), None, p_, n_, 0, None))
    native.check(t.lib.grip_text_backward_deep(t.handle, ge.data_ptr(), gp.data_ptr(), gd.data_ptr(), p_, n_, 0, None))
    torch.cuda.synchronize()
    assert torch.isfinite(gp).all() and torch.isfinite(gd).all() and gd.abs().max() > 0
    t.release(ws)
