"""Per-image visual prompts (GRIP_FWD_PER_IMAGE_PREFIX, ABI 9): image_prefix [B, P, d] through every ViT path, as the reference's
image_prefix.expand(B, -1, -1) accepts it (models/clip_encoders.py:148).  Forward and prompt gradient against the CPU oracle run live,
bit-identity with the shared-prompt path on every tower precision, the pool encode and the screen-and-refine pass, and the errors."""
import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 100


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


def _prompts(tag, B, P, d):
    """B different prompts (each image its own)."""
    return _inputs(f"ip.{tag}.{B}.{P}", (B, P, d), 0.05)


def _enc(tower, x, prefix, hilo=False):
    """Inference encode through encode_chunks (one chunk, current stream): the path every tower precision and the compensated stream share."""
    out = torch.empty(x.shape[0], tower.embed_dim, device="cuda")
    tower.encode_chunks(x, out, 0, x.shape[0], x.shape[0], prefix, streams=1, hilo=hilo)
    return out


@pytest.mark.parametrize("name,B,P", [("tiny", 3, 3), ("ViT-B/16", 4, 16)])
def test_forward_per_image_prompts_vs_oracle(models, name, B, P):
    """[B, P, d] with a different prompt per image against the CPU oracle's expand semantics: the f16 tower at the tower tests' tolerance,
    the exact tower at rel_tol 5e-5 (test_gpu_exact.py)."""
    from conftest import oracle_clip
    from oracle import wrappers as W
    from test_gpu_exact import _close
    from test_gpu_towers import assert_embeddings_close
    from grip_amd import config
    from grip_amd.models import CustomImageEncoder
    d = config.get_dims(name)
    om, _ = oracle_clip().load(name)
    x = _inputs(f"ip.x.{name}.{B}", (B, 3, d.image_resolution, d.image_resolution))
    prefix = _prompts(name, B, P, d.vision_width)
    with torch.no_grad():
        want = W.vision_forward(om.visual, x, prefix)
        got = CustomImageEncoder(models(name).visual)(x.cuda(), prefix.cuda())
        got_exact = CustomImageEncoder(models(name, exact=True).visual)(x.cuda(), prefix.cuda())
    assert_embeddings_close(got, want, f"{name} per-image prompts")
    _close(got_exact, want, f"{name} per-image prompts, exact tower", rel_tol=5e-5)
    # the prompts matter image by image: image 0 with image 1's prompt is another embedding
    with torch.no_grad():
        swapped = models(name).visual(x[:1].cuda(), prefix[1].cuda())
    assert not torch.equal(swapped, got[:1])


def _towers(models):
    m = models("small")
    return {"f16": (m.visual.tower, False), "f16+hilo": (m.visual.tower, True), "split-f16": (m.split_twin().visual.tower, False),
            "f32": (m.exact_twin().visual.tower, False)}


@pytest.mark.parametrize("form", ["f16", "f16+hilo", "split-f16", "f32"])
def test_per_image_bit_identity(models, form):
    """(a) one prompt repeated B times as [B, P, d] gives the shared call's bits; (b) row b of a per-image batch gives the bits of a batch-1
    forward of image b with prompt b."""
    tower, hilo = _towers(models)[form]
    B, P = 5, 4
    x = _inputs("ip.bits.x", (B, 3, 64, 64)).cuda()
    one = _inputs("ip.bits.p", (P, tower.width), 0.05).cuda()
    shared = _enc(tower, x, one, hilo)
    repeated = _enc(tower, x, one[None].expand(B, -1, -1).contiguous(), hilo)
    assert torch.equal(repeated, shared), f"{form}: repeated per-image prompt differs from the shared prompt"
    prefix = _prompts("bits", B, P, tower.width).cuda()
    per = _enc(tower, x, prefix, hilo)
    for b in range(B):
        alone = _enc(tower, x[b:b + 1], prefix[b], hilo)
        assert torch.equal(per[b:b + 1], alone), f"{form}: image {b} of the per-image batch differs from its batch-1 forward"
    assert not torch.equal(per, shared)


@pytest.mark.parametrize("name,B,P", [("tiny", 3, 3), ("ViT-B/16", 4, 16)])
def test_per_image_gradient_vs_oracle(models, name, B, P):
    """d loss / d image_prefix [B, P, d]: image b's own gradient, against CPU-oracle autograd image by image."""
    from conftest import oracle_clip
    from oracle import wrappers as W
    from test_gpu_backward import assert_grad_close
    from grip_amd import config
    from grip_amd.engine import VitPrefixFn
    d = config.get_dims(name)
    om, _ = oracle_clip().load(name)
    x = _inputs(f"ip.gx.{name}", (B, 3, d.image_resolution, d.image_resolution))
    prefix = _prompts(f"g.{name}", B, P, d.vision_width)
    w = _inputs(f"ip.gw.{name}", (B, d.embed_dim))
    pc = prefix.clone().requires_grad_(True)
    (W.vision_forward(om.visual, x, pc) * w).sum().backward()
    pg = prefix.clone().cuda().requires_grad_(True)
    (VitPrefixFn.apply(models(name).visual.tower, x.cuda(), pg) * w.cuda()).sum().backward()
    assert pg.grad.shape == (B, P, d.vision_width) and pg.grad.dtype == torch.float32
    for b in range(B):
        assert_grad_close(pg.grad[b], pc.grad[b], f"{name} prompt gradient of image {b}")


def test_repeated_prompt_gradient_sums_to_the_shared_gradient(models):
    """A [B, P, d] prompt made of one prompt repeated: its per-image gradients summed over b are the shared prompt's gradient (the same
    rows, added in another order); the per-image gradient is deterministic; a second backward of one forward is refused."""
    from grip_amd import native
    from grip_amd.engine import VitPrefixFn
    tower = models("ViT-B/16").visual.tower
    B, P = 16, 16
    x = _inputs("ip.sum.x", (B, 3, 224, 224)).cuda()
    one = _inputs("ip.sum.p", (P, 768), 0.02).cuda()
    w = _inputs("ip.sum.w", (B, 512)).cuda()
    ps = one.clone().requires_grad_(True)
    (VitPrefixFn.apply(tower, x, ps) * w).sum().backward()
    grads = []
    for _ in range(2):
        pp = one[None].expand(B, -1, -1).clone().requires_grad_(True)
        (VitPrefixFn.apply(tower, x, pp) * w).sum().backward()
        grads.append(pp.grad)
    assert torch.equal(grads[0], grads[1]), "per-image prompt gradient is not reproducible"
    # fp32 summation-order tolerance, element by element: 16 terms added in another order differ by at most ~16 ulp of the sum of |terms|
    summed = grads[0].double().sum(0)
    bound = 1e-5 * grads[0].double().abs().sum(0) + 1e-30
    err = ((summed - ps.grad.double()).abs() / bound).max().item()
    assert err <= 1.0, f"sum over images of the per-image gradient vs the shared gradient: {err:.3e} x the summation-order tolerance"
    # fp16 prompt: the gradient comes back in the prompt's dtype and shape
    ph = _prompts("half", 2, P, 768).cuda().half().requires_grad_(True)
    (VitPrefixFn.apply(tower, x[:2], ph) * w[:2]).sum().backward()
    assert ph.grad.shape == (2, P, 768) and ph.grad.dtype == torch.float16
    pp = _prompts("twice", 2, P, 768).cuda().requires_grad_(True)
    out = (VitPrefixFn.apply(tower, x[:2], pp) * w[:2]).sum()
    out.backward(retain_graph=True)
    with pytest.raises(native.GripError, match="already been back-propagated"):
        out.backward()


def test_pool_encode_per_image_prompts_is_chunk_independent(models):
    """encode_pool with [N, P, d]: the same bits at chunk sizes 440, 880 and an odd size, plain and compensated screen streams."""
    from grip_amd import pseudolabels as pl
    from conftest import structured_pool
    tower = models("small").visual.tower
    n, P = 2000, 4
    pool = structured_pool(31, n, 64)
    prefix = _prompts("pool", n, P, tower.width)         # on the host: each chunk's rows are moved with its images
    for screen in (False, "hilo"):
        ref = pl.encode_pool(tower, pool, chunk=440, prefix=prefix, screen=screen)
        for chunk in (880, 333):
            assert torch.equal(pl.encode_pool(tower, pool, chunk=chunk, prefix=prefix, screen=screen), ref), (screen, chunk)
        assert torch.equal(pl.encode_pool(tower, pool, chunk=880, prefix=prefix.cuda(), screen=screen), ref), screen
    with pytest.raises(ValueError, match="per-image"):
        pl.encode_pool(tower, pool, prefix=prefix[:-1])


def test_identical_lists_with_per_image_prompts(models):
    """Screen-and-refine with per-image prompts returns the lists of the f32 tower over the same prompts (test_gpu_identical.py's criterion:
    plain list equality with the exact mode), every tier encoding each row with its own prompt; rows pass through both refine tiers."""
    from conftest import structured_pool
    from grip_amd import clip, engine, pseudolabels as pl
    m = models("small")
    twin, split = m.exact_twin(), m.split_twin()
    n, P = 2000, 4
    pool = structured_pool(32, n, 64)
    prefix = _prompts("refine", n, P, m.visual.tower.width).cuda()
    classes = ["annual crop land", "forest", "herbaceous vegetation", "highway", "industrial buildings", "pasture", "river"]
    tok = clip.tokenize([f"a photo of a {c}" for c in classes]).cuda()
    paths = [f"pool/{i:06d}.jpg" for i in range(n)]
    labels = list(range(len(classes)))
    scale = m.logit_scale.exp().item()
    with torch.no_grad():
        txt = twin.encode_text(tok)
        e32 = torch.empty(n, m.visual.tower.embed_dim, device="cuda")
        twin.visual.tower.encode_chunks(pool, e32, 0, n, 250, prefix, streams=1)
    _, p32, _, a32 = engine.cosine_head(e32, txt, scale)
    p32h, a32h = p32.cpu().numpy(), a32.cpu().numpy()
    for k in (16, pl.K_ALL):
        want = pl.leaderboard(p32h, a32h, paths, labels, k)
        got = pl.identical_lists(m.visual.tower, twin.visual.tower, pool, txt, scale, paths, labels, k, prefix=prefix,
                                 visual_mid=split.visual.tower)
        st = pl.LAST_REFINE_STATS
        assert (list(got[0]), list(got[1])) == (list(want[0]), list(want[1])), f"k={k}: screen-and-refine lists differ from the f32 tower's"
        assert st["rows_mid_this_rank"] > 0 and st["rows_exact_this_rank"] > 0, st
    # the prompts are per image: the shared-prompt pass over the same pool is another set of embeddings
    assert not torch.equal(pl.encode_pool(m.visual.tower, pool, prefix=prefix[0]), pl.encode_pool(m.visual.tower, pool, prefix=prefix))


def test_per_image_prompt_errors(models):
    from grip_amd import native
    from grip_amd.engine import VitPrefixFn
    m = models("tiny")
    t = m.visual.tower
    x = torch.randn(3, 3, 32, 32, device="cuda")
    for bad in (torch.zeros(2, 2, 128, device="cuda"), torch.zeros(4, 2, 128, device="cuda")):
        with pytest.raises(native.GripError, match="one prompt per image"):
            m.visual(x, bad)
        with pytest.raises(native.GripError, match="one prompt per image"):
            VitPrefixFn.apply(t, x, bad.clone().requires_grad_(True))
    # [1, P, d] and [P, d] stay shared
    with torch.no_grad():
        p = torch.randn(2, 128, device="cuda")
        assert torch.equal(m.visual(x, p[None]), m.visual(x, p))
    # the flag is the vision tower's: a text tower refuses it
    tt = m.text_tower
    ids = torch.zeros(2, 77, dtype=torch.int32, device="cuda")
    ids[:, 0], ids[:, 1:5], ids[:, 5] = 49406, 343, 49407
    eot = ids.argmax(-1).to(torch.int32)
    ws = tt.workspace(2, 0, False)
    p_, n_ = tt._aligned(ws)
    out = torch.empty(2, tt.embed_dim, device="cuda")
    with pytest.raises(native.GripError, match="vision-tower flag"):
        native.check(tt.lib.grip_text_forward(tt.handle, ids.data_ptr(), eot.data_ptr(), None, 0, 1, 2, 0, out.data_ptr(), p_, n_,
                                              native.FWD_PER_IMAGE_PREFIX, None, None))
    # bit 16 is still unassigned; 32 is accepted, alone and with every other vision flag
    ws = t.workspace(3, 2, False)
    p_, n_ = t._aligned(ws)
    out = torch.empty(3, t.embed_dim, device="cuda")
    prefix = torch.randn(3, 2, 128, device="cuda")
    with pytest.raises(native.GripError, match="unknown flag bits"):
        native.check(t.lib.grip_vit_forward(t.handle, x.data_ptr(), 0, prefix.data_ptr(), 2, 3, out.data_ptr(), p_, n_, 16, None, None))
    native.check(t.lib.grip_vit_forward(t.handle, x.data_ptr(), 0, prefix.data_ptr(), 2, 3, out.data_ptr(), p_, n_,
                                        native.FWD_PER_IMAGE_PREFIX | native.FWD_NO_POS_EMB | native.FWD_STREAM_HILO, None, None))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert native.lib().grip_abi_version() == native.ABI_VERSION == 9
