"""GPU: the view kernel (csrc/augment.hip) element-wise against the float64 helper of tests/augment_ref.py, its bit-equalities (identity, flip,
launch composition, dataset item = batch row), 64-bit offsets, and the AUGMENT switch of the training strategies."""
import numpy as np
import pytest
import torch

from augment_ref import view_plane

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _augment():
    import grip_amd  # noqa: F401
    from grip_amd import augment
    return augment


# 11 boxes of a 20 x 28 image per n_px: whole image (20 x 28 -> 6 has 13 x 19 taps), 1 x 1, 1 x w, h x 1, one flush against each border,
# 3 x 5 (enlarged), an interior box, and the n_px x n_px identity box
def _boxes(n):
    return [(0, 0, 20, 28), (7, 9, 1, 1), (5, 2, 1, 20), (3, 11, 15, 1), (0, 5, 8, 9), (12, 4, 8, 10), (6, 0, 9, 7), (4, 19, 10, 9), (8, 10, 3, 5),
            (1, 1, 18, 26), (2, 3, n, n)]


def _views23(n):
    """23 views: every box without and with flip, plus the 1 x 1 box once more; rows repeat and are out of order."""
    b = [bx + (f,) for bx in _boxes(n) for f in (0, 1)] + [(19, 27, 1, 1, 1)]
    rows = [(5 * i + 2) % 3 for i in range(len(b))]
    return np.array(b, dtype=np.int64), rows


_SRC = {}


def _source(family):
    if family not in _SRC:
        rs = np.random.RandomState(11)
        x = rs.standard_normal((3, 3, 20, 28)).astype(np.float32)
        if family == "constant":
            x[:] = np.float32(-1.7923)
        elif family == "outlier":
            x[1, 2, 9, 13] = 1e4
        _SRC[family] = x
    return _SRC[family]


def _check(src, boxes, rows, n, out, label):
    """|out - ref| <= k 2^-24 A + 1e-30 on EVERY element, k = T_h + T_v + 2: the kernel is two-pass -- T_h multiply-adds into the f32 intermediate,
    T_v into the output (each fused: one rounding), and two singly-rounded weights per product; always <= T_h T_v + 4."""
    worst = 0.0
    for v, (box, row) in enumerate(zip(boxes, rows)):
        for c in range(3):
            ref, A, tv, th = view_plane(src[row, c], box[:4], n, flip=bool(box[4]))
            k = th + tv + 2
            assert (k <= th * tv + 4).all()
            err = np.abs(out[v, c].astype(np.float64) - ref)
            bound = k * U * A + 1e-30
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (label, v, tuple(box), c, float((err / bound).max()))
    print(f"{label}: worst |out - ref| / bound = {worst:.3f}")
    return worst


@pytest.mark.parametrize("family", ["randn", "constant", "outlier"])
@pytest.mark.parametrize("n", [16, 10, 6])
def test_views_match_the_float64_reference(n, family):
    A = _augment()
    src = _source(family)
    boxes, rows = _views23(n)
    out = A.views(torch.from_numpy(src).cuda(), boxes, rows=rows, n_px=n)
    assert tuple(out.shape) == (23, 3, n, n)
    _check(src, boxes, rows, n, out.cpu().numpy(), f"20x28 -> {n} {family}")


def test_views_at_224_cover_bands_and_tails():
    A = _augment()
    src = np.random.RandomState(5).standard_normal((2, 3, 224, 224)).astype(np.float32)
    boxes = np.array([(0, 0, 224, 224, 0), (10, 20, 150, 120, 1), (0, 0, 224, 100, 0), (100, 50, 37, 59, 1), (3, 7, 221, 217, 0)], dtype=np.int64)
    rows = [1, 0, 1, 1, 0]
    x = torch.from_numpy(src).cuda()
    out = A.views(x, boxes, rows=rows)
    assert torch.equal(out[0], x[1])
    _check(src, boxes, rows, 224, out.cpu().numpy(), "224 -> 224")


def test_bit_equalities_identity_flip_and_launch_composition():
    A = _augment()
    n = 16
    x = torch.from_numpy(_source("randn")).cuda()
    boxes, rows = _views23(n)
    out = A.views(x, boxes, rows=rows, n_px=n)
    ident = 2 * (len(_boxes(n)) - 1)                                   # the un-flipped identity view
    assert tuple(boxes[ident]) == (2, 3, n, n, 0)
    assert torch.equal(out[ident], x[rows[ident], :, 2:2 + n, 3:3 + n])
    # a flipped view is the mirror image of the un-flipped view of the same box and image, bit for bit
    plain = boxes.copy()
    plain[:, 4] = 0
    unflipped = A.views(x, plain, rows=rows, n_px=n)
    for v in range(len(boxes)):
        want = torch.flip(unflipped[v], dims=[-1]) if boxes[v, 4] else unflipped[v]
        assert torch.equal(out[v], want), v
    # one launch of 23 = 23 launches of one, also into a caller's buffer
    for v in range(len(boxes)):
        single = A.views(x, boxes[v:v + 1], rows=rows[v:v + 1], n_px=n)
        assert torch.equal(single[0], out[v]), v
    buf = torch.full((23, 3, n, n), float("nan"), device="cuda")
    assert A.views(x, boxes, rows=rows, n_px=n, out=buf) is buf and torch.equal(buf, out)
    # the scalar-store path (n_px % 4 != 0) and the 16-byte path agree where both apply: same taps, same order
    odd = A.views(x, np.array([(0, 0, 20, 28, 0), (0, 0, 20, 28, 1)]), rows=[1, 1], n_px=33)
    assert torch.equal(odd[1], torch.flip(odd[0], dims=[-1])) and torch.isfinite(odd).all()


def test_dataset_items_equal_batch_rows():
    A = _augment()
    from grip_amd.data import TensorPoolDataset
    pool = torch.from_numpy(np.random.RandomState(3).standard_normal((6, 3, 32, 32)).astype(np.float32)).cuda()
    files = [f"root/cls/{i}.jpg" for i in range(6)]
    names = [f.split("/")[-1] for f in files]
    strong, weak = A.ViewSampler(seed=2), A.ViewSampler(seed=9, scale=(0.5, 1.0))
    ds = TensorPoolDataset(files, pool, labels=list(range(6)), label_id=True, augmentations=(strong, weak))
    for epoch in (0, 4):
        ds.set_epoch(epoch)
        b1, b2 = strong.batch(pool, names, epoch, view=0), weak.batch(pool, names, epoch, view=1)
        for i in (4, 0, 3):                                           # any order, one item at a time
            img, a1, a2, label, name = ds[i]
            assert torch.equal(img, pool[i]) and name == names[i] and label == i
            assert torch.equal(a1, b1[i]) and torch.equal(a2, b2[i])
    assert not torch.equal(strong.batch(pool, names, 0), strong.batch(pool, names, 4))
    half = TensorPoolDataset(files, pool, augmentations=(None, weak))[2]
    assert half[1] is half[0] and torch.equal(half[2], weak.batch(pool, names, 0, view=1)[2])


def test_offsets_beyond_2_31_elements():
    A = _augment()
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip("needs 12 GiB of free device memory")
    N = 14300                                                         # 14 299 * 3 * 224 * 224 = 2.15e9 > 2^31 elements before the last image
    pool = torch.empty(N, 3, 224, 224, device="cuda")
    img = torch.from_numpy(np.random.RandomState(9).standard_normal((1, 3, 224, 224)).astype(np.float32)).cuda()
    pool[N - 1] = img[0]
    boxes = np.array([(0, 0, 224, 224, 0), (17, 40, 120, 150, 1), (200, 190, 24, 34, 0)], dtype=np.int64)
    far = A.views(pool, boxes, rows=[N - 1] * 3)
    near = A.views(img, boxes, rows=[0] * 3)
    assert torch.equal(far, near) and torch.equal(far[0], img[0])
    del pool


# ---------------------------------------------------------------------------------------------- strategies
def _conf(**kw):
    import grip_amd  # noqa: F401
    from grip_amd.methods.main import DEFAULTS, Config
    c = dict(DEFAULTS)
    c.update(OPTIM_SEED=1, VIS_ENCODER="small", DATASET_NAME="Synthetic", SPLIT_SEED=500, DATASET_DIR="", EPOCHS=2, WARMUP_EPOCHS=1,
             N_PSEUDOSHOTS=4, STEP_QUANTILE=50, LR=0.05, PREFIX_SIZE=4, TEXT_PREFIX_SIZE=4, VISION_PREFIX_SIZE=4, BATCH_SIZE=8, IMAGE_LOOKAHEAD=3,
             LEARNING_PARADIGM="ssl", MODEL="x")
    c.update(kw)
    return Config(**c)


_POOL, _RUNS = {}, {}
IDENTITY = dict(AUGMENT="rrc_flip", AUG_SCALE=(1.0, 1.0), AUG_RATIO=(1.0, 1.0), AUG_FLIP=0.0)


def _run(cls_name, **kw):
    """Two epochs of `train`'s loop (epochs numbered from 0) on a 35-image pool: batches of 8 and a ragged 3.  Returns (per-epoch stats, prompt
    snapshot, strategy); one run per configuration and process."""
    key = (cls_name, tuple(sorted(kw.items())))
    if key not in _RUNS:
        import grip_amd  # noqa: F401
        from grip_amd import methods
        from grip_amd.data import TensorPoolDataset
        from grip_amd.methods.main import synthetic_pool
        if not _POOL:
            classes, files, images, names = synthetic_pool(5, 7, 64, 5)
            _POOL["p"] = (classes, files, images.cuda(), names)
        classes, files, images, names = _POOL["p"]
        l2i = {c: i for i, c in enumerate(classes)}
        m = getattr(methods, cls_name)(_conf(**kw), l2i, classes, classes[:3], classes[3:], "cuda")
        m.define_model(classes)
        loader = m._loader(TensorPoolDataset(files, images, labels=names, label_map=l2i), True)
        stats = [m._train_epoch(loader, epoch=e) for e in range(2)]
        _RUNS[key] = (stats, m.prompt_snapshot(), m)
    return _RUNS[key]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("cls_name", ["TextualPrompt", "VisualPrompt"])
def test_identity_views_reproduce_the_unaugmented_run(tmp_path, monkeypatch, cls_name):
    monkeypatch.chdir(tmp_path)
    s_off, p_off, _ = _run(cls_name, CACHE_FROZEN_FEATURES=False)
    s_id, p_id, m = _run(cls_name, **IDENTITY)
    assert s_id == s_off and _same(p_id, p_off)
    if cls_name == "TextualPrompt":
        s_c, p_c, mc = _run(cls_name, CACHE_FROZEN_FEATURES=True)
        assert _same(p_id, p_c)
        assert len(mc.__dict__.get("_frozen_cache", {})) == 35 and not m.__dict__.get("_frozen_cache")


def test_default_views_are_reproducible_seeded_and_uncached(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    A = _augment()
    seen = []
    real = A.ViewSampler.batch

    def spy(self, images, names, epoch, n_px=None, view=0):
        out = real(self, images, names, epoch, n_px=n_px, view=view)
        seen.append((epoch, list(names), images.clone(), out.clone()))
        return out
    monkeypatch.setattr(A.ViewSampler, "batch", spy)
    s0, p0, m = _run("TextualPrompt", AUGMENT="rrc_flip")
    monkeypatch.setattr(A.ViewSampler, "batch", real)
    assert not m.__dict__.get("_frozen_cache")                       # neither read nor filled
    assert [e for e, _, _, _ in seen] == [0] * 5 + [1] * 5
    by_epoch = [{n: o[i] for e, names, _, o in seen if e == ep for i, n in enumerate(names)} for ep in (0, 1)]
    src = {n: x[i] for _, names, x, _ in seen for i, n in enumerate(names)}
    assert set(by_epoch[0]) == set(by_epoch[1]) and len(by_epoch[0]) == 35
    assert all(not torch.equal(by_epoch[0][n], by_epoch[1][n]) for n in by_epoch[0])      # another epoch: another view of every image
    assert all(not torch.equal(by_epoch[0][n], src[n]) for n in src)                      # and the views are not the pool images
    _RUNS.pop(("TextualPrompt", (("AUGMENT", "rrc_flip"),)))
    s1, p1, _ = _run("TextualPrompt", AUGMENT="rrc_flip")                                  # a second, independent run
    assert s1 == s0 and _same(p1, p0)
    _, p_seed, _ = _run("TextualPrompt", AUGMENT="rrc_flip", AUG_SEED=1)
    assert not _same(p_seed, p0)
    _, p_off, _ = _run("TextualPrompt", CACHE_FROZEN_FEATURES=False)
    assert not _same(p_off, p0)


@pytest.mark.parametrize("cls_name", ["TextualPrompt", "VisualPrompt", "MultimodalPrompt"])
def test_augmented_graph_replay_equals_eager_epoch(tmp_path, monkeypatch, cls_name):
    """The criterion of test_train_epoch_graph_replay_equals_eager_epoch: same losses, accuracies and trained parameters, bit for bit."""
    monkeypatch.chdir(tmp_path)
    s_g, _, m_g = _run(cls_name, AUGMENT="rrc_flip")
    s_e, _, m_e = _run(cls_name, AUGMENT="rrc_flip", GRAPH_STEPS=False)
    assert s_g == s_e, (s_g, s_e)
    p_g, p_e = ([p.detach() for p in m.model.parameters() if p.requires_grad] for m in (m_g, m_e))
    assert len(p_g) == len(p_e) and all(torch.equal(a, b) for a, b in zip(p_g, p_e))
    assert not m_e.__dict__.get("_frozen_cache")


def test_unknown_augmentation_is_refused(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError):
        _run("VisualPrompt", AUGMENT="colour_jitter")
