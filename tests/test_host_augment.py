"""CPU: the float64 view helper of the GPU tests against Pillow itself, the counter-based ViewSampler (reproducible, order- and batch-free,
known answers that follow from torchvision's get_params), the host-side refusals of augment.views, and the dataset slot left at its default."""
import numpy as np
import pytest
import torch

from augment_ref import view_plane

U = 2.0 ** -24


def _random_boxes(rs, H, W, count):
    out = [(0, 0, H, W), (0, 0, 1, 1), (H - 1, W - 1, 1, 1), (0, 0, 1, W), (0, 0, H, 1), (0, 0, H // 2, W // 2), (H - H // 2, W - W // 2, H // 2, W // 2)]
    while len(out) < count:
        h, w = int(rs.randint(1, H + 1)), int(rs.randint(1, W + 1))
        out.append((int(rs.randint(0, H - h + 1)), int(rs.randint(0, W - w + 1)), h, w))
    return out


@pytest.mark.parametrize("H,W,n", [(20, 28, 16), (20, 28, 10), (20, 28, 6), (32, 32, 32), (9, 7, 16)])
def test_reference_helper_matches_pillow(H, W, n):
    """Pillow's 32-bit float resample accumulates each pass in double and rounds to f32 after each: |pillow - ref| <= 2 * 2^-24 * A on every element
    (worst ratio over these 300 boxes: 1.90)."""
    from PIL import Image
    rs = np.random.RandomState(1000 * H + 10 * W + n)
    plane = rs.standard_normal((H, W)).astype(np.float32)
    worst = 0.0
    for (top, left, h, w) in _random_boxes(rs, H, W, 60):
        got = np.asarray(Image.fromarray(plane, "F").crop((left, top, left + w, top + h)).resize((n, n), Image.BICUBIC), dtype=np.float64)
        ref, A, _, _ = view_plane(plane, (top, left, h, w), n)
        err = np.abs(got - ref)
        worst = max(worst, float((err / (U * A + 1e-300)).max()))
        assert (err <= 2 * U * A).all(), ((top, left, h, w), float((err / (U * A + 1e-300)).max()))
    print(f"worst |pillow - ref| / (2^-24 A) at {(H, W, n)}: {worst:.3f}")


def test_reference_helper_identity_constant_and_flip():
    rs = np.random.RandomState(7)
    plane = rs.standard_normal((20, 28)).astype(np.float32)
    ref, A, tv, th = view_plane(plane, (3, 5, 16, 16), 16)
    assert np.array_equal(ref, plane[3:19, 5:21].astype(np.float64))           # weights 0, 1, 0, 0
    const = np.full((20, 28), 0.7310585786300049)
    for box, n in (((0, 0, 20, 28), 16), ((2, 3, 3, 5), 10), ((0, 0, 20, 28), 6), ((4, 4, 1, 1), 16)):
        ref, _, _, _ = view_plane(const, box, n)
        assert np.abs(ref - const[0, 0]).max() <= 3e-16
    ref, A, tv, th = view_plane(plane, (0, 0, 20, 28), 6)
    fref, fA, ftv, fth = view_plane(plane, (0, 0, 20, 28), 6, flip=True)
    assert np.array_equal(fref, ref[:, ::-1]) and np.array_equal(fA, A[:, ::-1]) and np.array_equal(fth, th[:, ::-1]) and np.array_equal(ftv, tv)
    assert th.max() == 19 and tv.max() == 13                                     # a shrinking box has long windows


# ---------------------------------------------------------------------------------------------- sampler
def _sampler(**kw):
    import grip_amd  # noqa: F401
    from grip_amd.augment import ViewSampler
    return ViewSampler(**kw)


def test_sampler_is_a_function_of_seed_name_epoch_view():
    s = _sampler(seed=3)
    names = [f"img_{i:03d}.jpg" for i in range(64)]
    a = s.boxes(names, 2, 48, 64)
    assert a.shape == (64, 5) and np.issubdtype(a.dtype, np.integer)
    assert np.array_equal(a, s.boxes(names, 2, 48, 64)) and np.array_equal(a, _sampler(seed=3).boxes(names, 2, 48, 64))
    perm = np.random.RandomState(0).permutation(64)
    assert np.array_equal(s.boxes([names[i] for i in perm], 2, 48, 64), a[perm])          # order
    assert np.array_equal(s.boxes(names[10:17], 2, 48, 64), a[10:17])                     # batch membership
    assert np.array_equal(s.boxes([names[5]], 2, 48, 64)[0], a[5])
    for other in (s.boxes(names, 3, 48, 64), s.boxes(names, 2, 48, 64, view=1), _sampler(seed=4).boxes(names, 2, 48, 64)):
        assert (other != a).any(axis=1).sum() >= 60                                       # epoch, view, seed: other draws
    for H, W in ((48, 64), (224, 224), (7, 3), (1, 1)):
        b = s.boxes(names, 0, H, W)
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 2] >= 1).all() and (b[:, 3] >= 1).all()
        assert (b[:, 0] + b[:, 2] <= H).all() and (b[:, 1] + b[:, 3] <= W).all() and set(b[:, 4].tolist()) <= {0, 1}
    assert len({tuple(r[:4]) for r in a.tolist()}) > 32                                   # and they are spread out


def test_sampler_known_answers():
    names = [f"n{i}" for i in range(200)]
    wide = _sampler(scale=(0.9, 1.0), ratio=(3 / 4, 4 / 3))
    assert (wide.boxes(names, 0, 4, 64)[:, :4] == (0, 29, 4, 5)).all()          # every attempt is too tall: central box of ratio 4/3
    assert (wide.boxes(names, 1, 64, 4)[:, :4] == (29, 0, 5, 4)).all()          # ... of ratio 3/4
    whole = _sampler(scale=(1.0, 1.0), ratio=(1.0, 1.0))
    assert (whole.boxes(names, 5, 32, 32)[:, :4] == (0, 0, 32, 32)).all()
    assert (_sampler(flip=0.0).boxes(names, 0, 32, 32)[:, 4] == 0).all()
    assert (_sampler(flip=1.0).boxes(names, 0, 32, 32)[:, 4] == 1).all()
    flips = int(_sampler(flip=0.5).boxes([f"f{i}" for i in range(4096)], 0, 32, 32)[:, 4].sum())
    assert 1888 <= flips <= 2208, flips                                          # 2048 +- 5 sigma (sigma = 32)


def test_sampler_statistics_follow_the_published_algorithm():
    """Accepted boxes keep area / (H W) inside `scale` and w / h inside `ratio` up to the rounding of w and h."""
    b = _sampler(seed=1).boxes([f"s{i}" for i in range(2000)], 0, 224, 224).astype(np.float64)
    area, ratio = b[:, 2] * b[:, 3] / (224 * 224), b[:, 3] / b[:, 2]
    assert area.min() >= 0.08 * 0.97 and area.max() <= 1.0 and 0.3 < area.mean() < 0.7
    assert ratio.min() >= 0.75 * 0.97 and ratio.max() <= (4 / 3) * 1.03
    assert b[:, 0].min() == 0 and (b[:, 0] + b[:, 2]).max() == 224 and b[:, 1].min() == 0 and (b[:, 1] + b[:, 3]).max() == 224


def test_rng_uniform_at_extends_uniform():
    import grip_amd  # noqa: F401
    from grip_amd import rng
    assert np.array_equal(rng.uniform(3, 5, 9), rng.uniform_at(3, 5, (0, 0, 0), 9))
    a, b = rng.uniform_at(3, 5, (1, 0, 0), 9), rng.uniform_at(3, 5, (0, 1, 0), 9)
    assert not np.array_equal(a, b) and not np.array_equal(a, rng.uniform(3, 5, 9))
    assert (a > 0).all() and (a <= 1).all()


# ---------------------------------------------------------------------------------------------- views() refusals
class _FakeCuda:
    """A CPU tensor that reports itself as a GPU tensor: the refusals are host logic and must fire before anything is uploaded."""

    def __init__(self, t, is_cuda=True):
        self._t, self.is_cuda = t, is_cuda

    def __getattr__(self, k):
        return getattr(self._t, k)


def test_views_refuses_on_the_host_before_any_launch(monkeypatch):
    import grip_amd  # noqa: F401
    from grip_amd import augment

    def boom(*a, **k):
        raise AssertionError("the launcher was reached")
    monkeypatch.setattr(augment, "_launch", boom)
    monkeypatch.setattr(torch, "is_tensor", lambda x: isinstance(x, (torch.Tensor, _FakeCuda)))
    img = _FakeCuda(torch.zeros(2, 3, 8, 12))
    ok = [[0, 0, 8, 12, 0], [1, 2, 3, 4, 1]]
    bad_sources = [_FakeCuda(torch.zeros(2, 3, 8, 12), is_cuda=False), _FakeCuda(torch.zeros(2, 3, 8, 12, dtype=torch.float16)),
                   _FakeCuda(torch.zeros(2, 3, 8, 12, dtype=torch.float64)), _FakeCuda(torch.zeros(2, 3, 12, 8).transpose(2, 3)),
                   _FakeCuda(torch.zeros(2, 1, 8, 12)), _FakeCuda(torch.zeros(3, 8, 12))]
    for src in bad_sources:
        with pytest.raises(ValueError):
            augment.views(src, ok)
    bad_boxes = [[[0, 0, 9, 12, 0]], [[1, 0, 8, 12, 0]], [[0, 1, 8, 12, 0]], [[0, 0, 8, 13, 0]], [[-1, 0, 4, 4, 0]], [[0, -1, 4, 4, 0]],
                 [[0, 0, 0, 4, 0]], [[0, 0, 4, 0, 0]], [[0, 0, -2, 4, 0]], [[7, 11, 2, 1, 0]], [[0, 0, 4, 4]], [[0.0, 0.0, 4.0, 4.0, 0.0]]]
    for b in bad_boxes:
        with pytest.raises(ValueError):
            augment.views(img, b)
    for rows in ([2, 0], [0, -1], [0], [0, 1, 1]):
        with pytest.raises(ValueError):
            augment.views(img, ok, rows=rows)
    with pytest.raises(ValueError):
        augment.views(img, ok, n_px=0)
    with pytest.raises(ValueError):
        augment.views(img, ok, out=torch.zeros(2, 3, 8, 9))
    # V = 0: an empty result, still without a launch
    empty = augment.views(img, np.zeros((0, 5), dtype=np.int64), n_px=6)
    assert tuple(empty.shape) == (0, 3, 6, 6) and empty.dtype == torch.float32


# ---------------------------------------------------------------------------------------------- dataset slot
def test_dataset_default_items_are_unchanged():
    import grip_amd  # noqa: F401
    from grip_amd.data import TensorPoolDataset
    pool = torch.arange(4 * 3 * 6 * 6, dtype=torch.float32).reshape(4, 3, 6, 6)
    files = [f"d/{i}.jpg" for i in range(4)]
    for ds in (TensorPoolDataset(files, pool, labels=[0, 1, 0, 1], label_id=True), TensorPoolDataset(files, pool, labels=[0, 1, 0, 1], label_id=True, augmentations=None),
               TensorPoolDataset(files, pool, labels=[0, 1, 0, 1], label_id=True, augmentations=(None, None))):
        assert ds.epoch == 0 and ds.augmentations == (None, None)
        ds.set_epoch(3)
        assert ds.epoch == 3
        img, a1, a2, label, name = ds[2]
        assert a1 is img and a2 is img and torch.equal(img, pool[2]) and label == 0 and name == "2.jpg"
    img, a1, a2, name = TensorPoolDataset(files, pool)[1]
    assert a1 is img and a2 is img and name == "1.jpg"
    with pytest.raises(ValueError):
        TensorPoolDataset(files, pool, augmentations=(None,))
