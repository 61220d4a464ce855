"""CPU: the plumbing of TPT that needs no GPU -- the config's TPT_* settings reach tpt.TestTimeTuner with the paper's defaults, bad values are refused when
the settings are read, keep = max(1, floor(rho views)), steps.ViewEntropyTargets carries (views, keep) and goes where a SoftTargets goes, and the boxes
of an item are a pure function of (seed, base name, view) with the epoch fixed at 0: the same whatever batch the item stands in."""
import types

import numpy as np
import pytest


def _settings(**kw):
    import grip_amd  # noqa: F401
    from grip_amd.methods.training_strategies import tpt_settings_from_config
    return tpt_settings_from_config(types.SimpleNamespace(**kw))


def test_config_settings_reach_the_tuner_with_the_papers_defaults():
    from grip_amd import tpt
    kw = _settings()
    assert kw == dict(views=64, rho=0.1, lr=5e-3, steps=1, scale=(0.08, 1.0), ratio=(0.75, 4.0 / 3.0), flip=0.5, seed=0)
    t = tpt.TestTimeTuner(None, None, **kw)
    assert (t.views, t.keep, t.lr, t.steps, t.episodes) == (64, 6, 5e-3, 1, 0)
    assert (t.sampler.scale, t.sampler.ratio, t.sampler.flip, t.sampler.seed) == ((0.08, 1.0), (0.75, 4.0 / 3.0), 0.5, 0)
    assert t.targets.key() == ("view_entropy", 64, 6) and t.targets.matrix is None
    kw = _settings(TPT_VIEWS=8, TPT_RHO=0.5, TPT_LR=1e-2, TPT_STEPS=2, TPT_SCALE=[0.3, 0.9], TPT_RATIO=[1.0, 1.0], TPT_FLIP=0.0, TPT_SEED=7)
    assert kw == dict(views=8, rho=0.5, lr=1e-2, steps=2, scale=(0.3, 0.9), ratio=(1.0, 1.0), flip=0.0, seed=7)


@pytest.mark.parametrize("bad", [dict(TPT_VIEWS=0), dict(TPT_VIEWS=65), dict(TPT_VIEWS=8.0), dict(TPT_VIEWS=True), dict(TPT_RHO=0.0), dict(TPT_RHO=1.5),
                                 dict(TPT_LR=-1.0), dict(TPT_LR=float("inf")), dict(TPT_STEPS=-1), dict(TPT_STEPS=1.5), dict(TPT_SCALE=(0.0, 1.0)),
                                 dict(TPT_RATIO=(2.0, 1.0)), dict(TPT_FLIP=1.5)])
def test_bad_settings_are_refused_when_they_are_read(bad):
    with pytest.raises(ValueError):
        _settings(**bad)


@pytest.mark.parametrize("views,rho,keep", [(64, 0.1, 6), (16, 0.1, 1), (8, 0.5, 4), (1, 0.1, 1), (10, 0.1, 1), (20, 0.1, 2), (64, 1.0, 64), (5, 0.99, 4)])
def test_keep_from_rho(views, rho, keep):
    from grip_amd import tpt
    assert tpt.keep_from_rho(views, rho) == keep == tpt.TestTimeTuner(None, None, views=views, rho=rho).keep


def test_a_graphed_episode_is_not_built():
    from grip_amd import tpt
    with pytest.raises(ValueError, match="graphed"):
        tpt.TestTimeTuner(None, None, graphed=True)


def test_view_entropy_targets():
    import grip_amd  # noqa: F401
    from grip_amd import steps
    t = steps.ViewEntropyTargets(8, 2)
    assert t.matrix is None and t.key() == ("view_entropy", 8, 2) and (t.views, t.keep) == (8, 2)
    for bad in ((0, 1), (65, 1), (8, 0), (8, 9), (8.0, 1), (8, True)):
        with pytest.raises(ValueError, match="ViewEntropyTargets"):
            steps.ViewEntropyTargets(*bad)


def test_encode_views_stays_on_its_rank_under_two_ranks(monkeypatch):
    """`predict` hands every rank different items, so the views of a batch must be encoded where they are: with a world of two ranks encode_views may reach
    neither the collective encode_pool nor dist.shard_range / allgather_rows, and every row it returns is the tower's row of THIS rank's view."""
    import torch

    from grip_amd import dist as gdist, pseudolabels as pl, tpt

    def collective(*a, **kw):
        raise AssertionError("encode_views entered a collective: the other rank holds other items")
    monkeypatch.setattr(gdist, "world", lambda: (1, 2))
    for mod, name in ((gdist, "shard_range"), (gdist, "allgather_rows"), (pl, "encode_pool")):
        monkeypatch.setattr(mod, name, collective)
    monkeypatch.setattr(pl, "make_views", lambda sampler, views, images, names: images.repeat_interleave(views, dim=0) + torch.arange(views).repeat(
        images.shape[0])[:, None, None, None])

    class Tower:
        embed_dim, device = 3, torch.device("cpu")

        def encode_chunks(self, images, out, lo, hi, chunk, prefix=None):
            assert (lo, hi) == (0, images.shape[0]) and prefix is None, "every view of the batch, on this rank"
            out[:hi - lo] = images[lo:hi].reshape(hi - lo, -1)[:, :3]

    t = tpt.TestTimeTuner(None, types.SimpleNamespace(visual=types.SimpleNamespace(tower=Tower())), views=4)
    images = torch.arange(5, dtype=torch.float32)[:, None, None, None].expand(5, 3, 2, 2) * 10
    feats = t.encode_views(images, [f"{i}.jpg" for i in range(5)])
    assert feats.shape == (5, 4, 3)
    assert torch.equal(feats[:, :, 0], torch.arange(5.0)[:, None] * 10 + torch.arange(4.0)[None, :])      # item i, view p: this rank's own rows, all of them


def test_an_items_boxes_do_not_depend_on_its_batch():
    from grip_amd import pseudolabels as pl, tpt
    from grip_amd.augment import ViewSampler
    names = [f"test/c{i % 3}/img_{i:03d}.jpg" for i in range(12)]
    t = tpt.TestTimeTuner(None, None, views=8, seed=3)
    whole = t.boxes(names, 64, 64).reshape(12, 8, 5)
    assert whole.dtype == np.int32 and (whole[:, 0] == (0, 0, 64, 64, 0)).all()      # view 0: the image itself
    ref = ViewSampler(seed=3, scale=(0.08, 1.0))
    for i, n in enumerate(names):
        for p in range(1, 8):
            assert tuple(whole[i, p]) == ref.box(n.split("/")[-1], 0, 64, 64, view=p)      # the base name, epoch 0, view p
    for bs in (4, 8, 5):      # batches of 4, 8 (a ragged tail) and 5: every item gets the boxes it has in the whole list
        got = np.concatenate([t.boxes(names[lo:lo + bs], 64, 64).reshape(-1, 8, 5) for lo in range(0, 12, bs)])
        assert np.array_equal(got, whole)
    assert np.array_equal(t.boxes(names[::-1], 64, 64).reshape(12, 8, 5)[::-1], whole)      # ... and wherever it stands (another rank's order)
    # the views of pseudolabels.MultiView under the same sampler settings: the shared helper
    mv = pl.MultiView(views=8, seed=3, scale=(0.08, 1.0))
    assert np.array_equal(mv.boxes(names, 64, 64), whole.reshape(-1, 5))
