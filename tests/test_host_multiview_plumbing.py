"""CPU: the plumbing of MULTIVIEW_PSEUDOLABELS that needs no GPU -- the config's MV_* settings reach pl.MultiView, MV_VIEWS outside 2 .. 64 and bad
parameters are refused, the pickle infix composes as cpl_ + mv_ + the transduction's, the installer takes only a MultiView, and the boxes of a pool are
a pure function of (seed, base name, view) with the epoch fixed at 0: view 0 the whole image, the same boxes in every pass."""
import types

import numpy as np
import pytest


def _pl():
    import grip_amd  # noqa: F401
    from grip_amd import pseudolabels as pl
    return pl


def test_config_settings_reach_the_multiview():
    pl = _pl()
    from grip_amd.methods.training_strategies import multi_view_from_config
    mv = multi_view_from_config(types.SimpleNamespace())
    assert (mv.views, mv.sampler.scale, mv.sampler.ratio, mv.sampler.flip, mv.sampler.seed) == (16, (0.5, 1.0), (0.75, 4.0 / 3.0), 0.5, 0)
    assert (mv.rho, mv.lam, mv.lam_y, mv.h2_floor, mv.outer, mv.inner, mv.keep_bytes) == (0.3, 4.0, 0.2, 2.0 ** -20, 5, 3, 0)
    conf = types.SimpleNamespace(MV_VIEWS=4, MV_SCALE=[0.3, 0.9], MV_RATIO=[1.0, 1.0], MV_FLIP=0.0, MV_SEED=7, MV_RHO=0.5, MV_LAMBDA=1.0, MV_LAMBDA_Y=0.5,
                                 MV_OUTER=2, MV_INNER=1, MV_CACHE_BYTES=1 << 20)
    mv = multi_view_from_config(conf, keep=True)
    assert (mv.views, mv.sampler.scale, mv.sampler.ratio, mv.sampler.flip, mv.sampler.seed) == (4, (0.3, 0.9), (1.0, 1.0), 0.0, 7)
    assert (mv.rho, mv.lam, mv.lam_y, mv.outer, mv.inner, mv.keep_bytes) == (0.5, 1.0, 0.5, 2, 1, 1 << 20)
    assert multi_view_from_config(conf, keep=False).keep_bytes == 0       # only a frozen tower keeps its view embeddings
    assert isinstance(mv, pl.MultiView) and mv.infix == "mv_"


@pytest.mark.parametrize("views", [1, 0, 65, -3, 2.0, True, None])
def test_views_outside_2_to_64_are_refused(views):
    pl = _pl()
    from grip_amd.methods.training_strategies import multi_view_from_config
    with pytest.raises(ValueError, match="views"):
        pl.MultiView(views=views)
    with pytest.raises(ValueError, match="views"):
        multi_view_from_config(types.SimpleNamespace(MV_VIEWS=views))
    assert pl.MultiView(views=2).views == 2 and pl.MultiView(views=64).views == 64


@pytest.mark.parametrize("bad", [dict(rho=0.0), dict(rho=1.5), dict(lam=-1.0), dict(lam_y=0.0), dict(h2_floor=0.0), dict(lam=float("inf")), dict(outer=-1),
                                 dict(inner=1.5), dict(scale=(0.0, 1.0)), dict(ratio=(2.0, 1.0)), dict(flip=1.5)])
def test_bad_parameters_are_refused(bad):
    with pytest.raises(ValueError):
        _pl().MultiView(**bad)


def test_infix_composes_and_the_installer_takes_only_a_multiview():
    pl = _pl()
    mv = pl.MultiView(views=4)
    assert pl.list_infix() == "" and pl.multiview() is None
    with pl.multi_view(None) as got:
        assert got is None and pl.multiview() is None and pl.list_infix() == ""
    with pl.multi_view(mv) as got:
        assert got is mv and pl.multiview() is mv and pl.list_infix() == "mv_"
        with pl.label_propagation(pl.BalancedAssignment(inner=pl.TransductiveGMM())):
            assert pl.list_infix() == "mv_ot_gmm_"
            with pl.candidate_sets(pl.CandidateSelection(), pl.CandidateStore()):
                assert pl.list_infix() == "cpl_mv_ot_gmm_"
        with pl.label_propagation(pl.LabelPropagation()):
            assert pl.list_infix() == "mv_lp_"
    assert pl.multiview() is None and pl.list_infix() == ""
    with pytest.raises(TypeError, match="MultiView"):
        with pl.multi_view(pl.LabelPropagation()):
            pass


def test_boxes_are_a_pure_function_of_seed_name_and_view():
    pl = _pl()
    from grip_amd.augment import ViewSampler
    names = ["pool/a/img_001.jpg", "pool/b/img_002.jpg", "img_003.jpg"]
    mv = pl.MultiView(views=5, seed=3)
    b = mv.boxes(names, 64, 64).reshape(3, 5, 5)
    assert b.dtype == np.int32 and (b[:, 0] == (0, 0, 64, 64, 0)).all()       # view 0: the whole image, un-flipped
    ref = ViewSampler(seed=3, scale=(0.5, 1.0))
    for i, n in enumerate(("img_001.jpg", "img_002.jpg", "img_003.jpg")):       # the base name, epoch 0, view p
        for p in range(1, 5):
            assert tuple(b[i, p]) == ref.box(n, 0, 64, 64, view=p)
    assert np.array_equal(mv.boxes(names, 64, 64), b.reshape(-1, 5))                                      # the same in every pass ...
    assert np.array_equal(pl.MultiView(views=5, seed=3).boxes(names[::-1], 64, 64).reshape(3, 5, 5)[::-1], b)      # ... and wherever the image stands
    assert np.array_equal(pl.MultiView(views=3, seed=3).boxes(names, 64, 64).reshape(3, 3, 5), b[:, :3])   # fewer views are a prefix of more
    assert not np.array_equal(pl.MultiView(views=5, seed=4).boxes(names, 64, 64).reshape(3, 5, 5)[:, 1:], b[:, 1:])
    assert len({tuple(x) for x in b[0, 1:]}) > 1                                                          # the views of an image differ
    ident = pl.MultiView(views=4, scale=(1.0, 1.0), ratio=(1.0, 1.0), flip=0.0).boxes(names, 64, 64)
    assert (ident == (0, 0, 64, 64, 0)).all()
