"""CPU: the plumbing of the test-time streaming cache that needs no GPU -- the config's TDA_* settings reach tda.StreamCache with the recalled defaults,
bad values are refused when the settings are read, and the host-side checks of engine.check_stream_cache_settings need no device."""
import types

import pytest

DEFAULTS = dict(pos_cap=3, neg_cap=2, pos_alpha=2.0, pos_beta=5.0, neg_alpha=0.117, neg_beta=1.0, neg_entropy=(0.2, 0.5), neg_mask=(0.03, 1.0))


def _cache(**kw):
    import grip_amd  # noqa: F401
    from grip_amd.methods.training_strategies import stream_cache_from_config
    return stream_cache_from_config(types.SimpleNamespace(**kw))


def test_config_settings_reach_the_cache_with_the_recalled_defaults():
    from grip_amd import engine, tda
    c = _cache()
    assert isinstance(c, tda.StreamCache) and c.settings == DEFAULTS == engine.STREAM_CACHE_DEFAULTS and c.streams == 0 and c.plan is None
    assert tda.StreamCache().settings == DEFAULTS
    c = _cache(TDA_POS_CAP=16, TDA_NEG_CAP=0, TDA_POS_ALPHA=1, TDA_POS_BETA=5.5, TDA_NEG_ALPHA=0.0, TDA_NEG_BETA=2, TDA_NEG_ENTROPY=[0.1, 0.9],
               TDA_NEG_MASK=[0.0, 0.5])
    assert c.settings == dict(pos_cap=16, neg_cap=0, pos_alpha=1.0, pos_beta=5.5, neg_alpha=0.0, neg_beta=2.0, neg_entropy=(0.1, 0.9), neg_mask=(0.0, 0.5))
    assert all(isinstance(c.settings[k], float) for k in ("pos_alpha", "neg_beta"))


@pytest.mark.parametrize("bad", [dict(TDA_POS_CAP=0), dict(TDA_POS_CAP=17), dict(TDA_POS_CAP=3.0), dict(TDA_POS_CAP=True), dict(TDA_NEG_CAP=-1),
                                 dict(TDA_NEG_CAP=17), dict(TDA_POS_ALPHA=-1.0), dict(TDA_POS_BETA=float("inf")), dict(TDA_NEG_ALPHA=float("nan")),
                                 dict(TDA_NEG_BETA=-0.5), dict(TDA_NEG_ENTROPY=(0.5, 0.2)), dict(TDA_NEG_ENTROPY=0.3), dict(TDA_NEG_ENTROPY=(0.1, 0.2, 0.3)),
                                 dict(TDA_NEG_MASK=(0.0, float("inf"))), dict(TDA_NEG_MASK=("a", "b"))])
def test_bad_settings_are_refused_when_they_are_read(bad):
    with pytest.raises(ValueError):
        _cache(**bad)


def test_the_engine_checks_need_no_device():
    import grip_amd  # noqa: F401
    from grip_amd import engine, native
    assert engine.check_stream_cache_settings("t") == (3, 2, 2.0, 5.0, 0.117, 1.0, (0.2, 0.5), (0.03, 1.0))
    with pytest.raises(native.GripError, match="pos_cap"):
        engine.check_stream_cache_settings("t", pos_cap=0)
    for fn in (engine.stream_cache_plan, lambda x: engine.stream_cache_head(x, x, {}), lambda x: engine.stream_cache(x, x)):
        with pytest.raises(native.GripError, match="base_logits must be a contiguous float32"):
            fn([[0.0]])


def test_the_switch_is_off_by_default_and_validation_keeps_the_plain_path():
    """The strategy reads TDA / TDA_VALIDATION where it reads TPT / TPT_VALIDATION (the source is the record: building a strategy needs the towers)."""
    import inspect

    import grip_amd  # noqa: F401
    from grip_amd.methods import training_strategies as ts
    src = inspect.getsource(ts)
    assert 'getattr(config, "TDA", False)' in src and 'getattr(self.config, "TDA_VALIDATION", False)' in src
