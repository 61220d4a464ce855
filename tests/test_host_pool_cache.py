"""pseudolabels.PoolFeatureCache: the bookkeeping that keeps a frozen pool's embeddings across pseudolabel passes, on CPU tensors with stand-in
towers (no GPU): what is a hit, what is a miss, what bypasses the cache, what the budget does.  The GPU side (bits, lists, encode counts, ranks) is
tests/test_gpu_pool_cache.py."""
import gc

import numpy as np
import pytest
import torch


class FakeTower:
    """What encode_pool needs of a tower: a device, a width and encode_chunks -- here a cheap deterministic function of the image, the prompt and the
    stream form, that counts the rows it encodes."""

    def __init__(self, embed_dim=8, salt=0.0):
        self.device, self.embed_dim, self.salt = "cpu", embed_dim, salt
        self.rows = 0

    def encode_chunks(self, images, out, lo, hi, chunk, prefix=None, streams=2, hilo=False, deep=None):
        for s in range(lo, hi, chunk):
            e = min(s + chunk, hi)
            x = images[s:e] if torch.is_tensor(images) else images(s, e)
            v = x.flatten(1).sum(1, keepdim=True) + self.salt + (0.5 if hilo else 0.0)
            if prefix is not None:
                v = v + 100.0
            if deep is not None:
                v = v + 1000.0
            out[s - lo: e - lo] = v + torch.arange(self.embed_dim, dtype=torch.float32)
            self.rows += e - s
        return out


class LazyPool:
    """A lazy pool like utils.clip_pseudolabels._pool_images builds for files: a callable (lo, hi) -> images that counts its calls."""

    def __init__(self, x):
        self.x, self.n, self.calls = x, x.shape[0], 0

    def __call__(self, lo, hi):
        self.calls += 1
        return self.x[lo:hi]


def _pl():
    import grip_amd  # noqa: F401
    from grip_amd import pseudolabels as pl
    return pl


def _paths(n, tag="a"):
    return [f"pool/{tag}{i:04d}.jpg" for i in range(n)]


def test_screen_hit_and_miss_rules():
    pl = _pl()
    c = pl.PoolFeatureCache()
    t1, t2 = FakeTower(), FakeTower()
    paths, emb = _paths(20), torch.randn(20, 8)
    assert c.screen(paths, t1) is None
    assert c.store_screen(paths, t1, "hilo", emb)
    got, form = c.screen(list(paths), t1)                      # an equal list of the same strings: a hit, and the tensor itself
    assert got is emb and form == "hilo"
    assert c.screen(tuple(paths), t1)[0] is emb
    other = _paths(20)
    other[7] = "pool/elsewhere.jpg"                            # same length, one other path: compared element-wise, a miss
    assert c.screen(other, t1) is None
    assert c.screen(paths[::-1], t1) is None                   # the same paths in another order are another pool
    assert c.screen(paths[:19], t1) is None
    assert c.screen(paths, t2) is None                         # another tower: its own entry
    st = c.stats()
    assert st["hits"] == 2 and st["misses"] == 5 and st["entries"] == 1 and st["bytes"] == 20 * 8 * 4
    with pytest.raises(ValueError):
        c.store_screen(paths, t1, "bf16", emb)


def test_a_freed_towers_entry_is_unreachable():
    pl = _pl()
    c = pl.PoolFeatureCache()
    paths = _paths(10)
    t = FakeTower()
    c.store_screen(paths, t, "plain", torch.zeros(10, 8))
    c.store_rows(paths, t, np.array([1, 3]), torch.ones(2, 8), 10)
    assert c.stats()["entries"] == 1 and c.stats()["bytes"] == 2 * 10 * 8 * 4
    del t
    gc.collect()
    st = c.stats()
    assert st["entries"] == 0 and st["bytes"] == 0
    again = FakeTower()                                         # whatever address it lands on: nothing of the old tower is served
    assert c.screen(paths, again) is None
    assert c.missing_rows(paths, again, np.array([1, 3])).tolist() == [1, 3]
    assert c.stats()["pools"] == 0


def test_stream_form_rules():
    """A plain request is never served a compensated ("hilo") entry; the plain stream is one function whether a screen chose it ("f16") or a caller
    asked for plain embeddings; identical_lists (no form constraint) takes whichever is there."""
    pl = _pl()
    assert pl.screen_forms(False) == ("f16", "plain") == pl.screen_forms("f16") and pl.screen_forms("hilo") == ("hilo",)
    c = pl.PoolFeatureCache()
    t, paths = FakeTower(), _paths(12)
    hilo = torch.full((12, 8), 2.0)
    c.store_screen(paths, t, "hilo", hilo)
    assert c.screen(paths, t, pl.screen_forms(False)) is None
    assert c.screen(paths, t, pl.screen_forms("f16")) is None
    assert c.screen(paths, t, pl.screen_forms("hilo"))[0] is hilo
    assert c.screen(paths, t) == (hilo, "hilo")                 # any form: what identical_lists asks
    plain = torch.full((12, 8), 3.0)
    c.store_screen(paths, t, "f16", plain)
    assert c.screen(paths, t, pl.screen_forms(False)) == (plain, "f16")
    assert c.screen(paths, t, pl.screen_forms("hilo"))[0] is hilo
    c2 = pl.PoolFeatureCache()
    c2.store_screen(paths, t, "plain", plain)
    assert c2.screen(paths, t, pl.screen_forms("f16")) == (plain, "plain") and c2.screen(paths, t, pl.screen_forms("hilo")) is None
    assert c2.screen(paths, t)[1] == "plain"


def test_encode_pool_reads_and_writes_the_cache_and_prompted_calls_bypass_it():
    pl = _pl()
    n = 37
    x = torch.randn(n, 3, 4, 4)
    paths = _paths(n)
    t = FakeTower()
    want = pl.encode_pool(t, x, chunk=16)
    want_hilo = pl.encode_pool(t, x, chunk=16, screen="hilo")
    assert t.rows == 2 * n and not torch.equal(want, want_hilo)
    c = pl.PoolFeatureCache()
    lazy = LazyPool(x)
    first = pl.encode_pool(t, lazy, chunk=16, cache=c, paths=paths)
    assert torch.equal(first, want) and t.rows == 3 * n and lazy.calls == 3           # 16 + 16 + 5: a ragged tail
    again = pl.encode_pool(t, lazy, chunk=16, cache=c, paths=paths)
    assert again is first and t.rows == 3 * n and lazy.calls == 3                     # nothing encoded, the images never asked for
    assert pl.encode_pool(t, lazy, chunk=16, screen="f16", cache=c, paths=paths) is first
    got_hilo = pl.encode_pool(t, lazy, chunk=16, screen="hilo", cache=c, paths=paths)   # a compensated request is not served the plain entry
    assert torch.equal(got_hilo, want_hilo) and t.rows == 4 * n
    assert c.stats()["entries"] == 1 and c.stats()["bytes"] == 2 * n * 8 * 4
    # a cache without the pool's paths has no key: as without a cache
    assert torch.equal(pl.encode_pool(t, x, chunk=16, cache=c), want) and t.rows == 5 * n
    with pytest.raises(ValueError):
        pl.encode_pool(t, x, chunk=16, cache=c, paths=paths[:-1])
    # prompts: neither read nor written
    before = (c.stats(), t.rows)
    shared, per_image, deep = torch.zeros(1, 2, 8), torch.zeros(n, 2, 8), torch.zeros(1, 2, 8)
    for kw in (dict(prefix=shared), dict(prefix=per_image), dict(prefix=shared, deep=deep)):
        out = pl.encode_pool(t, x, chunk=16, cache=c, paths=paths, **kw)
        assert not torch.equal(out, want)
    assert c.stats() == before[0] and t.rows == before[1] + 3 * n
    assert pl.use_cache(c, prefix=shared) is None and pl.use_cache(c, deep=deep) is None and pl.use_cache(c) is c


def test_nothing_is_cached_unless_a_cache_is_given_or_installed():
    pl = _pl()
    x, paths, t = torch.randn(9, 3, 2, 2), _paths(9), FakeTower()
    assert pl.use_cache(None) is None
    pl.encode_pool(t, x, chunk=4, paths=paths)
    pl.encode_pool(t, x, chunk=4, paths=paths)
    assert t.rows == 18
    c, inner = pl.PoolFeatureCache(), pl.PoolFeatureCache()
    with pl.pool_cache(c) as got:
        assert got is c and pl.use_cache(None) is c
        a = pl.encode_pool(t, x, chunk=4, paths=paths)
        with pl.pool_cache(inner):
            assert pl.use_cache(None) is inner and pl.use_cache(c) is c            # innermost installed; a cache given explicitly wins
        with pl.pool_cache(None):
            assert pl.use_cache(None) is c                                          # installing None installs nothing
        assert pl.encode_pool(t, x, chunk=4, paths=paths) is a
    assert t.rows == 27 and pl.use_cache(None) is None
    with pytest.raises(RuntimeError):
        with pl.pool_cache(c):
            raise RuntimeError("pass failed")
    assert pl.use_cache(None) is None                                               # uninstalled on the way out of a failed pass too
    pl.encode_pool(t, x, chunk=4, paths=paths)
    assert t.rows == 36


def test_partial_tier_hits_return_exactly_the_missing_rows_ascending():
    pl = _pl()
    c = pl.PoolFeatureCache()
    t, other, paths, n = FakeTower(), FakeTower(), _paths(50), 50
    table = torch.arange(n, dtype=torch.float32)[:, None] * torch.ones(1, 8)
    idx = np.array([2, 5, 11, 30, 49])
    assert c.missing_rows(paths, t, idx).tolist() == idx.tolist()
    assert c.store_rows(paths, t, idx, table[idx], n)
    assert c.filled_rows(paths, t).tolist() == idx.tolist()
    ask = np.array([0, 2, 3, 11, 12, 48, 49])
    miss = c.missing_rows(paths, t, ask)
    assert miss.tolist() == [0, 3, 12, 48] and miss.dtype == np.int64
    assert c.missing_rows(paths, other, ask).tolist() == ask.tolist()               # every tower has its own table
    with pytest.raises(KeyError):
        c.rows(paths, t, ask)
    c.store_rows(paths, t, miss, table[miss], n)
    assert torch.equal(c.rows(paths, t, ask), table[ask])                           # in the order asked
    assert c.missing_rows(paths, t, ask).size == 0
    assert c.filled_rows(paths, t).tolist() == sorted(set(idx.tolist()) | set(ask.tolist()))
    assert c.stats()["bytes"] == n * 8 * 4                                          # one dense table, allocated once


def test_budget_refuses_evicts_least_recently_used_and_clear_empties(caplog):
    pl = _pl()
    one = 16 * 8 * 4                        # bytes of one 16-row screen entry
    c = pl.PoolFeatureCache(max_bytes=2 * one + one // 2)
    t = FakeTower()
    pa, pb, pc = _paths(16, "a"), _paths(16, "b"), _paths(16, "c")
    assert c.store_screen(pa, t, "hilo", torch.zeros(16, 8)) and c.store_screen(pb, t, "hilo", torch.ones(16, 8))
    assert c.screen(pa, t) is not None                          # pool a is now the most recently used
    assert c.store_screen(pc, t, "hilo", torch.ones(16, 8))     # no room for three: the least recently used other pool (b) goes
    assert c.screen(pb, t) is None and c.screen(pa, t) is not None and c.screen(pc, t) is not None
    assert c.stats()["bytes"] == 2 * one and c.stats()["pools"] == 2
    # an entry that cannot fit even alone: refused, logged once
    big = _paths(64, "d")
    with caplog.at_level("WARNING"):
        assert not c.store_screen(big, t, "hilo", torch.zeros(64, 8))
        assert not c.store_rows(big, t, np.array([1]), torch.zeros(1, 8), 64)
    assert sum("pool feature cache" in r.getMessage() for r in caplog.records) == 1
    assert c.screen(big, t) is None and c.missing_rows(big, t, np.array([1])).tolist() == [1]
    assert c.stats()["bytes"] == 2 * one and c.screen(pa, t) is not None and c.screen(pc, t) is not None     # nothing was evicted for it
    # a tier table that does not fit beside its own pool's screen entry: the screen entry stays, the table is not created
    c2 = pl.PoolFeatureCache(max_bytes=one + one // 2)
    assert c2.store_screen(pa, t, "hilo", torch.zeros(16, 8))
    assert not c2.store_rows(pa, t, np.array([0]), torch.zeros(1, 8), 16)
    assert c2.screen(pa, t) is not None and c2.stats()["bytes"] == one
    c2.clear()
    assert c2.stats()["bytes"] == 0 and c2.stats()["entries"] == 0 and c2.screen(pa, t) is None


def test_strategy_defaults_carry_the_switch():
    import grip_amd  # noqa: F401
    from grip_amd.methods.main import DEFAULTS
    assert DEFAULTS["CACHE_POOL_FEATURES"] is True and DEFAULTS["POOL_CACHE_MAX_MB"] == 8192
