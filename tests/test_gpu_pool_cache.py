"""pseudolabels.PoolFeatureCache on the GPU: a textual strategy's pseudolabel passes over one pool share the frozen image towers' work.  Cached passes
return the uncached pass's lists (and bits), the f16 screen encodes the pool once, every refinement tower encodes a row once, visual / multimodal
strategies are untouched, and two ranks stay in step without gathering anything they already hold.

Shapes: `small` towers (width 256: the split-f16 tier exists), the class-structured pool of methods.main.synthetic_pool, N = 200 images x 8 classes in
chunks of 48 (four full chunks and a ragged tail of 8).  Encoded rows are counted by wrapping Tower.encode_chunks (sum of hi - lo per tower).  The
screen stream is pinned to "hilo" so that an uncached pass does not switch streams between two calls (screen_stream "auto" does, from the second pass
over a pool on): the row sets the tiers are asked for are then a function of (text features, k) alone, with or without a cache."""
import collections
import glob
import os
import pickle
import socket
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor, as_completed

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

N_CLASSES, PER_CLASS, RES, SEED, CHUNK = 8, 25, 64, 17, 48
K1, K2 = 3, 7                                       # GRIP grows the pseudo-shots per class from pass to pass
TEMPLATES = ("a photo of a {}", "a blurry sketch of one {}")      # pass 2 scores the pool against other text features


@pytest.fixture(autouse=True)
def _pinned_screen_stream(monkeypatch):
    monkeypatch.setenv("GRIP_SCREEN_STREAM", "hilo")
    monkeypatch.delenv("GRIP_PSEUDOLABEL_MODE", raising=False)
    monkeypatch.delenv("GRIP_SPLIT_TIER", raising=False)


@pytest.fixture
def encoded(monkeypatch):
    """encoded(tower) -> rows that tower's encode_chunks has been asked to encode so far."""
    import grip_amd  # noqa: F401
    from grip_amd import engine
    counts, alive = collections.Counter(), []
    real = engine.Tower.encode_chunks

    def counting(self, images, out, lo, hi, *a, **kw):
        if not counts[id(self)]:
            alive.append(self)              # (a counted tower's id is not reused while the test runs)
        counts[id(self)] += max(hi - lo, 0)
        return real(self, images, out, lo, hi, *a, **kw)
    monkeypatch.setattr(engine.Tower, "encode_chunks", counting)
    return lambda tower: counts[id(tower)]


class LazyPool:
    """A lazy pool as utils.clip_pseudolabels._pool_images builds for image files: callable for a slice, .take for scattered rows; counts both."""

    def __init__(self, x):
        self.x, self.n, self.calls, self.taken = x, x.shape[0], 0, 0

    def __call__(self, lo, hi):
        self.calls += 1
        return self.x[lo:hi]

    def take(self, idx):
        self.taken += len(idx)
        return self.x[torch.as_tensor(idx, device=self.x.device)]


_SETUP = {}


def setup():
    """Model, twins, pool and the two passes' text features: built once per process, never modified."""
    if not _SETUP:
        import grip_amd  # noqa: F401
        from grip_amd import clip
        from grip_amd.methods.main import synthetic_pool
        m, _ = clip.load("small", device="cuda")
        twin = m.exact_twin()
        classes, files, images, _ = synthetic_pool(N_CLASSES, PER_CLASS, RES, SEED)
        with torch.no_grad():
            txt = [twin.encode_text(clip.tokenize([t.format(" ".join(c.split("_"))) for c in classes]).cuda()) for t in TEMPLATES]
        _SETUP.update(m=m, twin=twin, x=images.cuda(), paths=[f"/data/pool/{f}" for f in files], labels=list(range(N_CLASSES)), txt=txt)
    return _SETUP


def run_pass(s, which, cache=None, images=None, mid=None):
    """One identical_lists pass: which = 0 (first text features, K1) or 1 (second text features, K2).  Returns (lists, stats)."""
    from grip_amd import pseudolabels as pl
    fp, lab = pl.identical_lists(s["m"].visual.tower, s["twin"].visual.tower, s["x"] if images is None else images, s["txt"][which], 100.0, s["paths"],
                                 s["labels"], (K1, K2)[which], chunk=CHUNK, exact_chunk=CHUNK, mid_chunk=CHUNK, visual_mid=mid, cache=cache)
    return (list(fp), list(lab)), dict(pl.LAST_REFINE_STATS)


_UNCACHED = {}


def uncached(s, which, mid=None):
    key = (which, mid is not None)
    if key not in _UNCACHED:
        _UNCACHED[key] = run_pass(s, which, mid=mid)
    return _UNCACHED[key]


# what a cached pass may differ in from the uncached one: who encoded how much, nothing the lists or bounds rest on
ENCODE_KEYS = {"rows_refined_this_rank", "rows_exact_this_rank", "rows_mid_this_rank", "rows_cached_exact", "rows_cached_mid", "screen_cached",
               "screen_marked_share", "screen_stream_next_pass"}


def same_scan(st, st_ref):
    return {k: v for k, v in st.items() if k not in ENCODE_KEYS} == {k: v for k, v in st_ref.items() if k not in ENCODE_KEYS}


def test_same_pass_twice_encodes_nothing_the_second_time(encoded):
    from grip_amd import pseudolabels as pl
    s = setup()
    t16, t32 = s["m"].visual.tower, s["twin"].visual.tower
    want, st_ref = uncached(s, 0)
    assert len(want[0]) > 0 and st_ref["screen_cached"] is False and st_ref["rows_cached_exact"] == st_ref["rows_cached_mid"] == 0
    c = pl.PoolFeatureCache()
    lazy = LazyPool(s["x"])
    n16, n32 = encoded(t16), encoded(t32)
    first, st1 = run_pass(s, 0, cache=c, images=lazy)
    assert first == want and same_scan(st1, st_ref)
    assert encoded(t16) - n16 == len(s["paths"]) and encoded(t32) - n32 == st_ref["rows_exact"] == st1["rows_exact_this_rank"] == lazy.taken
    assert lazy.calls == 5 and st1["screen_cached"] is False and st1["rows_cached_exact"] == 0
    emb, form = c.screen(s["paths"], t16)
    assert form == "hilo" and torch.equal(emb, pl.encode_pool(t16, s["x"], chunk=CHUNK, screen=form))
    n16, n32, calls, taken = encoded(t16), encoded(t32), lazy.calls, lazy.taken
    second, st2 = run_pass(s, 0, cache=c, images=lazy)
    assert second == want and same_scan(st2, st_ref)
    assert encoded(t16) == n16 and encoded(t32) == n32                 # 0 rows on every tower
    assert lazy.calls == calls and lazy.taken == taken                 # the images are never asked for
    assert st2["screen_cached"] is True and st2["screen_stream"] == "hilo" and st2["rows_cached_exact"] == st_ref["rows_exact"]
    assert st2["rows_exact_this_rank"] == st2["rows_refined_this_rank"] == 0
    assert c.stats()["entries"] == 2 and c.stats()["hits"] > 0


@pytest.mark.parametrize("tiers", [2, 3])
def test_grip_shaped_second_pass_encodes_only_rows_no_tower_has_seen(monkeypatch, encoded, tiers):
    """Pass 2 has other text features and a larger k, as a GRIP iteration has: its lists are the uncached pass's, the screen encodes nothing and a
    refinement tower encodes exactly the rows it is asked for and has not encoded in pass 1.  tiers = 3 forces the split-f16 middle tier
    (GRIP_SPLIT_TIER=1: pools this small would skip it).  That pass 2 asks for rows pass 1 encoded is guaranteed by the calibration sample (refine_scan
    spreads it evenly over the pool: a function of N alone, 64 rows here) and asserted below, so the comparison cannot pass vacuously."""
    from grip_amd import pseudolabels as pl
    s = setup()
    mid = None
    if tiers == 3:
        monkeypatch.setenv("GRIP_SPLIT_TIER", "1")
        mid = pl.mid_tower(s["m"], len(s["paths"]))
        assert mid is not None
    t16, t32 = s["m"].visual.tower, s["twin"].visual.tower
    refiners = {"exact": t32, **({"mid": mid} if mid is not None else {})}
    c = pl.PoolFeatureCache()
    first, _ = run_pass(s, 0, cache=c, mid=mid)
    assert first == uncached(s, 0, mid)[0]
    held = {t: c.filled_rows(s["paths"], tw) for t, tw in refiners.items()}
    # the uncached pass 2, counted
    n0 = {t: encoded(tw) for t, tw in refiners.items()}
    want, st_u = uncached(s, 1, mid)
    unc = {t: encoded(tw) - n0[t] for t, tw in refiners.items()}
    assert want != first and st_u["tiers"] == tiers and unc["exact"] == st_u["rows_exact"] and unc.get("mid", 0) == st_u["rows_mid"]
    # the rows pass 2 asks each tier for: what a pass over an empty cache writes into it
    probe = pl.PoolFeatureCache()
    assert run_pass(s, 1, cache=probe, mid=mid)[0] == want
    asked = {t: probe.filled_rows(s["paths"], tw) for t, tw in refiners.items()}
    assert {t: len(a) for t, a in asked.items()} == unc
    # the cached pass 2
    n16, n0 = encoded(t16), {t: encoded(tw) for t, tw in refiners.items()}
    got, st = run_pass(s, 1, cache=c, mid=mid)
    enc = {t: encoded(tw) - n0[t] for t, tw in refiners.items()}
    assert got == want and same_scan(st, st_u)
    assert encoded(t16) == n16 and st["screen_cached"] is True
    for t, tw in refiners.items():
        again, new = np.intersect1d(asked[t], held[t]), np.setdiff1d(asked[t], held[t])
        assert len(again) > 0, f"{t}: pass 2 asks for no row pass 1 encoded -- the case tests nothing"
        assert enc[t] == len(new) < unc[t], (t, enc, unc)
        assert c.filled_rows(s["paths"], tw).tolist() == np.union1d(asked[t], held[t]).tolist()
    # the new statistics say what was counted
    assert st["rows_exact_this_rank"] == enc["exact"] and st["rows_cached_exact"] == st_u["rows_exact"] - enc["exact"] > 0
    assert st["rows_mid_this_rank"] == enc.get("mid", 0) and st["rows_cached_mid"] == st_u["rows_mid"] - enc.get("mid", 0)
    assert (st["rows_cached_mid"] > 0) == (tiers == 3) and st["rows_refined_this_rank"] == sum(enc.values())


def _strategy(cls_name, tmp_path, monkeypatch, **kw):
    import grip_amd  # noqa: F401
    from grip_amd import methods
    from grip_amd.data import ImagePool, TensorPoolDataset
    from grip_amd.methods.main import synthetic_pool
    from test_gpu_strategies import _conf
    os.makedirs(tmp_path, exist_ok=True)
    monkeypatch.chdir(tmp_path)
    classes, files, images, names = synthetic_pool(6, 20, RES, 23)
    l2i = {c: i for i, c in enumerate(classes)}
    shots = [i for i in range(len(files)) if i % 20 < 2]                     # two labeled shots per class, 108 unlabeled images
    rest = [i for i in range(len(files)) if i % 20 >= 2]
    pool = ImagePool(files, images.cuda())                                    # one pool behind both views: GRIP merges pseudolabeled files into the training list
    train = TensorPoolDataset([files[i] for i in shots], pool, labels=[names[i] for i in shots], label_map=l2i)
    unlabeled = TensorPoolDataset([files[i] for i in rest], pool, labels=None, label_map=l2i)
    conf = _conf(MODEL="grip_" + cls_name.lower(), LEARNING_PARADIGM="ssl", EPOCHS=2, BATCH_SIZE=16, N_PSEUDOSHOTS=2, TEXT_PREFIX_SIZE=4, VISION_PREFIX_SIZE=4, **kw)
    m = getattr(methods, cls_name)(conf, l2i, "", classes, classes, classes, "cuda")
    return m, train, unlabeled


def test_f16_mode_gets_the_plain_stream_embeddings(tmp_path, monkeypatch, encoded):
    """GRIP_PSEUDOLABEL_MODE=f16 labels with the f16 towers' own embeddings (trained_features -> encode_pool(screen=False)): bit-identical with and
    without the cache, so its lists cannot move -- and the compensated screen of an identical-mode pass is another function of the image that a cache
    holding only it must not hand out."""
    from grip_amd import pseudolabels as pl
    m, _, unlabeled = _strategy("TextualFPL", tmp_path, monkeypatch)
    assert isinstance(m.pool_cache, pl.PoolFeatureCache)
    m.define_model(m.classes)
    monkeypatch.setenv("GRIP_PSEUDOLABEL_MODE", "f16")
    t16 = m.clip_model.visual.tower
    images, paths, n = unlabeled.images, list(unlabeled.filepaths), len(unlabeled)
    plain, txt = m.trained_features(images, m.classes, chunk=CHUNK)
    txt = txt.detach()
    # a cache that holds only a "hilo" screen of this pool (what an identical-mode pass leaves)
    hilo = pl.encode_pool(t16, images, chunk=CHUNK, screen="hilo", cache=m.pool_cache, paths=paths)
    assert m.pool_cache.screen(paths, t16) == (hilo, "hilo") and not torch.equal(hilo, plain)
    n0 = encoded(t16)
    with pl.pool_cache(m.pool_cache):
        got = m.trained_features(images, m.classes, chunk=CHUNK, paths=paths)[0]
    assert torch.equal(got, plain) and encoded(t16) - n0 == n            # not served by the "hilo" entry: encoded, and kept as the plain stream
    with pl.pool_cache(m.pool_cache):
        again = m.trained_features(images, m.classes, chunk=CHUNK, paths=paths)[0]
    assert torch.equal(again, plain) and encoded(t16) - n0 == n
    # the whole f16-mode pass of the strategy, with the cache and without
    want = pl.pseudolabel_from_features(plain, txt, m.scale(), paths, [m.label_to_idx[c] for c in m.classes], 4, argmax_on="logits")
    pl.LAST_REFINE_STATS = None
    cached = m.assign_pseudo_labels(4, unlabeled)
    got_lists = (list(cached.filepaths), list(cached.labels))
    assert encoded(t16) - n0 == n and pl.LAST_REFINE_STATS is None       # (f16 mode: no screen-and-refine pass ran)
    unlabeled.filepaths, unlabeled.labels = list(paths), None
    m.pool_cache = None
    plainly = m.assign_pseudo_labels(4, unlabeled)
    assert encoded(t16) - n0 == 2 * n
    assert got_lists == (list(plainly.filepaths), list(plainly.labels)) == (list(want[0]), list(want[1])) and len(want[0]) > 0


def _artefacts(root):
    out = {}
    for f in sorted(glob.glob(os.path.join(root, "pseudolabels", "*.pickle")) + glob.glob(os.path.join(root, "trained_prompts", "*.pickle"))):
        out[os.path.relpath(f, root)] = pickle.load(open(f, "rb"))
    return out


@pytest.mark.parametrize("step_quantile", [50, 25])
def test_textual_grip_encodes_the_pool_once_and_trains_the_same_prompts(tmp_path, monkeypatch, encoded, step_quantile):
    """TextualFPL.grip_train with CACHE_POOL_FEATURES True against False: the pseudolabel files of every iteration and the saved prompts are
    identical, and with the cache the f16 tower walks the unlabeled pool once (the frozen-CLIP pass of iteration 1 fills it) instead of once per
    iteration."""
    runs = {}
    for cache in (True, False):
        m, train, unlabeled = _strategy("TextualFPL", tmp_path / f"cache_{cache}", monkeypatch, STEP_QUANTILE=step_quantile, CACHE_POOL_FEATURES=cache)
        assert (m.pool_cache is not None) == cache
        n = len(unlabeled)
        m.grip_train(train, None, unlabeled)
        runs[cache] = (_artefacts(str(tmp_path / f"cache_{cache}")), encoded(m.clip_model.visual.tower), encoded(m.clip_model.exact_twin().visual.tower))
    iters = 100 // step_quantile
    (files_c, pool_c, exact_c), (files_r, pool_r, exact_r) = runs[True], runs[False]
    assert sorted(files_c) == sorted(files_r) and len([f for f in files_c if "_iter_" in f and f.startswith("pseudolabels")]) == iters
    for name in files_c:
        a, b = files_c[name], files_r[name]
        if name.startswith("pseudolabels"):
            assert a == b and len(a["filepaths"]) > 0, name
        else:
            assert len(a) == len(b) and all(np.array_equal(p, q) and p.dtype == q.dtype for p, q in zip(a, b)), name      # bit-identical prompts
    assert pool_c == n and pool_r == iters * n
    assert 0 < exact_c < exact_r                                             # the f32 tower re-encodes a row once, not once per iteration


@pytest.mark.parametrize("cls_name", ["VisualFPL", "MultimodalFPL"])
def test_strategies_with_trained_visual_prompts_have_no_cache(tmp_path, monkeypatch, encoded, cls_name):
    m, train, unlabeled = _strategy(cls_name, tmp_path, monkeypatch, STEP_QUANTILE=50)
    assert m.pool_cache is None
    n = len(unlabeled)
    m.grip_train(train, None, unlabeled)
    assert encoded(m.clip_model.visual.tower) == 2 * n                       # the pool is encoded every iteration, as before


WORKER = r'''
import os, sys, pickle, torch
sys.path.insert(0, os.environ["GRIP_REPO"]); sys.path.insert(0, os.path.join(os.environ["GRIP_REPO"], "tests"))
import grip_amd
from grip_amd import dist as gdist, pseudolabels as pl
import test_gpu_pool_cache as T
rank, ws = gdist.init_from_env()
s = T.setup()
c = pl.PoolFeatureCache()
first, _ = T.run_pass(s, 0, cache=c)
calls = []
real = c.missing_rows
def missing(paths, tower, idx):
    miss = real(paths, tower, idx)
    calls.append((len(idx), len(miss)))
    return miss
c.missing_rows = missing
gdist.trace("marker pass2_begin")
second, st = T.run_pass(s, 1, cache=c)
gdist.trace("marker pass2_end")
del c.missing_rows
plain = [T.run_pass(s, w)[0] for w in (0, 1)]
with open(os.environ["GRIP_OUT"] + f".{rank}", "wb") as f:
    pickle.dump({"ws": ws, "cached": [first, second], "uncached": plain, "calls": calls, "stats": st}, f)
gdist.barrier()
'''


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_children(cmds_envs, limit):
    """Start the children together, each under its own time limit; the first that fails or runs out of time ends the others."""
    procs = [subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for cmd, env in cmds_envs]
    failure = None
    with ThreadPoolExecutor(max_workers=len(procs)) as ex:
        waits = {ex.submit(p.communicate, timeout=limit): i for i, p in enumerate(procs)}
        for fut in as_completed(waits):
            i = waits[fut]
            try:
                _, err = fut.result()
                bad = None if procs[i].returncode == 0 else f"child {i} exited with {procs[i].returncode}: {err[-3000:]}"
            except subprocess.TimeoutExpired:
                bad = f"child {i} ran past {limit} s"
            if bad and failure is None:
                failure = bad
                for p in procs:
                    p.kill()
    for p in procs:
        p.wait()
    assert failure is None, failure


def test_two_ranks_gather_only_rows_nobody_holds(tmp_path):
    """Two ranks on one GPU over gloo (GRIP_SINGLE_DEVICE=1).  The cached passes return the single-process uncached lists on both ranks; pass 2
    enters no all-gather of pool embeddings and one all-gather of refined rows per tier call that has missing rows -- a tier call whose rows are
    all cached (the calibration sample of pass 1 is one) runs no collective at all."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    base = dict(os.environ, GRIP_SINGLE_DEVICE="1", GRIP_DIST_BACKEND="gloo", GRIP_REPO=REPO, PYTHONPATH=REPO, HSA_ENABLE_IPC_MODE_LEGACY="0",
                GRIP_SCREEN_STREAM="hilo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "GRIP_COMM_TRACE", "GRIP_PSEUDOLABEL_MODE", "GRIP_SPLIT_TIER", "GRIP_NATIVE_COMM"):
        base.pop(k, None)
    cmd = [sys.executable, str(script)]
    _run_children([(cmd, dict(base, GRIP_OUT=str(tmp_path / "single")))], 300)
    port = str(_port())
    trace = str(tmp_path / "comm.log")
    _run_children([(cmd, dict(base, GRIP_OUT=str(tmp_path / "out"), GRIP_COMM_TRACE=trace, WORLD_SIZE="2", RANK=str(r), LOCAL_RANK=str(r),
                              MASTER_ADDR="127.0.0.1", MASTER_PORT=port)) for r in (0, 1)], 300)
    ref = pickle.load(open(str(tmp_path / "single") + ".0", "rb"))
    assert ref["ws"] == 1 and ref["cached"] == ref["uncached"] and ref["uncached"][0] != ref["uncached"][1]
    ranks = [pickle.load(open(str(tmp_path / "out") + f".{r}", "rb")) for r in (0, 1)]
    lines = open(trace).read().splitlines()
    for r, got in enumerate(ranks):
        assert got["ws"] == 2 and got["cached"] == ref["uncached"] and got["uncached"] == ref["uncached"]
        assert got["calls"] == ranks[0]["calls"] == ref["calls"]                   # every rank computes the same miss sets
        mine = [l.split(" ", 1)[1] for l in lines if l.startswith(f"rank{r} ")]
        pass2 = mine[mine.index("marker pass2_begin") + 1: mine.index("marker pass2_end")]
        assert not any("tag=pool_embeddings" in l for l in pass2), pass2
        with_missing = sum(1 for asked, miss in got["calls"] if miss)
        assert len(got["calls"]) == got["stats"]["tier_calls"] and 0 < with_missing < len(got["calls"]), got["calls"]
        assert sum("tag=refined_rows" in l for l in pass2) == with_missing, (pass2, got["calls"])
        assert got["stats"]["screen_cached"] is True and got["stats"]["rows_cached_exact"] == sum(a - b for a, b in got["calls"])
    # the missing rows were encoded once between the two ranks, each its own shard's
    assert sum(g["stats"]["rows_exact_this_rank"] for g in ranks) == sum(b for _, b in ranks[0]["calls"]) == ref["stats"]["rows_exact_this_rank"]
