"""Pseudolabel engine: batched pool encode (sharded over ranks) -> cached text features ->
fused head -> exact sequential leaderboard.  This is the compute behind
utils.clip_pseudolabels.{compute_pseudo_labels, pseudolabel_top_k} and the nine
assign_pseudo_labels of the reference; those keep their signatures in grip_amd.utils / grip_amd.methods.

Two algorithmic changes against the reference loop (utils/clip_pseudolabels.py:31-61), neither of
which changes a result: the class prompts are encoded once instead of once per image, and images
go through the tower in chunks instead of one by one.
"""
import contextlib
import logging
import math
import os
import weakref

import numpy as np
import torch

from . import dist as gdist
from . import engine

log = logging.getLogger(__name__)

K_ALL = 10000000   # utils/clip_pseudolabels.py:27


def _path_ranks_literal(paths):
    order = {p: i for i, p in enumerate(sorted(set(paths)))}
    return np.fromiter((order[p] for p in paths), dtype=np.int64, count=len(paths))


def _path_ranks_bytes(paths):
    """The same ranks without a Python-level sort: ASCII paths as a fixed-width byte matrix (code-point order == byte order, a shorter
    string pads with NUL, which sorts first -- as a proper prefix does in Python), common prefix dropped, 8 bytes per big-endian u64
    column; one SIMD argsort when the first column already separates the strings, a column-wise stable sort otherwise."""
    n = len(paths)
    a = np.array(paths, dtype=np.bytes_)        # UnicodeEncodeError for non-ASCII strings: the caller falls back
    w = a.dtype.itemsize
    if w == 0:
        return np.zeros(n, dtype=np.int64)
    b = a.view(np.uint8).reshape(n, w)
    if int(b.min()) == 0 and any("\0" in p for p in paths):
        raise UnicodeEncodeError("ascii", "", 0, 1, "NUL inside a path")      # (padding and content would be confused)
    varies = b.min(axis=0) != b.max(axis=0)
    if not varies.any():
        return np.zeros(n, dtype=np.int64)
    b = b[:, int(np.argmax(varies)):]
    w = b.shape[1]
    c = np.zeros((n, w + (-w) % 8), dtype=np.uint8)
    c[:, :w] = b
    cols = c.view(">u8")
    first = np.ascontiguousarray(cols[:, 0]).astype(np.uint64)
    order = np.argsort(first)
    s0 = first[order]
    if cols.shape[1] > 1 and (s0[1:] == s0[:-1]).any():
        order = np.lexsort(cols.T[::-1])
    srt = cols[order]
    new = np.empty(n, dtype=np.int64)
    new[0] = 0
    np.cumsum((srt[1:] != srt[:-1]).any(axis=1), out=new[1:])
    out = np.empty(n, dtype=np.int64)
    out[order] = new
    return out


_RANK_CACHE = []        # [(tuple(paths), ranks)], most recent first: GRIP re-labels the same pool every iteration


def path_ranks(paths):
    """Dense rank of every path among all paths under Python's string order (the leaderboard breaks
    score ties by comparing the path strings, utils/clip_pseudolabels.py:79-82).  Vectorised (0.1 s at 400 000 paths against
    0.6 s for the literal form, tools/scan_scale.py) and remembered for the last few pools."""
    key = tuple(paths)
    for i, (k, r) in enumerate(_RANK_CACHE):
        if len(k) == len(key) and k == key:          # element-wise; identical string objects compare by pointer
            if i:
                _RANK_CACHE.insert(0, _RANK_CACHE.pop(i))
            return r
    try:
        r = _path_ranks_bytes(paths)
    except (UnicodeEncodeError, TypeError, ValueError):
        r = _path_ranks_literal(paths)
    r.setflags(write=False)
    _RANK_CACHE.insert(0, (key, r))
    del _RANK_CACHE[4:]
    return r


# When the compensated screen pays: it costs +6.6 % encode time -- as much as re-encoding 2.2 % of the pool with the split-f16 tier (0.1 ms against 34 us per image) -- and
# saves the rows its 2.2x tighter bound no longer marks: measured r06 at N = 50 000, 30 % of the plain screen's marked rows on the near-uniform timed pool (2 836 -> 1 999:
# plain wins by 1 %), 44 % on the structured pool (4 472 -> 2 498: compensated wins by 3 %), and the difference between 9.0k and 11.3k img/s on the stress model.
SCREEN_HILO_KEEP = 0.040    # a COMPENSATED pass that still marked more than this share of the pool (calibration, audit and non-finite rows aside) keeps the next pass compensated
SCREEN_HILO_TAKE = 0.064    # a PLAIN pass that marked more than this share sends the next pass to the compensated stream (the same break-even seen from the other side)
_SCREEN_CHOICE = {}         # pool key -> stream the NEXT pass over it screens with (what its last pass measured)


def screen_stream(key=None):
    """Residual stream of the f16 tower when it SCREENS a pool for identical_lists.  "hilo": a compensated pair of f16 numbers per element
    (GRIP_FWD_STREAM_HILO: the 24 roundings of the stream of a ViT-B/16 image no longer accumulate; the embeddings' direction error against the f32
    tower and the measured bound of the screen drop 2.2 - 2.5x, for +6.6 % encode time).  "f16": the plain stream (rounds 1-5).  $GRIP_SCREEN_STREAM =
    "auto" (default) picks per pool: the first pass over a pool screens compensated (the safe side: it never costs more than 6.6 %), every pass records the
    share of the pool its scan marked (note_screen_bound), and the next pass over the same pool -- GRIP re-labels one pool every iteration,
    pseudo_iterative.py:62-125 -- screens plain where that share says the tighter bound does not pay (SCREEN_HILO_KEEP / _TAKE).  The lists do not depend on
    the choice (both screens are certified against the same exact values); only the number of re-encoded rows does.  Train-mode forwards, evaluation and
    the f16 MODE always keep the plain stream."""
    v = os.environ.get("GRIP_SCREEN_STREAM", "auto")
    if v not in ("auto", "hilo", "f16"):
        raise ValueError(f"GRIP_SCREEN_STREAM={v!r}: expected 'auto', 'hilo' or 'f16'")
    return _SCREEN_CHOICE.get(key, "hilo") if v == "auto" else v


def note_screen_bound(key, stream, stats):
    """Record what a pass measured, for screen_stream("auto"): the share of the pool its scan marked decides the next pass's stream.  The statistics are
    identical on every rank, so every rank decides alike."""
    if key is None or not stats or stats.get("rows", 0) == 0:
        return
    marked = max(0, stats["rows_refined"] - stats["calibration_rows"] - stats["audit_rows"] - stats.get("nonfinite_screen_rows", 0)) / stats["rows"]
    _SCREEN_CHOICE[key] = "hilo" if marked > (SCREEN_HILO_KEEP if stream == "hilo" else SCREEN_HILO_TAKE) else "f16"
    stats["screen_stream"] = stream
    stats["screen_marked_share"] = marked
    stats["screen_stream_next_pass"] = _SCREEN_CHOICE[key]


# ------------------------------------------------------------------------------------------ frozen pool features across passes
POOL_CACHE_MAX_BYTES = 8 << 30      # per process.  A condition, not a measurement: 400 000 rows x 768 x 4 B x 3 tables ~ 3.7 GB is the largest pool a tool in the tree walks
_PLAIN_FORMS = ("f16", "plain")     # one function of the image: the plain residual stream, chosen as a screen ("f16") or asked for as it is (screen=False: "plain")
SCREEN_FORMS = ("hilo",) + _PLAIN_FORMS


def screen_forms(screen):
    """The cached stream forms an encode_pool(screen=...) request could have produced itself: the compensated stream serves only "hilo" requests; the
    plain stream is the same bits whether a screen picked it ("f16") or a caller asked for plain embeddings (False)."""
    return ("hilo",) if screen == "hilo" else _PLAIN_FORMS


class _TowerEntry:
    def __init__(self, tower):
        self.ref = weakref.ref(tower)       # not id(): a freed tower's id can come back with other weights
        self.screen = {}                    # stream form -> [N, E] f32 (the gathered pool embeddings, identical on every rank)
        self.rows = self.filled = None      # refinement tier: dense [N, E] f32 table + host mask of the rows it holds

    def tensors(self):
        return list(self.screen.values()) + ([self.rows] if self.rows is not None else [])

    def nbytes(self):
        return sum(_nbytes(t) for t in self.tensors())


def _nbytes(t):
    return t.untyped_storage().nbytes()     # (a gathered pool is a view of its padded buffer: the buffer is what stays resident)


class PoolFeatureCache:
    """Embeddings of FROZEN, prompt-free image towers over ordered pools, kept on the device between pseudolabel passes.  GRIP and iterative FPL label
    one pool every iteration (pseudo_iterative.py:62-125); with a textual strategy only the text features change between the passes, so the f16
    screen's embeddings and every row a refinement tower has re-encoded are the same bits each time.

    One entry per (pool, tower).  A pool is its ordered path tuple, compared element-wise like _RANK_CACHE (the paths NAME the images: a caller
    that puts other images behind the same paths must clear()).  A tower is held by weak reference: the entry of a freed tower is unreachable
    and dropped.  Calls with a visual prompt, per-image prompts or deep prompts must not come here at all (use_cache): their embeddings depend on
    trained parameters.  Screen embeddings are kept under the stream form they were encoded in (SCREEN_FORMS) and handed out only for forms the
    request could have produced itself; a tier entry is a dense [N, E] table and a mask of the rows written so far -- from the all-gathered rows, so
    every rank holds the same content and computes the same miss set.

    Budget: `max_bytes` over everything held (default POOL_CACHE_MAX_BYTES).  Storing evicts OTHER pools, least recently used first; an entry that
    still does not fit is not stored (logged once) and the pass runs as it does without a cache.  Tensors handed out are the cached ones: read-only."""

    def __init__(self, max_bytes=POOL_CACHE_MAX_BYTES):
        self.max_bytes = int(max_bytes)
        self._pools = []            # [(path tuple, [_TowerEntry])], most recently used first
        self.hits = self.misses = 0
        self._refused = False

    # ---- lookup
    def _find(self, paths, tower, create=False):
        key = paths if isinstance(paths, tuple) else tuple(paths)
        for _, towers in self._pools:           # entries of freed towers are unreachable: drop them (and a pool nothing is left of)
            towers[:] = [t for t in towers if t.ref() is not None]
        self._pools[:] = [p for p in self._pools if p[1]]
        for i, (k, towers) in enumerate(self._pools):
            if k is key or (len(k) == len(key) and k == key):      # element-wise; identical string objects compare by pointer
                if i:
                    self._pools.insert(0, self._pools.pop(i))
                break
        else:
            if not create:
                return None
            towers = []
            self._pools.insert(0, (key, towers))
        for t in towers:
            if t.ref() is tower:
                return t
        if create:
            towers.append(_TowerEntry(tower))
            return towers[-1]
        return None

    def _room(self, paths, need):
        """Make room for `need` more bytes of pool `paths`: other pools go, least recently used first; False when it cannot fit."""
        key = paths if isinstance(paths, tuple) else tuple(paths)
        other = [i for i, (k, _) in enumerate(self._pools) if not (len(k) == len(key) and k == key)]
        held = lambda ids: sum(t.nbytes() for i in ids for t in self._pools[i][1] if t.ref() is not None)      # noqa: E731
        own = held(set(range(len(self._pools))) - set(other))
        if own + need > self.max_bytes:         # not even alone: nothing is evicted for it
            if not self._refused:
                self._refused = True
                log.warning("pool feature cache: %.1f MB more for a pool of %d images do not fit the budget of %.1f MB: not cached, the pass re-encodes "
                            "as without a cache", need / 2 ** 20, len(key), self.max_bytes / 2 ** 20)
            return False
        while own + held(other) + need > self.max_bytes:
            del self._pools[other.pop()]        # (indices ascend: the last is the least recently used, and deleting it moves no other)
        return True

    # ---- screen
    def screen(self, paths, tower, forms=SCREEN_FORMS):
        """(embeddings [N, E], form) of the pool through `tower` in one of the stream `forms`, or None."""
        e = self._find(paths, tower)
        for f in forms if e is not None else ():
            if f in e.screen:
                self.hits += 1
                return e.screen[f], f
        self.misses += 1
        return None

    def store_screen(self, paths, tower, form, emb):
        """Keep the gathered [N, E] embeddings of the pool under stream form `form`.  False: over budget, not kept."""
        if form not in SCREEN_FORMS:
            raise ValueError(f"stream form {form!r}: expected one of {SCREEN_FORMS}")
        e = self._find(paths, tower)
        if e is not None and form in e.screen:
            return True
        if not self._room(paths, _nbytes(emb)):
            return False
        self._find(paths, tower, create=True).screen[form] = emb
        return True

    # ---- refinement tiers
    def missing_rows(self, paths, tower, idx):
        """The rows of `idx` (ascending) that `tower` has not encoded for this pool yet, ascending."""
        idx = np.asarray(idx, dtype=np.int64)
        e = self._find(paths, tower)
        miss = idx if e is None or e.filled is None else idx[~e.filled[idx]]
        if idx.size:
            if miss.size:
                self.misses += 1
            else:
                self.hits += 1
        return miss

    def filled_rows(self, paths, tower):
        """Ascending row numbers of the pool `tower` holds embeddings of."""
        e = self._find(paths, tower)
        return np.empty(0, np.int64) if e is None or e.filled is None else np.flatnonzero(e.filled)

    def store_rows(self, paths, tower, idx, rows, n):
        """Write the embeddings `rows` [len(idx), E] of the pool rows `idx` (of `n`) into the tier table of `tower`.  False: the table does not fit
        the budget and nothing was kept."""
        idx = np.asarray(idx, dtype=np.int64)
        e = self._find(paths, tower)
        if e is None or e.rows is None:
            if not self._room(paths, int(n) * rows.shape[1] * 4):
                return False
            e = self._find(paths, tower, create=True)
            e.rows = torch.zeros(int(n), rows.shape[1], dtype=torch.float32, device=rows.device)
            e.filled = np.zeros(int(n), dtype=bool)
        if idx.size:
            e.rows[torch.as_tensor(idx, device=e.rows.device)] = rows
            e.filled[idx] = True
        return True

    def rows(self, paths, tower, idx):
        """Embeddings [len(idx), E] of rows `idx`, all of which the tier table must hold."""
        idx = np.asarray(idx, dtype=np.int64)
        e = self._find(paths, tower)
        if e is None or e.filled is None or not e.filled[idx].all():
            raise KeyError("pool feature cache: rows asked for that were never stored")
        return e.rows[torch.as_tensor(idx, device=e.rows.device)]

    # ---- housekeeping
    def clear(self):
        self._pools.clear()

    def stats(self):
        live = [t for _, towers in self._pools for t in towers if t.ref() is not None]
        return {"bytes": sum(t.nbytes() for t in live), "entries": len(live), "pools": len(self._pools), "hits": self.hits, "misses": self.misses,
                "max_bytes": self.max_bytes}


_INSTALLED = []     # caches installed by pool_cache(), innermost last.  Empty unless a caller opened one: nothing is cached by default


@contextlib.contextmanager
def pool_cache(cache):
    """Install `cache` (a PoolFeatureCache, or None: no-op) for the encode_pool / identical_lists calls underneath that are not given one -- how it
    reaches the reference-named compute_pseudo_labels / pseudolabel_top_k, whose signatures are the reference's."""
    if cache is None:
        yield None
        return
    _INSTALLED.append(cache)
    try:
        yield cache
    finally:
        _INSTALLED.pop()


def use_cache(cache, prefix=None, deep=None):
    """The cache a pool pass works with: the one given, else the innermost installed one, else None -- and None for every call with a visual prompt
    (shared or per image) or deep prompts: those embeddings depend on trained parameters, the cache is neither read nor written."""
    if prefix is not None or deep is not None:
        return None
    return cache if cache is not None else (_INSTALLED[-1] if _INSTALLED else None)


@torch.no_grad()
def encode_pool(visual_tower, images, chunk=880, prefix=None, out=None, screen=False, deep=None, cache=None, paths=None):
    """Encode an ordered pool.  `images` is a tensor [N,3,R,R] (any device) or a callable
    (lo, hi) -> tensor for that slice.  With torch.distributed initialised the pool is sharded
    contiguously and the embeddings are all-gathered; returns [N, E] f32 on the device.
    screen: False, or the stream form ("hilo" / "f16") of a screen-and-refine pass's screen; True = screen_stream() without a pool history.
    prefix: None, one visual prompt for the whole pool ([P, d] / [1, P, d]), or one per image ([N, P, d], aligned with `images`: each rank
    reads the prompts of its own shard).  deep: None or [D, P, d] deep prompts of a shared prompt (Tower.encode_chunks).
    cache + paths: a PoolFeatureCache (or one installed by pool_cache) and the pool's ordered paths: a prompt-free call returns the cached embeddings
    of a stream form this request could have produced (screen_forms) without touching `images`, and stores what it had to encode."""
    if screen is True:
        screen = screen_stream()
    n = images.shape[0] if torch.is_tensor(images) else images.n
    cache = use_cache(cache, prefix, deep) if paths is not None else None
    if cache is not None:
        if len(paths) != n:
            raise ValueError(f"{len(paths)} paths for a pool of {n} images")
        paths = paths if isinstance(paths, tuple) else tuple(paths)
        hit = cache.screen(paths, visual_tower, screen_forms(screen))
        if hit is not None:
            return hit[0]
    if engine.is_per_image_prefix(prefix) and prefix.shape[0] != n:
        raise ValueError(f"per-image visual prompts [{prefix.shape[0]}, P, d] for a pool of {n} images")
    lo, hi, per = gdist.shard_range(n)
    dev = visual_tower.device
    local = torch.empty(max(hi - lo, 0), visual_tower.embed_dim, dtype=torch.float32, device=dev)
    visual_tower.encode_chunks(images, local, lo, hi, chunk, prefix, hilo=screen == "hilo", deep=deep)
    emb = gdist.allgather_rows(local, n, per, tag="pool_embeddings")
    if cache is not None:
        cache.store_screen(paths, visual_tower, screen or "plain", emb)
    return emb


def leaderboard(probs, pred, paths, class_labels, k):
    """(filepaths, labels) exactly as utils/clip_pseudolabels.py:103-112 rebuilds them."""
    if k == K_ALL:
        return list(paths), [class_labels[int(j)] for j in pred]
    img, cls = engine.leaderboard_scan(probs, pred, path_ranks(paths), k)
    return [paths[i] for i in img], [class_labels[int(c)] for c in cls]


# ------------------------------------------------------------------------------------------ screen and refine
REFINE_CALIB_ROWS = 256     # rows re-encoded exactly up front to measure the cheaper tiers' deviation on THIS pool
REFINE_MIN_SAMPLE = 64      # ... and never fewer than this (calibration and audit alike; pools under 256 rows: a quarter of the pool, at least 16).  Was 16 until r06: the
                            # log-odds bound of the compensated screen is tighter than any bound before it, and 18 rows are a thin sample to take a maximum over
REFINE_SAFETY = 2.0         # bound = safety x the largest deviation seen on any row re-encoded so far (it only ever grows)
REFINE_SAFETY_MID = 4.0     # the same for the middle tier: its bound rests on a quarter of the calibration rows (an f32 row costs 2.5 split-f16 ones), so it is
                            # given twice the margin instead (8 x was measured: 293 instead of 222 f32 rows per pass on the bench pool, +0.025 s) -- at 1e-5-sized deviations the extra band holds a handful of rows
REFINE_ESCALATE_AFTER = 8   # rounds after which whatever is still un-refined moves up a tier in one go (pathological pools only, see refine_scan)
REFINE_AUDIT_ROWS = 256     # un-refined rows re-encoded AFTER the scan certified its lists, to check the bound they were trusted to ($GRIP_REFINE_AUDIT)
REFINE_AUDIT_ROWS_LARGE = 1024   # ... for pools of REFINE_AUDIT_LARGE_POOL rows and more (what the lists take on trust there rests on a four times larger hold-out)
REFINE_AUDIT_LARGE_POOL = 50000
REFINE_AUDIT_MID_ROWS = 32  # rows the MIDDLE tier is trusted on that an audit sends through the exact tower (its deviations are f32-rounding-sized and tightly
                            # distributed; every row the scan sends on to the exact tower adds to the sample; an f32 row costs 2.5 split-f16 ones)
REFINE_MAX_AUDITS = 4       # audits that may each widen the bound before everything left is simply re-encoded
REFINE_ABS_EPS = 1e-30      # absolute slack of an un-refined probability: below this a softmax output has no relative accuracy (denormals, 0)
_EPS_CAP = 9e5              # grip_leaderboard_scan_bounded takes relative bounds below 1e6 (a bound >= 1 already means "anything below")
_DELTA_CAP = 80.0           # ... and log-odds bounds below 700 (e^80 already turns every interval into (0, 1))
_KR = _KU = 2.0 ** -20      # the log-odds form's slack for the f32 evaluation of p and 1 - p (csrc/leaderboard.cpp: kR, kU)


def audit_rows_default(n=0):
    v = os.environ.get("GRIP_REFINE_AUDIT", "")
    return int(v) if v.strip() else (REFINE_AUDIT_ROWS_LARGE if n >= REFINE_AUDIT_LARGE_POOL else REFINE_AUDIT_ROWS)


def bound_form():
    """Form of the per-row bound the screen-and-refine pass works with: "odds" (default) -- every entry's odds p / (1 - p) are known to a factor
    e^{+-delta} (include/grip_amd.h, bound_form 1: the form a logit error takes; tight for the p ~ 0.9+ entries on the board thresholds of a peaked
    pool) -- or "relative" (rounds 3-5: one relative bound on every probability of a tier).  $GRIP_REFINE_BOUND."""
    v = os.environ.get("GRIP_REFINE_BOUND", "odds")
    if v not in engine.BOUND_FORMS:
        raise ValueError(f"GRIP_REFINE_BOUND={v!r}: expected 'odds' or 'relative'")
    return v


def _deviation(approx, better, abs_eps):
    """Largest relative deviation between the approximate probabilities `approx` and the more accurate `better` of the same
    rows, beyond the absolute slack, relative to the SMALLER of the two values (so it bounds |better - approx| / approx, the form
    the scan's intervals use, and |approx / better - 1|, the form include/grip_amd.h states, alike).  Pairs that both lie inside
    the absolute slack are covered by it; a pair with one value at 0 and the other above the slack deviates infinitely."""
    a, b = np.asarray(approx, dtype=np.float64), np.asarray(better, dtype=np.float64)
    big = np.maximum(a, b) > abs_eps
    if not big.any():
        return 0.0
    d = np.maximum(np.abs(a - b)[big] - abs_eps, 0.0)
    m = np.minimum(a, b)[big]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, d / m, 0.0)
    return float(np.max(r))


def odds_interval(p, delta, abs_eps):
    """(lo, hi) of the true probability given an approximate `p` whose row obeys the log-odds bound `delta`: the numpy restatement of RowBound::interval
    (csrc/leaderboard.cpp, bound_form 1) that _deviation_odds inverts (tests hold the two together)."""
    s = np.asarray(p, dtype=np.float64)
    E = np.exp(np.float64(delta))
    q = 1.0 - s
    a_hi, a_lo = s * (1.0 + _KR), s * (1.0 - _KR)
    q_lo, q_hi = np.maximum(q - _KU, 0.0), np.maximum(q, 0.0) + _KU
    with np.errstate(divide="ignore", invalid="ignore"):
        hi = a_hi / (a_hi + q_lo / E) * (1.0 + _KR) + abs_eps
        lo = a_lo / (a_lo + q_hi * E) * (1.0 - _KR) - abs_eps
    return lo, hi


def _deviation_odds(approx, better, abs_eps):
    """Smallest delta >= 0 for which every value of `better` lies inside the log-odds interval of the corresponding value of `approx`
    (odds_interval): the largest deviation of the rows' odds, in the form the scan uses it.  Pairs inside the absolute slack deviate by 0; an approximate
    0 against a better value above the slack deviates infinitely."""
    a, b = np.asarray(approx, dtype=np.float64).ravel(), np.asarray(better, dtype=np.float64).ravel()
    if a.size == 0:
        return 0.0
    q = 1.0 - a
    a_hi, a_lo = a * (1.0 + _KR), a * (1.0 - _KR)
    q_lo, q_hi = np.maximum(q - _KU, 0.0), np.maximum(q, 0.0) + _KU
    with np.errstate(divide="ignore", invalid="ignore"):
        bu = (b - abs_eps) / (1.0 + _KR)                   # upper side: bu <= a_hi / (a_hi + q_lo / E)
        need = bu > a_hi / (a_hi + q_lo)
        e_up = np.where(need, np.where((a_hi > 0) & (bu < 1.0), q_lo * bu / (a_hi * (1.0 - bu)), np.inf), 1.0)
        bl = (b + abs_eps) / (1.0 - _KR)                   # lower side: bl >= a_lo / (a_lo + q_hi E)
        need = bl < a_lo / (a_lo + q_hi)
        e_lo = np.where(need, np.where(bl > 0, a_lo * (1.0 - bl) / (bl * q_hi), np.inf), 1.0)
    e = max(1.0, float(np.max(e_up)), float(np.max(e_lo)))
    return float(np.log(e)) if np.isfinite(e) else float("inf")


def scan_placement():
    """Where the bounded scan of a multi-rank pass runs: "root" (default) -- rank 0 scans with the CPUs of the whole node and broadcasts lists and
    marks -- or "replicated" (every rank scans: what rounds 1-4 did).  The scan is sequential and does not shard; replicated, the g ranks
    of a node run it at the same moment on 1/g of the CPUs each.  $GRIP_SCAN_PLACEMENT."""
    v = os.environ.get("GRIP_SCAN_PLACEMENT", "root")
    if v not in ("root", "replicated"):
        raise ValueError(f"GRIP_SCAN_PLACEMENT={v!r}: expected 'root' or 'replicated'")
    return v


def _usable_cpus():
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except Exception:
        pass
    return n


def scan_bounded(probs, pred, ranks, rel, k, abs_eps, form="relative"):
    """engine.leaderboard_scan_bounded for the current process group: one rank, or placement "replicated": the local scan.  Placement "root": rank 0
    runs it on every CPU the process may use (the native default divides them by $LOCAL_WORLD_SIZE; the count travels as an argument, ABI 8) and the
    other ranks receive (img, cls, ambiguous) in one broadcast of k C + N / 4 words -- they spend no CPU on it and cannot disagree with rank 0
    (tests/test_dist_gloo.py).  The first word of that message is the pair count, or -1 when rank 0's scan failed: every rank then raises together
    instead of waiting in the broadcast for the collective's watchdog."""
    rank, ws = gdist.world()
    if ws == 1 or scan_placement() != "root":
        return engine.leaderboard_scan_bounded(probs, pred, ranks, rel, k, abs_eps, form=form)
    n, c = probs.shape
    cap = n if int(k) == K_ALL else c * max(1, min(int(k), n))
    words = (n + 3) // 4
    buf = np.zeros(1 + 2 * cap + words, dtype=np.int32)
    failure = None
    if rank == 0:
        try:
            threads = 0 if "GRIP_SCAN_THREADS" in os.environ else min(16, _usable_cpus())
            img, cls, amb = engine.leaderboard_scan_bounded(probs, pred, ranks, rel, k, abs_eps, form=form, threads=threads)
            buf[0] = len(img)
            buf[1: 1 + len(img)] = img
            buf[1 + cap: 1 + cap + len(cls)] = cls
            buf[1 + 2 * cap:].view(np.uint8)[:n] = amb
        except (engine.native.GripError, MemoryError) as e:
            failure = e
            buf[0] = -1
    gdist.broadcast_array_(buf)
    m = int(buf[0])
    if m < 0:
        raise failure if failure is not None else engine.native.GripError("bounded leaderboard scan failed on rank 0 (see its log)")
    return buf[1: 1 + m].copy(), buf[1 + cap: 1 + cap + m].copy(), buf[1 + 2 * cap:].view(np.uint8)[:n].astype(bool)


def refine_scan(probs, pred, ranks, k, exact_rows, calib=REFINE_CALIB_ROWS, safety=REFINE_SAFETY, max_rounds=64, mid_rows=None,
                audit=None, abs_eps=REFINE_ABS_EPS, bound=None):
    """Leaderboard lists of the reference's fp32 scan from probabilities of the f16 towers (utils/clip_pseudolabels.py:38-112).

    `probs` [N, C] f32 / `pred` [N] come from the f16 image tower (the SCREEN; modified in place); `exact_rows(idx)` returns the
    exact (f32-tower) probabilities and arg-max of the rows `idx` (ascending int64 array); `mid_rows(idx)`, optional, the same from
    a MIDDLE tier (the split-f16 tower: far more accurate than the screen, several times cheaper than the f32 tower).  A row
    sits at level 0 (screen), 1 (middle) or 2 (exact, final).  Level-0 / level-1 values are trusted only up to a relative bound
    eps[level] = safety x (largest deviation seen so far between a value of that level and the better value that later replaced it),
    plus an absolute slack `abs_eps` for values in the denormal range; the bounds start from `calib` rows -- at most 1/16 of the pool,
    at least REFINE_MIN_SAMPLE = 64 -- spread evenly over it: all of them through the next tier up, every fourth through the exact tower as well when there
    is a middle tier.  grip_leaderboard_scan_bounded marks every non-final row
    that takes part in a comparison its bound cannot decide; marked rows move up one tier and the scan repeats until nothing is
    marked and no bound has moved: the lists are then certified, decision by decision, to be those of the scan over the all-f32
    probabilities PROVIDED every non-final row obeys its bound.

    That proviso is a measured bound, not a theorem about f16 arithmetic, so it is AUDITED: after certification `audit` (default
    256, 1 024 for pools of 50 000 rows and more; $GRIP_REFINE_AUDIT; 0 = off; at most 1/16 of the pool but at least 64) rows still at level 0 -- half of them members of the final boards where there are any, the rest
    drawn uniformly from the pool (seeded: every rank draws the same rows) -- are re-encoded by the next tier; if one of them turns
    out to deviate by MORE than the bound it was trusted to, the bound was understated: it is widened to safety x that deviation, the scan
    repeats under it and is audited again (at most REFINE_MAX_AUDITS times, after which every row left is re-encoded).  stats reports the audit (`audit_rows`, `audit_max_deviation`, `audit_widened`), the rows the final lists
    still take on trust (`unverified_rows`) and the number of rows every bound rests on (`observed_rows`).

    `bound` ("odds" / "relative", default bound_form()): what a tier's bound says.  "relative": every probability of the row is within the relative
    eps of the truth.  "odds" (r06): every entry's odds p / (1 - p) are within a factor e^{+-delta} of the truth -- the same statement for the small
    entries, (1 - p) times tighter for the large ones, and the one an embedding-direction error actually produces (a logit error of
    scale x <de, t_c>, whatever the probability).  Deviations are measured in the same form, entry by entry (_deviation_odds), so calibration,
    growth and audit work unchanged; `eps` / `max_deviation` in the stats are then deltas.
    Returns (img, cls, stats)."""
    n, c = probs.shape
    form = bound_form() if bound is None else bound
    if form not in engine.BOUND_FORMS:
        raise ValueError(f"refine_scan: bound={form!r}")
    deviation = _deviation if form == "relative" else _deviation_odds
    cap = _EPS_CAP if form == "relative" else _DELTA_CAP
    audit = audit_rows_default(n) if audit is None else int(audit)
    if audit > 0:
        audit = min(n, max(min(REFINE_MIN_SAMPLE, max(16, n // 4)), min(audit, n // 16)))       # like the calibration sample: at most 1/16 of the pool, at least 64 (16 .. n / 4 on tiny pools)
    level = np.zeros(n, dtype=np.int8)
    dev = [0.0, 0.0]                # largest deviation seen of a level-0 / level-1 value from the better value that replaced it
    n_mid = n_exact = 0

    def submit(fn, idx):
        """Start a tier's re-encode of rows `idx`: tier callbacks with a `.submit(idx)` (the GPU tiers: work enqueued on the tier's own stream, nothing
        waited for) return a callable that waits and hands back (probs, argmax); plain callbacks run here and now.  Two tiers submitted back to back run side
        by side on the GPU -- the f32 tower's few hundred rows per pass no longer run alone at a third of its rate (r06)."""
        idx = np.asarray(idx, dtype=np.int64)
        if idx.size == 0:
            return None
        stats["tier_calls"] += 1
        if hasattr(fn, "submit"):
            return fn.submit(idx)
        out = fn(idx)
        return lambda: out

    def to_exact(idx, measure=True, pending=None):
        nonlocal n_exact
        idx = np.asarray(idx, dtype=np.int64)
        if idx.size == 0:
            return
        p32, a32 = (pending or submit(exact_rows, idx))()
        for lv in (0, 1):
            sel = (level[idx] == lv) & np.isfinite(probs[idx]).all(axis=1)       # (a non-finite row says nothing about the tier's accuracy)
            if measure and sel.any():
                dev[lv] = max(dev[lv], deviation(probs[idx[sel]], p32[sel], abs_eps))
        probs[idx] = p32
        pred[idx] = a32
        level[idx] = 2
        n_exact += idx.size

    def to_mid(idx, pending=None):
        nonlocal n_mid
        idx = np.asarray(idx, dtype=np.int64)
        if idx.size == 0:
            return
        pm, am = (pending or submit(mid_rows, idx))()
        n_mid += idx.size           # (rows the tier ENCODED: an overflow inside it is paid for all the same)
        bad = ~np.isfinite(pm).all(axis=1)
        if bad.any():       # an overflow inside the cheaper tower (f16 range): those rows go straight to the exact tower
            to_exact(idx[bad], measure=False)
            idx, pm, am = idx[~bad], pm[~bad], am[~bad]
            if idx.size == 0:
                return
        # the middle tier's value is itself only known to eps[1]: a screen value within d of it is within d (1 + eps1) + eps1 of the truth
        # (log-odds form: the two factors multiply, the deltas add)
        fin = np.isfinite(probs[idx]).all(axis=1)      # (a non-finite screen row says nothing about the tier's accuracy: as in to_exact)
        if fin.any():
            d = deviation(probs[idx[fin]], pm[fin], abs_eps)
            dev[0] = max(dev[0], d * (1.0 + eps[1]) + eps[1] if form == "relative" else d + eps[1] + 4 * _KR)
        probs[idx] = pm
        pred[idx] = am
        level[idx] = 1

    def up(idx):
        """Move rows up one tier: level 0 -> middle tier where there is one, everything else -> exact."""
        idx = np.asarray(idx, dtype=np.int64)
        lo = idx[level[idx] == 0] if mid_rows is not None else idx[:0]
        hi = idx[level[idx] == 1] if mid_rows is not None else idx
        h_lo, h_hi = submit(mid_rows, lo), submit(exact_rows, hi)        # both tiers in flight before either is waited for
        to_mid(lo, pending=h_lo)
        to_exact(hi, pending=h_hi)

    def bound(lv):
        return min((safety if lv == 0 else max(safety, REFINE_SAFETY_MID)) * dev[lv], cap)

    stats = {"rows": n, "calibration_rows": 0, "rounds": 0, "scans": 0, "tier_calls": 0, "audits": 0, "audit_rows": 0, "audit_board_rows": 0, "audit_max_deviation": 0.0,
             "audit_widened": False}
    eps = [0.0, 0.0]
    if n == 0:
        return np.empty(0, np.int32), np.empty(0, np.int32), dict(stats, rows_refined=0, rows_mid=0, rows_exact=0, eps=0.0, eps_mid=0.0, max_deviation=0.0,
                                                                    max_deviation_mid=0.0, refined_per_round=[], safety=float(safety), unverified_rows=0,
                                                                    observed_rows=0, tiers=2 + (mid_rows is not None))
    broken = np.flatnonzero(~np.isfinite(probs).all(axis=1))       # rows the screen overflowed on (f16 range): up a tier at once, outside every bound --
    stats["nonfinite_screen_rows"] = int(broken.size)               # and BEFORE the calibration, so that none of them can enter a measured deviation.
    if mid_rows is not None:            # The middle tier keeps an f32 residual stream: it resolves them at 2.5x the exact tower's rate (what it
        to_mid(broken)                  # overflows on itself goes on to the exact tower inside to_mid); r05 sent them to the exact tower directly
    else:
        to_exact(broken, measure=False)
    # calibration rows: `calib`, but at most 1/16 of the pool -- and never fewer than REFINE_MIN_SAMPLE (a bound from a handful of rows is no bound) -- spread evenly over
    # the rows the screen is still trusted on (a row it overflowed on measures nothing; with no such rows: over the pool, as before)
    live = np.flatnonzero(level == 0)
    want = min(live.size, max(min(REFINE_MIN_SAMPLE, max(16, n // 4)), min(calib, n // 16)))
    cal = live[np.unique(np.linspace(0, live.size - 1, want).astype(np.int64))] if want else live
    if cal.size == 0:
        pass                            # every row is final already (an all-non-finite screen): nothing to calibrate, nothing left to trust
    elif mid_rows is not None:
        # With a middle tier the screen's bound is calibrated against IT (every calibration row; its own error is folded in), and the middle
        # tier's bound against the exact tower on every fourth calibration row (at least 16): its deviations are f32-rounding-sized and tightly
        # distributed (three f16 products with f32 accumulation: ~3 x 2^-23 per term), the rows the scan sends on to the exact tower and the
        # audit keep adding to the sample, and an f32 row costs 2.5x a split-f16 one.
        cal_x = cal[:: max(1, len(cal) // max(16, len(cal) // 4))]
        rest = np.setdiff1d(cal, cal_x)
        h_mid, h_ex, h_rest = submit(mid_rows, cal_x), submit(exact_rows, cal_x), submit(mid_rows, rest)     # the three calibration encodes side by side
        pm_x, _ = h_mid()
        n_mid += cal_x.size
        p32_x, a32_x = h_ex()
        n_exact += cal_x.size
        fin = np.isfinite(pm_x).all(axis=1)            # (a middle-tier overflow measures nothing either; the row is exact now anyway)
        if fin.any():
            dev[1] = deviation(pm_x[fin], p32_x[fin], abs_eps)
        eps[1] = bound(1)
        fin = np.isfinite(probs[cal_x]).all(axis=1)
        if fin.any():
            dev[0] = deviation(probs[cal_x[fin]], p32_x[fin], abs_eps)
        probs[cal_x], pred[cal_x], level[cal_x] = p32_x, a32_x, 2
        to_mid(rest, pending=h_rest)
    else:
        to_exact(cal)
    stats["calibration_rows"] = int(cal.size)
    stats["calibration_rows_exact"] = int((level[cal] == 2).sum())
    eps = [bound(0), bound(1)]
    per_round = []
    g = np.random.default_rng(1000003 * n + int(min(k, 1 << 30)))      # the audit's draw: a function of the problem only (identical on every rank)
    while True:
        rel = np.where(level == 2, np.float32(0), np.where(level == 1, np.float32(eps[1]), np.float32(eps[0]))).astype(np.float32)
        img, cls, amb = scan_bounded(probs, pred, ranks, rel, k, abs_eps, form)
        stats["scans"] += 1
        todo = np.flatnonzero(amb & (level < 2))
        moved = bound(0) > eps[0] or bound(1) > eps[1]
        if todo.size == 0 and not moved:
            # certified under the current bounds: audit rows that are still taken on trust
            pending = np.flatnonzero(level == 0)
            if audit <= 0 or pending.size == 0:
                break
            if stats["audits"] >= REFINE_MAX_AUDITS:      # every audit so far widened the bound: it cannot be trusted on this pool
                stats["escalated"] = True
                up(pending)
                per_round.append(int(pending.size))
                stats["rounds"] += 1
                eps = [max(eps[0], bound(0)), max(eps[1], bound(1))]
                continue
            in_board = np.zeros(n, dtype=bool)
            if k != K_ALL:
                in_board[np.asarray(img, dtype=np.int64)] = True
            members = pending[in_board[pending]]
            n_b = min(members.size, audit // 2)
            pick_b = g.choice(members, size=n_b, replace=False) if n_b else np.empty(0, np.int64)
            others = pending[~in_board[pending]] if n_b else pending
            n_o = min(others.size, audit - n_b)
            pick_o = g.choice(others, size=n_o, replace=False) if n_o else np.empty(0, np.int64)
            sample = np.unique(np.concatenate([pick_b, pick_o]).astype(np.int64))
            before = list(dev)
            dev[0] = dev[1] = 0.0
            h_mids = None
            if mid_rows is not None:                        # ... and a few rows the middle tier is trusted on go through the exact tower (beside the screen's sample:
                mids = np.flatnonzero(level == 1)           # drawn before it moves up, submitted first so that the two tiers run side by side)
                sample_mid = np.sort(g.choice(mids, size=min(mids.size, max(min(audit // 8, REFINE_AUDIT_MID_ROWS), 1)), replace=False)) if mids.size else mids
                h_mids = submit(exact_rows, sample_mid)
            up(sample)
            if mid_rows is not None:
                to_exact(sample_mid, pending=h_mids)
                stats["audit_mid_rows"] = stats.get("audit_mid_rows", 0) + int(sample_mid.size)
                stats["audit_max_deviation_mid"] = max(stats.get("audit_max_deviation_mid", 0.0), float(dev[1]))
            seen = list(dev)
            stats["audits"] += 1
            stats["audit_rows"] += int(sample.size)
            stats["audit_board_rows"] += int(n_b)
            stats["audit_max_deviation"] = max(stats["audit_max_deviation"], float(seen[0]))
            if seen[0] <= eps[0] and seen[1] <= eps[1]:
                dev[0], dev[1] = before                     # a hold-out check of the bounds, passed: they stay what the lists were certified under
                break
            # a row beyond the bound it was trusted to: the bound was understated -- widen it (safety x what was just seen) and scan again
            dev[0], dev[1] = max(before[0], seen[0]), max(before[1], seen[1])
            stats["audit_widened"] = True
            eps = [max(eps[0], bound(0)), max(eps[1], bound(1))]
            continue
        if stats["rounds"] >= max_rounds:
            raise RuntimeError(f"refine_scan: no fixed point after {max_rounds} rounds ({int((level > 0).sum())} of {n} rows refined)")
        if stats["rounds"] >= REFINE_ESCALATE_AFTER:
            # Heavily tied scores can keep a board in the reference's unsorted regime, where every comparison has to be certain and a
            # round only advances a few images in dataset order: stop trickling and move everything that is left up a tier.
            todo = np.flatnonzero(level < 2)
            stats["escalated"] = True
        up(todo)
        per_round.append(int(todo.size))
        stats["rounds"] += 1
        eps = [max(eps[0], bound(0)), max(eps[1], bound(1))]
    stats.update(rows_refined=int((level > 0).sum()), rows_mid=int(n_mid), rows_exact=int(n_exact), refined_per_round=per_round, eps=float(eps[0]),
                 eps_mid=float(eps[1]), max_deviation=float(dev[0]), max_deviation_mid=float(dev[1]), safety=float(safety), safety_mid=float(max(safety, REFINE_SAFETY_MID)),
                 unverified_rows=int((level == 0).sum()), observed_rows=int((level > 0).sum()), tiers=2 + (mid_rows is not None), abs_eps=float(abs_eps),
                 bound_form=form)
    return img, cls, stats


LAST_REFINE_STATS = None     # what the most recent identical_lists call did (rows re-encoded, rounds, bound): logged / reported by bench.py


def mode():
    """How pseudolabel passes compute their lists: "identical" (default: f16 screen + exact refinement, the lists of the fp32
    scan), "f16" (the f16 towers' lists as they are: boundary items may differ from the fp32 scan's), or "exact" is what a
    model loaded with clip.load(..., exact=True) does by itself.  $GRIP_PSEUDOLABEL_MODE."""
    import os
    m = os.environ.get("GRIP_PSEUDOLABEL_MODE", "identical")
    if m not in ("identical", "f16"):
        raise ValueError(f"GRIP_PSEUDOLABEL_MODE={m!r}: expected 'identical' or 'f16'")
    return m


SPLIT_TIER_MIN_ROWS = 4096      # pools below this go straight from the f16 screen to the f32 tower (the split twin costs HBM and a build)


def tier_streams():
    """HIP streams the re-encodes of a refinement tier alternate their chunks on ($GRIP_TIER_STREAMS, default 2 as for the pool encode: the split tower's
    bandwidth-bound kernels of one chunk run next to the GEMMs of the other, refine_split 0.81 -> 0.79 s per two passes; rows do not depend on it)."""
    return 1 if os.environ.get("GRIP_TIER_STREAMS", "2") == "1" else 2


def mid_tower(clip_model, n_rows):
    """The vision tower of `clip_model`'s split-f16 twin when the middle tier pays for a pool of `n_rows` rows, else None.
    $GRIP_SPLIT_TIER: "auto" (default: pools of >= SPLIT_TIER_MIN_ROWS rows), "1" always, "0" never."""
    import os
    want = os.environ.get("GRIP_SPLIT_TIER", "auto")
    if want == "0" or (want == "auto" and n_rows < SPLIT_TIER_MIN_ROWS) or not hasattr(clip_model, "split_twin"):
        return None
    if clip_model.dims.vision_width % 256:      # the split GEMM's 256 x 256 tiles (grip_tower_create refuses other widths at precision 2)
        return None
    try:
        twin = clip_model.split_twin()
    except engine.native.GripError as e:        # the tier is an optimisation: without it the screen's rows go straight to the f32 tower
        import logging
        logging.getLogger(__name__).warning("split-f16 middle tier unavailable (%s): refining with the f32 tower only", e)
        return None
    return None if twin is None else twin.visual.tower


def take_images(images, idx):
    """Rows `idx` (ascending int64 array) of an image pool: a tensor [N,3,R,R] or a lazy pool with .take(idx)."""
    if torch.is_tensor(images):
        return images[torch.as_tensor(idx, device=images.device)]
    return images.take(idx)


def take_prefix(prefix, idx):
    """The visual prompts of rows `idx` (ascending int64 array) of a pool, to go with take_images(images, idx): rows of a per-image prompt
    [N, P, d]; a shared prompt (None, [P, d], [1, P, d]) is every row's and comes back as it is."""
    if not engine.is_per_image_prefix(prefix):
        return prefix
    return prefix[torch.as_tensor(idx, device=prefix.device)]


def balanced_chunk(n_rows, chunk):
    """Rows per launch when `n_rows` rows go through a tower at most `chunk` at a time: the smallest size that keeps the number of launches
    (1 024 audit rows at 880 -> 2 x 512, not 880 + 144: the tail launch left the 256 x 256 GEMM tiles of the refinement towers a chip's worth of
    workgroups short).  Rows do not depend on the chunking."""
    parts = max(1, -(-int(n_rows) // max(1, int(chunk))))
    return max(1, -(-int(n_rows) // parts))


def tier_rows(tower, fetch, txt, scale, n, lo, hi, chunk, prefix=None, argmax_on="probs", on_rows=None, timer=None, deep=None, cache=None, paths=None,
              on_cached=None):
    """A refinement tier as refine_scan's callback: rows(idx) -> (probs [len(idx), C], arg-max) of the global rows `idx` (ascending) re-encoded by `tower`.
    Each rank encodes the rows of its own shard [lo, hi) -- `fetch(global_rows)` returns their images -- and one padded all-gather assembles the rest.
    prefix: None, a shared visual prompt, or per-image prompts [n, P, d] aligned with the pool (the rows' own prompts go with them: take_prefix).
    deep: None or the shared prompt's deep prompts [D, P, d] (every row alike).
    rows.submit(idx) only ENQUEUES the work, on the tier's own HIP stream, and returns the function that waits for it: two tiers submitted back to back
    (refine_scan does that wherever their row sets are independent) share the GPU instead of taking turns at small-batch efficiency.
    cache + paths (given explicitly, prompt-free tiers only): a PoolFeatureCache and the pool's path tuple.  Rows of `idx` the tower has encoded in an
    earlier pass come from the cache; each rank encodes only the MISSING rows of its shard, one all-gather runs over the missing rows (none when
    nothing is missing: the cache's content is the same on every rank, so every rank computes the same miss set), the head runs over the assembled
    rows in `idx` order and the missing rows are written back.  on_rows then counts the rows actually encoded, on_cached(m) the rows served."""
    dev = tower.device
    side = torch.cuda.Stream(device=dev)
    cache = use_cache(cache, prefix, deep) if cache is not None and paths is not None else None

    def submit(idx):
        import time
        t0 = time.perf_counter()
        need = idx if cache is None else cache.missing_rows(paths, tower, idx)
        mine = need[(need >= lo) & (need < hi)]
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            local = torch.empty(len(mine), tower.embed_dim, dtype=torch.float32, device=dev)
            if len(mine):
                tower.encode_chunks(lambda a, b: fetch(mine[a:b]), local, 0, len(mine), balanced_chunk(len(mine), chunk), take_prefix(prefix, mine),
                                    streams=tier_streams(), deep=deep)
            if on_rows is not None:
                on_rows(len(mine))
            if cache is None:
                got = gdist.allgather_selected(local, idx, n, tag="refined_rows")
            else:
                if on_cached is not None:
                    on_cached(len(idx) - len(need))
                got = gdist.allgather_selected(local, need, n, tag="refined_rows") if len(need) else local
                # the table is written and read on this tier's stream only, and every submit is waited for (result) before the pass ends: a later
                # pass's stream starts behind it.  A table over budget is never created: nothing was cached then, `need` is `idx`, `got` is complete
                if cache.store_rows(paths, tower, need, got, n):
                    got = cache.rows(paths, tower, idx)
            _, p, al, ap = engine.cosine_head(got, txt, scale)
            am = ap if argmax_on == "probs" else al
        if timer is not None:
            timer(time.perf_counter() - t0)

        def result():
            t1 = time.perf_counter()
            side.synchronize()
            out = p.cpu().numpy(), am.cpu().numpy()
            if timer is not None:
                timer(time.perf_counter() - t1)
            return out
        return result

    def rows(idx):
        return submit(idx)()
    rows.submit = submit
    return rows


@torch.no_grad()
def identical_lists(visual16, visual32, images, txt_exact, scale, paths, class_labels, k, chunk=880, exact_chunk=880, prefix=None,
                    argmax_on="probs", streams=2, emb16=None, visual_mid=None, mid_chunk=880, deep=None, cache=None):
    """(filepaths, labels) of the reference's fp32 pseudolabel scan (utils/clip_pseudolabels.py:24-112) at close to the f16
    towers' throughput: the whole pool goes through the f16 vision tower `visual16` (sharded over ranks, one all-gather), the
    head scores it against the EXACT text features `txt_exact`, and refine_scan re-encodes only the rows whose probabilities cannot
    decide a comparison the lists depend on -- with the split-f16 tower `visual_mid` (precision 2) where there is one, and with the
    f32 tower `visual32` what that tier cannot decide either (each rank re-encodes the marked rows of its own shard; one small
    all-gather per round and tier).  The lists are the exact mode's lists provided every row obeys the measured bound of the tier it
    was left at; the bound is calibrated on this pool, audited on a hold-out sample after certification and reported in
    LAST_REFINE_STATS (asserted equal to the exact mode at N = 50 000 in tests/test_gpu_identical.py).  prefix: None, one visual prompt for
    the pool, or one per image ([N, P, d]): every tier encodes a row with its own prompt.  deep: None or [D, P, d] deep prompts of a shared
    prompt, given to the screen and to every tier alike.
    cache: a PoolFeatureCache (or one installed by pool_cache) for prompt-free passes: the screen's embeddings come from it when it holds them in
    ANY stream form (the lists do not depend on the screen's stream; `images` is then never read for the screen and nothing is gathered), and every
    tier re-encodes only rows it has not encoded in an earlier pass over these `paths` (tier_rows).  refine_scan asks for the same rows and gets the
    same bits either way: lists, marks and bounds are those of the uncached pass.  LAST_REFINE_STATS: `screen_cached`, `rows_cached_mid` /
    `rows_cached_exact` (rows the tiers were asked for and did not encode); rows_*_this_rank count rows actually encoded."""
    global LAST_REFINE_STATS
    n = len(paths)
    if n == 0:
        _, _, LAST_REFINE_STATS = refine_scan(np.empty((0, max(len(class_labels), 1)), np.float32), np.empty(0, np.int32), np.empty(0, np.int64), k, None)
        LAST_REFINE_STATS.update(rows_refined_this_rank=0, rows_cached_mid=0, rows_cached_exact=0, screen_cached=False)
        return [], []
    cache = use_cache(cache, prefix, deep)
    pool = tuple(paths) if cache is not None else None
    key = (id(visual16), n, len(class_labels))        # the pool as far as the screen's choice of stream goes (same tower, same size, same class count)
    hit = cache.screen(pool, visual16) if cache is not None and emb16 is None else None
    stream = screen_stream(key) if emb16 is None and hit is None else None       # (a cached screen, like a given one, makes no stream choice)
    if hit is not None:
        emb = hit[0]
    else:
        emb = emb16 if emb16 is not None else encode_pool(visual16, images, chunk=chunk, prefix=prefix, screen=stream, deep=deep, cache=cache, paths=pool)
    dev = emb.device
    _, probs, am_l, am_p = engine.cosine_head(emb, txt_exact, scale)
    probs_h = probs.cpu().numpy()
    pred_h = (am_p if argmax_on == "probs" else am_l).cpu().numpy()
    lo, hi, _ = gdist.shard_range(n)
    encoded = {"exact": 0, "mid": 0}
    served = {"exact": 0, "mid": 0}

    def rows_through(tower, tier, tier_chunk):
        def count(m):
            encoded[tier] += m

        def count_cached(m):
            served[tier] += m
        return tier_rows(tower, lambda rows: take_images(images, rows), txt_exact, scale, n, lo, hi, tier_chunk, prefix, argmax_on, on_rows=count, deep=deep,
                         cache=cache, paths=pool, on_cached=count_cached)

    img, cls, stats = refine_scan(probs_h, pred_h, path_ranks(paths), k, rows_through(visual32, "exact", exact_chunk),
                                  mid_rows=rows_through(visual_mid, "mid", mid_chunk) if visual_mid is not None else None)
    stats["rows_refined_this_rank"] = encoded["exact"] + encoded["mid"]
    stats["rows_exact_this_rank"], stats["rows_mid_this_rank"] = encoded["exact"], encoded["mid"]
    stats["rows_cached_exact"], stats["rows_cached_mid"], stats["screen_cached"] = served["exact"], served["mid"], hit is not None
    if stream is not None:
        note_screen_bound(key, stream, stats)
    elif hit is not None:
        stats["screen_stream"] = hit[1]           # the form the cached screen was encoded in
    LAST_REFINE_STATS = stats
    return [paths[i] for i in img], [class_labels[int(c)] for c in cls]


# ------------------------------------------------------------------------------------------ transductive label propagation over the pool
class _PoolGraph:
    """The kNN graph of a pool for the transductive passes (LabelPropagation, TransductiveGMM): built per pass, or kept per pool.
    keep_graphs: keep (idx, sim) per pool, keyed by the ordered paths like PoolFeatureCache -- for callers whose image tower is frozen and
    prompt-free (the textual strategies: the graph is an invariant of the run); a caller whose features move builds it every pass (the default)."""

    def __init__(self, k, keep_graphs=False):
        self.k = int(k)
        if not 1 <= self.k <= engine.KNN_MAX_K:
            raise ValueError(f"{type(self).__name__}: k = {k} (1 .. {engine.KNN_MAX_K})")
        self.keep_graphs = bool(keep_graphs)
        self._graphs = []           # [(path tuple, fingerprint of the embeddings, idx, sim)], most recently used first
        self.graphs_built = 0

    def graph(self, img_emb, paths=None):
        """(idx, sim) of the pool's kNN graph (min(k, N - 1) neighbours): built, or the kept one of this ordered pool.  The paths name the images,
        not the features: a kept graph is handed out only while the embeddings' fingerprint (two float64 sums: one small reduction and one
        host read per pass) is the one it was built from, so other features behind the same paths -- another tower, a prompt, an adapter -- rebuild
        it instead of meeting a stale graph."""
        n = img_emb.shape[0]
        key = mark = None
        if self.keep_graphs and paths is not None:
            key = paths if isinstance(paths, tuple) else tuple(paths)
            ramp = torch.arange(1, n + 1, dtype=torch.float64, device=img_emb.device)      # (position-weighted: a permutation of the rows moves it)
            mark = (tuple(img_emb.shape), str(img_emb.device),
                    *torch.stack([img_emb.sum(dtype=torch.float64), torch.dot(img_emb.sum(dim=1, dtype=torch.float64), ramp)]).tolist())
            for i, (p, held, idx, sim) in enumerate(self._graphs):
                if len(p) == len(key) and p == key:
                    if held != mark:
                        del self._graphs[i]         # the same pool with other features: the graph is rebuilt below
                        break
                    if i:
                        self._graphs.insert(0, self._graphs.pop(i))
                    return idx, sim
        idx, sim = engine.knn_graph(img_emb, k=min(self.k, n - 1))
        self.graphs_built += 1
        if key is not None:
            self._graphs.insert(0, (key, mark, idx, sim))
            del self._graphs[4:]
        return idx, sim

    def clear(self):
        self._graphs.clear()


class LabelPropagation(_PoolGraph):
    """Settings of the transductive pseudolabel pass (off unless installed by label_propagation()): the head's probabilities of the whole pool are
    propagated over the pool's own kNN graph before the leaderboard scan -- images that lie together in the embedding space mostly share a class
    (Zhu & Ghahramani 2002; Zhou et al. 2004; ZLaP, CVPR 2024).  k neighbours per image (cosine of the embeddings), edge weights
    softmax(gamma * cosine) per row, `iters` steps of Z <- (1 - alpha) P + alpha W Z (engine.knn_graph / engine.label_propagate: a random walk on the
    directed graph, not ZLaP's symmetrised solve).  The defaults are untuned.  keep_graphs: see _PoolGraph."""
    infix = "lp_"       # of the pseudolabel pickle's name (utils.clip_pseudolabels.pseudolabel_top_k)

    def __init__(self, k=16, alpha=0.8, gamma=10.0, iters=10, keep_graphs=False):
        super().__init__(k, keep_graphs)
        self.alpha, self.gamma, self.iters = float(alpha), float(gamma), int(iters)
        if not 0.0 <= self.alpha < 1.0:
            raise ValueError(f"LabelPropagation: alpha = {alpha} (0 <= alpha < 1)")
        if not 0.0 <= self.gamma < float("inf"):
            raise ValueError(f"LabelPropagation: gamma = {gamma} (a finite gamma >= 0)")
        if self.iters < 1:
            raise ValueError(f"LabelPropagation: iters = {iters} (at least 1)")

    def transduce(self, img_emb, probs, paths=None):
        """(Z, pred) of the pool: the propagated probabilities and their first arg-max."""
        idx, sim = self.graph(img_emb, paths)
        return engine.label_propagate(probs, idx, sim, self.alpha, self.gamma, self.iters)

    def __repr__(self):
        return f"LabelPropagation(k={self.k}, alpha={self.alpha}, gamma={self.gamma}, iters={self.iters})"


class TransductiveGMM(_PoolGraph):
    """Settings of the transductive GMM pseudolabel pass (off unless installed by label_propagation()), after TransCLIP-ZS (Zanella, Gerin, Ben Ayed,
    NeurIPS 2024): one Gaussian per class with a shared diagonal covariance is fitted to the pool's unit image embeddings, the assignments Z are
    anchored to the head's probabilities P by a KL term of weight `lam` and smoothed over the pool's directed kNN graph (k neighbours, affinity
    max(0, cosine)); `iters` rounds of an M-step and an E-step of `z_iters` sweeps from Z = P (engine.gmm_transduce).  NOT TransCLIP's code: the first
    centres come from an M-step on P instead of the top-8 confident samples, the graph is directed, there is no few-shot term.  The defaults are
    untuned.  After a pass `state` holds the last (mean, var): they can score images that were not in the pool.  keep_graphs: see _PoolGraph."""
    infix = "gmm_"      # of the pseudolabel pickle's name

    def __init__(self, k=3, lam=1.0, iters=10, z_iters=5, var_floor=1e-8, keep_graphs=False):
        super().__init__(k, keep_graphs)
        self.lam, self.iters, self.z_iters, self.var_floor = float(lam), int(iters), int(z_iters), float(var_floor)
        if not 0.0 <= self.lam < float("inf"):
            raise ValueError(f"TransductiveGMM: lam = {lam} (a finite lam >= 0)")
        if self.iters < 1:
            raise ValueError(f"TransductiveGMM: iters = {iters} (at least 1)")
        if self.z_iters < 1:
            raise ValueError(f"TransductiveGMM: z_iters = {z_iters} (at least 1)")
        if not 0.0 < self.var_floor < float("inf"):
            raise ValueError(f"TransductiveGMM: var_floor = {var_floor} (a finite var_floor > 0)")
        self.state = None           # (mean [c, e], var [e]) of the most recent pass

    def transduce(self, img_emb, probs, paths=None):
        """(Z, pred) of the pool: the assignments of the recursion and their first arg-max; keeps (mean, var) in `state`."""
        idx, sim = self.graph(img_emb, paths)
        z, pred, mean, var, _ = engine.gmm_transduce(img_emb, probs, idx, sim, self.lam, self.iters, self.z_iters, self.var_floor)
        self.state = (mean, var)
        return z, pred

    def __repr__(self):
        return f"TransductiveGMM(k={self.k}, lam={self.lam}, iters={self.iters}, z_iters={self.z_iters}, var_floor={self.var_floor})"


class BalancedAssignment:
    """Settings of the balanced pseudolabel pass (off unless installed by label_propagation()): the pool's [n, c] probabilities are treated as an
    optimal-transport problem -- every row sums to one, every class receives the share `prior` gives it (None: the same share) -- and `iters`
    Sinkhorn-Knopp iterations are run on probs ** tau (engine.sinkhorn_balance; Cuturi 2013; SeLa, Asano et al. 2020; SwAV, Caron et al. 2020).  The
    leaderboard scan then ranks by the balanced Q and its arg-max, so a class the head is biased against is filled with the rows that lean towards it
    most instead of with other classes' overflow.  No epsilon-scaled cost, no stopping rule: `iters` is how hard the balance is pressed.  inner: None,
    a LabelPropagation or a TransductiveGMM whose Z is balanced instead of the head's probabilities.  prior: None or c finite positive weights (a list
    or a tensor).  The defaults are untuned.  After a pass `state` holds the last (mass [c], log_scale [c])."""

    def __init__(self, tau=1.0, iters=3, prior=None, inner=None):
        self.tau, self.iters = float(tau), int(iters)
        if not 0.0 < self.tau < float("inf"):
            raise ValueError(f"BalancedAssignment: tau = {tau} (a finite tau > 0)")
        if self.iters < 0:
            raise ValueError(f"BalancedAssignment: iters = {iters} (at least 0)")
        if prior is not None:
            prior = torch.as_tensor(prior, dtype=torch.float64).detach().cpu()
            if prior.dim() != 1 or prior.numel() < 1 or not bool((torch.isfinite(prior) & (prior > 0)).all()):
                raise ValueError(f"BalancedAssignment: prior must be a list of finite positive weights, one per class, got {prior.tolist()}")
        self.prior = prior
        if inner is not None and not isinstance(inner, (LabelPropagation, TransductiveGMM)):
            raise ValueError(f"BalancedAssignment: inner must be a LabelPropagation, a TransductiveGMM or None, got {type(inner).__name__}")
        self.inner = inner
        self.infix = "ot_" + (inner.infix if inner is not None else "")       # of the pseudolabel pickle's name: ot_, ot_lp_, ot_gmm_
        self.state = None           # (mass [c], log_scale [c]) of the most recent pass

    def transduce(self, img_emb, probs, paths=None):
        """(Q, pred) of the pool: the balanced assignment of inner's Z (of probs without an inner) and its first arg-max."""
        z = probs if self.inner is None else self.inner.transduce(img_emb, probs, paths)[0]
        if self.prior is not None and self.prior.numel() != z.shape[1]:
            raise ValueError(f"BalancedAssignment: a prior of {self.prior.numel()} weights for {z.shape[1]} classes")
        q, pred, mass, log_scale = engine.sinkhorn_balance(z, self.tau, self.iters, self.prior)
        self.state = (mass, log_scale)
        return q, pred

    def __repr__(self):
        return f"BalancedAssignment(tau={self.tau}, iters={self.iters}, prior={'None' if self.prior is None else 'given'}, inner={self.inner})"


_PROPAGATION = []   # settings installed by label_propagation(), innermost last.  Empty unless a caller opened one: every pass is per-image by default


@contextlib.contextmanager
def label_propagation(lp):
    """Install `lp` (a LabelPropagation, a TransductiveGMM or a BalancedAssignment, or None: no-op) for the pseudolabel passes underneath -- how it
    reaches the reference-named compute_pseudo_labels / pseudolabel_top_k, whose signatures are the reference's.  While one is installed
    pseudolabel_from_features transduces with it, the callers that would pick identical_lists take their plain branch (no reference list can be identical
    to a transduced one) and pseudolabel_top_k names its pickle after the object's `infix`: `..._pseudolabels_lp_split_...` /
    `..._pseudolabels_gmm_split_...` / `..._pseudolabels_ot_split_...` (`ot_lp_`, `ot_gmm_` with an inner transduction)."""
    if lp is None:
        yield None
        return
    if not isinstance(lp, (LabelPropagation, TransductiveGMM, BalancedAssignment)):
        raise TypeError(f"label_propagation: expected a LabelPropagation, a TransductiveGMM, a BalancedAssignment or None, got {type(lp).__name__}")
    _PROPAGATION.append(lp)
    try:
        yield lp
    finally:
        _PROPAGATION.pop()


def propagation():
    """The innermost installed LabelPropagation / TransductiveGMM / BalancedAssignment, or None."""
    return _PROPAGATION[-1] if _PROPAGATION else None


# ------------------------------------------------------------------------------------------ from the pass to the step: the matrix behind the lists
class _PoolRowStore:
    """The name / column bookkeeping SoftTargetStore and CandidateStore share: a device buffer `matrix` with one row per pool image that the store OWNS
    (the first record copies into it, every later one of the same shape, dtype and device overwrites it in place), the pool row of every BASE name and
    the column map of a training class list."""
    _dtype, _what, _keyed = torch.float32, "matrix", "soft targets"

    def __init__(self):
        self.matrix = None          # [n, columns] on the device, or None before the first pass
        self.class_labels = ()      # the label id of every class the pass ranked
        self.records = 0
        self._row_of = {}           # base name -> pool row, or -2 for a base name that occurs twice
        self._col_maps = {}         # tuple(training label ids) -> int32 [cz] device tensor (one tensor per list: a fixed address, checked once)

    def _columns(self, n_classes):
        return n_classes

    def record(self, paths, class_labels, z):
        name = str(self._dtype).replace("torch.", "")
        if not torch.is_tensor(z) or z.dim() != 2 or z.dtype != self._dtype or tuple(z.shape) != (len(paths), self._columns(len(class_labels))):
            raise ValueError(f"{type(self).__name__}.record: a {name} [{len(paths)}, {self._columns(len(class_labels))}] {self._what} was expected, got "
                             f"{getattr(z, 'shape', type(z))} {getattr(z, 'dtype', None)}")
        z = z.detach()
        if self.matrix is not None and self.matrix.shape == z.shape and self.matrix.device == z.device:
            self.matrix.copy_(z)
        else:
            self.matrix = z.clone(memory_format=torch.contiguous_format)
        labels = tuple(int(c) for c in class_labels)
        if labels != self.class_labels:
            self.class_labels = labels
            self._col_maps.clear()
        self._row_of = {}
        for i, p in enumerate(paths):
            name = p.split("/")[-1]
            self._row_of[name] = -2 if name in self._row_of else i
        self.records += 1

    def forget(self):
        """No name is in the pool any more (every row asked about is a hard row); the buffer stays where it is."""
        self._row_of = {}

    def rows(self, names, hard=None):
        """int32 [len(names)] on the matrix's device.  hard: optional list of flags, True = do not ask about this name (its row is -1: a labelled row
        of the batch, whatever it is called)."""
        if self.matrix is None:
            raise ValueError(f"{type(self).__name__}.rows: no pass has recorded a {self._what} yet")
        out = []
        for i, n in enumerate(names):
            if hard is not None and hard[i]:
                out.append(-1)
                continue
            r = self._row_of.get(n.split("/")[-1], -1)
            if r == -2:
                raise ValueError(f"{type(self).__name__}: the base name {n.split('/')[-1]!r} names two rows of the pool: {self._keyed} are keyed by base names, "
                                 "as the strategies' check_unlabeled is")
            out.append(r)
        return torch.tensor(out, dtype=torch.int32).to(self.matrix.device, non_blocking=True)

    def col_map(self, class_ids):
        if self.matrix is None:
            raise ValueError(f"{type(self).__name__}.col_map: no pass has recorded a {self._what} yet")
        key = tuple(int(c) for c in class_ids)
        if key not in self._col_maps:
            at = {c: i for i, c in enumerate(key)}
            missing = [c for c in self.class_labels if c not in at]
            if missing or len(at) != len(key):
                raise ValueError(f"{type(self).__name__}.col_map: the pass ranked classes {missing} that the training class list {list(key)} does not hold "
                                 "(or that list repeats a class)")
            self._col_maps[key] = torch.tensor([at[c] for c in self.class_labels], dtype=torch.int32, device=self.matrix.device)
        return self._col_maps[key]


class SoftTargetStore(_PoolRowStore):
    """Keeps the device matrix a transduced pseudolabel pass ranked (Z of LabelPropagation / TransductiveGMM, Q of BalancedAssignment) so that the
    prompt steps can train on the ROW behind a pseudolabel instead of its arg-max (engine.soft_ce; off unless installed by soft_targets()).
    record() is called by pseudolabel_from_features; the steps ask for
      rows(names)         the matrix row of every file name of a batch (int32 on the matrix's device), -1 for a name that is not in the pool.  Names are
                          BASE names: the dataset hands those out and the strategies' check_unlabeled is keyed by them; a base name that names two pool
                          rows raises when it is asked about;
      col_map(class_ids)  int32 [cz]: the position, in a step's training class list (label ids), of every class the pass ranked -- TRZSL ranks over
                          the unseen classes and trains over all of them.
    The store OWNS its buffer: the first record() copies the matrix into it and every later one of the same shape and device overwrites it in place,
    so the address a captured graph read the matrix from stays valid and the next replay trains on the new pass (steps.GraphedStep).  Another shape
    allocates another buffer (a graphed step sees its key move and runs eagerly until it is rebuilt).  Multi-rank runs need nothing: every rank
    ranks the same gathered pool."""


class CandidateStore(_PoolRowStore):
    """Keeps the candidate SETS of the last pseudolabel pass (engine.candidate_select's mask, int32 [n, ceil(cz / 32)] on the device; `mask` names the
    buffer) so that the prompt steps can train on the set behind a pseudolabel with the partial-label loss (engine.candidate_ce; off unless installed by
    candidate_sets()).  SoftTargetStore's contract: it owns its buffer, a later pass of the same shape lands at the same address -- a captured graph
    trains on the new sets -- rows(names, hard=) gives the mask row of every base name (-1: not in the pool, or a labelled row; a duplicated base name
    raises when asked about) and col_map(class_ids) the position, in a step's training class list, of every class the pass ranked."""
    _dtype, _what, _keyed = torch.int32, "mask", "candidate sets"

    def _columns(self, n_classes):
        return (n_classes + 31) // 32

    @property
    def mask(self):
        return self.matrix


_SOFT_STORES = []   # stores installed by soft_targets(), innermost last.  Empty unless a caller opened one: no pass records anything by default


@contextlib.contextmanager
def soft_targets(store):
    """Install `store` (a SoftTargetStore, or None: no-op) for the pseudolabel passes underneath, as pool_cache() and label_propagation() install
    theirs.  While one is installed pseudolabel_from_features records the matrix of every transduced pass in it, and pseudolabel_top_k does not read an
    existing pickle (a loaded list has no matrix behind it): the pass runs and rewrites the same file."""
    if store is None:
        yield None
        return
    if not isinstance(store, SoftTargetStore):
        raise TypeError(f"soft_targets: expected a SoftTargetStore or None, got {type(store).__name__}")
    _SOFT_STORES.append(store)
    try:
        yield store
    finally:
        _SOFT_STORES.pop()


def soft_target_store():
    """The innermost installed SoftTargetStore, or None."""
    return _SOFT_STORES[-1] if _SOFT_STORES else None


class CandidateSelection:
    """Settings of the candidate-set pseudolabel pass (off unless installed by candidate_sets(); Candidate Pseudolabel Learning, Zhang et al., ICML 2024):
    every pool image keeps a SET of classes (engine.candidate_select) -- the smallest prefix of its top classes whose running confidence reaches `tau`
    (intra-instance), joined by `combine` ("intersection", "union", "intra", "inter") with the classes that claim it among their most confident rows of
    the WHOLE matrix (inter-instance).  slots: how many boards' worth of rows a class claims -- a pass with k pseudo-shots per class uses
    claim = min(n, slots k), so GRIP's growing k grows the coverage with no schedule of its own.  The defaults are untuned."""
    infix = "cpl_"      # of the pseudolabel pickle's name, in front of lp_ / gmm_ / ot_...

    def __init__(self, tau=0.99, slots=2, combine="intersection"):
        self.tau, self.combine = float(tau), combine
        if not 0.0 < self.tau <= 1.0:
            raise ValueError(f"CandidateSelection: tau = {tau} (0 < tau <= 1)")
        if isinstance(slots, bool) or int(slots) != slots or int(slots) < 1:
            raise ValueError(f"CandidateSelection: slots = {slots!r} (an integer >= 1)")
        self.slots = int(slots)
        if combine not in engine.CANDIDATE_COMBINE:
            raise ValueError(f"CandidateSelection: combine = {combine!r} (one of {sorted(engine.CANDIDATE_COMBINE)})")
        self.state = None           # (count [n], threshold [cz]) of the most recent pass

    def claim(self, n, k):
        return n if k == K_ALL else max(1, min(n, self.slots * int(k)))

    def select(self, matrix, paths, class_labels, k, store):
        """(filepaths, labels) of a pass over `matrix` [n, cz]: every pool row with a non-empty set, in pool order, each once, with the member of highest
        rank as its (hard) label; the sets go to `store`."""
        mask, count, label, threshold = engine.candidate_select(matrix, self.claim(matrix.shape[0], k), self.tau, self.combine)
        store.record(paths, class_labels, mask)
        self.state = (count, threshold)
        lab = label.cpu().tolist()
        keep = [i for i, c in enumerate(lab) if c >= 0]
        return [paths[i] for i in keep], [class_labels[lab[i]] for i in keep]

    def __repr__(self):
        return f"CandidateSelection(tau={self.tau}, slots={self.slots}, combine={self.combine!r})"


_CANDIDATES = []    # (selection, store) installed by candidate_sets(), innermost last.  Empty unless a caller opened one


@contextlib.contextmanager
def candidate_sets(selection, store):
    """Install a CandidateSelection and the CandidateStore that receives its sets (or None, None: no-op) for the pseudolabel passes underneath, as
    label_propagation() and soft_targets() install theirs.  While one is installed pseudolabel_from_features runs the selection instead of the
    leaderboard scan -- on the matrix it would have ranked: Z / Q of an installed transduction, else the head's probabilities -- the callers that would
    pick identical_lists take their plain branch, and pseudolabel_top_k names its pickle `..._pseudolabels_cpl_split_...` (`cpl_lp_`, `cpl_gmm_`,
    `cpl_ot_...` with a transduction) and does not read an existing one (a loaded list has no sets behind it)."""
    if selection is None and store is None:
        yield None
        return
    if not isinstance(selection, CandidateSelection) or not isinstance(store, CandidateStore):
        raise TypeError(f"candidate_sets: expected a CandidateSelection and a CandidateStore (or None, None), got {type(selection).__name__} and "
                        f"{type(store).__name__}")
    _CANDIDATES.append((selection, store))
    try:
        yield store
    finally:
        _CANDIDATES.pop()


def candidates():
    """The innermost installed (CandidateSelection, CandidateStore), or None."""
    return _CANDIDATES[-1] if _CANDIDATES else None


def view_boxes(sampler, views, names, H, W):
    """int32 [len(names) * views, 5] of (top, left, height, width, flip), image-major: view 0 of every image is the whole image, un-flipped; view p >= 1 is
    the box `sampler` (an augment.ViewSampler) draws for (seed, base name, epoch 0, view p) -- an item's boxes depend on its name alone, not on its batch
    or the rank.  Shared by MultiView and tpt.TestTimeTuner."""
    out = np.empty((len(names), views, 5), dtype=np.int32)
    out[:, 0] = (0, 0, H, W, 0)
    for i, name in enumerate(names):
        base = os.path.basename(str(name))
        for p in range(1, views):
            out[i, p] = sampler.box(base, 0, H, W, view=p)
    return out.reshape(-1, 5)


def make_views(sampler, views, images, names):
    """images [B, 3, H, H] f32 on the GPU -> their views [B * views, 3, H, H] of view_boxes, image-major (view 0 is a bit-exact copy)."""
    from . import augment
    B, _, H, W = images.shape
    return augment.views(images, view_boxes(sampler, views, names, H, W), rows=np.repeat(np.arange(B, dtype=np.int64), views), n_px=H)


class MultiView:
    """Settings of the multi-view pseudolabel pass (off unless installed by multi_view(); after MTA, Zanella & Ben Ayed, CVPR 2024 -- the model of
    include/grip_amd.h, not the paper's code): every pool image is encoded `views` times -- view 0 the image as it is, views 1 .. V - 1 boxes of an
    augment.ViewSampler(seed, scale, ratio, flip) under the image's base name with the EPOCH FIXED AT 0, so a pool's views are the same in every pass
    and on every rank -- and the feature row the pass hands on is the inlier-weighted mean-shift mode of the image's view embeddings
    (engine.view_mode; the affinity of two views is the dot product of their class probabilities under the pass's text features).  The result is one
    [n, e] matrix, not normalised, that pseudolabel_from_features and everything behind it consume unchanged.  The cost is V tower forwards per image.
    rho, lam, lam_y are the paper's values; outer, inner and h2_floor are untuned.
    keep_bytes > 0 (textual strategies: the image tower is frozen): the [n, V, e] view embeddings of a pool are kept, keyed by its ordered paths, when
    they fit, and the next pass over the same pool encodes nothing.  `encodes` counts the pools actually encoded."""
    infix = "mv_"       # of the pseudolabel pickle's name, between cpl_ and lp_ / gmm_ / ot_...

    def __init__(self, views=16, scale=(0.5, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip=0.5, seed=0, rho=0.3, lam=4.0, lam_y=0.2, h2_floor=2.0 ** -20,
                 outer=5, inner=3, keep_bytes=0):
        from .augment import ViewSampler
        if isinstance(views, bool) or not isinstance(views, int) or not 2 <= views <= engine.VIEW_MODE_MAX_VIEWS:
            raise ValueError(f"MultiView: views = {views!r} (an integer in 2 .. {engine.VIEW_MODE_MAX_VIEWS})")
        self.views = views
        self.sampler = ViewSampler(seed=seed, scale=scale, ratio=ratio, flip=flip)       # (raises on a bad scale / ratio / flip)
        self.rho, self.lam, self.lam_y, self.h2_floor = float(rho), float(lam), float(lam_y), float(h2_floor)
        if not (0.0 < self.rho <= 1.0 and 0.0 <= self.lam < math.inf and 0.0 < self.lam_y < math.inf and 0.0 < self.h2_floor < math.inf):
            raise ValueError(f"MultiView: rho = {rho}, lam = {lam}, lam_y = {lam_y}, h2_floor = {h2_floor} (0 < rho <= 1, lam >= 0, lam_y > 0, "
                             f"h2_floor > 0, all finite)")
        for name, val in (("outer", outer), ("inner", inner)):
            if isinstance(val, bool) or not isinstance(val, int) or val < 0:
                raise ValueError(f"MultiView: {name} = {val!r} (an integer >= 0)")
        self.outer, self.inner = outer, inner
        self.keep_bytes = int(keep_bytes)
        self._kept = None       # (tuple(paths), tower, [n, V, e]) of the most recent pool that fitted
        self.encodes = 0
        self.last_y = None      # [n, V] view weights of the most recent aggregate (diagnostics)

    def boxes(self, names, H, W):
        """int32 [len(names) * V, 5] of (top, left, height, width, flip), image-major: view 0 of every image is the whole image, un-flipped; view p >= 1
        is the sampler's box of (seed, base name, epoch 0, view p)."""
        return view_boxes(self.sampler, self.views, names, H, W)

    def make_views(self, images, names):
        """images [B, 3, H, H] f32 on the GPU -> their views [B * V, 3, H, H], image-major (view 0 is a bit-exact copy)."""
        return make_views(self.sampler, self.views, images, names)

    @torch.no_grad()
    def encode_views(self, tower, images, paths, chunk=880, prefix=None, deep=None):
        """[n, V, e] f32: the view embeddings of an ordered pool (`images` as encode_pool takes it), max(1, chunk // V) images at a time, so a chunk of
        views is no larger than a chunk of images is today.  Every chunk of views goes through encode_pool WITHOUT a cache key (a view is not the pool
        image the PoolFeatureCache knows); what encode_pool does under torch.distributed is inherited."""
        n = images.shape[0] if torch.is_tensor(images) else images.n
        if len(paths) != n:
            raise ValueError(f"{len(paths)} paths for a pool of {n} images")
        key = tuple(paths)
        if prefix is None and deep is None and self._kept is not None and self._kept[0] == key and self._kept[1] is tower:
            return self._kept[2]
        V, dev = self.views, tower.device
        out = torch.empty(n, V, tower.embed_dim, dtype=torch.float32, device=dev)
        step = max(1, int(chunk) // V)
        per_image = engine.is_per_image_prefix(prefix)
        if hasattr(images, "plan"):
            images.plan(0, n, step)
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            x = (images[lo:hi] if torch.is_tensor(images) else images(lo, hi)).to(dev, torch.float32).contiguous()
            vw = self.make_views(x, paths[lo:hi])
            pf = prefix[lo:hi].repeat_interleave(V, dim=0) if per_image else prefix
            out[lo:hi] = encode_pool(tower, vw, chunk=chunk, prefix=pf, deep=deep).view(hi - lo, V, -1)
        self.encodes += 1
        if prefix is None and deep is None and 0 < _nbytes(out) <= self.keep_bytes:
            self._kept = (key, tower, out)
        return out

    @torch.no_grad()
    def aggregate(self, view_emb, txt, scale):
        """[n, e] modes of the [n, V, e] view embeddings: engine.cosine_head on the n V rows for the views' class probabilities, then engine.view_mode."""
        n, V, e = view_emb.shape
        _, probs, _, _ = engine.cosine_head(view_emb.reshape(n * V, e), txt, scale)
        mode, self.last_y = engine.view_mode(view_emb, probs.view(n, V, -1), rho=self.rho, lam=self.lam, lam_y=self.lam_y, h2_floor=self.h2_floor,
                                             outer=self.outer, inner=self.inner)
        return mode

    def features(self, tower, images, paths, txt, scale, chunk=880, prefix=None, deep=None):
        """encode_views + aggregate: what a pass hands to pseudolabel_from_features in place of encode_pool's rows."""
        return self.aggregate(self.encode_views(tower, images, paths, chunk=chunk, prefix=prefix, deep=deep), txt, scale)

    def __repr__(self):
        return (f"MultiView(views={self.views}, scale={self.sampler.scale}, ratio={self.sampler.ratio}, flip={self.sampler.flip}, seed={self.sampler.seed}, "
                f"rho={self.rho}, lam={self.lam}, lam_y={self.lam_y}, outer={self.outer}, inner={self.inner})")


_MULTIVIEW = []     # settings installed by multi_view(), innermost last.  Empty unless a caller opened one: every pass sees each pool image once by default


@contextlib.contextmanager
def multi_view(mv):
    """Install `mv` (a MultiView, or None: no-op) for the pseudolabel passes underneath, as label_propagation() / soft_targets() / candidate_sets()
    install theirs.  While one is installed compute_pseudo_labels and Strategy.trained_features hand the modes of the pool's views to
    pseudolabel_from_features instead of encode_pool's rows, the callers that would pick identical_lists take their plain branch (no reference list can
    be identical to a multi-view one), the PoolFeatureCache is neither read nor written for modes (they depend on the text features) and
    pseudolabel_top_k names its pickle `..._pseudolabels_mv_split_...` (`cpl_mv_lp_`, ... with the other switches)."""
    if mv is None:
        yield None
        return
    if not isinstance(mv, MultiView):
        raise TypeError(f"multi_view: expected a MultiView or None, got {type(mv).__name__}")
    _MULTIVIEW.append(mv)
    try:
        yield mv
    finally:
        _MULTIVIEW.pop()


def multiview():
    """The innermost installed MultiView, or None."""
    return _MULTIVIEW[-1] if _MULTIVIEW else None


def list_infix():
    """The infix of a pseudolabel pickle's name for what is installed: "", lp_ / gmm_ / ot_..., with mv_ in front under multi_view() and cpl_ in front
    of both under candidate_sets()."""
    return ((CandidateSelection.infix if candidates() is not None else "") + (MultiView.infix if multiview() is not None else "") +
            (propagation().infix if propagation() is not None else ""))


@torch.no_grad()
def pseudolabel_from_features(img_emb, txt_emb, scale, paths, class_labels, k, argmax_on="probs"):
    """Head + scan.  argmax_on: "probs" (compute_pseudo_labels, :39) or "logits" (assign_pseudo_labels).  With a LabelPropagation or a
    TransductiveGMM installed the scan runs on its Z over the whole (gathered, on every rank alike) pool and on arg-max Z, for both forms of argmax_on;
    a SoftTargetStore installed by soft_targets() then records that matrix.  With candidate_sets() installed the selection replaces the scan (on Z / Q,
    else on the head's probabilities): the lists are the pool rows with a non-empty candidate set, each once, in pool order."""
    logits, probs, am_l, am_p = engine.cosine_head(img_emb, txt_emb, scale)
    lp = propagation()
    cand = candidates()
    if lp is not None and img_emb.shape[0] >= 2:        # (a pool of one image has no neighbour to hear from)
        z, z_pred = lp.transduce(img_emb, probs, paths)
        store = soft_target_store()
        if store is not None:
            store.record(paths, class_labels, z)
        if cand is not None:
            return cand[0].select(z, paths, class_labels, k, cand[1])
        return leaderboard(z.cpu().numpy(), z_pred.cpu().numpy(), paths, class_labels, k)
    if soft_target_store() is not None:
        soft_target_store().forget()        # a pass without a transduction has no matrix: the rows of an earlier one no longer name its lists
    if cand is not None:
        return cand[0].select(probs, paths, class_labels, k, cand[1])
    pred = (am_p if argmax_on == "probs" else am_l).cpu().numpy()
    return leaderboard(probs.cpu().numpy(), pred, paths, class_labels, k)
