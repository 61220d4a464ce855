"""float64 references, bounds and inputs for the streaming-cache kernels (csrc/stream_cache.hip; the model of include/grip_amd.h, grip_stream_cache_plan /
grip_stream_cache_head), shared by the GPU tests and checked against each other on the host (tests/test_host_stream_cache_ref.py).  numpy throughout.

TWO REFERENCES, written independently.
  literal64    the algorithm as published: one item at a time, a Python list per class and polarity, the item scored after its own admission against
               what the lists hold at that moment.  It records who was resident when every item was scored.
  scan / evaluate64   the interval form: a scan of (H, pred) alone gives every item's interval [j, leave_j); item i then sums the keys with
               j <= i < leave_j.  The scan also runs on a DEVICE's own f32 entropy / pred (its comparisons are plain f32 comparisons, exact in numpy),
               and evaluate64 on a device's membership, so that only arithmetic is compared.

THE BOUNDS.  u = 2^-24, expf / logf within 2 ulp = 4 u relative (view_entropy_ref.py, whose per-row bounds bp and bH are used as they are: the row
statements are the same), first order in u with a unit of room per line; a sum of t terms in ANY order is within (t + 2) u of the sum of the absolute
values.  Nothing below is measured.
    c = 1       x - max = 0, expf(0) = 1, logf(1) = 0, lse = x, d = 0, p = 1, H = 0: every step is exact in any arithmetic -- bp = bH = 0.
    pred        the first arg-max of the f32 logits themselves: no arithmetic, it EQUALS the float64 one on every row without a NaN.
    negbits     bit y is decided where p_y is further than 2 bp_y from both ends of the mask window.
    dot_ij      an e-term f32 chain: (e + 2) u sum_k |f_ik f_jk| <= (e + 2) u |f_i| |f_j|                       (relative to |f_i| |f_j|)
    1 / |f|     the sum of squares (e + 2) u relative, so its root (e + 2) u / 2; sqrtf, the division: u each    brn = (e / 2 + 3) u
    s_ij        (dot rn_i) rn_j, two rounded products; |f_i| |f_j| rn_i rn_j = 1 to first order:                bs = (e + 2) u + 2 brn + 2 u |s|
    t           1 - s rounds once, beta (1 - s) once:                                                            bt = beta bs + 2 u |t|
    a           expf(-t) moves with its argument as exp(bt) - 1 and adds 4 u relative; 2^-126 for the subnormal range:
                                                                                                                 ba = a (exp(bt) (1 + 4 u) - 1) + 2^-126
    S           k live terms:                                                                                    bS = sum ba + (k + 2) u S
    out         two rounded products alpha S and two rounded additions, each no larger than M = |base| + alpha_p S_p + alpha_n S_n:
                                                                                                                 bout = alpha_p bS_p + alpha_n bS_n + 4 u M
The entropy bound bH also says when the mask bits are the only thing f32 may decide differently; the queue history is NOT compared with float64 -- it
is compared, exactly, with the scan below run on the device's own H and pred (an entropy order closer than the bounds may go either way, and whichever
way it goes the history must be the sequential algorithm's)."""
import numpy as np

import view_entropy_ref as V

U, TINY, EXP_REL = V.U, V.TINY, V.EXP_REL
INT32_MAX = 2 ** 31 - 1
DEFAULTS = dict(pos_cap=3, neg_cap=2, pos_alpha=2.0, pos_beta=5.0, neg_alpha=0.117, neg_beta=1.0, neg_entropy=(0.2, 0.5), neg_mask=(0.03, 1.0))


# ------------------------------------------------------------------------------------------ the per-item quantities
def rows64(x, neg_mask):
    """dict(p, H, pred, bits bool [n, c], bp, bH, decided bool [n, c]) of logits x [n, c] (f32 values) in float64.  A row with a NaN: H = NaN, nothing
    decided."""
    x = np.asarray(x)
    n, c = x.shape
    with np.errstate(all="ignore"):
        p, d, H, bp, bH = V.views64(x)
    if c == 1:
        bp, bH = np.zeros_like(bp), np.zeros_like(bH)
    bad = ~np.isfinite(x).all(1)
    H = np.where(bad, np.nan, H)
    pred = np.zeros(n, dtype=np.int64)
    for i in range(n):
        best = -np.inf
        for y in range(c):       # the FIRST arg-max, as the kernel takes it: strictly greater wins
            if x[i, y] > best:
                best, pred[i] = x[i, y], y
    lo, hi = (float(np.float32(v)) for v in neg_mask)      # the thresholds are the kernel's f32 parameters
    with np.errstate(invalid="ignore"):
        bits = (p > lo) & (p < hi)
        decided = (((np.abs(p - lo) > 2 * bp) & (np.abs(p - hi) > 2 * bp)) | (bp == 0)) & ~bad[:, None]      # (bp = 0: p is exact, c = 1)
    return dict(p=p, H=H, pred=pred, bits=bits, bp=bp, bH=bH, decided=decided)


def pack_bits(bits):
    """bool [n, c] -> int32 [n, ceil(c / 32)]: bit (y mod 32) of word y / 32, the layout of the candidate masks."""
    n, c = bits.shape
    words = (c + 31) // 32
    out = np.zeros((n, words), dtype=np.uint32)
    for y in range(c):
        out[:, y // 32] |= bits[:, y].astype(np.uint32) << np.uint32(y % 32)
    return out.view(np.int32)


def unpack_bits(words, c):
    w = np.ascontiguousarray(words).view(np.uint32)
    return np.stack([(w[:, y // 32] >> np.uint32(y % 32)) & np.uint32(1) for y in range(c)], axis=1).astype(bool)


def normalised_entropy(H, c, f32):
    """H / log c (0 for c = 1): in float64, or as the kernel forms it -- an f32 division by L = (float)log((double)c)."""
    if c == 1:
        return np.zeros_like(H)
    with np.errstate(invalid="ignore"):
        return (np.asarray(H, dtype=np.float32) / np.float32(np.log(np.float64(c)))) if f32 else np.asarray(H, dtype=np.float64) / np.log(np.float64(c))


# ------------------------------------------------------------------------------------------ the interval form
def scan(H, pred, c, cap, eligible=None):
    """leave int64 [n] of one polarity: the queue rule of the header played on (H, pred) in order; the comparisons are on H AS GIVEN (f32 or f64)."""
    n = len(H)
    leave = np.arange(n, dtype=np.int64)
    if cap == 0:
        return leave
    queues = [[] for _ in range(c)]
    for i in range(n):
        h = H[i]
        if not np.isfinite(h) or (eligible is not None and not eligible[i]):
            continue
        q = queues[int(pred[i])]
        if len(q) < cap:
            q.append(i)
            leave[i] = INT32_MAX
            continue
        worst = max(q, key=lambda j: (H[j], j))
        if h < H[worst]:
            q.remove(worst)
            leave[worst] = i
            q.append(i)
            leave[i] = INT32_MAX
    return leave


def plan_from(H, pred, c, pos_cap, neg_cap, neg_entropy, f32):
    """dict(pos_leave, neg_leave, pos_key, neg_key) of the scan on (H, pred): f32 = True plays the kernel's own comparisons on a device's entropy_out."""
    hn = normalised_entropy(H, c, f32)
    lo, hi = (np.float32(v) for v in neg_entropy) if f32 else neg_entropy
    with np.errstate(invalid="ignore"):
        elig = (hn > lo) & (hn < hi)
    pos = scan(H, pred, c, pos_cap)
    neg = scan(H, pred, c, neg_cap, elig)
    idx = np.arange(len(H))
    return dict(pos_leave=pos, neg_leave=neg, pos_key=idx[pos != idx], neg_key=idx[neg != idx])


def live(leave):
    """bool [n, n]: L[i, j] = key j is resident when item i is scored (j <= i < leave_j)."""
    n = len(leave)
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    return (j <= i) & (i < np.asarray(leave)[None, :])


def evaluate64(base, feats, pred, bits, pos_leave, neg_leave, pos_alpha, pos_beta, neg_alpha, neg_beta):
    """(out, bound) float64 [n, c]: the header's score on a GIVEN membership (pred int [n], bits bool [n, c], the two leave arrays) and its f32 bound."""
    base, f = np.asarray(base, dtype=np.float64), np.asarray(feats, dtype=np.float64)
    n, c = base.shape
    e = f.shape[1]
    with np.errstate(all="ignore"):
        fh = f / np.sqrt((f * f).sum(1, keepdims=True))
        s = fh @ fh.T
    bs = (e + 2) * U + 2 * (e / 2 + 3) * U + 2 * U * np.abs(s)
    onehot = np.zeros((n, c))
    onehot[np.arange(n), np.asarray(pred)] = 1.0
    out, bound, mag = base.copy(), np.zeros((n, c)), np.abs(base)
    for sign, alpha, beta, leave, values in ((1.0, pos_alpha, pos_beta, pos_leave, onehot), (-1.0, neg_alpha, neg_beta, neg_leave, bits.astype(np.float64))):
        L = live(leave).astype(np.float64)
        t = beta * (1.0 - s)
        bt = beta * bs + 2 * U * np.abs(t)
        with np.errstate(all="ignore"):
            a = np.exp(-t)
            ba = a * (np.exp(bt) * (1 + EXP_REL) - 1) + TINY
        a, ba = np.where(L > 0, a, 0.0), np.where(L > 0, ba, 0.0)      # (a dead pair may hold a NaN: it is not part of any sum)
        S, bS, k = a @ values, ba @ values, L @ values
        bS = bS + (k + 2) * U * S
        out = out + sign * alpha * S
        bound = bound + alpha * bS
        mag = mag + alpha * S
    return out, bound + 4 * U * mag


def reference64(base, feats, **settings):
    """The interval form end to end in float64: dict(out, H, pred, bits, pos_leave, neg_leave, pos_key, neg_key, members) with members[pol][i] the
    frozenset of keys live when item i is scored."""
    st = dict(DEFAULTS, **settings)
    r = rows64(base, st["neg_mask"])
    c = np.asarray(base).shape[1]
    pl = plan_from(r["H"], r["pred"], c, st["pos_cap"], st["neg_cap"], st["neg_entropy"], f32=False)
    out, _ = evaluate64(base, feats, r["pred"], r["bits"], pl["pos_leave"], pl["neg_leave"], st["pos_alpha"], st["pos_beta"], st["neg_alpha"], st["neg_beta"])
    members = [[frozenset(np.nonzero(row)[0].tolist()) for row in live(pl[k])] for k in ("pos_leave", "neg_leave")]
    return dict(out=out, H=r["H"], pred=r["pred"], bits=r["bits"], members=members, **pl)


# ------------------------------------------------------------------------------------------ the literal loop
def literal64(base, feats, **settings):
    """The algorithm one item at a time in float64, Python lists per class: dict(out [n, c], members) as reference64's.  Shares no code with the
    interval form."""
    st = dict(DEFAULTS, **settings)
    x, f = np.asarray(base, dtype=np.float64), np.asarray(feats, dtype=np.float64)
    n, c = x.shape
    pos_q = [[] for _ in range(c)]      # entries (H, index)
    neg_q = [[] for _ in range(c)]
    ent_lo, ent_hi = st["neg_entropy"]
    mask_lo, mask_hi = st["neg_mask"]
    logc = np.log(np.float64(c))
    out = x.copy()
    members = [[], []]
    mask_of = {}
    with np.errstate(all="ignore"):
        unit = f / np.sqrt((f * f).sum(1, keepdims=True))
        cos = unit @ unit.T
    for i in range(n):
        xi = x[i]
        with np.errstate(all="ignore"):
            mx = xi.max()
            lse = mx + np.log(np.exp(xi - mx).sum())
            prob = np.exp(xi - lse)
            H = float(-(prob * (xi - lse)).sum())
        if np.isnan(xi).any():
            H = float("nan")
        pred = 0
        for y in range(1, c):
            if xi[y] > xi[pred]:
                pred = y
        mask_of[i] = [y for y in range(c) if mask_lo < prob[y] < mask_hi]
        hn = H / logc if c > 1 else 0.0

        def admit(queue, cap):
            if cap == 0 or not np.isfinite(H):
                return
            if len(queue) < cap:
                queue.append((H, i))
                return
            queue.sort()
            if H < queue[-1][0]:
                queue[-1] = (H, i)
        admit(pos_q[pred], st["pos_cap"])
        if ent_lo < hn < ent_hi:
            admit(neg_q[pred], st["neg_cap"])
        for y in range(c):
            s = 0.0
            for _, j in sorted(pos_q[y], key=lambda t: t[1]):
                s += np.exp(-st["pos_beta"] * (1.0 - cos[i, j]))
            if pos_q[y]:
                out[i, y] += st["pos_alpha"] * s
        neg_sum = np.zeros(c)
        for j in sorted(j for q in neg_q for _, j in q):
            a = np.exp(-st["neg_beta"] * (1.0 - cos[i, j]))
            for y in mask_of[j]:
                neg_sum[y] += a
        out[i] -= st["neg_alpha"] * neg_sum
        members[0].append(frozenset(j for q in pos_q for _, j in q))
        members[1].append(frozenset(j for q in neg_q for _, j in q))
    return dict(out=out, members=members)


# ------------------------------------------------------------------------------------------ inputs
POOLS = ("normal", "peaked", "descending", "ascending", "duplicates", "nan_row")


def pool(kind, n, c, e, seed=0):
    """(base f32 [n, c], feats f32 [n, e]) of one input pool.
    normal / peaked   N(0, 1) and 30 N(0, 1) logits;
    descending        every item predicts class 0 and the entropies fall strictly along the stream (the step between neighbours is far above bH): every
                      item is admitted, m = n, and once the queue is full every item evicts one;  ascending: the same rows in reverse -- after the fill
                      nothing is admitted;
    duplicates        every row of a normal pool twice in a row: exact entropy ties, the later item must not enter a full queue on a tie;
    nan_row           a normal pool with one row of NaNs (never admitted, scored as a NaN row)."""
    rng = np.random.default_rng(1000 * seed + 7 * n + 13 * c + e)
    feats = rng.standard_normal((n, e)).astype(np.float32) * np.float32(1.5)
    if kind in ("normal", "nan_row"):
        base = rng.standard_normal((n, c))
        if kind == "nan_row":
            base[n // 2] = np.nan
    elif kind == "peaked":
        base = 30.0 * rng.standard_normal((n, c))
    elif kind in ("descending", "ascending"):
        base = np.zeros((n, c)) + 0.125 * rng.standard_normal((1, c))
        base[:, 0] = 1.0 + np.arange(n) * (8.0 / max(n, 1))
        if kind == "ascending":
            base = base[::-1]
    elif kind == "duplicates":
        half = rng.standard_normal(((n + 1) // 2, c))
        base = np.repeat(half, 2, axis=0)[:n]
        feats = np.repeat(feats[:(n + 1) // 2], 2, axis=0)[:n] + np.float32(0.01) * rng.standard_normal((n, e)).astype(np.float32)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(base, dtype=np.float32), np.ascontiguousarray(feats, dtype=np.float32)


def settings_for(kind, caps):
    """The settings a pool is run with.  The windows are chosen so that the queues see traffic and the float64 reference alone decides the mask bits: the
    peaked pools keep the upper mask end away from 1 (a top probability within 1e-7 of 1 is undecidable at ANY precision of lse: p < 1 or p = 1), the
    others run the default (0.03, 1.0)."""
    pos_cap, neg_cap = caps
    return dict(DEFAULTS, pos_cap=pos_cap, neg_cap=neg_cap, neg_entropy=(0.02, 0.995) if kind != "peaked" else (1e-4, 0.9),
                neg_mask=(0.03, 0.95) if kind == "peaked" else (0.03, 1.0))


CASES = [(kind, n, c, e, caps) for kind in POOLS for (n, c, e, caps) in
         ((1, 1, 64, (1, 0)), (2, 2, 64, (3, 2)), (63, 33, 64, (3, 2)), (65, 102, 512, (16, 16)), (257, 102, 64, (3, 2)), (257, 2, 64, (1, 0)),
          (65, 1, 64, (3, 2)), (257, 33, 512, (16, 16)))]


def planted(seed, n=2000, c=20, e=64, scale=20.0):
    """(base f32 [n, c], feats f32 [n, e], labels [n]): a stream whose features cluster by class and whose zero-shot head is BIASED (its class directions
    are the prototypes plus noise), so that a cache built from the stream itself has something to add."""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((c, e))
    proto /= np.linalg.norm(proto, axis=1, keepdims=True)
    head = proto + 1.2 * rng.standard_normal((c, e)) / np.sqrt(e)
    head /= np.linalg.norm(head, axis=1, keepdims=True)
    labels = rng.integers(0, c, n)
    feats = proto[labels] + 2.5 * rng.standard_normal((n, e)) / np.sqrt(e)
    unit = feats / np.linalg.norm(feats, axis=1, keepdims=True)
    base = scale * unit @ head.T
    return base.astype(np.float32), feats.astype(np.float32), labels
