"""References, bound and inputs for the candidate-set kernels (csrc/candidate.hip), shared by the GPU tests and checked against independent oracles on the
host (tests/test_host_candidate_ref.py).

SELECTION (grip_candidate_select), NumPy, compared BIT FOR BIT: threshold[c] = np.sort(column)[::-1][claim - 1]; the inter set of a row is
{c : p[c] >= threshold[c]}; the intra set ranks the classes by a stable argsort of -p (probability descending, index ascending), takes
s = np.cumsum(sorted p, dtype=float32) -- the sequential f32 sum s_j = s_{j-1} + p_(j), which the host test checks against a literal loop -- and keeps rank 0
and every rank j >= 1 with s_{j-1} < tau.  combine: intersection, union, intra, inter.  mask packs class j into bit j % 32 of int32 word j // 32; count is
the set's size; label its member of highest rank or -1.

LOSS (grip_candidate_ce), float64 on the SAME f32 operands with a per-element bound, in the conventions of tests/soft_ce_ref.py (whose constants and
softmax / lse bounds are reused): first-order forward error propagation through the kernel's own sequence of operations, u = 2^-24, expf and logf 2 u
relative, inputs exact, every result that can underflow carries 2^-126 absolute; nothing in the bound is measured.
    a row i with 0 <= cand_row[i] < cand_rows is a CANDIDATE row, S = {col_map[j] : bit j of its mask row set, col_map[j] in [0, c)}; any other row is HARD.
    lse, p   of the whole row: as soft_ce_ref (e_lse, e_p)
    over S   the maximum of S is exact; zS = x - mS rounds once: e_z = u |zS|; expf: e_ex = ex expm1(e_z) + 2 u ex e^{e_z} + 2^-126; the sum of at most
             ceil(c / 64) in-lane terms and six wave levels: e_sS = sum e_ex + (ceil(c / 64) + 6) u sS; lgS = logf(sS), lseS = mS + lgS:
             e_lseS = e_sS / sS + 2 u |lgS| + u |lseS|;  q = ex / sS: e_q = e_ex / sS + ex e_sS / sS^2 + u q + 2^-126 (q = 0 exactly outside S)
    hard     sub = x[label] and q = onehot(label) are exact (a label outside [0, c): q = 0, the row is not in the loss)
    term     d = lse - sub, term = w d:  e_term = |w| (e_lse + e_sub + u |d|) + u |term|
    loss     ceil(n / 4) in-wave adds and three across the waves:  e_loss = sum e_term + (ceil(n / 4) + 3) u sum |term| + 2^-126
    grad     d = p - q, g = w d:  e_g = |w| (e_p + e_q + u |d|) + u |g| + 2^-126
A candidate row whose mapped set is empty contributes nothing: its term is out of the loss and its gradient row is exactly 0."""
import numpy as np
import torch

from soft_ce_ref import EXP_REL, LOG_REL, TINY, U, _depth, _sm

COMBINE = ("intersection", "union", "intra", "inter")


# ------------------------------------------------------------------------------------------ selection
def words(c):
    return (c + 31) // 32


def pack(member):
    """bool [n, c] -> int32 [n, ceil(c / 32)]: class j is bit j % 32 of word j // 32."""
    n, c = member.shape
    padded = np.zeros((n, 32 * words(c)), dtype=np.uint8)
    padded[:, :c] = member
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint32).view(np.int32).reshape(n, words(c))


def unpack(mask, c):
    """int32 [n, words] -> bool [n, c]."""
    bits = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8).reshape(mask.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :c].astype(bool)


def thresholds(p, claim):
    return np.sort(p, axis=0)[::-1][claim - 1].astype(np.float32)


class Ranking:
    """What every (claim, tau, combine) of one pool shares, computed once: the columns sorted, the stable rank order of every row, each class's rank
    (`pos`) and the sequential f32 running sums in rank order."""

    def __init__(self, p):
        self.p = p = np.ascontiguousarray(p, dtype=np.float32)
        self.n, self.c = p.shape
        self.columns = np.sort(p, axis=0)[::-1]
        self.order = np.argsort(-p, axis=1, kind="stable")
        self.pos = np.empty_like(self.order)
        np.put_along_axis(self.pos, self.order, np.broadcast_to(np.arange(self.c), p.shape), axis=1)
        self.s = np.cumsum(np.take_along_axis(p, self.order, axis=1), axis=1, dtype=np.float32)

    def threshold(self, claim):
        return np.ascontiguousarray(self.columns[claim - 1], dtype=np.float32)

    def inter(self, claim, threshold=None):
        return self.p >= (self.threshold(claim) if threshold is None else np.asarray(threshold, dtype=np.float32))[None]

    def intra(self, tau):
        keep = np.ones((self.n, self.c), dtype=bool)         # by rank: rank 0 always, rank j >= 1 iff s_{j-1} < tau
        keep[:, 1:] = self.s[:, :-1] < np.float32(tau)
        return np.take_along_axis(keep, self.pos, axis=1)


def combine_sets(intra, inter, combine):
    """The member matrix of a combine mode (NumPy arrays or torch tensors)."""
    return {"intersection": intra & inter, "union": intra | inter, "intra": intra, "inter": inter}[combine]


def select(p, claim, tau, combine="intersection", threshold=None):
    """(mask int32 [n, words], count int32 [n], label int32 [n], threshold f32 [c]) of a float32 [n, c] array; `threshold` given: used as is."""
    r = p if isinstance(p, Ranking) else Ranking(p)
    thr = r.threshold(claim) if threshold is None else np.asarray(threshold, dtype=np.float32)
    member = combine_sets(r.intra(tau), r.inter(claim, thr), combine)
    best = np.where(member, r.pos, r.c).min(axis=1)           # the member of highest rank
    label = np.where(best < r.c, r.order[np.arange(r.n), np.minimum(best, r.c - 1)], -1).astype(np.int32)
    return pack(member), member.sum(axis=1).astype(np.int32), label, thr


def outputs_t(member, pos, order):
    """(mask, count, label) int32 torch tensors of a bool member matrix [n, c] on its device (pos, order: Ranking's, int64 tensors there): what the kernel
    must return for that set, built with torch so that a large case needs no host pass per mode."""
    n, c = member.shape
    w = words(c)
    padded = torch.zeros(n, 32 * w, dtype=torch.int64, device=member.device)
    padded[:, :c] = member
    word = (padded.view(n, w, 32) << torch.arange(32, device=member.device)).sum(-1)
    mask = torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)
    best = torch.where(member, pos, torch.full_like(pos, c)).min(dim=1).values
    label = torch.where(best < c, order.gather(1, best.clamp(max=c - 1)[:, None])[:, 0], torch.full_like(best, -1)).to(torch.int32)
    return mask, member.sum(1).to(torch.int32), label


# ------------------------------------------------------------------------------------------ loss
def members(cand, cand_row, col_map, n, c, dev="cpu"):
    """(is_cand bool [n], member bool [n, c]) on `dev` (the device of cand_row when there is one): the mapped set of every candidate row."""
    dev = cand_row.device if cand_row is not None else dev
    is_cand = torch.zeros(n, dtype=torch.bool, device=dev)
    member = torch.zeros(n, c, dtype=torch.bool, device=dev)
    if cand is None:
        return is_cand, member
    r = cand_row.long()
    is_cand = (r >= 0) & (r < cand.shape[0])
    cz = col_map.shape[0]
    j = torch.arange(cz, device=dev)
    bits = ((cand.long()[:, j // 32] >> (j % 32)) & 1).bool()          # [rows, cz]
    cm = col_map.long()
    ok = (cm >= 0) & (cm < c)
    full = torch.zeros(cand.shape[0], c, dtype=torch.bool, device=dev)
    full[:, cm[ok]] = bits[:, ok]
    member[is_cand] = full[r[is_cand]]
    return is_cand, member


def candidate_ce64(logits, labels, weight, cand=None, cand_row=None, col_map=None):
    """dict of the float64 values and bounds: loss, e_loss (0-d); grad, e_grad [n, c]; term, e_term, counted, is_cand, empty [n]."""
    x, w = logits.double(), weight.double()[:, None]
    n, c = x.shape
    dev = x.device
    lab = labels.long()
    valid = (lab >= 0) & (lab < c)
    is_cand, member = members(cand, cand_row, col_map, n, c, dev)
    empty = is_cand & ~member.any(-1)
    live = is_cand & ~empty
    # lse and p of the whole row: tests/soft_ce_ref.py
    m = x.max(-1, keepdim=True).values
    z = x - m
    e_z = U * z.abs()
    ex = z.exp()
    e_ex = ex * torch.expm1(e_z) + EXP_REL * ex * e_z.exp() + TINY
    sm = _sm(ex)
    e_sm = _sm(e_ex) + _depth(c) * U * sm
    lg = sm.log()
    lse = m + lg
    e_lse = e_sm / sm + LOG_REL * lg.abs() + U * lse.abs()
    p = ex / sm
    e_p = e_ex / sm + ex * e_sm / sm ** 2 + U * p + TINY
    # the same over S
    mS = torch.where(member, x, torch.full_like(x, -float("inf"))).max(-1, keepdim=True).values
    mS = torch.where(live[:, None], mS, torch.zeros_like(mS))
    zS = torch.where(member, x - mS, torch.zeros_like(x))
    e_zS = U * zS.abs()
    exS = torch.where(member, zS.exp(), torch.zeros_like(x))
    e_exS = torch.where(member, exS * torch.expm1(e_zS) + EXP_REL * exS * e_zS.exp() + TINY, torch.zeros_like(x))
    sS = torch.where(live[:, None], _sm(exS), torch.ones_like(mS))
    e_sS = _sm(e_exS) + _depth(c) * U * sS
    lgS = sS.log()
    lseS = mS + lgS
    e_lseS = e_sS / sS + LOG_REL * lgS.abs() + U * lseS.abs()
    qS = exS / sS
    e_qS = torch.where(member, e_exS / sS + exS * e_sS / sS ** 2 + U * qS + TINY, torch.zeros_like(x))
    onehot = ((torch.arange(c, device=dev)[None] == lab[:, None]) & valid[:, None]).double()
    x_lab = (x * onehot).sum(-1, keepdim=True)
    q = torch.where(is_cand[:, None], qS, onehot)
    e_q = torch.where(is_cand[:, None], e_qS, torch.zeros_like(x))
    sub = torch.where(is_cand[:, None], lseS, x_lab)
    e_sub = torch.where(is_cand[:, None], e_lseS, torch.zeros_like(lseS))
    d = lse - sub
    term = w * d
    e_term = w.abs() * (e_lse + e_sub + U * d.abs()) + U * term.abs()
    counted = ((w[:, 0] != 0) & (live | (~is_cand & valid)))[:, None]
    loss = (term * counted).sum()
    e_loss = (e_term * counted).sum() + ((n + 3) // 4 + 3) * U * (term.abs() * counted).sum() + TINY
    dg = p - q
    grad = w * dg
    e_grad = w.abs() * (e_p + e_q + U * dg.abs()) + U * grad.abs() + TINY
    grad = torch.where(empty[:, None], torch.zeros_like(grad), grad)
    e_grad = torch.where(empty[:, None], torch.zeros_like(e_grad), e_grad)
    return dict(loss=loss, e_loss=e_loss, grad=grad, e_grad=e_grad, term=term[:, 0], e_term=e_term[:, 0], counted=counted[:, 0], is_cand=is_cand, empty=empty)


def check(ref, loss, grad=None):
    """Assert every element of the kernel's outputs against `ref` (candidate_ce64); returns the worst |err| / bound."""
    worst = 0.0
    for name, got, want, b in (("loss", loss, ref["loss"], ref["e_loss"]), ("grad", grad, ref["grad"], ref["e_grad"])):
        if got is None:
            continue
        err = (got.double().reshape(want.shape) - want).abs()
        ratio = float(torch.where(err == 0, torch.zeros_like(err), err / b).max())
        assert bool(torch.isfinite(got).all()) and bool((err <= b).all()), f"candidate_ce: |{name} - {name}64| is {ratio:.2f} x its bound"
        worst = max(worst, ratio)
    return worst


def candidate_ce_f32(logits, labels, weight, cand=None, cand_row=None, col_map=None):
    """An f32 emulation of the kernel in torch (torch's own summation order): what the checker must accept.  (loss, grad)."""
    x, w = logits.float(), weight.float()[:, None]
    n, c = x.shape
    lab = labels.long()
    valid = (lab >= 0) & (lab < c)
    is_cand, member = members(cand, cand_row, col_map, n, c, x.device)
    live = is_cand & member.any(-1)
    m = x.max(-1, keepdim=True).values
    ex = torch.exp(x - m)
    sm = _sm(ex)
    lse = m + torch.log(sm)
    mS = torch.where(member, x, torch.full_like(x, -float("inf"))).max(-1, keepdim=True).values
    mS = torch.where(live[:, None], mS, torch.zeros_like(mS))
    exS = torch.where(member, torch.exp(x - mS), torch.zeros_like(x))
    sS = torch.where(live[:, None], _sm(exS), torch.ones_like(mS))
    onehot = ((torch.arange(c)[None] == lab[:, None]) & valid[:, None]).float()
    q = torch.where(is_cand[:, None], exS / sS, onehot)
    sub = torch.where(is_cand[:, None], mS + torch.log(sS), (x * onehot).sum(-1, keepdim=True))
    counted = ((w[:, 0] != 0) & (live | (~is_cand & valid)))[:, None]
    grad = w * (ex / sm - q)
    grad[is_cand & ~live] = 0.0
    return ((w * (lse - sub)) * counted).sum(), grad


# ------------------------------------------------------------------------------------------ inputs and cases of the loss
CS = (1, 63, 64, 65, 102, 129, 300)
NS = (1, 4, 5, 67)
SHAPES = [(n, c) for n in NS for c in CS]
CAND_ROWS = 9
_ROW_PATTERN = (2, -1, 0, 1, CAND_ROWS, 3, -1, 4, 5, -7, 6, 7, 8)        # mask row of batch row i (cycled): < 0 and CAND_ROWS mark hard rows


def czs(c):
    """The mask widths of the case table: 1, c - 1 and c where they exist."""
    return sorted({v for v in (1, c - 1, c) if 1 <= v <= c})


def sets(cz, seed):
    """cand int32 [CAND_ROWS, words(cz)]: row 0 empty, row 1 the single class cz - 1, row 2 full, row 3 two classes, the others random with about cz / 8 + 1
    members (possibly none)."""
    g = torch.Generator().manual_seed(seed)
    member = torch.rand(CAND_ROWS, cz, generator=g) < (cz / 8 + 1) / cz
    member[0] = False
    member[1] = False
    member[1, cz - 1] = True
    member[2] = True
    member[3] = False
    member[3, 0] = True
    member[3, cz // 2] = True
    return torch.from_numpy(pack(member.numpy()).copy())


def operands(n, c, cz, seed=None):
    """(logits [n, c], labels [n] int32, weight [n], cand [CAND_ROWS, words(cz)] int32, cand_row [n] int32, col_map [cz] int32) on the CPU: hard and candidate
    rows, empty, singleton and full sets, zero weights (i = 3 mod 5) and negative ones, labels outside [0, c) on a hard row (i = 6 mod 13: label c) and on a
    candidate one (i = 7 mod 13: -3, never read), a mask row index outside the matrix; col_map is the head of a permutation of the c columns."""
    g = torch.Generator().manual_seed(1000 * n + 10 * c + cz if seed is None else seed)
    i = torch.arange(n)
    logits = (4 * torch.randn(n, c, generator=g)).float()
    labels = torch.randint(0, c, (n,), generator=g).to(torch.int32)
    labels[i % 13 == 6] = c
    labels[i % 13 == 7] = -3
    weight = (0.25 + torch.rand(n, generator=g)).float() * torch.where(torch.rand(n, generator=g) < 0.2, -1.0, 1.0)
    weight[i % 5 == 3] = 0.0
    cand_row = torch.tensor([_ROW_PATTERN[k % len(_ROW_PATTERN)] for k in range(n)], dtype=torch.int32)
    col_map = torch.randperm(c, generator=g)[:cz].to(torch.int32)
    return logits, labels, weight.float(), sets(cz, seed=7 * c + cz), cand_row, col_map


# ------------------------------------------------------------------------------------------ inputs and cases of the selection
SEL_NS = (1, 2, 17, 64, 65, 1000, 4099)
SEL_CS = (1, 2, 31, 32, 33, 102, 129, 300, 1024)
SEL_TAUS = (0.5, 0.99, 1.0)
SEL_KINDS = ("softmax", "quantised", "duplicates", "uniform")


def claims(n, c):
    return sorted({1, min(2, n), n, min(n, max(1, -(-2 * n // c)))})


def pool(n, c, kind, seed=0):
    """float32 [n, c] probabilities (finite, >= 0).  softmax: rows of a softmax with a few dominant classes; quantised: multiples of 2^-6 (ties everywhere,
    exact sums); duplicates: columns 0 and c - 1 equal, rows 0 and n - 1 equal, one column zero in every row; uniform: every third row exactly 1 / c."""
    g = np.random.default_rng(1000003 * n + 101 * c + seed)
    z = 3.0 * g.standard_normal((n, c)) + 4.0 * (g.random((n, c)) < 2.0 / c)
    p = np.exp(z - z.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    if kind == "quantised":
        p = (np.floor(g.random((n, c)) ** 4 * 64) / 64).astype(np.float32)
    elif kind == "duplicates":
        p[:, c - 1] = p[:, 0]
        p[n - 1] = p[0]
        p[:, c // 2] = 0.0
    elif kind == "uniform":
        p[::3] = np.float32(1.0) / np.float32(c)
    return np.ascontiguousarray(p)
