"""float64 reference, bounds and inputs for the view-entropy kernel (csrc/view_entropy.hip; the model of include/grip_amd.h, grip_view_entropy), shared by
the GPU tests and shown to hold for an f32 emulation of the kernel's operation order on the host (tests/test_host_view_entropy_ref.py).  numpy throughout.
The reference runs in float64 on the SAME f32 logits, so only the arithmetic differs; it can evaluate the loss and the gradient on a GIVEN selection (the
selection is a constant of the gradient, and where two entropies are closer than their bounds either order is right).

THE MODEL.  Per view p of an image: lse_p = max + log sum exp(x - max), p_pc = exp(x_pc - lse_p), H_p = sum_c p_pc (lse_p - x_pc).  The `keep` views of
smallest H_p are selected (ties to the lower index, a non-finite H_p after every finite one).  pbar_c = (1 / keep) sum_{p selected} p_pc,
loss_i = -sum_c pbar_c log max(pbar_c, 2^-126), loss = (1 / n) sum_i loss_i, g_c = -(log max(pbar_c, 2^-126) + 1) / (keep n), and a selected view gets
grad x_pj = p_pj (g_j - sum_c p_pc g_c), every other view zero.

THE BOUNDS.  u = 2^-24 (the unit roundoff of f32; one ulp is 2 u), expf and logf within 2 ulp = 4 u relative (what tests/sinkhorn_ref.py, gmm_ref.py and
view_mode_ref.py assume), first order in u with a unit of room per line; a sum of t terms in ANY order is within (t + 2) u of the sum of the absolute
values, so no bound knows how the kernel or the emulation adds.  Nothing below is measured.
    sum_p       t_j = x_j - max rounds once (u |t_j|), e_j = expf(t_j) is within (4 + |t_j|) u relative, the sum adds (c + 2) u:
                    es = (c + 2) u + sum_j e_j (4 + |t_j|) u / sum_j e_j                 (relative to the sum)
    lse_p       L = logf(sum): es + 4 u |L|; lse = max + L rounds once:                  blse = es + 4 u |L| + u |lse|
    d_pj        d = lse - x_j rounds once:                                               bd = blse + u d
    p_pj        expf(-d) moves with its argument EXACTLY as exp(bd) - 1 and adds 4 u relative; a result in or below the subnormal range has no relative
                accuracy, whence 2^-126 absolute:                                        bp = p (exp(bd) (1 + 4 u) - 1) + 2^-126
    H_p         term = p d (a product, or the fused multiply-add the sum ends in: u); c terms:
                    bH = sum_j (bp d + (p + bp) bd + u p d) + (c + 2) u H
    pbar_c      s = sum of keep values of p: sum bp + (keep + 2) u s; the division by keep rounds once:
                    bpbar = (sum_{p selected} bp_pc + (keep + 2) u s_c) / keep + u pbar_c + 2^-126
    lg_c        log max(., 2^-126) is monotone: it lies between its values at the ends of [pbar - bpbar, pbar + bpbar] (EXACT, no linearisation at the
                floor), and logf adds 4 u relative:                                      blg = max(lg_hi - lg, lg - lg_lo) + 4 u |lg|
    loss_i      t_c = pbar_c lg_c:  bt = bpbar |lg| + (pbar + bpbar) blg + u |t|;        bloss_i = sum_c bt_c + (c + 2) u sum_c |t_c|
    loss        n terms and the factor fl(1 / n) (u) and its product (u):                bloss = (sum_i bloss_i + (n + 4) u sum_i |loss_i|) / n
    g0_c        g0 = -(lg + 1) / keep: the addition and the division round once each:    bg0 = (blg + u |lg + 1|) / keep + u |g0|
    dot_p       sum_c p_pc g0_c:   bdot = sum_c (bp |g0| + (p + bp) bg0 + u |p g0|) + (c + 2) u sum_c |p g0|
    grad x_pj   r = g0_j - dot rounds once: br = bg0_j + bdot + u |r|; then two products and fl(1 / n), u each, and 2^-126 for a result in the subnormal range:
                    bgrad = (bp |r| + (p + bp) br) / n + 3 u |grad| + 2^-126
The entropy bound bH also says when a selection is DECIDED: where the float64 gap between the keep-th and the (keep + 1)-th smallest entropy of an image
exceeds twice its largest bH, an f32 ranking cannot differ from the float64 one (check_selection)."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
EXP_REL = 4.0 * U       # expf: 2 ulp
LOG_REL = 4.0 * U       # logf: 2 ulp
EPS64 = 2.0 ** -53      # the unit roundoff of float64


def select(H, keep):
    """bool [v]: the `keep` entries of smallest H, ties to the lower index, a non-finite H after every finite one (index ascending)."""
    H = np.asarray(H)
    fin = np.isfinite(H)
    order = sorted(range(len(H)), key=lambda p: (not fin[p], H[p] if fin[p] else 0.0, p))
    sel = np.zeros(len(H), dtype=bool)
    sel[order[:keep]] = True
    return sel


def views64(x):
    """(p, d, H, bp, bH) of logits x [..., c] (f32 values) in float64: the per-view part and its bounds."""
    x = np.asarray(x, dtype=np.float64)
    c = x.shape[-1]
    m = x.max(-1, keepdims=True)
    t = x - m
    e = np.exp(t)
    s = e.sum(-1, keepdims=True)
    es = (c + 2) * U + (e * (4 + np.abs(t)) * U).sum(-1, keepdims=True) / s
    L = np.log(s)
    lse = m + L
    blse = es + LOG_REL * np.abs(L) + U * np.abs(lse)
    d = lse - x
    bd = blse + U * d
    p = np.exp(-d)
    bp = p * (np.exp(bd) * (1 + EXP_REL) - 1) + TINY
    H = (p * d).sum(-1)
    bH = (bp * d + (p + bp) * bd + U * p * d).sum(-1) + (c + 2) * U * H
    return p, d, H, bp, bH


def _lg(pbar):
    return np.log(np.maximum(pbar, TINY))


def run64(x, keep, selection=None):
    """x f32 [n, v, c] -> dict of float64 values and bounds: loss, loss_i [n], grad [n, v, c], H [n, v], sel bool [n, v] (the float64 selection, or the
    GIVEN one), mean [n, c], and bloss, bloss_i, bgrad, bH, bmean."""
    x = np.asarray(x)
    n, v, c = x.shape
    p, d, H, bp, bH = views64(x)
    sel = np.stack([select(H[i], keep) for i in range(n)]) if selection is None else np.asarray(selection).astype(bool)
    assert sel.shape == (n, v) and (sel.sum(1) == keep).all(), "a selection holds exactly `keep` views of every image"
    w = sel[:, :, None].astype(np.float64)
    s = (p * w).sum(1)
    pbar = s / keep
    bpbar = ((bp * w).sum(1) + (keep + 2) * U * s) / keep + U * pbar + TINY
    lg = _lg(pbar)
    blg = np.maximum(_lg(pbar + bpbar) - lg, lg - _lg(pbar - bpbar)) + LOG_REL * np.abs(lg)
    t = pbar * lg
    bt = bpbar * np.abs(lg) + (pbar + bpbar) * blg + U * np.abs(t)
    loss_i = -t.sum(1)
    bloss_i = bt.sum(1) + (c + 2) * U * np.abs(t).sum(1)
    loss = loss_i.sum() / n
    bloss = (bloss_i.sum() + (n + 4) * U * np.abs(loss_i).sum()) / n
    g0 = -(lg + 1) / keep
    bg0 = (blg + U * np.abs(lg + 1)) / keep + U * np.abs(g0)
    pg = p * g0[:, None, :]
    dot = pg.sum(2, keepdims=True)
    bdot = (bp * np.abs(g0)[:, None, :] + (p + bp) * bg0[:, None, :] + U * np.abs(pg)).sum(2, keepdims=True) + (c + 2) * U * np.abs(pg).sum(2, keepdims=True)
    r = g0[:, None, :] - dot
    br = bg0[:, None, :] + bdot + U * np.abs(r)
    grad = p * r / n * w
    bgrad = ((bp * np.abs(r) + (p + bp) * br) / n + 3 * U * np.abs(grad) + TINY) * w      # (an unselected row is exactly zero: its bound is zero)
    gscale = p * (np.abs(g0)[:, None, :] + np.abs(pg).sum(2, keepdims=True)) / n * w       # the size of a gradient element BEFORE g_j - dot cancels
    return dict(loss=loss, loss_i=loss_i, grad=grad, H=H, sel=sel, mean=pbar, bloss=bloss, bloss_i=bloss_i, bgrad=bgrad, bH=bH, bmean=bpbar,
                gscale=gscale, lscale=np.abs(t).sum() / n)


def agree_rel(keep, c):
    """Relative tolerance for two float64 evaluations of the model written differently (test_host_view_entropy_ref.py: this file against torch autograd on
    the paper's formulation): each side adds c terms per view and keep views per class, (c + keep) EPS64 relative to the sums of absolute values, its exp
    and log are within an ulp (2 EPS64) and the chain lse -> p -> pbar -> log -> g -> dot passes the error on a handful of times: 8 (c + keep + 8) EPS64,
    relative to lscale for the loss and to gscale for a gradient element (the sizes before cancellation)."""
    return 8.0 * (c + keep + 8) * EPS64


def check_selection(x, keep, sel):
    """Asserts the selection statement of the issue for a kernel's (or an emulation's) selection `sel` [n, v] on logits x [n, v, c]; returns the number of
    images whose selection was DECIDED (it had to equal the float64 one)."""
    x = np.asarray(x)
    n, v, c = x.shape
    sel = np.asarray(sel).astype(bool)
    _, _, H, _, bH = views64(x)
    decided = 0
    for i in range(n):
        assert sel[i].sum() == keep, (i, sel[i])
        want = select(H[i], keep)
        if keep == v:
            assert sel[i].all()
            decided += 1
            continue
        srt = np.sort(H[i])
        slack = 2.0 * bH[i].max()
        if srt[keep] - srt[keep - 1] > slack:
            assert (sel[i] == want).all(), (i, sel[i], want, H[i])
            decided += 1
        else:
            assert (H[i][sel[i]] <= srt[keep] + slack).all(), (i, H[i], sel[i])      # none clearly behind the (keep + 1)-th smallest
        for a in range(v):       # bit-identical views: the lower index first
            for b in range(a + 1, v):
                if sel[i, b] and not sel[i, a]:
                    assert not np.array_equal(x[i, a], x[i, b]), (i, a, b)
    return decided


# ------------------------------------------------------------------------------------------ the kernel's operation order in f32
def _wave_sum(vals):
    """The DPP tree of common.h's wave_sum on 64 f32 lane values: xor 1, xor 2, the half mirror, the mirror of each 16-lane row, then (r0 + r1) + (r2 + r3)."""
    v = np.asarray(vals, dtype=np.float32).copy()
    lanes = np.arange(64)
    for perm in (lanes ^ 1, lanes ^ 2, (lanes & ~7) | (7 - (lanes & 7)), (lanes & ~15) | (15 - (lanes & 15))):
        v = (v + v[perm]).astype(np.float32)
    return np.float32(np.float32(v[0] + v[16]) + np.float32(v[32] + v[48]))


def _strided_sum(terms, lanes):
    """Lane l adds terms[l], terms[l + lanes], ... in ascending order (f32); returns the `lanes` partial sums."""
    terms = np.asarray(terms, dtype=np.float32)
    out = np.zeros(lanes, dtype=np.float32)
    for j0 in range(0, len(terms), lanes):
        chunk = terms[j0:j0 + lanes]
        out[:len(chunk)] = (out[:len(chunk)] + chunk).astype(np.float32)
    return out


def run_f32(x, keep):
    """The kernel's sequence of operations on the host in f32 (numpy's expf / logf, no fused multiply-add): dict(loss, grad, H, sel, mean)."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    n, v, c = x.shape
    inv_n = f(1.0) / f(n)
    H, lse = np.zeros((n, v), f), np.zeros((n, v), f)
    sel = np.zeros((n, v), bool)
    mean, grad, loss_i = np.zeros((n, c), f), np.zeros((n, v, c), f), np.zeros(n, f)
    for i in range(n):
        for p in range(v):
            m = x[i, p].max()
            s = _wave_sum(_strided_sum(np.exp((x[i, p] - m).astype(f)).astype(f), 64))
            lse[i, p] = f(m + np.log(s).astype(f))
            d = (lse[i, p] - x[i, p]).astype(f)
            H[i, p] = _wave_sum(_strided_sum((np.exp(-d).astype(f) * d).astype(f), 64))
        sel[i] = select(H[i], keep)
        s = np.zeros(c, f)
        for p in np.flatnonzero(sel[i]):
            s = (s + np.exp((x[i, p] - lse[i, p]).astype(f)).astype(f)).astype(f)
        pbar = (s / f(keep)).astype(f)
        lg = np.log(np.maximum(pbar, f(TINY))).astype(f)
        parts = _strided_sum(-(pbar * lg).astype(f), 256)
        w = [_wave_sum(parts[64 * k:64 * k + 64]) for k in range(4)]
        loss_i[i] = f(f(f(w[0] + w[1]) + w[2]) + w[3])
        g = (-(lg + f(1.0)).astype(f) / f(keep)).astype(f)
        mean[i] = pbar
        for p in np.flatnonzero(sel[i]):
            pp = np.exp((x[i, p] - lse[i, p]).astype(f)).astype(f)
            dot = _wave_sum(_strided_sum((pp * g).astype(f), 64))
            grad[i, p] = ((pp * (g - dot).astype(f)).astype(f) * inv_n).astype(f)
    acc = loss_i[0]
    for i in range(1, n):
        acc = f(acc + loss_i[i])
    return dict(loss=f(acc * inv_n), loss_i=loss_i, grad=grad, H=H, sel=sel, mean=mean)


def worst_ratios(got, x, keep):
    """{output: worst |err| / bound} of a result dict (loss, grad, H, mean; sel gives the selection the reference is evaluated ON), asserting nothing."""
    ref = run64(x, keep, selection=got["sel"])
    out = {}
    for name, bname in (("loss", "bloss"), ("grad", "bgrad"), ("H", "bH"), ("mean", "bmean")):
        err = np.abs(np.asarray(got[name], dtype=np.float64) - ref[name])
        bound = np.asarray(ref[bname], dtype=np.float64)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        out[name] = float(np.max(ratio))
    return out


# ------------------------------------------------------------------------------------------ inputs
KINDS = ("normal", "saturated", "uniform", "duplicates")
NS, VS, CS = (1, 3), (1, 2, 5, 16, 17, 64), (1, 2, 63, 64, 65, 102, 1000)
C_LIMIT = 16000


def keeps(v):
    return sorted({1, max(1, int(0.1 * v)), v})


def logits(kind, n, v, c, seed=0):
    """f32 [n, v, c].  normal: N(0, 1).  saturated: 30 N(0, 1) -- a saturated softmax, whole classes of pbar under the floor.  uniform: constant rows (every
    entropy log c: the selection is all ties).  duplicates: N(0, 1) with bit-identical copies of views (forced ties between rows that are not constant)."""
    g = np.random.default_rng([seed, n, v, c, KINDS.index(kind)])
    x = g.standard_normal((n, v, c)).astype(np.float32)
    if kind == "saturated":
        x = (np.float32(30.0) * x).astype(np.float32)
    elif kind == "uniform":
        x = np.broadcast_to(g.standard_normal((n, v, 1)).astype(np.float32), (n, v, c)).copy()
    elif kind == "duplicates":
        for i in range(n):
            for p in range(1, v):
                if p % 3 != 1:
                    x[i, p] = x[i, int(g.integers(0, p))]
    return x


def cases():
    """Every (kind, n, v, c) of the GPU test; each runs all of keeps(v).  The case at the c limit comes last."""
    out = [(kind, n, v, c) for kind in KINDS for n in NS for v in VS for c in CS]
    return out + [("normal", 1, 5, C_LIMIT)]


def case_id(case):
    return "-".join(str(x) for x in case)


# ------------------------------------------------------------------------------------------ the planted pool of the issue
def planted_accuracies(seed, rho=0.5, lr=5e-3, scale=30.0):
    """A planted pool, not a dataset (view_mode_ref.planted_pool: 2 000 images, 20 classes, e = 64, V = 16, half the views of an image missed, view 0
    clean, imperfect text), in float64: the accuracy of the single view, of the mean of the views' probabilities, of the MTA mode (view_mode_ref) and of
    TPT -- per image, the tuned parameter is a residual R [classes, e] on the text prototypes (t = normalise(txt + R)), the episode is ONE normalised-
    gradient step on the marginal entropy of the keep = max(1, floor(rho V)) most confident views from a zero state (the first Adam step:
    R = -lr g / (|g| + 1e-8), element by element), and the image is classified by view 0 under its own t."""
    import view_mode_ref as VM
    base = VM.planted_accuracies(seed)
    f, _, txt, labels = VM.planted_pool(seed)
    fn = (f / f.norm(dim=2, keepdim=True)).numpy()
    txt, labels = txt.numpy(), labels.numpy()
    n, v, e = fn.shape
    keep = max(1, int(np.floor(rho * v)))
    x = scale * fn @ txt.T                                       # [n, v, c]
    # the gradient of every image's OWN loss (n = 1 each): run64's gradient carries 1 / n, which is undone
    ref = run64(x, keep)
    gl = ref["grad"] * n                                         # [n, v, c]
    gt = scale * np.einsum("nvc,nve->nce", gl, fn)               # d loss_i / d t, t = txt (unit rows)
    gr = gt - (gt * txt[None]).sum(2, keepdims=True) * txt[None]      # through the normalisation at |txt| = 1
    R = -lr * gr / (np.abs(gr) + 1e-8)
    t = txt[None] + R
    t = t / np.linalg.norm(t, axis=2, keepdims=True)
    pred = np.einsum("ne,nce->nc", fn[:, 0], t).argmax(1)
    return dict(single=base["single"], mean_probability=base["mean_probability"], mode=base["mode"], tpt=float((pred == labels).mean()))
