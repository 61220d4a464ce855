"""float64 reference, bound and inputs for the multi-view mode kernel (csrc/view_mode.hip), shared by the GPU tests and shown to hold for an f32 emulation
on the host (tests/test_host_view_mode_ref.py).  Everything works on torch tensors of any device.  u = 2^-24 (the unit roundoff of f32; one ulp is 2 u).
Every term below follows from the inputs, u and the documented 2-ulp accuracy of expf alone; nothing in it is measured.  The reference runs in float64 on
the SAME f32 inputs (view_emb, view_probs, the f32 parameters, the start state), so only the arithmetic differs.  Sums are bounded for ANY order of
accumulation (t terms: t u relative to the sum of the absolute values), so the bound does not know how the kernel or the emulation adds.

THE RECURSION (include/grip_amd.h).  u_p = f_p / |f_p|, G = U U^T, d2 = max(0, 2 - 2 G); h2_p = max(mean of the r smallest d2_pq (q != p), floor),
r = max(1, floor(rho (V - 1))); A = S S^T; from (m, y):  k_p = exp(-|u_p - m|^2 / (2 h2_p));  `inner` times y = softmax_p((k_p + lam (A y)_p) / lam_y);
m = sum_p y_p k_p u_p / max(sum_p y_p k_p, 2^-126).

THE BOUND, first order in u with a unit of room per line, carried from step to step (bm [e] bounds |m - m64|, by [V] bounds |y - y64|).
    u_pd        |f|^2 is a sum of e squares: (e + 2) u relative; its root halves that, the root, the reciprocal and the product round once each:
                    eu = (e / 2 + 5) u,   |u_pd - u64_pd| <= eu |u_pd|
    G_pq        each operand carries eu, the contraction (e + 2) u, all relative to Pabs_pq = sum_d |u_pd u_qd| (<= 1):  bG = (2 eu + (e + 2) u) Pabs
    d2_pq       2 G is exact, the subtraction rounds once, the clamp at 0 is 1-Lipschitz:    bd2 = 2 bG + u d2
    h2_p        the sum of the r smallest entries of a row is a minimum over r-subsets of subset sums, so it moves by at most the largest subset sum of
                the entries' bounds -- NO exclusion of near-ties is needed, the sum is continuous where members swap:
                    bh2_p = (sum of the r largest bd2_pq (q != p) + (r + 1) u S_p) / r        (S_p the sum; r - 1 additions and the division; the floor is 1-Lipschitz)
    A_pq        bA = (c + 2) u sum_c |s_pc s_qc|
    k_p         t_d = u_pd - m_d:  bt_d = eu |u_pd| + bm_d + u |t_d|;   D_p = sum_d t_d^2:  bD = 2 sum_d |t_d| bt_d + sum_d bt_d^2 + (e + 2) u D
                a_p = D_p / (2 h2_p) lies in [(D - bD)+ / (2 (h2 + bh2)), (D + bD) / (2 max(h2 - bh2, floor))] widened by 2 u (the division); exp is monotone,
                so k lies between the exponentials of the ends (EXACT, no linearisation); expf adds 4 u relative:   bk = max(k_hi - k, k - k_lo) + 5 u k + 2^-120
    y_p         g_p = sum_q A_pq y_q:  bg = sum_q (bA_pq (y_q + by_q) + A_pq by_q) + (V + 2) u sum_q |A_pq y_q|
                arg_p = (k_p + lam g_p) / lam_y:  barg = (bk + lam bg) / lam_y + 3 u |arg_p|
                the softmax subtracts its maximum first and moves EXACTLY within the monotone interval of tests/sinkhorn_ref.py / gmm_ref.py under
                barg' = barg + u (max - arg) + 2 u max barg;  its own arithmetic:   by = max(hi - y, y - lo) + (V + 8) u y + 2^-126
    m_d         w_p = y_p k_p:  bw = by k + y bk + by bk + u w;   den = sum_p w_p:  bden = sum bw + (V + 1) u den
                num_d = sum_p w_p u_pd:  bnum_d = sum_p (bw_p + (w_p + bw_p) eu) |u_pd| + (V + 2) u sum_p w_p |u_pd|
                with bden < den / 2 (else the bound is VACUOUS: infinity):   bm_d = (bnum_d + |m_d| bden) / (den - bden) + 2 u |m_d| + 2^-126
The start state carries bm = eu |u_0d| (no mode_in) and by = u / V (no y_in), else zero.  The bound of y grows by up to 2 lam max(A) / lam_y per inner
iteration (40 max(A) at the defaults): over a free run at the defaults it is vacuous wherever the views' probabilities are peaked, which check_run REPORTS
(the share of elements whose bound says nothing); the tight checks are the forced single steps (outer = 1, inner = 1 from a state of the float64
trajectory), and GENTLE below is a parameter set under which the bound stays non-vacuous for a whole run on these inputs."""
import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
DEFAULTS = dict(rho=0.3, lam=4.0, lam_y=0.2, h2_floor=2.0 ** -20, outer=5, inner=3)
GENTLE = dict(rho=0.3, lam=0.25, lam_y=1.0, h2_floor=2.0 ** -20, outer=3, inner=2)       # non-vacuous for the whole run (test_host_view_mode_ref.py shows it)


def _f32(x):
    return float(np.float32(x))


def rank_count(rho, v):
    return max(1, int(math.floor(_f32(rho) * (v - 1))))


def _offdiag(x, fill):
    v = x.shape[-1]
    return x.masked_fill(torch.eye(v, dtype=torch.bool, device=x.device), fill)


def setup64(f, s, rho, h2_floor):
    """The step-independent part in float64 with its bounds: dict(u, eu, h2, bh2, A, bA)."""
    n, v, e = f.shape
    f = f.double()
    u = f / f.norm(dim=2, keepdim=True)
    eu = (e / 2 + 5) * U
    ua = u.abs()
    g = u @ u.transpose(1, 2)
    bg = (2 * eu + (e + 2) * U) * (ua @ ua.transpose(1, 2))
    d2 = (2 - 2 * g).clamp_min(0.0)
    bd2 = 2 * bg + U * d2
    r = rank_count(rho, v)
    ssum = _offdiag(d2, float("inf")).sort(dim=2).values[..., :r].sum(2)
    top = _offdiag(bd2, 0.0).topk(r, dim=2).values.sum(2)
    floor = _f32(h2_floor)
    h2 = (ssum / r).clamp_min(floor)
    bh2 = (top + (r + 1) * U * ssum) / r + TINY
    out = dict(u=u, eu=eu, h2=h2, bh2=bh2, floor=floor, A=None, bA=None, v=v, e=e)
    if s is not None:
        s = s.double()
        out["A"] = s @ s.transpose(1, 2)
        out["bA"] = (s.shape[2] + 2) * U * (s.abs() @ s.abs().transpose(1, 2))
    return out


def start64(st, mode_in, y_in):
    """(m, y, bm, by) of the start state."""
    u, v = st["u"], st["v"]
    if mode_in is None:
        m, bm = u[:, 0].clone(), st["eu"] * u[:, 0].abs()
    else:
        m, bm = mode_in.double().clone(), torch.zeros_like(u[:, 0])
    if y_in is None:
        y = torch.full(u.shape[:2], 1.0 / v, dtype=torch.float64, device=u.device)
        by = torch.full_like(y, U / v)
    else:
        y, by = y_in.double().clone(), torch.zeros(u.shape[:2], dtype=torch.float64, device=u.device)
    return m, y, bm, by


def _softmax_interval(arg, barg, v):
    mx = arg.max(dim=1, keepdim=True).values
    ba = (barg + U * (mx - arg) + 2 * U * barg.max(dim=1, keepdim=True).values).clamp_max(700.0)
    y = torch.softmax(arg, dim=1)
    up, dn = y * torch.exp(ba), y * torch.exp(-ba)
    hi = up / (up + (dn.sum(1, keepdim=True) - dn).clamp_min(0.0)).clamp_min(TINY)
    lo = dn / (dn + (up.sum(1, keepdim=True) - up).clamp_min(0.0)).clamp_min(TINY)
    return y, torch.maximum(hi - y, y - lo).clamp_min(0.0) + (v + 8) * U * y + TINY


def step64(st, m, y, bm, by, lam, lam_y, inner):
    """One outer step in float64 with its bounds: (m, y, bm, by)."""
    u, eu, h2, bh2, v, e = st["u"], st["eu"], st["h2"], st["bh2"], st["v"], st["e"]
    lam, lam_y = _f32(lam), _f32(lam_y)
    bm = bm.clamp_max(1e30)       # (a vacuous bound stays vacuous, and 0 x infinity never arises below)
    t = u - m[:, None, :]
    bt = eu * u.abs() + bm[:, None, :] + U * t.abs()
    d = (t * t).sum(2)
    bd = 2 * (t.abs() * bt).sum(2) + (bt * bt).sum(2) + (e + 2) * U * d
    a = d / (2 * h2)
    a_lo = (d - bd).clamp_min(0.0) / (2 * (h2 + bh2)) * (1 - 2 * U)
    a_hi = (d + bd) / (2 * (h2 - bh2).clamp_min(st["floor"])) * (1 + 2 * U)
    k = torch.exp(-a)
    bk = torch.maximum(torch.exp(-a_lo) - k, k - torch.exp(-a_hi)).clamp_min(0.0) + 5 * U * k + 2.0 ** -120
    A, bA = st["A"], st["bA"]
    for _ in range(inner):
        if A is None:
            arg, barg = k / lam_y, bk / lam_y
        else:
            g = (A @ y[:, :, None])[:, :, 0]
            bg = (bA @ (y + by)[:, :, None] + A @ by[:, :, None] + (v + 2) * U * (A.abs() @ y.abs()[:, :, None]))[:, :, 0]
            arg, barg = (k + lam * g) / lam_y, (bk + lam * bg) / lam_y
        barg = barg + 3 * U * arg.abs()
        y, by = _softmax_interval(arg, barg, v)
    w = y * k
    bw = by * k + y * bk + by * bk + U * w
    den = w.sum(1)
    bden = bw.sum(1) + (v + 1) * U * den
    ua = u.abs()
    num = (w[:, :, None] * u).sum(1)
    bnum = ((bw + (w + bw) * eu)[:, :, None] * ua).sum(1) + (v + 2) * U * (w[:, :, None] * ua).sum(1)
    m = num / den.clamp_min(TINY)[:, None]
    ok = (bden < den / 2) & (den > 2 * TINY)
    room = torch.where(ok, den - bden, torch.ones_like(den))
    bm = (bnum + m.abs() * bden[:, None]) / room[:, None] + 2 * U * m.abs() + TINY
    bm = torch.where(ok[:, None], bm, torch.full_like(bm, float("inf")))
    return m, y, bm, by


def run64(f, s, rho, lam, lam_y, h2_floor, outer, inner, mode_in=None, y_in=None, trajectory=False):
    """(m64, y64, h2_64, bm, by, bh2) of the recursion; with trajectory=True also the list of the (m, y) states BEFORE every outer step, rounded to f32."""
    st = setup64(f, s, rho, h2_floor)
    m, y, bm, by = start64(st, mode_in, y_in)
    states = []
    for _ in range(outer):
        states.append((m.float(), y.float()))
        m, y, bm, by = step64(st, m, y, bm, by, lam, lam_y, inner)
    out = (m, y, st["h2"], bm, by, st["bh2"])
    return out + (states,) if trajectory else out


def vacuous_share(m64, bm, by):
    """The share of the elements of (mode, y) whose bound says nothing: not finite, or as large as the value's own range (|m_d| <= 1, y_p <= 1)."""
    bad_m = ~torch.isfinite(bm) | (bm >= 1.0)
    bad_y = ~torch.isfinite(by) | (by >= 1.0)
    return float((bad_m.sum() + bad_y.sum()) / (bad_m.numel() + bad_y.numel()))


def check_run(f, s, params, mode_in, y_in, mode, y, h2):
    """Assert every element of mode, y and h2 (h2 may be None) against float64 under the carried bound; returns (worst |err| / bound, vacuous share)."""
    m64, y64, h64, bm, by, bh2 = run64(f, s, mode_in=mode_in, y_in=y_in, **params)
    worst = 0.0
    for name, got, want, b in (("mode", mode, m64, bm), ("y", y, y64, by), ("h2", h2, h64, bh2)):
        if got is None:
            continue
        err = (got.double() - want).abs()
        ratio = float((err / b).max())
        assert torch.isfinite(got).all() and (err <= b).all(), f"view_mode: |{name} - {name}64| is {ratio:.2f} x its bound"
        worst = max(worst, ratio)
    return worst, vacuous_share(m64, bm, by)


def run_f32(f, s, rho, lam, lam_y, h2_floor, outer, inner, mode_in=None, y_in=None):
    """An f32 emulation of the kernel in torch (no fused multiply-add, torch's own summation orders): what the checker must accept.  (mode, y, h2)."""
    n, v, e = f.shape
    one = torch.ones((), dtype=torch.float32)
    u = f * (one / torch.sqrt((f * f).sum(2, keepdim=True)))
    d2 = (2 - 2 * (u @ u.transpose(1, 2))).clamp_min(0.0)
    r = rank_count(rho, v)
    sel = _offdiag(d2, float("inf")).sort(dim=2).values[..., :r]
    ssum = sel[..., 0].clone()
    for j in range(1, r):
        ssum = ssum + sel[..., j]
    h2 = (ssum / np.float32(r)).clamp_min(_f32(h2_floor))
    A = None if s is None else s @ s.transpose(1, 2)
    m = u[:, 0].clone() if mode_in is None else mode_in.clone()
    y = torch.full((n, v), 1.0, dtype=torch.float32) / np.float32(v) if y_in is None else y_in.clone()
    lam, lam_y = torch.tensor(lam, dtype=torch.float32), torch.tensor(lam_y, dtype=torch.float32)
    for _ in range(outer):
        t = u - m[:, None, :]
        k = torch.exp(-((t * t).sum(2) / (2 * h2)))
        for _ in range(inner):
            arg = k if A is None else k + lam * (A @ y[:, :, None])[:, :, 0]
            arg = arg / lam_y
            x = torch.exp(arg - arg.max(dim=1, keepdim=True).values)
            y = x / x.sum(1, keepdim=True)
        w = y * k
        m = (w[:, :, None] * u).sum(1) / w.sum(1).clamp_min(TINY)[:, None]
    return m, y, h2


def run_loops(f, s, rho, lam, lam_y, h2_floor, outer, inner):
    """The recursion restated with plain Python loops and `math` on lists (float64, from the defaults' start state): an independent second opinion
    for run64 on small shapes.  (mode, y, h2) as nested lists."""
    n, v, e = f.shape
    lam, lam_y, floor = _f32(lam), _f32(lam_y), _f32(h2_floor)
    r = rank_count(rho, v)
    modes, ys, h2s = [], [], []
    for i in range(n):
        fi = [[float(x) for x in row] for row in f[i].tolist()]
        si = None if s is None else [[float(x) for x in row] for row in s[i].tolist()]
        u = []
        for p in range(v):
            nr = math.sqrt(sum(x * x for x in fi[p]))
            u.append([x / nr for x in fi[p]])
        h2 = []
        for p in range(v):
            ds = sorted((max(0.0, 2 - 2 * sum(a * b for a, b in zip(u[p], u[q]))), q) for q in range(v) if q != p)
            h2.append(max(sum(d for d, _ in ds[:r]) / r, floor))
        m, y = list(u[0]), [1.0 / v] * v
        for _ in range(outer):
            k = [math.exp(-sum((a - b) ** 2 for a, b in zip(u[p], m)) / (2 * h2[p])) for p in range(v)]
            for _ in range(inner):
                arg = []
                for p in range(v):
                    g = 0.0 if si is None else sum(sum(a * b for a, b in zip(si[p], si[q])) * y[q] for q in range(v))
                    arg.append((k[p] + lam * g) / lam_y)
                mx = max(arg)
                x = [math.exp(a - mx) for a in arg]
                y = [a / sum(x) for a in x]
            den = max(sum(y[p] * k[p] for p in range(v)), TINY)
            m = [sum(y[p] * k[p] * u[p][d] for p in range(v)) / den for d in range(e)]
        modes.append(m)
        ys.append(y)
        h2s.append(h2)
    return modes, ys, h2s


# ------------------------------------------------------------------------------------------ inputs and cases
KINDS = ("plain", "dup", "copy0", "outlier", "scale")


def inputs(n, v, e, c, kind, seed):
    """(view_emb f32 [n, v, e], view_probs f32 [n, v, c] or None): views = a unit centre + 0.5 x unit noise; probabilities = softmax of 3 x randn logits with
    4 on the image's class.  "dup": the second half of the views (at least view 1) are bit-copies of one another -- their r smallest distances are zero and
    h2 sits on the floor; "copy0": view 1 is a bit-copy of view 0; "outlier": every third view (never view 0) is an unrelated direction with unrelated
    probabilities; "scale": every view is multiplied by its own 10^U(-3, 3) (un-normalised inputs of mixed scale)."""
    g = torch.Generator().manual_seed(seed)

    def unit(*shape):
        x = torch.randn(*shape, generator=g, dtype=torch.float64)
        return x / x.norm(dim=-1, keepdim=True)
    f = unit(n, 1, e) + 0.5 * unit(n, v, e)
    logits = None
    if c is not None:
        logits = 3 * torch.randn(n, v, c, generator=g, dtype=torch.float64)
        cls = torch.randint(0, c, (n,), generator=g)
        logits[torch.arange(n), :, cls] += 4
    if kind == "dup":
        h = min(max(1, v // 2), v - 1)
        f[:, h:] = f[:, h:h + 1]
        if logits is not None:
            logits[:, h:] = logits[:, h:h + 1]
    elif kind == "copy0":
        f[:, 1] = f[:, 0]
    elif kind == "outlier":
        idx = torch.arange(2, v, 3)
        f[:, idx] = unit(n, len(idx), e)
        if logits is not None:
            logits[:, idx] = 3 * torch.randn(n, len(idx), c, generator=g, dtype=torch.float64)
    elif kind == "scale":
        f = f * 10 ** (6 * torch.rand(n, v, 1, generator=g, dtype=torch.float64) - 3)
    return f.float(), None if logits is None else torch.softmax(logits, dim=2).float()


# every v (one tile, part of one, several, 64), every e, every c and none, every n; the corners; then the special pools on two shapes
SHAPES = ([(3, v, 512, 102) for v in (2, 3, 16, 33, 64)] + [(3, 16, e, 102) for e in (64, 1024)] + [(3, 16, 512, c) for c in (1, 5, 130, None)] +
          [(n, 16, 512, 102) for n in (1, 17)] + [(17, 64, 1024, 130), (1, 2, 64, 1), (17, 33, 1024, None), (3, 3, 64, 5)])
CASES = [(*shape, "plain") for shape in SHAPES] + [(n, v, e, c, kind) for (n, v, e, c) in ((3, 16, 512, 102), (3, 33, 64, None), (3, 2, 64, 5))
                                                   for kind in KINDS[1:]]


def case_inputs(case):
    n, v, e, c, kind = case
    return inputs(n, v, e, c, kind, seed=1000 * n + 10 * v + e + (c or 0))


def case_id(case):
    return "-".join(str(x) for x in case)


# ------------------------------------------------------------------------------------------ the planted pool of the issue
def planted_pool(seed, n=2000, classes=20, e=64, v=16, view_sd=2.0, text_sd=1.5, scale=30.0):
    """(view_emb f64 [n, v, e], view_probs f64 [n, v, classes], txt f64 [classes, e], labels [n]).  Class prototypes are random unit vectors; a clean view
    is its class's prototype + view_sd x unit noise; half of the views 1 .. v - 1 are "crops that missed": ANOTHER class's prototype (drawn per view) +
    the same noise; view 0 is always clean.  The text prototypes are imperfect: prototype + text_sd x unit noise, normalised."""
    g = torch.Generator().manual_seed(seed)

    def unit(*shape):
        x = torch.randn(*shape, generator=g, dtype=torch.float64)
        return x / x.norm(dim=-1, keepdim=True)
    proto = unit(classes, e)
    txt = proto + text_sd * unit(classes, e)
    txt = txt / txt.norm(dim=1, keepdim=True)
    labels = torch.arange(n) % classes
    src = labels[:, None].repeat(1, v)
    missed = torch.zeros(n, v, dtype=torch.bool)
    for i in range(n):
        missed[i, 1 + torch.randperm(v - 1, generator=g)[: v // 2]] = True
    other = (labels[:, None] + torch.randint(1, classes, (n, v), generator=g)) % classes
    src = torch.where(missed, other, src)
    f = proto[src] + view_sd * unit(n, v, e)
    fn = f / f.norm(dim=2, keepdim=True)
    probs = torch.softmax(scale * (fn @ txt.T), dim=2)
    return f, probs, txt, labels


def planted_accuracies(seed, params=None):
    """The four columns of the planted experiment in float64: single view, mean of the unit view embeddings, the mode, mean of the views' probabilities."""
    p = dict(DEFAULTS if params is None else params)
    f, probs, txt, labels = planted_pool(seed)
    u = f / f.norm(dim=2, keepdim=True)

    def acc(feat):
        return float(((feat @ txt.T).argmax(1) == labels).double().mean())
    st = setup64(f, probs, p["rho"], p["h2_floor"])
    m, y, bm, by = start64(st, None, None)
    for _ in range(p["outer"]):
        m, y, bm, by = step64(st, m, y, bm, by, p["lam"], p["lam_y"], p["inner"])
    return dict(single=acc(u[:, 0]), mean_embedding=acc(u.mean(1)), mode=acc(m), mean_probability=float((probs.mean(1).argmax(1) == labels).double().mean()))
