"""Float64 references, per-element error bounds and case tables of the trained linear probe (csrc/linear_probe.hip; models/probe_models.py), shared by
the CPU tests (tests/test_host_probe_ref.py) and the GPU tests.  Every bound is derived from the inputs, u = 2^-24 and the 1-ulp (= 2 u) accuracy of expf
and logf alone, in the manner of tests/gda_ref.py and tests/soft_ce_ref.py: nothing in this file comes from a measurement of the kernels.

Model of the arithmetic (include/grip_amd.h).  The f32 MFMA and fmaf are exact products followed by ONE rounding of the sum, so a chain of k accumulations
obeys |err| <= gamma_k sum |terms| whatever the order; + - * / are correctly rounded.  Per element, first order, each factor (1 + small) kept as 1.01:

  score   s_ic = u_i . W_c, one chain over e:                     (e + 4) u on P_ic = sum_d |u_id W_cd|
  logit   v = fmaf(scale, s, b), x = base + v:                    dx = scale (e + 4) u P + u |v| + u |x|   (+ what a perturbed (W, b) adds: fit_bound)
  shift   z = x - max (the max is exact on the computed x; lse and softmax do not depend on the shift): dz = dx + u (|z| + dx + max_k dx_k)
  exp     E = expf(z):                                            dE = E expm1(dz) + 2 u E e^dz + 2^-126
  sum     S = sum_c E_c, ceil(c / 8) terms a lane + 3 butterfly:  dS = sum dE + gamma_{ceil(c/8)+3} sum (E + dE)
  softmax p = E / S:                                              dp = (dE + p dS) / (S - dS) + u p
  lse     = max + logf(S):                                        dl = dS / (S - dS) + 2 u log S + u |lse|
  T       = sum_c t_c ascending (soft rows; 1 exactly on hard):   dT = gamma_c T
  t . x   hard: x_y, dx_y; soft: ceil(c / 8) + 3 fmaf/adds:       dd = sum t dx + gamma_{ceil(c/8)+3} sum t (|x| + dx)
  row     r fmaf(T, lse, -t.x):                                   dr = r (T dl + dT (|lse| + dl) + dd + 2 u (|T lse| + |t.x|))
  g       r fmaf(T, p, -t):                                       dg = r (T dp + dT (p + dp) + 2 u (T p + t + T dp))
  loss    norm x (32 rows a workgroup, ceil(blocks / 256) strided, 256 in order): norm (sum dr + gamma_{32+ceil(blocks/256)+257} sum (|row| + dr))
  grad_w  fl(norm scale) sum_i g_ic u_id over the fixed row partition:  norm scale (sum_i dg |u| + gamma_k sum_i (|g| + dg) |u|) + 2 u |grad_w|,
          k = rows of a slice + slices + 1;  grad_b the same with |u| = 1 and one product.
"""
import numpy as np
import torch

from gda_ref import TINY, U, case_id, f64, gamma  # noqa: F401  (case_id is re-exported to the tests)
import gda_ref

SCORE_ROWS, ROWS = 32, 64      # csrc/linear_probe.hip PB_BM / PB_ROWS (engine.PROBE_SCORE_ROWS / PROBE_ROWS)
SLACK = 1.01


def slice_cap(c, e):
    return min(64, max(4, 1024 // (-(-c // 128) * -(-e // 64))))


def split(n, c, e):
    """(rows per slice, slices) of the contraction's fixed partition (csrc/linear_probe.hip, probe_plan)."""
    nch = -(-n // ROWS)
    per = -(-nch // slice_cap(c, e))
    return per * ROWS, -(-nch // per)


# ------------------------------------------------------------------------------------------ cases
KINDS = ("hard", "soft", "mixed", "ignored", "null", "big", "zerosoft")
_NS, _CS, _ES = (1, 5, 63, 64, 65, 257, 1000), (1, 3, 64, 65, 102, 257, 1000), (4, 36, 512, 1024)
CASES = [(n, _CS[(i + 2 * j) % 7], _ES[(i + j) % 4], KINDS[(3 * i + j) % 7]) for i, n in enumerate(_NS) for j in range(4)]
CASES += [
    (33, 102, 36, "mixed"),         # one row beyond a workgroup of the score kernel (32 rows)
    (4097, 3, 36, "mixed"),         # slice cap 64: 65 chunks -> 2 chunks a slice, 33 slices, the last one a single row
    (513, 1000, 1024, "hard"),      # slice cap 8: 9 chunks -> 2 chunks a slice, 5 slices, the last one a single row
    (8225, 3, 4, "zerosoft"),       # 258 workgroups of the score kernel: the strided loss sum takes a second term in two of its 256 chains
    (130, 257, 512, "big"),         # c > 256: one class tile per staging of the rows, five of them
    (70, 129, 68, "soft"),          # c just over the contraction's 128-class tile, e just over its 64-column tile
]


def probe_inputs(n, c, e, kind, seed):
    """dict(F f32 [n, e] unit rows, W [c, e], b [c] or None, base [n, c] or None, y int32 [n], soft [n, c] or None, r [n] or None, scale, norm) on the CPU.
    hard / soft / mixed: the rows' targets; `ignored`: no soft matrix, labels -1 and c + 5 and weights 0 from row 1 on, those rows NaN in F and base;
    `null`: base, b and r are NULL (mixed rows); `big`: logits of magnitude 100; `zerosoft`: mixed, and the last soft row's target is all zeros."""
    g = torch.Generator().manual_seed(seed)
    F = torch.nn.functional.normalize(torch.randn(n, e, generator=g, dtype=torch.float64), dim=1).float()
    big = kind == "big"
    W = torch.randn(c, e, generator=g) * (0.6 if big else 0.05)
    b = torch.randn(c, generator=g) * (20.0 if big else 0.5)
    base = torch.randn(n, c, generator=g) * (60.0 if big else 5.0)
    y = torch.randint(0, c, (n,), generator=g).to(torch.int32)
    r = torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(0.37), torch.tensor(1.0))
    soft = torch.softmax(torch.randn(n, c, generator=g) * 2, dim=1) * (0.5 + torch.rand(n, 1, generator=g))      # non-negative, rows do NOT sum to one
    pick = torch.rand(n, generator=g)
    if kind == "hard" or kind == "big":
        soft = None
    elif kind == "soft":
        y[:] = -1
    elif kind in ("mixed", "null", "zerosoft"):
        y[pick < 0.5] = -1
        if kind == "zerosoft":
            y[n - 1] = -1
            soft[n - 1] = 0
    elif kind == "ignored":
        soft = None
        idx = torch.arange(n)
        y[(idx >= 1) & (pick < 0.2)] = -1
        y[(idx >= 1) & (pick >= 0.2) & (pick < 0.35)] = c + 5
        r[(idx >= 1) & (pick >= 0.35) & (pick < 0.5)] = 0.0
        dead = (idx >= 1) & (pick < 0.5)
        F[dead] = float("nan")
        base[dead] = float("nan")
    if kind == "null":
        b = base = r = None
    inp = dict(F=F, W=W, b=b, base=base, y=y, soft=soft, r=r, scale=100.0 if not big else 30.0, norm=1.0)
    inp["norm"] = float(np.float32(1.0 / _prep(inp)["r"].sum()))
    return inp


def _prep(inp):
    F, W = f64(inp["F"]), f64(inp["W"])
    (n, e), c = F.shape, W.shape[0]
    y = inp["y"].detach().cpu().numpy().astype(np.int64)
    has_soft = inp["soft"] is not None
    r = np.ones(n) if inp["r"] is None else f64(inp["r"])
    ok = (((y >= 0) & (y < c)) | ((y == -1) & has_soft)) & (r != 0)
    r = np.where(ok, r, 0.0)
    F = np.where(ok[:, None], F, 0.0)                                       # a row that does not contribute is not read
    base = np.zeros((n, c)) if inp["base"] is None else np.where(ok[:, None], f64(inp["base"]), 0.0)
    b = np.zeros(c) if inp["b"] is None else f64(inp["b"])
    t = np.zeros((n, c))
    hard, softrow = ok & (y >= 0), ok & (y == -1)
    t[hard, y[hard]] = 1.0
    if has_soft:
        t[softrow] = f64(inp["soft"])[softrow]
    return dict(F=F, W=W, b=b, base=base, y=y, r=r, t=t, hard=hard, softrow=softrow, ok=ok, n=n, c=c, e=e,
                s=float(np.float32(inp["scale"])), nu=float(np.float32(inp["norm"])))


def _forward(p):
    v = p["s"] * (p["F"] @ p["W"].T) + p["b"][None, :]
    x = p["base"] + v
    m = x.max(1)
    E = np.exp(x - m[:, None])
    S = E.sum(1)
    lse = m + np.log(S)
    T = p["t"].sum(1)
    dot = (p["t"] * x).sum(1)
    return dict(v=v, x=x, m=m, E=E, S=S, lse=lse, T=T, dot=dot, prob=E / S[:, None])


def objective64(inp):
    """(loss, grad_w [c, e], grad_b [c]) of the data term in float64 on the f32 inputs."""
    p = _prep(inp)
    f = _forward(p)
    row = p["r"] * (f["T"] * f["lse"] - f["dot"])
    g = p["r"][:, None] * (f["T"][:, None] * f["prob"] - p["t"])
    return p["nu"] * row.sum(), p["nu"] * p["s"] * (g.T @ p["F"]), p["nu"] * g.sum(0)


def objective_bound(inp, dW=None, db=None):
    """(d loss, d grad_w, d grad_b): the bounds of the module docstring; dW [c, e], db [c] (optional): element-wise bounds on what the (W, b) the kernel
    was given differ from inp's, which enter dx as scale |u| . dW + db."""
    p = _prep(inp)
    f = _forward(p)
    n, c, e, s, nu, r, t = p["n"], p["c"], p["e"], p["s"], p["nu"], p["r"], p["t"]
    aF = np.abs(p["F"])
    dx = s * (e + 4) * U * (aF @ np.abs(p["W"]).T) + U * np.abs(f["v"]) + U * np.abs(f["x"])
    if dW is not None:
        dx = dx + s * (aF @ dW.T) + db[None, :]
    z = f["x"] - f["m"][:, None]
    dz = dx + U * (np.abs(z) + dx + dx.max(1, keepdims=True))
    E, S = f["E"], f["S"]
    dE = E * np.expm1(dz) + 2 * U * E * np.exp(dz) + TINY
    kc = -(-c // 8) + 3
    dS = dE.sum(1) + gamma(kc) * (E + dE).sum(1)
    assert (dS < 0.5 * S).all(), "the bound on the softmax denominator is not below half of it: nothing bounds the logarithm"
    prob = f["prob"]
    dp = (dE + prob * dS[:, None]) / (S - dS)[:, None] + U * prob
    dl = dS / (S - dS) + 2 * U * np.abs(np.log(S)) + U * np.abs(f["lse"])
    T = f["T"]
    dT = np.where(p["softrow"], gamma(c) * T, 0.0)
    dd = (t * dx).sum(1) + np.where(p["softrow"], gamma(kc) * (t * (np.abs(f["x"]) + dx)).sum(1), 0.0)
    row = r * np.abs(T * f["lse"] - f["dot"])
    dr = SLACK * r * (T * dl + dT * (np.abs(f["lse"]) + dl) + dd + 2 * U * (np.abs(T * f["lse"]) + np.abs(f["dot"])))
    g = r[:, None] * np.abs(T[:, None] * prob - t)
    dg = SLACK * r[:, None] * (T[:, None] * dp + dT[:, None] * (prob + dp) + 2 * U * (T[:, None] * prob + t + T[:, None] * dp)) + TINY
    nblk = -(-n // SCORE_ROWS)
    kl = SCORE_ROWS + -(-nblk // 256) + 257
    bl = SLACK * nu * (dr.sum() + gamma(kl) * (row + dr).sum()) + TINY
    rows, slices = split(n, c, e)
    k = min(rows, n) + slices + 1
    red_w = dg.T @ aF + gamma(k) * ((g + dg).T @ aF)
    red_b = dg.sum(0) + gamma(k) * (g + dg).sum(0)
    bw = SLACK * nu * s * red_w * (1 + 2 * U) + 2 * U * nu * s * (g.T @ aF) + TINY
    bb = SLACK * nu * red_b * (1 + U) + U * nu * g.sum(0) + TINY
    return bl, bw, bb


def check_objective(inp, loss, gw, gb):
    """Worst |err| / bound of (loss, grad_w, grad_b); asserts every element is within its bound."""
    l64, w64, b64 = objective64(inp)
    bl, bw, bb = objective_bound(inp)
    ratios = (abs(float(loss) - l64) / bl, float((np.abs(f64(gw) - w64) / bw).max()), float((np.abs(f64(gb) - b64) / bb).max()))
    assert all(np.isfinite(x) for x in ratios) and max(ratios) <= 1, f"objective: worst |err| / bound = loss {ratios[0]:.3f}, grad_w {ratios[1]:.3f}, grad_b {ratios[2]:.3f}"
    return ratios


def emulate_objective(inp):
    """An f32 torch emulation in the kernel's order (the logits, the shifted exponentials, the scaled residuals, the slices of the row partition one by
    one): it must stay under objective_bound."""
    p = _prep(inp)
    F, W = torch.from_numpy(p["F"]).float(), torch.from_numpy(p["W"]).float()
    b, base = torch.from_numpy(p["b"]).float(), torch.from_numpy(p["base"]).float()
    r, t = torch.from_numpy(p["r"]).float(), torch.from_numpy(p["t"]).float()
    s, nu = np.float32(p["s"]), np.float32(p["nu"])
    x = base + (float(s) * (F @ W.T) + b[None, :])
    m = x.max(1, keepdim=True).values
    E = torch.exp(x - m)
    S = E.sum(1, keepdim=True)
    lse = (m + torch.log(S))[:, 0]
    T = torch.zeros(p["n"])
    for k in range(p["c"]):
        T = T + t[:, k]
    row = r * (T * lse - (t * x).sum(1))
    g = r[:, None] * (T[:, None] * (E / S) - t)
    rows, slices = split(p["n"], p["c"], p["e"])
    gw, gb = torch.zeros_like(W), torch.zeros_like(b)
    for q in range(slices):
        gw = gw + g[q * rows:(q + 1) * rows].T @ F[q * rows:(q + 1) * rows]
        gb = gb + g[q * rows:(q + 1) * rows].sum(0)
    return float(np.float32(nu) * row.sum().numpy()), float(np.float32(nu * s)) * gw, float(nu) * gb


# ------------------------------------------------------------------------------------------ the fit
def default_lr(scale, l2):
    """1 / (1/2 (scale^2 + 1) + l2): the reciprocal of a Lipschitz bound on the gradient (unit rows, the CE Hessian in the logits <= I / 2, nu normalises)."""
    return 1.0 / (0.5 * (scale * scale + 1.0) + l2)


def fit64(inp, l2, lr, mu, iters, state=None, want_bound=False):
    """The heavy-ball recursion of include/grip_amd.h in float64 from (inp W, inp b, state = (mom_w, mom_b) or zeros), the scalars rounded to f32 as the
    kernel receives them: (W, b, mom_w, mom_b, trace [iters]).  want_bound: also (dW, db, dmw, dmb, dtrace), the objective's bound carried through the
    update's own sequence -- G = fmaf(l2, W, gw), m = fmaf(mu, m, G), W = fmaf(-lr, m, W): one rounding each -- with the bounds on (W, b) fed back into
    every logit of the next iteration.  That feedback multiplies the bound by about 1 + lr scale^2 sum_d |u_d| per iteration: FIT_TIGHT_ITERS says up to
    where the test is a precision claim."""
    l2, lr, mu = (float(np.float32(v)) for v in (l2, lr, mu))
    cur = dict(inp)
    W, b = f64(inp["W"]).copy(), (np.zeros(inp["W"].shape[0]) if inp["b"] is None else f64(inp["b"]).copy())
    mw, mb = (np.zeros_like(W), np.zeros_like(b)) if state is None else (f64(state[0]).copy(), f64(state[1]).copy())
    dW, db, dmw, dmb = np.zeros_like(W), np.zeros_like(b), np.zeros_like(W), np.zeros_like(b)
    trace, dtrace = [], []
    for _ in range(iters):
        cur["W"], cur["b"] = torch.from_numpy(W), torch.from_numpy(b)
        loss, gw, gb = objective64(cur)
        trace.append(loss)
        if want_bound:
            bl, bw, bb = objective_bound(cur, dW, db)
            dtrace.append(bl)
        G = l2 * W + gw
        mw = mu * mw + G
        mb = mu * mb + gb
        W_new, b_new = W - lr * mw, b - lr * mb
        if want_bound:
            dG = l2 * dW + bw + U * np.abs(G)
            dmw = SLACK * (mu * dmw + dG + U * np.abs(mw))
            dmb = SLACK * (mu * dmb + bb + U * np.abs(mb))
            dW = SLACK * (dW + lr * dmw + U * np.abs(W_new))
            db = SLACK * (db + lr * dmb + U * np.abs(b_new))
        W, b = W_new, b_new
    out = (W, b, mw, mb, np.asarray(trace))
    return out + ((dW, db, dmw, dmb, np.asarray(dtrace)),) if want_bound else out


FIT_TIGHT_ITERS = 3     # up to here the bound on W is at most a few tens of u wide at FIT_CASES (derived: the test prints it); at FIT_GROSS_ITERS it is
FIT_GROSS_ITERS = 8     # hundreds to thousands of u (a relative 10^-3 of |W| in the three-class case) and only guards against gross error -- a wrong sign, a
                        # missing momentum term -- as DESIGN 17.4 says of its iterated bound; by 12 iterations it no longer bounds the logarithm at all
FIT_CASES = [(65, 3, 36, "mixed"), (257, 102, 64, "hard"), (130, 65, 512, "zerosoft")]
FIT_HYPER = dict(l2=1.0, mu=0.9)


def check_fit(inp, l2, lr, mu, iters, W, b, mw, mb, trace, state=None):
    """Worst |err| / bound over (W, b, mom_w, mom_b, trace)."""
    W64, b64, mw64, mb64, tr64, (dW, db, dmw, dmb, dtr) = fit64(inp, l2, lr, mu, iters, state, want_bound=True)
    ratios = tuple(float((np.abs(f64(a) - r) / (d + TINY)).max()) for a, r, d in ((W, W64, dW), (b, b64, db), (mw, mw64, dmw), (mb, mb64, dmb), (trace, tr64, dtr)))
    assert all(np.isfinite(x) for x in ratios) and max(ratios) <= 1, f"fit({iters}): worst |err| / bound (W, b, mom_w, mom_b, trace) = {ratios}"
    return ratios


def emulate_fit(inp, l2, lr, mu, iters):
    """f32 emulation: emulate_objective + the update in numpy float32 (plain products and sums: two roundings where the kernel's fmaf has one)."""
    cur = dict(inp)
    W = inp["W"].clone().float()
    b = torch.zeros(W.shape[0]) if inp["b"] is None else inp["b"].clone().float()
    mw, mb, trace = torch.zeros_like(W), torch.zeros_like(b), []
    l2, lr, mu = (float(np.float32(v)) for v in (l2, lr, mu))
    for _ in range(iters):
        cur["W"], cur["b"] = W, b
        loss, gw, gb = emulate_objective(cur)
        trace.append(loss)
        mw = (mu * mw.double() + (l2 * W.double() + gw.double())).float()
        mb = (mu * mb.double() + gb.double()).float()
        W = (W.double() - lr * mw.double()).float()
        b = (b.double() - lr * mb.double()).float()
    return W, b, mw, mb, torch.tensor(trace)


# ------------------------------------------------------------------------------------------ the planted experiment
PLANTED_L2 = (0.1, 1.0, 10.0)
PROBE_L2 = 0.1      # the default: the best mean accuracy of the two planted shapes at seed 0 among PLANTED_L2
PROBE_ITERS, PROBE_MOMENTUM, PROBE_SCALE = 300, 0.9, 100.0


def planted_train_logits(C, e, seed, shots=16, n_test_per_class=10, wrong=0.2, n_nuis=4, nuis=1.5):
    """CLIP logits of gda_ref.planted_pool's TRAINING rows (that function returns the test rows' only): the same generator replayed draw for draw; the test
    logits it rebuilds on the way are compared bit for bit with planted_pool's, so the two cannot drift apart."""
    Ftr, _, fte, _, clip = gda_ref.planted_pool(C, e, seed)
    g = torch.Generator().manual_seed(1000 * seed + C + e)
    text_noise = 1.6 / e ** 0.5
    proto = torch.nn.functional.normalize(torch.randn(C, e, generator=g, dtype=torch.float64), dim=1)
    torch.randn(n_nuis, e, generator=g, dtype=torch.float64)
    for m in (C * shots,):
        torch.randn(m, n_nuis, generator=g, dtype=torch.float64)
        torch.randn(m, e, generator=g, dtype=torch.float64)
    torch.rand(C * shots, generator=g)
    torch.randint(0, max(C - 1, 1), (C * shots,), generator=g)
    m = C * n_test_per_class
    torch.randn(m, n_nuis, generator=g, dtype=torch.float64)
    torch.randn(m, e, generator=g, dtype=torch.float64)
    torch.rand(m, 1, generator=g, dtype=torch.float64)
    text = torch.nn.functional.normalize(proto + text_noise * torch.randn(C, e, generator=g, dtype=torch.float64), dim=1)
    again = (100.0 * torch.nn.functional.normalize(fte.double(), dim=1) @ text.T).float()
    assert torch.equal(again, clip), "planted_train_logits no longer replays gda_ref.planted_pool"
    return (100.0 * Ftr.double() @ text.T).float()


def planted_accuracies(C, e, seed, l2=PROBE_L2, iters=PROBE_ITERS, mu=PROBE_MOMENTUM, scale=PROBE_SCALE):
    """{zero_shot, gda, probe, probe_from_gda} accuracies (alpha = 1) of the planted pool in float64, and the probe's loss trace from zero."""
    Ftr, ytr, fte, yte, clip = gda_ref.planted_pool(C, e, seed)
    base = planted_train_logits(C, e, seed)
    yy = yte.numpy()
    ute = torch.nn.functional.normalize(fte.double(), dim=1).numpy()
    out = {"zero_shot": float((f64(clip).argmax(1) == yy).mean())}
    _, wg, bg = gda_ref.fit64(Ftr, ytr, None, C)
    out["gda"] = float((gda_ref.head64(fte, torch.from_numpy(wg), torch.from_numpy(bg), 1.0, clip).argmax(1) == yy).mean())
    lr = default_lr(scale, l2)
    for name, W0, b0 in (("probe", np.zeros((C, e)), np.zeros(C)), ("probe_from_gda", wg / scale, -bg)):
        inp = dict(F=Ftr, W=torch.from_numpy(W0), b=torch.from_numpy(b0), base=base, y=ytr.to(torch.int32), soft=None, r=None, scale=scale,
                   norm=1.0 / Ftr.shape[0])
        W, b, _, _, trace = fit64(inp, l2, lr, mu, iters)
        out[name] = float(((f64(clip) + scale * ute @ W.T + b[None, :]).argmax(1) == yy).mean())
        out[name + "_loss"] = (float(trace[0]), float(trace[-1]))
    return out
