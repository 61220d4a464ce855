"""Float64 references and per-element error bounds of the Gaussian discriminant head (csrc/gda_head.hip; models/gda_models.py), shared by the CPU
tests (tests/test_host_gda_ref.py) and the GPU tests.  Every bound is derived from the inputs and u = 2^-24 alone (in the manner of DESIGN 16.4):
nothing in this file comes from a measurement of the kernels.

Model of the arithmetic.  The f32 MFMA and fmaf are exact products followed by ONE rounding of the sum, so a chain of k accumulations obeys the
classical bound |err| <= gamma_k sum |terms|, gamma_k = k u / (1 - k u), whatever the order; + - * / sqrt are correctly rounded (relative error u).
"""
import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126


def gamma(k):
    return k * U / (1.0 - k * U)


def f64(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def case_id(case):
    return "-".join(str(x).replace(".", "p") for x in case)


# ------------------------------------------------------------------------------------------ scatter
SCATTER_ROWS, SCATTER_SLICES = 256, 16      # csrc/gda_head.hip GD_ROWS / GD_SLICES (engine.GDA_SCATTER_ROWS / GDA_SCATTER_SLICES)
_E_CYCLE = (4, 64, 68, 192, 512)
_KINDS = ("plain", "weighted", "empty", "samerows")
S_CASES = [(n, c, _E_CYCLE[(i * 4 + j) % 5], _KINDS[(i + j) % 4]) for i, n in enumerate((1, 5, 255, 257, 549)) for j, c in enumerate((1, 2, 65, 102))]
S_CASES.append((17 * 256 + 3, 5, 68, "weighted"))       # 18 chunks -> 9 slices of 2 chunks, the last one ragged (259 rows)


def scatter_split(n):
    """(rows per slice, slices) of the kernel's fixed partition."""
    nch = -(-n // SCATTER_ROWS)
    per = -(-nch // SCATTER_SLICES)
    return per * SCATTER_ROWS, -(-nch // per)


def scatter_inputs(n, c, e, kind, seed):
    """(F f32 [n, e] unit rows, y int32 [n], r f32 [n] or None, mean f32 [c, e]) on the CPU.  `weighted`: pseudo rows weigh 0.37 and row 0 weighs 0;
    `empty`: class c // 2 owns no row (c >= 2); `samerows`: the rows of a class are bit-identical, so with the mean equal to that row S is exactly 0.
    The mean is the float64 weighted class mean rounded to f32 (the kernel takes ANY centre: it is an input)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, c, (n,), generator=g)
    if kind == "empty" and c >= 2:
        y = torch.where(y == c // 2, (y + 1) % c, y)
    proto = torch.nn.functional.normalize(torch.randn(c, e, generator=g, dtype=torch.float64), dim=1)
    nuis = torch.randn(1, e, generator=g, dtype=torch.float64) * 0.5
    F = proto[y] + (0.0 if kind == "samerows" else 1.0) * (0.3 * torch.randn(n, e, generator=g, dtype=torch.float64) +
                                                          torch.randn(n, 1, generator=g, dtype=torch.float64) * nuis)
    F = torch.nn.functional.normalize(F, dim=1).float()
    r = None
    if kind == "weighted":
        r = torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(0.37), torch.tensor(1.0))
        r[0] = 0.0
    mean = class_means64(F, y, r, c).float()
    return F, y.to(torch.int32), r, mean


def class_means64(F, y, r, c):
    """float64 weighted class means [c, e] (zero for a class of zero weight) as a torch float64 tensor."""
    Fd, yd = F.double().cpu(), y.long().cpu()
    rd = torch.ones(Fd.shape[0], dtype=torch.float64) if r is None else r.double().cpu()
    z = torch.zeros(Fd.shape[0], c, dtype=torch.float64)
    z[torch.arange(Fd.shape[0]), yd] = rd
    cnt = z.sum(0)
    s = z.T @ Fd
    return torch.where(cnt[:, None] > 0, s / cnt.clamp(min=TINY)[:, None], torch.zeros_like(s))


def centred(F, y, r, mean):
    """(d float64 [n, e] = fl32(F - mean[y]) of the rows that count -- zero rows elsewhere --, r float64 [n])."""
    Ft, mt, yt = F.detach().cpu().float(), mean.detach().cpu().float(), y.detach().cpu().long()
    c = mt.shape[0]
    ok = (yt >= 0) & (yt < c)
    rt = torch.ones(Ft.shape[0]) if r is None else r.detach().cpu().float()
    ok &= rt != 0
    d = (Ft - mt[yt.clamp(0, c - 1)]).double()          # one f32 rounding, as the kernel's load path
    d[~ok] = 0
    return d.numpy(), torch.where(ok, rt, torch.zeros_like(rt)).double().numpy()


def scatter64(F, y, r, mean):
    """S = sum_i r_i d_i d_i^T in float64, d = fl32(F - mean[y]) (the centre is the kernel's own input)."""
    d, rr = centred(F, y, r, mean)
    return (d * rr[:, None]).T @ d


def scatter_bound(F, y, r, mean):
    """|S~ - S| <= gamma_k sum_i r_i |d_ia| |d_ib| + k 2^-126, k = (rows of a slice) + (slices) + 1: one rounding of r_i d_ia, one per accumulated
    row of the slice's chain, one per slice added."""
    d, rr = centred(F, y, r, mean)
    rows, slices = scatter_split(d.shape[0])
    k = min(rows, d.shape[0]) + slices + 1
    return gamma(k) * ((np.abs(d) * rr[:, None]).T @ np.abs(d)) + k * TINY


def emulate_scatter(F, y, r, mean):
    """An f32 torch emulation of the kernel's scatter (same partition, f32 accumulation): it must stay under scatter_bound."""
    d64, rr = centred(F, y, r, mean)
    d = torch.from_numpy(d64).float()
    a = d * torch.from_numpy(rr).float()[:, None]
    rows, slices = scatter_split(d.shape[0])
    S = torch.zeros(d.shape[1], d.shape[1])
    for s in range(slices):
        S = S + a[s * rows:(s + 1) * rows].T @ d[s * rows:(s + 1) * rows]
    return torch.tril(S) + torch.tril(S, -1).T


def check_scatter(F, y, r, mean, S):
    """Worst |err| / bound over every element; asserts every element is within its bound."""
    err = np.abs(f64(S) - scatter64(F, y, r, mean))
    bound = scatter_bound(F, y, r, mean)
    ratio = err / bound
    assert (err <= bound).all(), f"scatter: worst |err| / bound = {ratio.max():.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return float(ratio.max())


# ------------------------------------------------------------------------------------------ SPD solve
V_CASES = [(4, 1, 1.0, "scatter"), (64, 2, 0.1, "scatter"), (68, 65, 1.0, "scatter"), (132, 102, 0.1, "scatter"), (512, 102, 1.0, "scatter"),
           (512, 2, 0.1, "scatter"), (68, 2, 0.0, "diag"), (132, 1, 1.0, "scatter")]


def solve_inputs(e, c, kind, seed):
    """(a f32 [e, e] symmetric, a_scale, rhs f32 [c, e]): a real within-class scatter of 3 e + 7 rows (rounded to f32) and the class means, or a
    positive diagonal matrix."""
    if kind == "diag":
        g = torch.Generator().manual_seed(seed)
        a = torch.diag(torch.rand(e, generator=g) * 3 + 0.01)
        return a, 0.5, torch.randn(c, e, generator=g)
    n = 3 * e + 7
    F, y, r, mean = scatter_inputs(n, c, e, "plain", seed)
    S = torch.from_numpy(scatter64(F, y, r, mean)).float()
    return torch.tril(S) + torch.tril(S, -1).T, 1.0 / n, mean


def spd_matrix64(a, a_scale, ridge_rel):
    """(M float64 from the LOWER triangle of a and the f32 values of the scalars, E: the element-wise bound on |M~ - M| of forming it in f32)."""
    A = np.tril(f64(a))
    A = A + np.tril(A, -1).T
    e = A.shape[0]
    s, rho = float(np.float32(a_scale)), float(np.float32(ridge_rel))
    dg = np.diag(A)
    shift = rho * s * dg.sum() / e
    M = s * A + shift * np.eye(e)
    # off the diagonal one product: u |s a_ij|.  The diagonal: the trace is a sum of e terms in some order (gamma_e sum |a_ii|), the shift three more
    # roundings, M_ii = fmaf(s, a_ii, shift~) one more.
    shift_abs = rho * s * np.abs(dg).sum() / e
    E = U * np.abs(s * A)
    np.fill_diagonal(E, U * (np.abs(s * dg) + shift_abs) + 1.01 * gamma(e + 3) * shift_abs)
    return M, E


def solve64(a, a_scale, ridge_rel, rhs):
    M, _ = spd_matrix64(a, a_scale, ridge_rel)
    return np.linalg.solve(M, f64(rhs).T).T


def check_solve(a, a_scale, ridge_rel, rhs, x, L):
    """The three inequalities of the Cholesky backward-error theorems (Higham, Accuracy and Stability, Thm 10.3 / 10.4 -- valid for any summation
    order), element-wise, with the kernel's own factor L~ and solution x^ evaluated in float64 and the bound E of forming M added:
        |L~ L~^T - M| <= gamma_{e+1} |L~| |L~^T| + E
        |rhs - M x^|  <= (gamma_{3e+1} |L~| |L~^T| + E) |x^|
        |x^ - x|      <= |M^-1| (that)
    Returns the worst |err| / bound of each."""
    M, E = spd_matrix64(a, a_scale, ridge_rel)
    e = M.shape[0]
    Lt, xh, b = f64(L), f64(x), f64(rhs)
    assert (np.triu(Lt, 1) == 0).all(), "the factor must be lower triangular (zeros above the diagonal)"
    LL = np.abs(Lt) @ np.abs(Lt).T
    tiny = e * TINY
    r1 = np.abs(Lt @ Lt.T - M) / (gamma(e + 1) * LL + E + tiny)
    res_bound = (gamma(3 * e + 1) * LL + E) @ np.abs(xh).T + tiny       # [e, c]
    r2 = np.abs(b.T - M @ xh.T) / res_bound
    Minv = np.linalg.inv(M)
    x64 = Minv @ b.T
    r3 = np.abs(xh.T - x64) / (np.abs(Minv) @ res_bound * (1 + 1e-9) + 1e-12 * np.abs(x64) + tiny)
    out = tuple(float(r.max()) for r in (r1, r2, r3))
    assert out[0] <= 1 and out[1] <= 1 and out[2] <= 1, f"solve: worst |err| / bound = factor {out[0]:.3f}, residual {out[1]:.3f}, solution {out[2]:.3f}"
    return out


def emulate_solve(a, a_scale, ridge_rel, rhs):
    """An f32 emulation (unblocked Cholesky-Banachiewicz and the two substitutions in numpy float32): it must pass check_solve."""
    A = np.tril(a.detach().cpu().float().numpy())
    A = A + np.tril(A, -1).T
    e = A.shape[0]
    s, rho = np.float32(a_scale), np.float32(ridge_rel)
    shift = np.float32(np.float32(np.float32(rho * s) * A.diagonal().sum(dtype=np.float32)) / np.float32(e))
    M = (s * A).astype(np.float32)
    M[np.arange(e), np.arange(e)] = (s * A.diagonal() + shift).astype(np.float32)
    L = np.zeros((e, e), dtype=np.float32)
    for j in range(e):
        L[j, j] = np.sqrt(M[j, j] - np.dot(L[j, :j], L[j, :j]))
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    b = rhs.detach().cpu().float().numpy()
    yv = np.zeros_like(b)
    for j in range(e):
        yv[:, j] = (b[:, j] - yv[:, :j] @ L[j, :j]) / L[j, j]
    xv = np.zeros_like(b)
    for j in range(e - 1, -1, -1):
        xv[:, j] = (yv[:, j] - xv[:, j + 1:] @ L[j + 1:, j]) / L[j, j]
    return torch.from_numpy(xv), torch.from_numpy(L)


# ------------------------------------------------------------------------------------------ linear head
_HE = (4, 64, 512, 1024)
H_CASES = [(n, c, _HE[(i + j) % 4], ("nobase", "base", "inplace")[(i * 5 + j) % 3]) for i, n in enumerate((1, 63, 65, 200))
           for j, c in enumerate((1, 64, 65, 102, 129))]


def head_inputs(n, c, e, seed):
    """(f f32 [n, e] NOT normalised, w f32 [c, e], bias f32 [c], base f32 [n, c], alpha)."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(n, e, generator=g) * (0.2 + 3 * torch.rand(n, 1, generator=g))
    w = torch.randn(c, e, generator=g) * 4
    bias = torch.randn(c, generator=g) * 2
    base = torch.randn(n, c, generator=g) * 30
    return f, w, bias, base, 1.7


def head64(f, w, bias, alpha, base=None):
    F, W = f64(f), f64(w)
    t = (F @ W.T) / np.sqrt((F * F).sum(1))[:, None]
    out = float(np.float32(alpha)) * (t - f64(bias)[None, :])
    return out if base is None else f64(base) + out


def head_bound(f, w, bias, alpha, base=None):
    """score: one chain over e, (e + 4) u on P = sum_d |f_d w_cd| / |f|; the norm: the sum of squares is a sum of e terms in some order
    (gamma_e, halved by the square root), the square root, the reciprocal and the product with the score: (e / 2 + 3) u on P; the bias, the scale and
    the base: three roundings (or fewer where the compiler fuses) on |alpha| (|t| + |bias|), one on the result."""
    F, W, B = f64(f), f64(w), np.abs(f64(bias))[None, :]
    nrm = np.sqrt((F * F).sum(1))[:, None]
    P = (np.abs(F) @ np.abs(W).T) / nrm
    t = np.abs((F @ W.T) / nrm)
    al = abs(float(np.float32(alpha)))
    e = F.shape[1]
    bound = al * (e + 4 + e / 2 + 3) * U * P + 3 * U * al * (t + B)
    if base is not None:
        bound = bound + U * np.abs(f64(base))
    return 1.01 * bound + TINY


def emulate_head(f, w, bias, alpha, base=None):
    ft, wt = f.detach().cpu().float(), w.detach().cpu().float()
    rn = 1.0 / torch.sqrt((ft * ft).sum(1, keepdim=True))
    v = float(alpha) * ((ft @ wt.T) * rn - bias.detach().cpu().float()[None, :])
    return v if base is None else base.detach().cpu().float() + v


def check_head(f, w, bias, alpha, base, out):
    err = np.abs(f64(out) - head64(f, w, bias, alpha, base))
    bound = head_bound(f, w, bias, alpha, base)
    ratio = err / bound
    assert (err <= bound).all(), f"head: worst |err| / bound = {ratio.max():.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return float(ratio.max())


# ------------------------------------------------------------------------------------------ the whole fit
def fit64(F, y, r, C, shrink=1.0, prior=None, diagonal=False):
    """(mean, w, bias) float64 numpy of the model of models/gda_models.py on the f32 unit rows F.  diagonal: the covariance keeps its diagonal only
    (the variant the planted experiment compares with)."""
    mean = class_means64(F, y, r, C)
    d = f64(F) - mean.numpy()[y.long().cpu().numpy()]
    rr = np.ones(d.shape[0]) if r is None else f64(r)
    S = (d * rr[:, None]).T @ d
    W, e = rr.sum(), d.shape[1]
    A = S / W + shrink * np.trace(S) / (W * e) * np.eye(e)
    if diagonal:
        A = np.diag(np.diag(A))
    mu = mean.numpy()
    w = np.linalg.solve(A, mu.T).T
    bias = 0.5 * (mu * w).sum(1)
    if prior is not None:
        bias = bias - np.log(f64(prior))
    cnt = np.zeros(C)
    np.add.at(cnt, y.long().cpu().numpy(), rr)
    w[cnt == 0] = 0
    bias[cnt == 0] = 0
    return mu, w, bias


def fit_bound(F, y, r, C, shrink=1.0):
    """First-order element-wise bounds (dw [C, e], dbias [C]) on what the f32 pipeline (gmm_mstep -> class_scatter -> spd_solve -> bias in torch) may
    differ from fit64 on the same F, times 2 for the second-order terms:
      means     |dmu_c|  <= gamma_{2n+3} sum_{i in c} r_i |F_i| / N_c                       (a sum of <= n terms in some order, the count, the division)
      scatter   |dS_ab|  <= sum_i r_i (|d_a| (dmu_b + u |d_b|) + |d_b| (dmu_a + u |d_a|)) + scatter_bound   (moved centres, rounded d, the SYRK)
      matrix    |dA|     <= |dS| / W + u |S| / W + E of spd_matrix64                          (1 / W rounded to f32)
      solve     |dw_c|   <= |A^-1| ((|dA| + gamma_{3e+1} |L| |L^T|) |w_c| + dmu_c)            (perturbation + Higham Thm 10.4)
      bias      |db_c|   <= 1/2 (|mu_c| . dw_c + dmu_c . |w_c|) + gamma_{e+2} 1/2 |mu_c| . |w_c|"""
    mu, w, _ = fit64(F, y, r, C, shrink)
    Fd, yy = f64(F), y.long().cpu().numpy()
    n, e = Fd.shape
    rr = np.ones(n) if r is None else f64(r)
    cnt = np.zeros(C)
    np.add.at(cnt, yy, rr)
    absum = np.zeros((C, e))
    np.add.at(absum, yy, np.abs(Fd) * rr[:, None])
    dmu = gamma(2 * n + 3) * absum / np.maximum(cnt, TINY)[:, None]
    d = np.abs(Fd - mu[yy])
    dm = dmu[yy] + U * d
    cross = (d * rr[:, None]).T @ dm
    rows, slices = scatter_split(n)
    k = min(rows, n) + slices + 1
    dS = cross + cross.T + gamma(k) * ((d * rr[:, None]).T @ d)
    S = (d * rr[:, None]).T @ d        # |S| <= this
    W = rr.sum()
    shift = shrink * np.trace(S) / (W * e)
    A64 = ((Fd - mu[yy]) * rr[:, None]).T @ (Fd - mu[yy]) / W + shift * np.eye(e)
    dA = dS / W + 2 * U * S / W
    dA[np.arange(e), np.arange(e)] += shrink * (np.trace(dS) / (W * e)) + 1.01 * gamma(e + 6) * shift
    L = np.linalg.cholesky(A64)
    Ainv = np.abs(np.linalg.inv(A64))
    pert = dA + gamma(3 * e + 1) * (np.abs(L) @ np.abs(L).T)
    dw = 2 * (Ainv @ (pert @ np.abs(w).T + dmu.T)).T
    db = 2 * (0.5 * ((np.abs(mu) * dw).sum(1) + (dmu * np.abs(w)).sum(1)) + gamma(e + 2) * 0.5 * (np.abs(mu) * np.abs(w)).sum(1))
    dw[cnt == 0] = 0
    db[cnt == 0] = 0
    return dw, db


def composed_logit_bound(f, w, bias, alpha, base, dw, db):
    """|logits~ - logits64| for a head run on the pipeline's own (w~, bias~): head_bound on those + |alpha| (sum_d |f_d| dw_cd / |f| + db_c)."""
    F = f64(f)
    nrm = np.sqrt((F * F).sum(1))[:, None]
    return head_bound(f, w, bias, alpha, base) + abs(float(alpha)) * ((np.abs(F) @ dw.T) / nrm + db[None, :])


# ------------------------------------------------------------------------------------------ the planted experiment
PLANTED_SHAPES = ((20, 64), (102, 512))
PLANTED_SEEDS = (0, 1, 2)


def planted_pool(C, e, seed, shots=16, n_test_per_class=10, wrong=0.2, n_nuis=4, nuis=1.5, noise=None, text_noise=None):
    """A planted pool (not a dataset): unit prototypes + four strong nuisance directions shared by all classes + isotropic noise; `shots` training rows
    per class of which `wrong` carry a wrong label; CLIP logits = 100 x cosine to noisy copies of the prototypes.  Returns f32 tensors
    (train F unit, train y (noisy), test f NOT normalised, test y, test clip logits)."""
    g = torch.Generator().manual_seed(1000 * seed + C + e)
    noise = 1.2 / e ** 0.5 if noise is None else noise
    text_noise = 1.6 / e ** 0.5 if text_noise is None else text_noise
    proto = torch.nn.functional.normalize(torch.randn(C, e, generator=g, dtype=torch.float64), dim=1)
    dirs = torch.nn.functional.normalize(torch.randn(n_nuis, e, generator=g, dtype=torch.float64), dim=1)

    def draw(labels):
        m = labels.numel()
        x = proto[labels] + nuis * torch.randn(m, n_nuis, generator=g, dtype=torch.float64) @ dirs + noise * torch.randn(m, e, generator=g, dtype=torch.float64)
        return x

    ytr = torch.arange(C).repeat_interleave(shots)
    Ftr = torch.nn.functional.normalize(draw(ytr), dim=1).float()
    flip = torch.rand(ytr.numel(), generator=g) < wrong
    ynoisy = torch.where(flip, (ytr + 1 + torch.randint(0, max(C - 1, 1), ytr.shape, generator=g)) % C, ytr)
    yte = torch.arange(C).repeat_interleave(n_test_per_class)
    fte = (draw(yte) * (0.5 + torch.rand(yte.numel(), 1, generator=g, dtype=torch.float64))).float()
    text = torch.nn.functional.normalize(proto + text_noise * torch.randn(C, e, generator=g, dtype=torch.float64), dim=1)
    clip = (100.0 * torch.nn.functional.normalize(fte.double(), dim=1) @ text.T).float()
    return Ftr, ynoisy, fte, yte, clip


def planted_accuracies(C, e, seed):
    """{zero-shot, gda (alpha 1), diagonal (alpha 1), gda3 (alpha 3)} accuracies of the planted pool in float64."""
    Ftr, ytr, fte, yte, clip = planted_pool(C, e, seed)
    yy = yte.numpy()
    out = {"zero_shot": float((f64(clip).argmax(1) == yy).mean())}
    for name, diag, alpha in (("gda", False, 1.0), ("diagonal", True, 1.0), ("gda3", False, 3.0)):
        _, w, bias = fit64(Ftr, ytr, None, C, diagonal=diag)
        out[name] = float((head64(fte, torch.from_numpy(w), torch.from_numpy(bias), alpha, clip).argmax(1) == yy).mean())
    return out
