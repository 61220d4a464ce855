"""float64 references, bounds and inputs for the transductive GMM kernels (csrc/gmm_transduce.hip), shared by the GPU tests and shown to hold for an
f32 emulation on the host (tests/test_host_gmm_ref.py).  Everything works on torch tensors of any device.  u = 2^-24 (the unit roundoff of f32; one ulp
is 2 u).  Every bound below follows from the inputs, u and the documented accuracy of expf / logf alone; nothing in it is measured.  The references
run in float64 on the SAME f32 inputs, so only the arithmetic differs.

M-STEP.  An f32 sum of m terms t, in any order, with or without fused multiply-adds, products included: |err| <= m u sum |t| (first order).
    count    N_c = sum_i Z_ic                      |err| <= n u N_c                                                  (Z >= 0)
    sums     S_cd = sum_i Z_ic F_id                |err| <= n u T_cd,  T = Z^T |F|
    centres  mu_cd = S_cd / N_c                    |err| <= (n u T_cd + |mu_cd| n u N_c) / N_c + u |mu_cd| <= (2 n + 1) u T_cd / N_c   (T_cd / N_c >= |mu_cd|)
             asserted: bm_cd = (2 n + 4) u T_cd / N_c (three u of room for the second-order terms); N_c = 0 exactly: mu_c = 0 exactly.
    variance V_d = sum_i sum_c Z_ic (F_id - mu_cd)^2, the kernel's own centres being off by up to bm_cd: with d = F_id - mu_cd (float64) and
             D = |d| + bm_cd the kernel's difference is at most D in size (its own rounding, u D, goes into the 4 u below), so a term Z d^2 is off by at
             most Z ((D^2 - d^2) + 4 u D^2)  (the centre's error kept to second order -- d can be 0 --; subtraction, square and product: 4 u), and the sum
             of the n c non-negative terms by n c u sum Z D^2:
                 bV_d = sum_i sum_c Z_ic ((D^2 - d^2) + (n c + 4) u D^2)
             var_d = max(var_floor, V_d / n) (the maximum moves nothing apart): bv_d = bV_d / n + 2 u V_d / n   (the division and float(n)).
Every bound gets 2^-126 for a result in the subnormal range.

E-STEP.  W_cd = mu_cd / var_d is relative u.  With A_ic = sum_d |F_id mu_cd| / var_d (<= |F_i| |mu_c / var|, the scale of the dot product) and
B_c = 1/2 sum_d mu_cd^2 / var_d:
    the dot of e terms on a W that is itself relative u:   (e + 1) u A_ic;        the bias, e terms likewise:   (e + 2) u B_c
    their difference rounds once: u (A_ic + B_c)
    lam log max(P, 2^-126): logf within 2 ulp = 4 u relative, the product (or the fused multiply-add it ends in) u:   5 u lam |log|
    the sum of the two rounds once:  u (A_ic + B_c + lam |log|)
so the static score G_ic + lam log P_ic is off by at most          bs_ic = (e + 4) u (A_ic + B_c) + 6 u lam |log max(P_ic, 2^-126)|.
A sweep's argument a_ic = static + sum_j w_ij Z_{idx_ij, c}, w = max(0, sim) (exact), as k fused multiply-adds in list order and one addition, on a Z that is
itself off by up to b^t (b^0 = 0: both sides start from the same z_in):
    beta_ic = bs_ic + sum_j w_ij b^t_{idx_ij, c} + k u sum_j w_ij Z^t_{idx_ij, c} + u |a_ic|
so a sweep passes the neighbours' error on amplified by at most sum_j max(0, sim_ij).  The softmax subtracts the row's maximum first (neutral but for the
rounding of the difference: u (max_i - a_ic), + 2 u max_c beta_ic for the kernel's own maximum and argument), so the exponent is off by at most
    beta'_ic = beta_ic + u (max_i - a_ic) + 2 u max_c beta_ic
and a softmax whose arguments move by at most beta'_c moves EXACTLY within (no linearisation; it is monotone in every argument)
    lo_c = z_c e^{-beta'_c} / (z_c e^{-beta'_c} + sum_{j != c} z_j e^{+beta'_j}),     hi_c = z_c e^{+beta'_c} / (z_c e^{+beta'_c} + sum_{j != c} z_j e^{-beta'_j})
Its own arithmetic: expf within 2 ulp (4 u), the sum of c terms (c u), the division (u): relative (c + 8) u with room; an exponential or a quotient in
the subnormal range: 2^-126.      b^{t+1}_ic = max(hi_c - z_c, z_c - lo_c) + (c + 8) u z_c + 2^-126.
argmax_out is the FIRST maximum of the kernel's own row, exactly."""
import itertools

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
ROWS = 256      # the M-step's fixed row partition (engine.GMM_MSTEP_ROWS; csrc/gmm_transduce.hip GM_ROWS)


# ------------------------------------------------------------------------------------------ M-step
def mstep64(z, f, var_floor, bounds=False):
    """(count [c], mean [c, e], var [e]) in float64 -- the direct two-pass form -- and, with bounds=True, the three bounds of the module docstring."""
    zd, fd = z.double(), f.double()
    n, c = zd.shape
    cnt = zd.sum(0)
    s = zd.T @ fd
    mean = torch.where(cnt[:, None] == 0, torch.zeros_like(s), s / cnt[:, None].clamp_min(TINY))
    t = zd.T @ fd.abs()
    bm = torch.where(cnt[:, None] == 0, torch.zeros_like(s), (2 * n + 4) * U * t / cnt[:, None].clamp_min(TINY)) + TINY
    v = torch.zeros(fd.shape[1], dtype=torch.float64, device=fd.device)
    bv = torch.zeros_like(v)
    step = max(1, (1 << 22) // max(1, n * fd.shape[1]))            # classes at a time: the [n, classes, e] differences stay below 32 MiB
    for c0 in range(0, c, step):
        d = fd[:, None, :] - mean[None, c0:c0 + step, :]
        w = zd[:, c0:c0 + step, None]
        v += (w * d * d).sum((0, 1))
        if bounds:
            big = (d.abs() + bm[None, c0:c0 + step, :]) ** 2
            bv += (w * ((big - d * d) + (n * c + 4) * U * big)).sum((0, 1))
    var = (v / n).clamp_min(float(np.float32(var_floor)))
    if not bounds:
        return cnt, mean, var
    return cnt, mean, var, n * U * cnt + TINY, bm, bv / n + 2 * U * v / n + TINY


def check_mstep(z, f, var_floor, count, mean, var):
    """Assert every element of the three outputs against float64; returns the worst |err| / bound."""
    c64, m64, v64, bc, bm, bv = mstep64(z, f, var_floor, bounds=True)
    worst = 0.0
    for name, got, want, b in (("count", count, c64, bc), ("mean", mean, m64, bm), ("var", var, v64, bv)):
        err = (got.double() - want).abs()
        ratio = float((err / b).max())
        assert torch.isfinite(got).all() and (err <= b).all(), f"M-step: |{name} - {name}64| is {ratio:.2f} x its bound"
        worst = max(worst, ratio)
    return worst


def mstep_f32(z, f, var_floor):
    """An f32 emulation of the kernels in torch (f32 matmul, the two-pass variance class by class): what the checker must accept."""
    cnt = z.sum(0)
    s = z.T @ f
    mean = torch.where(cnt[:, None] == 0, torch.zeros_like(s), s / cnt[:, None].clamp_min(TINY))
    v = torch.zeros(f.shape[1])
    for j in range(z.shape[1]):
        d = f - mean[j]
        v = v + (z[:, j:j + 1] * (d * d)).sum(0)
    return cnt, mean, (v / z.shape[0]).clamp_min(var_floor)


# ------------------------------------------------------------------------------------------ E-step
def _static64(f, mean, var, probs, lam):
    fd, md, vd = f.double(), mean.double(), var.double()
    w = md / vd
    bias = 0.5 * (md * w).sum(1)
    logp = torch.log(probs.double().clamp_min(TINY))
    lam = float(np.float32(lam))
    static = fd @ w.T - bias + lam * logp
    e = fd.shape[1]
    bs = (e + 4) * U * (fd.abs() @ w.abs().T + bias) + 6 * U * lam * logp.abs()
    return static, bs


def estep64(f, mean, var, probs, idx, sim, z_in, lam, z_iters):
    """(Z64 [n, c], bound [n, c]) of the module docstring: the float64 sweeps on the given graph and the bound carried through them."""
    static, bs = _static64(f, mean, var, probs, lam)
    (n, c), k = static.shape, idx.shape[1]
    ix, w = idx.long(), sim.double().clamp_min(0.0)
    z, b = z_in.double(), torch.zeros_like(static)
    for _ in range(z_iters):
        nbz = torch.zeros_like(static)
        nbb = torch.zeros_like(static)
        for j in range(k):                                           # (list order, as the kernel; float64 does not care)
            nbz += w[:, j:j + 1] * z[ix[:, j]]
            nbb += w[:, j:j + 1] * b[ix[:, j]]
        a = static + nbz
        beta = bs + nbb + k * U * nbz.abs() + U * a.abs()
        mx = a.max(dim=1, keepdim=True).values
        beta = beta + U * (mx - a) + 2 * U * beta.max(dim=1, keepdim=True).values
        z = torch.softmax(a, dim=1)
        up, dn = z * torch.exp(beta), z * torch.exp(-beta)
        hi = up / (up + (dn.sum(1, keepdim=True) - dn).clamp_min(0.0)).clamp_min(TINY)
        lo = dn / (dn + (up.sum(1, keepdim=True) - up).clamp_min(0.0)).clamp_min(TINY)
        b = torch.maximum(hi - z, z - lo).clamp_min(0.0) + (c + 8) * U * z + TINY
    return z, b


def check_estep(f, mean, var, probs, idx, sim, z_in, lam, z_iters, out, argmax=None):
    """Assert every element of `out` against the float64 sweeps and argmax (the first maximum of out's own row); returns the worst |err| / bound."""
    z, b = estep64(f, mean, var, probs, idx, sim, z_in, lam, z_iters)
    err = (out.double() - z).abs()
    ratio = float((err / b).max())
    assert torch.isfinite(out).all() and (err <= b).all(), f"E-step: |Z - Z64| is {ratio:.2f} x its bound"
    if argmax is not None:
        first = np.argmax(out.cpu().numpy(), axis=1)
        assert np.array_equal(argmax.cpu().numpy().astype(np.int64), first), "E-step: argmax_out is not the first maximum of the row"
    return ratio


def estep_f32(f, mean, var, probs, idx, sim, z_in, lam, z_iters):
    """An f32 emulation of the kernels in torch (no fused multiply-adds): what the checker must accept."""
    w = mean / var
    static = (f @ w.T - 0.5 * (mean * w).sum(1)) + torch.tensor(lam, dtype=torch.float32) * torch.log(probs.clamp_min(TINY))
    ix, wt = idx.long(), sim.clamp_min(0.0)
    z = z_in
    for _ in range(z_iters):
        acc = torch.zeros_like(static)
        for j in range(ix.shape[1]):
            acc = acc + wt[:, j:j + 1] * z[ix[:, j]]
        a = static + acc
        x = torch.exp(a - a.max(dim=1, keepdim=True).values)
        z = x / x.sum(1, keepdim=True)
    return z, torch.from_numpy(np.argmax(z.numpy(), axis=1).astype(np.int32))


def transduce64(f, probs, idx, sim, lam, iters, z_iters, var_floor):
    """(Z64, mean64, var64, count64, largest bound): the whole recursion in float64 from Z = probs on unit rows f.  The bound is the largest E-step bound
    of any of the `iters` E-steps, each taken from its own float64 operands: what one call's f32 arithmetic can move an assignment by (it is NOT carried
    from round to round through the centres; the planted-cluster test holds the reference's margins 100 x clear of it instead)."""
    z, worst = probs.double(), 0.0
    for _ in range(iters):
        cnt, mean, var = mstep64(z, f, var_floor)
        z, b = estep64(f, mean, var, probs, idx, sim, z, lam, z_iters)
        worst = max(worst, float(b.max()))
    return z, mean, var, cnt, worst


# ------------------------------------------------------------------------------------------ inputs and cases
def unit_rows(n, e, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, e, generator=g), dim=1)


def soft_rows(n, c, seed):
    """Z / P rows: softmaxes of 4 randn."""
    return torch.softmax(4 * torch.randn(n, c, generator=torch.Generator().manual_seed(seed)), dim=1)


def mstep_inputs(n, c, e, kind, seed):
    """(Z, F).  kind "zerocol": column c // 2 of Z is exactly 0 (the rows no longer sum to 1: weights are weights); "samerows": every row of F is the same."""
    z, f = soft_rows(n, c, seed), unit_rows(n, e, seed + 1)
    if kind == "zerocol":
        z[:, c // 2] = 0.0
    if kind == "samerows":
        f = f[:1].repeat(n, 1).contiguous()
    return z, f


def graph_inputs(n, k, seed):
    """A random directed graph (self-loops and repeated neighbours included: n = 1 is nothing else) with sorted similarities in [-0.2, 1]: the negative ones
    must contribute nothing."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n, (n, k), generator=g, dtype=torch.int32)
    idx[0, 0] = 0                                                   # a self-loop for certain
    if k > 1:
        idx[n - 1, 1] = idx[n - 1, 0]                               # ... and a repeated neighbour
    sim = torch.sort(1.2 * torch.rand(n, k, generator=g) - 0.2, dim=1, descending=True).values
    if k > 1:
        sim[:, -1] = -sim[:, -1].abs() - 0.01                       # ... and a negative entry in every row
    return idx, sim


def estep_inputs(n, c, e, k, kind, seed):
    """(F, mean, var, P, idx, sim, Z_in): unit rows, centres of norm 1 or 0.1 (by the seed's parity: saturated and soft assignments), var log-uniform in
    [1e-4, 1e-2].  kind "zeroprob": P has exact zeros (the 2^-126 clamp)."""
    g = torch.Generator().manual_seed(seed + 2)
    f = unit_rows(n, e, seed)
    mean = unit_rows(c, e, seed + 1) * (1.0 if seed % 2 else 0.1)
    var = torch.exp(torch.log(torch.tensor(1e-4)) + torch.rand(e, generator=g) * torch.log(torch.tensor(100.0)))
    probs, z_in = soft_rows(n, c, seed + 3), soft_rows(n, c, seed + 4)
    if kind == "zeroprob":
        probs[torch.rand(n, c, generator=g) < 0.3] = 0.0
        probs[0, :] = 0.0
    idx, sim = graph_inputs(n, k, seed + 5)
    return f, mean, var, probs, idx, sim, z_in


NS = (1, 5, 257, ROWS - 1, 2 * ROWS + 37)           # 257 is also ROWS + 1; the last: three chunks, the third ragged
CS = (1, 2, 64, 65, 102, 300)
ES = (4, 64, 512, 1028)
M_CASES = [(n, c, ES[(i + i // 4) % 4], "plain") for i, (n, c) in enumerate(itertools.product(NS, CS))] + \
          [(257, 65, 64, "zerocol"), (2 * ROWS + 37, 2, 512, "zerocol"), (257, 102, 512, "samerows")]
assert {m[2] for m in M_CASES} == set(ES)

HYPER = [(k, zi, lam) for k in (1, 3, 32) for zi in (1, 2, 5) for lam in (0.0, 1.0, 4.0)]
E_CASES = [(n, c, ES[(i + i // 4) % 4], *HYPER[(i + i // 27) % 27], "plain") for i, (n, c) in enumerate(itertools.product(NS, CS + (128, 129)))] + \
          [(257, 102, 512, 3, 5, 1.0, "zeroprob"), (5, 65, 64, 32, 2, 4.0, "zeroprob")]
assert {c[3] for c in E_CASES} == {1, 3, 32} and {c[4] for c in E_CASES} == {1, 2, 5} and {c[5] for c in E_CASES} == {0.0, 1.0, 4.0}


def case_id(case):
    return "-".join(f"{v:g}" if isinstance(v, float) else str(v) for v in case)
