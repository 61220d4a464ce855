"""float64 references and checkers for the label-propagation kernels (csrc/knn_graph.hip), shared by the GPU tests and shown to have teeth on
the host (tests/test_host_knn_ref.py).  Everything works on torch tensors of any device.  u = 2^-24.

SCORE BOUND.  The kernel's score is fl(fl(fl(q . x) * rq) * rx) with rq = fl(1 / sqrt(fl(sum q_d^2))), all f32.  Against the float64 cosine
s_ij = q^_i . x^_j (q^ = q / |q|) and with T_ij = sum_d |q^_id x^_jd| (>= |s_ij|), to first order in u:
    the f32 dot of e terms, in any order, with or without fused multiply-adds:      |err| <= e u sum_d |q_d x_d|      = e u T_ij |q| |x|
    a row's sum of squares (e positive terms, any order): relative (e + 1) u; the square root halves that and rounds once, the reciprocal
    rounds once: each reciprocal norm is relative ((e + 1) / 2 + 2) u, the two together (e + 5) u
    the two scalings: 2 u
so |score - s_ij| <= e u T_ij + (e + 7) u |s_ij| <= (2 e + 7) u T_ij; the bound asserted is
    r_ij = (2 e + 12) u T_ij
(five u of room for the second-order terms).  Nothing in it comes from a measurement.

PROPAGATION BOUND.  Z^{t+1}_i = fl(alpha * A_i + fl((1 - alpha)) p_i), A_i = sum_k w_ik Z^t_{idx_ik} as k fused multiply-adds in list order, run in
float64 on the SAME idx / sim (and the f32 values of alpha and gamma).  With b^t the bound on |Z^t(f32) - Z^t(f64)| (b^0 = 0: both start from probs):
    the error already in the neighbours' rows passes through the convex combination:       alpha sum_k w_ik b^t_{idx_ik}
    k fused multiply-adds (k u on sum_k w |Z|), the rounding of 1 - alpha, its product with p_i and the final fma (3 u): together at most
                                                                  (k + 8) u ((1 - alpha) |p_i| + alpha sum_k w_ik |Z^t_{idx_ik}|)
    the weights themselves are f32: x = fl(gamma * fl(sim_k - sim_0)) is relative 2 u, i.e. the exponential moves by 2 gamma |sim_k - sim_0| u;
    expf is within 2 u; the k-term sum is relative k u and the division rounds once:
                                          |dw_ik| <= (2 gamma |sim_ik - sim_i0| + k + 6) u w_ik + 2^-126   (the last term: a weight in the subnormal range)
    and they enter as                                                                      alpha sum_k |dw_ik| |Z^t_{idx_ik}|
b^{t+1}_i is the sum of the three (+ 2^-126 for a result in the subnormal range).  Every element is asserted against it, rows sum to 1 within the
row's summed bound (plus what the rows of probs themselves miss 1 by), argmax_out is the FIRST maximum of the kernel's own row, exactly."""
import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126


# ------------------------------------------------------------------------------------------ kNN graph
def cosine64(q, x):
    """(s64, r): the float64 cosines [n, m] and the score bound of the module docstring."""
    qd, xd = q.double(), x.double()
    qh, xh = qd / qd.norm(dim=1, keepdim=True), xd / xd.norm(dim=1, keepdim=True)
    return qh @ xh.T, (2 * q.shape[1] + 12) * U * (qh.abs() @ xh.abs().T)


def check_graph(q, x, idx, sim, self_offset=-1, duplicates=()):
    """Assert properties (a) - (e) of a kNN graph (idx int32 [n, k], sim f32 [n, k]) of queries q [n, e] against base x [m, e] on EVERY row; returns the worst
    |sim - s64| / r.  duplicates: pairs (lo, hi), lo < hi, of bit-identical base rows."""
    n, k = idx.shape
    m = x.shape[0]
    s64, r = cosine64(q, x)
    ix = idx.long()
    rows = torch.arange(n, device=ix.device)
    me = rows + self_offset if self_offset >= 0 else torch.full_like(rows, -1)
    # (a) in range, distinct, not the excluded row
    assert ((ix >= 0) & (ix < m)).all(), "(a) range: an index outside [0, m)"
    assert (torch.sort(ix, dim=1).values.diff(dim=1) > 0).all() if k > 1 else True, "(a) distinct: a row lists a base row twice"
    assert (ix != me[:, None]).all(), "(a) self: a row lists the row excluded for it"
    # (b) the scores
    err = (sim.double() - s64.gather(1, ix)).abs()
    rb = r.gather(1, ix)
    ratio = float((err / rb).max())
    assert torch.isfinite(sim).all() and (err <= rb).all(), f"(b) score: |sim - s64| is {ratio:.2f} x its bound"
    # (c) ordered by (sim descending, idx ascending) on the list's own values
    if k > 1:
        a, b = sim[:, :-1], sim[:, 1:]
        assert ((a > b) | ((a == b) & (ix[:, :-1] < ix[:, 1:]))).all(), "(c) order: a list is not sorted by (sim descending, index ascending)"
    # (d) selection: no row left out is better than a row returned by more than the two bounds
    out = torch.ones(n, m, dtype=torch.bool, device=ix.device)
    out.scatter_(1, ix, False)
    if self_offset >= 0:
        out[rows, me] = False
    lo_in = (s64 + r).gather(1, ix).min(dim=1).values
    hi_out = torch.where(out, s64 - r, torch.full_like(s64, -float("inf"))).max(dim=1).values
    bad = torch.nonzero(lo_in < hi_out).flatten()
    assert bad.numel() == 0, f"(d) selection: rows {bad[:8].tolist()} return a neighbour that is worse than one left out by more than the bounds"
    # (e) bit-identical base rows: the higher index only right behind the lower one, with the same bits
    for lo, hi in duplicates:
        assert lo < hi and torch.equal(x[lo], x[hi])
        has = ix == hi
        for i in torch.nonzero(has.any(dim=1)).flatten().tolist():
            if int(me[i]) == lo:
                continue            # (the lower twin is the row itself: excluded)
            p = int(torch.nonzero(has[i]).flatten()[0])
            assert p >= 1 and int(ix[i, p - 1]) == lo, f"(e) tie: row {i} lists duplicate {hi} without {lo} right before it"
            assert sim[i, p - 1].view(torch.int32) == sim[i, p].view(torch.int32), f"(e) tie: row {i} scores the duplicates {lo} and {hi} differently"
    return ratio


def knn_f32(q, x, k, self_offset=-1):
    """An f32 emulation of the kernel in torch (f32 matmul, f32 reciprocal norms on the score, stable sort): what the checker must accept."""
    s = (q @ x.T) * (1.0 / q.pow(2).sum(1).sqrt())[:, None] * (1.0 / x.pow(2).sum(1).sqrt())[None, :]
    if self_offset >= 0:
        rows = torch.arange(q.shape[0], device=q.device)
        s[rows, rows + self_offset] = -float("inf")
    val, ix = torch.sort(s, dim=1, descending=True, stable=True)
    return ix[:, :k].to(torch.int32).contiguous(), val[:, :k].contiguous()


# ------------------------------------------------------------------------------------------ propagation
def propagate64(probs, idx, sim, alpha, gamma, iters):
    """(Z64 [n, c], bound [n, c]) of the module docstring: the float64 recursion on the given idx / sim and the bound carried through it."""
    a, g = float(np.float32(alpha)), float(np.float32(gamma))
    n, k = idx.shape
    ix = idx.long()
    d = sim.double() - sim.double()[:, :1]
    w = torch.exp(g * d)
    w = w / w.sum(dim=1, keepdim=True)
    dw = (2 * g * d.abs() + k + 6) * U * w + TINY
    p = probs.double()
    z, b = p.clone(), torch.zeros_like(p)
    for _ in range(iters):
        zn, bn = z[ix], b[ix]                                        # [n, k, c]
        az = (w[:, :, None] * zn.abs()).sum(1)
        b = a * (w[:, :, None] * bn).sum(1) + (k + 8) * U * ((1 - a) * p.abs() + a * az) + a * (dw[:, :, None] * zn.abs()).sum(1) + TINY
        z = (1 - a) * p + a * (w[:, :, None] * zn).sum(1)
    return z, b


def check_propagation(probs, idx, sim, alpha, gamma, iters, out, argmax=None):
    """Assert every element of `out` against the float64 recursion, the row sums, and argmax (the first maximum of out's own row); returns the worst
    |err| / bound."""
    z, b = propagate64(probs, idx, sim, alpha, gamma, iters)
    err = (out.double() - z).abs()
    ratio = float((err / b).max())
    assert torch.isfinite(out).all() and (err <= b).all(), f"propagation: |Z - Z64| is {ratio:.2f} x its bound"
    miss = (probs.double().sum(1) - 1).abs().max()
    assert ((out.double().sum(1) - 1).abs() <= b.sum(1) + miss).all(), "propagation: a row does not sum to 1 within its bound"
    if argmax is not None:
        first = np.argmax(out.cpu().numpy(), axis=1)
        assert np.array_equal(argmax.cpu().numpy().astype(np.int64), first), "propagation: argmax_out is not the first maximum of the row"
    return ratio


def propagate_f32(probs, idx, sim, alpha, gamma, iters):
    """An f32 emulation of the kernel in torch (no fused multiply-adds): what the checker must accept."""
    a, g = torch.tensor(alpha, dtype=torch.float32), torch.tensor(gamma, dtype=torch.float32)
    ix = idx.long()
    w = torch.exp(g * (sim - sim[:, :1]))
    w = w / w.sum(dim=1, keepdim=True)
    z = probs.clone()
    for _ in range(iters):
        acc = torch.zeros_like(probs)
        for j in range(ix.shape[1]):
            acc = acc + w[:, j:j + 1] * z[ix[:, j]]
        z = a * acc + (1 - a) * probs
    return z, torch.from_numpy(np.argmax(z.cpu().numpy(), axis=1).astype(np.int32))


# ------------------------------------------------------------------------------------------ inputs
def embeddings(n, e, seed, device="cpu"):
    """[n, e] rows of norms 0.1 .. 30 (as the cache-head inputs)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, e, generator=g) * (0.1 + 29.9 * torch.rand(n, 1, generator=g)) / e ** 0.5).to(device)
