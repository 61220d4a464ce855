"""float64 references of the f16 GEMM epilogues (csrc/gemm.hip) with a derived bound on |kernel - value| per element ("f16 GEMM kernel
tests").  Plain torch float64 on whatever device the inputs live on; nothing here calls the library.

Everything is computed on the inputs exactly as the kernel reads them (f16 A, W, resid, aux; f32 bias, rowstat, colsum, stat_in).  u = 2^-24 (one f32
rounding), h = 2^-11 (one f16 rounding), q = 2^-25 (half the f16 subnormal spacing).  S = |A| |W|^T + |bias|.  The accumulator -- a chain of K exact
products added one rounding each onto the bias, in ANY slice order -- is within E(acc) = (K + 2) u S of the value; `ksplit` partial sums added in index
order add (ksplit - 1) u S.  Every later step adds its own rounding and carries the error of its operands; nothing in a bound is measured.

reference(inp, epi, ...) returns {name: (value, bound)} for every buffer the launch writes.  `fault` names ONE deliberate error applied to the value
(never to the bound): tests/test_host_gemm_ref.py shows with them that the bound is not vacuous."""
import math

import torch

from rowops_fwd_ref import stats_finalize

U, H, Q = 2.0 ** -24, 2.0 ** -11, 2.0 ** -25
EPI_F32, EPI_BIAS_F16, EPI_BIAS_GELU_F16, EPI_BIAS_RESID, EPI_F16, EPI_GELUGRAD_F16, EPI_F32_SCALE, EPI_LNFOLD_F16, EPI_LNFOLD_GELU_F16, EPI_BIAS_RESID_STATS = range(10)
HAS_BIAS = (EPI_BIAS_F16, EPI_BIAS_GELU_F16, EPI_BIAS_RESID, EPI_BIAS_RESID_STATS)
FOLD = (EPI_LNFOLD_F16, EPI_LNFOLD_GELU_F16)
RESID = (EPI_BIAS_RESID, EPI_BIAS_RESID_STATS)
F32_OUT = (EPI_F32, EPI_F32_SCALE)
FAMILIES = ("randn", "cancel", "exact", "onehot")
GELU_C = 1.702
FAULTS = ("drop_slice", "double_slice", "bias_neighbour", "resid_next_row", "gelu_1p7", "aux_next_row", "drop_colsum_mean", "rstd_next_row", "drop_partial_17",
          "stat_neighbour_tile", "stat_of_rounded", "lo_of_unrounded_hi", "scale_twice")


def half_store(ref, e):
    """An f32 value within e of ref, rounded to f16 (subnormals kept): within e + h (|ref| + e) + q."""
    return e + H * (ref.abs() + e) + Q


def _sigmoid(x):
    """s = 1 / (1 + exp2(c x)) as the kernel forms it, c = fl(-1.702 log2 e) (three roundings from the true constant), x exact: (s, relative error of s).
    t = c x is within 4 u |t|; v_exp_f32 is 1 ulp (2 u) on top of exp2's own ln 2 |dt|; 1 + e one rounding; v_rcp_f32 1 ulp (2 u)."""
    t = GELU_C * 1.4426950408889634 * x.abs()
    eps_e = math.log(2.0) * 4 * U * t + 2 * U
    s = torch.sigmoid(GELU_C * x)
    return s, eps_e * (1 - s) + 3 * U


def quick_gelu(x, e_x, c=GELU_C):
    """x s(x) with x within e_x: the sigmoid's relative error, the product's rounding, and e_x through the derivative (|g''| <= 0.851 everywhere: the
    second-order term is at most e_x^2 / 2).  2^-100: the sigmoid where exp2 overflows (the kernel returns 0 for a value below 2^-128)."""
    s, eps = _sigmoid(x)
    g = x * torch.sigmoid(c * x)
    dg = s * (1 + GELU_C * x * (1 - s))
    return g, (x * s).abs() * (eps + U) + dg.abs() * e_x + 0.5 * e_x * e_x + 2.0 ** -100


def quick_gelu_grad(x):
    """d = s (1 + (1.702 x) (1 - s)) on an exact f16 x: (value, bound), the five f32 operations of quick_gelu_grad counted one rounding each (a contraction
    has fewer) and fl(1.702) one more."""
    s, eps = _sigmoid(x)
    a = (GELU_C * x).abs()
    b = a * (1 - s)
    c = 1 + GELU_C * x * (1 - s)
    e_c = a * (3 * U * (1 - s) + s * eps) + U * b + U * c.abs()
    d = s * c
    return d, s * e_c + c.abs() * s * eps + U * d.abs()


def tile_stats(v, e_v):
    """(sum, sum of squares) of the f32 v per row and 64-column tile: (v0 + v1) + (v2 + v3) and four DPP levels (6 adds deep); a four-term fma chain and four
    levels (8 roundings deep) -- the counts of DESIGN.md section 12.1.  -> ((sum, E), (sq, E)), each [N / 64, M]."""
    M, N = v.shape
    vt, et = v.reshape(M, N // 64, 64), e_v.reshape(M, N // 64, 64)
    sm, sq = vt.sum(-1), (vt * vt).sum(-1)
    e_sm = et.sum(-1) + 6 * U * vt.abs().sum(-1)
    e_sq = (2 * vt.abs() * et + et * et).sum(-1) + 8 * U * sq
    return (sm.T.contiguous(), e_sm.T.contiguous()), (sq.T.contiguous(), e_sq.T.contiguous())


def reference(inp, epi, ksplit=1, scalar=1.0, stats=False, hi_stored=None, fault=None, slice0=0):
    """{name: (value, bound)}: "out", and where the launch writes them "out2", "stat_part" [N / 64, M, 2], "hilo" (hi + lo of a compensated stream; with
    hi_stored given also "lo", the value the kernel must have stored beside ITS hi).  epi 3 with stats = True is the statistics-carrying form.  slice0: first
    column of the 32-wide K slice the slice faults act on."""
    A, W = inp["A"].double(), inp["W"].double()
    (M, K), N = A.shape, W.shape[0]
    bias = inp["bias"].double() if epi in HAS_BIAS or epi in FOLD else torch.zeros(N, dtype=torch.float64, device=A.device)
    mm_bias = bias if epi in HAS_BIAS else torch.zeros_like(bias)
    Af = A
    if fault in ("drop_slice", "double_slice"):
        Af = A.clone()
        Af[:, slice0:slice0 + 32] *= 0.0 if fault == "drop_slice" else 2.0
    acc = Af @ W.T + (mm_bias.roll(-4) if fault == "bias_neighbour" else mm_bias)
    S = A.abs() @ W.abs().T + mm_bias.abs()
    e_acc = (K + 2 + ksplit - 1) * U * S
    res = {}
    if epi == EPI_F32:
        res["out"] = (acc, e_acc)
    elif epi == EPI_F32_SCALE:
        ref = acc * scalar * (scalar if fault == "scale_twice" else 1.0)
        e = abs(scalar) * e_acc
        res["out"] = (ref, e + U * ((acc * scalar).abs() + e))
    elif epi in (EPI_F16, EPI_BIAS_F16):
        res["out"] = (acc, half_store(acc, e_acc))
    elif epi == EPI_BIAS_GELU_F16:
        g, e_g = quick_gelu(acc, e_acc, 1.7 if fault == "gelu_1p7" else GELU_C)
        res["out"] = (g, half_store(quick_gelu(acc, e_acc)[0], e_g))
        res["out2"] = (acc, half_store(acc, e_acc))
    elif epi in RESID:
        r = inp["resid"].double()
        if "resid_lo" in inp:
            r = r + inp["resid_lo"].double()        # exact in f32 for a pair split off one f32 number (make_inputs)
        if fault == "resid_next_row":
            r = r.roll(-1, 0)
        v = acc + r
        true = A @ W.T + mm_bias + (inp["resid"].double() + (inp["resid_lo"].double() if "resid_lo" in inp else 0.0))
        e_v = e_acc + U * (true.abs() + e_acc)
        res["out"] = (v, half_store(true, e_v))
        if "resid_lo" in inp:
            res["hilo"] = (v, e_v + 2.0 ** -22 * (true.abs() + e_v) + 2 * Q)
            if hi_stored is not None:
                d = true - hi_stored.double()
                res["lo"] = (v - (v if fault == "lo_of_unrounded_hi" else hi_stored.double()), e_v + H * (d.abs() + e_v) + Q)
        if stats or epi == EPI_BIAS_RESID_STATS:
            sv = v.half().double() if fault == "stat_of_rounded" else v
            (sm, e_sm), (sq, e_sq) = tile_stats(sv, e_v)
            (_, e_sm), (_, e_sq) = tile_stats(true, e_v)
            if fault == "stat_neighbour_tile":
                sm, sq = sm.roll(-1, 0), sq.roll(-1, 0)
            res["stat_part"] = (torch.stack([sm, sq], -1), torch.stack([e_sm, e_sq], -1))
    elif epi == EPI_GELUGRAD_F16:
        x = inp["aux"].double()
        d, e_d = quick_gelu_grad(x.roll(-1, 0) if fault == "aux_next_row" else x)
        d0, e_d = quick_gelu_grad(x)
        ref = acc * d
        e = d0.abs() * e_acc + acc.abs() * e_d + e_acc * e_d
        e = e + U * ((acc * d0).abs() + e)
        res["out"] = (ref, half_store(acc * d0, e))
    elif epi in FOLD:
        cs = inp["colsum"].double()
        if "stat_in" in inp:
            part = inp["stat_in"]
            if fault == "drop_partial_17":
                part = torch.cat([part[:16], part[17:]])
            mean, _, rstd, _ = stats_finalize(part, K)
            _, e_mean, _, e_rstd = stats_finalize(inp["stat_in"], K)
            mean0, _, rstd0, _ = stats_finalize(inp["stat_in"], K)
        else:
            mean0, rstd0 = inp["rowstat"].double()[:, :1], inp["rowstat"].double()[:, 1:]
            mean, rstd = mean0, rstd0
            e_mean = e_rstd = torch.zeros_like(mean)
        if fault == "rstd_next_row":
            rstd = rstd.roll(-1, 0)
        p = cs * mean * (0.0 if fault == "drop_colsum_mean" else 1.0)
        y = (acc - p) * rstd + bias
        # the bound, on the unfaulted values: p = cs mean (one rounding, E(mean) carried); d = acc - p is a cancellation, its error is that of its operands;
        # m = d rstd; y = m + bias'
        p0 = cs * mean0
        e_p = cs.abs() * e_mean + U * (p0.abs() + cs.abs() * e_mean)
        d0 = acc - p0
        e_d = e_acc + e_p
        e_d = e_d + U * (d0.abs() + e_d)
        m0 = d0 * rstd0
        e_m = rstd0.abs() * e_d + d0.abs() * e_rstd + e_d * e_rstd
        e_m = e_m + U * (m0.abs() + e_m)
        y0 = m0 + bias
        e_y = e_m + U * (y0.abs() + e_m)
        if epi == EPI_LNFOLD_F16:
            res["out"] = (y, half_store(y0, e_y))
        else:
            g, _ = quick_gelu(y, e_y, 1.7 if fault == "gelu_1p7" else GELU_C)
            g0, e_g = quick_gelu(y0, e_y)
            res["out"] = (g, half_store(g0, e_g))
            res["out2"] = (y, half_store(y0, e_y))
    else:
        raise ValueError(epi)
    return res


def split_hilo(x):
    """An f32 tensor as a compensated f16 pair: hi = f16(x), lo = f16(x - hi).  hi + lo is then exact in f32 (both lie on the grid of x's last bit)."""
    hi = x.float().half()
    return hi, (x.float() - hi.float()).half()


def exact_magnitudes(K):
    """`exact` family: A in [-a, a], W in [-1, 1], bias and resid in [-8, 8], all integers.  A row of K products has a standard deviation of
    sqrt(K (a (a + 1) / 3) (2 / 3)) <= 37 for a = 2 (K <= 1024) and a = 1 (longer): every partial sum stays far below 2^24 (exact in f32 in any order) and,
    asserted on the reference by assert_exact_family, |v| < 512 so that a 64-column tile's sum of squares stays below 2^24 too."""
    return 2 if K <= 1024 else 1


def make_inputs(family, M, N, K, seed, device="cpu", stat_parts=0, hilo=False):
    """Seeded inputs of one case, every buffer an epilogue may read: A [M, K], W [N, K], resid, aux [M, N] f16; bias, colsum [N], rowstat [M, 2] f32; with
    stat_parts = K / 64 the per-64-column partial (sum, sum of squares) of A's rows as stat_in [parts, M, 2]; with hilo the pair resid / resid_lo."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    inp = {}
    if family in ("randn", "cancel"):
        A, W = rn(M, K), rn(N, K) * K ** -0.5
        if family == "cancel":
            # four pairs of columns (k, k + K / 2): A carries +-32 c_r on both, W the same O(1) weight with opposite signs.  The pair's products cancel
            # EXACTLY in the value and leave 2 x 32 |c w| in S: S >= 64 |ref| on most elements, |ref| stays O(1)
            ks = torch.arange(4) * 5 + 1
            c = 32.0 * (1 + rn(M, 1).abs())
            w = (1 + rn(N, 4).abs()).half().float()
            A[:, ks], A[:, ks + K // 2] = c.expand(M, 4).clone(), c.expand(M, 4).clone()
            A = A.half().float()
            A[:, ks + K // 2] = A[:, ks]
            W[:, ks], W[:, ks + K // 2] = w, -w
        bias, resid, aux = 0.5 * rn(N), rn(M, N), 2.0 * rn(M, N)
        resid32 = resid
    elif family == "exact":
        a = exact_magnitudes(K)
        A, W, bias, resid, aux = ri(-a, a, M, K), ri(-1, 1, N, K), ri(-8, 8, N), ri(-8, 8, M, N), ri(-3, 3, M, N)
        resid32 = resid
    elif family == "onehot":
        A = torch.zeros(M, K)
        A[torch.arange(M), (7 * torch.arange(M)) % K] = 1.0
        # |W| <= 254 (f16 integers; with bias and resid |v| < 512: a tile's squares sum exactly), distinct over any 509 consecutive k or n (509 is prime)
        W = ((131 * torch.arange(N)[:, None] + 7 * torch.arange(K)[None]) % 509 - 254).float()
        bias, resid, aux = ri(-8, 8, N), ri(-8, 8, M, N), ri(-3, 3, M, N)
        resid32 = resid
    else:
        raise ValueError(family)
    inp.update(A=A.half(), W=W.half(), bias=bias.float(), aux=aux.half())
    if hilo:
        if family in ("randn", "cancel"):
            resid32 = resid * (1 + 1e-4 * rn(M, N))
        else:
            resid32 = resid + ri(-1, 1, M, N) * 2.0 ** -12            # an integer stream with a nonzero low half, hi + lo + acc still exact in f32
        inp["resid"], inp["resid_lo"] = split_hilo(resid32)
    else:
        inp["resid"] = resid.half()
    Ad, Wd = inp["A"].double(), inp["W"].double()
    if family in ("exact", "onehot"):       # integer colsum and mean, rstd a power of two: the folded value is exact in f32
        inp["colsum"] = ri(-4, 4, N)
        inp["rowstat"] = torch.stack([ri(-3, 3, M), 2.0 ** ri(-2, 1, M)], -1)
    else:
        inp["colsum"] = Wd.sum(-1).float()
        mean, var = Ad.mean(-1), Ad.var(-1, unbiased=False)
        inp["rowstat"] = torch.stack([mean, (var + 1e-5).rsqrt()], -1).float()
    if stat_parts:
        assert stat_parts * 64 == K
        t = Ad.reshape(M, stat_parts, 64)
        inp["stat_in"] = torch.stack([t.sum(-1).T, (t * t).sum(-1).T], -1).float().contiguous()
    return {k: v.contiguous().to(device) for k, v in inp.items()}


def assert_exact_family(inp, res, epi):
    """The arithmetic that makes `exact` and `onehot` exact, asserted on the float64 reference: every value is a multiple of 2^-12 (integers; 2^-2 after a
    power-of-two rstd; 2^-12 in the compensated stream's low half) and the sum of the magnitudes of everything that enters an element stays below 2^24 in
    that unit -- so every intermediate is exact in f32, in any order -- and |v| < 512 where a tile's 64 squares are summed (their sum stays below 2^24)."""
    S = inp["A"].double().abs() @ inp["W"].double().abs().T
    # + 64: |bias| + |resid| + |colsum mean| + |bias'| <= 8 + 9 + 12 + 8; x 2: the largest rstd; x 4096: the unit of the last bit
    assert (float(S.max()) + 64) * 2 * 4096 < 2.0 ** 24, float(S.max())
    for name in exact_names(epi, "hilo" in res):
        if name not in res:
            continue
        ref = res[name][0]
        assert bool((ref * 4096 == (ref * 4096).round()).all()), name
    if "stat_part" in res:
        v = res["out"][0]
        assert float(v.abs().max()) < 512, float(v.abs().max())


def exact_names(epi, hilo=False):
    """The outputs that are exact on the `exact` and `onehot` families (QuickGELU and its derivative are not: they stay under the bound; nor are the squares
    of a compensated stream, whose values carry a 2^-12 low half: 2^-24 in the square)."""
    if epi in (EPI_BIAS_GELU_F16, EPI_LNFOLD_GELU_F16):
        return ("out2",)
    if epi == EPI_GELUGRAD_F16:
        return ()
    if epi in RESID:
        return ("out", "hilo", "lo") if hilo else ("out", "stat_part")
    return ("out",)
