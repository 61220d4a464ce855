"""float64 references of the f32 tier (csrc/gemm_f32.hip, csrc/attention_f32.hip) and of the split-f16 tier (csrc/gemm_split.hip, the EMODE 3 epilogue of
csrc/gemm.hip, csrc/attention_split.hip) with a derived bound on |kernel - value| per element ("Tier kernel tests").  Plain torch float64 on
whatever device the inputs live on; nothing here calls the library.

u = 2^-24 (one f32 rounding).  The value is ALWAYS that of the f32 inputs as given -- the split of an operand into hi = f16(x), lo = f16(x - hi) is part of
the kernel, so what it loses (|x - hi - lo| <= 2^-22 |x| + 2^-25, weights carried x 2^8) is in the bound, not in the value.  Nothing in a bound is measured.

gemm_reference(inp, tier, epi, ...) returns {name: (value, bound)} for every buffer the launch writes; attention_reference(...) returns (value, bound)."""
import math

import torch

import attention_ref as AR
import gemm_ref as GR

U = 2.0 ** -24
REP_REL, REP_ABS = 2.0 ** -22, 2.0 ** -25      # hi + lo of an unscaled value: two f16 roundings, the second one's subnormal quantum
W_SCALE = 256.0                                # SP1_W_SCALE (csrc/common.h): weight images carry it, the floor of a weight is 2^-33 in units of w
EXP_ULP = 1.0                                  # expf of the ROCm device library: 1 ulp (HIP math API accuracy table, as DESIGN sections 11, 12): 2 u relative
F32_MIN = 2.0 ** -126                          # a result below the f32 normal range (flushed, or on the subnormal grid)
EPI_F32, EPI_BIAS, EPI_GELU, EPI_RESID, EPI_SCALE = 0, 1, 2, 3, 6
HAS_BIAS = (EPI_BIAS, EPI_GELU, EPI_RESID)
GEMM_FAMILIES = ("randn", "cancel", "onehot", "onehot_w", "grid", "lo-grid")
ATT_FAMILIES = ("randn", "peaked", "leak", "peaked_last", "peaked_first")


# ------------------------------------------------------------------------------------------------ the split representation and its layout
def split(x, scale=1.0):
    """hi = f16(x scale), lo = f16(x scale - hi) (round to nearest even, subnormals kept): what split_f16x4 must store."""
    x = x.float() * scale
    hi = x.half()
    return hi, (x - hi.float()).half()


def to_layout(hi, lo):
    """[rows, K] hi and lo -> the split layout: per row and 32 consecutive columns one line [32 hi | 32 lo], as f16 [rows, 2 K]."""
    rows, K = hi.shape
    return torch.stack([hi.reshape(rows, K // 32, 32), lo.reshape(rows, K // 32, 32)], 2).reshape(rows, 2 * K).contiguous()


def from_layout(buf, rows, K):
    """The split layout (any dtype of 4 bytes per element, or f16 [rows, 2 K]) -> (hi, lo), each [rows, K] f16."""
    v = buf.view(torch.float16).reshape(-1)[:rows * 2 * K].reshape(rows, K // 32, 2, 32)
    return v[:, :, 0].reshape(rows, K), v[:, :, 1].reshape(rows, K)


def dup_layout(hi):
    """The duplicated weight image [32 hi | 32 hi] of f16-exact weights."""
    return to_layout(hi, hi)


def _is_f16(x):
    return x.float().half().float() == x.float()


def rep_error(x, floor=REP_ABS):
    """|x - hi - lo| per element: 0 for an f16 number (hi = x, lo = 0), else 2^-22 |x| + the quantum of a lo below the f16 normal range."""
    x = x.double()
    return torch.where(_is_f16(x), torch.zeros_like(x), REP_REL * x.abs() + floor)


def lo_size(x, floor=2.0 ** -24):
    """|lo| per element: 0 for an f16 number, else |x - hi| <= 2^-11 |x| (or 2^-25 under a subnormal hi), rounded once more."""
    x = x.double()
    return torch.where(_is_f16(x), torch.zeros_like(x), 2.0 ** -11 * (1 + 2.0 ** -11) * x.abs() + floor)


def split_store(ref, e):
    """A value within e of ref written through store4(SplitRow) and read back as hi + lo."""
    return e + REP_REL * (ref.abs() + e) + REP_ABS


# ------------------------------------------------------------------------------------------------ QuickGELU of the f32 tower
def quick_gelu_exact(x, e_x, c=GR.GELU_C):
    """x / (1 + expf(-1.702f x)) with x within e_x (csrc/gemm_f32.hip): t = fl(-1.702) x is within 2 u |t| (the constant, the product); expf adds
    EXP_ULP ulp = 2 EXP_ULP u on top of exp's own |dt|; the add one rounding; the IEEE division half an ulp (u).  The denominator d = 1 + e has the
    relative error (1 - s) eps_e + u.  e_x goes through the derivative as in gemm_ref.quick_gelu (|g''| <= 0.851)."""
    t = GR.GELU_C * x.abs()
    s = torch.sigmoid(GR.GELU_C * x)
    eps_e = 2 * U * t + 2 * EXP_ULP * U
    rel = (1 - s) * eps_e + 2 * U
    g = x * torch.sigmoid(c * x)
    dg = s * (1 + GR.GELU_C * x * (1 - s))
    return g, (x * s).abs() * rel + dg.abs() * e_x + 0.5 * e_x * e_x + F32_MIN


# ------------------------------------------------------------------------------------------------ GEMM
def _nz(x):
    return (x != 0).double()


def gemm_reference(inp, tier, epi, w_exact=False, scalar=1.0, exact_sum=False):
    """{name: (value, bound)} of one launch.  tier 1: gemm_f32_kernel.  tier 2: gemm_split1_kernel (three passes) or, w_exact, gemm_k64p_kernel<EPI, 3, true>
    (two passes; every element of W is an f16 number).  "out" of the tier-2 GELU epilogue is what hi + lo of the split layout must give.
    exact_sum: a one-hot family -- every element has ONE non-zero hi.hi product, so the accumulator is hi (+ lo), exact in f32 (both lie on the grid of
    the f32 operand's last bit): no accumulation term (asserted here)."""
    A, W = inp["A"].double(), inp["W"].double()
    (M, K), N = A.shape, W.shape[0]
    has_bias = epi in HAS_BIAS
    bias = inp["bias"].double() if has_bias else torch.zeros(N, dtype=torch.float64, device=A.device)
    acc = A @ W.T + bias
    Saw = A.abs() @ W.abs().T
    if tier == 1:
        n_terms = _nz(A) @ _nz(W).T
        e_acc = (n_terms + 2) * U * (Saw + bias.abs())            # an fmaf chain in k order, started at the bias
        if exact_sum:
            assert float(n_terms.max()) <= 1
            e_acc = U * acc.abs() if has_bias else torch.zeros_like(acc)
    else:
        Ws = W * W_SCALE
        assert bool((Ws.abs() < 65520).all()), "weight image overflows f16"
        if w_exact:
            assert bool(_is_f16(Ws).all()), "w_exact: W must hold f16 numbers"
        # a w - (a_hi w_hi + a_hi w_lo + a_lo w_hi) = a_lo w_lo + r_a w + (a - r_a) r_w, per k, in units of w
        ra, la = rep_error(A), lo_size(A)
        rw, lw = rep_error(Ws) / W_SCALE, lo_size(Ws) / W_SCALE
        term = la @ lw.T + ra @ W.abs().T + (A.abs() + ra) @ rw.T
        # the chain: every non-zero product is one add into the single accumulator (products of f16 numbers are exact in f32), in any slice order
        a_hi, a_lo = _nz(A), _nz(la)
        w_hi, w_lo = _nz(W), _nz(lw)
        n_terms = a_hi @ w_hi.T + a_lo @ w_hi.T + a_hi @ w_lo.T
        S3 = Saw * (1 + 2.0 ** -9)                                 # |a_hi w_hi| + |a_hi w_lo| + |a_lo w_hi| <= (1 + 2^-11)(1 + 2 x 2^-11 (1 + 2^-11)) |a w| + floors
        S3 = S3 + 2.0 ** -24 * (_nz(la) @ W.abs().T) + 2.0 ** -32 * (A.abs() @ _nz(lw).T)
        if w_exact:           # the chain starts at 2^8 bias (exact) and is scaled by 2^-8 (exact)
            e_sum = (n_terms + 2) * U * (S3 + bias.abs())
            if exact_sum:
                # One or two non-zero products (hi, then lo) added onto 2^8 bias INSIDE the f16 MFMA.  Its adder is not specified as round-to-nearest (a
                # single such add came back 1.9 u off on the MI355X where the f32 MFMA and the VALU stay within u): each non-zero add is taken as
                # faithful -- the result one of the two neighbouring f32 numbers, an error below one ulp <= 2 u of the partial sum.  Without a bias
                # the adds are onto zero and of hi + lo: exact.
                assert float((a_hi @ w_hi.T).max()) <= 1
                e_sum = 2 * U * n_terms * (S3 + bias.abs()) if has_bias else torch.zeros_like(acc)
            e_acc = term + e_sum
        else:                 # the bias is added in the epilogue: one more rounding
            e_sum = (n_terms + 2) * U * S3
            if exact_sum:
                assert float((a_hi @ w_hi.T).max()) <= 1
                e_sum = torch.zeros_like(acc)
            e_acc = term + e_sum
            if has_bias:
                e_acc = e_acc + U * (acc.abs() + e_acc)
    res = {}
    if epi in (EPI_F32, EPI_BIAS):
        res["out"] = (acc, e_acc)
    elif epi == EPI_SCALE:
        assert tier == 1
        e = abs(scalar) * e_acc
        res["out"] = (acc * scalar, e + U * ((acc * scalar).abs() + e))
    elif epi == EPI_RESID:
        v = acc + inp["resid"].double()
        res["out"] = (v, e_acc + U * (v.abs() + e_acc))
    elif epi == EPI_GELU:
        if tier == 1:
            res["out"] = quick_gelu_exact(acc, e_acc)
            res["out2"] = (acc, e_acc)
        else:
            g, e_g = GR.quick_gelu(acc, e_acc)       # quick_gelu_exact_s: v_exp_f32 and v_rcp_f32, the form of DESIGN 15.1
            res["out"] = (g, split_store(g, e_g))
    else:
        raise ValueError(epi)
    return res


def make_gemm_inputs(family, M, N, K, seed, w_exact=False, device="cpu"):
    """Seeded f32 inputs of one case: A [M, K], W [N, K], bias [N], resid [M, N].  w_exact: W rounded to f16 numbers (the two-pass form)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    if family in ("randn", "cancel"):
        A = rn(M, K) * torch.exp(rn(1, K) * 0.7)          # the heavy-tailed column scale of LayerNorm outputs / MLP hiddens (tests/test_gpu_split.py)
        W = rn(N, K) * K ** -0.5
        if family == "cancel":
            # four pairs of columns (k, k + K / 2): A carries 32 c_r on both, W the same O(1) weight with opposite signs: the pair's products cancel
            # EXACTLY in the value and leave 2 x 32 |c w| in S
            ks = torch.arange(4) * 5 + 1
            c = 32.0 * (1 + rn(M, 1).abs())
            w = 1 + rn(N, 4).abs()
            if w_exact:
                w = w.half().float()
            A[:, ks], A[:, ks + K // 2] = c.expand(M, 4).clone(), c.expand(M, 4).clone()
            W[:, ks], W[:, ks + K // 2] = w, -w
        bias, resid = 0.5 * rn(N), rn(M, N)
    elif family == "onehot":
        # one 1 per row of A at k = 7 r mod K (all positions of a slice and all slices once M >= K: gcd(7, K) = 1): out = one weight
        A = torch.zeros(M, K)
        A[torch.arange(M), (7 * torch.arange(M)) % K] = 1.0
        W = rn(N, K) * K ** -0.5
        bias, resid = 0.5 * rn(N), rn(M, N)
    elif family == "onehot_w":
        # the mirror: one 1 per row of W at k = 5 n mod K, general A: out = one activation
        A = rn(M, K) * torch.exp(rn(1, K) * 0.7)
        W = torch.zeros(N, K)
        W[torch.arange(N), (5 * torch.arange(N)) % K] = 1.0
        bias, resid = 0.5 * rn(N), rn(M, N)
    elif family == "grid":
        a = GR.exact_magnitudes(K)
        A, W, bias, resid = ri(-a, a, M, K), ri(-1, 1, N, K), ri(-8, 8, N), ri(-8, 8, M, N)
    elif family == "lo-grid":
        # hi a small NON-ZERO integer, lo = +-2^-12: the split is lossless and every partial sum of the three formed products is a multiple of 2^-12
        nzint = lambda *s: ri(1, 3, *s) * (2 * ri(0, 1, *s) - 1)
        pm = lambda *s: (2 * ri(0, 1, *s) - 1) * 2.0 ** -12
        A = nzint(M, K) + pm(M, K)
        W = (nzint(N, K) + (0 if w_exact else pm(N, K))) / W_SCALE
        bias, resid = ri(-4, 4, N), ri(-4, 4, M, N)
    else:
        raise ValueError(family)
    if w_exact:
        W = W.half().float()
    return {k: v.float().contiguous().to(device) for k, v in dict(A=A, W=W, bias=bias, resid=resid).items()}


def assert_grid_family(inp, tier):
    """`grid`: every value an integer, the sum of the magnitudes of everything that enters an element (the 2^8 of the split tier's weight image included)
    below 2^24: every intermediate is exact in f32 in any order, and every lo part is zero."""
    A, W = inp["A"].double(), inp["W"].double()
    for t in (A, W, inp["bias"].double(), inp["resid"].double()):
        assert bool((t == t.round()).all())
    S = A.abs() @ W.abs().T + inp["bias"].double().abs() + inp["resid"].double().abs()
    assert float(S.max()) * (W_SCALE if tier == 2 else 1) < 2.0 ** 24
    if tier == 2:
        assert bool(_is_f16(A).all()) and bool(_is_f16(W * W_SCALE).all())


def lo_grid_expected(inp, epi):
    """`lo-grid`: the value the split kernels must give EXACTLY, sum (a w - a_lo w_lo) [+ bias [+ resid]], with the conditions that make it so asserted:
    the split is lossless, all formed products (in the image's 2^8 units) are multiples of 2^-12, the sum of their magnitudes and of 2^8 (|bias| + |resid|)
    is below 2^24 in that unit, and the epilogue's value (multiples of 2^-20 once the 2^8 is divided out) stays below 2^4."""
    a_hi, a_lo = (t.double() for t in split(inp["A"]))
    w_hi, w_lo = (t.double() for t in split(inp["W"], W_SCALE))
    assert bool((a_hi + a_lo == inp["A"].double()).all()) and bool((w_hi + w_lo == inp["W"].double() * W_SCALE).all())
    assert bool((a_hi != 0).all()) and bool((w_hi != 0).all())
    unit = 2.0 ** 12
    for t in (a_hi, a_lo, w_hi, w_lo):
        assert bool((t * unit == (t * unit).round()).all())
    # products: hi hi integers, hi lo multiples of 2^-12 (hi an integer); all multiples of 2^-12
    mag = a_hi.abs() @ w_hi.abs().T + a_hi.abs() @ w_lo.abs().T + a_lo.abs() @ w_hi.abs().T
    extra = (inp["bias"].double().abs() + inp["resid"].double().abs()) * W_SCALE
    assert float((mag + extra).max()) * unit < 2.0 ** 24
    v = (a_hi @ w_hi.T + a_hi @ w_lo.T + a_lo @ w_hi.T) / W_SCALE
    if epi in HAS_BIAS:
        v = v + inp["bias"].double()
    if epi == EPI_RESID:
        v = v + inp["resid"].double()
    assert float(v.abs().max()) < 16 and bool((v * 2.0 ** 20 == (v * 2.0 ** 20).round()).all())
    return v


# ------------------------------------------------------------------------------------------------ attention
def make_attention_inputs(family, B, S, H, causal, seed, device="cpu"):
    """qkv [B*S, 3 H 64] f32.  randn / peaked / leak: attention_ref's families, every element pushed off the f16 grid by a relative 2^-12 .. 2^-13 (the
    split kernels must need their lo parts).  peaked_last / peaked_first: every row's dominant key is its last visible one (the running maximum of the
    tiled kernel rises in the LAST 32-key tile: a late rescale of everything accumulated) / key 0 (no rescale after the first tile)."""
    g = torch.Generator().manual_seed(seed + 77)
    if family in AR.FAMILIES:
        qkv = AR.make_inputs(family, B, S, H, causal, seed)[0].float()
    else:
        q, k, v = (torch.randn(B, H, S, 64, generator=g) for _ in range(3))
        i = torch.arange(S)
        t = (i if causal else torch.full((S,), S - 1)) if family == "peaked_last" else torch.zeros(S, dtype=torch.long)
        q = 3.0 * q + 3.0 * k[:, :, t]
        v = torch.sign(v) * (0.5 + v.abs()).clamp_max(4.0)
        qkv = torch.cat((AR.rows(q), AR.rows(k), AR.rows(v)), dim=1)
    qkv = qkv * (1 + 2.0 ** -13 * (1 + torch.rand(qkv.shape, generator=g)))
    return qkv.float().contiguous().to(device)


def _per_row(x, B, S, H):
    """[B, H, S, 1] -> [B*S, H*64]."""
    return AR.rows(x.expand(B, H, S, 64))


def attention_terms(qkv, B, S, H, causal):
    """attention_ref.attention on the f32 values, plus per query row (expanded over its head's 64 columns): amax = the largest sum_d |q_d k_d| / 8 over its
    visible keys, dsplit = the largest error of a three-pass split score, n_vis = its visible keys."""
    res = AR.attention(qkv, B, S, H, causal)
    q, k, _ = AR.unpack(qkv, B, S, H)
    q = q / 8.0
    vis = torch.ones(S, S, dtype=torch.bool, device=qkv.device)
    if causal:
        vis = vis.tril()
    Aij = q.abs() @ k.abs().transpose(-1, -2)
    # the three-pass score, K = 64, nothing scaled: a_lo w_lo + r_q k + (q + r_q) r_k per dim, then (3 x 64 + 2) u sum |terms|
    rq, lq, rk, lk = rep_error(q), lo_size(q), rep_error(k), lo_size(k)
    d = lq @ lk.transpose(-1, -2) + rq @ k.abs().transpose(-1, -2) + (q.abs() + rq) @ rk.transpose(-1, -2) + (3 * 64 + 2) * U * Aij * (1 + 2.0 ** -9)
    neg = torch.zeros_like(Aij).masked_fill(~vis, float("-inf"))
    res["amax"] = _per_row((Aij + neg).amax(-1, keepdim=True), B, S, H)
    res["dsplit"] = _per_row((d + neg).amax(-1, keepdim=True), B, S, H)
    res["n_vis"] = _per_row(vis.double().sum(-1)[None, None, :, None].expand(B, H, S, 1), B, S, H)
    return res


def bound_attention_f32(res, split_out=False):
    """attn_fwd_f32_kernel: attention_ref.bound_exact's count (the f32 score chain, the f32 sums of S terms, exp and division) plus what the running-maximum
    form adds to a probability's relative error -- s - m rounded once (u |s - m| <= 2 u A, absolute in the exponent), the same for every m - m' of a rescale
    (they telescope: the maximum rises by at most 2 A in all), and per 32-key tile corr = expf (EXP_ULP ulp), l *= corr and o *= corr (one rounding each) --
    twice: in the numerator and in the row sum.  split_out: the store into the split layout."""
    tiles = math.ceil(res["S"] / 32)
    extra = 2 * (4 * res["A"] + 2 * EXP_ULP + tiles * (2 * EXP_ULP + 1)) * U * res["scale_o"]
    e = AR.bound_exact(res) + extra
    return split_store(res["out"], e) if split_out else e


def bound_attention_split(res):
    """attn_fwd_split_kernel.  A probability p~ = exp2(fma(s, log2 e, -m log2 e)) has the relative error rel = expm1(dsplit + 4 u amax) + 2 u: the split score
    (attention_terms), the fma (u |s - m| log2 e + the constant's u |s| log2 e, times ln 2: <= 3 u amax), m log2 e (u amax) and v_exp_f32 (1 ulp = 2 u).
    P is split UNSCALED (2^-22 p~ + 2^-25 per key), V is split, and the product drops p_lo v_lo: per key 3 x 2^-22 p~ |v| + 2^-25 (|v| + p~); with the
    row sum L >= 1 this is 3 x 2^-22 scale_o + 2^-25 sub_o in units of the output (sub_o = sum_j |v_j| + n |ref|: attention_ref).  The chains: 3 n + 2 adds
    for o (+ oc), n + 2 for each half of the row sum, the adds o + oc and sum_h + sum_l, the division and the product: 6 u.  Then the split store."""
    n = res["n_vis"]
    rel = torch.expm1(res["dsplit"] + 4 * U * res["amax"]) + 2 * U
    ref, so = res["out"].abs(), res["scale_o"]
    e = rel * (so + ref)
    e = e + 3 * REP_REL * (1 + 2.0 ** -10) * so + REP_ABS * (1 + 2.0 ** -9) * (res["sub_o"] + 1) + REP_REL * ref
    e = e + (3 * n + 2) * U * so * (1 + 2.0 ** -9) + (n + 2) * U * ref + 6 * U * ref
    return split_store(res["out"], e)
