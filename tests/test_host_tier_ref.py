"""CPU: the float64 references and bounds of the f32 and split-f16 tier kernels (tests/tier_ref.py; DESIGN.md, "Tier kernel tests").

(a) every kernel's arithmetic, restated in numpy float32 / float16 -- the f32 fmaf chain in k order; the three-pass and two-pass split chains with the
    32-wide K slices sequential, reversed and rotated by every start slice; the online softmax over 32-key tiles; the split attention with its hi / lo
    products -- stays within the bound on every element of every input family (and is bit-equal to float64 on the exact families);
(b) single faults applied to those restatements leave it on at least one element."""
import json

import numpy as np
import pytest
import torch

import tier_ref as T

F, H16 = np.float32, np.float16
KS = (64, 128, 256, 768)
M, N = 8, 32
SCALAR = 0.375
LOG2E = F(1.4426950408889634)


def np_split(x, scale=1.0):
    x = (x.astype(F) * F(scale)).astype(F)
    hi = x.astype(H16)
    return hi.astype(F), (x - hi.astype(F)).astype(H16).astype(F)


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def slice_orders(K):
    """[orders, K / 32] slice indices: sequential, reversed, rotated by every start slice."""
    ns = K // 32
    return np.array([list(range(ns)), list(range(ns))[::-1]] + [[(s + r) % ns for s in range(ns)] for r in range(1, ns)])


# ------------------------------------------------------------------------------------------------ GEMM restatements
def chain_f32(inp, has_bias):
    """gemm_f32_kernel: acc = bias; acc = fmaf(a_k, w_k, acc) for k ascending."""
    A, W = inp["A"].numpy(), inp["W"].numpy()
    acc = np.broadcast_to(inp["bias"].numpy() if has_bias else np.zeros(W.shape[0], F), (A.shape[0], W.shape[0])).astype(F)
    for k in range(A.shape[1]):
        acc = fma32(A[:, k, None], W[None, :, k], acc)
    return acc[None]


def chain_split(inp, has_bias, w_exact, fault=None):
    """The split kernels' accumulator for every slice order [orders, M, N], already divided by 2^8.  Three passes: per slice the 32 hi.hi products, then
    w_lo a_hi, then w_hi a_lo, one add each.  Two passes (w_exact): the chain starts at 2^8 bias; per slice a_hi w then a_lo w."""
    a_hi, a_lo = np_split(inp["A"].numpy())
    w_hi, w_lo = np_split(inp["W"].numpy(), T.W_SCALE)
    if fault == "lo_neighbour_line":
        a_lo = np.roll(a_lo, 32, axis=1)
    K = a_hi.shape[1]
    sl = slice_orders(K)
    start = inp["bias"].numpy() * F(T.W_SCALE) if (w_exact and has_bias) else np.zeros(w_hi.shape[0], F)
    acc = np.broadcast_to(start, (sl.shape[0], a_hi.shape[0], w_hi.shape[0])).astype(F)
    frag = np.ones(w_hi.shape[0], F)
    if fault == "drop_alo_fragment":
        frag[16:32] = 0
    passes = [(a_hi, w_hi), (a_lo, w_hi)] if w_exact else [(a_hi, w_hi), (a_hi, w_lo), (a_lo, w_hi * frag[:, None])]
    if fault == "drop_wlo":
        passes = [passes[0], passes[2]]
    for step in range(sl.shape[1]):
        for x, y in passes:
            for j in range(32):
                k = 32 * sl[:, step] + j
                acc += x[:, k].T[:, :, None] * y[:, k].T[:, None, :]
    return acc if fault == "no_unscale" else acc * F(1 / T.W_SCALE)


def epilogue(inp, tier, epi, acc, w_exact, fault=None):
    """{name: float64 array [orders, M, N]} from accumulators: gemm_f32_kernel's epilogue, gemm_split1_kernel's (bias added here) or
    epilogue_rows_split_impl's (bias already in the chain).  The split layout is read back as hi + lo."""
    bias, resid = inp["bias"].numpy(), inp["resid"].numpy()
    if fault == "bias_neighbour":
        bias = np.roll(bias, -1)
    if fault == "resid_next_row":
        resid = np.roll(resid, -1, axis=0)
    v = acc
    if tier == 2 and not w_exact and epi in T.HAS_BIAS:
        v = v + bias
    out = {}
    if epi == T.EPI_SCALE:
        v = v * F(SCALAR)
    if epi == T.EPI_RESID:
        v = v + resid
    if epi == T.EPI_GELU:
        c = F(1.7) if fault == "gelu_1p7" else F(1.702)
        with np.errstate(over="ignore"):
            if tier == 1:
                out["out2"] = v.astype(np.float64)
                v = v / (F(1) + np.exp(-c * v, dtype=F))
            else:
                v = v * (F(1) / (F(1) + np.exp2(F(-c * LOG2E) * v, dtype=F)))
                hi, lo = np_split(v)
                if fault == "split_ulp":       # lo taken from a value one f16 ulp away from the one hi was rounded from
                    lo = ((v + np.spacing(hi.astype(H16)).astype(F)) - hi).astype(H16).astype(F)
                out["out"] = hi.astype(np.float64) + lo.astype(np.float64)
                return out
    out["out"] = v.astype(np.float64)
    return out


def accumulate(inp, tier, epi, w_exact, fault=None):
    has_bias = epi in T.HAS_BIAS
    if fault == "bias_neighbour" and (tier == 1 or w_exact):      # the bias enters through the chain's start
        inp = dict(inp, bias=inp["bias"].roll(-1))
    return chain_f32(inp, has_bias) if tier == 1 else chain_split(inp, has_bias, w_exact, fault)


def worst_ratio(got, res):
    w = 0.0
    for name, (ref, bound) in res.items():
        err = np.abs(got[name] - ref.numpy())
        assert np.isfinite(err).all(), name
        bn = bound.numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            w = max(w, float(np.where(bn > 0, err / bn, np.where(err == 0, 0.0, np.inf)).max()))
    return w


FORMS = [(1, False), (2, False), (2, True)]        # f32 kernel, three passes, two passes


def epis_of(tier):
    return (0, 1, 2, 3, 6) if tier == 1 else (0, 1, 2, 3)


def families_of(tier, K):
    return [f for f in T.GEMM_FAMILIES if not (f == "lo-grid" and (tier == 1 or K > 128))]


# ------------------------------------------------------------------------------------------------ (a) GEMM
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("tier,w_exact", FORMS)
def test_the_gemm_restatements_stay_within_the_bound(tier, w_exact, K):
    worst = {}
    for family in families_of(tier, K):
        inp = T.make_gemm_inputs(family, M, N, K, 11 + K, w_exact=w_exact)
        accs = {}
        for epi in epis_of(tier):
            hb = epi in T.HAS_BIAS
            if hb not in accs:
                accs[hb] = accumulate(inp, tier, epi, w_exact)
            got = epilogue(inp, tier, epi, accs[hb], w_exact)
            res = T.gemm_reference(inp, tier, epi, w_exact=w_exact, scalar=SCALAR, exact_sum=family.startswith("onehot"))
            r = worst_ratio(got, res)
            assert r <= 1.0, (family, epi, r)
            worst[family] = max(worst.get(family, 0.0), r)
            if family == "grid" and epi != T.EPI_GELU:
                T.assert_grid_family(inp, tier)
                assert np.array_equal(got["out"], np.broadcast_to(res["out"][0].numpy(), got["out"].shape)), (family, epi)
            if family == "lo-grid" and epi != T.EPI_GELU:
                want = T.lo_grid_expected(inp, epi).numpy()
                assert np.array_equal(got["out"], np.broadcast_to(want, got["out"].shape)), (family, epi)
    print("worst |err| / bound, tier %d w_exact %d K=%d:" % (tier, w_exact, K), json.dumps({k: round(v, 3) for k, v in worst.items()}))


# ------------------------------------------------------------------------------------------------ (b) GEMM
GEMM_FAULTS = [
    ("drop_alo_fragment", 2, False, 0), ("drop_wlo", 2, False, 0), ("lo_neighbour_line", 2, False, 0), ("lo_neighbour_line", 2, True, 0),
    ("no_unscale", 2, True, 1), ("bias_neighbour", 1, False, 1), ("bias_neighbour", 2, False, 1), ("bias_neighbour", 2, True, 1),
    ("resid_next_row", 1, False, 3), ("resid_next_row", 2, False, 3), ("resid_next_row", 2, True, 3),
    ("gelu_1p7", 1, False, 2), ("gelu_1p7", 2, False, 2), ("gelu_1p7", 2, True, 2), ("split_ulp", 2, False, 2), ("split_ulp", 2, True, 2),
]


@pytest.mark.parametrize("fault,tier,w_exact,epi", GEMM_FAULTS)
def test_a_single_gemm_fault_leaves_the_bound(fault, tier, w_exact, epi):
    K = 128
    inp = T.make_gemm_inputs("randn", M, N, K, 11 + K, w_exact=w_exact)
    res = T.gemm_reference(inp, tier, epi, w_exact=w_exact, scalar=SCALAR)
    assert worst_ratio(epilogue(inp, tier, epi, accumulate(inp, tier, epi, w_exact), w_exact), res) <= 1.0
    got = epilogue(inp, tier, epi, accumulate(inp, tier, epi, w_exact, fault), w_exact, fault)
    assert worst_ratio(got, res) > 1.0, fault


# ------------------------------------------------------------------------------------------------ attention restatements
def heads_np(qkv, B, S, Hh):
    x = qkv.numpy().reshape(B, S, 3, Hh, 64).transpose(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def online_f32(q, k, v, causal, fault=None):
    """attn_fwd_f32_kernel for one (sequence, head): one query per row, keys in tiles of 32."""
    S = q.shape[0]
    q = q * F(0.124 if fault == "scale" else 0.125)
    qi = np.arange(S)
    m, l, o = np.full(S, -np.inf, F), np.zeros(S, F), np.zeros((S, 64), F)
    for k0 in range(0, S, 32):
        keys = np.arange(k0, min(k0 + 32, S))
        s = np.zeros((S, len(keys)), F)
        for d in range(64):
            s = fma32(q[:, d, None], k[None, keys, d], s)
        if causal:
            s = np.where(keys[None, :] > qi[:, None] + (1 if fault == "mask" else 0), F(-np.inf), s)
        mn = np.maximum(m, s.max(-1))
        with np.errstate(invalid="ignore"):
            corr = np.where(np.isinf(mn), F(1), np.exp(m - mn, dtype=F))
        if fault != "corr_l":
            l = l * corr
        o = o * corr[:, None]
        for j in range(len(keys)):
            with np.errstate(invalid="ignore"):
                p = np.where(np.isinf(s[:, j]), F(0), np.exp(s[:, j] - mn, dtype=F))
            l = l + p
            o = fma32(p[:, None], v[None, keys[j], :], o)
        m = mn
    return o / l[:, None]


def split_mfma(q, k, v, causal, fault=None):
    """attn_fwd_split_kernel for one (sequence, head)."""
    S = q.shape[0]
    qh, ql = np_split(q * F(0.125))
    kh, kl = np_split(k)
    vh, vl = np_split(v)
    acc, cor = np.zeros((S, S), F), np.zeros((S, S), F)
    for kk in range(2):
        dims = range(kk * 32, kk * 32 + 32)
        for d in dims:
            acc += qh[:, d, None] * kh[None, :, d]
        for d in dims:
            cor += qh[:, d, None] * kl[None, :, d]
        for d in dims:
            cor += ql[:, d, None] * kh[None, :, d]
    s = acc + cor
    if causal:
        s = np.where(np.arange(S)[None, :] > np.arange(S)[:, None], F(-np.inf), s)
    m2 = s.max(-1) * LOG2E
    p = np.exp2(fma32(s, np.broadcast_to(LOG2E, s.shape), -m2[:, None]), dtype=F)
    ph, pl = np_split(p)
    if fault == "drop_pl":
        pl = np.zeros_like(pl)
    o, oc, sh, sl = np.zeros((S, 64), F), np.zeros((S, 64), F), np.zeros(S, F), np.zeros(S, F)
    for c0 in range(0, S, 32):
        keys = range(c0, min(c0 + 32, S))
        for j in keys:
            o += ph[:, j, None] * vh[None, j, :]
        for j in keys:
            oc += ph[:, j, None] * vl[None, j, :]
        for j in keys:
            oc += pl[:, j, None] * vh[None, j, :]
        for j in keys:
            sh += ph[:, j]
        for j in keys:
            sl += pl[:, j]
    inv = F(1) / (sh + sl)
    return (o + oc) * inv[:, None]


def run_attention(kind, qkv, B, S, Hh, causal, fault=None):
    """[B*S, Hh*64] float64: the restatement's output; the split layout (split kernel, f32 kernel with split output) read back as hi + lo."""
    q, k, v = heads_np(qkv, B, S, Hh)
    out = np.zeros((B, Hh, S, 64), F)
    for b in range(B):
        for h in range(Hh):
            out[b, h] = (split_mfma if kind == "split" else online_f32)(q[b, h], k[b, h], v[b, h], causal, fault)
    out = out.transpose(0, 2, 1, 3).reshape(B * S, Hh * 64)
    if kind == "f32":
        return out.astype(np.float64)
    hi, lo = np_split(out)
    if fault == "split_ulp":
        lo = ((out + np.spacing(hi.astype(H16)).astype(F)) - hi).astype(H16).astype(F)
    return hi.astype(np.float64) + lo.astype(np.float64)


def attention_bound(kind, res):
    return T.bound_attention_split(res) if kind == "split" else T.bound_attention_f32(res, split_out=(kind == "f32_split"))


# ------------------------------------------------------------------------------------------------ (a), (b) attention
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("family", T.ATT_FAMILIES)
def test_the_attention_restatements_stay_within_the_bound(family, causal):
    worst = {}
    for S in (17, 33, 70):
        B, Hh = 2, 1
        qkv = T.make_attention_inputs(family, B, S, Hh, causal, 5 + S)
        res = T.attention_terms(qkv, B, S, Hh, causal)
        for kind in ("f32", "f32_split", "split"):
            got = run_attention(kind, qkv, B, S, Hh, causal)
            r = float((np.abs(got - res["out"].numpy()) / attention_bound(kind, res).numpy()).max())
            assert r <= 1.0, (kind, S, r)
            worst[kind] = max(worst.get(kind, 0.0), r)
    print("worst |err| / bound, %s causal %d:" % (family, causal), json.dumps({k: round(v, 3) for k, v in worst.items()}))


ATT_FAULTS = [("corr_l", "f32", "peaked_last", 0), ("mask", "f32", "randn", 1), ("scale", "f32", "randn", 0), ("scale", "f32_split", "randn", 0),
              ("drop_pl", "split", "randn", 0), ("split_ulp", "f32_split", "randn", 0), ("split_ulp", "split", "randn", 1)]


@pytest.mark.parametrize("fault,kind,family,causal", ATT_FAULTS)
def test_a_single_attention_fault_leaves_the_bound(fault, kind, family, causal):
    B, S, Hh = 1, 70, 1
    qkv = T.make_attention_inputs(family, B, S, Hh, causal, 5 + S)
    res = T.attention_terms(qkv, B, S, Hh, causal)
    bound, ref = attention_bound(kind, res).numpy(), res["out"].numpy()
    assert float((np.abs(run_attention(kind, qkv, B, S, Hh, causal) - ref) / bound).max()) <= 1.0
    assert float((np.abs(run_attention(kind, qkv, B, S, Hh, causal, fault) - ref) / bound).max()) > 1.0, fault


# ------------------------------------------------------------------------------------------------ the split itself
def test_the_split_of_the_reference_is_what_the_layout_says():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -0.0, 65504.0, -65504.0, 2.0 ** -15, 3 * 2.0 ** -26, 0.1, -1e-3])
    hi, lo = T.split(x)
    assert torch.equal(hi, x.half()) and torch.equal(lo, (x - x.half().float()).half())
    err = (x.double() - hi.double() - lo.double()).abs()
    assert bool((err <= T.rep_error(x)).all())
    lay = T.to_layout(hi.repeat(32)[None, :320].reshape(2, 160), lo.repeat(32)[None, :320].reshape(2, 160))
    h2, l2 = T.from_layout(lay, 2, 160)
    assert torch.equal(h2.reshape(-1), hi.repeat(32)[:320]) and torch.equal(l2.reshape(-1), lo.repeat(32)[:320])
