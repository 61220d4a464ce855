"""CPU: the float64 reference and bound of the f16 GEMM epilogues (tests/gemm_ref.py) and the case table of the GPU test (tests/gemm_cases.py).

(a) every epilogue formula of csrc/gemm.hip, restated in numpy float32 with the K slices summed sequentially, reversed, rotated by every start slice and in
    2, 3, 4 and 8 split-K parts, stays within the bound on every element of every input family;
(b) single faults -- applied to the float64 value, or to the float32 restatement where the fault is a precision step -- leave it;
(c) the case table, run through grip_debug_gemm_plan, names every kernel instantiation the six launch_* helpers of gemm.hip can launch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_cases as GC
import gemm_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
KS = (64, 128, 192, 320, 768, 3072)
M, N = 4, 128


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic in numpy float32
def slice_orders(K):
    """[orders, K] column indices: 32-wide slices sequential, reversed and rotated by every start slice, ascending inside a slice."""
    ns = K // 32
    sl = [list(range(ns)), list(range(ns))[::-1]] + [[(s + r) % ns for s in range(ns)] for r in range(1, ns)]
    return np.array([[32 * s + j for s in o for j in range(32)] for o in sl])


def chain(A, W, start, idx):
    """acc[o] = the k-ordered chain start + a_k w_k over the columns idx[o] (products of f16 numbers are exact in f32: one rounding per add)."""
    acc = np.broadcast_to(start.astype(F), (idx.shape[0], A.shape[0], W.shape[0])).copy()
    for j in range(idx.shape[1]):
        acc += A[:, idx[:, j]].T[:, :, None] * W[:, idx[:, j]].T[:, None, :]
    return acc


_ACC = {}


def accumulate(inp, epi, K, key=None):
    """Every summation order of the accumulator, stacked: (acc [orders, M, N], ksplit of each order).  key: the inputs' name (A, W and bias depend on the
    family and K alone), computed once per bias / no bias."""
    if key is not None:
        key = key + (epi in R.HAS_BIAS,)
        if key not in _ACC:
            _ACC[key] = accumulate(inp, epi, K)
        return _ACC[key]
    A, W = inp["A"].float().numpy(), inp["W"].float().numpy()
    bias = inp["bias"].numpy() if epi in R.HAS_BIAS else np.zeros(W.shape[0], F)
    accs, ksp = [chain(A, W, bias[None, :], slice_orders(K))], [1] * (K // 32 + 1)
    for parts in (2, 3, 4, 8):
        if (K // 64) % parts:
            continue
        w = K // parts
        total = None
        for p in range(parts):
            part = chain(A, W, bias[None, :] if p == 0 else np.zeros((1, W.shape[0]), F), np.arange(p * w, (p + 1) * w)[None])
            total = part if total is None else total + part
        accs.append(total)
        ksp.append(parts)
    return np.concatenate(accs), np.array(ksp)


def sigmoid32(x):
    c = F(F(-1.702) * F(1.4426950408889634))
    with np.errstate(over="ignore"):
        return F(1) / (F(1) + np.exp2(c * x, dtype=F))


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def tile_stats32(v):
    """[.., M, N] -> (sum, sq) [.., M, N / 64]: (v0 + v1) + (v2 + v3), an fma chain for the squares, then four pairwise levels over the 16 lanes."""
    q = v.reshape(v.shape[:-1] + (v.shape[-1] // 64, 16, 4))
    sm = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    sq = fma32(q[..., 0], q[..., 0], fma32(q[..., 1], q[..., 1], fma32(q[..., 2], q[..., 2], q[..., 3] * q[..., 3])))
    for _ in range(4):
        sm, sq = sm[..., 0::2] + sm[..., 1::2], sq[..., 0::2] + sq[..., 1::2]
    return sm[..., 0], sq[..., 0]


def row_stat32(part, K, eps=1e-5):
    """row_stat / ln_stats_finalize: the pairs added in index order, mean = sm fl(1 / K), var = max(sq fl(1 / K) - mean mean, 0), rsqrt(var + eps)."""
    part = part.numpy()
    sm, sq = np.zeros(part.shape[1], F), np.zeros(part.shape[1], F)
    for p in range(part.shape[0]):
        sm, sq = sm + part[p, :, 0], sq + part[p, :, 1]
    inv = F(1) / F(K)
    mean = sm * inv
    var = np.maximum(sq * inv - mean * mean, F(0))
    with np.errstate(divide="ignore"):
        return mean, F(1) / np.sqrt(var + F(eps), dtype=F)


def epilogue32(inp, epi, acc, scalar=1.0, fault=None):
    """{name: float32 or float16 array [orders, ...]} from accumulators acc [orders, M, N]: the statements of epilogue_rows_impl."""
    h = lambda x: x.astype(np.float16)
    out = {}
    K = inp["A"].shape[1]
    if epi == R.EPI_F32:
        out["out"] = acc
    elif epi == R.EPI_F32_SCALE:
        out["out"] = acc * F(scalar)
    elif epi in (R.EPI_F16, R.EPI_BIAS_F16):
        out["out"] = h(acc)
    elif epi == R.EPI_BIAS_GELU_F16:
        out["out2"], out["out"] = h(acc), h(acc * sigmoid32(acc))
    elif epi in R.RESID:
        r = inp["resid"].float().numpy()
        if "resid_lo" in inp:
            r = r + inp["resid_lo"].float().numpy()
        v = (h(acc).astype(F) if fault == "acc_rounded_first" else acc) + r
        hi = h(v)
        out["out"] = hi
        if "resid_lo" in inp:
            out["lo"] = h(v - (v if fault == "lo_of_unrounded_hi" else hi.astype(F)))
        if epi == R.EPI_BIAS_RESID_STATS:
            sm, sq = tile_stats32(hi.astype(F) if fault == "stat_of_rounded" else v)
            out["stat_part"] = np.stack([np.swapaxes(sm, -1, -2), np.swapaxes(sq, -1, -2)], -1)
    elif epi == R.EPI_GELUGRAD_F16:
        x = inp["aux"].float().numpy()
        s = sigmoid32(x)
        out["out"] = h(acc * (s * (F(1) + F(1.702) * x * (F(1) - s))))
    else:
        if "stat_in" in inp:
            mean, rstd = row_stat32(inp["stat_in"], K, 0.0 if fault == "no_eps" else 1e-5)
        else:
            mean, rstd = inp["rowstat"][:, 0].numpy(), inp["rowstat"][:, 1].numpy()
        with np.errstate(invalid="ignore", over="ignore"):
            y = (acc - inp["colsum"].numpy()[None, None, :] * mean[None, :, None]) * rstd[None, :, None] + inp["bias"].numpy()
        if epi == R.EPI_LNFOLD_F16:
            out["out"] = h(y)
        else:
            out["out2"], out["out"] = h(y), h(y * sigmoid32(y))
    return out


def ratios(got, res, inp):
    """worst |got - ref| / bound per output name (hi + lo checked as "hilo")."""
    w = {}
    for name, (ref, bound) in res.items():
        if name == "hilo":
            g = got["out"].astype(np.float64) + got["lo"].astype(np.float64)
        elif name == "lo":
            continue
        else:
            g = got[name].astype(np.float64)
        err = np.abs(g - ref.numpy())
        assert np.isfinite(err).all(), name
        bn = bound.numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            w[name] = float(np.where(bn > 0, err / bn, np.where(err == 0, 0.0, np.inf)).max())      # (a one-hot row on a zero weight: value and bound are 0)
    return w


def inputs(family, K, epi, seed=3, **kw):
    return R.make_inputs(family, M, N, K, seed + K, **kw)


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_the_float32_restatement_stays_within_the_bound(family, K):
    worst = {}
    for epi in range(10):
        variants = [dict()]
        if epi == R.EPI_BIAS_RESID_STATS:
            variants.append(dict(hilo=True))
        if epi in R.FOLD and family in ("randn", "cancel"):
            variants.append(dict(stat_parts=K // 64))
        for kw in variants:
            inp = inputs(family, K, epi, **kw)
            acc, ksp = accumulate(inp, epi, K, (family, K))
            got = epilogue32(inp, epi, acc, scalar=0.375)
            for o in range(acc.shape[0]):
                if ksp[o] > 1 and epi != R.EPI_F32 and epi not in R.RESID:
                    continue        # split-K exists for the f32 store and (cooperative) the residual epilogues
                g1 = {k: v[o] for k, v in got.items()}
                hi = torch.from_numpy(g1["out"]) if "resid_lo" in inp else None
                res = R.reference(inp, epi, ksplit=int(ksp[o]), scalar=0.375, hi_stored=hi)
                if family in ("exact", "onehot") and o == 0:
                    R.assert_exact_family(inp, res, epi)
                w = ratios(g1, res, inp)
                assert max(w.values()) <= 1.0, (epi, kw, o, w)
                if family in ("exact", "onehot"):       # exact in f32, whatever the order: the bits of float64
                    for name in R.exact_names(epi, "resid_lo" in inp):
                        if name in ("hilo", "lo") or name not in res:
                            continue
                        want = res[name][0].numpy()
                        assert np.array_equal(g1[name], want.astype(g1[name].dtype)), (epi, kw, o, name)
                key = "epi%d%s" % (epi, "".join("-" + k for k in kw))
                worst[key] = max(worst.get(key, 0.0), max(w.values()))
    print("worst |err| / bound, %s K=%d:" % (family, K), json.dumps({k: round(v, 3) for k, v in sorted(worst.items())}))


@pytest.mark.parametrize("K", KS)
def test_the_cancel_family_is_decided_by_the_accumulation_term(K):
    inp = R.make_inputs("cancel", 64, N, K, 5)
    A, W = inp["A"].double(), inp["W"].double()
    ref, S = A @ W.T, A.abs() @ W.abs().T
    assert float((S >= 64 * ref.abs()).double().mean()) > 0.9 and float(ref.abs().max()) < 6e4


# ------------------------------------------------------------------------------------------------ (b)
def _leaves(inp, epi, fault, names=None, **kw):
    """The faulted float64 value is further than TWICE the bound from the value on some element: a kernel with that fault, its own roundings included, fails."""
    res, bad = R.reference(inp, epi, **kw), R.reference(inp, epi, fault=fault, **kw)
    worst = max(float(((bad[n][0] - res[n][0]).abs() / res[n][1]).max()) for n in (names or res))
    assert worst > 2.0, (fault, epi, worst)
    return worst


VALUE_FAULTS = [     # (fault, epilogue, family, K, keywords of make_inputs / reference, output names)
    ("drop_slice", R.EPI_F32, "randn", 768, {}, {}, None),
    ("drop_slice", R.EPI_F32, "cancel", 768, {}, {}, None),
    ("drop_slice", R.EPI_BIAS_F16, "randn", 3072, {}, dict(slice0=3040), None),
    ("double_slice", R.EPI_F32, "randn", 768, {}, dict(slice0=32), None),
    ("bias_neighbour", R.EPI_BIAS_F16, "randn", 192, {}, {}, None),
    ("resid_next_row", R.EPI_BIAS_RESID, "randn", 192, {}, {}, None),
    ("gelu_1p7", R.EPI_BIAS_GELU_F16, "randn", 192, {}, {}, ("out",)),
    ("gelu_1p7", R.EPI_LNFOLD_GELU_F16, "randn", 192, {}, {}, ("out",)),
    ("aux_next_row", R.EPI_GELUGRAD_F16, "randn", 192, {}, {}, None),
    ("drop_colsum_mean", R.EPI_LNFOLD_F16, "randn", 192, {}, {}, None),
    ("rstd_next_row", R.EPI_LNFOLD_F16, "randn", 192, {}, {}, None),
    ("drop_partial_17", R.EPI_LNFOLD_F16, "randn", 1280, dict(stat_parts=20), {}, None),
    ("stat_neighbour_tile", R.EPI_BIAS_RESID_STATS, "randn", 192, {}, {}, ("stat_part",)),
    ("scale_twice", R.EPI_F32_SCALE, "randn", 192, {}, dict(scalar=0.375), None),
]


@pytest.mark.parametrize("fault,epi,family,K,mk,rk,names", VALUE_FAULTS, ids=["%s-e%d-%s-K%d" % f[:4] for f in VALUE_FAULTS])
def test_a_single_fault_in_the_value_leaves_the_bound(fault, epi, family, K, mk, rk, names):
    inp = inputs(family, K, epi, **mk)
    if fault == "drop_partial_17":       # rows with a mean: a dropped partial moves it (the randn rows' own mean is O(K^-1/2))
        inp["A"] = (inp["A"].float() + 1.0).half()
        t = inp["A"].double().reshape(M, 20, 64)
        inp["stat_in"] = torch.stack([t.sum(-1).T, (t * t).sum(-1).T], -1).float().contiguous()
    _leaves(inp, epi, fault, names, **rk)


PRECISION_FAULTS = [("acc_rounded_first", R.EPI_BIAS_RESID, "randn", 192, {}, "out"), ("stat_of_rounded", R.EPI_BIAS_RESID_STATS, "randn", 64, {}, "stat_part"),
                    ("lo_of_unrounded_hi", R.EPI_BIAS_RESID_STATS, "randn", 192, dict(hilo=True), "hilo"), ("no_eps", R.EPI_LNFOLD_F16, "flat", 128, dict(stat_parts=2), "out")]


@pytest.mark.parametrize("fault,epi,family,K,mk,name", PRECISION_FAULTS, ids=[f[0] for f in PRECISION_FAULTS])
def test_a_single_precision_fault_in_the_restatement_leaves_the_bound(fault, epi, family, K, mk, name):
    inp = inputs("randn" if family == "flat" else family, K, epi, **mk)
    if family == "flat":                  # constant rows: the variance is zero and eps is all rsqrt sees
        inp["A"] = torch.ones(M, K).half() * torch.tensor([1.0, -2.0, 0.5, 3.0]).half()[:, None]
        t = inp["A"].double().reshape(M, 2, 64)
        inp["stat_in"] = torch.stack([t.sum(-1).T, (t * t).sum(-1).T], -1).float().contiguous()
    acc, _ = accumulate(inp, epi, K)
    for f, must_hold in ((None, True), (fault, False)):
        got = {k: v[0] for k, v in epilogue32(inp, epi, acc[:1], fault=f).items()}
        res = R.reference(inp, epi, hi_stored=torch.from_numpy(got["out"]) if "resid_lo" in inp else None)
        with np.errstate(invalid="ignore"):
            g = got["out"].astype(np.float64) + got["lo"].astype(np.float64) if name == "hilo" else got[name].astype(np.float64)
            err = np.abs(g - res[name][0].numpy()) / res[name][1].numpy()
        worst = float(np.nanmax(np.where(np.isfinite(err), err, np.inf)))
        assert (worst <= 1.0) if must_hold else (worst > 1.0), (fault, f, worst)


# ------------------------------------------------------------------------------------------------ (c)
# Every kernel instantiation launch_two_stage, launch_ring, launch_ringw, launch_big, launch_k64 and launch_k64p (csrc/gemm.hip) can launch, one per line:
# a branch added to or taken from one of the six helpers is one line here.
INSTANTIATIONS = [
    # launch_two_stage: 64- and 128-row tiles, every epilogue
    "gemm_f16_kernel<0, 2>",
    "gemm_f16_kernel<1, 2>",
    "gemm_f16_kernel<2, 2>",
    "gemm_f16_kernel<3, 2>",
    "gemm_f16_kernel<4, 2>",
    "gemm_f16_kernel<5, 2>",
    "gemm_f16_kernel<6, 2>",
    "gemm_f16_kernel<7, 2>",
    "gemm_f16_kernel<8, 2>",
    "gemm_f16_kernel<9, 2>",
    "gemm_f16_kernel<0, 4>",
    "gemm_f16_kernel<1, 4>",
    "gemm_f16_kernel<2, 4>",
    "gemm_f16_kernel<3, 4>",
    "gemm_f16_kernel<4, 4>",
    "gemm_f16_kernel<5, 4>",
    "gemm_f16_kernel<6, 4>",
    "gemm_f16_kernel<7, 4>",
    "gemm_f16_kernel<8, 4>",
    "gemm_f16_kernel<9, 4>",
    # launch_ring: 3- and 4-slot ring
    "gemm_ring_kernel<0, 3>",
    "gemm_ring_kernel<1, 3>",
    "gemm_ring_kernel<2, 3>",
    "gemm_ring_kernel<3, 3>",
    "gemm_ring_kernel<4, 3>",
    "gemm_ring_kernel<5, 3>",
    "gemm_ring_kernel<6, 3>",
    "gemm_ring_kernel<7, 3>",
    "gemm_ring_kernel<8, 3>",
    "gemm_ring_kernel<9, 3>",
    "gemm_ring_kernel<0, 4>",
    "gemm_ring_kernel<1, 4>",
    "gemm_ring_kernel<2, 4>",
    "gemm_ring_kernel<3, 4>",
    "gemm_ring_kernel<4, 4>",
    "gemm_ring_kernel<5, 4>",
    "gemm_ring_kernel<6, 4>",
    "gemm_ring_kernel<7, 4>",
    "gemm_ring_kernel<8, 4>",
    "gemm_ring_kernel<9, 4>",
    # launch_ringw: 32 rows
    "gemm_ringw_kernel<0, 4, 1>",
    "gemm_ringw_kernel<1, 4, 1>",
    "gemm_ringw_kernel<2, 4, 1>",
    "gemm_ringw_kernel<3, 4, 1>",
    "gemm_ringw_kernel<4, 4, 1>",
    "gemm_ringw_kernel<5, 4, 1>",
    "gemm_ringw_kernel<6, 4, 1>",
    "gemm_ringw_kernel<7, 4, 1>",
    "gemm_ringw_kernel<8, 4, 1>",
    "gemm_ringw_kernel<9, 4, 1>",
    # 64 rows
    "gemm_ringw_kernel<0, 4, 2>",
    "gemm_ringw_kernel<1, 4, 2>",
    "gemm_ringw_kernel<2, 4, 2>",
    "gemm_ringw_kernel<3, 4, 2>",
    "gemm_ringw_kernel<4, 4, 2>",
    "gemm_ringw_kernel<5, 4, 2>",
    "gemm_ringw_kernel<6, 4, 2>",
    "gemm_ringw_kernel<7, 4, 2>",
    "gemm_ringw_kernel<8, 4, 2>",
    "gemm_ringw_kernel<9, 4, 2>",
    # 96 rows: three epilogues
    "gemm_ringw_kernel<3, 5, 3>",
    "gemm_ringw_kernel<9, 5, 3>",
    "gemm_ringw_kernel<4, 5, 3>",
    # 128 rows, 5-slot ring
    "gemm_ringw_kernel<0, 5, 4>",
    "gemm_ringw_kernel<1, 5, 4>",
    "gemm_ringw_kernel<2, 5, 4>",
    "gemm_ringw_kernel<3, 5, 4>",
    "gemm_ringw_kernel<4, 5, 4>",
    "gemm_ringw_kernel<5, 5, 4>",
    "gemm_ringw_kernel<6, 5, 4>",
    "gemm_ringw_kernel<7, 5, 4>",
    "gemm_ringw_kernel<8, 5, 4>",
    "gemm_ringw_kernel<9, 5, 4>",
    # 128 rows, 3-slot ring
    "gemm_ringw_kernel<0, 3, 4>",
    "gemm_ringw_kernel<1, 3, 4>",
    "gemm_ringw_kernel<2, 3, 4>",
    "gemm_ringw_kernel<3, 3, 4>",
    "gemm_ringw_kernel<4, 3, 4>",
    "gemm_ringw_kernel<5, 3, 4>",
    "gemm_ringw_kernel<6, 3, 4>",
    "gemm_ringw_kernel<7, 3, 4>",
    "gemm_ringw_kernel<8, 3, 4>",
    "gemm_ringw_kernel<9, 3, 4>",
    # launch_big: 256x256 on four slots, 256x128 on three
    "gemm_big_kernel<0, 256, 256, 4>",
    "gemm_big_kernel<1, 256, 256, 4>",
    "gemm_big_kernel<2, 256, 256, 4>",
    "gemm_big_kernel<3, 256, 256, 4>",
    "gemm_big_kernel<4, 256, 256, 4>",
    "gemm_big_kernel<5, 256, 256, 4>",
    "gemm_big_kernel<6, 256, 256, 4>",
    "gemm_big_kernel<7, 256, 256, 4>",
    "gemm_big_kernel<8, 256, 256, 4>",
    "gemm_big_kernel<9, 256, 256, 4>",
    "gemm_big_kernel<0, 256, 128, 3>",
    "gemm_big_kernel<1, 256, 128, 3>",
    "gemm_big_kernel<2, 256, 128, 3>",
    "gemm_big_kernel<3, 256, 128, 3>",
    "gemm_big_kernel<4, 256, 128, 3>",
    "gemm_big_kernel<5, 256, 128, 3>",
    "gemm_big_kernel<6, 256, 128, 3>",
    "gemm_big_kernel<7, 256, 128, 3>",
    "gemm_big_kernel<8, 256, 128, 3>",
    "gemm_big_kernel<9, 256, 128, 3>",
    # launch_k64: 192- and 256-row tiles, no statistics-carrying form
    "gemm_k64_kernel<0, 8, 6>",
    "gemm_k64_kernel<1, 8, 6>",
    "gemm_k64_kernel<2, 8, 6>",
    "gemm_k64_kernel<3, 8, 6>",
    "gemm_k64_kernel<4, 8, 6>",
    "gemm_k64_kernel<5, 8, 6>",
    "gemm_k64_kernel<6, 8, 6>",
    "gemm_k64_kernel<7, 8, 6>",
    "gemm_k64_kernel<8, 8, 6>",
    "gemm_k64_kernel<0, 8, 8>",
    "gemm_k64_kernel<1, 8, 8>",
    "gemm_k64_kernel<2, 8, 8>",
    "gemm_k64_kernel<3, 8, 8>",
    "gemm_k64_kernel<4, 8, 8>",
    "gemm_k64_kernel<5, 8, 8>",
    "gemm_k64_kernel<6, 8, 8>",
    "gemm_k64_kernel<7, 8, 8>",
    "gemm_k64_kernel<8, 8, 8>",
    # launch_k64p: form 0 of every epilogue
    "gemm_k64p_kernel<0, 0, false>",
    "gemm_k64p_kernel<1, 0, false>",
    "gemm_k64p_kernel<2, 0, false>",
    "gemm_k64p_kernel<3, 0, false>",
    "gemm_k64p_kernel<4, 0, false>",
    "gemm_k64p_kernel<5, 0, false>",
    "gemm_k64p_kernel<6, 0, false>",
    "gemm_k64p_kernel<7, 0, false>",
    "gemm_k64p_kernel<8, 0, false>",
    "gemm_k64p_kernel<9, 0, false>",
    # the other forms of the three pool-encode epilogues
    "gemm_k64p_kernel<7, 4, true>",
    "gemm_k64p_kernel<7, 4, false>",
    "gemm_k64p_kernel<7, 2, false>",
    "gemm_k64p_kernel<7, 1, false>",
    "gemm_k64p_kernel<8, 2, true>",
    "gemm_k64p_kernel<8, 4, false>",
    "gemm_k64p_kernel<8, 2, false>",
    "gemm_k64p_kernel<8, 1, false>",
    "gemm_k64p_kernel<9, 1, true>",
    "gemm_k64p_kernel<9, 1, false>",
]


def planned_kernels(knob):
    """The table's cases of one knob set through the plan hook of THIS process: every case must get the kernel it names.  -> the set of kernels."""
    import grip_amd  # noqa: F401
    from grip_amd import native
    lib = native.lib()
    got = set()
    for c in GC.all_cases():
        if c["knob"] != knob:
            continue
        rc, text = GC.plan(lib, c)
        assert GC.plan_is_intended(c, rc, text), (c["id"], c["knob"], c["kernel"], c["expect"], text)
        got.add(c["kernel"])
    return got


_CHILD = """
import json, sys
sys.path.insert(0, {repo!r})
sys.path.insert(0, {tests!r})
import test_host_gemm_ref as T
print("KERNELS " + json.dumps(sorted(T.planned_kernels({knob!r}))))
"""


def test_the_case_table_reaches_every_instantiation():
    for k in os.environ:
        assert not k.startswith(("GRIP_GEMM_", "GRIP_COOP_SPLIT", "GRIP_KROT_M")), f"{k} is set: the default part of the table needs the default knobs"
    reached = set(planned_kernels(""))
    for knob in GC.KNOBS:
        name, value = knob.split("=")
        env = dict(os.environ)
        env[name] = value
        p = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), knob=knob)], env=env, capture_output=True, text=True, timeout=300)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("KERNELS ")]
        assert p.returncode == 0 and line, p.stdout[-2000:] + p.stderr[-4000:]
        reached |= set(json.loads(line[0][8:]))
    want = INSTANTIATIONS
    assert len(want) == len(set(want)) == 141
    assert not set(want) - reached, sorted(set(want) - reached)
    assert not reached - set(want), sorted(reached - set(want))


def test_the_case_table_holds_what_it_is_there_for():
    cases = GC.all_cases()
    assert sorted({c["expect"]["tiles"] for c in cases if c["group"] == "persistent8"}) == [1, 3, 8, 9, 30]
    assert all(c["expect"] == dict(colgroup=2, tiles=130) for c in cases if c["knob"] == "GRIP_GEMM_COLGROUP=2")
    assert all("finalize" in c["expect"] for c in cases if c["group"] == "stat_in")


def test_the_case_table_keeps_to_small_shapes():
    for c in GC.all_cases():
        assert c["M"] <= 4300 or (c["M"], c["N"], c["K"]) == (16385, 512, 128), c["id"]
