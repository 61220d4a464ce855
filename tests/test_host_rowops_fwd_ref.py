"""CPU: the derived bounds of tests/rowops_fwd_ref.py hold for f32 arithmetic in three reduction orders and are not vacuous (what makes
tests/test_gpu_rowops_fwd.py meaningful).  No GPU, no library call.

(a) The formulas of csrc/rowops.hip evaluated in numpy float32: every element of every family and width is within the bound.  A row sum is formed as a
    wave forms it -- each of the 64 lanes adds its own vectors in index order -- and the 64 lane sums are then taken sequentially, pairwise and in reverse (63
    dependent adds where wave_sum has six levels); a 64-column tile of vit_deep_insert's statistics is 16 lanes x 4 elements, summed over its lanes in the same
    three orders; the partial pairs of ln_stats_finalize are summed over the parts in the three orders.  (One sequential chain over a whole row, d - 1 adds deep, is
    not what the bound describes: on `flat` rows that are not f16 numbers it leaves the (4 NV + 6) u bound, 1.08 x at d = 256.)  The worst |err| / bound per kernel is printed and written to tests/_out/rowops_fwd_ref_host.json.
(b) Fifteen single faults applied to the float64 value: each leaves the bound on at least one element at every width, on the family named."""
import numpy as np
import pytest
import torch

import rowops_fwd_ref as FR
from conftest import write_report
from test_host_rowops_ref import F, ORDERS, _rsum

_REPORT = {}
EPS = F(1e-5)


def _ratio(got, ref, bound):
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref.numpy()) / bound.numpy()).max())


def _wsum(v, order, group=4):
    """A row sum as a wave forms it: lane l owns the `group`-element vectors l, l + 64, ... and adds them in index order (the kernel's in-lane adds); the 64
    lane sums are then added sequentially, pairwise or in reverse -- 63 dependent adds where wave_sum has six levels."""
    v = v.astype(F)
    n = v.shape[-1] // group
    pad = (-n) % 64
    v = v.reshape(v.shape[:-1] + (n, group))
    if pad:
        v = np.concatenate([v, np.zeros(v.shape[:-2] + (pad, group), F)], axis=-2)
    v = v.reshape(v.shape[:-2] + ((n + pad) // 64, 64, group))
    lanes = np.zeros(v.shape[:-3] + (64,), F)
    for i in range(v.shape[-3]):
        for e in range(group):
            lanes = lanes + v[..., i, :, e]
    return _rsum(lanes, order)


def _ln_stats_f32(x, order):
    d = F(x.shape[-1])
    mean = _wsum(x, order) / d
    c = x - mean
    return mean, c, F(1) / np.sqrt(_wsum(c * c, order) / d + EPS)


def _ln_f32(x, gamma, beta, order):
    mean, c, rstd = _ln_stats_f32(x, order)
    y = ((c * rstd) * gamma) + beta
    assert y.dtype == F
    return y


def _onepass_f32(S1, S2, d, inv_mul):
    if inv_mul:
        inv = F(1) / F(d)
        mean, m2 = S1 * inv, S2 * inv
    else:
        mean, m2 = S1 / F(d), S2 / F(d)
    var = np.maximum(m2 - mean * mean, F(0))
    return mean, F(1) / np.sqrt(var + EPS)


def _split_f32(y):
    hi = y.astype(np.float16)
    lo = ((y - hi.astype(F)) * F(FR.SPLIT_LO_SCALE)).astype(np.float16)
    return hi.astype(np.float64) + lo.astype(np.float64) / FR.SPLIT_LO_SCALE


def _assemble_inputs(family, d, seed, B=3, P=2, G2=3):
    rows, gamma, beta = FR.make_rows(family, B * G2 + 1 + B * P + 1 + G2, d, seed)
    patch, cls, prefix, pos = rows[:B * G2], rows[B * G2], rows[B * G2 + 1:B * G2 + 1 + B * P], rows[B * G2 + 1 + B * P:]
    return patch, cls, 0.5 * pos, prefix, gamma, beta, B, P, G2


def _embed_inputs(family, d, seed, C=3, T=6, P=2, vocab=9):
    rows, _, _ = FR.make_rows(family, vocab + C * P + T, d, seed)
    tok, prefix, pos = rows[:vocab], rows[vocab:vocab + C * P], 0.01 * rows[vocab + C * P:]
    ids = torch.randint(0, vocab - 1, (C, T), generator=torch.Generator().manual_seed(seed)).int()
    return ids, tok, pos, prefix, P, C, T


@pytest.mark.parametrize("family", FR.FAMILIES)
@pytest.mark.parametrize("d", FR.WIDTHS)
def test_bound_holds_for_f32_in_three_reduction_orders(d, family):
    seed = d + len(family)
    worst = {}
    x16, _, gamma = FR.make_inputs(family, 12, d, 1, seed)
    rows, _, beta = FR.make_rows(family, 12, d, seed)
    g32, b32 = gamma.numpy().astype(F), beta.numpy().astype(F)
    patch, cls, pos, prefix, _, _, B, P, G2 = _assemble_inputs(family, d, seed)
    S = 1 + P + G2
    ids, tok, tpos, tpre, TP, C, T = _embed_inputs(family, d, seed)
    for order in ORDERS:
        # LayerNorm: the f16 stream in (f16 out) and f32 in (f32 and split-layout out)
        ref, bound = FR.ln_fwd(x16.double(), gamma, beta)
        y = _ln_f32(x16.float().numpy(), g32, b32, order)
        worst[order + ".ln.f16"] = _ratio(y.astype(np.float16), ref, bound + FR.half_bound(ref, bound))
        ref, bound = FR.ln_fwd(rows.double(), gamma, beta)
        y = _ln_f32(rows.numpy(), g32, b32, order)
        worst[order + ".ln.f32"] = _ratio(y, ref, bound)
        if d % 32 == 0:
            worst[order + ".ln.split"] = _ratio(_split_f32(y), ref, bound + FR.split_bound(ref, bound))
        # vit_assemble_ln, per-image prompts: stream, rowstat of the f32 output, x_lo given the stored hi
        y64, e_y, (mean, e_mean, rstd, e_rstd) = FR.vit_assemble(patch, cls, pos, prefix, gamma, beta, B, P, G2, 1)
        v = np.zeros((B, S, d), F)
        v[:, 0] = cls.numpy() + pos[0].numpy()
        v[:, 1:1 + P] = prefix.numpy().reshape(B, P, d)
        v[:, 1 + P:] = patch.numpy().reshape(B, G2, d) + pos[1:1 + G2].numpy()
        y = _ln_f32(v.reshape(B * S, d), g32, b32, order)
        worst[order + ".assemble.x"] = _ratio(y, y64, e_y)
        m2, _, r2 = _ln_stats_f32(y, order)
        worst[order + ".assemble.rowstat"] = max(_ratio(m2, mean, e_mean), _ratio(r2, rstd, e_rstd))
        hi = y.astype(np.float16)
        lref, lbound = FR.x_lo(y64, e_y, torch.from_numpy(hi))
        worst[order + ".assemble.x_lo"] = _ratio((y - hi.astype(F)).astype(np.float16), lref, lbound)
        # text_embed: the row and its one-pass statistics
        v64, e_v, (mean, e_mean, rstd, e_rstd) = FR.text_embed(ids, tok, tpos, tpre, TP, C, C, T, 0)
        cs, ts = FR.seq_rows(C, T, 0, "cpu")
        src = tok.numpy()[ids.long()[cs, ts].numpy()]
        isp = ((ts >= 1) & (ts <= TP)).numpy()
        src[isp] = tpre.numpy().reshape(C, TP, d)[cs.numpy()[isp], ts.numpy()[isp] - 1]
        v = src + tpos.numpy()[ts.numpy()]
        worst[order + ".embed.x"] = _ratio(v, v64, e_v + 1e-300)
        m1, r1 = _onepass_f32(_wsum(v, order), _wsum(v * v, order), d, False)
        worst[order + ".embed.rowstat"] = max(_ratio(m1, mean, e_mean), _ratio(r1, rstd, e_rstd))
        # vit_deep_insert: statistics of the values as stored, plain and compensated; ln_stats_finalize on the tile pairs
        if d % 64 == 0:
            for comp in (False, True):
                hi, lo, (ts_, e_ts, tq_, e_tq), (mean, e_mean, rstd, e_rstd) = FR.deep_insert(rows, comp)
                st = hi.float().numpy() + lo.float().numpy() if comp else hi.float().numpy()
                assert st.dtype == F
                t = st.reshape(12, d // 64, 16, 4)                                   # a tile: 16 lanes x 4 elements; the lane's share as the kernel forms it,
                lane_s = (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])           # then the 16 lanes in the three orders (the kernel: four DPP levels)
                lane_q = t[..., 0] * t[..., 0] + (t[..., 1] * t[..., 1] + (t[..., 2] * t[..., 2] + t[..., 3] * t[..., 3]))
                ts32, tq32 = _rsum(lane_s, order)[..., 0], _rsum(lane_q, order)[..., 0]
                key = order + (".deep.comp" if comp else ".deep.plain")
                worst[key + ".stat_part"] = max(_ratio(ts32, ts_, e_ts), _ratio(tq32, tq_, e_tq))
                m1, r1 = _onepass_f32(_rsum(ts32, "sequential"), _rsum(tq32, "sequential"), d, True)
                worst[key + ".rowstat"] = max(_ratio(m1, mean, e_mean), _ratio(r1, rstd, e_rstd))
            part = torch.from_numpy(np.stack([ts32.T, tq32.T], -1))                      # [tiles, M, 2]
            mean, e_mean, rstd, e_rstd = FR.stats_finalize(part, d)
            m1, r1 = _onepass_f32(_rsum(ts32, order), _rsum(tq32, order), d, True)
            worst[order + ".finalize"] = max(_ratio(m1, mean, e_mean), _ratio(r1, rstd, e_rstd))
        # ln_fold_weights on W = the f16 rows [12, d]
        bias = torch.linspace(-1, 1, 12)
        Wg, (cs_, e_cs), (bo, e_bo) = FR.fold_weights(x16, gamma, beta, bias)
        w32 = x16.float().numpy()
        wg32 = (g32 * w32).astype(np.float16)
        assert np.array_equal(wg32.view(np.int16), Wg.numpy().view(np.int16))
        worst[order + ".fold.colsum"] = _ratio(_wsum(wg32.astype(F), order, 1)[:, 0], cs_, e_cs)
        worst[order + ".fold.bias"] = _ratio(bias.numpy() + _wsum(b32 * w32, order, 1)[:, 0], bo, e_bo)
    per_kernel = {}
    for k, v in worst.items():
        name = k.split(".", 1)[1]
        per_kernel[name] = max(per_kernel.get(name, 0.0), round(v, 4))
    _REPORT[f"{family}.d{d}"] = per_kernel
    write_report("rowops_fwd_ref_host.json", _REPORT)
    print(f"{family} d={d}: worst |err| / bound = {max(worst.values()):.3f} ({max(worst, key=worst.get)})")
    assert max(worst.values()) <= 1.0, worst


def test_one_pass_rstd_bound_per_family():
    """E(rstd) / rstd of text_embed's one-pass statistics at d = 768: a property of the kernel (the cancellation in sum v^2 / d - mean^2), recorded, not shrunk."""
    out = {}
    for family in FR.FAMILIES:
        ids, tok, pos, pre, P, C, T = _embed_inputs(family, 768, 5)
        _, _, (_, _, rstd, e_rstd) = FR.text_embed(ids, tok, pos, pre, P, C, C, T, 0)
        out[family] = float((e_rstd / rstd).max())
    _REPORT["embed E(rstd) / rstd at d = 768"] = out
    write_report("rowops_fwd_ref_host.json", _REPORT)
    print(out)
    assert out["flat"] > 10 * out["randn"] and all(np.isfinite(v) for v in out.values()), out


def _exceeds(value, ref, bound):
    return bool(((value - ref).abs() > bound).any())


def _fault_case(fault, family, d):
    seed = 7 * d + len(family)
    rows, gamma, beta = FR.make_rows(family, 10, d, seed)
    if fault in ("no_eps", "d_plus_4", "gamma_tail_one", "drop_beta"):
        ref, bound = FR.ln_fwd(rows.double(), gamma, beta)
        return _exceeds(FR.ln_fwd(rows.double(), gamma, beta, None, fault)[0], ref, bound)
    if fault == "read_row_off_by_one":
        index = torch.tensor([2, 4], dtype=torch.int32)
        ref, bound = FR.ln_gather(rows, index, 5, 2, gamma, beta)
        return _exceeds(FR.ln_gather(rows, index, 5, 2, gamma, beta, fault)[0], ref, bound)
    if fault in ("pos_on_prompt", "pos_j_for_1_plus_j", "prompt_of_image_0", "x_lo_of_unrounded_hi"):
        patch, cls, pos, prefix, gamma, beta, B, P, G2 = _assemble_inputs(family, d, seed)
        y, e_y, _ = FR.vit_assemble(patch, cls, pos, prefix, gamma, beta, B, P, G2, 1)
        if fault == "x_lo_of_unrounded_hi":
            hi = y.float().half()
            ref, bound = FR.x_lo(y, e_y, hi)
            return _exceeds(FR.x_lo(y, e_y, hi, fault)[0], ref, bound)
        return _exceeds(FR.vit_assemble(patch, cls, pos, prefix, gamma, beta, B, P, G2, 1, fault)[0], y, e_y)
    if fault in ("class_0_context", "token_off_by_one", "embed_stats_of_stored"):
        ids, tok, pos, pre, P, C, T = _embed_inputs(family, d, seed)
        v, e_v, (mean, e_mean, rstd, e_rstd) = FR.text_embed(ids, tok, pos, pre, P, C, C, T, 0)
        fv, _, (fmean, _, frstd, _) = FR.text_embed(ids, tok, pos, pre, P, C, C, T, 0, fault)
        if fault == "embed_stats_of_stored":
            return _exceeds(fmean, mean, e_mean) or _exceeds(frstd, rstd, e_rstd)
        return _exceeds(fv, v, e_v)
    if fault in ("deep_stats_of_unrounded", "drop_tile"):
        if d % 64:
            return True                                  # the statistics exist for d % 64 == 0 only (the launcher refuses the rest)
        _, _, (ts, e_ts, tq, e_tq), (mean, e_mean, rstd, e_rstd) = FR.deep_insert(rows, False)
        _, _, (fts, _, ftq, _), (fmean, _, frstd, _) = FR.deep_insert(rows, False, fault)
        hit = _exceeds(fmean, mean, e_mean) or _exceeds(frstd, rstd, e_rstd)
        if fault == "drop_tile":                         # ln_stats_finalize takes the same decision
            part = torch.stack([ts.T, tq.T], -1).float()
            mean, e_mean, rstd, e_rstd = FR.stats_finalize(part, d)
            fmean, _, frstd, _ = FR.stats_finalize(part, d, fault)
            hit = hit and (_exceeds(fmean, mean, e_mean) or _exceeds(frstd, rstd, e_rstd))
        else:
            hit = hit and (_exceeds(fts, ts, e_ts) or _exceeds(ftq, tq, e_tq))
        return hit
    assert fault == "colsum_unrounded"
    W = rows.half()
    _, (cs, e_cs), _ = FR.fold_weights(W, gamma, beta, torch.zeros(10))
    return _exceeds(FR.fold_weights(W, gamma, beta, torch.zeros(10), fault)[1][0], cs, e_cs)


NAMED_FAMILY = {"no_eps": "flat"}


@pytest.mark.parametrize("fault", FR.FAULTS)
def test_each_single_fault_exceeds_the_bound(fault):
    """Asserted at every width on the family the fault is named for (randn where none is named); the other families are recorded."""
    caught = {fam: [d for d in FR.WIDTHS if _fault_case(fault, fam, d)] for fam in FR.FAMILIES}
    _REPORT.setdefault("faults", {})[fault] = {fam: ("all widths" if len(ds) == len(FR.WIDTHS) else ds) for fam, ds in caught.items()}
    write_report("rowops_fwd_ref_host.json", _REPORT)
    print(f"{fault}: caught at widths {caught}")
    assert caught[NAMED_FAMILY.get(fault, "randn")] == list(FR.WIDTHS), caught
