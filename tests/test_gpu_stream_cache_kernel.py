"""grip_stream_cache_plan / grip_stream_cache_head (csrc/stream_cache.hip) through engine.stream_cache_plan / stream_cache_head, over the case list and the
pools of tests/stream_cache_ref.py.  H: every element against float64 under the derived bound.  pred: EQUAL to the float64 first arg-max on every row
without a NaN (no arithmetic decides it).  negbits: equal to the float64 bits wherever the probability is further than twice its bound from both window
ends.  leave, the key lists and the counts: EQUAL to the reference scan played on the device's OWN entropy_out / pred_out.  Logits: every element against
float64 evaluated on the device's membership, under the bound derived from the chain lengths.  Two calls bit-equal; causality at k in {1, n / 2, n - 1};
a column without a live key is base, bit for bit; neg_cap = 0 equals the positive-only evaluation.  The worst |err| / bound per output goes to
tests/_out/stream_cache_kernel.json."""
import numpy as np
import pytest
import torch

import stream_cache_ref as R
from conftest import write_report

pytestmark = pytest.mark.gpu
_REPORT = {}
_HEAD = ("pos_alpha", "pos_beta", "neg_alpha", "neg_beta")
_PLAN = ("pos_cap", "neg_cap", "neg_entropy", "neg_mask")


def _run(base, feats, st):
    """dict of numpy arrays: the plan's fields, counts, and out."""
    from grip_amd import engine
    x, f = torch.from_numpy(base).cuda(), torch.from_numpy(feats).cuda()
    plan = engine.stream_cache_plan(x, **{k: st[k] for k in _PLAN})
    out = engine.stream_cache_head(x, f, plan, negative=st["neg_cap"] > 0, **{k: st[k] for k in _HEAD})
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in plan.items()}
    got["out"] = out.cpu().numpy()
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def _same(a, b, n=None):
    """Bit equality of two runs (the key lists up to their counts; rows < n when n is given)."""
    for k in ("entropy", "pred", "negbits", "out") + (() if n is not None else ("pos_leave", "neg_leave", "counts")):
        if not np.array_equal(_bits(a[k][:n]), _bits(b[k][:n])):
            return False
    if n is None:
        return all(np.array_equal(a[k][:a["counts"][p]], b[k][:b["counts"][p]]) for p, k in enumerate(("pos_key", "neg_key")))
    return True


def _worst(name, ratio):
    _REPORT[name] = max(_REPORT.get(name, 0.0), float(ratio))


def _check(base, feats, st, got):
    n, c = base.shape
    r = R.rows64(base, st["neg_mask"])
    ok = np.isfinite(base).all(1)
    # H: every element
    assert np.array_equal(np.isfinite(got["entropy"]), ok), "H is finite exactly where the row is"
    err = np.abs(got["entropy"][ok].astype(np.float64) - r["H"][ok])
    bound = r["bH"][ok]
    assert (err <= bound).all(), (err.max(), bound[err.argmax()])
    if (bound > 0).any():
        _worst("H", (err[bound > 0] / bound[bound > 0]).max())
    # pred and the mask bits
    assert np.array_equal(got["pred"][ok], r["pred"][ok]) and ((got["pred"] >= 0) & (got["pred"] < c)).all()
    bits = R.unpack_bits(got["negbits"], c)
    assert np.array_equal(bits[r["decided"]], r["bits"][r["decided"]])
    assert np.array_equal(R.pack_bits(bits), got["negbits"]), "a bit at or beyond c is set"
    # the queue history: the sequential scan on the device's own numbers
    want = R.plan_from(got["entropy"], got["pred"], c, st["pos_cap"], st["neg_cap"], st["neg_entropy"], f32=True)
    for p, name in enumerate(("pos", "neg")):
        assert np.array_equal(got[name + "_leave"].astype(np.int64), want[name + "_leave"]), name
        assert got["counts"][p] == len(want[name + "_key"]) and np.array_equal(got[name + "_key"][:got["counts"][p]], want[name + "_key"]), name
    # the logits: float64 on the device's membership
    ref, b = R.evaluate64(base, feats, got["pred"], bits, got["pos_leave"], got["neg_leave"], *(st[k] for k in _HEAD))
    assert np.array_equal(np.isnan(got["out"]), np.isnan(ref))
    fin = ~np.isnan(ref)
    err = np.abs(got["out"].astype(np.float64) - ref)[fin]
    assert (err <= b[fin]).all(), (err.max(), b[fin][err.argmax()])
    if err.size:      # (a stream that is one row of NaNs has no finite element)
        _worst("logits", (err / b[fin]).max())
    # a column without a live key is base, bit for bit
    onehot = np.zeros((n, c), dtype=bool)
    onehot[np.arange(n), got["pred"]] = True
    touched = (R.live(got["pos_leave"]).astype(np.int64) @ onehot.astype(np.int64) + R.live(got["neg_leave"]).astype(np.int64) @ bits.astype(np.int64)) > 0
    assert np.array_equal(_bits(got["out"])[~touched], _bits(base)[~touched])
    return touched


@pytest.mark.parametrize("kind,n,c,e,caps", R.CASES)
def test_every_output_against_float64_and_the_sequential_scan(kind, n, c, e, caps):
    base, feats = R.pool(kind, n, c, e)
    st = R.settings_for(kind, caps)
    got = _run(base, feats, st)
    touched = _check(base, feats, st, got)
    assert _same(got, _run(base, feats, st)), "two calls differ"
    if kind == "descending" and c > 1:
        assert got["counts"][0] == n, "m = n: every item is admitted"
    assert touched[0, got["pred"][0]] or not np.isfinite(base[0]).all(), "item 0 is scored after its own admission"
    for k in sorted({1, n // 2, n - 1} - {0, n}):      # causality: the first k rows of the whole stream are the stream of the first k items
        part = _run(base[:k], feats[:k], st)
        assert _same(part, got, k), k
        for p, name in enumerate(("pos_key", "neg_key")):
            assert np.array_equal(part[name][:part["counts"][p]], [j for j in got[name][:got["counts"][p]] if j < k])
    write_report("stream_cache_kernel.json", _REPORT)


def test_without_a_negative_queue_the_result_is_the_positive_term_alone():
    base, feats = R.pool("normal", 257, 33, 64)
    st = R.settings_for("normal", (3, 0))
    got = _run(base, feats, st)
    assert got["counts"][1] == 0 and np.array_equal(got["neg_leave"], np.arange(257))
    ref, b = R.evaluate64(base, feats, got["pred"], np.zeros((257, 33), dtype=bool), got["pos_leave"], got["neg_leave"], *(st[k] for k in _HEAD))
    assert (np.abs(got["out"] - ref) <= b).all()
    # the plan of a stream WITH a negative queue, evaluated with negative = False, gives the same bits
    from grip_amd import engine
    x, f = torch.from_numpy(base).cuda(), torch.from_numpy(feats).cuda()
    plan = engine.stream_cache_plan(x, **{k: dict(st, neg_cap=2)[k] for k in _PLAN})
    assert int(plan["counts"][1]) > 0
    out = engine.stream_cache_head(x, f, plan, negative=False, **{k: st[k] for k in _HEAD})
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(got["out"]))
    whole, plan2 = engine.stream_cache(x, f, **dict(st, neg_cap=2))
    assert not torch.equal(whole, out) and torch.equal(plan2["neg_leave"], plan["neg_leave"])


def test_bad_arguments_are_refused_on_the_host():
    from grip_amd import engine, native
    x, f = torch.zeros(4, 3, device="cuda"), torch.ones(4, 8, device="cuda")
    plan = engine.stream_cache_plan(x)
    for call in (lambda: engine.stream_cache_plan(x, pos_cap=0), lambda: engine.stream_cache_plan(x, neg_cap=17),
                 lambda: engine.stream_cache_plan(x.double()), lambda: engine.stream_cache_plan(x, neg_entropy=(0.5, 0.2)),
                 lambda: engine.stream_cache_head(x, torch.ones(4, 6, device="cuda"), plan), lambda: engine.stream_cache_head(x, f[:3], plan),
                 lambda: engine.stream_cache_head(x, f, dict(plan, pred=plan["pred"][:2])), lambda: engine.stream_cache_head(x, f, plan, pos_beta=float("nan"))):
        with pytest.raises(native.GripError):
            call()
