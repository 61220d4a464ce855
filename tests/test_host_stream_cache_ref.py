"""The two float64 references of tests/stream_cache_ref.py against each other, on the host: the literal item-by-item loop (Python lists per class) and
the interval form (a scan of (H, pred), then every item against the keys with j <= i < leave_j) agree EXACTLY on who is resident when every item is
scored and to 1e-12 on every logit, over the case list of the GPU test; the pools leave at most 1 % of the mask bits undecided by the float64 reference
alone; the pools do what they are built for (m = n with an eviction per item, no admission after the fill, ties keep the earlier item, a NaN row is
never admitted); a stream cut after k items gives the first k rows of the whole stream.  A planted stream reports base against adapted accuracy for
three seeds -- reported, not ranked."""
import numpy as np
import pytest

import stream_cache_ref as R


def _close(a, b, tol):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    scale = np.maximum(1.0, np.abs(np.where(nan, 0.0, a)))
    assert (np.abs(np.where(nan, 0.0, a - b)) <= tol * scale).all(), float(np.nanmax(np.abs(a - b) / scale))


@pytest.mark.parametrize("kind,n,c,e,caps", R.CASES)
def test_the_literal_loop_and_the_interval_form_agree(kind, n, c, e, caps):
    base, feats = R.pool(kind, n, c, e)
    st = R.settings_for(kind, caps)
    lit, ref = R.literal64(base, feats, **st), R.reference64(base, feats, **st)
    for pol in (0, 1):
        assert lit["members"][pol] == ref["members"][pol], f"polarity {pol}: the residents differ"
    _close(lit["out"], ref["out"], 1e-12)
    # the key lists are the ever-admitted items, the intervals start at the item itself
    idx = np.arange(n)
    for pol, name in enumerate(("pos", "neg")):
        ever = sorted(set().union(*ref["members"][pol])) if n else []
        assert ref[name + "_key"].tolist() == ever
        assert (ref[name + "_leave"] >= idx).all()


@pytest.mark.parametrize("kind,n,c,e,caps", R.CASES)
def test_the_float64_reference_decides_the_mask_bits_of_the_pools(kind, n, c, e, caps):
    base, _ = R.pool(kind, n, c, e)
    r = R.rows64(base, R.settings_for(kind, caps)["neg_mask"])
    rows_ok = np.isfinite(base).all(1)
    undecided = int((~r["decided"][rows_ok]).sum())
    assert undecided <= 0.01 * rows_ok.sum() * c, (undecided, rows_ok.sum() * c)
    assert np.array_equal(R.unpack_bits(R.pack_bits(r["bits"]), c), r["bits"])


def test_the_pools_do_what_they_are_built_for():
    n, c, e, cap = 65, 33, 64, 3
    st = R.settings_for("descending", (cap, 2))
    base, feats = R.pool("descending", n, c, e)
    ref = R.reference64(base, feats, **st)
    assert (ref["pred"] == 0).all() and (np.diff(ref["H"]) < 0).all()
    assert len(ref["pos_key"]) == n, "every item is admitted: m = n"
    assert ref["pos_leave"][:n - cap].tolist() == list(range(cap, n)), "once the queue is full every item evicts the oldest (largest H)"
    assert (ref["pos_leave"][n - cap:] == R.INT32_MAX).all()
    base, feats = R.pool("ascending", n, c, e)
    ref = R.reference64(base, feats, **st)
    assert ref["pos_key"].tolist() == list(range(cap)) and (ref["pos_leave"][cap:] == np.arange(cap, n)).all(), "nothing is admitted after the fill"
    # ties: one class, capacity 1 -- the second copy of a row never replaces the first
    base, feats = R.pool("duplicates", 64, 1, e)
    ref = R.reference64(base, feats, **R.settings_for("duplicates", (1, 0)))
    assert ref["pos_key"].tolist() == [0]
    base, feats = R.pool("duplicates", 64, 2, e)
    ref = R.reference64(base, feats, **R.settings_for("duplicates", (1, 0)))
    assert all(j % 2 == 0 for j in ref["pos_key"]), "the later item of an exact tie entered a full queue"
    base, feats = R.pool("nan_row", 65, 33, e)
    ref = R.reference64(base, feats, **R.settings_for("nan_row", (16, 16)))
    assert 32 not in ref["pos_key"] and 32 not in ref["neg_key"] and np.isnan(ref["H"][32]) and ref["pos_leave"][32] == 32
    assert len(ref["neg_key"]) > 0, "the negative queue saw no traffic"


@pytest.mark.parametrize("kind", ["normal", "descending"])
def test_a_stream_cut_short_gives_the_first_rows_of_the_whole_stream(kind):
    n, c, e = 65, 33, 64
    st = R.settings_for(kind, (3, 2))
    base, feats = R.pool(kind, n, c, e)
    whole = R.reference64(base, feats, **st)
    for k in (1, n // 2, n - 1):
        part = R.reference64(base[:k], feats[:k], **st)
        _close(part["out"], whole["out"][:k], 1e-12)      # (numpy's matrix products are not bit-stable across shapes; the kernel's rows are: GPU test)
        assert part["members"][0] == whole["members"][0][:k] and part["members"][1] == whole["members"][1][:k]
        assert part["pos_key"].tolist() == [j for j in whole["pos_key"] if j < k]


def test_no_negative_queue_is_the_positive_term_alone():
    base, feats = R.pool("normal", 65, 33, 64)
    st = R.settings_for("normal", (3, 0))
    ref = R.reference64(base, feats, **st)
    assert len(ref["neg_key"]) == 0
    both = R.reference64(base, feats, **dict(st, neg_cap=2))
    assert np.array_equal(ref["pos_leave"], both["pos_leave"]) and not np.array_equal(ref["out"], both["out"])
    r = R.rows64(base, st["neg_mask"])
    pos_only, _ = R.evaluate64(base, feats, r["pred"], np.zeros_like(r["bits"]), ref["pos_leave"], ref["neg_leave"], st["pos_alpha"], st["pos_beta"],
                               st["neg_alpha"], st["neg_beta"])
    assert np.array_equal(pos_only, ref["out"])


def test_planted_stream_reports_base_against_adapted_accuracy(capsys):
    rows = []
    for seed in (0, 1, 2):
        base, feats, labels = R.planted(seed)
        assert base.shape == (2000, 20) and feats.shape == (2000, 64)
        ref = R.reference64(base, feats)      # the default settings
        acc0, acc1 = float((base.argmax(1) == labels).mean()), float((ref["out"].argmax(1) == labels).mean())
        rows.append((seed, acc0, acc1, len(ref["pos_key"]), len(ref["neg_key"])))
        assert np.isfinite(ref["out"]).all() and 0.0 < acc0 < 1.0
    with capsys.disabled():
        for seed, acc0, acc1, mp, mn in rows:      # reported for all three seeds; no ranking is asserted
            print(f"\nplanted stream seed {seed}: base accuracy {acc0:.4f}, adapted {acc1:.4f} (ever-admitted keys: {mp} positive, {mn} negative)")
