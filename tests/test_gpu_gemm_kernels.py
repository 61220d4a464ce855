"""Every f16 GEMM kernel instantiation and epilogue of csrc/gemm.hip, element by element against float64 ("f16 GEMM kernel tests").

The cases are tests/gemm_cases.py's (tests/test_host_gemm_ref.py shows that they reach every instantiation), the references and bounds tests/gemm_ref.py's
(derived, nothing measured).  Every launch goes through grip_debug_gemm_args, and only after grip_debug_gemm_plan has named the intended kernel for exactly
these integers.  A has m_pad rows, NaN from row M on; every buffer a kernel reads is followed by 32 NaN rows, every buffer it writes is NaN-prefilled and
32 rows longer -- with ldc = 3 N the columns outside the window are guards too.  Owned elements must come back finite and within the bound (equal to the
float64 value on the `exact` and `onehot` families), guards untouched.  The worst |err| / bound of every case goes to tests/_out/gemm_kernels.json."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import gemm_cases as GC
import gemm_ref as R
from conftest import REPO, write_report

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 32
REPORT = {}
_INPUTS = {}
_CHILD_ABNORMAL = []


def _p(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + offset) if t is not None else ctypes.c_void_p(0)


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native, native.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    """A HIP error after a launch ends the session: nothing more is started on a GPU that has faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a GEMM launch, stopping: %s" % e, returncode=3)


def inputs_of(c):
    """One input set per (family, shape, options that add a buffer): the epilogues of a shape share it, and with it the float64 product."""
    key = (c["family"], c["M"], c["N"], c["K"], c["stat_parts"], c["hilo"])
    if key not in _INPUTS:
        if len(_INPUTS) > 8:
            _INPUTS.clear()
        seed = 1000 + c["M"] + 3 * c["N"] + 7 * c["K"]
        _INPUTS[key] = R.make_inputs(c["family"], c["M"], c["N"], c["K"], seed, "cuda", stat_parts=c["stat_parts"], hilo=c["hilo"])
    return _INPUTS[key]


class Buffers:
    """The device buffers of one launch.  wide(): an [M, N] tensor inside a NaN [(M + GUARD), ldc] buffer at column col0."""

    def __init__(self, c, inp):
        M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
        self.c, self.ldc, self.col0 = c, GC.ldc_of(c), (N if c["ldc3"] else 0)
        self.m_pad = GC.m_pad_of(M)
        dev = "cuda"
        self.A = torch.full((self.m_pad, K), NAN, dtype=torch.float16, device=dev)
        self.A[:M] = inp["A"]
        self.W = inp["W"]
        f32_out = epi in R.F32_OUT
        self.parts = c["ksplit"] if (c["ksplit"] > 1 and not c["coop"]) else 1
        self.out = torch.full((self.parts, M + GUARD, self.ldc), NAN, dtype=torch.float32 if f32_out else torch.float16, device=dev)
        self.resid = self.wide(inp["resid"]) if epi == 3 else None
        self.lo = self.wide(inp["resid_lo"]) if c["hilo"] else None
        self.aux = self.wide(inp["aux"]) if epi == 5 else None
        self.out2 = torch.full((M + GUARD, self.ldc), NAN, dtype=torch.float16, device=dev) if c["out2"] else None
        self.stat_part = torch.full((N // 64 * M + GUARD, 2), NAN, device=dev) if c["stats"] else None
        self.rowstat = self.stat_in = self.colsum = None
        if epi in R.FOLD:
            self.colsum = inp["colsum"]
            self.rowstat = torch.full((M + GUARD, 2), NAN, device=dev)
            if c["stat_parts"]:
                self.stat_in = torch.cat([inp["stat_in"].reshape(-1, 2), torch.full((GUARD, 2), NAN, device=dev)])
            else:
                self.rowstat[:M] = inp["rowstat"]
        self.scratch = self.counter = None
        if c["coop"]:
            self.tiles = -(-M // 64) * (N // 128)
            self.scratch = torch.full((self.tiles * c["ksplit"] * 8192 + GUARD * 64,), NAN, device=dev)
            self.counter = torch.zeros(self.tiles * 4 + GUARD, dtype=torch.int32, device=dev)
        if c["inplace"]:
            self.out = self.resid.unsqueeze(0)

    def wide(self, t):
        b = torch.full((self.c["M"] + GUARD, self.ldc), NAN, dtype=t.dtype, device=t.device)
        b[:self.c["M"], self.col0:self.col0 + self.c["N"]] = t
        return b

    def window(self, b):
        return b[..., :self.c["M"], self.col0:self.col0 + self.c["N"]]

    def guards_intact(self, b):
        g = torch.ones(b.shape, dtype=torch.bool, device=b.device)
        g[..., :self.c["M"], self.col0:self.col0 + self.c["N"]] = False
        return bool(torch.isnan(b[g]).all())


def launch(lib, native, c, inp, m_pad=None):
    """Plan first, then launch: -> Buffers.  A case the plan does not send to the kernel it names (with the launch fields it is there for) is not launched.
    m_pad: the value TOLD to the plan and the launcher, where it is to be smaller than what is allocated."""
    rc, text = GC.plan(lib, c, m_pad=m_pad)
    assert GC.plan_is_intended(c, rc, text), (c["id"], c["kernel"], c["expect"], text)
    b = Buffers(c, inp)
    if m_pad is not None:
        b.m_pad = m_pad
    es = 4 if c["epi"] in R.F32_OUT else 2
    if c["budget"]:
        native.check(lib.grip_set_cu_budget(c["budget"]))
    try:
        native.check(lib.grip_debug_gemm_args(
            c["epi"], _p(b.A), _p(b.W), c["M"], c["N"], c["K"], b.ldc, _p(inp["bias"]) if (c["epi"] in R.HAS_BIAS or c["epi"] in R.FOLD) else None,
            _p(b.resid, 2 * b.col0), _p(b.lo, 2 * b.col0), _p(b.aux, 2 * b.col0), _p(b.out, es * b.col0), _p(b.out2, 2 * b.col0), c["scalar"],
            _p(b.stat_part), _p(b.rowstat), _p(b.colsum), _p(b.stat_in), c["stat_parts"], c["ksplit"] if c["ksplit"] > 1 else 0, GC.split_stride_of(c),
            _p(b.scratch), _p(b.counter), b.m_pad, c["variant"], c["rot_rows"], _stream()))
    finally:
        if c["budget"]:
            native.check(lib.grip_set_cu_budget(0))
    return b


def check(c, inp, b):
    """Every element of every buffer the launch wrote.  -> {name: worst |err| / bound}; raises on a touched guard, a non-finite owned element, an element
    outside its bound or, on the exact families, one that is not the float64 value."""
    M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
    exact = c["family"] in ("exact", "onehot")
    hi = b.window(b.out[0]).contiguous() if c["hilo"] else None
    res = R.reference(inp, epi, ksplit=c["ksplit"], scalar=c["scalar"], stats=c["stats"], hi_stored=hi)
    if exact:
        R.assert_exact_family(inp, res, 9 if c["stats"] else epi)
    got = {}
    if b.parts > 1:       # split-K: every partial against its own K range, and their sum in index order
        w = K // b.parts
        total = None
        for p in range(b.parts):
            sub = dict(inp, A=inp["A"][:, p * w:(p + 1) * w].contiguous(), W=inp["W"][:, p * w:(p + 1) * w].contiguous())
            res["part%d" % p] = R.reference(sub, 0)["out"]
            got["part%d" % p] = b.window(b.out[p])
            total = got["part%d" % p].clone() if total is None else total + got["part%d" % p]
        got["out"] = total
        assert b.guards_intact(b.out), "split-K partial: guard touched"
    else:
        assert b.guards_intact(b.out[0]), "out: guard touched"
        got["out"] = b.window(b.out[0])
    if c["out2"]:
        assert b.guards_intact(b.out2), "out2: guard touched"
        got["out2"] = b.window(b.out2)
    else:
        res.pop("out2", None)
    if c["stats"]:
        assert bool(torch.isnan(b.stat_part[N // 64 * M:]).all()), "stat_part: guard touched"
        got["stat_part"] = b.stat_part[:N // 64 * M].reshape(N // 64, M, 2)
    if c["hilo"]:
        assert b.guards_intact(b.lo), "resid_lo: guard touched"
        got["lo"] = b.window(b.lo)
        got["hilo"] = got["out"].double() + got["lo"].double()
    if c["coop"]:
        assert bool((b.counter == 0).all()), "cooperative split-K: tickets not back to zero"
        assert bool(torch.isnan(b.scratch[b.tiles * c["ksplit"] * 8192:]).all()), "cooperative split-K: scratch guard touched"
    if epi in R.FOLD:
        if c["stat_parts"] and c["variant"] == 6:      # finalised into rowstat by the launcher: M rows written, the guard not
            assert bool(torch.isfinite(b.rowstat[:M]).all()) and bool(torch.isnan(b.rowstat[M:]).all()), "rowstat: finalised rows / guard"
        elif c["stat_parts"]:
            assert bool(torch.isnan(b.rowstat).all()), "rowstat written by a kernel that reads the partial sums itself"
    worst = {}
    for name, (ref, bound) in res.items():
        g = got[name]
        assert bool(torch.isfinite(g).all()), (name, "owned element not finite")
        err = (g.double() - ref).abs()
        ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, 0.0, float("inf"))).max().item()      # (a one-hot row on a zero weight: value and bound are 0)
        worst[name] = ratio
        if exact and name in R.exact_names(9 if c["stats"] else epi, c["hilo"]) and not name.startswith("part"):
            want = ref if name == "hilo" else ref.to(g.dtype)
            assert bool((g == want).all()), _first_mismatch(c, name, g, want)
        if exact and name.startswith("part"):
            assert bool((g.double() == ref).all()), _first_mismatch(c, name, g.double(), ref)
    return worst, got


def _first_mismatch(c, name, g, want):
    """What an exact family's failure says: the first element that is not the float64 value -- for `onehot` with the one k its row reads."""
    bad = (g != want).nonzero()
    at = tuple(int(i) for i in bad[0])
    msg = "%s%s = %r, the float64 value is %r (%d elements differ)" % (name, list(at), g[at].item(), want[at].item(), bad.shape[0])
    if c["family"] == "onehot" and name in ("out", "out2"):
        msg += "; row %d reads k = %d only, column %d" % (at[-2], (7 * at[-2]) % c["K"], at[-1])
    return msg


def run_cases(cases, twice=True):
    """-> (report rows, failures).  Every case is launched (twice: the two runs must agree bit for bit) and checked; a failure does not stop the others."""
    native, lib = _lib()
    rows, failures = {}, []
    for c in cases:
        try:
            inp = inputs_of(c)
            b = launch(lib, native, c, inp)
            _sync()
            worst, _ = check(c, inp, b)
            if twice:
                b2 = launch(lib, native, c, inp)
                _sync()
                for x, y in ((b.out, b2.out), (b.out2, b2.out2), (b.stat_part, b2.stat_part), (b.lo, b2.lo)):
                    if x is not None:
                        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), "two runs differ"
            rows[c["id"] + (" " + c["knob"] if c["knob"] else "")] = dict(kernel=c["kernel"], worst=worst)
            bad = {k: v for k, v in worst.items() if not v <= 1.0}
            if bad:
                failures.append((c["id"], c["kernel"], bad))
        except AssertionError as e:
            failures.append((c["id"], c["kernel"], str(e)[:400]))
    return rows, failures


def _report(rows):
    REPORT.update(rows)
    write_report("gemm_kernels.json", REPORT)


GROUPS = sorted({c["group"] for c in GC.all_cases() if not c["knob"]})


@pytest.mark.parametrize("group", GROUPS)
def test_every_case_of_a_group_matches_float64(group):
    rows, failures = run_cases([c for c in GC.all_cases() if c["group"] == group and not c["knob"]])
    _report(rows)
    print(group, "worst |err| / bound:", max(max(r["worst"].values()) for r in rows.values()) if rows else None)
    assert not failures, failures[:8]


# ------------------------------------------------------------------------------------------------ non-default knobs: one fresh process per set, one after another
_CHILD = "import sys; sys.path.insert(0, {tests!r}); import test_gpu_gemm_kernels as T; T.child_main({knob!r}, {out!r})"


def child_main(knob, out):
    rows, failures = run_cases([c for c in GC.all_cases() if c["knob"] == knob], twice=False)
    with open(out, "w") as f:
        json.dump(dict(rows=rows, failures=failures), f, default=str)


@pytest.mark.parametrize("knob", GC.KNOBS)
def test_the_knob_only_instantiations_match_float64(knob):
    if _CHILD_ABNORMAL:
        pytest.fail("the child of %s ended abnormally: no further child is started" % _CHILD_ABNORMAL[0])
    name, value = knob.split("=")
    env = {k: v for k, v in os.environ.items() if not k.startswith(("GRIP_GEMM_", "GRIP_COOP_SPLIT", "GRIP_KROT_M"))}
    env[name] = value
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "child.json")
        try:
            p = subprocess.run([sys.executable, "-c", _CHILD.format(tests=os.path.join(REPO, "tests"), knob=knob, out=out)], env=env, capture_output=True, text=True,
                               timeout=240)
        except subprocess.TimeoutExpired:
            _CHILD_ABNORMAL.append(knob)
            raise
        if p.returncode != 0 or not os.path.exists(out):
            _CHILD_ABNORMAL.append(knob)
            pytest.fail("child exit %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:]))
        with open(out) as f:
            res = json.load(f)
    assert res["rows"], "the child ran no case"
    _report(res["rows"])
    assert not res["failures"], res["failures"][:8]


# ------------------------------------------------------------------------------------------------ exact statements
def _one(shape, epi, M, N, K, family="randn", **kw):
    return GC._case("statement", GC.SHAPES[shape] if isinstance(shape, str) else shape, epi, M, N, K, family, **kw)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("shape", ["ringw32", "ringw64", "ringw128s", "f16x2", "big128", "big256", "k64x8", "k64x6", "k64p"])
def test_the_residual_in_place_equals_out_of_place_and_the_stream_does_not_depend_on_stat_part(shape):
    native, lib = _lib()
    sh = GC.SHAPES[shape]
    M, N, K = 2 * sh["T"] + 5, sh["Ns"][-1], sh["Ks"][-1]
    outs = []
    variants = [dict(), dict(inplace=True)] + ([] if sh.get("nostats") else [dict(stats=True), dict(stats=True, inplace=True)])
    for kw in variants:
        c = _one(shape, 3, M, N, K, **kw)
        b = launch(lib, native, c, inputs_of(c))
        _sync()
        outs.append(_bits(b.window(b.out[0])))
    for o in outs[1:]:
        assert torch.equal(outs[0], o)


# Same operands through every kernel the plan can give an inference launch (rot_rows = 0), in sets that share (M, N, K) because no single shape is
# accepted by all of them: the two-stage kernel serves K <= 128 at default knobs, the 3-slot ring and the 96-row form need more than 256 64-row tiles,
# the 5-slot 128-row ring more than 12 slices.  Each set holds kernels of other families to compare with.
BIT_SETS = {
    "K320-N384": (389, 384, 320, ["ringw32", "ringw64", "ringw128s", "big128"]),
    "K320-N768": (389, 768, 320, ["ringw32", "ringw64", "ringw128s", "big128", "big256", "k64x8", "k64x6", "k64p"]),
    "two-stage-K64": (389, 384, 64, ["f16x2", "f16x4"]),
    "two-stage-K128": (389, 768, 128, ["f16x2", "ringw128s", "big128", "big256", "k64x8", "k64x6", "k64p"]),
    "ring3-and-96-rows": (2785, 768, 320, ["ring3", "ringw96", "ringw128s", "big128", "big256", "k64x8", "k64x6", "k64p"]),
    "ringw-5-slot": (389, 768, 832, ["ringw128l", "ringw64", "big128", "big256", "k64x8", "k64p"]),
}


@pytest.mark.parametrize("name", sorted(BIT_SETS))
def test_the_inference_kernels_give_one_anothers_bits_without_the_row_rotation(name):
    """tests/test_gpu_determinism.py: "every kernel of gemm.hip sums a row's K slices in the same rotated order" -- with rot_rows = 0 a row's bits must not
    depend on the kernel that serves it.  Held inside each set of BIT_SETS, with the epilogues of the inference path: the bias store, the plain f16 store,
    the statistics-carrying residual (stream and statistics) and the two LayerNorm-folded forms."""
    native, lib = _lib()
    M, N, K, shapes = BIT_SETS[name]
    differ, compared = [], 0
    for epi, kw in ((1, {}), (4, {}), (3, dict(stats=True)), (7, {}), (8, {})):
        first = None
        for shape in shapes:
            sh = GC.SHAPES[shape]
            if (kw.get("stats") and sh.get("nostats")) or epi not in (sh.get("epis") or GC.ALL):
                continue
            c = _one(sh, epi, M, N, K, **kw)
            b = launch(lib, native, c, inputs_of(c))
            _sync()
            got = [_bits(b.window(b.out[0]))] + ([b.stat_part.view(torch.int32).clone()] if kw.get("stats") else [])
            if first is None:
                first = (shape, got)
                continue
            compared += 1
            if not all(torch.equal(x, y) for x, y in zip(first[1], got)):
                differ.append((epi, first[0], shape, [int((x != y).sum()) for x, y in zip(first[1], got)]))
    assert compared >= len(shapes) - 1
    assert not differ, differ


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_launches_write_nothing():
    native, lib = _lib()
    refusals = [
        ("variant 8 with statistics", _one("k64x6", 3, 200, 256, 192, stats=True), {}),
        ("a 96-row epilogue that is not built, reached through an unpadded m_pad", None, {}),
        ("stat_parts without stat_in", _one("ringw128s", 7, 200, 128, 128, stat_parts=2), dict(drop="stat_in")),
        ("the cooperative form without scratch", _one(dict(kern="gemm_ringw_kernel<{e}, 4, 2>", variant=0), 3, 133, 128, 512, ksplit=2, coop=True), dict(drop="scratch")),
        ("split-K with an epilogue that is not EPI_F32", _one("ringw64", 1, 133, 128, 384, ksplit=2), {}),
    ]
    for what, c, opt in refusals:
        if c is None:
            # the 96-row form has three epilogues and no_instance() behind the others.  The plan never names it for them; the one way to it is the
            # automatic choice, and with A not padded to 96-row tiles the plan must keep that launch away too: it goes to the 3-slot ring instead, is
            # launched (A allocated as always, m_pad told as M) and checked like any case
            c = _one(dict(kern="gemm_ring_kernel<{e}, 3>", variant=0), 3, 2785, 768, 320, stats=True)
            inp = inputs_of(c)
            b = launch(lib, native, c, inp, m_pad=2785)
            _sync()
            worst, _ = check(c, inp, b)
            assert max(worst.values()) <= 1.0, (what, worst)
            continue
        inp = inputs_of(c)
        b = Buffers(c, inp)
        before = {k: v.clone() for k, v in vars(b).items() if isinstance(v, torch.Tensor)}
        if opt.get("drop") == "stat_in":
            b.stat_in = None
        if opt.get("drop") == "scratch":
            b.scratch = b.counter = None
        present = GC.present_bits(c) & ~(2 if opt.get("drop") == "stat_in" else 0) & ~(16 if opt.get("drop") == "scratch" else 0)
        rc, text = GC.plan(lib, c, present=present)
        assert rc != 0, (what, text)
        es = 4 if c["epi"] in R.F32_OUT else 2
        rc = lib.grip_debug_gemm_args(
            c["epi"], _p(b.A), _p(b.W), c["M"], c["N"], c["K"], b.ldc, _p(inp["bias"]), _p(b.resid), _p(b.lo), _p(b.aux), _p(b.out, es * b.col0), _p(b.out2), 1.0,
            _p(b.stat_part), _p(b.rowstat), _p(b.colsum), _p(b.stat_in), c["stat_parts"], c["ksplit"] if c["ksplit"] > 1 else 0, GC.split_stride_of(c),
            _p(b.scratch), _p(b.counter), b.m_pad, c["variant"], c["rot_rows"], _stream())
        _sync()
        assert rc != 0 and lib.grip_last_error().decode() == text, (what, rc, text)
        assert bool(torch.isnan(b.out).all()), what
        for k, v in before.items():       # every buffer, read or written, is bit for bit what it was
            assert torch.equal(getattr(b, k).view(torch.int16) if getattr(b, k) is not None else v.view(torch.int16), v.view(torch.int16)), (what, k)
