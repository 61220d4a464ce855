"""The GEMM kernels of the f32 tier (gemm_f32_kernel) and of the split-f16 tier (gemm_split1_kernel: three passes; gemm_k64p_kernel<EPI, 3, true>: two
passes through the EMODE 3 epilogue) and the kernels that write the split layout (split_rows_kernel, split_dup_weights_kernel), element by element
against float64 ("Tier kernel tests").

References and bounds are tests/tier_ref.py's (derived, nothing measured).  Every launch goes through grip_debug_gemm_tier, and only after
grip_debug_gemm_plan has named the expected family for these integers (the two-pass form: the persistent kernel's plan with K' = 2 K).  A has m_pad rows,
NaN from row M on; every buffer a kernel reads is followed by 32 NaN rows (the K/V form's W and bias are also PRECEDED by the NaN rows of the projection
they are cut out of); every buffer it writes is NaN-prefilled and 32 rows longer -- with ldc != N the columns outside the window are guards too.  The
operand images of the split tier are built here, in torch, not by the kernels under test.  Owned elements must come back finite and within the bound
(bit-equal to float64 on `grid`, to the exact formed sum on `lo-grid`), guards untouched, no element left out.  The worst |err| / bound of every case
goes to tests/_out/tier_gemm_kernels.json."""
import ctypes

import pytest
import torch

import gemm_cases as GC
import tier_ref as T
from conftest import write_report

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 32
SCALAR = 0.375
REPORT = {}
VISITED = set()
_INPUTS = {}
FORMS = {"f32": (1, 0), "split3": (2, 0), "split2": (2, 1)}          # name -> (tier, w_exact)
KERNEL = {"f32": "gemm_f32_kernel", "split3": "gemm_split1_kernel", "split2": "gemm_k64p_kernel<EPI, 3, true>"}
EPIS = {"f32": (0, 1, 2, 3, 6), "split3": (0, 1, 2, 3), "split2": (0, 1, 2, 3)}
# (M, N, K, kv): kv = the K/V projection of the tiers' last block (N = 2 d, ldc = 3 d, out = qkv + d columns, W = in_w + d rows)
SHAPES = {
    "f32": [(1, 128, 32, 0), (127, 256, 64, 0), (128, 256, 64, 0), (129, 256, 64, 0), (200, 384, 96, 0), (129, 640, 160, 0), (130, 256, 64, 1)],
    "split3": [(1, 256, 64, 0), (255, 256, 64, 0), (256, 256, 64, 0), (257, 256, 64, 0), (100, 512, 192, 0), (257, 768, 256, 0), (130, 512, 64, 1)],
    "split2": [(1, 256, 64, 0), (255, 256, 64, 0), (256, 256, 64, 0), (257, 256, 64, 0), (100, 512, 192, 0), (257, 768, 256, 0), (130, 512, 64, 1)],
}


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
        pytest.exit("GPU error after a tier GEMM launch, stopping: %s" % e, returncode=3)


def inputs_of(family, M, N, K, w_exact):
    key = (family, M, N, K, w_exact)
    if key not in _INPUTS:
        if len(_INPUTS) > 12:
            _INPUTS.clear()
        _INPUTS[key] = T.make_gemm_inputs(family, M, N, K, 2000 + M + 3 * N + 7 * K, w_exact=bool(w_exact), device="cuda")
    return _INPUTS[key]


def families_of(form, K):
    return [f for f in T.GEMM_FAMILIES if not (f == "lo-grid" and (form == "f32" or K > 128)) and not (f == "cancel" and K < 64)]


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def plan_text(lib, form, epi, M, N, K, ldc, m_pad, out2, n_cu=256):
    tier, w_exact = FORMS[form]
    buf = ctypes.create_string_buffer(512)
    if form == "split2":
        rc = lib.grip_debug_gemm_plan(epi, M, N, 2 * K, ldc, m_pad, 6, 0, 0, 0, 0, 0, 0, n_cu, buf, len(buf))
    else:
        rc = lib.grip_debug_gemm_plan(epi, M, N, K, ldc, m_pad, 0, 0, tier, 0, 8 if out2 else 0, 0, 0, n_cu, buf, len(buf))
    return rc, buf.value.decode()


class Launch:
    """The buffers of one launch and, after run(), what it wrote."""

    def __init__(self, form, epi, inp, M, N, K, kv=False, out2=False, inplace=False):
        self.form, self.epi, self.M, self.N, self.K = form, epi, M, N, K
        tier, w_exact = FORMS[form]
        self.ldc, self.col0 = (3 * N // 2, N // 2) if kv else (N, 0)
        self.m_pad = -(-M // 256) * 256
        self.split_out = tier == 2 and epi == T.EPI_GELU
        rows_before = N // 2 if kv else 0          # W and bias of the K/V form start d rows into the packed projection's
        A = _nan(self.m_pad + GUARD, K)
        A[:M] = inp["A"]
        Wf = _nan(rows_before + N + GUARD, K)
        Wf[rows_before:rows_before + N] = inp["W"]
        if tier == 1:
            self.A, self.W, self.w_off = A, Wf, rows_before * K * 4
        else:
            self.A = T.to_layout(*T.split(A))
            hi, lo = T.split(Wf, T.W_SCALE)
            if w_exact:
                assert not bool((lo[rows_before:rows_before + N] != 0).any())
                self.W = T.dup_layout(hi)
            else:
                self.W = T.to_layout(hi, lo)
            self.w_off = rows_before * K * 4
        self.bias = None
        if epi in T.HAS_BIAS:
            self.bias = _nan(rows_before + N + GUARD)
            self.bias[rows_before:rows_before + N] = inp["bias"]
        self.b_off = rows_before * 4
        self.resid = self.wide(inp["resid"]) if epi == T.EPI_RESID else None
        self.out = self.resid if inplace else (_nan(M + GUARD, 2 * self.ldc, dtype=torch.float16) if self.split_out else _nan(M + GUARD, self.ldc))
        self.out2 = _nan(M + GUARD, self.ldc) if out2 else None

    def wide(self, t):
        b = _nan(self.M + GUARD, self.ldc)
        b[:self.M, self.col0:self.col0 + self.N] = t
        return b

    def run(self, lib, native, budget=0):
        tier, w_exact = FORMS[self.form]
        rc, text = plan_text(lib, self.form, self.epi, self.M, self.N, self.K, self.ldc, self.m_pad, self.out2 is not None, budget or 256)
        want = {"f32": "f32", "split3": "split", "split2": "gemm_k64p_kernel<%d," % self.epi}[self.form]
        assert rc == 0 and GC.kernel_of(text).startswith(want), (self.form, text)
        self.plan = GC.plan_fields(text)
        if budget:
            native.check(lib.grip_set_cu_budget(budget))
        try:
            native.check(lib.grip_debug_gemm_tier(tier, w_exact, self.epi, _p(self.A), _p(self.W, self.w_off), self.M, self.N, self.K, self.ldc,
                                                  _p(self.bias, self.b_off), _p(self.resid, 4 * self.col0), _p(self.out, 4 * self.col0),
                                                  _p(self.out2, 4 * self.col0), SCALAR, self.m_pad, _stream()))
        finally:
            if budget:
                native.check(lib.grip_set_cu_budget(0))
        _sync()
        if tier == 2:
            assert lib.grip_debug_split_last_wlo() == (0 if w_exact else 1)
        VISITED.add((KERNEL[self.form], self.epi))
        return self

    def window(self, b):
        """(owned values as stored, guards all still NaN) of a written buffer."""
        M, N = self.M, self.N
        if b.dtype == torch.float16:         # the split layout: lines of [32 hi | 32 lo], row pitch 2 ldc halfs
            v = b.reshape(M + GUARD, self.ldc // 32, 2, 32)
            l0, l1 = self.col0 // 32, (self.col0 + N) // 32
            own = v[:M, l0:l1]
            g = torch.ones(v.shape, dtype=torch.bool, device=b.device)
            g[:M, l0:l1] = False
            return own.contiguous(), bool(torch.isnan(v[g]).all())
        g = torch.ones(b.shape, dtype=torch.bool, device=b.device)
        g[:M, self.col0:self.col0 + N] = False
        return b[:M, self.col0:self.col0 + N].contiguous(), bool(torch.isnan(b[g]).all())

    def values(self):
        """{name: float64 [M, N]} with the guards checked."""
        got = {}
        for name, b in (("out", self.out), ("out2", self.out2)):
            if b is None:
                continue
            own, intact = self.window(b)
            assert intact, (name, "guard touched")
            assert bool(torch.isfinite(own).all()), (name, "owned element not finite")
            if b.dtype == torch.float16:
                own = (own[:, :, 0].double() + own[:, :, 1].double()).reshape(self.M, self.N)
            got[name] = own
        return got

    def bits(self):
        return [self.window(b)[0].view(torch.int16) for b in (self.out, self.out2) if b is not None]


def check(L, inp, family):
    """-> worst |err| / bound over the buffers the launch wrote; raises on a guard, a non-finite element or an exactness statement."""
    tier, w_exact = FORMS[L.form]
    res = T.gemm_reference(inp, tier, L.epi, w_exact=bool(w_exact), scalar=SCALAR, exact_sum=family.startswith("onehot"))
    got = L.values()
    if L.out2 is None:
        res.pop("out2", None)
    worst = 0.0
    for name, (ref, bound) in res.items():
        err = (got[name].double() - ref).abs()
        worst = max(worst, torch.where(bound > 0, err / bound, torch.where(err == 0, 0.0, float("inf"))).max().item())
    if L.epi != T.EPI_GELU and family == "grid":
        T.assert_grid_family(inp, tier)
        assert bool((got["out"].double() == res["out"][0]).all()), "grid: not the float64 value"
    if L.epi != T.EPI_GELU and family == "lo-grid":
        assert bool((got["out"].double() == T.lo_grid_expected(inp, L.epi)).all()), "lo-grid: not the exact formed sum"
    return worst


def variants_of(form, epi):
    if epi == T.EPI_GELU and form == "f32":
        return [dict(out2=True), dict(out2=False)]
    if epi == T.EPI_RESID:
        return [dict(), dict(inplace=True)]
    return [dict()]


def run_shape(form, M, N, K, kv, budget=0, families=None):
    native, lib = _lib()
    tier, w_exact = FORMS[form]
    failures, rows = [], {}
    for family in families or families_of(form, K):
        inp = inputs_of(family, M, N, K, w_exact)
        for epi in EPIS[form]:
            for kw in variants_of(form, epi):
                cid = "%s-e%d-%dx%dx%d%s-%s%s" % (form, epi, M, N, K, "-kv" if kv else "", family, "".join("-" + k for k in kw if kw[k]))
                try:
                    L = Launch(form, epi, inp, M, N, K, kv=bool(kv), **kw).run(lib, native, budget)
                    if budget:
                        assert L.plan["grid"] < L.plan["tiles"], L.plan
                    w = check(L, inp, family)
                    rows[cid] = dict(kernel=KERNEL[form], family=family, worst=w)
                    if not w <= 1.0:
                        failures.append((cid, w))
                except AssertionError as e:
                    failures.append((cid, str(e)[:300]))
    REPORT.update(rows)
    write_report("tier_gemm_kernels.json", REPORT)
    print(form, (M, N, K, kv), "worst |err| / bound:", max(r["worst"] for r in rows.values()) if rows else None)
    assert not failures, failures[:8]


CASES = [(form,) + s for form in FORMS for s in SHAPES[form]]


@pytest.mark.parametrize("form,M,N,K,kv", CASES, ids=["%s-%dx%dx%d%s" % (c[0], c[1], c[2], c[3], "-kv" if c[4] else "") for c in CASES])
def test_every_epilogue_and_family_matches_float64(form, M, N, K, kv):
    run_shape(form, M, N, K, kv)


def test_the_two_pass_pipeline_crosses_tile_boundaries_under_a_cu_budget():
    """12 tiles of 256 x 256 on 8 workgroups: the persistent kernel's K pipeline runs on into the next tile with its first stages under the epilogue."""
    run_shape("split2", 768, 1024, 128, 0, budget=8, families=["randn", "grid", "lo-grid"])


# ------------------------------------------------------------------------------------------------ bit statements
@pytest.mark.parametrize("form", list(FORMS))
def test_a_rows_bits_depend_on_neither_m_nor_its_position_nor_the_run(form):
    native, lib = _lib()
    tier, w_exact = FORMS[form]
    M, N, K, r = 300, 512, 128, 277
    inp = inputs_of("randn", M, N, K, w_exact)
    one = {k: (v[r:r + 1].contiguous() if k in ("A", "resid") else v) for k, v in inp.items()}
    for epi in EPIS[form]:
        a = Launch(form, epi, inp, M, N, K).run(lib, native)
        b = Launch(form, epi, inp, M, N, K).run(lib, native)
        c = Launch(form, epi, one, 1, N, K).run(lib, native)
        for x, y, z in zip(a.bits(), b.bits(), c.bits()):
            assert torch.equal(x, y), (form, epi, "two identical launches differ")
            assert torch.equal(x.reshape(M, -1)[r], z.reshape(-1)), (form, epi, "row %d alone differs from row %d of %d" % (r, r, M))


@pytest.mark.parametrize("form", list(FORMS))
def test_the_residual_in_place_equals_out_of_place(form):
    native, lib = _lib()
    tier, w_exact = FORMS[form]
    for M, N, K, kv in ((300, 512, 128, False), (130, 512, 64, True)):
        inp = inputs_of("randn", M, N, K, w_exact)
        a = Launch(form, 3, inp, M, N, K, kv=kv).run(lib, native)
        b = Launch(form, 3, inp, M, N, K, kv=kv, inplace=True).run(lib, native)
        assert torch.equal(a.bits()[0], b.bits()[0])
        assert b.window(b.out)[1], "in place: guard touched"


# ------------------------------------------------------------------------------------------------ the split layout itself
def _special_values(rows, K, seed):
    """f32 rows holding f16 rounding ties (both parities), f16 subnormals and values below them, -0.0, +-65504 and ordinary numbers."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g) * torch.exp(torch.randn(rows, K, generator=g) * 3)
    x = x.clamp(-6e4, 6e4)
    sp = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2.0 ** -15, 3 * 2.0 ** -26, 2.0 ** -24, 1.5 * 2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 2.0 ** -26,
          -0.0, 0.0, 65504.0, -65504.0, 65504.0 - 2.0 ** -8, 0.1, 2049.0, 2051.0, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -24]
    x.reshape(-1)[:len(sp)] = torch.tensor(sp)
    x.reshape(-1)[K * (rows - 1) + K - len(sp):] = torch.tensor(sp)
    return x


def test_split_rows_writes_exactly_hi_and_lo_at_the_layouts_positions():
    native, lib = _lib()
    rows, K = 37, 96
    x = _special_values(rows, K, 3).cuda()
    xin = torch.cat([x, _nan(GUARD, K)])
    out = _nan(rows + GUARD, 2 * K, dtype=torch.float16)
    native.check(lib.grip_debug_split_rows(_p(xin), _p(out), rows, K, _stream()))
    _sync()
    want = T.to_layout(*T.split(x))
    assert torch.equal(out[:rows].view(torch.int16), want.view(torch.int16))
    assert bool(torch.isnan(out[rows:]).all()), "guard touched"
    hi, lo = T.from_layout(out[:rows], rows, K)
    assert torch.equal(hi.view(torch.int16), x.half().view(torch.int16)) and torch.equal(lo.view(torch.int16), (x - x.half().float()).half().view(torch.int16))
    VISITED.add(("split_rows_kernel", 0))


@pytest.mark.parametrize("dup", [0, 1])
def test_split_weights_writes_the_scaled_image_and_its_flags(dup):
    native, lib = _lib()
    rows, K = 37, 96
    flags = (ctypes.c_int * 2)(7, 7)

    def image(w):
        win = torch.cat([w, _nan(GUARD, K)])
        out = _nan(rows + GUARD, 2 * K, dtype=torch.float16)
        native.check(lib.grip_debug_split_weights(_p(win), _p(out), rows, K, dup, flags, _stream()))
        _sync()
        assert bool(torch.isnan(out[rows:]).all()), "guard touched"
        return out[:rows]

    general = (_special_values(rows, K, 5) / T.W_SCALE).cuda()           # x 2^8 is exact: the image holds the special values themselves
    exact = (general * T.W_SCALE).half().float() / T.W_SCALE            # f16 numbers once scaled
    for w, lo_nonzero in ((general, 1), (exact, 0)):
        if dup and lo_nonzero:
            continue          # the duplicated image exists for f16-exact weights only
        got = image(w)
        hi, lo = T.split(w, T.W_SCALE)
        assert torch.equal(hi.view(torch.int16), (w * T.W_SCALE).half().view(torch.int16))
        want = T.dup_layout(hi) if dup else T.to_layout(hi, lo)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert (flags[0], flags[1]) == (0, lo_nonzero), (flags[0], flags[1])
    if not dup:
        over = exact.clone()
        over[rows // 2, K // 2] = 65520.0 / T.W_SCALE          # rounds to inf in f16 (so it is no f16 number either); the flag is an ordinary store,
        image(over)                                            # no launch consumes this image
        assert flags[0] == 1 and flags[1] == 1, (flags[0], flags[1])
        under = exact.clone()
        under[rows // 2, K // 2] = 65519.0 / T.W_SCALE         # the largest scaled value that still rounds to 65504
        image(under)
        assert flags[0] == 0 and flags[1] == 1, (flags[0], flags[1])
    VISITED.add(("split_dup_weights_kernel" if dup else "split_rows_kernel<weights>", 0))


def test_every_instantiation_named_was_reached():
    want = {(KERNEL[f], e) for f in FORMS for e in EPIS[f]} | {("split_rows_kernel", 0), ("split_rows_kernel<weights>", 0), ("split_dup_weights_kernel", 0)}
    assert VISITED == want, VISITED ^ want
