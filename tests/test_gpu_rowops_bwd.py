"""Every kernel of csrc/rowops_bwd.hip through its debug hook, element by element against float64 (tests/rowops_ref.py) under the bound derived in
DESIGN.md, "Row backward kernel tests"; nothing in a bound comes from a measurement (tests/test_host_rowops_ref.py shows that f32 arithmetic meets
it in three reduction orders and that ten single faults do not).  Every case records its worst |err| / bound in tests/_out/rowops_bwd_kernels.json.

Every input buffer is followed by 32 guard rows of NaN, every output buffer is NaN-prefilled and followed by guard rows: an owned row must come back
finite, a guard row untouched.  The gap between two split-K partials is NaN too.  Only in-range `index` values are passed."""
import ctypes
import os
import re

import pytest
import torch

import rowops_ref as RR
from conftest import REPO, write_report

pytestmark = pytest.mark.gpu
GUARD = 32
WIDTHS = list(RR.WIDTHS)
PARTS = [1, 2, 3, 4, 5, 6, 8, 9]
_REPORT = {"worst": {}}


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native, native.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _padded(x):
    """x (rows first; a vector counts as one row) followed by GUARD rows of NaN in one allocation; returns (buffer, view of the owned rows)."""
    x = x.cuda()
    rows = x if x.dim() > 1 else x[None]
    buf = torch.full((rows.shape[0] + GUARD,) + tuple(rows.shape[1:]), float("nan"), device="cuda", dtype=x.dtype)
    buf[:rows.shape[0]] = rows
    return buf, buf[:rows.shape[0]]


def _nan_out(n_rows, cols, dtype=torch.float32):
    buf = torch.full((n_rows + GUARD, cols), float("nan"), device="cuda", dtype=dtype)
    return buf, buf[:n_rows]


def _owned(buf, n_rows, what):
    assert torch.isfinite(buf[:n_rows]).all(), f"{what}: an owned row was not written (or is not finite)"
    assert torch.isnan(buf[n_rows:]).all(), f"{what}: a guard row was written"


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check(kernel, case, what, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = (err / bound).max().item()
    _REPORT.setdefault(case, {})[what] = round(ratio, 4)
    w = _REPORT["worst"]
    w[kernel] = max(w.get(kernel, 0.0), round(ratio, 4))
    assert torch.isfinite(got).all() and (err <= bound).all(), f"{case} {what}: |err| is {ratio:.3f} x its bound"


@pytest.fixture(autouse=True)
def _report():
    yield
    write_report("rowops_bwd_kernels.json", _REPORT)


# ------------------------------------------------------------------------------------------------ ln_bwd_add
class _AddBuffers:
    """The device buffers of one ln_bwd_add shape: x, the `parts` partials part_stride = M d + 4 d floats apart with NaN between and after them, gamma,
    and the previous dx.  run() restores dx, NaN-fills dxh, launches M_run <= M rows and returns copies of the rows it owns."""

    def __init__(self, x, dyp, gamma, old):
        self.parts, self.M, self.d = dyp.shape
        self.stride = self.M * self.d + 4 * self.d
        self.xbuf, self.x = _padded(x)
        self.gbuf, self.gamma = _padded(gamma)
        self.dln = torch.full((self.parts * self.stride + GUARD * self.d,), float("nan"), device="cuda")
        for p in range(self.parts):
            self.dln[p * self.stride:p * self.stride + self.M * self.d] = dyp[p].reshape(-1)
        self.old = old.cuda()

    def run(self, what, M_run=None):
        native, lib = _lib()
        M = self.M if M_run is None else M_run
        dbuf, dx = _padded(self.old[:M])
        hbuf, dxh = _nan_out(M, self.d, torch.float16)
        native.check(lib.grip_debug_ln_bwd_add(_p(self.x), _p(self.dln), self.parts, self.stride, _p(self.gamma), _p(dx), _p(dxh), M, self.d, _stream()))
        _owned(dbuf, M, what + " dx")
        _owned(hbuf, M, what + " dxh")
        return dx, dxh


def _add_case(case, x, dyp, gamma, old, alone=False):
    M = x.shape[0]
    ref, bound = RR.ln_bwd_add(x, dyp, gamma, old)
    bufs = _AddBuffers(x, dyp, gamma, old)
    dx, dxh = bufs.run(case)
    _check("ln_bwd_add", case, "dx", dx, ref, bound)
    _check("ln_bwd_add", case, "dxh", dxh, ref, bound + RR.half_bound(ref, bound))
    assert _same_bits(dxh, dx.half()), f"{case}: dxh is not f16(dx)"
    dx2, dxh2 = bufs.run(case)
    assert _same_bits(dx, dx2) and _same_bits(dxh, dxh2), f"{case}: two runs differ in bits"
    if alone:
        for r in range(M):
            one = _AddBuffers(x[r:r + 1], dyp[:, r:r + 1], gamma, old[r:r + 1])
            rx, rxh = one.run(case)
            assert _same_bits(rx[0], dx[r]) and _same_bits(rxh[0], dxh[r]), f"{case}: row {r} launched alone differs in bits"
    return bufs, dx, dxh


@pytest.mark.parametrize("family", RR.FAMILIES)
@pytest.mark.parametrize("d", WIDTHS)
def test_ln_bwd_add_few_rows(d, family):
    """The full cross of width x family x M in 1, 3, 4, 5 x every partial count (add_parts<1..4> and their combinations up to 4 + 4)."""
    x, dyp, gamma = RR.make_inputs(family, 5, d, max(PARTS), seed=d + len(family), device="cuda")
    old = torch.randn(5, d, generator=torch.Generator().manual_seed(d)).cuda()
    for M in (1, 3, 4, 5):
        for parts in PARTS:
            _add_case(f"add.{family}.d{d}.M{M}.p{parts}", x[:M], dyp[:parts, :M], gamma, old[:M], alone=M == 5)


@pytest.mark.parametrize("family", RR.FAMILIES)
@pytest.mark.parametrize("M", [1024, 1025])
@pytest.mark.parametrize("i", range(len(WIDTHS)))
def test_ln_bwd_add_early_and_streaming(i, M, family):
    """M = 1024 is the last EARLY launch (every load in flight), M = 1025 the first streaming one: every width and every partial count in both."""
    d, parts = WIDTHS[i], PARTS[(i + len(family)) % len(PARTS)]
    x, dyp, gamma = RR.make_inputs(family, M, d, parts, seed=d + M + parts, device="cuda")
    old = torch.randn(M, d, generator=torch.Generator().manual_seed(d)).cuda()
    _add_case(f"add.{family}.d{d}.M{M}.p{parts}", x, dyp, gamma, old)


@pytest.mark.parametrize("d,parts", [(768, 3), (512, 8)])
def test_ln_bwd_add_streaming_and_early_forms_on_the_same_buffers(d, parts):
    """Rows 0 .. 1023 of the M = 1025 launch (streaming form) against the M = 1024 launch (EARLY form) on the same buffers.  The source comment used to
    promise the same bits; on an MI355X 38 793 of 786 432 elements (4.9 %) differ in bits at d = 768, parts = 3 (NV = 3) and none at d = 512, parts = 8
    (NV = 2), because the compiler contracts other multiply-add pairs in the two forms of some instantiations (fp-contract=fast).  The comment and DESIGN now say so; what holds, and is asserted, is that each form is
    within the derived bound of the same float64 value on every element (so the two are within twice the bound of each other), that each is
    bit-reproducible, and that the f16 copy of each is f16(dx).  The share of differing elements is recorded."""
    x, dyp, gamma = RR.make_inputs("randn", 1025, d, parts, seed=d, device="cuda")
    old = torch.randn(1025, d, generator=torch.Generator().manual_seed(d)).cuda()
    ref, bound = RR.ln_bwd_add(x, dyp, gamma, old)
    bufs = _AddBuffers(x, dyp, gamma, old)
    case = f"add.forms.d{d}.p{parts}"
    sx, sxh = bufs.run("streaming", 1025)
    ex, exh = bufs.run("early", 1024)
    _check("ln_bwd_add", case, "streaming dx", sx, ref, bound)
    _check("ln_bwd_add", case, "early dx", ex, ref[:1024], bound[:1024])
    assert ((sx[:1024].double() - ex.double()).abs() <= 2 * bound[:1024]).all(), f"{case}: the two forms are further apart than twice the bound"
    assert _same_bits(sxh, sx.half()) and _same_bits(exh, ex.half()), f"{case}: dxh is not f16(dx)"
    sx2, _ = bufs.run("streaming", 1025)
    ex2, _ = bufs.run("early", 1024)
    assert _same_bits(sx, sx2) and _same_bits(ex, ex2), f"{case}: two runs of one form differ in bits"
    _REPORT[case]["share of elements whose bits differ between the forms"] = round((_bits(sx[:1024]) != _bits(ex)).float().mean().item(), 5)


# ------------------------------------------------------------------------------------------------ ln_bwd_init
def _index_for(n, stride, first=0):
    """Read positions 0, stride - 1 and the middle, cycled over the sequences (offset by `first` in the fill form's convention)."""
    return torch.tensor([first + (0, stride - 1, stride // 2)[b % 3] for b in range(n)], dtype=torch.int32)


@pytest.mark.parametrize("d", [128, 768, 1280])
@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("stride", [1, 5, 77])
def test_ln_bwd_init(stride, parts, d):
    native, lib = _lib()
    n = 3
    M = n * stride
    for k, given in enumerate((False, True)):
        family = RR.FAMILIES[(stride + parts + d // 128 + k) % 3]
        case = f"init.{family}.d{d}.stride{stride}.p{parts}.{'index' if given else 'null'}"
        x, dyp, gamma = RR.make_inputs(family, M, d, parts, seed=d + stride + parts, device="cuda")
        rows_add = torch.randn(n, d, generator=torch.Generator().manual_seed(stride)).cuda()
        index = _index_for(n, stride).cuda() if given else None
        ref, bound = RR.ln_bwd_init(x, dyp, gamma, rows_add, index, stride)
        bufs = _AddBuffers(x, dyp, gamma, torch.zeros(M, d))
        abuf, add = _padded(rows_add)
        dbuf, dx = _nan_out(M, d)
        hbuf, dxh = _nan_out(M, d, torch.float16)
        native.check(lib.grip_debug_ln_bwd_init(_p(bufs.x), _p(bufs.dln), parts, bufs.stride, _p(bufs.gamma), _p(add), _p(index), stride, _p(dx), _p(dxh),
                                                M, d, _stream()))
        _owned(dbuf, M, case)
        _owned(hbuf, M, case)
        _check("ln_bwd_init", case, "dx", dx, ref, bound)
        _check("ln_bwd_init", case, "dxh", dxh, ref, bound + RR.half_bound(ref, bound))
        assert _same_bits(dxh, dx.half()), f"{case}: dxh is not f16(dx)"


# ------------------------------------------------------------------------------------------------ ln_bwd_scatter / ln_bwd_scatter_fill
def _scatter_case(case, kernel, family, n, stride, first, M, d, index, fill):
    native, lib = _lib()
    x, dyp, gamma = RR.make_inputs(family, max(M, n), d, 1, seed=d + n + stride + first, device="cuda")
    x, dy = x[:M], dyp[0, :n]
    ref, bound, at = RR.ln_bwd_scatter(x, dy, gamma, index, stride, M)
    xbuf, xv = _padded(x)
    ybuf, yv = _padded(dy)
    gbuf, gv = _padded(gamma)
    dbuf, dx = _nan_out(M, d)
    hbuf, dxh = _nan_out(M, d, torch.float16)
    native.check(lib.grip_debug_ln_bwd_scatter(_p(xv), _p(yv), _p(index), stride, first, _p(gv), _p(dx), _p(dxh), n, M, d, fill, _stream()))
    other = torch.ones(M, dtype=torch.bool, device="cuda")
    other[at] = False
    assert torch.isnan(dbuf[M:]).all() and torch.isnan(hbuf[M:]).all(), f"{case}: a guard row was written"
    _check(kernel, case, "dx", dx[at], ref[at], bound[at])
    _check(kernel, case, "dxh", dxh[at], ref[at], bound[at] + RR.half_bound(ref[at], bound[at]))
    assert _same_bits(dxh[at], dx[at].half()), f"{case}: dxh is not f16(dx)"
    if fill:
        assert (_bits(dx[other]) == 0).all() and (_bits(dxh[other]) == 0).all(), f"{case}: a row that is no read row is not exactly zero"
    else:
        assert torch.isnan(dx[other]).all() and torch.isnan(dxh[other]).all(), f"{case}: a row that is no read row was written"


@pytest.mark.parametrize("stride", [1, 50, 77])
@pytest.mark.parametrize("n", [1, 4, 5])
def test_ln_bwd_scatter(n, stride):
    ds = (128, 320, 768, 1280, 2048)
    k = 0
    for given in (False, True):
        for d in (ds[(n + stride) % 5], ds[(n + stride + 2) % 5]):
            family = RR.FAMILIES[k % 3]
            k += 1
            index = _index_for(n, stride).cuda() if given else None
            _scatter_case(f"scatter.{family}.d{d}.n{n}.stride{stride}.{'index' if given else 'null'}", "ln_bwd_scatter", family, n, stride, 0, n * stride, d, index, 0)


@pytest.mark.parametrize("first", [0, 16])
@pytest.mark.parametrize("stride", [1, 50, 77])
@pytest.mark.parametrize("n", [1, 4, 5])
def test_ln_bwd_scatter_fill(n, stride, first):
    """Sequences start at row `first`; the read row of sequence b is b * stride + index[b] with first <= index[b] < first + stride (csrc/tower.hip), so a
    NULL index (position 0) exists for first = 0 only.  Rows before `first` and the three rows after the last sequence must be zero."""
    ds = (128, 320, 768, 1280, 2048)
    k = 0
    for extra in (0, 3):
        M = first + n * stride + extra
        for given in ((False, True) if first == 0 else (True,)):
            d = ds[(n + stride + first + k) % 5]
            family = RR.FAMILIES[k % 3]
            k += 1
            index = _index_for(n, stride, first).cuda() if given else None
            _scatter_case(f"fill.{family}.d{d}.n{n}.stride{stride}.first{first}.M{M}.{'index' if given else 'null'}", "ln_bwd_scatter_fill", family, n, stride,
                          first, M, d, index, 1)


# ------------------------------------------------------------------------------------------------ vit_prefix_grad (shared, per image, deep)
def _vit_deep_emulation(rows, inv):
    """f32 adds in the kernel's stated order: wave w adds b = w, w + 8, ..., then wave 0 adds waves 1 .. 7 in order, then x scale.  rows [B, P, d] f32."""
    B = rows.shape[0]
    acc = [torch.zeros_like(rows[0]) for _ in range(8)]
    for w in range(8):
        for b in range(w, B, 8):
            acc[w] = acc[w] + rows[b]
    for w in range(1, 8):
        acc[0] = acc[0] + acc[w]
    return acc[0] * inv


@pytest.mark.parametrize("d", [128, 768, 2048])
@pytest.mark.parametrize("B", [1, 7, 8, 9, 17])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_vit_prefix_grad(mode, B, d):
    native, lib = _lib()
    kernel = ("vit_prefix_grad", "vit_prefix_grad_per_image", "vit_deep_grad")[mode]
    k = 0
    for P in (1, 4):
        for S in (1 + P, 1 + P + 3):
            for inv in (1.0, 2.0 ** -7):
                family = RR.FAMILIES[(k + B) % 3]
                k += 1
                case = f"vit{mode}.{family}.d{d}.B{B}.P{P}.S{S}.inv{inv:g}"
                n_pre = B * P if mode == 1 else P
                g = torch.Generator().manual_seed(d + B + P + S)
                x, dyp, gamma = RR.make_inputs(family, max(B * S, n_pre), d, 1, seed=d + B + P + S, device="cuda")
                prefix = (x[:n_pre].float() * (1 + 1e-4 * torch.randn(n_pre, d, generator=g).cuda())).contiguous()      # f32 values that are not f16 numbers
                stream = dyp[0, :B * S].contiguous()
                ref, bound = RR.vit_prefix_grad(stream, prefix, gamma, inv, B, S, P, mode)
                sbuf, sv = _padded(stream)
                hbuf, hv = _nan_out(B * S, d, torch.float16)
                pbuf, pv = _padded(prefix)
                gbuf, gv = _padded(gamma)
                cbuf, cv = _padded(torch.tensor([float("nan"), inv]))          # scale[0] is not read
                obuf, out = _nan_out(n_pre, d)
                native.check(lib.grip_debug_vit_prefix_grad(_p(sv), _p(hv), _p(pv), _p(gv), _p(cv), _p(out), B, S, P, d, mode, _stream()))
                _owned(obuf, n_pre, case)
                _check(kernel, case, "grad", out, ref.reshape(n_pre, d), bound.reshape(n_pre, d))
                assert torch.isnan(sbuf[B * S:]).all() and torch.isnan(hbuf[B * S:]).all(), f"{case}: a guard row of dx / dxh was written"
                if mode != 2:
                    assert _same_bits(sv, stream) and torch.isnan(hv).all(), f"{case}: dx / dxh must not be written"
                    continue
                emu = _vit_deep_emulation(stream.reshape(B, S, d)[:, 1:1 + P], inv)
                assert _same_bits(out, emu), f"{case}: not the bits of the stated order of f32 adds"
                read = torch.zeros(B, S, dtype=torch.bool, device="cuda")
                read[:, 1:1 + P] = True
                read = read.reshape(-1)
                assert (_bits(sv[read]) == 0).all() and (_bits(hv[read]) == 0).all(), f"{case}: a row that was summed is not exactly zero"
                assert _same_bits(sv[~read], stream[~read]) and torch.isnan(hv[~read]).all(), f"{case}: a row that was not summed was written"


# ------------------------------------------------------------------------------------------------ text_prefix_grad (shallow, deep)
@pytest.mark.parametrize("d", [128, 320, 512])
@pytest.mark.parametrize("C", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("deep", [0, 1])
def test_text_prefix_grad(deep, C, d):
    native, lib = _lib()
    kernel = "text_deep_grad" if deep else "text_prefix_grad"
    for P in (1, 4):
        for T in (P + 2, 77):
            g = torch.Generator().manual_seed(d + C + P + T)
            stream = torch.randn(C * T, d, generator=g) * (1 + 100 * (torch.rand(C * T, d, generator=g) < 0.01))
            stream = stream.cuda()
            for pc in sorted({1, C}):
                inv = (1.0, 2.0 ** -7)[(P + T + pc) % 2]
                case = f"text{deep}.d{d}.C{C}.pc{pc}.P{P}.T{T}.inv{inv:g}"
                ref, bound = RR.text_prefix_grad(stream, inv, C, T, P, pc)
                sbuf, sv = _padded(stream)
                hbuf, hv = _nan_out(C * T, d, torch.float16)
                cbuf, cv = _padded(torch.tensor([float("nan"), inv]))
                obuf, out = _nan_out(pc * P, d)
                native.check(lib.grip_debug_text_prefix_grad(_p(sv), _p(hv), _p(cv), _p(out), C, T, P, pc, d, deep, _stream()))
                _owned(obuf, pc * P, case)
                _check(kernel, case, "grad", out, ref.reshape(pc * P, d), bound.reshape(pc * P, d))
                rows = stream.reshape(C, T, d)[:, 1:1 + P]
                if pc == 1:
                    emu = torch.zeros(P, d, device="cuda")
                    for c in range(C):
                        emu = emu + rows[c]                                   # sequential f32 adds in class order
                else:
                    emu = rows
                assert _same_bits(out, (emu * inv).reshape(pc * P, d)), f"{case}: not the bits of sequential f32 adds in class order"
                assert torch.isnan(sbuf[C * T:]).all() and torch.isnan(hbuf[C * T:]).all(), f"{case}: a guard row of dx / dxh was written"
                if not deep:
                    assert _same_bits(sv, stream) and torch.isnan(hv).all(), f"{case}: dx / dxh must not be written"
                    continue
                read = torch.zeros(C, T, dtype=torch.bool, device="cuda")
                read[:, 1:1 + P] = True
                read = read.reshape(-1)
                assert (_bits(sv[read]) == 0).all() and (_bits(hv[read]) == 0).all(), f"{case}: a row that was summed is not exactly zero"
                assert _same_bits(sv[~read], stream[~read]) and torch.isnan(hv[~read]).all(), f"{case}: a row that was not summed was written"


# ------------------------------------------------------------------------------------------------ grad_scale_cast
def _scale_inputs(kind, n, g):
    pos = n - 1                                             # the amax element last: the scalar tail and the last vector must see it
    v = torch.randn(n, generator=g)
    if kind == "randn":
        return v * 1e-3
    if kind in ("amax32", "below64"):
        v = (2 * torch.rand(n, generator=g) - 1) * 20
        v[pos] = 32.0 if kind == "amax32" else -torch.nextafter(torch.tensor(64.0), torch.tensor(0.0)).item()
        return v
    if kind == "zeros":
        return torch.zeros(n)
    if kind == "tiny":
        v = (2 * torch.rand(n, generator=g) - 1) * 1e-30
        v[pos] = 1e-30
        return v
    v[pos] = float("inf")
    return v


@pytest.mark.parametrize("kind", ["randn", "amax32", "below64", "zeros", "tiny", "inf"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4096, 65536, 65537, 65540, 200000])
def test_grad_scale_cast(n, kind):
    """Registers (n % 4 == 0, n <= 65 536), two loops over memory, and the scalar path (n % 4 != 0).  Everything is exact."""
    native, lib = _lib()
    case = f"scale.{kind}.n{n}"
    v = _scale_inputs(kind, n, torch.Generator().manual_seed(n)).cuda()
    s0, s1, g16 = RR.grad_scale_cast(v)
    vbuf = torch.full((n + GUARD * 64,), float("nan"), device="cuda")
    vbuf[:n] = v
    obuf = torch.full((n + GUARD * 64,), float("nan"), device="cuda", dtype=torch.float16)
    cbuf = torch.full((2 + GUARD,), float("nan"), device="cuda")
    native.check(lib.grip_debug_grad_scale_cast(_p(vbuf), _p(obuf), _p(cbuf), n, _stream()))
    assert torch.isnan(obuf[n:]).all() and torch.isnan(cbuf[2:]).all(), f"{case}: a guard element was written"
    got0, got1 = cbuf[0].item(), cbuf[1].item()
    assert (got0, got1) == (s0, s1), f"{case}: scale ({got0}, {got1}), expected ({s0}, {s1})"
    amax = v.abs().max().item()
    want = {"randn": None, "amax32": 1.0, "below64": 1.0, "zeros": 1.0, "tiny": 2.0 ** 40, "inf": 1.0}[kind]
    if want is None:
        assert 32.0 <= amax * got0 < 64.0 and got0 * got1 == 1.0, f"{case}: amax {amax} x scale {got0} is outside [32, 64)"
    else:
        assert (got0, got1) == (want, 1.0 / want), f"{case}: scale ({got0}, {got1})"
    assert _same_bits(obuf[:n], (v * cbuf[0]).half()) and _same_bits(obuf[:n], g16), f"{case}: g16 is not f16(g x scale[0])"
    _REPORT.setdefault(case, {})["exact"] = 0.0
    _REPORT["worst"].setdefault("grad_scale_cast", 0.0)


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_any_launch():
    native, lib = _lib()
    header = open(os.path.join(REPO, "include", "grip_amd.h")).read()
    ERR_ARG = int(re.search(r"\bGRIP_ERR_ARG\s*=\s*(\d+)", header).group(1))
    f = torch.full((4096,), float("nan"), device="cuda")                         # never read or written: every call is refused by its launcher
    h = torch.full((4096,), float("nan"), device="cuda", dtype=torch.float16)
    idx = torch.zeros(8, dtype=torch.int32, device="cuda")
    s = _stream()
    add = lambda d=128, parts=1, stride=1024: lib.grip_debug_ln_bwd_add(_p(h), _p(f), parts, stride, _p(f), _p(f), _p(h), 1, d, s)
    init = lambda d=128, parts=1, stride=1024, seq=1: lib.grip_debug_ln_bwd_init(_p(h), _p(f), parts, stride, _p(f), _p(f), _p(idx), seq, _p(f), _p(h), 1, d, s)
    scat = lambda d=128, stride=1, first=0, fill=1: lib.grip_debug_ln_bwd_scatter(_p(h), _p(f), _p(idx), stride, first, _p(f), _p(f), _p(h), 1, 1, d, fill, s)
    vit = lambda mode, B=1, S=2, P=1, d=128: lib.grip_debug_vit_prefix_grad(_p(f), _p(h), _p(f), _p(f), _p(f), _p(f), B, S, P, d, mode, s)
    text = lambda deep, C=2, T=3, P=1, pc=1, d=128: lib.grip_debug_text_prefix_grad(_p(f), _p(h), _p(f), _p(f), C, T, P, pc, d, deep, s)
    refused = [
        (lambda: add(d=130), b"unsupported width 130"), (lambda: add(d=2052), b"unsupported width 2052"),
        (lambda: add(parts=0), b"ln_bwd_add: bad partial layout"), (lambda: add(stride=1026), b"ln_bwd_add: bad partial layout"),
        (lambda: init(d=130), b"unsupported width 130"), (lambda: init(d=2052), b"unsupported width 2052"),
        (lambda: init(parts=0), b"ln_bwd_init: bad layout"), (lambda: init(stride=1026), b"ln_bwd_init: bad layout"), (lambda: init(seq=0), b"ln_bwd_init: bad layout"),
        (lambda: scat(d=130), b"unsupported width 130"), (lambda: scat(d=2052), b"unsupported width 2052"), (lambda: scat(d=130, fill=0), b"unsupported width 130"),
        (lambda: scat(stride=0), b"ln_bwd_scatter_fill: bad layout"), (lambda: scat(first=-1), b"ln_bwd_scatter_fill: bad layout"),
    ]
    for mode, name in ((0, b"vit_prefix_grad: bad shape"), (1, b"vit_prefix_grad_per_image: bad shape"), (2, b"vit_deep_grad: bad arguments")):
        refused += [(lambda m=mode: vit(m, B=0), name), (lambda m=mode: vit(m, P=0), name), (lambda m=mode: vit(m, S=2, P=2), name),
                    (lambda m=mode: vit(m, d=130), b"unsupported width 130"), (lambda m=mode: vit(m, d=2052), b"unsupported width 2052")]
    for deep, name in ((0, b"text_prefix_grad: bad arguments"), (1, b"text_deep_grad: bad arguments")):
        refused += [(lambda k=deep: text(k, C=0), name), (lambda k=deep: text(k, P=0), name), (lambda k=deep: text(k, T=2, P=1), name),
                    (lambda k=deep: text(k, d=130), name), (lambda k=deep: text(k, C=3, pc=2), name)]
    for i, (call, message) in enumerate(refused):
        assert call() == ERR_ARG, f"call {i} ({message}) was not refused"
        assert message in lib.grip_last_error(), (i, message, lib.grip_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(f).all() and torch.isnan(h).all() and (idx == 0).all(), "a refused call wrote something"
