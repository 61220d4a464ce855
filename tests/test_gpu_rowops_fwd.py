"""Every kernel of csrc/rowops.hip through its debug hook, element by element against float64 (tests/rowops_fwd_ref.py) under the bound derived in DESIGN.md,
"Row forward and head kernel tests"; nothing in a bound comes from a measurement (tests/test_host_rowops_fwd_ref.py shows that f32 arithmetic meets it and that
fifteen single faults do not).  Every case records its worst |err| / bound in tests/_out/rowops_fwd_kernels.json.

Every input buffer is followed by 32 guard rows of NaN, every output buffer is NaN-prefilled and followed by guard rows: an owned row must come back finite, a
guard row (and every row the kernel does not own) untouched."""
import ctypes
import os
import re

import pytest
import torch

import rowops_fwd_ref as FR
from conftest import REPO, write_report

pytestmark = pytest.mark.gpu
GUARD = 32
WIDTHS = list(FR.WIDTHS)
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
    """x (rows first; a vector counts as one row) followed by GUARD rows of NaN in one allocation; the view of the owned rows."""
    x = x.cuda()
    rows = x if x.dim() > 1 else x[None]
    buf = torch.full((rows.shape[0] + GUARD,) + tuple(rows.shape[1:]), float("nan"), device="cuda", dtype=x.dtype)
    buf[:rows.shape[0]] = rows
    return buf[:rows.shape[0]] if x.dim() > 1 else buf[0]


def _nan_out(n_rows, cols, dtype=torch.float32):
    buf = torch.full((n_rows + GUARD, cols), float("nan"), device="cuda", dtype=dtype)
    return buf, buf[:n_rows]


def _owned(buf, n_rows, what):
    assert torch.isfinite(buf[:n_rows]).all(), f"{what}: an owned row was not written (or is not finite)"
    assert torch.isnan(buf[n_rows:]).all(), f"{what}: a guard row was written"


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _check(kernel, case, what, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = (err / bound).max().item()
    _REPORT.setdefault(case, {})[what] = round(ratio, 4)
    w = _REPORT["worst"]
    w[kernel] = max(w.get(kernel, 0.0), round(ratio, 4))
    assert torch.isfinite(got).all() and (err <= bound).all(), f"{case} {what}: |err| is {ratio:.3f} x its bound"


def _exact(kernel, case):
    _REPORT.setdefault(case, {})["exact"] = 0.0
    _REPORT["worst"].setdefault(kernel, 0.0)


@pytest.fixture(autouse=True)
def _report():
    yield
    write_report("rowops_fwd_kernels.json", _REPORT)


# ------------------------------------------------------------------------------------------------ ln_f16_kernel: the three modes and the gather form
def _ln_run(x, gamma, beta, mode, M, index=None, stride=1, gather=0, n=None):
    """One launch on the first M rows (or the n gathered rows); -> the owned output rows, decoded to a plain [rows, d] tensor for mode 2, and the raw buffer."""
    native, lib = _lib()
    d = x.shape[-1]
    rows = n if gather else M
    buf, out = _nan_out(rows, 2 * d if mode == 2 else d, torch.float16 if mode != 1 else torch.float32)
    native.check(lib.grip_debug_layernorm_modes(_p(x), _p(index), stride, _p(gamma), _p(beta), _p(out), mode, gather, rows, d, _stream()))
    _owned(buf, rows, f"ln mode {mode}")
    return (FR.unsplit(out, rows, d) if mode == 2 else out), out


@pytest.mark.parametrize("family", FR.FAMILIES)
@pytest.mark.parametrize("d", WIDTHS)
def test_layernorm_modes(d, family):
    """d in WIDTHS (NV 1 .. 8, 5 -> 6 and 7 -> 8) x M in 1, 3, 4, 5 x {f16 stream -> f16, f32 -> f32, f32 -> split layout}."""
    native, lib = _lib()
    x16, _, gamma = FR.make_inputs(family, 5, d, 1, seed=d + len(family), device="cuda")
    x32, _, beta = FR.make_rows(family, 5, d, seed=d + len(family), device="cuda")
    x16, x32, gamma, beta = _padded(x16), _padded(x32), _padded(gamma), _padded(beta)
    for mode, x in ((0, x16), (1, x32), (2, x32)):
        ref, bound = FR.ln_fwd(x.double(), gamma, beta)
        bound = bound + (FR.half_bound(ref, bound) if mode == 0 else FR.split_bound(ref, bound) if mode == 2 else 0)
        for M in (1, 3, 4, 5):
            case = f"ln.{family}.d{d}.M{M}.mode{mode}"
            got, raw = _ln_run(x, gamma, beta, mode, M)
            _check("ln_f16_kernel mode %d" % mode, case, family, got, ref[:M], bound[:M])
            assert _same_bits(raw, _ln_run(x, gamma, beta, mode, M)[1]), f"{case}: two runs differ in bits"
        for r in range(5):              # row r of the M = 5 launch against the same row launched alone
            assert _same_bits(raw[r:r + 1], _ln_run(x[r:r + 1], gamma, beta, mode, 1)[1]), f"ln.{family}.d{d}.mode{mode}: row {r} launched alone differs in bits"
    # the f16-in and the f32-in instantiations on an input that is an f16 number
    _, o16 = _ln_run(x16, gamma, beta, 0, 5)
    _, o32 = _ln_run(x16.float().contiguous(), gamma, beta, 1, 5)
    buf, oh = _nan_out(5, d, torch.float16)
    native.check(lib.grip_debug_layernorm(_p(x16.float().contiguous()), _p(gamma), _p(beta), _p(oh), 5, d, _stream()))
    assert _same_bits(o16, o32.half()) and _same_bits(o16, oh), f"ln.{family}.d{d}: the f16-in and f32-in instantiations differ in bits on f16 input"


def _index_for(n, stride):
    return torch.tensor([(0, stride - 1, stride // 2)[b % 3] for b in range(n)], dtype=torch.int32)


@pytest.mark.parametrize("stride", [1, 5, 77])
@pytest.mark.parametrize("d", [128, 768, 1280])
def test_layernorm_gather_form(d, stride):
    """CLS / EOT gather: row r reads x[r stride + index[r]] (index NULL: position 0), read positions 0, stride - 1 and the middle; f16 and f32 streams."""
    n = 4
    k = 0
    for given in (False, True):
        for mode in (0, 1):
            family = FR.FAMILIES[(k + stride + d // 128) % 3]
            k += 1
            case = f"gather_ln.{family}.d{d}.stride{stride}.{'index' if given else 'null'}.mode{mode}"
            x16, _, gamma = FR.make_inputs(family, n * stride, d, 1, seed=d + stride, device="cuda")
            x32, _, beta = FR.make_rows(family, n * stride, d, seed=d + stride, device="cuda")
            x = _padded(x16 if mode == 0 else x32)
            gamma, beta = _padded(gamma), _padded(beta)
            index = _index_for(n, stride).cuda() if given else None
            ref, bound = FR.ln_gather(x, index, stride, n, gamma, beta)
            if mode == 0:
                bound = bound + FR.half_bound(ref, bound)
            got, raw = _ln_run(x, gamma, beta, mode, None, index, stride, 1, n)
            _check("ln_f16_kernel gather", case, family, got, ref, bound)
            at = FR.read_rows(n, stride, index, "cuda")
            assert _same_bits(raw, _ln_run(x[at].contiguous(), gamma, beta, mode, n)[1]), f"{case}: not the bits of the plain form on the gathered rows"


# ------------------------------------------------------------------------------------------------ vit_assemble_ln
FORMS = ((1, 0, 0), (1, 1, 0), (0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1))        # (f32 stream, rowstat, x_lo)


def _assemble_run(patch, cls, pos, prefix, P, gamma, beta, B, G2, d, f32, want_stat, want_lo, per_image, case):
    native, lib = _lib()
    rows = B * (1 + P + G2)
    xbuf, x = _nan_out(rows, d, torch.float32 if f32 else torch.float16)
    sbuf, stat = _nan_out(rows, 2)
    lbuf, lo = _nan_out(rows, d, torch.float16)
    native.check(lib.grip_debug_vit_assemble(_p(patch), _p(cls), _p(pos), _p(prefix), P, _p(gamma), _p(beta), _p(x), f32, _p(stat if want_stat else None), B, G2, d,
                                             _p(lo if want_lo else None), per_image, _stream()))
    _owned(xbuf, rows, case + " x")
    for want, buf, name in ((want_stat, sbuf, "rowstat"), (want_lo, lbuf, "x_lo")):
        if want:
            _owned(buf, rows, f"{case} {name}")
        else:
            assert torch.isnan(buf).all(), f"{case}: {name} was written although NULL was passed"
    return x, stat, lo


@pytest.mark.parametrize("d", [128, 768, 1280, 2048])
@pytest.mark.parametrize("B", [1, 3])
def test_vit_assemble_ln(B, d):
    """P in 0, 1, 4 x G2 in 1, 4, 9 x pos NULL / given x shared / per-image prompt x {f32 stream, f16 stream with and without rowstat and x_lo}; distinct random rows."""
    k = 0
    for P in (0, 1, 4):
        for G2 in (1, 4, 9):
            family = FR.FAMILIES[(k + B + d // 128) % 3]
            k += 1
            n_rows = B * G2 + 1 + (1 + G2) + B * max(P, 1)
            rows, gamma, beta = FR.make_rows(family, n_rows, d, seed=d + 10 * P + G2 + B, device="cuda")
            gamma, beta = _padded(gamma), _padded(beta)
            patch, cls = _padded(rows[:B * G2]), _padded(rows[B * G2])
            pos_rows = _padded(0.5 * rows[B * G2 + 1:B * G2 + 2 + G2])
            pre_all = _padded(rows[B * G2 + 2 + G2:B * G2 + 2 + G2 + B * max(P, 1)])
            for pos in (None, pos_rows):
                for per_image in (0, 1):
                    prefix = (pre_all[:B * P] if per_image else pre_all[:P]) if P else None
                    y, e_y, (mean, e_mean, rstd, e_rstd) = FR.vit_assemble(patch, cls, pos, prefix, gamma, beta, B, P, G2, per_image)
                    for f32, ws, wl in FORMS:
                        case = f"assemble.{family}.d{d}.B{B}.P{P}.G{G2}.pos{int(pos is not None)}.per{per_image}.f32{f32}.stat{ws}.lo{wl}"
                        x, stat, lo = _assemble_run(patch, cls, pos, prefix, P, gamma, beta, B, G2, d, f32, ws, wl, per_image, case)
                        _check("vit_assemble_ln_kernel x", case, "x", x, y, e_y if f32 else e_y + FR.half_bound(y, e_y))
                        if ws:
                            _check("vit_assemble_ln_kernel rowstat", case, "mean", stat[:, :1], mean, e_mean)
                            _check("vit_assemble_ln_kernel rowstat", case, "rstd", stat[:, 1:], rstd, e_rstd)
                        if wl:
                            ref, bound = FR.x_lo(y, e_y, x)
                            _check("vit_assemble_ln_kernel x_lo", case, "x_lo", lo, ref, bound)
                    if per_image and P:      # every image given the same prompt: the bits of the shared form
                        same = _padded(pre_all[:P].repeat(B, 1))
                        a = _assemble_run(patch, cls, pos, same, P, gamma, beta, B, G2, d, 0, 1, 1, 1, "same prompt, per image")
                        b = _assemble_run(patch, cls, pos, pre_all[:P], P, gamma, beta, B, G2, d, 0, 1, 1, 0, "same prompt, shared")
                        assert all(_same_bits(u, v) for u, v in zip(a, b)), f"assemble.d{d}.B{B}.P{P}.G{G2}: shared and per-image forms differ in bits on the same prompt"


# ------------------------------------------------------------------------------------------------ vit_deep_insert (vision and text)
def _finalize(part, parts, M, d):
    """ln_stats_finalize alone (grip_debug_ln_fold with W = NULL) on part [parts, M, 2] -> rowstat [M, 2], NaN-prefilled and guarded."""
    native, lib = _lib()
    sbuf, stat = _nan_out(M, 2)
    native.check(lib.grip_debug_ln_fold(None, None, None, None, None, None, None, 0, 0, _p(part), parts, _p(stat), M, d, _stream()))
    assert torch.isnan(sbuf[M:]).all(), "ln_stats_finalize: a guard row was written"
    return stat


def _deep_case(kernel, case, deep, pc, B, nb, S, P, Ps, M, d, f32, want_lo, want_part, want_stat, text, dest):
    """B: the image / class count passed; nb: the sequences that hold a set of prompt rows (1 in the shared-prefix layout); dest: the stream row of every (b, p),
    [nb, P] long.  Checks the stream, x_lo, stat_part, rowstat and that every other row keeps its NaN prefill."""
    native, lib = _lib()
    tiles = d // 64
    xbuf, x = _nan_out(M, d, torch.float32 if f32 else torch.float16)
    lbuf, lo = _nan_out(M, d, torch.float16)
    pbuf = torch.full((tiles * M + GUARD, 2), float("nan"), device="cuda")
    part = pbuf[:tiles * M].view(tiles, M, 2)
    sbuf, stat = _nan_out(M, 2)
    native.check(lib.grip_debug_deep_insert(_p(deep), pc, _p(x), f32, _p(lo if want_lo else None), _p(part if want_part else None), _p(stat if want_stat else None),
                                            B, S, P, Ps, M, d, text, _stream()))
    src = deep.reshape(pc, P, d)[torch.arange(nb, device="cuda") % pc].reshape(nb * P, d)       # class b reads its own context, or the shared one
    at = dest.reshape(-1)
    other = torch.ones(M + GUARD, dtype=torch.bool, device="cuda")
    other[at] = False
    if not f32:
        _, _, (ts, e_ts, tq, e_tq), (mean, e_mean, rstd, e_rstd) = FR.deep_insert(src, bool(want_lo))
    assert _same_bits(x[at], src if f32 else src.half()), f"{case}: the stream rows are not {'deep' if f32 else 'f16(deep)'}"
    assert torch.isnan(xbuf[other]).all(), f"{case}: a stream row that holds no deep prompt was written"
    if want_lo:
        assert _same_bits(lo[at], (src - src.half().float()).half()), f"{case}: x_lo is not f16(deep - f16(deep))"
    assert torch.isnan(lbuf[other]).all() and (want_lo or torch.isnan(lbuf).all()), f"{case}: an x_lo row that holds no deep prompt was written"
    if want_part:
        _check(kernel, case, "tile sum", part[:, at, 0].T, ts, e_ts)
        _check(kernel, case, "tile sum of squares", part[:, at, 1].T, tq, e_tq)
        assert torch.isnan(part[:, other[:M]]).all() and torch.isnan(pbuf[tiles * M:]).all(), f"{case}: a stat_part pair of another row was written"
    else:
        assert torch.isnan(pbuf).all(), f"{case}: stat_part was written although NULL was passed"
    if want_stat:
        _check(kernel, case, "mean", stat[at, :1], mean, e_mean)
        _check(kernel, case, "rstd", stat[at, 1:], rstd, e_rstd)
    assert torch.isnan(sbuf[other]).all() and (want_stat or torch.isnan(sbuf).all()), f"{case}: a rowstat pair of another row was written"
    if want_part and want_stat:         # "identical roundings": ln_stats_finalize on the stat_part of the same launch
        assert _same_bits(_finalize(part, tiles, M, d)[at], stat[at]), f"{case}: rowstat is not, in bits, ln_stats_finalize of the stat_part of the same launch"
    _exact(kernel, case)


DEEP_FORMS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (0, 1, 1))     # (x_lo, stat_part, rowstat) of an f16 stream


@pytest.mark.parametrize("d", [128, 320, 768, 2048])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_vit_deep_insert(B, d):
    """P in 1, 4 x S in 1 + P, 4 + P x {f32 stream; f16 stream with each of x_lo, stat_part, rowstat, all three, and the two statistics}.  (d = 320 is 5 tiles of 64
    columns: the statistics exist there too.)"""
    k = 0
    for P in (1, 4):
        for S in (1 + P, 4 + P):
            family = FR.FAMILIES[(k + B + d // 64) % 3]
            k += 1
            deep = _padded(FR.make_rows(family, P, d, seed=d + B + P + S, device="cuda")[0])
            M = B * S + 3
            dest = torch.arange(B, device="cuda")[:, None] * S + 1 + torch.arange(P, device="cuda")[None]
            case = f"deep.{family}.d{d}.B{B}.P{P}.S{S}"
            _deep_case("vit_deep_insert_kernel", case + ".f32", deep, 1, B, B, S, P, 0, M, d, 1, 0, 0, 0, 0, dest)
            for wl, wp, ws in DEEP_FORMS:
                _deep_case("vit_deep_insert_kernel", f"{case}.lo{wl}.part{wp}.stat{ws}", deep, 1, B, B, S, P, 0, M, d, 0, wl, wp, ws, 0, dest)


@pytest.mark.parametrize("d", [128, 768])
@pytest.mark.parametrize("C", [1, 5])
def test_text_deep_insert(C, d):
    """prefix_classes in 1, C; the plain layout and the shared-prefix layout (shared_rows = P + 1, one shared context: the P rows exist once)."""
    k = 0
    for P in (1, 4):
        for S in (P + 2, 9):
            for pc, Ps in sorted({(1, 0), (C, 0), (1, P + 1)}):
                family = FR.FAMILIES[(k + C) % 3]
                k += 1
                deep = _padded(FR.make_rows(family, pc * P, d, seed=d + C + P + S + pc, device="cuda")[0])
                M = (Ps + C * (S - Ps) if Ps else C * S) + 2
                nb = 1 if Ps else C
                dest = (torch.arange(nb, device="cuda")[:, None] * S if not Ps else torch.zeros(1, 1, dtype=torch.long, device="cuda")) + 1 + torch.arange(P, device="cuda")[None]
                case = f"text_deep.{family}.d{d}.C{C}.pc{pc}.P{P}.S{S}.shared{Ps}"
                _deep_case("vit_deep_insert_kernel (text)", case + ".f32", deep, pc, C, nb, S, P, Ps, M, d, 1, 0, 0, 0, 1, dest)
                for wp, ws in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    _deep_case("vit_deep_insert_kernel (text)", f"{case}.part{wp}.stat{ws}", deep, pc, C, nb, S, P, Ps, M, d, 0, 0, wp, ws, 1, dest)


# ------------------------------------------------------------------------------------------------ text_embed
@pytest.mark.parametrize("d", [128, 512, 768])
@pytest.mark.parametrize("C", [1, 3, 5])
def test_text_embed(C, d):
    """T in P + 2, 20 x ld_ids in T, 77 x P in 0, 1, 4 x prefix_classes in 1, C x shared_rows in 0, P + 1 x pos NULL / given, vocab 50; ids 0, vocab - 1 and, clamped,
    -1 and vocab.  f16 and f32 streams, rowstat NULL and given."""
    native, lib = _lib()
    vocab = 50
    k = 0
    for P in (0, 1, 4):
        for T in (P + 2, 20):
            family = FR.FAMILIES[(k + C + d // 128) % 3]
            k += 1
            rows, _, _ = FR.make_rows(family, vocab + C * max(P, 1) + T, d, seed=d + C + P + T, device="cuda")
            tok, pre_all, pos_rows = _padded(rows[:vocab]), _padded(rows[vocab:vocab + C * max(P, 1)]), _padded(0.01 * rows[vocab + C * max(P, 1):])
            for ld in sorted({T, 77}):
                g = torch.Generator().manual_seed(d + C + P + T + ld)
                ids = torch.full((C + 1, ld), 2 ** 30, dtype=torch.int32)            # what lies beyond T, and the row after the last class, must not be read
                ids[:C, :T] = torch.randint(0, vocab, (C, T), generator=g).int()
                for c in range(C):
                    ids[c, 0] = (-1, vocab, 0, vocab - 1)[c % 4]
                    ids[c, P + 1] = (0, vocab - 1, -1, vocab)[c % 4]
                ids = ids.cuda()
                for pc in sorted({1, C}):
                    for Ps in ((0, P + 1) if (P and pc == 1) else (0,)):
                        for pos in (None, pos_rows):
                            prefix = pre_all[:pc * P] if P else None
                            v, e_v, (mean, e_mean, rstd, e_rstd) = FR.text_embed(ids[:C], tok, pos, prefix, P, pc, C, T, Ps)
                            n_rows = v.shape[0]
                            for f32, ws in ((0, 0), (0, 1), (1, 1)):
                                case = f"embed.{family}.d{d}.C{C}.T{T}.ld{ld}.P{P}.pc{pc}.shared{Ps}.pos{int(pos is not None)}.f32{f32}.stat{ws}"
                                xbuf, x = _nan_out(n_rows, d, torch.float32 if f32 else torch.float16)
                                sbuf, stat = _nan_out(n_rows, 2)
                                native.check(lib.grip_debug_text_embed(_p(ids), ld, _p(tok), _p(pos), _p(prefix), P, pc, _p(x), f32, _p(stat if ws else None), C, T, d,
                                                                       vocab, Ps, _stream()))
                                _owned(xbuf, n_rows, case)
                                _check("text_embed_kernel x", case, "x", x, v, e_v + (0 if f32 else FR.half_bound(v, e_v)) + 1e-300)
                                v32 = v.float() if pos is None else None              # without pos the row is a copy: exact
                                if v32 is not None:
                                    assert _same_bits(x, v32 if f32 else v32.half()), f"{case}: not a copy of the source row"
                                if ws:
                                    _owned(sbuf, n_rows, case + " rowstat")
                                    _check("text_embed_kernel rowstat", case, "mean", stat[:, :1], mean, e_mean)
                                    _check("text_embed_kernel rowstat", case, "rstd", stat[:, 1:], rstd, e_rstd)
                                else:
                                    assert torch.isnan(sbuf).all(), f"{case}: rowstat was written although NULL was passed"


# ------------------------------------------------------------------------------------------------ im2col, transpose, gather_rows: exact
@pytest.mark.parametrize("patch", [14, 16, 32])
@pytest.mark.parametrize("B", [1, 3])
def test_im2col(B, patch):
    """R in 2 p, 3 p x Kpad in {K rounded up to 8, to 64, that + 64} x the four type pairs against the header's formula as a torch index expression: patch 14 runs
    the per-element path everywhere, 16 and 32 the 8-element path except in the padding, so equality with the formula is equality of the two paths."""
    native, lib = _lib()
    K = 3 * patch * patch
    for R in (2 * patch, 3 * patch):
        img32 = torch.randn(B, 3, R, R, generator=torch.Generator().manual_seed(R + B)).cuda()
        for Kpad in sorted({(K + 7) // 8 * 8, (K + 63) // 64 * 64, (K + 7) // 8 * 8 + 64}):
            for in16 in (0, 1):
                img = _padded(img32.half() if in16 else img32)
                for out32 in (0, 1):
                    case = f"im2col.p{patch}.R{R}.B{B}.Kpad{Kpad}.in16{in16}.out32{out32}"
                    n = B * (R // patch) ** 2
                    obuf, out = _nan_out(n, Kpad, torch.float32 if out32 else torch.float16)
                    native.check(lib.grip_debug_patch_gather(_p(img), in16, _p(out), out32, B, R, patch, Kpad, _stream()))
                    assert torch.isnan(obuf[n:]).all(), f"{case}: a guard row was written"
                    assert _same_bits(out, FR.im2col(img, patch, Kpad, out.dtype)), f"{case}: not the header's formula"
                    assert (_bits(out[:, K:]) == 0).all(), f"{case}: a padding column is not an exact zero"
                    _exact("im2col_kernel", case)


def test_im2col_past_the_grid_cap():
    """B = 112, R = 224, p = 16, Kpad = 768: 2 107 392 eight-element chunks, more than the 8 192 x 256 threads of the capped grid, so the grid-stride loop runs twice."""
    native, lib = _lib()
    B, R, p, Kpad = 112, 224, 16, 768
    img = _padded(torch.randn(B, 3, R, R, generator=torch.Generator().manual_seed(1)).half())
    n = B * (R // p) ** 2
    assert n * (Kpad // 8) > 8192 * 256
    obuf, out = _nan_out(n, Kpad, torch.float16)
    native.check(lib.grip_debug_patch_gather(_p(img), 1, _p(out), 0, B, R, p, Kpad, _stream()))
    assert torch.isnan(obuf[n:]).all(), "a guard row was written"
    assert _same_bits(out, FR.im2col(img, p, Kpad, torch.float16)), "not the header's formula"
    _exact("im2col_kernel", "im2col.past_grid_cap")


@pytest.mark.parametrize("rows,cols", [(1, 1), (63, 65), (64, 64), (65, 63), (130, 200)])
def test_transpose(rows, cols):
    native, lib = _lib()
    for pad in (0, 8):
        for f32 in (0, 1):
            dt = torch.float32 if f32 else torch.float16
            src = torch.randn(rows, cols + pad, generator=torch.Generator().manual_seed(rows + cols)).to(dt)
            src[:, cols:] = float("nan")                 # the columns between cols and ld_in are not part of the matrix
            x = _padded(src)
            obuf, out = _nan_out(cols, rows, dt)
            native.check(lib.grip_debug_transpose(_p(x), _p(out), f32, rows, cols, cols + pad, _stream()))
            case = f"transpose.{rows}x{cols}.ld{cols + pad}.f32{f32}"
            assert torch.isnan(obuf[cols:]).all(), f"{case}: a guard row was written"
            assert _same_bits(out, x[:, :cols].T.contiguous()), f"{case}: not the transpose"
            _exact("transpose_kernel", case)


@pytest.mark.parametrize("stride", [1, 50])
@pytest.mark.parametrize("n", [1, 5])
def test_gather_rows(n, stride):
    native, lib = _lib()
    for four, ds in ((0, (128, 768)), (1, (4, 132, 768))):
        for d in ds:
            for given in (False, True):
                dt = torch.float32 if four else torch.float16
                x = _padded(torch.randn(n * stride, d, generator=torch.Generator().manual_seed(n + stride + d)).to(dt))
                index = _index_for(n, stride).cuda() if given else None
                obuf, out = _nan_out(n, d, dt)
                native.check(lib.grip_debug_gather_rows(_p(x), _p(index), stride, _p(out), n, d, four, _stream()))
                case = f"gather_rows{4 if four else ''}.n{n}.stride{stride}.d{d}.{'index' if given else 'null'}"
                assert torch.isnan(obuf[n:]).all(), f"{case}: a guard row was written"
                assert _same_bits(out, x[FR.read_rows(n, stride, index, "cuda")]), f"{case}: not the read rows"
                _exact("gather_rows4_kernel" if four else "gather_rows_kernel", case)


# ------------------------------------------------------------------------------------------------ ln_stats_finalize, ln_fold_weights
@pytest.mark.parametrize("M", [1, 255, 256, 257])
@pytest.mark.parametrize("parts", [2, 5, 12, 32])
def test_ln_stats_finalize(parts, M):
    native, lib = _lib()
    d = 64 * parts
    family = FR.FAMILIES[(parts + M) % 3]
    rows = FR.make_rows(family, M, d, seed=parts + M, device="cuda")[0]
    t = rows.reshape(M, parts, 64)
    part = torch.stack([t.sum(-1).T, (t * t).sum(-1).T], -1).contiguous()          # [parts, M, 2] f32: the kernel's exact inputs
    pbuf = torch.full((parts * M + GUARD, 2), float("nan"), device="cuda")
    pbuf[:parts * M] = part.reshape(-1, 2)
    mean, e_mean, rstd, e_rstd = FR.stats_finalize(part, d)
    stat = _finalize(pbuf, parts, M, d)
    case = f"finalize.{family}.parts{parts}.M{M}"
    assert torch.isfinite(stat).all(), case
    _check("ln_stats_finalize_kernel", case, "mean", stat[:, :1], mean, e_mean)
    _check("ln_stats_finalize_kernel", case, "rstd", stat[:, 1:], rstd, e_rstd)


@pytest.mark.parametrize("K", [64, 320, 768])
@pytest.mark.parametrize("N", [1, 3, 4, 5])
def test_ln_fold_weights(N, K):
    native, lib = _lib()
    for family in FR.FAMILIES:
        x16, _, gamma = FR.make_inputs(family, N, K, 1, seed=N + K, device="cuda")
        beta = 0.2 * torch.randn(K, generator=torch.Generator().manual_seed(K)).cuda()
        bias = torch.randn(N, generator=torch.Generator().manual_seed(N)).cuda()
        W, gamma, beta, bias = _padded(x16), _padded(gamma), _padded(beta), _padded(bias)
        Wg, (cs, e_cs), (bo, e_bo) = FR.fold_weights(W, gamma, beta, bias)
        wbuf, wg = _nan_out(N, K, torch.float16)
        cbuf, colsum = _nan_out(N, 1)
        bbuf, bout = _nan_out(N, 1)
        native.check(lib.grip_debug_ln_fold(_p(W), _p(gamma), _p(beta), _p(bias), _p(wg), _p(colsum), _p(bout), N, K, None, 0, None, 0, K, _stream()))
        case = f"fold.{family}.N{N}.K{K}"
        for buf in (wbuf, cbuf, bbuf):
            _owned(buf, N, case)
        assert _same_bits(wg, Wg), f"{case}: Wg is not f16(gamma W)"
        _check("ln_fold_weights_kernel", case, "colsum", colsum[:, 0], cs, e_cs)
        _check("ln_fold_weights_kernel", case, "bias_out", bout[:, 0], bo, e_bo)


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_before_any_launch():
    native, lib = _lib()
    header = open(os.path.join(REPO, "include", "grip_amd.h")).read()
    ERR_ARG = int(re.search(r"\bGRIP_ERR_ARG\s*=\s*(\d+)", header).group(1))
    f = torch.full((8192,), float("nan"), device="cuda")                         # never read or written: every call is refused by its launcher
    h = torch.full((8192,), float("nan"), device="cuda", dtype=torch.float16)
    idx = torch.zeros(64, dtype=torch.int32, device="cuda")
    s, N = _stream(), None
    ln = lambda x=f, g=f, out=f, mode=1, gather=0, stride=1, M=1, d=128: lib.grip_debug_layernorm_modes(_p(x), _p(idx), stride, _p(g), _p(f), _p(out), mode, gather, M, d, s)
    asm = lambda patch=f, prefix=f, P=1, x=f, B=1, G2=1, d=128: lib.grip_debug_vit_assemble(_p(patch), _p(f), _p(f), _p(prefix), P, _p(f), _p(f), _p(x), 1, N, B, G2, d, N, 0, s)
    emb = lambda ids=idx, tok=f, prefix=f, P=1, x=f, C=1, T=4, ld=4, d=128, vocab=8: lib.grip_debug_text_embed(_p(ids), ld, _p(tok), _p(f), _p(prefix), P, 1, _p(x), 1, N, C, T, d,
                                                                                                                vocab, 0, s)
    i2c = lambda img=f, out=f, B=1, R=32, patch=16, Kpad=768: lib.grip_debug_patch_gather(_p(img), 0, _p(out), 1, B, R, patch, Kpad, s)
    tr = lambda a=f, b=f, rows=4, cols=4, ld=4: lib.grip_debug_transpose(_p(a), _p(b), 1, rows, cols, ld, s)
    ga = lambda x=f, out=f, n=1, stride=1, d=128, four=1: lib.grip_debug_gather_rows(_p(x), _p(idx), stride, _p(out), n, d, four, s)
    fold = lambda W=h, g=f, N_=1, K=64, part=None, parts=0, stat=None, M=0: lib.grip_debug_ln_fold(_p(W), _p(g), _p(f), _p(f), _p(h), _p(f), _p(f), N_, K, _p(part), parts, _p(stat),
                                                                                                   M, 64, s)
    refused = [
        (lambda: ln(x=None), b"layernorm: null pointer or empty input"), (lambda: ln(M=0), b"layernorm: null pointer or empty input"),
        (lambda: ln(d=130), b"unsupported width 130"), (lambda: ln(mode=2, d=144), b"layernorm (split layout)"),
        (lambda: ln(gather=1, out=None), b"gather_ln: null pointer or bad shape"), (lambda: ln(gather=1, stride=0), b"gather_ln: null pointer or bad shape"),
        (lambda: ln(gather=1, M=0), b"gather_ln: null pointer or bad shape"), (lambda: ln(gather=1, d=2052), b"unsupported width 2052"),
        (lambda: asm(patch=None), b"vit_assemble_ln: null pointer"), (lambda: asm(prefix=None), b"vit_assemble_ln: null pointer"),
        (lambda: asm(B=0), b"vit_assemble_ln: bad shape"), (lambda: asm(G2=0), b"vit_assemble_ln: bad shape"), (lambda: asm(P=-1), b"vit_assemble_ln: bad shape"),
        (lambda: asm(d=130), b"unsupported width 130"),
        (lambda: emb(tok=None), b"text_embed: null pointer"), (lambda: emb(prefix=None), b"text_embed: null pointer"), (lambda: emb(C=0), b"text_embed: bad shape"),
        (lambda: emb(T=1, P=1), b"text_embed: bad shape"), (lambda: emb(vocab=0), b"text_embed: bad shape"), (lambda: emb(T=5, ld=4), b"text_embed: bad shape"),
        (lambda: emb(d=130), b"text_embed: width"),
        (lambda: i2c(img=None), b"im2col: null pointer or empty batch"), (lambda: i2c(B=0), b"im2col: null pointer or empty batch"),
        (lambda: i2c(patch=0), b"im2col: bad geometry"), (lambda: i2c(R=16, patch=32), b"im2col: bad geometry"), (lambda: i2c(R=40), b"im2col: bad geometry"),
        (lambda: i2c(Kpad=760), b"im2col: bad geometry"), (lambda: i2c(Kpad=772), b"im2col: bad geometry"),
        (lambda: tr(a=None), b"transpose: null pointer or bad shape"), (lambda: tr(rows=0), b"transpose: null pointer or bad shape"),
        (lambda: tr(cols=0), b"transpose: null pointer or bad shape"), (lambda: tr(ld=3), b"transpose: null pointer or bad shape"),
        (lambda: ga(x=None), b"gather_rows4: null pointer or bad shape"), (lambda: ga(n=0), b"gather_rows4: null pointer or bad shape"),
        (lambda: ga(stride=0), b"gather_rows4: null pointer or bad shape"), (lambda: ga(d=130), b"gather_rows4: null pointer or bad shape"),
        (lambda: ga(x=h, out=h, four=0, n=0), b"gather_rows: null pointer or bad shape"), (lambda: ga(x=h, out=h, four=0, d=132), b"gather_rows: null pointer or bad shape"),
        (lambda: ga(x=h, out=None, four=0), b"gather_rows: null pointer or bad shape"),
        (lambda: fold(g=None), b"ln_fold_weights: null pointer or bad shape"), (lambda: fold(N_=0), b"ln_fold_weights: null pointer or bad shape"),
        (lambda: fold(K=0), b"ln_fold_weights: null pointer or bad shape"),
        (lambda: fold(W=None, part=f, parts=0, stat=f, M=1), b"ln_stats_finalize: null pointer or bad shape"),
        (lambda: fold(W=None, part=f, parts=1, stat=None, M=1), b"ln_stats_finalize: null pointer or bad shape"),
        (lambda: fold(W=None, part=f, parts=1, stat=f, M=0), b"ln_stats_finalize: null pointer or bad shape"),
    ]
    for i, (call, message) in enumerate(refused):
        assert call() == ERR_ARG, f"call {i} ({message}) was not refused"
        assert message in lib.grip_last_error(), (i, message, lib.grip_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(f).all() and torch.isnan(h).all() and (idx == 0).all(), "a refused call wrote something"
