"""The head kernels of csrc/head.hip (public ABI: grip_cosine_head, grip_cosine_head_backward, grip_weighted_ce), element by element against float64
(tests/head_ref.py) under the bound derived in DESIGN.md, "Row forward and head kernel tests"; nothing in a bound comes from a measurement
(tests/test_host_head_ref.py).  Every case records its worst |err| / bound in tests/_out/head_kernels.json.

Every input buffer is followed by 32 guard rows of NaN, every output buffer is NaN-prefilled and followed by guard rows that must keep their bits.  No test
feeds zero-norm rows or non-finite embeddings."""
import ctypes

import pytest
import torch

import head_ref as HR
from conftest import write_report

pytestmark = pytest.mark.gpu
GUARD = 32
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
    x = x.cuda()
    rows = x if x.dim() > 1 else x[:, None]
    buf = torch.full((rows.shape[0] + GUARD,) + tuple(rows.shape[1:]), float("nan") if x.is_floating_point() else 2 ** 30, device="cuda", dtype=x.dtype)
    buf[:rows.shape[0]] = rows
    return buf[:rows.shape[0]] if x.dim() > 1 else buf[:rows.shape[0], 0]


def _nan_out(n_rows, cols):
    buf = torch.full((n_rows + GUARD, cols), float("nan"), device="cuda")
    return buf, buf[:n_rows]


def _int_out(n):
    buf = torch.full((n + GUARD,), -7, device="cuda", dtype=torch.int32)
    return buf, buf[:n]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _check(kernel, case, what, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = (err / bound).max().item()
    _REPORT.setdefault(case, {})[what] = round(ratio, 4)
    w = _REPORT["worst"]
    w[kernel + " " + what] = max(w.get(kernel + " " + what, 0.0), round(ratio, 4))
    assert torch.isfinite(got).all() and (err <= bound).all(), f"{case} {what}: |err| is {ratio:.3f} x its bound"


@pytest.fixture(autouse=True)
def _report():
    yield
    write_report("head_kernels.json", _REPORT)


# ------------------------------------------------------------------------------------------------ cosine_head
def _head(img, txt, scale, want_probs=True, want_aml=True, want_amp=True):
    """One launch; -> (logits, probs, am_logits, am_probs), None for what was not asked for.  Guards checked."""
    native, lib = _lib()
    n, c, e = img.shape[0], txt.shape[0], img.shape[1]
    lbuf, logits = _nan_out(n, c)
    pbuf, probs = _nan_out(n, c)
    abuf, aml = _int_out(n)
    bbuf, amp = _int_out(n)
    sbuf, scratch = _nan_out(c, e)
    native.check(lib.grip_cosine_head(_p(img), _p(txt), scale, n, c, e, _p(logits), _p(probs if want_probs else None), _p(aml if want_aml else None),
                                      _p(amp if want_amp else None), _p(scratch), _stream()))
    assert torch.isfinite(logits).all() and torch.isnan(lbuf[n:]).all() and torch.isnan(sbuf[c:]).all(), "logits / scratch: owned row not written or guard row written"
    assert (torch.isfinite(probs).all() if want_probs else torch.isnan(probs).all()) and torch.isnan(pbuf[n:]).all(), "probs: written although NULL, or a guard row written"
    for want, buf, name in ((want_aml, abuf, "am_logits"), (want_amp, bbuf, "am_probs")):
        assert (buf[n:] == -7).all() and (want or (buf == -7).all()), f"{name}: written although NULL, or a guard element written"
    return logits, probs if want_probs else None, aml if want_aml else None, amp if want_amp else None


@pytest.mark.parametrize("n,c,e,scale", HR.HEAD_CASES)
def test_cosine_head(n, c, e, scale):
    """Both forms (16 waves per row: n <= 64 and e <= 1024; 4 waves otherwise), every n, c, e of HR.HEAD_CASES, scale 1 and 100."""
    img, txt = HR.head_inputs(n, c, e, HR.head_case_seed(n, c, e), device="cuda")
    img, txt = _padded(img), _padded(txt)
    (lg, e_lg), (p, e_p) = HR.cosine_head(img, txt, scale)
    form = 16 if (n <= 64 and e <= 1024) else 4
    case = f"head.n{n}.c{c}.e{e}.scale{scale:g}.waves{form}"
    logits, probs, aml, amp = _head(img, txt, scale)
    _check(f"cosine_head_kernel<{form}>", case, "logits", logits, lg, e_lg)
    _check(f"cosine_head_kernel<{form}>", case, "probs", probs, p, e_p)
    srow = (probs.double().sum(-1) - 1).abs()
    assert (srow <= e_p.sum(-1)).all(), f"{case}: a probs row does not sum to 1 within its bound"
    # exact: the arg-maxes are the first-index arg-max of the kernel's own outputs
    assert torch.equal(aml.long(), HR.first_argmax(logits)) and torch.equal(amp.long(), HR.first_argmax(probs)), f"{case}: not the first-index arg-max of its own output"
    # against float64 on every row with a clear winner
    for name, got, ref, bound in (("logits", aml, lg, e_lg), ("probs", amp, p, e_p)):
        share, clear = HR.excluded_share(ref, bound)
        _REPORT[case][f"rows left out of the {name} arg-max comparison"] = share
        assert share <= 0.01, f"{case}: {share:.3f} of the rows have no clear float64 winner"
        assert torch.equal(got.long()[clear], ref.argmax(-1)[clear]), f"{case}: arg-max of {name} differs from float64 on a row with a clear winner"
    # every NULL combination: what is written has the bits of the full launch
    for wp in (False, True):
        for wl in (False, True):
            for wa in (False, True):
                l2, p2, a2, b2 = _head(img, txt, scale, wp, wl, wa)
                assert _same_bits(l2, logits) and (not wp or _same_bits(p2, probs)) and (not wl or torch.equal(a2, aml)) and (not wa or torch.equal(b2, amp)), \
                    f"{case}: probs={wp} am_logits={wl} am_probs={wa} differs from the full launch"


@pytest.mark.parametrize("c,e", [(102, 512), (5, 260), (1024, 1024)])
def test_cosine_head_forms_agree_in_bits(c, e):
    """The source's claim: a class's logit is computed by one wave in the same order whatever the form.  Rows 0 .. 63 of an n = 65 launch (4 waves per row) against the
    n = 64 launch (16 waves per row) on the same buffers."""
    img, txt = HR.head_inputs(65, c, e, 5, device="cuda")
    img, txt = _padded(img), _padded(txt)
    a = _head(img, txt, 100.0)
    b = _head(img[:64], txt, 100.0)
    assert _same_bits(a[0][:64], b[0]) and _same_bits(a[1][:64], b[1]), "logits / probs of the two forms differ in bits"
    assert torch.equal(a[2][:64], b[2]) and torch.equal(a[3][:64], b[3]), "arg-maxes of the two forms differ"
    _REPORT.setdefault(f"head.forms.c{c}.e{e}", {})["exact"] = 0.0


@pytest.mark.parametrize("n,e", [(3, 512), (65, 512), (2, 2048)])
def test_cosine_head_ties_go_to_the_lowest_index(n, e):
    """Duplicated text rows give equal bits at (j, j + 1) (one wave, two of its four dot products), (j, j + 4) (two waves) and (j, j + 64) (one lane, two of its
    classes); the image rows lean on one of the duplicated rows, so the maximum itself is tied."""
    c = 102
    img, txt = HR.head_inputs(n, c, e, 9, device="cuda")
    pairs = ((10, 11), (30, 34), (20, 84))
    for j, k in pairs:
        txt[k] = txt[j]
    for r in range(n):
        img[r] = txt[pairs[r % 3][0]] * 1.5 + 0.05 * img[r]
    img, txt = _padded(img), _padded(txt)
    logits, probs, aml, amp = _head(img, txt, 100.0)
    for j, k in pairs:
        assert _same_bits(logits[:, j], logits[:, k]) and _same_bits(probs[:, j], probs[:, k]), f"duplicated text rows {j}, {k} do not give equal bits"
    want = torch.tensor([pairs[r % 3][0] for r in range(n)], device="cuda")
    assert torch.equal(aml.long(), want) and torch.equal(amp.long(), want), (aml, amp, want)
    assert torch.equal(aml.long(), HR.first_argmax(logits)) and torch.equal(amp.long(), HR.first_argmax(probs))


# ------------------------------------------------------------------------------------------------ cosine_head_backward
@pytest.mark.parametrize("n,c,e", [(1, 1, 4), (2, 9, 260), (4, 2, 512), (5, 16, 2048), (8, 5, 4), (9, 47, 260), (16, 8, 512), (47, 4, 2048), (3, 6, 260), (6, 3, 512),
                                   (16, 47, 512)])
def test_cosine_head_backward(n, c, e):
    """n_other (c for grad_img, n for grad_txt) takes every residue mod 8 (3 and 6 through the added sizes 3 and 6), including the `two == false` tail of a wave's
    last trip; grad_logits from a real softmax - one-hot; the text side reads it transposed with ld_dl = c."""
    native, lib = _lib()
    scale = 100.0 if (n + c) % 2 else 1.0
    img, txt = HR.head_inputs(n, c, e, n + c + e, device="cuda")
    (_, _), (p, _) = HR.cosine_head(img, txt, scale)
    dl = ((p - torch.nn.functional.one_hot(torch.arange(n, device="cuda") % c, c)) / n).float()
    img, txt, dl = _padded(img), _padded(txt), _padded(dl)
    gi, e_gi = HR.cosine_head_bwd(img, txt, scale, dl)
    gt, e_gt = HR.cosine_head_bwd(txt, img, scale, dl.T)
    case = f"head_bwd.n{n}.c{c}.e{e}.scale{scale:g}"
    out = {}
    for mode in ("both", "img", "txt"):
        ibuf, gimg = _nan_out(n, e)
        tbuf, gtxt = _nan_out(c, e)
        native.check(lib.grip_cosine_head_backward(_p(img), _p(txt), scale, n, c, e, _p(dl), _p(gimg if mode != "txt" else None), _p(gtxt if mode != "img" else None),
                                                   _stream()))
        assert torch.isnan(ibuf[n:]).all() and torch.isnan(tbuf[c:]).all(), f"{case} {mode}: a guard row was written"
        assert torch.isnan(gimg).all() if mode == "txt" else torch.isfinite(gimg).all(), f"{case} {mode}: grad_img"
        assert torch.isnan(gtxt).all() if mode == "img" else torch.isfinite(gtxt).all(), f"{case} {mode}: grad_txt"
        out[mode] = (gimg, gtxt)
    _check("cosine_head_bwd_kernel", case, "grad_img", out["both"][0], gi, e_gi)
    _check("cosine_head_bwd_kernel", case, "grad_txt", out["both"][1], gt, e_gt)
    assert _same_bits(out["img"][0], out["both"][0]) and _same_bits(out["txt"][1], out["both"][1]), f"{case}: one gradient alone differs in bits from both together"


# ------------------------------------------------------------------------------------------------ weighted_ce
def _ce(x, lab, w, want_grad=True):
    native, lib = _lib()
    n, c = x.shape
    lbuf = torch.full((1 + GUARD,), float("nan"), device="cuda")
    gbuf, grad = _nan_out(n, c)
    native.check(lib.grip_weighted_ce(_p(x), _p(lab), _p(w), n, c, _p(lbuf), _p(grad if want_grad else None), _stream()))
    assert torch.isfinite(lbuf[0]) and torch.isnan(lbuf[1:]).all() and torch.isnan(gbuf[n:]).all(), "loss not written, or a guard element written"
    assert torch.isfinite(grad).all() if want_grad else torch.isnan(grad).all(), "grad: not written, or written although NULL"
    return lbuf[0], grad


@pytest.mark.parametrize("c", [1, 5, 64, 65, 102, 1000])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 64])
def test_weighted_ce(n, c):
    for spread in (1.0, 30.0):
        g = torch.Generator().manual_seed(n + c)
        x = _padded((spread * torch.randn(n, c, generator=g)).float())
        lab = torch.randint(0, c, (n,), generator=g).int()
        w = (torch.rand(n, generator=g) * (torch.arange(n) % 3 != 1)).float()              # every third row has weight zero (n = 1: none)
        for kind in ("plain", "label -1", "label c", "all weights zero"):
            lab_k, w_k = lab.clone(), w.clone()
            if kind == "label -1":
                lab_k[0] = -1
            if kind == "label c":
                lab_k[n - 1] = c
            if kind == "all weights zero":
                w_k.zero_()
            if kind != "all weights zero" and n > 1:
                w_k[0] = max(w_k[0].item(), 0.25)                                         # the row with the out-of-range label has a weight
            labd, wd = _padded(lab_k), _padded(w_k)
            (loss, e_loss), (grad, e_grad) = HR.weighted_ce(x, labd, wd)
            case = f"ce.n{n}.c{c}.spread{spread:g}.{kind}"
            got_loss, got_grad = _ce(x, labd, wd)
            if kind == "all weights zero":
                assert got_loss.item() == 0.0 and (got_grad == 0).all(), f"{case}: loss {got_loss.item()}"
                continue
            _check("weighted_ce_kernel", case, "loss", got_loss.reshape(1), loss.reshape(1), e_loss.reshape(1) + HR.TINY)
            _check("weighted_ce_kernel", case, "grad", got_grad, grad, e_grad)
            loss2, _ = _ce(x, labd, wd, want_grad=False)
            assert loss2.item() == got_loss.item(), f"{case}: the loss depends on grad being NULL"
            if kind in ("label -1", "label c"):                                           # the documented behaviour: the row is left out of the loss, no one-hot subtracted
                r = 0 if kind == "label -1" else n - 1
                assert (got_grad[r] >= 0).all() and abs(got_grad[r].double().sum().item() - wd[r].item()) <= e_grad[r].sum().item(), f"{case}: row {r} is not w softmax"
