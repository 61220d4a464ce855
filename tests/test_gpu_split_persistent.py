"""The two-pass split-f16 GEMMs (weights that are f16 numbers: GemmArgs::w_exact) on the persistent f16 GEMM kernel.

An activation row in the split layout is one 128-byte line [32 hi | 32 lo] per 32 k: read as f16 it is A'[M, 2K], and against the weight image
W'[N, 2K] = [32 w | 32 w] the plain f16 GEMM A' W'^T issues the hi and the lo product of every fragment pair into one f32 accumulator
(csrc/gemm.hip, gemm_k64p_kernel<EPI, 3, true>; csrc/gemm_split.hip, launch_gemm_split).  Everything here goes through grip_debug_gemm_split
with W = W.half().float(); the reference is the float64 product of the same f32 inputs with the error measure and the tolerances of
tests/test_gpu_split.py: 4e-7 for the plain product, 5e-7 with bias / residual, 8e-7 through QuickGELU, against |a|.|w| plus the 3.1e-8 floor
of an unscaled lo part.

Shapes = the smallest at which this kernel can go wrong:
  (256, 256, 64)     K' = 128: two K steps, the pipeline's minimum -- the next tile's prefetch is issued at the only two stage boundaries
  (100, 768, 768)    three tiles (fewer than XCDs) in a 256-row pad whose padding rows hold NaN
  (257, 512, 128)    a second row panel holding one live row
  (6000, 3072, 128)  288 tiles: more than the CUs, so workgroups walk several tiles, unevenly split over the XCDs
  (1500, 768, 3072)  the long K walk"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(256, 256, 64), (100, 768, 768), (257, 512, 128), (6000, 3072, 128), (1500, 768, 3072)]
LO_SCALE = 1.0       # csrc/common.h GRIP_SPLIT_LO_SCALE


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native, native.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _unsplit(buf, rows, K):
    v = buf.view(torch.float16).reshape(rows, K // 32, 2, 32).double()
    return (v[:, :, 0] + v[:, :, 1] / LO_SCALE).reshape(rows, K)


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


@functools.lru_cache(maxsize=None)
def _problem(M, N, K):
    """Inputs and the float64 reference of one shape, computed once and shared (read-only) by every test of the shape."""
    g = torch.Generator(device="cuda").manual_seed(M * 13 + N + K)
    Mp = (M + 255) // 256 * 256
    A = torch.randn(Mp, K, device="cuda", generator=g)
    A[M:] = float("nan")       # padding rows must never reach a stored row
    A[:M] *= torch.exp(torch.randn(1, K, device="cuda", generator=g) * 0.7)      # heavy-tailed column scale, as LayerNorm outputs have
    W = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).half().float()
    bias = torch.randn(N, device="cuda", generator=g)
    resid = torch.randn(M, N, device="cuda", generator=g)
    ref = A[:M].double() @ W.double().t()
    mag = A[:M].double().abs() @ W.double().abs().t()
    floor = 3.1e-8 * W.double().abs().sum(1)[None, :]
    return dict(M=M, N=N, K=K, Mp=Mp, A=A, W=W, bias=bias, resid=resid, ref=ref, mag=mag, floor=floor)


def _run(pb, epi, out, bias=None, resid=None, A=None, M=None, Mp=None, W=None):
    native, lib = _lib()
    A = pb["A"] if A is None else A
    M = pb["M"] if M is None else M
    Mp = pb["Mp"] if Mp is None else Mp
    W = pb["W"] if W is None else W
    a_s = torch.empty(Mp * pb["K"], device="cuda")
    w_s = torch.empty(pb["N"] * pb["K"], device="cuda")
    native.check(lib.grip_debug_gemm_split(epi, _p(A), _p(W), M, pb["N"], pb["K"], _p(bias), _p(resid), _p(out), _p(a_s), _p(w_s), Mp, _stream()))
    return lib.grip_debug_split_last_wlo(), w_s


def _worst(pb, got, want, extra):
    """max of (|got - want| - floor) / (error scale of the dot product + the magnitudes of what the epilogue adds)"""
    return (((got.double() - want).abs() - pb["floor"]).clamp_min(0) / (pb["mag"] + extra + want.abs())).max().item()


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_plain_product_against_float64(M, N, K):
    pb = _problem(M, N, K)
    out = torch.full((M, N), 7.0, device="cuda")
    wlo, w_s = _run(pb, 0, out)
    assert wlo == 0                                                  # the two-pass form ran
    v = w_s.view(torch.float16).reshape(N, K // 32, 2, 32)
    assert (v[:, :, 1] == 0).all()                                   # the caller's weight image stays in the standard layout
    err = (((out.double() - pb["ref"]).abs() - pb["floor"]).clamp_min(0) / pb["mag"]).max().item()
    print(f"M={M} N={N} K={K}: plain product max (|err| - floor) / (|a|.|w|) = {err:.2e}")
    assert torch.isfinite(out).all()
    assert err <= 4e-7, err
    out2 = torch.full((M, N), -3.0, device="cuda")                   # two identical launches: equal bits
    _run(pb, 0, out2)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_bias_epilogue_against_float64(M, N, K):
    pb = _problem(M, N, K)
    out = torch.full((M, N), 7.0, device="cuda")
    assert _run(pb, 1, out, bias=pb["bias"])[0] == 0
    b = pb["bias"].double()
    err = _worst(pb, out, pb["ref"] + b, b.abs())
    print(f"M={M} N={N} K={K}: bias epilogue {err:.2e}")
    assert err <= 5e-7, err


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_residual_epilogue_against_float64_in_and_out_of_place(M, N, K):
    pb = _problem(M, N, K)
    out = torch.full((M, N), 7.0, device="cuda")
    assert _run(pb, 3, out, bias=pb["bias"], resid=pb["resid"])[0] == 0
    b, r = pb["bias"].double(), pb["resid"].double()
    err = _worst(pb, out, pb["ref"] + b + r, b.abs() + r.abs())
    print(f"M={M} N={N} K={K}: residual epilogue {err:.2e}")
    assert err <= 5e-7, err
    r2 = pb["resid"].clone()             # in place (out aliases resid), as the tower uses it
    _run(pb, 3, r2, bias=pb["bias"], resid=r2)
    assert torch.equal(r2, out)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gelu_epilogue_writes_the_split_layout(M, N, K):
    pb = _problem(M, N, K)
    h = torch.zeros(M * N, device="cuda")
    assert _run(pb, 2, h, bias=pb["bias"])[0] == 0
    b = pb["bias"].double()
    err = _worst(pb, _unsplit(h, M, N), quick_gelu(pb["ref"] + b), b.abs() + 0.1)
    print(f"M={M} N={N} K={K}: QuickGELU epilogue {err:.2e}")
    assert err <= 8e-7, err


def test_a_rows_bits_do_not_depend_on_the_launch():
    """Rows 700..799 of the M = 1500 launch, the same rows as a 100-row launch, and the same rows placed inside a 6000-row launch (the
    refinement re-encodes gathered, arbitrarily chunked rows); likewise a slice of the 288-tile launch, whose workgroups walk several tiles."""
    pb = _problem(1500, 768, 3072)
    N, K = pb["N"], pb["K"]
    out = torch.empty(1500, N, device="cuda")
    _run(pb, 0, out)
    sub = torch.zeros(256, K, device="cuda")
    sub[:100] = pb["A"][700:800]
    o100 = torch.empty(100, N, device="cuda")
    _run(pb, 0, o100, A=sub, M=100, Mp=256)
    assert torch.equal(o100, out[700:800])
    g = torch.Generator(device="cuda").manual_seed(3)
    big = torch.randn(6144, K, device="cuda", generator=g)
    big[5003:5103] = pb["A"][700:800]
    big[6000:] = float("nan")
    o6000 = torch.empty(6000, N, device="cuda")
    _run(pb, 0, o6000, A=big, M=6000, Mp=6144)
    assert torch.equal(o6000[5003:5103], out[700:800])
    for epi in (1, 3):       # the epilogues that carry a bias / a residual: the same, through the 100-row launch
        full = torch.empty(1500, N, device="cuda")
        _run(pb, epi, full, bias=pb["bias"], resid=pb["resid"] if epi == 3 else None)
        part = torch.empty(100, N, device="cuda")
        _run(pb, epi, part, bias=pb["bias"], resid=pb["resid"][700:800].contiguous() if epi == 3 else None, A=sub, M=100, Mp=256)
        assert torch.equal(part, full[700:800])

    pw = _problem(6000, 3072, 128)       # 288 tiles on the device against 12
    wide = torch.empty(6000, 3072, device="cuda")
    _run(pw, 0, wide)
    subw = torch.zeros(256, 128, device="cuda")
    subw[:100] = pw["A"][700:800]
    ow = torch.empty(100, 3072, device="cuda")
    _run(pw, 0, ow, A=subw, M=100, Mp=256)
    assert torch.equal(ow, wide[700:800])


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_weights_off_the_f16_grid_take_the_three_pass_kernel(M, N, K):
    pb = _problem(M, N, K)
    W2 = pb["W"] * (1 + 2.0 ** -13)
    out = torch.empty(M, N, device="cuda")
    wlo, _ = _run(pb, 0, out, W=W2)
    assert wlo == 1
    ref2 = pb["A"][:M].double() @ W2.double().t()
    err = (((out.double() - ref2).abs() - pb["floor"]).clamp_min(0) / pb["mag"]).max().item()
    assert err <= 4e-7, err


def test_small_tower_on_an_fp16_checkpoint():
    """Model `small`, fp16_checkpoint=True: every block GEMM of the split twin runs the two-pass form; chunk 32 equals chunk 7 bit for bit and
    the embeddings stay within 5e-6 (relative L2) of the exact twin's."""
    import grip_amd  # noqa: F401
    from grip_amd import clip, pseudolabels as pl
    from grip_amd.data.synthetic import structured_images
    native, lib = _lib()
    m, _ = clip.load("small", device="cuda", fp16_checkpoint=True)
    twin, split = m.exact_twin(), m.split_twin()
    x = structured_images(77, 0, 96, 64).cuda()
    with torch.no_grad():
        e32 = pl.encode_pool(twin.visual.tower, x, chunk=32)
        es = pl.encode_pool(split.visual.tower, x, chunk=32)
        assert lib.grip_debug_split_last_wlo() == 0
        es7 = pl.encode_pool(split.visual.tower, x, chunk=7)
    assert torch.equal(es, es7)
    r_s = ((es - e32).norm(dim=1) / e32.norm(dim=1)).max().item()
    print(f"small, fp16 checkpoint: embedding rel L2 split vs exact twin {r_s:.2e}")
    assert r_s <= 5e-6, r_s
