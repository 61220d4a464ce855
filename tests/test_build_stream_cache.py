"""Build-time guard for the streaming cache (csrc/stream_cache.hip): the file compiles for gfx950 and every kernel of it reports no scratch; the built
library exports the four symbols of include/grip_amd.h, the host layer declares them, the _workspace calls answer without a device, and every
out-of-range argument is refused with GRIP_ERR_ARG before anything is launched or written."""
import ctypes
import os
import re
import shutil

import pytest

from test_build_resources import HIPCC, _resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("sc_row_kernel", "sc_scan_kernel", "sc_compact_kernel", "sc_rnorm_kernel", "sc_head_kernel", "sc_finish_kernel")
SYMBOLS = ("grip_stream_cache_plan_workspace", "grip_stream_cache_plan", "grip_stream_cache_head_workspace", "grip_stream_cache_head")


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_stream_cache_kernels_compile_without_scratch():
    res = _resources("stream_cache.hip")
    for name in KERNELS:
        assert len([k for k in res if name + "E" in k]) == 1, sorted(res)
    for k, v in res.items():
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
    assert len(res) == len(KERNELS)


def _lib():
    import grip_amd  # noqa: F401
    from grip_amd import native
    return native, native.lib()


def test_the_library_exports_the_symbols_and_the_header_declares_them():
    native, lib = _lib()
    header = open(os.path.join(ROOT, "include", "grip_amd.h")).read()
    for s in SYMBOLS:
        assert s in native.EXPORTS and hasattr(lib, s) and re.search(rf"\bint {s}\(", header), s
    assert "(ABI 9 additions) Test-time streaming cache" in header and "NOT THE PAPER'S CODE" in header


def test_the_workspace_calls_need_no_device_and_bad_arguments_are_refused():
    native, lib = _lib()
    header = open(os.path.join(ROOT, "include", "grip_amd.h")).read()
    ERR_ARG = int(re.search(r"\bGRIP_ERR_ARG\s*=\s*(\d+)", header).group(1))
    nbytes = ctypes.c_size_t(12345)
    assert lib.grip_stream_cache_plan_workspace(10000, 102, ctypes.byref(nbytes)) == 0 and nbytes.value == 0
    assert lib.grip_stream_cache_head_workspace(10000, 102, 512, ctypes.byref(nbytes)) == 0
    assert nbytes.value >= 10000 * 4 + 2 * 10000 * 102 * 4
    for args in ((0, 102), (10, 0), ((1 << 30) + 1, 4)):
        assert lib.grip_stream_cache_plan_workspace(*args, ctypes.byref(nbytes)) == ERR_ARG, args
    for args in ((0, 102, 512), (10, 0, 512), (10, 102, 0), (10, 102, 510), (10, 102, 1028)):
        assert lib.grip_stream_cache_head_workspace(*args, ctypes.byref(nbytes)) == ERR_ARG, args
    assert lib.grip_stream_cache_plan_workspace(10, 10, None) == ERR_ARG
    # the launching calls: host buffers stand in for device memory -- a refused call touches none of them
    n, c, e = 8, 5, 16
    f32 = lambda k: (ctypes.c_float * k)(*([7.0] * k))
    i32 = lambda k: (ctypes.c_int32 * k)(*([-7] * k))
    x, feats, out, H = f32(n * c), f32(n * e), f32(n * c), f32(n)
    ints = {k: i32(n) for k in ("pred", "pos_leave", "neg_leave", "negbits", "pos_key", "neg_key")}
    counts, ws = i32(2), (ctypes.c_char * 4096)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)

    def plan(n=n, c=c, pos_cap=3, neg_cap=2, ent=(0.2, 0.5), mask=(0.03, 1.0), x=x, counts=counts):
        return lib.grip_stream_cache_plan(p(x), n, c, pos_cap, neg_cap, ent[0], ent[1], mask[0], mask[1], p(H), p(ints["pred"]), p(ints["pos_leave"]),
                                          p(ints["neg_leave"]), p(ints["negbits"]), p(ints["pos_key"]), p(ints["neg_key"]), p(counts) if counts else None,
                                          None, 0, None)

    def head(n=n, c=c, e=e, alpha=2.0, beta=5.0, feats=feats, negbits=ints["negbits"], ws_bytes=4096, out=out):
        return lib.grip_stream_cache_head(p(x), p(feats) if feats else None, p(ints["pred"]), p(negbits) if negbits else None, p(ints["pos_leave"]),
                                          p(ints["neg_leave"]), p(ints["pos_key"]), p(ints["neg_key"]), p(counts), alpha, beta, 0.117, 1.0, n, c, e,
                                          p(out) if out else None, p(ws), ws_bytes, None)
    inf, nan = float("inf"), float("nan")
    refused = [plan(n=0), plan(c=0), plan(pos_cap=0), plan(pos_cap=17), plan(neg_cap=-1), plan(neg_cap=17), plan(ent=(0.5, 0.2)), plan(ent=(nan, 0.5)),
               plan(mask=(0.0, inf)), plan(mask=(0.5, 0.1)), plan(x=None), plan(counts=None),
               head(n=0), head(c=0), head(e=0), head(e=18), head(e=1028), head(alpha=nan), head(beta=inf), head(feats=None), head(out=None),
               head(negbits=None), head(ws_bytes=64)]
    assert refused == [ERR_ARG] * len(refused), refused
    assert b"workspace too small" in lib.grip_last_error()
    assert list(out) == [7.0] * (n * c) and list(H) == [7.0] * n and list(counts) == [-7, -7] and all(list(v) == [-7] * n for v in ints.values())
