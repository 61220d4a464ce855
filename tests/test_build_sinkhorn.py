"""Build-time guard for the balanced-assignment kernels (csrc/sinkhorn.hip): the file compiles for gfx950, every kernel of it reports its resources and
hipcc's remarks show no scratch (register spills) for any of them -- the register forms of the pass kernel hold a whole chunk of rows (16 x 2 values)
and must keep them in registers: an array the compiler indexed dynamically would show here as scratch."""
import shutil

import pytest

from test_build_resources import HIPCC, _resources

KERNELS = ("sk_pass_any_kernel", "sk_final_kernel")
PASSES = 2      # sk_pass_kernel<1>, <2> (classes in registers)


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_sinkhorn_kernels_compile_without_scratch():
    res = _resources("sinkhorn.hip")
    for name in KERNELS:
        assert len([k for k in res if name in k]) == 1, sorted(res)
    assert len([k for k in res if "sk_pass_kernel" in k]) == PASSES, sorted(res)
    for k, v in res.items():
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
    assert len([k for k in res if "ScratchSize [bytes/lane]" in res[k]]) == len(res) == len(KERNELS) + PASSES      # every kernel of the file reported
    for k, v in res.items():
        if "sk_pass" in k:
            assert v["Occupancy [waves/SIMD]"] >= 4, (k, v)      # a streaming kernel: latency is hidden by waves, not by a pipeline
