"""Build-time guard for the Gaussian discriminant head kernels (csrc/gda_head.hip): the file compiles for gfx950, hipcc's resource remarks show no
scratch (register spills) for any kernel in it -- the scatter kernel carries four MFMA accumulators, the panel kernel a 4 x 4 register tile and three
64 x 64 LDS blocks, the head kernel four accumulators and two staged operand pairs -- and the head kernel leaves room for at least two workgroups per
CU."""
import shutil

import pytest

from test_build_resources import HIPCC, _resources

KERNELS = ("gda_scatter_kernel", "gda_scatter_final_kernel", "gda_form_kernel", "gda_panel_kernel", "gda_back_kernel", "gda_factor_copy_kernel",
           "gda_head_kernel")


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_gda_kernels_compile_without_scratch():
    res = _resources("gda_head.hip")
    for name in KERNELS:
        assert len([k for k in res if name + "E" in k]) == 1, sorted(res)
    for k, v in res.items():
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
    assert len([k for k in res if "ScratchSize [bytes/lane]" in res[k]]) == len(res) == len(KERNELS)      # every kernel of the file reported
    head = [v for k, v in res.items() if "gda_head_kernel" in k][0]
    assert head["Occupancy [waves/SIMD]"] >= 2, head      # 4 waves per workgroup, one per SIMD: >= 2 workgroups per CU
