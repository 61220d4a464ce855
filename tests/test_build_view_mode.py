"""Build-time guard for the multi-view mode kernel (csrc/view_mode.hip): the file compiles for gfx950, its one kernel reports its resources and hipcc's
remarks show no scratch (register spills) -- the contract of grip_view_mode says "no scratch"; the state between the sweeps (the two [V, V] matrices, the
bandwidths, the weights and the mode) is in the LDS, small enough for four workgroups per CU."""
import shutil

import pytest

from test_build_resources import HIPCC, _resources

KERNELS = {"view_mode_kernel": 1}


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_view_mode_kernel_compiles_without_scratch():
    res = _resources("view_mode.hip")
    for name, instances in KERNELS.items():
        assert len([k for k in res if name in k]) == instances, sorted(res)
    for k, v in res.items():
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
    assert len([k for k in res if "ScratchSize [bytes/lane]" in res[k]]) == len(res) == sum(KERNELS.values())      # every kernel of the file reported
    kernel = list(res.values())[0]
    assert kernel["Occupancy [waves/SIMD]"] >= 4, kernel      # its 37.5 KiB of LDS leave room for four workgroups in a CU's 160 KiB
