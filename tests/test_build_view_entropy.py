"""Build-time guard for the view-entropy kernels (csrc/view_entropy.hip): the file compiles for gfx950, every kernel of it reports its resources and
hipcc's remarks show no scratch (register spills) -- the contract of grip_view_entropy says "no scratch".  (That the static LDS leaves the 16 000 classes
of the contract their 64 000 bytes is shown by the launch at the class limit in tests/test_gpu_view_entropy_kernel.py.)"""
import shutil

import pytest

from test_build_resources import HIPCC, _resources

KERNELS = {"view_entropy_kernel": 1, "view_entropy_mean_kernel": 1, "view_entropy_recompute_kernel": 1}


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_view_entropy_kernels_compile_without_scratch():
    res = _resources("view_entropy.hip")
    for name, instances in KERNELS.items():
        assert len([k for k in res if name + "E" in k]) == instances, sorted(res)      # (the mangled name: its length prefix and the E keep the names apart)
    for k, v in res.items():
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
    assert len([k for k in res if "ScratchSize [bytes/lane]" in res[k]]) == len(res) == sum(KERNELS.values())      # every kernel of the file reported
