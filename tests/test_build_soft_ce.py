"""Build-time guard for the soft-target cross-entropy kernel (csrc/soft_ce.hip): the file compiles for gfx950, every kernel of it reports its resources and
hipcc's remarks show no scratch (register spills) for any of them -- the contract of grip_soft_ce says "no scratch", and the only state the rows share is
the inverse column map in the LDS."""
import shutil

import pytest

from test_build_resources import HIPCC, _resources

KERNELS = ("soft_ce_kernel",)


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_soft_ce_kernels_compile_without_scratch():
    res = _resources("soft_ce.hip")
    for name in KERNELS:
        assert len([k for k in res if name in k]) == 1, sorted(res)
    for k, v in res.items():
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
    assert len([k for k in res if "ScratchSize [bytes/lane]" in res[k]]) == len(res) == len(KERNELS)      # every kernel of the file reported
