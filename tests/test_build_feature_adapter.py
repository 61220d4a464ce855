"""Build-time guard for the feature adapter (csrc/feature_adapter.hip): it compiles for gfx950 and hipcc's resource remarks show no scratch
(register spills) for any kernel in it -- the forward is instantiated per accumulator count, and the widest (h = 256: 16 accumulators, eight staged
16-byte pieces of W1 per thread) is where a spill would appear first."""
import shutil

import pytest

from test_build_resources import HIPCC, _resources


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_feature_adapter_kernels_compile_without_scratch():
    res = _resources("feature_adapter.hip")
    fwd = [k for k in res if "fa_fwd_kernel" in k]
    bwd = [k for k in res if "fa_bwd_" in k]
    assert len(fwd) == 5 and len(bwd) == 2, sorted(res)
    for k in fwd + bwd:
        assert res[k].get("ScratchSize [bytes/lane]", 0) == 0, (k, res[k])
    assert len([k for k in res if "ScratchSize [bytes/lane]" in res[k]]) == len(res) == 7      # every kernel of the file reported
