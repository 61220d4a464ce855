"""Build-time guard for the linear probe kernels (csrc/linear_probe.hip): the file compiles for gfx950, hipcc's resource remarks show no scratch
(register spills) for any kernel in it -- the score kernel carries eight MFMA accumulators (four class tiles x two sixteens) and nine staged operand
vectors, the contraction eight accumulators -- and the score kernel, whose main loop hides its global loads behind MFMAs, keeps the two waves per SIMD
that DESIGN 21.3 states (its LDS is dynamic: at c <= 128 it leaves room for two workgroups per CU as well)."""
import shutil

import pytest

from test_build_resources import HIPCC, _resources

KERNELS = ("probe_score_kernel", "probe_contract_kernel", "probe_final_kernel", "probe_update_kernel")


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_probe_kernels_compile_without_scratch():
    res = _resources("linear_probe.hip")
    for name in KERNELS:
        assert len([k for k in res if name + "E" in k]) == 1, sorted(res)
    for k, v in res.items():
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
    assert len([k for k in res if "ScratchSize [bytes/lane]" in res[k]]) == len(res) == len(KERNELS)      # every kernel of the file reported
    score = [v for k, v in res.items() if "probe_score_kernel" in k][0]
    assert score["Occupancy [waves/SIMD]"] == 2, score      # 148 VGPRs + 32 AGPRs
    contract = [v for k, v in res.items() if "probe_contract_kernel" in k][0]
    assert contract["Occupancy [waves/SIMD]"] >= 4, contract
