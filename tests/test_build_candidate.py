"""Build-time guard for the candidate-set kernels (csrc/candidate.hip): the file compiles for gfx950, every kernel of it reports its resources and hipcc's
remarks show no scratch (register spills) for any of them -- the contracts of grip_candidate_select and grip_candidate_ce say "no scratch"; the only shared
state is the digit histogram of a column tile and the inverse column map, both in the LDS."""
import shutil

import pytest

from test_build_resources import HIPCC, _resources

KERNELS = {"cs_init_kernel": 1, "cs_hist_kernel": 1, "cs_pick_kernel": 1, "cs_row_kernel": 4, "candidate_ce_kernel": 1}      # cs_row_kernel: NP = 1, 2, 4 and 0


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_candidate_kernels_compile_without_scratch():
    res = _resources("candidate.hip")
    for name, instances in KERNELS.items():
        assert len([k for k in res if name in k]) == instances, sorted(res)
    for k, v in res.items():
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
    assert len([k for k in res if "ScratchSize [bytes/lane]" in res[k]]) == len(res) == sum(KERNELS.values())      # every kernel of the file reported
    hist = [v for k, v in res.items() if "cs_hist_kernel" in k][0]
    assert hist["Occupancy [waves/SIMD]"] >= 4, hist      # its 32 KiB of counters ([256 digits][32 columns]) leave room for 4+ workgroups in a CU's 160 KiB
