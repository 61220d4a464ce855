"""Build-time guard for the transductive GMM kernels (csrc/gmm_transduce.hip): the file compiles for gfx950, hipcc's resource remarks show no scratch
(register spills) for any kernel in it -- the sums kernel carries eight MFMA accumulators, the variance kernel eight centres of four columns, the scores
kernel four accumulators and two staged operand pairs -- and the scores kernel leaves room for at least two workgroups per CU."""
import shutil

import pytest

from test_build_resources import HIPCC, _resources

KERNELS = ("gmm_sum_kernel", "gmm_mean_kernel", "gmm_var_kernel", "gmm_var_final_kernel", "gmm_prep_kernel", "gmm_score_kernel")
SWEEPS = 3      # gmm_sweep_kernel<1>, <2> (classes in registers) and <0> (any number of classes)


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_gmm_kernels_compile_without_scratch():
    res = _resources("gmm_transduce.hip")
    for name in KERNELS:
        assert len([k for k in res if name in k]) == 1, sorted(res)
    assert len([k for k in res if "gmm_sweep_kernel" in k]) == SWEEPS, sorted(res)
    for k, v in res.items():
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
    assert len([k for k in res if "ScratchSize [bytes/lane]" in res[k]]) == len(res) == len(KERNELS) + SWEEPS      # every kernel of the file reported
    score = [v for k, v in res.items() if "gmm_score_kernel" in k][0]
    assert score["Occupancy [waves/SIMD]"] >= 2, score      # 4 waves per workgroup, one per SIMD: >= 2 workgroups per CU
