"""Build-time guard for the label-propagation kernels (csrc/knn_graph.hip): the file compiles for gfx950 and hipcc's resource remarks show no scratch
(register spills) for any kernel in it -- the graph kernel carries four accumulators, two staged operand pairs and the 16 scores of the selection
epilogue (fully unrolled: an indexed register array is where a spill would appear first) -- and its LDS leaves room for two workgroups per CU."""
import shutil

import pytest

from test_build_resources import HIPCC, _resources

KERNELS = ("knn_rnorm_kernel", "knn_graph_kernel", "knn_merge_kernel", "lp_weight_kernel", "lp_step_kernel")


@pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not installed")
def test_knn_graph_kernels_compile_without_scratch():
    res = _resources("knn_graph.hip")
    for name in KERNELS:
        assert len([k for k in res if name in k]) == 1, sorted(res)
    for k, v in res.items():
        assert v.get("ScratchSize [bytes/lane]", 0) == 0, (k, v)
    assert len([k for k in res if "ScratchSize [bytes/lane]" in res[k]]) == len(res) == len(KERNELS)      # every kernel of the file reported
    graph = [v for k, v in res.items() if "knn_graph_kernel" in k][0]
    assert graph["Occupancy [waves/SIMD]"] >= 2, graph      # 4 waves per workgroup, one per SIMD: >= 2 workgroups per CU
