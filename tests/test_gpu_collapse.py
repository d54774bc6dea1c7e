"""The least-cost 6-wide collapse (platinum_amd/csrc/pt_collapse.h, lbvh.hip) on the device, against the brute-force oracle and against the area
rule it replaces ($PTAMD_COLLAPSE_AREA=1, in the same process).  The scenes and references are those of tests/test_gpu_bvh_builder.py
(tests/bvh_layouts.py, tests/bvh_cases.py): every leaf slot is individually visible, so a slot the collapse lost or duplicated shows.

Sizes: a root with fewer children than its width (2 ... 9), 13 and 31, one leaf more than a full 6-wide tree of two and three levels (37, 217), 257,
kPlocTail = 1 024 (the single-block tail fills every row of the cost table), 1 025 (the device-driven passes fill the first rows, the tail reads them)
and 4 097.  Layouts: `scatter`, which builds 6-wide at every size, and `coincident` (identical boxes: every cost ties)."""
import numpy as np
import pytest

from platinum_amd import abi, scenes

import bvh_cases as C
import bvh_layouts as L   # noqa: F401  (the scenes behind bvh_cases)
from conftest import skip_if_structure_env_preset
from test_gpu_bvh_builder import STACK, _run_case

pytestmark = pytest.mark.gpu

SLOTS = (2, 3, 4, 5, 6, 7, 8, 9, 13, 31, 37, 217, 257, 1024, 1025, 4097)


def _ceil_div(a, b):
    return -(-a // b)


@pytest.mark.parametrize("layout", ["scatter", "coincident"])
@pytest.mark.parametrize("n", SLOTS)
def test_least_cost_collapse_sizes(gpu_renderer, monkeypatch, n, layout):
    """tracePrimary of samples 0-3 and debugSample(0) equal the brute-force oracle's bit for bit (_run_case); the tree has the same leaf slots as
    the area rule's, no more nodes than it, between ceil((L - 1) / 5) and L - 1 of them, and fits the traversal stack."""
    skip_if_structure_env_preset()
    monkeypatch.delenv("PTAMD_COLLAPSE_AREA", raising=False)
    st, sc = _run_case(gpu_renderer, n, layout)
    new = (st.leaf_slots, st.bvh_nodes, st.bvh_max_depth)
    monkeypatch.setenv("PTAMD_COLLAPSE_AREA", "1")
    gpu_renderer.startRender(sc, L.build(n, layout)[1:3], 1, max_bounces=2)
    sa = gpu_renderer.stats()
    area = (sa.leaf_slots, sa.bvh_nodes, sa.bvh_max_depth)
    print("n %d %s: least cost (slots, nodes, levels) %s, area rule %s" % (n, layout, new, area))
    slots = new[0]
    assert slots == area[0] and slots in (n, sc.triangle_count)   # (the triangle count under $PTAMD_NO_PAIRS)
    assert new[1] <= area[1], (new, area)
    assert _ceil_div(slots - 1, 5) <= new[1] <= slots - 1, (new, slots)
    assert 1 <= new[2] and new[2] * 5 <= STACK, new
    assert area[2] * 5 <= STACK, area


def test_least_cost_collapse_renders_the_same_image_with_no_more_node_visits(gpu_renderer, monkeypatch):
    """field_scene(grid=4), 96x54, 2 spp, 4 bounces under both collapses: the accumulators are bit-identical (the answer does not depend on the
    structure) and a closest-hit ray visits no more nodes in the least-cost tree (pt_measure_traversal's exact counts)."""
    skip_if_structure_env_preset()
    sc = scenes.field_scene(grid=4)
    got = {}
    for rule in ("cost", "area"):
        if rule == "area":
            monkeypatch.setenv("PTAMD_COLLAPSE_AREA", "1")
        else:
            monkeypatch.delenv("PTAMD_COLLAPSE_AREA", raising=False)
        gpu_renderer.selectKernel(abi.INTEGRATOR_MIS)
        gpu_renderer.startRender(sc, (96, 54), 2, max_bounces=4)
        gpu_renderer.render(0)
        acc = gpu_renderer.readbackAccumulator().copy()
        gpu_renderer.measureTraversal(0)
        st = gpu_renderer.stats()
        got[rule] = (acc, st.nodes_per_closest_ray, st.bvh_nodes, st.leaf_slots)
        print("%s: %d nodes over %d slots, %d levels; per closest-hit ray %.4f nodes, %.4f triangle tests; per shadow ray %.4f, %.4f" % (
            rule, st.bvh_nodes, st.leaf_slots, st.bvh_max_depth, st.nodes_per_closest_ray, st.tris_per_closest_ray, st.nodes_per_shadow_ray,
            st.tris_per_shadow_ray))
    assert got["cost"][0].tobytes() == got["area"][0].tobytes()
    assert np.isfinite(got["cost"][0]).all()
    assert got["cost"][3] == got["area"][3]
    assert got["cost"][2] <= got["area"][2]
    assert 0 < got["cost"][1] <= got["area"][1], (got["cost"][1], got["area"][1])
