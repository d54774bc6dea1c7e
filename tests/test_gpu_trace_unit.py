"""k_trace_closest and k_trace_shadow live in a translation unit of their own (platinum_amd/csrc/trace_kernels.hip, built without SLP packing, the
closest-hit kernel at one block per CU more) over the ray loop of trace_loop.h.  Packed and scalar f32 instructions are the same IEEE
operations, so every answer must still be the oracle's BIT FOR BIT, at the smallest shapes that reach every path of the moved loop:

  Cornell box 32 x 32, 2 batches of 3 samples   lane refill from partly filled chunks, both trace kernels; MIS and the simple integrator
  the field scene 96 x 54, 64 samples, one batch   full chunks, lane replacement inside a chunk run
  the `expo` mosaic of 257 slots (tests/bvh_layouts.py: nested boxes, a chain-like tree of 19 6-wide levels)   the deepest tree a 6-wide walk takes
  the `coincident` mosaic of 4 097 slots, one pixel per cell   every box the same box: a stack that passes the kernel's LDS rows, so that
                                                 entries are pushed to and popped from the HBM slab behind them (sized by the largest grid)
each in the default 6-wide structure and under $PTAMD_BVH4 (the 4-wide instantiations are in the unit too).  The oracle's answers are computed
once per session and shared by both structures."""
import os
import re

import numpy as np
import pytest

from platinum_amd import abi, scenes
from platinum_amd.renderer import make_params

import bvh_cases as C
import bvh_layouts as L
import oracle_lib
from conftest import skip_if_structure_env_preset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = (257, "expo")
# name: (scene, width, height, spp, samples in flight, bounces)
RENDERS = {
    "cornell": (lambda: scenes.cornell_scene("bench"), 32, 32, 6, 3, 4),
    "field": (lambda: scenes.field_scene(8), 96, 54, 64, 64, 4),
}
_REF = {}


def _same_bits_or_both_nan(a, b):
    """Bitwise equality, except that NaNs only have to coincide: x86 and gfx950 produce default NaNs of opposite sign."""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def _reference(name, integrator):
    """(accumulator, ray counts) of the oracle for one render, once per session; read-only."""
    if (name, integrator) not in _REF:
        make, w, h, spp, _, bounces = RENDERS[name]
        o = oracle_lib.OracleScene(make(), make_params(w, h, spp, bounces, integrator=integrator))
        acc = o.render(0, spp)
        acc.flags.writeable = False
        so = o.stats()
        _REF[(name, integrator)] = (acc, (so.closest_rays, so.shadow_rays, so.shaded_hits, so.paths))
    return _REF[(name, integrator)]


def _structure(monkeypatch, bvh4):
    if bvh4:
        skip_if_structure_env_preset()
        monkeypatch.setenv("PTAMD_BVH4", "1")


@pytest.mark.parametrize("bvh4", [False, True], ids=["six_wide", "four_wide"])
@pytest.mark.parametrize("name,integrator", [("cornell", abi.INTEGRATOR_MIS), ("cornell", abi.INTEGRATOR_SIMPLE), ("field", abi.INTEGRATOR_MIS)])
def test_renders_are_the_oracles_bit_for_bit(gpu_renderer, monkeypatch, name, integrator, bvh4):
    r = gpu_renderer
    make, w, h, spp, sif, bounces = RENDERS[name]
    _structure(monkeypatch, bvh4)
    r.selectKernel(integrator)
    r.startRender(make(), (w, h), spp, max_bounces=bounces, samples_in_flight=sif)
    while r.status() & abi.STATUS_BUSY:
        r.render(1)
    acc = r.readbackAccumulator()
    assert r.renderProgress() == (spp, spp)
    ref, rays = _reference(name, integrator)
    assert _same_bits_or_both_nan(acc, ref), "accumulator differs at (y, x, c) %s" % np.argwhere(acc.view(np.uint32) != ref.view(np.uint32))[:5].tolist()
    st = r.stats()
    assert (st.closest_rays, st.shadow_rays, st.shaded_hits, st.paths) == rays
    if integrator == abi.INTEGRATOR_MIS:
        assert st.shadow_rays > 0   # the shadow kernel ran


DEEP = [4097]   # 8 levels 6-wide, 11 levels 4-wide: the smallest of the builder tests' sizes at which both walks pass their LDS rows


@pytest.mark.parametrize("bvh4", [False, True], ids=["six_wide", "four_wide"])
@pytest.mark.parametrize("n", DEEP)
def test_coincident_boxes_fill_the_stack_past_its_lds_rows(gpu_renderer, monkeypatch, n, bvh4):
    """n copies of one triangle over the whole image (`coincident`, one pixel per cell): every box is the same box, every ray enters every child
    of every node and no hit culls a sibling (all hits tie), so a lane's stack holds every sibling it has passed on the way down.  The lowest id wins
    every pixel.  That the walk popped every entry it pushed, the ones in the HBM slab included, shows in the counts of the instrumented camera
    rays (one bounce: they are the only closest-hit rays): every ray visits every node and tests every triangle.  (A library whose stack
    dropped what passed the LDS rows visited fewer: that is how these sizes were found to reach the slab.)"""
    r = gpu_renderer
    _structure(monkeypatch, bvh4)
    sc, W, H = L.mosaic(n, "coincident", cell_px=1)
    if ("deep", n) not in _REF:
        o = oracle_lib.OracleScene(sc, make_params(W, H, 1, 1), use_bvh=False)
        _REF[("deep", n)] = [o.trace_primary(s) for s in (0, 3)]
    r.selectKernel(abi.INTEGRATOR_MIS)
    r.startRender(sc, (W, H), 1, max_bounces=1)
    r.measureTraversal(0)
    st = r.stats()
    print("n %d: %d nodes, %d levels; per camera ray %.3f nodes, %.3f triangles" % (n, st.bvh_nodes, st.bvh_max_depth, st.nodes_per_closest_ray, st.tris_per_closest_ray))
    assert st.leaf_slots == n
    assert st.nodes_per_closest_ray == st.bvh_nodes and st.tris_per_closest_ray == n
    for s, c in zip((0, 3), _REF[("deep", n)]):
        g = r.tracePrimary(s)
        assert (c["instance"] == 0).all() and (c["primitive"] == 0).all()
        for k in ("instance", "primitive"):
            assert np.array_equal(g[k], c[k]), (s, k, np.argwhere(g[k] != c[k])[:4].tolist(), g[k][g[k] != c[k]][:4].tolist())
        for k in "tuv":
            assert np.array_equal(g[k].view(np.uint32), c[k].view(np.uint32)), (s, k)


def _define(src, name):
    m = re.search(r"^#define %s (\d+)\s*$" % name, src, re.M)
    assert m, name
    return int(m.group(1))


@pytest.mark.parametrize("bvh4", [False, True], ids=["six_wide", "four_wide"])
def test_a_chain_deeper_than_the_lds_stack_rows_gives_the_brute_force_hits(gpu_renderer, monkeypatch, bvh4):
    """Depths over fifteen decades make nested boxes: a camera ray's walk descends level after level with the siblings it passed still on its stack.
    levels * pushes per level exceeds the LDS rows of the walk (both read from pt_bvh.h): the stack MAY pass them.  Measured, it does not: a
    chain's nodes have one inner child each, the leaves go to the leaf queue, and a library whose stack dropped everything past the LDS rows
    still passed this test (19 levels 6-wide, 24 levels 4-wide).  The case stays for the deep tree; the test that does reach the HBM slab is
    test_coincident_boxes_fill_the_stack_past_its_lds_rows above."""
    r = gpu_renderer
    n, layout = CHAIN
    _structure(monkeypatch, bvh4)
    sc, W, H, ids, field = L.build(n, layout)
    ref = C.reference(n, layout)
    r.selectKernel(abi.INTEGRATOR_MIS)
    r.startRender(sc, (W, H), 1, max_bounces=2)
    st = r.stats()
    src = open(os.path.join(ROOT, "platinum_amd", "csrc", "pt_bvh.h")).read()
    walk = "Walk4" if bvh4 else "Walk6"
    body = re.search(r"^struct %s \{.*?^\};" % walk, src, re.M | re.S).group(0)
    pushes = int(re.search(r"kPushesPerLevel = (\d+)", body).group(1))
    rows = _define(src, "PT_LDS_STACK" if bvh4 else "PT_LDS_STACK6")
    assert re.search(r"kStackRows = %s\b" % ("kLdsStack" if bvh4 else "kLdsStack6"), body)
    if not any(v in os.environ for v in ("PTAMD_RADIX_TREE", "PTAMD_TWO_LEVEL", "PTAMD_TEST_W6_LEVELS", "PTAMD_BVH_LEGACY")) and (bvh4 or "PTAMD_BVH4" not in os.environ):
        print("%s: %d levels x %d pushes against %d LDS rows" % (walk, st.bvh_max_depth, pushes, rows))
        assert st.bvh_max_depth * pushes > rows, (st.bvh_max_depth, pushes, rows)
    for s, c in zip(L.SAMPLES, ref["primary"]):
        g = r.tracePrimary(s)
        for k in ("instance", "primitive"):
            assert np.array_equal(g[k], c[k]), (s, k, np.argwhere(g[k] != c[k])[:4].tolist())
        for k in "tuv":
            assert np.array_equal(g[k].view(np.uint32), c[k].view(np.uint32)), (s, k)
        assert len(L.missing_ids(g, ids, field)) == 0
    rg, hg = r.debugSample(0)   # ... and the shadow kernel over the same tree
    assert np.array_equal(hg, ref["hits"]) and _same_bits_or_both_nan(rg, ref["radiance"])
