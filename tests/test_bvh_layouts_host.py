"""What makes tests/test_gpu_bvh_builder.py meaningful, checked with the oracle alone: in every mosaic that module renders (tests/bvh_layouts.py)
the brute-force oracle — the intersection contract itself, no tree — sees EVERY leaf slot in EACH traced sample, and the oracle's own tree
gives the same records.  A slot the product's builder loses, or boxes too small, then costs a primary hit that the contract demands.
(`coincident` is the exception by construction: n copies of one triangle, the lowest id wins every pixel.)"""
import numpy as np
import pytest

import bvh_cases as C
import bvh_layouts as L

CASES = [c for c in C.mosaic_cases() if c[1] != "coincident"] + [(n, "instances", False) for n in C.INSTANCE_SIZES]


def _id(c):
    return "%s-%d%s" % (c[1], c[0], "-paired" if c[2] else "")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_brute_force_oracle_sees_every_slot_in_every_sample_and_its_tree_agrees(case):
    n, layout, paired = case
    sc, W, H, count, field = L.build(n, layout, paired)
    assert count == (2 * n if paired else n) and (len(sc.nodes) == n if layout == "instances" else sc.triangle_count == count)
    brute = C.reference(n, layout, paired, paths=False)["primary"]
    tree = L.oracle_primary(sc, W, H, True)
    for s, hb, ht in zip(L.SAMPLES, brute, tree):
        assert hb.shape == (H, W)
        miss = L.missing_ids(hb, count, field)
        assert len(miss) == 0, "sample %d: the contract itself does not see %s %s" % (s, field, miss[:8].tolist())
        assert hb.tobytes() == ht.tobytes(), "sample %d: the oracle's tree and its brute force differ" % s


def test_coincident_is_one_triangle_n_times_and_the_lowest_id_wins_every_pixel():
    sc, W, H = L.mosaic(9, "coincident")
    v = sc.meshes[0].positions[:, :3].reshape(9, 3, 3)
    assert (v == v[0]).all() and sc.triangle_count == 9
    for hb in C.reference(9, "coincident", paths=False)["primary"]:
        assert (hb["instance"] == 0).all() and (hb["primitive"] == 0).all()


def test_layouts_are_degenerate_in_the_way_their_names_say():
    n = 1025
    vert = lambda lay, **kw: L.mosaic(n, lay, **kw)[0].meshes[0].positions[:, :3]
    sc = vert("scatter")
    assert len(np.unique(sc, axis=0)) == 3 * n                       # no two triangles share a vertex position: n slots, n triangles
    assert len(np.unique(vert("flat")[:, 2])) == 1                    # zero extent on an axis
    line = vert("line").reshape(n, 3, 3)
    cen = 0.5 * (line.min(1) + line.max(1))
    assert len(np.unique(cen[:, 1])) == 1 and len(np.unique(cen[:, 2])) == 1 and len(np.unique(cen[:, 0])) == n   # collinear box centres
    for m in (2, n, 2049):
        e = L.mosaic(m, "expo")[0].meshes[0].positions[:, :3].astype(np.float64)
        assert np.abs(e).max() <= 1e15 and np.abs(e).max() > 0.9e15 and np.abs(e[:3]).max() <= 1.0
    out = vert("outlier").reshape(n, 3, 3)
    far = np.flatnonzero(-out[:, 0, 2] > 100.0)
    assert far.tolist() == [n // 2] and out[far[0], 0, 2] == np.float32(-4e6) and (-np.delete(out, far[0], 0)[:, :, 2]).max() <= 3.0
    assert (vert("negative") < 0).all() and (np.asarray(L.NEGATIVE_SHIFT) < 0).all()
    for m in C.LAYOUT_SIZES:
        lo, hi = L.world_bounds(L.mosaic(m, "straddle")[0])
        assert (lo < 0).all() and (hi > 0).all(), (m, lo, hi)
    pair = L.mosaic(n, "scatter", paired=True)[0].meshes[0]
    idx = pair.indices.reshape(n, 2, 3)
    assert pair.triangle_count == 2 * n and all(len(set(a) & set(b)) == 2 for a, b in idx[:: 97].tolist())   # two vertex indices in common


def test_instance_mosaic_is_one_triangle_mesh_under_translation_and_uniform_scale():
    sc, W, H = L.instance_mosaic(1025)
    assert len(sc.meshes) == 1 and sc.meshes[0].triangle_count == 1 and len(sc.nodes) == 1025
    for node in sc.nodes[:: 41]:
        w = np.asarray(node.world)
        assert w[0, 0] == w[1, 1] == w[2, 2] > 0 and np.count_nonzero(w[:3, :3]) == 3


def test_the_largest_case_is_4097_slots_in_a_260_by_256_image():
    assert max(c[0] for c in C.mosaic_cases()) == 4097 and L.mosaic(4097, "scatter")[1:] == (260, 256)
