"""CPU: first hits and first-hit AOVs of the oracle (its tree and its brute force) and of the host build of the product's stage functions
against the float64 geometric witness (geometry_witness.py; scenes in geometry_cases.py).  Every other geometric check in the suite is
"two programs by the same author agree"; this one holds the instance transform (mirrored and non-uniform scales), the flattening, which
corner of a triangle is v0 and what u and v mean, interpolate3's barycentric order, transformVec on normals, the UV order and the camera
constants against geometry written down once more, from the scene description, in float64.

Asserted: every answer lies in the witness's allowed set; t and the point rebuilt from (u, v) lie within geometry_witness.BOUNDS; the normal,
depth, hit flag and albedo (untextured and textured) of HostScene.stage_aov on those hits do too; at least 99 % of the rays of every scene
not built for ties or edge-on views are decided by the witness alone.  Each test prints its figures before it asserts (pytest -s shows them).

Out of scope: alpha cut-outs (the alpha test drops hits by a random draw), thin-lens cameras, normal-mapped materials, hits of later bounces
and shadow rays, the BSDF."""
import numpy as np
import pytest

import denoise_lib as dl
import emu_lib
import geometry_cases as gc
import geometry_witness as gw
import oracle_lib
from platinum_amd import scenes
from platinum_amd.renderer import make_params

check_hits, check_aovs = gw.check_hits, gw.check_aovs
CASE_SIZES = [(n, s) for n in gc.CASES for s in gc.SIZES]
IDS = ["%s-%dx%d" % (n, s[0], s[1]) for n, s in CASE_SIZES]


def _sides(sc, p, monkeypatch):
    sides = {"oracle tree": oracle_lib.OracleScene(sc, p, use_bvh=True), "oracle brute force": oracle_lib.OracleScene(sc, p, use_bvh=False),
             "host build": emu_lib.EmuScene(sc, p)}
    monkeypatch.setenv("EMU_WIDE6", "1")    # the device's default form: 6-wide nodes, two triangles per leaf slot (read at emu_create)
    monkeypatch.setenv("EMU_PAIRS", "1")
    sides["host build, pair slots"] = emu_lib.EmuScene(sc, p)
    monkeypatch.delenv("EMU_WIDE6")
    monkeypatch.delenv("EMU_PAIRS")
    return sides


@pytest.mark.parametrize("name,size", CASE_SIZES, ids=IDS)
def test_first_hits_are_allowed_and_within_the_bounds(name, size, monkeypatch):
    W, H = size
    sc = gc.scene(name)
    sides = _sides(sc, make_params(W, H, 1024, 1), monkeypatch)
    seen = set()
    for s in gc.SAMPLES:
        w = gc.witness(name, sides["oracle tree"].constants(), W, H, s)
        if gc.CASES[name].coverage:
            assert w.decided_share >= gw.DECIDED_SHARE, (name, s, w.decided_share)
        for what, side in sides.items():
            assert bytes(side.constants().camera) == bytes(sides["oracle tree"].constants().camera)
            k = check_hits(w, side.trace_primary(s), "%s %dx%d sample %d, %s" % (name, W, H, s, what))
            seen |= set(w.T.inst[k[k >= 0]].tolist())
        assert w.decided_hit.any()
    if name == "tmin":
        assert seen == {0, 1}    # both walls: the near one is passed along the axis and hit towards the corners


@pytest.mark.parametrize("name,size", CASE_SIZES, ids=IDS)
def test_first_hit_aovs_match_the_witness(name, size):
    W, H = size
    sc = gc.scene(name)
    p = make_params(W, H, 1024, 1)
    o = oracle_lib.OracleScene(sc, p)
    hs = dl.HostScene(sc, p)
    for s in gc.SAMPLES:
        w = gc.witness(name, o.constants(), W, H, s)
        hits = o.trace_primary(s)
        bad, err = w.check_hits(hits)
        assert bad.size == 0
        k = err["k"]
        a, n = (x.reshape(-1, 4) for x in hs.stage_aov(s, hits))
        rays = np.flatnonzero(k >= 0)
        assert rays.size and np.all(n[rays, 3] == 1.0)                                          # the hit flag
        miss = np.flatnonzero(k < 0)
        assert np.all(n[miss] == 0.0) and np.all(a[miss, 3] == 0.0) and np.all(a[miss, :3] == 1.0)   # aov_miss: white, no normal, t = 0
        check_aovs(w, rays, k[rays], a[rays], n[rays], a[rays, 3], "%s %dx%d sample %d" % (name, W, H, s))
        if name == "uv_order":
            assert sum(w.T.materials[m].base_texture >= 0 for m in w.T.mat[k[rays]]) > rays.size // 2    # the textured path is what is seen


def test_on_the_truth_scene_the_forward_matrix_normal_is_the_true_normal():
    """What makes the normal check on geometry_cases.truth_scene a check against truth: every instance there is a rotation times a uniform
    scale, for which M n and the inverse transpose's M^-T n have the same direction."""
    T = gc.triangles("truth")
    rng = np.random.default_rng(3)
    n = rng.normal(size=(T.count, 3))
    fwd = np.einsum("nrc,nc->nr", T.m3, n)
    inv_t = np.einsum("nrc,nc->nr", np.linalg.inv(T.m3).transpose(0, 2, 1), n)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    assert np.abs(unit(fwd) - unit(inv_t)).max() < 1e-6      # (the matrices are float32 products of float32 rotations: orthogonal to ~1e-7)
    T = gc.triangles("uv_order")                             # and it is NOT so under the non-uniform scales of the other scenes
    fwd = np.einsum("nrc,nc->nr", T.m3, n[:T.count])
    inv_t = np.einsum("nrc,nc->nr", np.linalg.inv(T.m3).transpose(0, 2, 1), n[:T.count])
    assert np.abs(unit(fwd) - unit(inv_t)).max() > 0.1


def test_the_random_cases_hold_mirrored_and_anisotropic_instances():
    facts = gc._check_random_seeds()
    assert len(facts) >= 6 and all(d < 0 for d, _ in facts) and max(r for _, r in facts) >= 3.0


def test_witness_on_a_triangle_worked_by_hand():
    """o = 0, d = -z: the triangle (−1,−1,−2) (3,−1,−2) (−1,3,−2) is met at t = 2 with u = v = 1/4 (the point is v0 + (e1 + e2) / 4)."""
    v = np.array([[-1, -1, -2], [3, -1, -2], [-1, 3, -2]], np.float64)
    t, u, vv, cond = gw._tuvc(np.zeros(3), np.array([0.0, 0.0, -1.0]), v[0], v[1], v[2])
    assert (t, u, vv) == (2.0, 0.25, 0.25) and cond == pytest.approx(16.0 / (4.0 * 4.0))
    # and the sample positions are the sampler's: pixel + Halton(offset, dims 0 and 1), known answers from the KAT file's first offset
    fx, fy = gw.sample_positions(2, 1, 0)
    off = int(gw.halton_offset(np.array([0]), np.array([0]), 0)[0])
    assert off == 251852841
    assert 0 <= fx[0] < 1 and 1 <= fx[1] < 2 and 0 <= fy[0] < 1


@pytest.mark.parametrize("camera", list(gc.CAMERAS))
@pytest.mark.parametrize("size", [(640, 480), (50, 35), (192, 108)], ids=lambda s: "%dx%d" % s)
def test_camera_constants_of_the_oracle_and_the_host_build(camera, size):
    pos, target, f, sensor = gc.CAMERAS[camera]
    o = oracle_lib.OracleScene(gc.camera_scene(camera), make_params(size[0], size[1], 1, 1))
    gw.check_camera(o.constants(), size[0], size[1], pos, target, sensor, f)
    e = emu_lib.EmuScene(gc.camera_scene(camera), make_params(size[0], size[1], 1, 1))
    gw.check_camera(e.constants(), size[0], size[1], pos, target, sensor, f)


def test_the_default_camera_case_is_the_references_menu_entry():
    a, b = scenes.cornell_scene("default"), gc.camera_scene("default")
    assert np.array_equal(a.camera_world, b.camera_world) and a.camera == b.camera
    a, b = scenes.cornell_scene("bench"), gc.camera_scene("bench")
    assert np.array_equal(a.camera_world, b.camera_world) and a.camera == b.camera


def measure_oracle():
    """The worst error of the oracle (tree and brute force; AOVs on the tree's hits) against the witness over every case, size and sample:
    what geometry_witness.MEASURED records."""
    worst = dict.fromkeys(gw.MEASURED, 0.0)
    for name in gc.CASES:
        sc = gc.scene(name)
        for W, H in gc.SIZES:
            p = make_params(W, H, 1024, 1)
            tree, brute, hs = oracle_lib.OracleScene(sc, p, use_bvh=True), oracle_lib.OracleScene(sc, p, use_bvh=False), dl.HostScene(sc, p)
            for s in gc.SAMPLES:
                w = gc.witness(name, tree.constants(), W, H, s)
                for o in (brute, tree):
                    hits = o.trace_primary(s)
                    _, err = w.check_hits(hits)
                    worst["t"], worst["point"] = max(worst["t"], err["t"][0]), max(worst["point"], err["point"][0])
                k = err["k"]                            # (hits, k: the tree's)
                rays = np.flatnonzero(k >= 0)
                a, n = (x.reshape(-1, 4) for x in hs.stage_aov(s, hits))
                ref = w.aov(rays, k[rays])
                worst["normal"] = max(worst["normal"], float(np.abs(n[rays, :3] - ref["normal"]).max()))
                worst["albedo"] = max(worst["albedo"], float(np.abs(a[rays, :3] - ref["albedo"]).max()))
    return worst


def test_the_bounds_table_is_four_times_the_oracles_measured_worst():
    worst = measure_oracle()
    print("measured on the oracle:", worst)
    for q, m in gw.MEASURED.items():
        assert worst[q] <= m <= 1.05 * worst[q], (q, worst[q], m)     # (recorded to three digits, rounded up)
        assert gw.BOUNDS[q] == 4.0 * m
