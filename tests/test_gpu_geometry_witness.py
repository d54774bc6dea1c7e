"""GPU: the device's first hits and first-hit AOVs against the float64 geometric witness (geometry_witness.py; scenes in geometry_cases.py),
directly — not via the oracle.  pt_trace_primary under every acceleration structure (6-wide, $PTAMD_BVH4, the two-level structure, the radix
tree): the answer may differ between structures on a ray the witness leaves undecided, but it must stay in the allowed set, and t and the
point rebuilt from (u, v) must lie within geometry_witness.BOUNDS — bounds measured on the oracle, never on the device.  An actual 1 spp
render with AOVs, from the per-pixel leaf lists (k_camera_primary, the default) and without them: hit / miss per pixel in the allowed set,
and on decided pixels MOMENTS.r against t_k, NORMAL.rgb against the witness normal, ALBEDO.rgb against the witness albedo — the one place
where the fused bounce-0 kernel's t and the UV / normal interpolation behind it meet a reference other than the oracle.  The camera
constants against the geometry they stand for.  One tile / one wave (8x8) and one pixel (1x1).

Out of scope: alpha cut-outs (the alpha test drops hits by a random draw), thin-lens cameras, normal-mapped materials, hits of later bounces
and shadow rays (their rays cannot be observed through the ABI), the BSDF."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_cases as gc  # noqa: E402
import geometry_witness as gw  # noqa: E402
from conftest import STRUCTURE_ENV, skip_if_structure_env_preset  # noqa: E402
from platinum_amd import abi  # noqa: E402
from platinum_amd.renderer import Renderer  # noqa: E402

pytestmark = pytest.mark.gpu

SHOTS = (((48, 32), 0), ((50, 35), 977))       # (size, sample): whole tiles, and partial 8x8 tiles in both directions
INSTANCED = [n for n, c in gc.CASES.items() if c.instanced]
RADIX_CASES = ("cornell_sphere", "random8")


def _start(r, name, size, first_sample=0, aov=False, **kw):
    r.setDenoiseOptions(enabled=1 if aov else 0)
    r.clearRenderRegion()
    r.selectKernel(abi.INTEGRATOR_MIS)
    r.startRender(gc.scene(name), size, 1, max_bounces=1, first_sample=first_sample, **kw)


def _check_trace(r, name, size, sample, what):
    w = gc.witness(name, r.constants(), size[0], size[1], sample)
    if gc.CASES[name].coverage:
        assert w.decided_share >= gw.DECIDED_SHARE, (name, size, sample, w.decided_share)     # (a property of the witness, not of the device)
    gw.check_hits(w, r.tracePrimary(sample), "%s %dx%d sample %d, %s" % (name, size[0], size[1], sample, what))
    return w


@pytest.mark.parametrize("name", list(gc.CASES))
def test_first_hits_on_the_default_structure(gpu_renderer, name):
    for size, sample in SHOTS:
        _start(gpu_renderer, name, size)
        _check_trace(gpu_renderer, name, size, sample, "default structure")


@pytest.mark.parametrize("name", list(gc.CASES))
def test_first_hits_on_the_four_wide_form(gpu_renderer, name, monkeypatch):
    skip_if_structure_env_preset()
    size, sample = SHOTS[1]
    monkeypatch.setenv("PTAMD_BVH4", "1")
    _start(gpu_renderer, name, size)
    monkeypatch.delenv("PTAMD_BVH4")
    _check_trace(gpu_renderer, name, size, sample, "4-wide")


@pytest.mark.parametrize("name", INSTANCED)
def test_first_hits_on_the_two_level_structure(gpu_renderer, name):
    size, sample = SHOTS[1]
    _start(gpu_renderer, name, size, accel_structure=abi.ACCEL_TWO_LEVEL)
    assert gpu_renderer.stats().accel_two_level == 1
    _check_trace(gpu_renderer, name, size, sample, "two-level")


@pytest.mark.parametrize("name", RADIX_CASES)
def test_first_hits_on_the_radix_tree(gpu_renderer, name, monkeypatch):
    skip_if_structure_env_preset()
    size, sample = SHOTS[1]
    monkeypatch.setenv("PTAMD_RADIX_TREE", "1")
    _start(gpu_renderer, name, size)
    monkeypatch.delenv("PTAMD_RADIX_TREE")
    _check_trace(gpu_renderer, name, size, sample, "radix tree")


@pytest.mark.parametrize("size", [(8, 8), (1, 1)], ids=["one_wave", "one_pixel"])
def test_first_hits_at_the_wave_edge_sizes(gpu_renderer, size):
    for name in ("cornell_sphere", "random8"):
        _start(gpu_renderer, name, size)
        for sample in (0, 977):
            _check_trace(gpu_renderer, name, size, sample, "default structure")


# ---- an actual render --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk_renderer():
    """A renderer that never builds the camera-ray leaf lists: bounce 0 through k_raygen + the ordinary traversal (the switch is read at pt_create)."""
    assert os.environ.get("PTAMD_NO_CAMERA_LISTS", "0") in ("", "0"), "this module compares the switch's two sides"
    os.environ["PTAMD_NO_CAMERA_LISTS"] = "1"
    try:
        r = Renderer(device=0)
    finally:
        del os.environ["PTAMD_NO_CAMERA_LISTS"]
    yield r
    r.close()


def _check_render(r, name, size, sample, what):
    _start(r, name, size, first_sample=sample, aov=True)
    lists = r.cameraListStats()
    r.render(0)
    r.wait()
    albedo, normal, moments = (r.readbackAov(k).reshape(-1, 4) for k in (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS))
    r.setDenoiseOptions(enabled=0)
    w = gc.witness(name, r.constants(), size[0], size[1], sample)
    what = "%s %dx%d sample %d, %s" % (name, size[0], size[1], sample, what)
    hit = normal[:, 3]
    assert np.all((hit == 0.0) | (hit == 1.0))
    shown_miss, shown_hit = np.flatnonzero(hit == 0.0), np.flatnonzero(hit == 1.0)
    wrong = shown_miss[~w.allow_miss[shown_miss]]
    assert wrong.size == 0, "%s: %d pixels shown as a miss where the witness allows none; %s" % (what, wrong.size, w.describe(int(wrong[0])))
    wrong = shown_hit[w.n_hits[shown_hit] == 0]
    assert wrong.size == 0, "%s: %d pixels shown as a hit where the witness allows none; %s" % (what, wrong.size, w.describe(int(wrong[0])))
    rays = np.flatnonzero(w.decided_hit)
    assert rays.size and np.all(hit[rays] == 1.0)
    gw.check_aovs(w, rays, w.k[rays], albedo[rays], normal[rays], moments[rays, 0], what)
    return lists


@pytest.mark.parametrize("name", list(gc.CASES))
def test_a_one_sample_render_shows_the_witnesss_first_hits(gpu_renderer, walk_renderer, name):
    preset = any(v in os.environ for v in STRUCTURE_ENV)
    for size, sample in SHOTS:
        lists = _check_render(gpu_renderer, name, size, sample, "from the leaf lists")
        if not preset and gc.triangles(name).count > 8:      # (a structure whose root is a leaf has no lists: host_scene.h camera_lists_wanted)
            assert lists.built == 1 and lists.pixels_listed > 0
        assert _check_render(walk_renderer, name, size, sample, "without lists").built == 0


# ---- camera constants ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", list(gc.CAMERAS))
def test_camera_constants_of_the_device(gpu_renderer, camera):
    pos, target, f, sensor = gc.CAMERAS[camera]
    for size in ((640, 480), (50, 35), (192, 108)):
        gpu_renderer.setDenoiseOptions(enabled=0)
        gpu_renderer.startRender(gc.camera_scene(camera), size, 1, max_bounces=1)
        gw.check_camera(gpu_renderer.constants(), size[0], size[1], pos, target, sensor, f)
