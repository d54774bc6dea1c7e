"""GPU: bounce 0 as one kernel (k_camera_primary) leaves every bit where k_raygen + k_trace_closest leave it.  Two renderers in
one process — the default and one created under $PTAMD_NO_CAMERA_LISTS=1 (the ordinary traversal) — must agree on every accumulator word and on
the ray counters.  The shapes are the smallest at which each path of the
kernel can go wrong: batches whose iterations straddle pixels (the per-lane walk), batches of a multiple of 64 samples (the wave walk, with
whole iterations squeezed out of partial tiles), a tail batch, flagged pixels behind the fused kernel, cut-outs and misses, and the AOV pass
that reads the queue behind it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCHES = ("PTAMD_NO_CAMERA_LISTS", "PTAMD_TEST_CAMLIST_CAP")


def _renderer_under(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Renderer(device=0)    # (the PTAMD_* switches are read at pt_create)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def pair():
    """(fused, no lists)"""
    for k in SWITCHES:
        assert os.environ.get(k, "0") in ("", "0"), "this module compares the switches' two sides"
    rs = [Renderer(device=0), _renderer_under({"PTAMD_NO_CAMERA_LISTS": "1"})]
    yield rs
    for r in rs:
        r.close()


@pytest.fixture(scope="module")
def pair_tiny():
    """the same two with two entries per pixel: some pixels are left to the walk"""
    rs = [_renderer_under({"PTAMD_TEST_CAMLIST_CAP": "2"}), _renderer_under({"PTAMD_NO_CAMERA_LISTS": "1"})]
    yield rs
    for r in rs:
        r.close()


@pytest.fixture(scope="module")
def field():
    return scenes.field_scene(grid=4)


def _render(r, sc, size, spp, bounces=4, steps=(0,), sif=0, aov=False, region=None):
    r.setDenoiseOptions(enabled=1 if aov else 0)
    if region:
        r.setRenderRegion(*region)
    else:
        r.clearRenderRegion()
    r.startRender(sc, size, spp, max_bounces=bounces, samples_in_flight=sif)
    cl = r.cameraListStats()
    for n in steps:
        r.render(n)
        r.wait()
    acc = r.readbackAccumulator()
    st = r.stats()
    aovs = [r.readbackAov(k) for k in (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)] if aov else []
    r.setDenoiseOptions(enabled=0)
    r.clearRenderRegion()
    return acc, (st.closest_rays, st.shadow_rays, st.shaded_hits, st.paths), cl, aovs


def _same(a, b):
    assert a[1] == b[1]
    for img_a, img_b in zip([a[0]] + a[3], [b[0]] + b[3]):
        diff = np.flatnonzero(img_a.view(np.uint32) != img_b.view(np.uint32))
        assert diff.size == 0, "%d words differ, the first at %d" % (diff.size, diff[0])


def _both(rs, *args, **kw):
    fused, walk = (_render(r, *args, **kw) for r in rs)
    assert fused[1][3] > 0
    _same(fused, walk)
    return fused, walk


@pytest.mark.parametrize("spp", [1, 46, 64, 130])
def test_field_scene_with_partial_tiles(pair, field, spp):
    # 67x41: partial tiles on both edges.  1 and 46 samples: iterations straddle pixels; 64: one pixel per iteration; 130: 64 + 64 + 2
    fused, walk = _both(pair, field, (67, 41), spp, sif=64)
    assert fused[2].built == 1 and fused[2].pixels_walk == 0 and walk[2].built == 0


def test_two_iterations_per_pixel(pair, field):
    _both(pair, field, (67, 41), 128, sif=128)


def test_cornell_in_two_consecutive_batches(pair):
    fused, _ = _both(pair, scenes.cornell_scene("bench"), (64, 64), 16, steps=(8, 8), sif=8)
    assert fused[2].built == 1 and fused[2].pixels_walk == 0


def test_cutouts_and_environment(pair):
    _both(pair, scenes.textured_scene(), (64, 48), 8)


@pytest.mark.parametrize("spp", [46, 64])
def test_flagged_pixels_go_to_the_walk_behind_the_fused_kernel(pair_tiny, field, spp):
    fused, _ = _both(pair_tiny, field, (67, 41), spp, sif=64)
    assert fused[2].built == 1 and fused[2].capacity == 2 and 0 < fused[2].pixels_walk < 67 * 41


@pytest.mark.parametrize("spp", [46, 64])
def test_first_hit_aovs_read_the_queue_behind_the_fused_kernel(pair, field, spp):
    fused, _ = _both(pair, field, (67, 41), spp, sif=64, aov=True)
    assert len(fused[3]) == 3 and np.any(fused[3][0][..., :3] != 0)


def test_thin_lens_and_region_renders_keep_their_kernels(pair):
    sc = scenes.cornell_scene("bench")
    _both(pair, sc, (64, 64), 8, region=(9, 5, 50, 41))
    sc.camera.aperture = 2.0
    sc.camera.focus_distance = 15.0
    fused, _ = _both(pair, sc, (64, 64), 8)
    assert fused[2].built == 0
