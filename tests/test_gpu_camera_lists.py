"""GPU: camera rays traced from per-pixel leaf lists (platinum_amd/csrc/pt_camlist.h).  A render with the lists holds the bits
of a render without them: two renderers in one process, one created under $PTAMD_NO_CAMERA_LISTS=1, must agree on every accumulator bit
and on the ray counters.  A third, created with a tiny test-only capacity, exercises the pixels that are left to the ordinary traversal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer  # noqa: E402

pytestmark = pytest.mark.gpu


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
def r_on():
    assert os.environ.get("PTAMD_NO_CAMERA_LISTS", "0") in ("", "0"), "this module compares lists on against lists off"
    r = Renderer(device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def r_off():
    r = _renderer_under({"PTAMD_NO_CAMERA_LISTS": "1"})
    yield r
    r.close()


@pytest.fixture(scope="module")
def r_tiny():
    r = _renderer_under({"PTAMD_TEST_CAMLIST_CAP": "2"})
    yield r
    r.close()


@pytest.fixture(scope="module")
def field():
    return scenes.field_scene(grid=4)


def _render(r, sc, size, spp, bounces=4, steps=(0,), sif=0):
    r.startRender(sc, size, spp, max_bounces=bounces, samples_in_flight=sif)
    cl = r.cameraListStats()
    for n in steps:
        r.render(n)
        r.wait()
    acc = r.readbackAccumulator()
    st = r.stats()
    return acc, (st.closest_rays, st.shadow_rays, st.shaded_hits, st.paths), cl


def _same(a, b):
    acc_a, cnt_a, _ = a
    acc_b, cnt_b, _ = b
    assert cnt_a == cnt_b
    diff = np.flatnonzero(acc_a.view(np.uint32) != acc_b.view(np.uint32))
    assert diff.size == 0, "%d accumulator words differ, the first at %d" % (diff.size, diff[0])


@pytest.mark.parametrize("spp", [1, 46, 64, 130])
def test_field_scene_is_bit_identical_with_and_without_lists(r_on, r_off, field, spp):
    # 67x41: partial tiles on both edges; 46 samples: chunks straddle pixels; 130 in batches of 64: 64 + 64 + 2
    on = _render(r_on, field, (67, 41), spp, sif=64)
    off = _render(r_off, field, (67, 41), spp, sif=64)
    assert on[2].built == 1 and on[2].pixels_listed + on[2].pixels_walk == 67 * 41 and on[2].pixels_walk == 0
    assert on[2].entries > 0 and on[2].build_ms > 0 and sum(on[2].length_histogram) == 67 * 41
    assert off[2].built == 0 and off[2].pixels_listed == 0 and off[2].entries == 0
    _same(on, off)


def test_cornell_in_two_consecutive_batches(r_on, r_off):
    sc = scenes.cornell_scene("bench")
    on = _render(r_on, sc, (64, 64), 16, steps=(8, 8), sif=8)
    off = _render(r_off, sc, (64, 64), 16, steps=(8, 8), sif=8)
    assert on[2].built == 1 and on[2].pixels_walk == 0 and off[2].built == 0
    _same(on, off)


def test_textured_scene_with_cutouts_and_environment(r_on, r_off):
    sc = scenes.textured_scene()
    on = _render(r_on, sc, (64, 48), 8)
    off = _render(r_off, sc, (64, 48), 8)
    assert on[2].built == 1 and off[2].built == 0
    _same(on, off)


def test_thin_lens_camera_builds_no_lists(r_on, r_off):
    sc = scenes.cornell_scene("bench")
    sc.camera.aperture = 2.0
    sc.camera.focus_distance = 15.0
    on = _render(r_on, sc, (64, 64), 8)
    off = _render(r_off, sc, (64, 64), 8)
    assert on[2].built == 0 and on[2].pixels_listed == 0 and on[2].pixels_walk == 0 and on[2].entries == 0
    _same(on, off)


def test_a_tiny_capacity_leaves_some_pixels_to_the_walk_and_changes_no_bit(r_tiny, r_off, field):
    tiny = _render(r_tiny, field, (67, 41), 46, sif=64)
    off = _render(r_off, field, (67, 41), 46, sif=64)
    assert tiny[2].built == 1 and tiny[2].capacity == 2
    assert 0 < tiny[2].pixels_walk < 67 * 41 and tiny[2].pixels_listed == 67 * 41 - tiny[2].pixels_walk
    _same(tiny, off)
