"""GPU: the sun-and-sky generator (include/ptamd.h pt_generate_sky, platinum_amd/csrc/sky.hip).  The device equals the host build of
pt_sky.h (tests/emu/sky_emu.cpp) bit for bit -- image, covered texels, solid angle -- over sizes and option sets, and lies within the
float32 bound of the float64 witness; a render lit by a generated sky equals the oracle's render of the same image, accumulator and ray
counters; the equirectangular camera reads the map back, pixel for texel; the call needs no render and leaves one alone."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib  # noqa: E402
import projection_lib as pl  # noqa: E402
import sky_lib as sl  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer, make_params  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def r():
    x = Renderer(device=0)
    yield x
    x.close()


def _assert_device_equals_host(r, o, w, h, what):
    got, st = r.generateSky(options=o, width=w, height=h, stats=True)
    want, hst, flags = sl.host_sky(o, w, h)
    bad = (sl.bits(got) != sl.bits(want)).any(axis=-1)
    assert not bad.any(), "%s: %d texels differ, first (y, x) %s: device %s, host %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:2].tolist(), want[bad][:2].tolist())
    assert st.sun_texels == hst.sun_texels and st.sun_solid_angle == hst.sun_solid_angle, what
    assert st.sun_direction[:] == hst.sun_direction[:] and st.sun_radius_used == hst.sun_radius_used, what
    assert st.kernel_ms > 0, what
    return got, flags


# 1 x 1: one lane of one block; 8 x 4, 37 x 19: a partial block; 64 x 32: eight blocks; 256 x 128: 128 blocks, rows that cross blocks
@pytest.mark.parametrize("w,h", sl.GPU_SIZES)
@pytest.mark.parametrize("name", list(sl.OPTION_SETS))
def test_the_device_equals_the_host_build_and_lies_within_the_bound_of_the_witness(r, name, w, h):
    o = sl.case_options(name, w, h)
    got, flags = _assert_device_equals_host(r, o, w, h, "%s %dx%d" % (name, w, h))
    assert np.isfinite(got).all() and (got >= 0).all() and (got[..., 3] == 1).all()
    wit = sl.witness(name, w, h)
    ground, blocked = sl.unpack_flags(flags)
    mask = sl.compared(ground, blocked, wit)
    err = sl.rel_err(got, wit, mask)
    print("%s %d x %d: %.4g (bound %.4g), %.4f left out" % (name, w, h, err, sl.BOUNDS["bound"], 1 - mask.mean()))
    assert 1 - mask.mean() <= sl.LEFT_OUT_CAP
    assert err <= sl.BOUNDS["bound"]


def test_a_narrow_disc_on_a_wide_map_and_a_map_of_one_column(r):
    """2048 x 64: the disc's radius is pi / 64 on texels 32 times narrower than tall, so the coverage early-out is taken by whole waves on
    both sides of the sun; 1 x 64: a single column."""
    _assert_device_equals_host(r, sl.options(sun_azimuth=2.0, sun_elevation=0.3), 2048, 64, "2048x64")
    _assert_device_equals_host(r, sl.options(sun_azimuth=0.8), 1, 64, "1x64")


def test_generate_sky_needs_no_render_and_leaves_one_alone():
    fresh = Renderer(device=0)
    try:
        o = sl.options(sun_elevation=0.2)
        _assert_device_equals_host(fresh, o, 37, 19, "before any render")
        fresh.startRender(scenes.cornell_scene("bench"), (48, 32), 2, max_bounces=3)
        fresh.render(0)
        fresh.wait()
        acc, st = fresh.readbackAccumulator(), fresh.stats()
        fresh.generateSky(options=o, width=37, height=19)
        st2 = fresh.stats()
        assert np.array_equal(sl.bits(fresh.readbackAccumulator()), sl.bits(acc))
        assert (st.closest_rays, st.shadow_rays, st.paths) == (st2.closest_rays, st2.shadow_rays, st2.paths)
        lib = fresh._lib
        out = np.zeros((4, 8, 4), np.float32)
        bad = sl.options(dust_density=11.0)
        assert lib.pt_generate_sky(fresh._h, C.byref(bad), 8, 4, out.ctypes.data, None) == -1 and b"dust_density" in lib.pt_last_error()
        assert lib.pt_generate_sky(fresh._h, C.byref(o), 0, 4, out.ctypes.data, None) == -1 and b"texels" in lib.pt_last_error()
        assert lib.pt_generate_sky(fresh._h, C.byref(o), 8, 4, out.ctypes.data, None) == 0      # (stats_out may be null)
    finally:
        fresh.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def daylight_scene(r):
    """A ground quad and a box under a 64 x 32 daylight environment, the sun at e = 0.5 with its disc."""
    sc = scenes.Scene(name="daylight")
    ground = sc.add_mesh(scenes.plane(20.0))
    sc.add_instance(ground, scenes.Transform(), [scenes.Material(base_color=(0.6, 0.55, 0.5, 1.0))])
    box = sc.add_mesh(scenes.cube(1.5))
    sc.add_instance(box, scenes.Transform(translation=(0.0, 0.75, 0.0), rotation=(0.0, 0.5, 0.0)), [scenes.Material(base_color=(0.8, 0.3, 0.2, 1.0))])
    st = sc.set_sky(r, width=64, height=32, sun_elevation=0.5, sun_azimuth=2.4)
    assert st.sun_texels > 0 and sc.textures[sc.env_texture].pixels.shape == (32, 64, 4)
    sc.set_camera(scenes.Camera.with_focal_length(28.0), scenes.Transform(translation=(4.0, 2.5, 6.0), target=(0.0, 0.6, 0.0), track=True))
    return sc


def test_a_render_under_a_generated_sky_equals_the_oracles(r):
    sc = daylight_scene(r)
    w, h, spp, bounces = 32, 32, 16, 4
    r.selectKernel(abi.INTEGRATOR_MIS)
    r.startRender(sc, (w, h), spp, max_bounces=bounces)
    r.render(0)
    r.wait()
    acc, st = r.readbackAccumulator(), r.stats()
    o = oracle_lib.OracleScene(sc, make_params(w, h, spp, bounces))
    try:
        ref, so = o.render(0, spp), o.stats()
    finally:
        o.close()
    bad = (sl.bits(acc) != sl.bits(ref)).any(axis=-1)
    assert not bad.any(), "%d pixels differ, first (y, x) %s: device %s, oracle %s" % (
        int(bad.sum()), np.argwhere(bad)[:4].tolist(), acc[bad][:2].tolist(), ref[bad][:2].tolist())
    assert (st.closest_rays, st.shadow_rays, st.shaded_hits, st.paths) == (so.closest_rays, so.shadow_rays, so.shaded_hits, so.paths)
    lit = acc[..., :3].astype(np.float64)
    assert np.isfinite(lit).all() and lit.mean() > 0 and st.shadow_rays > 0       # the sun and sky light the scene by next-event estimation too


def test_the_equirectangular_camera_reads_the_map_back(r):
    """Default EQUIRECT at the map's resolution, looking along +x with y up: the pixels whose camera rays miss hold the map's texels."""
    sc = pl.probe_scene()
    sc.set_sky(r, width=64, height=32, sun_elevation=0.5, sun_azimuth=2.4)
    env = sc.textures[sc.env_texture].pixels
    H, W = env.shape[:2]
    r.setProjection(pl.projection(abi.PROJ_EQUIRECT))
    try:
        for s in (0, 977):
            r.startRender(sc, (W, H), 1, max_bounces=3, first_sample=s)
            miss = r.tracePrimary(s)["instance"] < 0
            r.render(0)
            r.wait()
            acc = r.readbackAccumulator()
            pl.check_probe(env, acc, miss, s, "daylight, sample %d" % s)
            y, x = np.unravel_index(np.argmax(acc[..., :3].sum(axis=-1)), (H, W))
            ey, ex = np.unravel_index(np.argmax(env[..., :3].sum(axis=-1)), (H, W))
            assert abs(int(y) - int(ey)) <= 1 and min((x - ex) % W, (ex - x) % W) <= 1     # the sun stands where the map has it
    finally:
        r.setProjection(pl.projection(abi.PROJ_PERSPECTIVE))
