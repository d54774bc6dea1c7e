"""GPU: the ambient-occlusion pass.  pt_debug_ao against the host build of pt_ao.h bit for bit; a render's counts against
the sum of pt_debug_ao's states, however the samples are batched and the queues laid out, and under every acceleration structure; the
float64 witness (ao_witness.py) on the device's own rays, with the table of the host test and no figure taken from the device; regions and
adaptive renders; thin-lens and orthographic cameras; every other output unchanged with AO on; restarts and every error code.
Sizes 48x32, 50x35 and 24x17, at most 64 samples in flight."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import ao_lib  # noqa: E402
import conftest  # noqa: E402
import geometry_cases as gc  # noqa: E402
import geometry_witness as gw  # noqa: E402
import projection_lib as pl  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer, make_params  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE, SPP, BOUNCES = (24, 17), 16, 3     # 24x17: a partial tile row, and a 1-pixel-high edge tile
W, H = SIZE
INF = float("inf")
INVALID, BAD_STATE, UNSUPPORTED = -1, -5, -6
SWITCHES = ("PTAMD_NO_CAMERA_LISTS", "PTAMD_TEST_CAMLIST_CAP", "PTAMD_TILES_PER_SEG", "PTAMD_SEG_BANDS", "PTAMD_REFILL")
AOVS = (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)


@pytest.fixture(scope="module")
def rr():
    r = Renderer(device=0)
    yield r
    r.close()


@pytest.fixture
def r(rr):
    rr.setAmbientOcclusionOptions(enabled=0, distance=1.0)
    yield rr
    rr.setAmbientOcclusionOptions(enabled=0, distance=1.0)


def _start(r, sc, size=SIZE, spp=SPP, bounces=BOUNCES, sif=0, ao=True, distance=2.0, aov=False, matte=False, film=False, region=None,
           adaptive=None, proj=None, **kw):
    r.setAmbientOcclusionOptions(enabled=1 if ao else 0, distance=distance)
    r.setDenoiseOptions(enabled=1 if aov else 0)
    r.setMatteOptions(enabled=1 if matte else 0)
    r.setFilmOptions(enabled=1 if film else 0)
    if region:
        r.setRenderRegion(*region)
    else:
        r.clearRenderRegion()
    if adaptive:
        r.setAdaptiveOptions(enabled=1, min_spp=adaptive[0], interval=adaptive[1], threshold=adaptive[2])
    else:
        r.setAdaptiveOptions(enabled=0)
    if proj is not None:
        r.setProjection(proj)
    try:
        r.startRender(sc, size, spp, max_bounces=bounces, samples_in_flight=sif, **kw)
    finally:   # (these options are read at startRender: the renderer goes back to its defaults for whoever uses it next)
        r.setAmbientOcclusionOptions(enabled=0, distance=1.0)
        r.setDenoiseOptions(enabled=0)
        r.setMatteOptions(enabled=0)
        r.setFilmOptions(enabled=0)
        r.clearRenderRegion()
        r.setAdaptiveOptions(enabled=0)
        if proj is not None:
            r.setProjection(pl.projection(abi.PROJ_PERSPECTIVE))


def _counts(r, sc, steps=(0,), **kw):
    _start(r, sc, **kw)
    for n in steps:
        r.render(n)
        r.wait()
    return r.readbackAmbientOcclusionCounts()


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


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_debug_equals_host(r, host, samples, distance, what):
    seen = set()
    for s in samples:
        got, want = r.debugAmbientOcclusion(s), host.debug(s, distance)
        for g, w, part in zip(got, want, ("origins", "directions", "states")):
            assert _same(g, w), "%s sample %d: %s differ at %s" % (what, s, part, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:3].tolist())
        seen |= set(np.unique(got[2]).tolist())
    return seen


@pytest.fixture(scope="module")
def textured():
    return scenes.textured_scene()


@pytest.fixture(scope="module")
def want16(textured):
    """The host build's counts of SPP samples of scenes.textured_scene() at SIZE, distance 2: computed once and read only"""
    c = ao_lib.HostAo(textured, make_params(W, H, 1024, BOUNCES)).counts(0, SPP, 2.0)
    c.flags.writeable = False
    return c


# ---- 1. the device equals the host build -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(48, 32), (50, 35)], ids=["48x32", "50x35"])
def test_debug_rays_and_states_equal_the_host_build_on_cornell(r, size):
    sc = gc.scene("cornell")
    host = ao_lib.HostAo(sc, make_params(size[0], size[1], 1024, BOUNCES))
    for D in (2.0, INF):
        _start(r, sc, size=size, distance=D)
        seen = _assert_debug_equals_host(r, host, (0, 1, 977), D, "cornell %dx%d distance %g" % (size + (D,)))
        assert seen >= {abi.AO_OCCLUDED, abi.AO_OPEN}


def test_debug_rays_and_states_equal_the_host_build_with_cut_outs_and_an_open_sky(r, textured):
    host = ao_lib.HostAo(textured, make_params(W, H, 1024, BOUNCES))
    for D in (2.0, INF):
        _start(r, textured, distance=D)
        seen = _assert_debug_equals_host(r, host, (0, 1, 977), D, "textured distance %g" % D)
        assert seen == {abi.AO_MISS, abi.AO_OCCLUDED, abi.AO_OPEN}


# ---- 2. a render equals its debug entry ------------------------------------------------------------------------------------------------------
def test_a_renders_counts_are_the_sum_of_the_debug_states(r, textured, want16):
    got = _counts(r, textured, sif=5)
    v = r.readbackAmbientOcclusion()
    st = r.ambientOcclusionStats()
    summed = np.zeros((H, W, 2), np.uint32)
    for s in range(SPP):
        ao_lib.fold_states(r.debugAmbientOcclusion(s)[2], summed)
    assert np.array_equal(got, summed) and np.array_equal(got, want16)
    assert np.array_equal(r.readbackAmbientOcclusionCounts(), got)      # the debug entry left the render's state alone
    assert v.dtype == np.float32 and _same(v, ao_lib.ao_value(got)) and _same(r.readbackAmbientOcclusion(), v)
    assert st.rays == int(got[..., 0].sum()) and st.ms_trace == 0.0 and st.ms_fold == 0.0
    assert 0 < got[..., 1].sum() < got[..., 0].sum() < W * H * SPP


def test_the_timer_classes_are_ao_own(r, textured):
    r.setProfiling(True)
    try:
        base = None
        for on in (False, True):
            _start(r, textured, sif=SPP, ao=on)
            r.render(0)
            r.wait()
            s = r.stats()
            launches = (s.launches_closest, s.launches_shadow)
            if on:
                a = r.ambientOcclusionStats()
                print("AO trace %.3f ms, fold %.3f ms" % (a.ms_trace, a.ms_fold))
                assert a.ms_trace > 0.0 and a.ms_fold > 0.0
                assert launches == base                                  # the AO trace is counted in no class of pt_stats
            base = launches
    finally:
        r.setProfiling(False)


# ---- 3. batching and layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sif", [1, 7, 8, 9, 16])
def test_counts_do_not_depend_on_the_batch_size(r, textured, want16, sif):
    got = _counts(r, textured, sif=sif)
    assert r.stats().batches == -(-SPP // sif)
    assert np.array_equal(got, want16)


def test_one_sample_calls_and_a_restart(r, textured, want16):
    assert np.array_equal(_counts(r, textured, steps=(1,) * SPP), want16)
    half = _counts(r, textured, steps=(8,))
    assert 0 < half[..., 0].sum() < want16[..., 0].sum()
    assert np.array_equal(_counts(r, textured), want16)                  # pt_start_render again: the counts start from 0


def test_a_64_sample_batch_takes_the_wave_walk(r):
    """samples_in_flight = 64 with a 64-sample step: k_camera_primary<true>"""
    sc = gc.scene("cornell")
    want = ao_lib.HostAo(sc, make_params(W, H, 1024, BOUNCES)).counts(0, 64, 2.0)
    _start(r, sc, spp=64, sif=64)
    if not any(v in os.environ for v in conftest.STRUCTURE_ENV + ("PTAMD_NO_CAMERA_LISTS",)):
        assert r.cameraListStats().built == 1
    r.render(0)
    r.wait()
    assert r.stats().batches == 1
    assert np.array_equal(r.readbackAmbientOcclusionCounts(), want)


@pytest.mark.parametrize("env", [{"PTAMD_NO_CAMERA_LISTS": "1"}, {"PTAMD_TEST_CAMLIST_CAP": "2"}, {"PTAMD_TILES_PER_SEG": "1", "PTAMD_SEG_BANDS": "2"},
                                 {"PTAMD_REFILL": "0"}, {"PTAMD_REFILL": "32"}],
                         ids=["no_lists", "unlisted_walk", "tiles_per_seg_1_bands_2", "refill_0", "refill_32"])
def test_counts_do_not_depend_on_the_queue_layout_or_the_camera_trace(textured, want16, env):
    for k in SWITCHES:
        assert os.environ.get(k, "0") in ("", "0"), "this test compares the switches' two sides"
    x = _renderer_under(env)
    try:
        got = _counts(x, textured, sif=SPP)
        if "PTAMD_TEST_CAMLIST_CAP" in env and not any(v in os.environ for v in conftest.STRUCTURE_ENV):
            cs = x.cameraListStats()
            assert cs.built == 1 and cs.pixels_walk > 0 and cs.pixels_listed > 0      # some pixels take the unlisted walk
        if "PTAMD_NO_CAMERA_LISTS" in env:
            assert x.cameraListStats().built == 0
        assert np.array_equal(got, want16)
    finally:
        x.close()


# ---- 4. structures ---------------------------------------------------------------------------------------------------------------------------
def test_counts_are_equal_under_every_one_bvh_structure(r, textured, want16, monkeypatch):
    conftest.skip_if_structure_env_preset()
    for var in (None, "PTAMD_BVH4", "PTAMD_RADIX_TREE"):
        if var:
            monkeypatch.setenv(var, "1")     # (read when the structure is built: at pt_start_render)
        got = _counts(r, textured, sif=SPP)
        if var:
            monkeypatch.delenv(var)
        assert np.array_equal(got, want16), var


def test_the_two_level_structure_satisfies_the_witness_and_agrees_where_it_decides(r):
    conftest.skip_if_structure_env_preset()
    name, size, D = "truth", (48, 32), 2.0
    sc = gc.scene(name)
    x = _renderer_under({"PTAMD_TWO_LEVEL": "1"})
    try:
        _start(r, sc, size=size, distance=D)
        _start(x, sc, size=size, distance=D)
        assert x.stats().accel_two_level == 1 and r.stats().accel_two_level == 0
        for s in (0, 977):
            a, b = r.debugAmbientOcclusion(s), x.debugAmbientOcclusion(s)
            ao_lib.check_witness(name, size[0], size[1], s, D, b[0], b[1], b[2], "two-level sample %d" % s)
            occ, opn = ao_lib.witness_classes(name, size[0], size[1], s, a[0], a[1])[D]
            decided = (occ | opn).reshape(a[2].shape)
            same_ray = (a[0].view(np.uint32) == b[0].view(np.uint32)).all(-1) & (a[1].view(np.uint32) == b[1].view(np.uint32)).all(-1)
            print("two-level sample %d: %d of %d AO rays identical to the default structure's" % (s, same_ray.sum(), same_ray.size))
            both = decided & same_ray
            assert both.mean() > 0.9 and np.array_equal(a[2][both], b[2][both])
    finally:
        x.close()


# ---- 5. the witness on the device ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "truth"])
def test_device_rays_satisfy_the_witness(r, name):
    for size in gc.SIZES:
        py, px = np.mgrid[0:size[1], 0:size[0]]
        for D in ao_lib.DISTANCES:
            _start(r, gc.scene(name), size=size, distance=D)
            for s in gc.SAMPLES:
                o, d = r.debugCameraRays(s)
                cam = (o, d, gw.halton_offset(px.ravel(), py.ravel(), s).reshape(size[1], size[0]))
                ao_lib.check_side(name, size[0], size[1], s, D, cam, r.tracePrimary(s), r.debugAmbientOcclusion(s),
                                  "device, %s %dx%d sample %d" % (name, size[0], size[1], s))


# ---- 6. regions and adaptive renders ---------------------------------------------------------------------------------------------------------
REGION = (5, 3, 19, 14)      # not tile-aligned


def test_a_region_keeps_the_full_frame_counts_inside_and_nothing_outside(r, textured, want16):
    got = _counts(r, textured, sif=7, region=REGION)
    inside = np.zeros((H, W), bool)
    inside[REGION[1]:REGION[3], REGION[0]:REGION[2]] = True
    assert np.array_equal(got[inside], want16[inside]) and not got[~inside].any() and want16[~inside].any()
    assert np.all(r.readbackAmbientOcclusion()[~inside] == 1.0)


def test_an_adaptive_tile_holds_the_counts_of_its_own_samples(r):
    kind, _size, bounces, _spp, min_spp, interval, threshold = al.CONFIGS["textured99"]
    sc, size, spp = al.config_scene(kind), (33, 19), 64
    got = _counts(r, sc, size=size, spp=spp, bounces=bounces, adaptive=(min_spp, interval, threshold))
    n = r.readbackSampleCounts()
    classes = sorted(set(n.ravel().tolist()))
    print("sample counts:", al.histogram(n))
    assert len(classes) > 1 and classes[-1] <= spp and classes[0] >= min_spp, classes
    assert np.all(got[..., 0] <= n) and np.all(got[..., 1] <= got[..., 0])
    host = ao_lib.HostAo(sc, make_params(size[0], size[1], 1024, bounces))
    want = np.zeros((size[1], size[0], 2), np.uint32)
    for s in range(classes[-1]):
        st = host.debug(s, 2.0)[2]
        ao_lib.fold_states(np.where(s < n, st, abi.AO_MISS).astype(np.uint32), want)
    assert np.array_equal(got, want)


# ---- 7. other cameras ------------------------------------------------------------------------------------------------------------------------
def test_thin_lens_and_orthographic_cameras_equal_the_host_build(r):
    size = (48, 32)
    p = make_params(size[0], size[1], 1024, BOUNCES)
    lens = ao_lib.thin_lens_scene()
    _start(r, lens, size=size)
    assert r.constants().camera.apertureRadius > 0.0
    assert len(_assert_debug_equals_host(r, ao_lib.HostAo(lens, p), (0, 977), 2.0, "thin lens")) >= 2
    sc = gc.scene("cornell")
    ortho = pl.projection(abi.PROJ_ORTHOGRAPHIC, ortho_height=9.0)
    _start(r, sc, size=size, proj=ortho)
    assert r.renderProjection().kind == abi.PROJ_ORTHOGRAPHIC
    assert len(_assert_debug_equals_host(r, ao_lib.HostAo(sc, p, proj=ortho), (0, 977), 2.0, "orthographic")) >= 2
    r.render(0)
    r.wait()
    assert np.array_equal(r.readbackAmbientOcclusionCounts(), ao_lib.HostAo(sc, p, proj=ortho).counts(0, SPP, 2.0))


# ---- 8. nothing else moves -------------------------------------------------------------------------------------------------------------------
def _everything_else(r, sc, ao, **kw):
    _start(r, sc, sif=5, ao=ao, aov=True, matte=True, film=True, **kw)
    r.render(0)
    r.wait()
    st = r.stats()
    out = [r.readbackAccumulator()] + [r.readbackAov(k) for k in AOVS] + [r.readbackFilm()]
    slots = [r.readbackMatteSlots(layer) for layer in (abi.MATTE_INSTANCE, abi.MATTE_MATERIAL)]
    return out, slots, r.readbackSampleCounts(), r.readbackRenderTarget(), (st.closest_rays, st.shadow_rays, st.shaded_hits, st.paths, st.batches)


@pytest.mark.parametrize("gmon", [False, True])
def test_every_other_output_is_the_same_bits_with_ao_on(r, textured, want16, gmon):
    kw = dict(flags=abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON, gmonBuckets=4) if gmon else {}
    off = _everything_else(r, textured, False, **kw)
    assert r._lib.pt_read_ao(r._h, np.empty((H, W), np.float32).ctypes.data) == BAD_STATE
    on = _everything_else(r, textured, True, **kw)
    assert np.array_equal(r.readbackAmbientOcclusionCounts(), want16)    # GMoN is independent
    assert on[4] == off[4] and on[4][3] == W * H * SPP
    assert np.array_equal(on[2], off[2]) and np.array_equal(on[3], off[3])
    for a, b in zip(on[1], off[1]):
        assert np.array_equal(a, b)
    for a, b in zip(on[0], off[0]):
        assert np.any(a != 0) and al.same_bits_or_both_nan(a, b).all()


# ---- 9. restarts and errors ------------------------------------------------------------------------------------------------------------------
def test_an_ao_off_restart_releases_the_buffers_and_every_error_code(r, textured):
    L, h = r._lib, r._h
    out, cnt = np.empty((H, W), np.float32), np.empty((H, W, 2), np.uint32)
    _start(r, textured)
    r.render(0)
    assert L.pt_read_ao(h, out.ctypes.data) == 0
    assert L.pt_read_ao(h, None) == INVALID and L.pt_read_ao_counts(h, None) == INVALID and L.pt_get_ao_stats(h, None) == INVALID
    assert L.pt_debug_ao(h, 0, None, None, None) == 0                    # (any output may be left out)
    _start(r, textured, ao=False)
    r.render(0)
    r.wait()
    for call in (lambda: L.pt_read_ao(h, out.ctypes.data), lambda: L.pt_read_ao_counts(h, cnt.ctypes.data),
                 lambda: L.pt_debug_ao(h, 0, None, None, cnt.ctypes.data), lambda: L.pt_get_ao_stats(h, C.byref(abi.AoStats()))):
        assert call() == BAD_STATE and b"ambient occlusion" in L.pt_last_error()
    for bad in (dict(enabled=2), dict(distance=0.0), dict(distance=-1.0), dict(distance=float("nan"))):
        o = r.ambientOcclusionOptions()
        for k, v in bad.items():
            setattr(o, k, v)
        assert L.pt_set_ao_options(h, C.byref(o)) == INVALID, bad
    assert L.pt_set_ao_options(h, None) == INVALID
    assert (r.ambientOcclusionOptions().enabled, r.ambientOcclusionOptions().distance) == (0, 1.0)   # a refused struct changes nothing
    fresh = Renderer(device=0)
    try:
        assert fresh._lib.pt_read_ao(fresh._h, out.ctypes.data) == BAD_STATE      # before pt_start_render
        assert fresh._lib.pt_debug_ao(fresh._h, 0, None, None, None) == BAD_STATE
    finally:
        fresh.close()
    g = Renderer(devices=[0, 0])
    try:
        o = g.ambientOcclusionOptions()
        o.enabled = 1
        assert g._lib.pt_set_ao_options(g._h, C.byref(o)) == UNSUPPORTED and b"device group" in g._lib.pt_last_error()
        o.enabled = 0
        assert g._lib.pt_set_ao_options(g._h, C.byref(o)) == 0
        o.distance = -1.0
        assert g._lib.pt_set_ao_options(g._h, C.byref(o)) == INVALID
        assert g._lib.pt_read_ao(g._h, out.ctypes.data) == UNSUPPORTED and g._lib.pt_read_ao_counts(g._h, cnt.ctypes.data) == UNSUPPORTED
        assert g._lib.pt_debug_ao(g._h, 0, None, None, None) == UNSUPPORTED
        assert g._lib.pt_get_ao_stats(g._h, C.byref(abi.AoStats())) == UNSUPPORTED
    finally:
        g.close()
