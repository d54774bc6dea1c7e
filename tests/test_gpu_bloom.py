"""GPU: bloom (include/ptamd.h pt_bloom_options, platinum_amd/csrc/bloom.hip).  pt_debug_bloom equals the host build of pt_bloom.h
(tests/emu/bloom_emu.cpp) bit for bit, image and pyramid, over sizes, cards and option sets; on renders the target, read and presented, equals the oracle's post-process of the host bloom of the
image the target shows, on plain, auto-exposed, denoised, region and device-group renders; enabled = 0 leaves a renderer without the
feature; option changes without a restart, a restart at another size; errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bloom_lib as bl  # noqa: E402
import oracle_lib  # noqa: E402
import region_lib as rl  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer, make_params  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
B = 4
SIZE, SPP = (67, 45), 4      # the rendered Cornell `bench` of the tests below
ON = dict(enabled=1, intensity=0.35, threshold=0.25, knee=0.125, scatter=0.8, levels=5)   # strong enough to move most bytes of the target


def _restore(r):
    r.clearRenderRegion()
    for struct, default, setter in ((abi.BloomOptions, "pt_default_bloom_options", r.setBloomOptions),
                                    (abi.ExposureOptions, "pt_default_exposure_options", r.setExposureOptions),
                                    (abi.DenoiseOptions, "pt_default_denoise_options", r.setDenoiseOptions)):
        o = struct()
        getattr(r._lib, default)(C.byref(o))
        setter(o)
    r.resetExposure()
    r.setPostProcessOptions(r.postProcessOptions())
    r.setTonemapOptions(r.tonemapOptions())


@pytest.fixture
def r(gpu_renderer):
    _restore(gpu_renderer)
    yield gpu_renderer
    _restore(gpu_renderer)      # the session's renderer goes on with bloom disabled


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _render(r, sc, size=SIZE, spp=SPP, bounces=B, **kw):
    r.startRender(sc, size, spp, max_bounces=bounces, **kw)
    r.render(0)
    r.wait()


def _scaled(img, gain):
    out = np.array(img, np.float32)
    with np.errstate(all="ignore"):
        out[..., :3] *= f32(gain)
    return out


def _oracle_target(sc, size, img, po, to):
    o = oracle_lib.OracleScene(sc, make_params(size[0], size[1], 1, B))
    try:
        return o.postprocess(img, po, to)
    finally:
        o.close()


def _present(r):
    """The presented image, copied off the device buffer presentRenderTarget returns."""
    ptr, stream = r.presentRenderTarget()
    assert ptr and stream
    hip = abi.load_library()
    w, h = r.size
    got = np.empty((h, w, 4), np.uint8)
    assert hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
    assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), C.c_void_p(ptr), C.c_size_t(got.nbytes), 2) == 0  # hipMemcpyDeviceToHost
    return got


def _assert_debug_equals_host(r, img, o, what):
    got, got_pyr = r.debugBloom(img, options=o, pyramid=True)
    want, want_pyr = bl.host_bloom(img, o, pyramid=True)
    bad = (_bits(got) != _bits(want)).any(axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first (y, x) %s: device %s, host %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:2].tolist(), want[bad][:2].tolist())
    assert got_pyr.shape == want_pyr.shape
    badp = (_bits(got_pyr) != _bits(want_pyr)).any(axis=-1)
    assert not badp.any(), "%s: %d pyramid texels differ, first %s: device %s, host %s" % (
        what, int(badp.sum()), np.argwhere(badp)[:4].ravel().tolist(), got_pyr[badp][:2].tolist(), want_pyr[badp][:2].tolist())


# ---- pt_debug_bloom against the host build -------------------------------------------------------------------------------------------------
# 1x1, 2x1, 1x7, 3x2: levels collapsing, clamps on every side; 16x16, 17x15: one block, a partial second block; 33x31: the tile halo crosses
# blocks; 67x45; 256x128, 258x128, 254x128: levels whose width is a multiple of the tile, one more and one less; 8192x1 with 12 levels: one row
# of 256 blocks, every level a single row
DEBUG_SIZES = bl.SIZES + [(258, 128), (254, 128), (8192, 1)]


@pytest.mark.parametrize("W,H", DEBUG_SIZES)
def test_debug_bloom_equals_the_host_build(r, W, H):
    sets = dict(bl.OPTION_SETS)
    if (W, H) == (8192, 1):
        sets["defaults-12"] = dict(levels=12)
    for name in bl.CARDS + ("nonfinite",):
        img = bl.card(name, W, H)
        for setname, f in sets.items():
            _assert_debug_equals_host(r, img, bl.options(**f), "%s %dx%d %s" % (name, W, H, setname))


def test_debug_bloom_needs_no_render_and_leaves_the_renderer_alone():
    fresh = Renderer(device=0)
    try:
        img = bl.card("loguniform", 67, 45)
        _assert_debug_equals_host(fresh, img, bl.options(**ON), "before any render")
        _render(fresh, scenes.cornell_scene("bench"))
        acc, base = fresh.readbackAccumulator(), fresh.readbackRenderTarget()
        fresh.debugBloom(img, options=bl.options(**ON))
        assert np.array_equal(fresh.readbackRenderTarget(), base) and np.array_equal(_bits(fresh.readbackAccumulator()), _bits(acc))
    finally:
        fresh.close()


# ---- a rendered Cornell --------------------------------------------------------------------------------------------------------------------
def _check_target(r, sc, size, src, post=None, what=""):
    """The target, read and presented, equals the oracle's post-process of the host bloom of `src` (the image the target shows, already
    scaled where auto exposure is on) with the renderer's bloom options."""
    po, to = post or (r.postProcessOptions(), r.tonemapOptions())
    target = _oracle_target(sc, size, bl.host_bloom(src, r.bloomOptions()), po, to)
    got = r.readbackRenderTarget()
    bad = (got != target).any(axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first (y, x) %s: device %s, oracle %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:2].tolist(), target[bad][:2].tolist())
    assert np.array_equal(_present(r), target), what + ", presented"
    return target


def test_rendered_cornell_target(r):
    sc = scenes.cornell_scene("bench")
    _render(r, sc)
    acc = r.readbackAccumulator()
    plain = r.readbackRenderTarget()
    r.setBloomOptions(**ON)
    t = _check_target(r, sc, SIZE, acc, what="agx")
    assert (t != plain).any(axis=-1).mean() > 0.25
    po, to = r.postProcessOptions(), r.tonemapOptions()
    to.tonemapper = abi.TONEMAP_KHRONOS_PBR
    po.exposure, po.contrast, po.saturation = 0.7, 12.0, -8.0
    r.setPostProcessOptions(po)
    r.setTonemapOptions(to)
    _check_target(r, sc, SIZE, acc, post=(po, to), what="khronos, graded")
    po.ca_amount = 40.0     # chromatic aberration reads neighbours of the bloomed image
    r.setPostProcessOptions(po)
    _check_target(r, sc, SIZE, acc, post=(po, to), what="khronos, chromatic aberration")
    to.tonemapper = abi.TONEMAP_AGX
    r.setTonemapOptions(to)
    _check_target(r, sc, SIZE, acc, post=(po, to), what="agx, chromatic aberration")
    r.setBloomOptions(bl.options(enabled=1))      # the defaults, switched on
    _check_target(r, sc, SIZE, acc, post=(po, to), what="default options")
    assert np.array_equal(_bits(r.readbackAccumulator()), _bits(acc))


def test_bloom_runs_after_auto_exposure(r):
    sc = scenes.cornell_scene("bench")
    _render(r, sc)
    acc = r.readbackAccumulator()
    r.setExposureOptions(enabled=1)
    m = r.readbackExposureMeter()
    r.setBloomOptions(**ON)
    assert m.gain != 1.0
    _check_target(r, sc, SIZE, _scaled(acc, m.gain), what="auto exposure")
    m2 = r.readbackExposureMeter()      # the meter sees the image ahead of bloom
    assert (m2.metered, m2.weighted, m2.gain, list(m2.bins)) == (m.metered, m.weighted, m.gain, list(m.bins))


def test_bloom_of_the_denoised_target(r):
    sc = scenes.cornell_scene("bench")
    r.setDenoiseOptions(enabled=1, apply_to_target=1)
    _render(r, sc)
    den, acc = r.readbackDenoised(), r.readbackAccumulator()
    assert not np.array_equal(_bits(den), _bits(acc))
    r.setBloomOptions(**ON)
    _check_target(r, sc, SIZE, den, what="apply_to_target")
    assert np.array_equal(_bits(r.readbackDenoised()), _bits(den)) and np.array_equal(_bits(r.readbackAccumulator()), _bits(acc))


def test_region_render_scatters_light_into_the_zeros_outside(r):
    sc, rect = scenes.cornell_scene("bench"), (5, 3, 45, 30)      # test_gpu_region.py's unaligned rectangle
    r.setRenderRegion(*rect)
    _render(r, sc, SIZE, 2)
    acc = r.readbackAccumulator()
    inside = rl.mask(*SIZE, rect)
    assert not _bits(acc)[~inside].any()
    zeros = _oracle_target(sc, SIZE, np.zeros_like(acc), r.postProcessOptions(), r.tonemapOptions())
    assert np.array_equal(r.readbackRenderTarget()[~inside], zeros[~inside])
    r.setBloomOptions(**ON)
    t = _check_target(r, sc, SIZE, acc, what="region")
    assert (t[~inside][:, :3] != zeros[~inside][:, :3]).any()            # light outside the rectangle ...
    assert np.array_equal(t[~inside][:, 3], zeros[~inside][:, 3])        # ... under the alpha bytes of a zero pixel
    assert not _bits(bl.host_bloom(acc, r.bloomOptions()))[~inside][:, 3].any()


def test_device_group_blooms_the_merged_image():
    sc = scenes.cornell_scene("bench")
    g = Renderer(devices=[0, 0])
    try:
        _render(g, sc, SIZE, 6)
        acc = g.readbackAccumulator()
        plain = g.readbackRenderTarget()
        g.setBloomOptions(**ON)
        t = _check_target(g, sc, SIZE, acc, what="group")
        assert not np.array_equal(t, plain)
        g.setBloomOptions(enabled=0)
        assert np.array_equal(g.readbackRenderTarget(), plain)
        assert np.array_equal(_bits(g.readbackAccumulator()), _bits(acc))
    finally:
        g.close()


# ---- unchanged when off --------------------------------------------------------------------------------------------------------------------
def test_disabled_before_and_after_an_enabled_read_is_a_renderer_without_bloom(r):
    sc = scenes.cornell_scene("bench")
    fresh = Renderer(device=0)      # never enables bloom
    try:
        fresh.setDenoiseOptions(enabled=1)
        _render(fresh, sc)
        base_acc, base, base_den = fresh.readbackAccumulator(), fresh.readbackRenderTarget(), fresh.readbackDenoised()
        base_meter = fresh.readbackExposureMeter()
    finally:
        fresh.close()
    r.setDenoiseOptions(enabled=1)
    _render(r, sc)
    acc = r.readbackAccumulator()
    assert np.array_equal(_bits(acc), _bits(base_acc))
    r.setBloomOptions(enabled=0, intensity=0.9, threshold=0.1)
    before, before_presented = r.readbackRenderTarget(), _present(r)
    r.setBloomOptions(enabled=1)
    on = r.readbackRenderTarget()
    # the accumulator, the denoised image and the meter with bloom on ...
    m = r.readbackExposureMeter()
    assert np.array_equal(_bits(r.readbackAccumulator()), _bits(acc)) and np.array_equal(_bits(r.readbackDenoised()), _bits(base_den))
    assert bytes(m) == bytes(base_meter)
    r.setBloomOptions(enabled=0, levels=3)
    after, after_presented = r.readbackRenderTarget(), _present(r)
    for img in (before, before_presented, after, after_presented):
        assert np.array_equal(img, base)
    assert not np.array_equal(on, base)
    # ... and off
    assert np.array_equal(_bits(r.readbackAccumulator()), _bits(acc)) and np.array_equal(_bits(r.readbackDenoised()), _bits(base_den))
    assert bytes(r.readbackExposureMeter()) == bytes(base_meter)


# ---- restarts and refusals -----------------------------------------------------------------------------------------------------------------
def test_options_change_between_reads_and_a_restart_at_another_size(r):
    sc = scenes.cornell_scene("bench")
    _render(r, sc)
    acc = r.readbackAccumulator()
    r.setBloomOptions(**ON)
    a = _check_target(r, sc, SIZE, acc, what="first options")
    r.setBloomOptions(intensity=0.8, threshold=0.0, knee=0.0, scatter=1.0, levels=12)      # no restart
    b = _check_target(r, sc, SIZE, acc, what="second options")
    assert not np.array_equal(a, b)
    big = (131, 97)     # a larger pyramid and scratch image than the first render's
    _render(r, sc, big, 2)
    _check_target(r, sc, big, r.readbackAccumulator(), what="restart, larger")
    small = (33, 17)
    _render(r, sc, small, 2)
    _check_target(r, sc, small, r.readbackAccumulator(), what="restart, smaller")


def test_errors():
    lib = abi.load_library()
    sc = scenes.cornell_scene("bench")
    fresh = Renderer(device=0)
    try:
        fresh.setBloomOptions(**ON)     # the options are accepted before pt_start_render; a target is not
        out = np.zeros((45, 67, 4), np.uint8)
        assert lib.pt_read_render_target(fresh._h, out.ctypes.data) == -5 and b"pt_start_render" in lib.pt_last_error()      # PT_ERR_BAD_STATE
        dev, stream = C.c_void_p(), C.c_void_p()
        assert lib.pt_present_render_target(fresh._h, C.byref(dev), C.byref(stream)) == -5 and b"pt_start_render" in lib.pt_last_error()
        _render(fresh, sc)
        on = fresh.readbackRenderTarget()
        img = np.ones((4, 4, 4), np.float32)
        res = np.zeros((4, 4, 4), np.float32)

        def still_works():
            assert np.array_equal(fresh.readbackRenderTarget(), on)

        for bad in (dict(intensity=1.5), dict(threshold=-1.0), dict(knee=float("nan")), dict(scatter=0.0), dict(levels=0), dict(levels=13)):
            o = bl.options(enabled=1, **bad)
            assert lib.pt_set_bloom_options(fresh._h, C.byref(o)) == -1      # PT_ERR_INVALID_ARGUMENT
            assert lib.pt_debug_bloom(fresh._h, img.ctypes.data, 4, 4, C.byref(o), res.ctypes.data, None) == -1
            still_works()
        o = bl.options()
        assert lib.pt_set_bloom_options(fresh._h, None) == -1
        assert lib.pt_debug_bloom(fresh._h, None, 4, 4, C.byref(o), res.ctypes.data, None) == -1
        assert lib.pt_debug_bloom(fresh._h, img.ctypes.data, 4, 4, None, res.ctypes.data, None) == -1
        assert lib.pt_debug_bloom(fresh._h, img.ctypes.data, 4, 4, C.byref(o), None, None) == -1
        assert lib.pt_debug_bloom(fresh._h, img.ctypes.data, 0, 4, C.byref(o), res.ctypes.data, None) == -1
        still_works()
        assert lib.pt_debug_bloom(fresh._h, img.ctypes.data, 4, 4, C.byref(o), res.ctypes.data, None) == 0      # (pyramid_out may be null)
        assert np.array_equal(_bits(res), _bits(bl.host_bloom(img, o)))
        still_works()
    finally:
        fresh.close()
