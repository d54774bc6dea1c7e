"""GPU: auto exposure (include/ptamd.h pt_exposure_options, platinum_amd/csrc/exposure.hip).  pt_debug_exposure equals the host build of
pt_exposure.h (tests/emu/exposure_emu.cpp) bit for bit, record and scaled image, over sizes, cards and rectangles; on renders the meter
equals the host meter of the read-back image and the target equals the oracle's post-process of (image * gain), read and presented, on
plain, denoised, region, adaptive, NaN, GMoN and device-group renders; enabled = 0 leaves a renderer without the feature; smoothing and
reset; errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import exposure_lib as ex  # noqa: E402
import oracle_lib  # noqa: E402
import region_lib as rl  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer, make_params  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
B = 4
SIZE, SPP = (33, 17), 4      # the rendered Cornell `bench` of most tests below


def _restore(r):
    r.clearRenderRegion()
    for struct, default, setter in ((abi.ExposureOptions, "pt_default_exposure_options", r.setExposureOptions),
                                    (abi.DespeckleOptions, "pt_default_despeckle_options", r.setDespeckleOptions),
                                    (abi.AdaptiveOptions, "pt_default_adaptive_options", r.setAdaptiveOptions),
                                    (abi.DenoiseOptions, "pt_default_denoise_options", r.setDenoiseOptions)):
        o = struct()
        getattr(r._lib, default)(C.byref(o))
        setter(o)
    r.resetExposure()
    r.setPostProcessOptions(r.postProcessOptions())
    r.setTonemapOptions(r.tonemapOptions())
    r.setGmonOptions(cap=1.0)
    r.selectKernel(abi.INTEGRATOR_MIS)


@pytest.fixture
def r(gpu_renderer):
    _restore(gpu_renderer)
    yield gpu_renderer
    _restore(gpu_renderer)      # the session's renderer goes on with auto exposure disabled and no previous ev


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


def _assert_debug_equals_host(r, img, rect, o, what):
    got, got_scaled = r.debugExposure(img, rect=rect, options=o)
    want, want_scaled = ex.host_meter(img, rect=rect, o=o)
    ex.assert_same_record(got, want, what)
    bad = (_bits(got_scaled) != _bits(want_scaled)).any(axis=-1)
    assert not bad.any(), "%s: %d scaled pixels differ, first (y, x) %s: device %s, host %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got_scaled[bad][:2].tolist(), want_scaled[bad][:2].tolist())
    return got


# ---- pt_debug_exposure against the host build ----------------------------------------------------------------------------------------------
# 1x1; 15x9: a partial block; 16x16: one block; 17x33: three blocks, the last partial; 1x40: one pixel per row; 67x45; 256x4: rows as wide as
# a block, 1024 pixels
@pytest.mark.parametrize("size", [(1, 1), (15, 9), (16, 16), (17, 33), (1, 40), (67, 45), (256, 4)])
def test_debug_exposure_equals_the_host_build_on_a_log_uniform_card(r, size):
    w, h = size
    img = ex.log_uniform_card(w, h, seed=w * 131 + h)
    for o in (ex.options(), ex.options(low_fraction=0.0, high_fraction=1.0, target_log2=3.0), ex.options(low_fraction=0.3, high_fraction=0.31, max_ev=1.0)):
        m = _assert_debug_equals_host(r, img, None, o, "%dx%d" % size)
        assert m.metered + m.below + m.above + m.nonfinite == w * h


def test_debug_exposure_on_the_special_value_card(r):
    card = ex.special_card()       # 1 row of 523 pixels: wider than two blocks
    m = _assert_debug_equals_host(r, card, None, ex.options(), "special card")
    assert m.below and m.above and m.nonfinite >= 3 and m.metered > 500
    tall = np.ascontiguousarray(card.transpose(1, 0, 2))      # the same pixels, one per row
    ex.assert_same_record(r.debugExposure(tall, options=ex.options(), scaled=False)[0], m, "special card, transposed")


def test_debug_exposure_on_a_constant_and_a_two_value_image(r):
    """Every lane of every wave in one bin (the per-wave aggregation's case), then two bins per wave in runs of 5 pixels."""
    const = np.tile(np.array([0.37, 0.37, 0.37, 0.5], np.float32), (64, 64, 1))
    m = _assert_debug_equals_host(r, const, None, ex.options(), "constant")
    assert m.metered == 4096 and np.count_nonzero(np.array(m.bins[:])) == 1
    two = const.copy()
    two[:, (np.arange(64) // 5) % 2 == 1, :3] = 11.0
    m = _assert_debug_equals_host(r, two, None, ex.options(), "two values")
    assert sorted(np.array(m.bins[:])[np.array(m.bins[:]) > 0].tolist()) == [64 * 30, 64 * 34]
    black = np.zeros((16, 16, 4), np.float32)       # nothing metered: gain 1
    m = _assert_debug_equals_host(r, black, None, ex.options(), "black")
    assert (m.metered, m.below, m.gain) == (0, 256, 1.0)


# NULL; the issue's rectangle; one pixel (the last one); columns 1..5 (no edge on a 4-pixel boundary), one row, one column
@pytest.mark.parametrize("rect", [None, (3, 2, 14, 9), (16, 32, 17, 33), (1, 1, 6, 32), (2, 7, 15, 8), (9, 0, 10, 33)])
def test_debug_exposure_over_a_rectangle(r, rect):
    img = ex.log_uniform_card(17, 33, seed=7)
    img[5, 4] = np.nan          # inside the issue's rectangle
    img[0, 0, :3] = 0.0         # outside it
    o = ex.options(smoothing=0.9)       # pt_debug_exposure runs without a smoothing state: ev = target_ev
    m = _assert_debug_equals_host(r, img, rect, o, str(rect))
    x0, y0, x1, y1 = rect or (0, 0, 17, 33)
    assert m.metered + m.below + m.above + m.nonfinite == (x1 - x0) * (y1 - y0) and m.ev == m.target_ev
    ex.assert_matches_numpy(m, img, rect, ex.options(), what=str(rect))


def test_debug_exposure_needs_no_render_and_leaves_the_renderer_alone():
    fresh = Renderer(device=0)
    try:
        img = ex.log_uniform_card(67, 45, seed=2)
        _assert_debug_equals_host(fresh, img, (5, 3, 45, 30), ex.options(), "before any render")
        _render(fresh, scenes.cornell_scene("bench"))
        acc = fresh.readbackAccumulator()
        fresh.setExposureOptions(enabled=1, smoothing=0.5)
        fresh.debugExposure(img)
        m = fresh.readbackExposureMeter()
        assert m.ev == m.target_ev      # the debug run left no previous ev behind
        assert np.array_equal(_bits(fresh.readbackAccumulator()), _bits(acc))
    finally:
        fresh.close()


# ---- a rendered Cornell --------------------------------------------------------------------------------------------------------------------
def _check_target(r, sc, size, src, rect=None, opts=None, prev_ev=None, post=None, what=""):
    """The device meter equals the host meter of `src` (the read-back image the target shows); the target, read and presented, equals the
    oracle's post-process of src * gain with the gain of the device's record.  post = the (post, tonemap) options set on the renderer
    (default: the defaults).  Returns the record."""
    po, to = post or (r.postProcessOptions(), r.tonemapOptions())
    opts = r.exposureOptions() if opts is None else opts
    m = r.readbackExposureMeter()
    want, _ = ex.host_meter(src, rect=rect, o=opts, prev_ev=prev_ev, scaled=False)
    ex.assert_same_record(m, want, what)
    target = _oracle_target(sc, size, _scaled(src, m.gain), po, to)
    got = r.readbackRenderTarget()
    bad = (got != target).any(axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first (y, x) %s: device %s, oracle %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:2].tolist(), target[bad][:2].tolist())
    if prev_ev is None:     # (with a smoothing state the read above has advanced it: the next target applies another ev)
        assert np.array_equal(_present(r), target), what + ", presented"
    return m


def test_rendered_cornell_meter_and_target(r):
    sc = scenes.cornell_scene("bench")
    _render(r, sc)
    acc = r.readbackAccumulator()
    plain = r.readbackRenderTarget()
    r.setExposureOptions(enabled=1)
    m = _check_target(r, sc, SIZE, acc, what="defaults")
    assert m.metered > 400 and m.gain != 1.0 and not np.array_equal(r.readbackRenderTarget(), plain)
    # a non-default tonemapper with grading, the user's exposure as compensation on top, then chromatic aberration (it reads neighbours of
    # the scaled image)
    po, to = r.postProcessOptions(), r.tonemapOptions()
    to.tonemapper = abi.TONEMAP_KHRONOS_PBR
    po.exposure, po.contrast, po.saturation = 0.7, 12.0, -8.0
    po.vig_amount, po.vig_midpoint = -1.5, 10.0
    r.setPostProcessOptions(po)
    r.setTonemapOptions(to)
    _check_target(r, sc, SIZE, acc, post=(po, to), what="khronos, graded")
    po.ca_amount = 40.0
    to.tonemapper = abi.TONEMAP_FLIM
    r.setPostProcessOptions(po)
    r.setTonemapOptions(to)
    _check_target(r, sc, SIZE, acc, post=(po, to), what="flim, chromatic aberration")
    r.setExposureOptions(target_log2=1.0, low_fraction=0.4, high_fraction=0.6, max_ev=2.5)
    _check_target(r, sc, SIZE, acc, post=(po, to), what="other options")
    assert np.array_equal(_bits(r.readbackAccumulator()), _bits(acc))


def test_disabled_before_and_after_an_enabled_read_is_a_renderer_without_auto_exposure(r):
    sc = scenes.cornell_scene("bench")
    fresh = Renderer(device=0)      # never enables auto exposure
    try:
        _render(fresh, sc)
        base_acc, base = fresh.readbackAccumulator(), fresh.readbackRenderTarget()
    finally:
        fresh.close()
    _render(r, sc)
    acc = r.readbackAccumulator()
    assert np.array_equal(_bits(acc), _bits(base_acc))
    r.setExposureOptions(enabled=0, target_log2=5.0)
    before, before_presented = r.readbackRenderTarget(), _present(r)
    r.setExposureOptions(enabled=1)
    on = r.readbackRenderTarget()
    r.readbackExposureMeter()
    r.setExposureOptions(enabled=0, smoothing=0.5)
    after, after_presented = r.readbackRenderTarget(), _present(r)
    for img in (before, before_presented, after, after_presented):
        assert np.array_equal(img, base)
    assert not np.array_equal(on, base)
    assert np.array_equal(_bits(r.readbackAccumulator()), _bits(acc))


# ---- combinations --------------------------------------------------------------------------------------------------------------------------
def test_denoised_target_is_metered_and_the_denoised_image_stays_unscaled(r):
    sc = scenes.cornell_scene("bench")
    r.setDenoiseOptions(enabled=1, apply_to_target=1)
    _render(r, sc)
    den, acc = r.readbackDenoised(), r.readbackAccumulator()
    assert not np.array_equal(_bits(den), _bits(acc))
    r.setExposureOptions(enabled=1)
    _check_target(r, sc, SIZE, den, what="apply_to_target")
    assert np.array_equal(_bits(r.readbackDenoised()), _bits(den)) and np.array_equal(_bits(r.readbackAccumulator()), _bits(acc))
    for k in (abi.AOV_ALBEDO, abi.AOV_MOMENTS):
        assert np.isfinite(r.readbackAov(k)).all()
    r.setDenoiseOptions(apply_to_target=0)      # AOVs kept, but the target shows the accumulator: so does the meter
    _check_target(r, sc, SIZE, acc, what="AOVs without apply_to_target")


def test_region_render_meters_the_region_only(r):
    sc, size, rect = scenes.cornell_scene("bench"), (67, 45), (5, 3, 45, 30)      # test_gpu_region.py's unaligned rectangle
    r.setRenderRegion(*rect)
    _render(r, sc, size, 2)
    acc = r.readbackAccumulator()
    inside = rl.mask(*size, rect)
    assert not _bits(acc)[~inside].any()
    r.setExposureOptions(enabled=1)
    m = _check_target(r, sc, size, acc, rect=rect, what="region")
    assert m.metered + m.below + m.above + m.nonfinite == (rect[2] - rect[0]) * (rect[3] - rect[1])
    whole, _ = ex.host_meter(acc, o=ex.options(), scaled=False)
    assert whole.below > m.below        # the zeros outside the region are not even counted
    zeros = _oracle_target(sc, size, np.zeros_like(acc), r.postProcessOptions(), r.tonemapOptions())
    assert np.array_equal(r.readbackRenderTarget()[~inside], zeros[~inside])


def test_adaptive_render(r):
    kind, size, bounces, spp, m_, i, thr, policy = al.config("cornell67")
    r.setAdaptiveOptions(enabled=1, threshold=thr, min_spp=m_, interval=i)
    sc = al.config_scene(kind)
    _render(r, sc, size, spp, bounces=bounces, nonfinite_policy=policy)
    assert len(np.unique(r.readbackSampleCounts())) >= 3
    r.setExposureOptions(enabled=1)
    _check_target(r, sc, size, r.readbackAccumulator(), what="adaptive")


@pytest.mark.parametrize("policy", [abi.NONFINITE_PROPAGATE, abi.NONFINITE_ZERO])
def test_render_with_nan_samples(r, policy):
    """test_gpu_nonfinite.py's scene.  With PT_NONFINITE_PROPAGATE the NaN samples reach the accumulator: the meter counts those pixels as
    nonfinite (> 0), they stay NaN in the scaled image and the post-process shows them black.  With PT_NONFINITE_ZERO the samples are dropped
    before the accumulator, which is then finite: the meter has nothing non-finite to count."""
    seed, size, spp = 24, (71, 45), 24
    sc = scenes.random_scene(seed)
    _render(r, sc, size, spp, bounces=3 + seed % 7, nonfinite_policy=policy)
    acc = r.readbackAccumulator()
    nan = np.isnan(acc).any(axis=-1)
    r.setExposureOptions(enabled=1)
    m = _check_target(r, sc, size, acc, what="policy %d" % policy)
    assert m.nonfinite == int((~np.isfinite(ex.np_lum(acc))).sum())
    if policy == abi.NONFINITE_PROPAGATE:
        assert m.nonfinite > 0 and nan.any()
        assert (r.readbackRenderTarget()[nan] == np.array([0, 0, 0, 255], np.uint8)).all()
    else:
        assert m.nonfinite == 0 and not nan.any()


def test_gmon_render(r):
    sc = scenes.cornell_scene("bench")
    _render(r, sc, SIZE, 8, gmonBuckets=4, flags=abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON)
    r.setExposureOptions(enabled=1)
    _check_target(r, sc, SIZE, r.readbackAccumulator(), what="GMoN")


# ---- smoothing -----------------------------------------------------------------------------------------------------------------------------
def test_smoothing_across_reads_and_a_restart(r):
    sc, sc2 = scenes.cornell_scene("bench"), scenes.cornell_scene("default")
    _render(r, sc)
    acc = r.readbackAccumulator()
    o1 = ex.options(enabled=1, smoothing=0.5)
    o2 = ex.options(enabled=1, smoothing=0.5, target_log2=0.0)
    r.setExposureOptions(o1)
    # first use: no previous ev, the target applies its own target_ev (two meter reads first: they do not advance anything)
    for _ in range(2):
        m = r.readbackExposureMeter()
        assert m.ev == m.target_ev
    e1 = _check_target(r, sc, SIZE, acc, opts=o1, what="first read").ev         # also presents: smoothing from e1 to the same target stays at e1
    t1 = ex.host_meter(acc, o=o1, scaled=False)[0].target_ev
    assert e1 == t1
    # second read, towards another target: the recurrence from e1; meter reads in between show it and do not advance it
    r.setExposureOptions(o2)
    want2 = ex.host_meter(acc, o=o2, prev_ev=e1, scaled=False)[0]
    assert want2.ev == f32(e1) + f32(0.5) * (f32(want2.target_ev) - f32(e1)) and want2.ev != want2.target_ev
    for _ in range(2):
        ex.assert_same_record(r.readbackExposureMeter(), want2, "meter between reads")
    e2 = _check_target(r, sc, SIZE, acc, opts=o2, prev_ev=e1, what="second read").ev
    # a restart with another camera keeps the state
    _render(r, sc2)
    acc2 = r.readbackAccumulator()
    want3 = ex.host_meter(acc2, o=o2, prev_ev=e2, scaled=False)[0]
    assert want3.ev != want3.target_ev
    e3 = _check_target(r, sc2, SIZE, acc2, opts=o2, prev_ev=e2, what="after the restart").ev
    ex.assert_same_record(r.readbackExposureMeter(), ex.host_meter(acc2, o=o2, prev_ev=e3, scaled=False)[0], "state after the third read")
    # a reset forgets it
    r.resetExposure()
    m = r.readbackExposureMeter()
    assert m.ev == m.target_ev == ex.host_meter(acc2, o=o2, scaled=False)[0].target_ev
    _check_target(r, sc2, SIZE, acc2, opts=o2, what="after the reset")


# ---- device group --------------------------------------------------------------------------------------------------------------------------
def test_device_group_meters_the_merged_image():
    sc = scenes.cornell_scene("bench")
    g = Renderer(devices=[0, 0])
    try:
        _render(g, sc, SIZE, 6)
        acc = g.readbackAccumulator()
        plain = g.readbackRenderTarget()
        g.setExposureOptions(enabled=1)
        m = _check_target(g, sc, SIZE, acc, what="group")
        assert m.gain != 1.0
        g.setExposureOptions(enabled=0)
        assert np.array_equal(g.readbackRenderTarget(), plain)
        assert np.array_equal(_bits(g.readbackAccumulator()), _bits(acc))
    finally:
        g.close()


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    lib = abi.load_library()
    sc = scenes.cornell_scene("bench")
    fresh = Renderer(device=0)
    try:
        m = abi.ExposureMeter()
        assert lib.pt_read_exposure_meter(fresh._h, C.byref(m)) == -5 and b"pt_start_render" in lib.pt_last_error()     # PT_ERR_BAD_STATE
        assert lib.pt_reset_exposure(fresh._h) == 0         # nothing to forget yet
        _render(fresh, sc)
        base = fresh.readbackRenderTarget()
        fresh.setExposureOptions(enabled=1)
        on = fresh.readbackRenderTarget()
        img = np.ones((4, 4, 4), np.float32)

        def still_works():
            assert np.array_equal(fresh.readbackRenderTarget(), on) and not np.array_equal(on, base)

        for bad in (dict(smoothing=1.0), dict(low_fraction=0.95), dict(max_ev=40.0), dict(target_log2=float("nan"))):
            o = ex.options(enabled=1, **bad)
            assert lib.pt_set_exposure_options(fresh._h, C.byref(o)) == -1      # PT_ERR_INVALID_ARGUMENT
            assert lib.pt_debug_exposure(fresh._h, img.ctypes.data, 4, 4, None, C.byref(o), C.byref(m), None) == -1
            still_works()
        o = ex.options()
        assert lib.pt_set_exposure_options(fresh._h, None) == -1
        assert lib.pt_read_exposure_meter(fresh._h, None) == -1
        assert lib.pt_debug_exposure(fresh._h, None, 4, 4, None, C.byref(o), C.byref(m), None) == -1
        assert lib.pt_debug_exposure(fresh._h, img.ctypes.data, 4, 4, None, None, C.byref(m), None) == -1
        assert lib.pt_debug_exposure(fresh._h, img.ctypes.data, 4, 4, None, C.byref(o), None, None) == -1
        assert lib.pt_debug_exposure(fresh._h, img.ctypes.data, 0, 4, None, C.byref(o), C.byref(m), None) == -1
        rect = (C.c_uint32 * 4)(0, 0, 5, 4)
        assert lib.pt_debug_exposure(fresh._h, img.ctypes.data, 4, 4, C.addressof(rect), C.byref(o), C.byref(m), None) == -1
        still_works()
        assert lib.pt_debug_exposure(fresh._h, img.ctypes.data, 4, 4, None, C.byref(o), C.byref(m), None) == 0 and m.metered == 16
        still_works()
    finally:
        fresh.close()
