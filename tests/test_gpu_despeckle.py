"""GPU: the denoiser's firefly clamp (include/ptamd.h pt_despeckle_options, platinum_amd/csrc/denoise.hip k_dn_despeckle).
pt_read_denoised equals the host build of the filter with the clamp (tests/emu/despeckle_emu.cpp) on the device's own accumulator, AOVs
and counts, bit for bit, on whole frames, a region render, an adaptive render and a scene with NaN samples; a disabled clamp leaves the
bits of a renderer that never enabled it; the present path; errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import denoise_lib as dl  # noqa: E402
import despeckle_lib as ds  # noqa: E402
import oracle_lib  # noqa: E402
import region_lib as rl  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer, make_params  # noqa: E402

pytestmark = pytest.mark.gpu

AOVS = (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)
B = 4


def _restore(r):
    r.clearRenderRegion()
    for struct, default, setter in ((abi.DespeckleOptions, "pt_default_despeckle_options", r.setDespeckleOptions),
                                    (abi.AdaptiveOptions, "pt_default_adaptive_options", r.setAdaptiveOptions),
                                    (abi.DenoiseOptions, "pt_default_denoise_options", r.setDenoiseOptions)):
        o = struct()
        getattr(r._lib, default)(C.byref(o))
        setter(o)
    r.setPostProcessOptions(r.postProcessOptions())
    r.setTonemapOptions(r.tonemapOptions())
    r.selectKernel(abi.INTEGRATOR_MIS)


@pytest.fixture
def r(gpu_renderer):
    _restore(gpu_renderer)
    yield gpu_renderer
    _restore(gpu_renderer)      # the session's renderer goes on with the clamp disabled


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _render(r, sc, size, spp, bounces=B, **kw):
    r.setDenoiseOptions(enabled=1)
    r.startRender(sc, size, spp, max_bounces=bounces, **kw)
    r.render(0)
    r.wait()


def _inputs(r):
    """The device's own read-back accumulator and AOVs."""
    return [r.readbackAccumulator()] + [r.readbackAov(k) for k in AOVS]


def _assert_same(got, want, what, nan=False):
    same = al.same_bits_or_both_nan(got, want) if nan else _bits(got) == _bits(want)
    bad = ~same.all(axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first (y, x) %s: device %s, host %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:2].tolist(), want[bad][:2].tolist())


# 15x9: one partial block; 16x16: exactly one; 17x33: 2 x 3 blocks, one pixel wide at the right; 1x40: no horizontal neighbour; 67x45
@pytest.mark.parametrize("spp", [1, 6])
@pytest.mark.parametrize("size", [(15, 9), (16, 16), (17, 33), (1, 40), (67, 45)])
def test_denoised_equals_the_host_filter_with_the_clamp(r, size, spp):
    _render(r, scenes.cornell_scene("bench"), size, spp)
    imgs = _inputs(r)
    N = r.renderProgress()[0]
    assert N == spp
    for it in (1, 5):
        r.setDenoiseOptions(iterations=it)
        off = dl.host_filter(*imgs, N, iterations=it)
        for t in (1.0, 2.0, 8.0):
            r.setDespeckleOptions(enabled=1, threshold=t)
            got = r.readbackDenoised()
            want = ds.host_filter(*imgs, N, iterations=it, enabled=1, threshold=t)
            _assert_same(got, want, "%dx%d %d spp, %d iterations, threshold %g" % (size + (spp, it, t)))
            if t == 1.0:    # every strict local maximum of the luminance is clamped: the clamp took part
                assert not np.array_equal(_bits(want), _bits(off)), (size, spp, it)


def test_iterations_zero_returns_the_accumulator_with_the_clamp_enabled(r):
    _render(r, scenes.cornell_scene("bench"), (17, 33), 1)
    acc = r.readbackAccumulator()
    r.setDenoiseOptions(iterations=0)
    r.setDespeckleOptions(enabled=1, threshold=1.0)
    assert np.array_equal(_bits(r.readbackDenoised()), _bits(acc))


def test_disabled_before_and_after_an_enabled_read_is_a_renderer_without_the_clamp(r):
    sc, size, spp = scenes.cornell_scene("bench"), (67, 45), 1
    fresh = Renderer(device=0)      # never enables the clamp
    try:
        _render(fresh, sc, size, spp)
        base = fresh.readbackDenoised()
        base_target = fresh.readbackRenderTarget()
    finally:
        fresh.close()
    _render(r, sc, size, spp)
    assert np.array_equal(_bits(base), _bits(dl.host_filter(*_inputs(r), spp)))
    before = r.readbackDenoised()
    r.setDespeckleOptions(enabled=1)                # takes effect at the next read: no restart
    on = r.readbackDenoised()
    r.setDespeckleOptions(enabled=0, threshold=8.0)
    after = r.readbackDenoised()
    assert np.array_equal(_bits(before), _bits(base)) and np.array_equal(_bits(after), _bits(base))
    assert not np.array_equal(_bits(on), _bits(base))
    assert np.array_equal(r.readbackRenderTarget(), base_target)


def test_region_render_skips_neighbours_outside_the_region(r):
    size, rect, spp = (67, 45), (5, 3, 45, 30), 1      # test_gpu_region.py's unaligned rectangle
    r.setRenderRegion(*rect)
    _render(r, scenes.cornell_scene("bench"), size, spp)
    imgs = _inputs(r)
    inside = rl.mask(*size, rect)
    assert not _bits(imgs[0])[~inside].any()
    for t in (1.0, 2.0):
        r.setDespeckleOptions(enabled=1, threshold=t)
        got = r.readbackDenoised()
        _assert_same(got, ds.host_filter(*imgs, spp, enabled=1, threshold=t, rect=rect), "region, threshold %g" % t, nan=True)
        assert not _bits(got)[~inside].any()
    # the region's border pixels took their limit from inside the region only: the full frame's filter, cropped, differs
    r.clearRenderRegion()
    _render(r, scenes.cornell_scene("bench"), size, spp)
    full = ds.host_filter(*_inputs(r), spp, enabled=1, threshold=2.0)
    assert not np.array_equal(_bits(full[inside]), _bits(got[inside]))


def test_adaptive_render_with_per_tile_counts(r):
    kind, size, bounces, spp, m, i, thr, policy = al.config("cornell67")
    r.setAdaptiveOptions(enabled=1, threshold=thr, min_spp=m, interval=i)
    _render(r, al.config_scene(kind), size, spp, bounces=bounces, nonfinite_policy=policy)
    imgs, counts = _inputs(r), r.readbackSampleCounts()
    assert len(np.unique(counts)) >= 3
    for it in (1, 5):
        r.setDenoiseOptions(iterations=it)
        r.setDespeckleOptions(enabled=1, threshold=1.0)
        want = ds.host_filter(*imgs, 0, iterations=it, enabled=1, threshold=1.0, counts=counts)
        _assert_same(r.readbackDenoised(), want, "adaptive, %d iterations" % it, nan=True)
        assert not np.array_equal(_bits(want), _bits(al.host_filter_counts(*imgs, counts, iterations=it)))


def test_scene_with_nan_samples(r):
    seed, size, spp = 24, (71, 45), 24
    _render(r, scenes.random_scene(seed), size, spp, bounces=3 + seed % 7, nonfinite_policy=abi.NONFINITE_PROPAGATE)
    imgs = _inputs(r)
    nan = np.isnan(imgs[0]).any(axis=-1)
    assert nan.any() and not nan.all()
    for t in (1.0, 2.0):
        r.setDespeckleOptions(enabled=1, threshold=t)
        got = r.readbackDenoised()
        _assert_same(got, ds.host_filter(*imgs, spp, enabled=1, threshold=t), "random_scene(24), threshold %g" % t, nan=True)
        assert np.array_equal(np.isnan(got).any(axis=-1), nan)      # a NaN pixel stays where it is and reaches no other


def test_render_target_and_present_show_the_clamped_image(r):
    sc, (w, h), spp = scenes.cornell_scene("bench"), (67, 45), 1
    _render(r, sc, (w, h), spp)
    r.setDenoiseOptions(apply_to_target=1)
    unclamped = r.readbackRenderTarget()
    r.setDespeckleOptions(enabled=1, threshold=2.0)
    den = ds.host_filter(*_inputs(r), spp, enabled=1, threshold=2.0)
    o = oracle_lib.OracleScene(sc, make_params(w, h, spp, B))
    try:
        want = o.postprocess(den, r.postProcessOptions(), r.tonemapOptions())
    finally:
        o.close()
    target = r.readbackRenderTarget()
    assert np.array_equal(target, want) and not np.array_equal(target, unclamped)
    ptr, stream = r.presentRenderTarget()
    assert ptr and stream
    r.wait()
    hip = abi.load_library()
    got = np.empty((h, w, 4), np.uint8)
    assert hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
    assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), C.c_void_p(ptr), C.c_size_t(got.nbytes), 2) == 0  # hipMemcpyDeviceToHost
    assert np.array_equal(got, want)


def test_errors(r):
    lib = r._lib
    for t in (0.5, 0.0, -1.0, float("inf"), float("nan")):
        bad = abi.DespeckleOptions(1, t)
        assert lib.pt_set_despeckle_options(r._h, C.byref(bad)) == -1 and b"threshold" in lib.pt_last_error(), t   # PT_ERR_INVALID_ARGUMENT
    assert lib.pt_set_despeckle_options(r._h, None) == -1
    assert lib.pt_set_despeckle_options(r._h, C.byref(abi.DespeckleOptions(1, 1.0))) == 0
    g = Renderer(devices=[0, 0])
    try:
        o = g.despeckleOptions()
        o.enabled = 1
        assert lib.pt_set_despeckle_options(g._h, C.byref(o)) == -6 and b"group" in lib.pt_last_error()     # PT_ERR_UNSUPPORTED
        o.enabled = 0
        assert lib.pt_set_despeckle_options(g._h, C.byref(o)) == 0
        assert lib.pt_set_despeckle_options(g._h, C.byref(abi.DespeckleOptions(0, 0.5))) == -1
    finally:
        g.close()
