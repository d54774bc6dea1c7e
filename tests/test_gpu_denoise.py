"""GPU: first-hit AOVs and the a-trous denoiser (include/ptamd.h ABI 5, platinum_amd/csrc/denoise.hip).
AOVs change no existing result; the AOV images are bit-identical however the samples are batched and equal the host build of
stage_aov / lum; pt_read_denoised equals the host build of the filter on the device's own inputs; the present path; errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_lib as dl  # noqa: E402
import oracle_lib  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer, make_params  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def r(gpu_renderer):
    yield gpu_renderer
    o = abi.DenoiseOptions()
    gpu_renderer._lib.pt_default_denoise_options(C.byref(o))
    gpu_renderer.setDenoiseOptions(o)
    gpu_renderer.setGmonOptions(cap=1.0)


def _render(r, sc, w, h, spp, bounces, aov, batches=None, **kw):
    r.setDenoiseOptions(enabled=1 if aov else 0)
    r.startRender(sc, (w, h), spp, max_bounces=bounces, **kw)
    if batches is None:
        r.render(0)
    else:
        for b in batches:
            r.render(b)
            r.wait()
    r.wait()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", ["cornell", "textured", "gmon"])
def test_aovs_change_no_existing_result(r, name):
    if name == "cornell":
        sc, w, h, spp, b, kw = scenes.cornell_scene("bench"), 128, 96, 16, 4, {}
    elif name == "textured":
        sc, w, h, spp, b, kw = scenes.textured_scene(), 96, 54, 8, 6, {}
    else:
        sc, w, h, spp, b, kw = scenes.cornell_scene("bench"), 80, 72, 16, 4, dict(flags=abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON, gmonBuckets=4)
    outs = []
    for aov in (False, True):
        r.setDenoiseOptions(apply_to_target=0)
        _render(r, sc, w, h, spp, b, aov, **kw)
        outs.append((r.readbackAccumulator(), r.readbackRenderTarget()))
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0]))
    assert np.array_equal(outs[0][1], outs[1][1])


def test_aov_images_do_not_depend_on_batching(r):
    sc = scenes.cornell_scene("bench")
    got = []
    for batches, sif in ((None, 128), ([16] * 8, 16), ([24] * 5 + [8], 24)):
        _render(r, sc, 72, 40, 128, 4, True, batches=batches, samples_in_flight=sif)
        got.append([r.readbackAov(k) for k in (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)])
    for k in range(3):
        assert np.array_equal(_bits(got[0][k]), _bits(got[1][k])), k
        assert np.array_equal(_bits(got[0][k]), _bits(got[2][k])), k


@pytest.mark.parametrize("name", ["cornell", "textured"])
def test_one_sample_aovs_equal_the_host_stage(r, name):
    sc, w, h, b = (scenes.cornell_scene("bench"), 64, 48, 4) if name == "cornell" else (scenes.textured_scene(), 96, 54, 6)
    _render(r, sc, w, h, 1, b, True)
    alb, nrm, mom = (r.readbackAov(k) for k in (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS))
    hits = r.tracePrimary(0)
    rad, _ = r.debugSample(0)
    hs = dl.HostScene(sc, make_params(w, h, 1, b))
    a_host, n_host = hs.stage_aov(0, hits)
    assert (hits["instance"] >= 0).any()
    assert np.array_equal(_bits(alb[..., :3]), _bits(a_host[..., :3]))
    assert np.array_equal(_bits(nrm), _bits(n_host))
    assert np.array_equal(_bits(mom[..., 0]), _bits(a_host[..., 3]))
    lum, lum2 = dl.host_lum(rad)
    assert np.array_equal(_bits(mom[..., 1]), _bits(lum)) and np.array_equal(_bits(mom[..., 2]), _bits(lum2))


def _inputs(r):
    acc = r.readbackAccumulator()
    a, n, m = (r.readbackAov(k) for k in (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS))
    return acc, a, n, m, r.renderProgress()[0]


@pytest.mark.parametrize("iters,gmon", [(1, False), (5, False), (5, True), (0, False), (8, True)])
def test_denoised_equals_host_filter_on_the_devices_inputs(r, iters, gmon):
    kw = dict(flags=abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON, gmonBuckets=3) if gmon else {}
    _render(r, scenes.textured_scene(), 333, 217, 6, 5, True, **kw)
    r.setDenoiseOptions(iterations=iters)
    got = r.readbackDenoised()
    acc, a, n, m, N = _inputs(r)
    want = dl.host_filter(acc, a, n, m, N, iterations=iters)
    assert np.array_equal(_bits(got), _bits(want))


def test_denoised_full_size_c3_rows(r):
    _render(r, scenes.field_scene(), 1920, 1080, 128, 8, True)
    got = r.readbackDenoised()
    acc, a, n, m, N = _inputs(r)
    rows = slice(500, 580)   # the filter's support at 5 iterations is 2 * (1 + 2 + 4 + 8 + 16) = 62 rows: feed it 62 rows of margin
    lo, hi = rows.start - 62, rows.stop + 62
    want = dl.host_filter(acc[lo:hi], a[lo:hi], n[lo:hi], m[lo:hi], N)
    assert np.array_equal(_bits(got[rows]), _bits(want[rows.start - lo: rows.stop - lo]))


def test_render_target_and_present_show_the_denoised_image(r):
    sc = scenes.cornell_scene("bench")
    w, h = 96, 80
    _render(r, sc, w, h, 4, 4, True)
    r.setDenoiseOptions(apply_to_target=1)
    den = r.readbackDenoised()
    target = r.readbackRenderTarget()
    o = oracle_lib.OracleScene(sc, make_params(w, h, 4, 4))
    assert np.array_equal(target, o.postprocess(den, r.postProcessOptions(), r.tonemapOptions()))
    ptr, stream = r.presentRenderTarget()
    assert ptr and stream
    r.wait()
    hip = abi.load_library()
    got = np.empty((h, w, 4), np.uint8)
    assert hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
    assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), C.c_void_p(ptr), C.c_size_t(got.nbytes), 2) == 0  # hipMemcpyDeviceToHost
    assert np.array_equal(got, target)


def test_errors(r):
    lib = r._lib
    _render(r, scenes.cornell_scene("bench"), 32, 32, 2, 4, False)
    buf = np.zeros((32, 32, 4), np.float32)
    assert lib.pt_read_aov(r._h, abi.AOV_ALBEDO, buf.ctypes.data) == -5      # PT_ERR_BAD_STATE
    assert lib.pt_read_denoised(r._h, buf.ctypes.data) == -5
    base = r.denoiseOptions()
    for field, value in (("iterations", 9), ("sigma_luminance", 0.0), ("sigma_normal", -1.0), ("sigma_depth", float("inf")),
                         ("sigma_luminance", float("nan"))):
        o = r.denoiseOptions()
        setattr(o, field, value)
        assert lib.pt_set_denoise_options(r._h, C.byref(o)) == -1, field   # PT_ERR_INVALID_ARGUMENT
    assert lib.pt_set_denoise_options(r._h, C.byref(base)) == 0
    _render(r, scenes.cornell_scene("bench"), 32, 32, 2, 4, True)
    assert lib.pt_read_aov(r._h, 3, buf.ctypes.data) == -1


def test_device_group_refuses_aovs_and_v4_create_still_works():
    g = Renderer(devices=[0, 0])
    try:
        o = g.denoiseOptions()
        o.enabled = 1
        assert g._lib.pt_set_denoise_options(g._h, C.byref(o)) == -6     # PT_ERR_UNSUPPORTED
        o.enabled = 0
        assert g._lib.pt_set_denoise_options(g._h, C.byref(o)) == 0
    finally:
        g.close()
    lib = abi.load_library()
    info = abi.CreateInfo()
    info.abi_version = 4
    info.device_ordinal = 0
    info.lut_path = abi.LUT_PATH.encode()
    h = C.c_void_p()
    assert lib.pt_create(C.byref(info), C.byref(h)) == 0 and h.value
    lib.pt_destroy(h)
