"""GPU: render regions.  A region render is a restriction of the full-frame render: inside the rectangle every output
holds the bits of the render without a region (the oracle's running mean, the host build's AOVs, the device's own full-frame render),
outside it everything is all-zero bits, alpha included; the denoiser filters the rectangle as an image of its own; adaptive sampling
judges a tile over its pixels inside the rectangle (region_lib.reference_region_render, made without the device)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import denoise_lib as dl  # noqa: E402
import oracle_lib  # noqa: E402
import region_lib as rl  # noqa: E402
from platinum_amd import abi  # noqa: E402
from platinum_amd.renderer import Renderer, make_params  # noqa: E402

pytestmark = pytest.mark.gpu

AOVS = (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)
KEYS = ("acc", "albedo", "normal", "moments")
W, H, B = 67, 45, 4                       # cornell67's scene and size
RECTS = [(5, 3, 45, 30), (8, 8, 40, 32), (66, 44, 67, 45), (31, 0, 32, 45), (0, 0, 67, 45)]
R0 = RECTS[0]


def _restore(r):
    r.clearRenderRegion()
    o = abi.AdaptiveOptions()
    r._lib.pt_default_adaptive_options(C.byref(o))
    r.setAdaptiveOptions(o)
    d = abi.DenoiseOptions()
    r._lib.pt_default_denoise_options(C.byref(d))
    r.setDenoiseOptions(d)
    r.setPostProcessOptions(r.postProcessOptions())
    r.setTonemapOptions(r.tonemapOptions())
    r.selectKernel(abi.INTEGRATOR_MIS)


@pytest.fixture
def r(gpu_renderer):
    _restore(gpu_renderer)
    yield gpu_renderer
    _restore(gpu_renderer)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _scene():
    return al.config_scene("cornell")


def _drive(r, step):
    """step = 0: everything at once; else render(step) until the render is done."""
    if step == 0:
        r.render(0)
    else:
        while r.status() & abi.STATUS_DONE == 0:
            r.render(step)


def _render(r, rect, spp, aov=False, step=0, size=(W, H), bounces=B, scene=None, **kw):
    """A uniform render of the rectangle (None: no region), finished."""
    if rect is None:
        r.clearRenderRegion()
    else:
        r.setRenderRegion(*rect)
    r.setAdaptiveOptions(enabled=0)
    r.setDenoiseOptions(enabled=1 if aov else 0)
    r.startRender(_scene() if scene is None else scene, size, spp, max_bounces=bounces, **kw)
    _drive(r, step)
    r.wait()
    assert r.status() & abi.STATUS_DONE and r.renderProgress() == (spp, spp)


def _state(r, aov=False):
    out = dict(counts=r.readbackSampleCounts(), acc=r.readbackAccumulator())
    if aov:
        for key, k in zip(KEYS[1:], AOVS):
            out[key] = r.readbackAov(k)
    st = r.stats()
    out["paths"], out["nonfinite"] = st.paths, st.nonfinite_samples
    return out


@functools.lru_cache(maxsize=None)
def _oracle(spp, first=0, integrator=abi.INTEGRATOR_MIS):
    """The oracle's running mean of the whole frame (read only) and the non-finite samples it met."""
    o = oracle_lib.OracleScene(_scene(), make_params(W, H, spp, B, first_sample=first, integrator=integrator))
    try:
        acc = o.render(first, spp)
        nonfinite = o.stats().nonfinite
    finally:
        o.close()
    acc.flags.writeable = False
    return acc, nonfinite


@functools.lru_cache(maxsize=None)
def _host(spp):
    """(acc, albedo, normal, moments) of the whole frame on the host build (read only)."""
    out = dl.HostScene(_scene(), make_params(W, H, spp, B)).render(0, spp)
    for a in out:
        a.flags.writeable = False
    return tuple(out)


_FULL = {}


def _device_full(r, spp):
    """The device's own render without a region: once per spp."""
    if spp not in _FULL:
        _render(r, None, spp)
        _FULL[spp] = _state(r)
    return _FULL[spp]


def _assert_restriction(got, want_acc, rect, spp, what="", size=(W, H)):
    """got = a uniform region render: inside the rectangle the bits of want_acc, the count spp; outside zero bits and no samples."""
    w, h = size
    inside = rl.mask(w, h, rect)
    bad = (_bits(got["acc"]) != _bits(want_acc)).any(axis=-1) & inside
    assert not bad.any(), "%s: %d pixels of the region differ, first (y, x) %s" % (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert not _bits(got["acc"])[~inside].any(), what + ": outside the region"
    assert (got["acc"][inside][:, 3] == 1.0).all()
    assert (got["counts"][inside] == spp).all() and not got["counts"][~inside].any(), what
    assert got["paths"] == int(inside.sum()) * spp, (what, got["paths"])


# ---- uniform renders ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [6, 37])
@pytest.mark.parametrize("rect", RECTS)
def test_uniform_region_is_a_restriction_of_the_full_render(r, rect, spp):
    want, nonfinite = _oracle(spp)
    full = _device_full(r, spp)
    assert np.array_equal(_bits(full["acc"]), _bits(want)) and full["paths"] == W * H * spp
    _render(r, rect, spp)
    got = _state(r)
    _assert_restriction(got, want, rect, spp, "oracle")
    _assert_restriction(got, full["acc"], rect, spp, "full-frame device render")
    assert got["nonfinite"] == full["nonfinite"] == nonfinite == 0
    if rect == (0, 0, W, H):      # the full-frame region: every output of the render without a region
        assert np.array_equal(_bits(got["acc"]), _bits(full["acc"])) and np.array_equal(got["counts"], full["counts"])
        assert got["paths"] == full["paths"]


@pytest.mark.parametrize("sif", [1, 3, 128])
@pytest.mark.parametrize("step", [0, 1, 5])
def test_region_does_not_depend_on_batching(r, sif, step):
    spp = 37
    _render(r, R0, spp, step=step, samples_in_flight=sif)
    assert r.stats().samples_in_flight == min(sif, spp)
    _assert_restriction(_state(r), _oracle(spp)[0], R0, spp, "sif %d step %d" % (sif, step))


def test_region_with_first_sample_1000(r):
    want = _oracle(6, first=1000)[0]
    assert not np.array_equal(_bits(want), _bits(_oracle(6)[0]))
    _render(r, R0, 6, first_sample=1000)
    _assert_restriction(_state(r), want, R0, 6, "first_sample 1000")


def test_region_with_the_simple_integrator(r):
    want = _oracle(6, integrator=abi.INTEGRATOR_SIMPLE)[0]
    assert not np.array_equal(_bits(want), _bits(_oracle(6)[0]))
    r.selectKernel(abi.INTEGRATOR_SIMPLE)
    _render(r, R0, 6)
    _assert_restriction(_state(r), want, R0, 6, "SIMPLE")


@pytest.mark.parametrize("bands", [1, 7])
def test_region_under_other_queue_layouts(bands):
    """3 tiles per segment: the region's virtual tiles share segments, and the last segment that holds one is partly empty."""
    preset = [v for v in ("PTAMD_TILES_PER_SEG", "PTAMD_SEG_BANDS") if v in os.environ]
    if preset:
        pytest.skip("preset for the whole session: " + ", ".join(preset))
    spp = 37
    os.environ["PTAMD_TILES_PER_SEG"], os.environ["PTAMD_SEG_BANDS"] = "3", str(bands)
    try:
        rr = Renderer(device=0)
    finally:
        del os.environ["PTAMD_TILES_PER_SEG"], os.environ["PTAMD_SEG_BANDS"]
    try:
        _render(rr, R0, spp, aov=True)
        got = _state(rr, aov=True)
    finally:
        rr.close()
    _assert_restriction(got, _oracle(spp)[0], R0, spp, "3 tiles per segment, %d bands" % bands)
    inside = rl.mask(W, H, R0)
    for key, w in zip(KEYS, _host(spp)):
        assert np.array_equal(_bits(got[key])[inside], _bits(w)[inside]) and not _bits(got[key])[~inside].any(), key


# ---- AOVs --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rect", RECTS)
def test_region_aovs_equal_the_host_render_inside_and_zero_outside(r, rect):
    spp = 6
    want = _host(spp)
    assert np.array_equal(_bits(want[0]), _bits(_oracle(spp)[0]))
    _render(r, rect, spp)
    off = _state(r)
    _render(r, rect, spp, aov=True)
    got = _state(r, aov=True)
    assert np.array_equal(_bits(got["acc"]), _bits(off["acc"]))          # the accumulator: the same bits with AOVs on or off
    assert got["paths"] == off["paths"]
    inside = rl.mask(W, H, rect)
    for key, w in zip(KEYS, want):
        bad = (_bits(got[key]) != _bits(w)).any(axis=-1) & inside
        assert not bad.any(), "%s: %d pixels differ, first (y, x) %s" % (key, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert not _bits(got[key])[~inside].any(), key + " outside the region"


# ---- the denoiser ------------------------------------------------------------------------------------------------------------------------
def _crop(a, rect):
    x0, y0, x1, y1 = rect
    return np.ascontiguousarray(a[y0:y1, x0:x1])


def _assert_denoised(den, want_crop, rect, what):
    inside = rl.mask(*den.shape[1::-1], rect)
    got = _crop(den, rect)
    bad = (_bits(got) != _bits(want_crop)).any(axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first (y, x) of the crop %s" % (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert not _bits(den)[~inside].any(), what + ": outside the region"


@pytest.mark.parametrize("rect", RECTS)
def test_region_denoised_is_the_host_filter_on_the_crop(r, rect):
    spp = 37
    imgs = _host(spp)
    _render(r, rect, spp, aov=True)
    for it in (1, 5):
        r.setDenoiseOptions(iterations=it)
        want = dl.host_filter(*[_crop(a, rect) for a in imgs], spp, iterations=it)
        _assert_denoised(r.readbackDenoised(), want, rect, "%d iterations" % it)
        if rect == (66, 44, 67, 45):      # a single pixel has no tap but itself: its accumulator pixel
            acc = r.readbackAccumulator()
            assert np.array_equal(_bits(r.readbackDenoised()[44, 66, :3]), _bits(acc[44, 66, :3]))
    r.setDenoiseOptions(iterations=0)
    want = _crop(imgs[0], rect).copy()
    want[..., 3] = 1.0
    _assert_denoised(r.readbackDenoised(), want, rect, "0 iterations")
    if rect not in ((66, 44, 67, 45), (0, 0, W, H)):
        # the filter saw the rectangle only: the full frame's filter, cropped, differs at its border
        full = dl.host_filter(*imgs, spp, iterations=5)
        assert not np.array_equal(_bits(_crop(full, rect)), _bits(dl.host_filter(*[_crop(a, rect) for a in imgs], spp, iterations=5)))


def _start_adaptive(r, name, rect, aov=True, **kw):
    kind, size, bounces, spp, m, i, thr, policy = al.config(name)
    r.setRenderRegion(*rect)
    r.setDenoiseOptions(enabled=1 if aov else 0)
    r.setAdaptiveOptions(enabled=1, threshold=thr, min_spp=m, interval=i)
    r.startRender(al.config_scene(kind), size, spp, max_bounces=bounces, nonfinite_policy=policy, **kw)


def test_adaptive_region_denoised_uses_each_pixels_own_count(r):
    """A tile-aligned rectangle: the crop's tiles are the image's, so adaptive_lib.host_filter_counts (which reads a count per tile of the
    image it is given) filters the crop with each pixel's own count."""
    name, rect = "cornell67", (8, 8, 40, 32)
    ref = rl.reference_region_render(name, rect)
    assert len(np.unique(ref["counts"][rl.mask(W, H, rect)])) >= 3
    _start_adaptive(r, name, rect)
    r.render(0)
    r.wait()
    assert np.array_equal(r.readbackSampleCounts(), ref["counts"])
    for it in (1, 5):
        r.setDenoiseOptions(iterations=it)
        want = al.host_filter_counts(*[_crop(ref[k], rect) for k in KEYS], _crop(ref["counts"], rect), iterations=it)
        _assert_denoised(r.readbackDenoised(), want, rect, "adaptive, %d iterations" % it)


# ---- adaptive sampling with a region -----------------------------------------------------------------------------------------------------
def _adaptive_state(r):
    out = _state(r, aov=True)
    return out


def _assert_is_region_reference(got, ref, what, nan=False):
    assert np.array_equal(got["counts"], ref["counts"]), what + " counts"
    for key in KEYS:
        same = al.same_bits_or_both_nan(got[key], ref[key]) if nan else _bits(got[key]) == _bits(ref[key])
        bad = ~same.all(axis=-1)
        assert not bad.any(), "%s %s: %d pixels differ, first (y, x) %s" % (what, key, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert got["paths"] == ref["paths"], what
    assert got["nonfinite"] == int(ref["nonfinite"].sum()), what


@pytest.mark.parametrize("name", ["cornell67", "textured99"])
@pytest.mark.parametrize("sif", [1, 3, 128])
def test_adaptive_region_equals_the_host_reference(r, name, sif):
    rect = rl.REGIONS[name]
    ref = rl.reference_region_render(name)
    spp = al.config(name)[3]
    assert len(np.unique(ref["counts"])) >= 6 and ref["counts"].max() == spp       # 0 outside and at least 5 classes inside
    _start_adaptive(r, name, rect, samples_in_flight=sif)
    _drive(r, {1: 5, 3: 0, 128: 1}[sif])
    r.wait()
    assert r.status() & abi.STATUS_DONE
    _assert_is_region_reference(_adaptive_state(r), ref, "%s sif %d" % (name, sif))


@pytest.mark.parametrize("name,at", [("cornell67", 20), ("textured99", 24)])
def test_adaptive_region_with_blocking_reads_in_the_middle(r, name, at):
    rect = rl.REGIONS[name]
    ref = rl.reference_region_render(name)
    _size, spp = al.config(name)[1], al.config(name)[3]
    _start_adaptive(r, name, rect)
    r.render(at)
    mid = _adaptive_state(r)
    inside = rl.mask(_size[0], _size[1], rect)
    assert np.array_equal(mid["counts"], np.minimum(ref["counts"], at)) and not mid["counts"][~inside].any()
    assert r.renderProgress() == (at, spp) and r.status() & abi.STATUS_DONE == 0
    stopped = inside & (ref["counts"] <= at)
    assert stopped.any() and np.array_equal(_bits(mid["acc"])[stopped], _bits(ref["acc"])[stopped])
    r.render(0)
    r.wait()
    _assert_is_region_reference(_adaptive_state(r), ref, "%s after reads at %d" % (name, at))


def test_adaptive_region_with_nan_samples(r):
    name = "nan996"
    rect = rl.REGIONS[name]
    _kind, (w, h), _B, spp, _m, _i, _t, policy = al.config(name)
    assert policy == abi.NONFINITE_PROPAGATE
    inside = rl.mask(w, h, rect)
    assert inside[34, 7] and inside[43, 30]               # both NaN pixels, (7, 34) and (30, 43), lie in the region
    ref = rl.reference_region_render(name)
    nan = np.isnan(ref["acc"]).any(axis=-1)
    assert nan[34, 7] and nan[43, 30] and int(nan.sum()) == 2 and int(ref["nonfinite"].sum()) >= 2
    _start_adaptive(r, name, rect)
    r.render(0)
    r.wait()
    got = _adaptive_state(r)
    _assert_is_region_reference(got, ref, name, nan=True)
    assert np.array_equal(np.isnan(got["acc"]).any(axis=-1), nan)


# ---- present -----------------------------------------------------------------------------------------------------------------------------
def _present(r):
    ptr, stream = r.presentRenderTarget()
    assert ptr and stream
    r.wait()
    hip = abi.load_library()
    got = np.empty((H, W, 4), np.uint8)
    assert hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
    assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), C.c_void_p(ptr), C.c_size_t(got.nbytes), 2) == 0  # hipMemcpyDeviceToHost
    return got


def test_render_target_is_the_oracles_postprocess_of_the_region_image(r):
    spp = 37
    _render(r, R0, spp, aov=True)
    acc = r.readbackAccumulator()
    inside = rl.mask(W, H, R0)
    assert not _bits(acc)[~inside].any()
    o = oracle_lib.OracleScene(_scene(), make_params(W, H, spp, B))
    try:
        for tm, ca in ((abi.TONEMAP_AGX, 0.0), (abi.TONEMAP_AGX, 40.0), (abi.TONEMAP_FLIM, 40.0)):
            po, to = r.postProcessOptions(), r.tonemapOptions()
            to.tonemapper = tm
            po.ca_amount = ca
            po.vig_amount, po.vig_midpoint = -1.5, 10.0
            r.setPostProcessOptions(po)
            r.setTonemapOptions(to)
            r.setDenoiseOptions(apply_to_target=0)
            want = o.postprocess(acc, po, to)
            assert np.array_equal(r.readbackRenderTarget(), want), (tm, ca)
            assert np.array_equal(_present(r), want), (tm, ca, "presented")
            if ca:     # chromatic aberration reads neighbours: the region's border pixels see the zeros outside
                assert (want != o.postprocess(_oracle(spp)[0], po, to)).any(axis=-1)[inside].any()
            r.setDenoiseOptions(apply_to_target=1)
            den = r.readbackDenoised()
            assert not _bits(den)[~inside].any() and not np.array_equal(_bits(den), _bits(acc))
            want = o.postprocess(den, po, to)
            assert np.array_equal(r.readbackRenderTarget(), want), (tm, ca, "apply_to_target")
            assert np.array_equal(_present(r), want), (tm, ca, "apply_to_target, presented")
    finally:
        o.close()


# ---- restarts, debug batches, refusals ---------------------------------------------------------------------------------------------------
def test_restarts_among_region_adaptive_both_and_neither(r):
    spp = 6
    want = _oracle(spp)[0]
    # region -> another region
    for rect in (R0, (31, 0, 32, 45)):
        _render(r, rect, spp)
        _assert_restriction(_state(r), want, rect, spp, "region %s" % (rect,))
    # -> no region: the plain render
    _render(r, None, spp)
    got = _state(r)
    assert np.array_equal(_bits(got["acc"]), _bits(want)) and (got["counts"] == spp).all() and got["paths"] == W * H * spp
    # -> region with adaptive sampling
    name = "cornell67"
    _start_adaptive(r, name, rl.REGIONS[name])
    r.render(0)
    r.wait()
    _assert_is_region_reference(_adaptive_state(r), rl.reference_region_render(name), "region with adaptive")
    # -> adaptive alone: the full-frame adaptive render
    r.clearRenderRegion()
    _kind, size, bounces, aspp, m, i, thr, _p = al.config(name)
    r.startRender(al.config_scene(_kind), size, aspp, max_bounces=bounces)
    r.render(0)
    r.wait()
    full = al.reference(name)
    assert np.array_equal(r.readbackSampleCounts(), full["counts"]) and np.array_equal(_bits(r.readbackAccumulator()), _bits(full["acc"]))
    # -> region alone, after adaptive
    _render(r, (8, 8, 40, 32), spp, aov=True)
    _assert_restriction(_state(r), want, (8, 8, 40, 32), spp, "region after adaptive")
    # -> plain
    _render(r, None, spp)
    got = _state(r)
    assert np.array_equal(_bits(got["acc"]), _bits(want)) and (got["counts"] == spp).all() and got["paths"] == W * H * spp


def test_trace_primary_in_the_middle_of_a_region_render_is_full_frame(r):
    spp = 37
    r.clearRenderRegion()
    r.setAdaptiveOptions(enabled=0)
    r.setDenoiseOptions(enabled=0)
    r.startRender(_scene(), (W, H), spp, max_bounces=B)
    r.render(20)
    r.wait()
    want = r.tracePrimary(3)
    rad_want = r.debugSample(3)[0]
    assert (want["instance"] >= 0).any()
    r.setRenderRegion(*R0)
    r.startRender(_scene(), (W, H), spp, max_bounces=B)
    r.render(20)
    r.wait()
    got = r.tracePrimary(3)
    assert got.tobytes() == want.tobytes()
    assert r.debugSample(3)[0].tobytes() == rad_want.tobytes()
    r.measureTraversal(0)
    r.render(0)
    r.wait()
    _assert_restriction(_state(r), _oracle(spp)[0], R0, spp, "after debug batches")


def test_refusals(r):
    lib = r._lib
    sc = _scene()
    snap = sc.snapshot()
    # GMoN with a region: refused at start
    r.setRenderRegion(*R0)
    p = make_params(W, H, 8, B, flags=abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON, gmon_buckets=4)
    assert lib.pt_start_render(r._h, C.byref(snap.struct), C.byref(p)) == -6 and b"GMON" in lib.pt_last_error()
    # a region that does not fit the image: invalid at start, and the message names the region
    for rect in ((5, 3, W + 1, 30), (5, 3, 45, H + 1)):
        r.setRenderRegion(*rect)
        p = make_params(W, H, 8, B)
        assert lib.pt_start_render(r._h, C.byref(snap.struct), C.byref(p)) == -1 and b"region" in lib.pt_last_error(), rect
    # an empty region: invalid at set, and the region in effect stays
    bad = abi.RenderRegion(1, 5, 3, 5, 30)
    assert lib.pt_set_render_region(r._h, C.byref(bad)) == -1
    r.setRenderRegion(*R0)
    _render(r, R0, 6)
    _assert_restriction(_state(r), _oracle(6)[0], R0, 6, "after the refusals")
    # a device group: refused at set; a disabled region is accepted
    g = Renderer(devices=[0, 0])
    try:
        o = abi.RenderRegion(1, *R0)
        assert lib.pt_set_render_region(g._h, C.byref(o)) == -6 and b"group" in lib.pt_last_error()
        g.clearRenderRegion()
    finally:
        g.close()


# ---- two tiles per segment ---------------------------------------------------------------------------------------------------------------
def test_full_size_region_two_tiles_per_segment(r):
    w, h, spp = 2051, 1029, 4
    rect = (1001, 500, 1900, 1029)
    q = abi.QueuePlan()
    abi.check(r._lib, r._lib.pt_plan_queues(w, h, spp, 0, 200 << 30, 0, 4, C.byref(q)))
    assert q.tiles_per_seg == 2
    _render(r, None, spp, size=(w, h))
    full = _state(r)
    assert full["paths"] == w * h * spp
    _render(r, rect, spp, size=(w, h))
    got = _state(r)
    _assert_restriction(got, full["acc"], rect, spp, "2051x1029", size=(w, h))
    assert got["paths"] == (1900 - 1001) * (1029 - 500) * spp
