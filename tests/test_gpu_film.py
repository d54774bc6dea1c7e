"""GPU: the transparent film against an independent reference — the oracle's debug_sample(s) masked by
trace_primary(s)["instance"] >= 0 and folded by the float32 numpy restatement of tests/film_lib.py — bit for bit, however the samples are
batched; the cross-checks against the accumulator and the AOVs; every other output unchanged; regions, adaptive renders, non-finite samples;
the backdrop through the display chain, read and presented, against the oracle's post-process of the numpy compose of the device's own
film; and every error code.  The scene is scenes.textured_scene() (environment, soft alpha cut-outs, open sky) at 24x17 x 16 spp."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import bloom_lib as bl  # noqa: E402
import denoise_lib as dl  # noqa: E402
import exposure_lib as el  # noqa: E402
import film_lib as fl  # noqa: E402
import selection_lib as sl  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer  # noqa: E402
from test_gpu_bloom import ON as BLOOM_ON, _oracle_target, _present, _scaled  # noqa: E402
from test_nonfinite_reference import NAN_SAMPLES  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZE, SPP, BOUNCES = (24, 17), 16, 4     # 24x17: a partial tile row, and a 1-pixel-high edge tile
W, H = SIZE
INVALID, BAD_STATE, UNSUPPORTED = -1, -5, -6
SWITCHES = ("PTAMD_NO_CAMERA_LISTS", "PTAMD_TEST_CAMLIST_CAP")
AOVS = (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)
GREY = (0.18, 0.25, 0.6)


@pytest.fixture(scope="module")
def rr():
    r = Renderer(device=0)
    yield r
    r.close()


def _defaults(r):
    r.setFilmOptions(fl.options())
    r.setSelectionOptions(enabled=0)
    r.setSelection([])
    r.setExposureOptions(enabled=0)
    r.setBloomOptions(enabled=0)
    r.setDenoiseOptions(enabled=0, apply_to_target=0)
    r.resetExposure()


@pytest.fixture
def r(rr):
    _defaults(rr)
    yield rr
    _defaults(rr)


@pytest.fixture(scope="module")
def sc():
    return scenes.textured_scene()


@pytest.fixture(scope="module")
def ref(sc):
    """(L (SPP, H, W, 4), hit (SPP, H, W), the reference film (H, W, 4)), computed once and read only"""
    L, hit = fl.reference_samples(sc, SIZE, SPP, BOUNCES)
    film = fl.np_fold(L, hit)
    film.flags.writeable = False
    return L, hit, film


def _start(r, sc, size=SIZE, spp=SPP, bounces=BOUNCES, sif=0, film=True, aov=False, matte=False, region=None, adaptive=None, **kw):
    r.setFilmOptions(enabled=1 if film else 0)
    r.setDenoiseOptions(enabled=1 if aov else 0)
    r.setMatteOptions(enabled=1 if matte else 0)
    if region:
        r.setRenderRegion(*region)
    else:
        r.clearRenderRegion()
    if adaptive:
        r.setAdaptiveOptions(enabled=1, min_spp=adaptive[0], interval=adaptive[1], threshold=adaptive[2])
    else:
        r.setAdaptiveOptions(enabled=0)
    try:
        r.startRender(sc, size, spp, max_bounces=bounces, samples_in_flight=sif, **kw)
    finally:   # (these options are read at startRender: the renderer goes back to its defaults for whoever uses it next)
        r.setFilmOptions(enabled=0)
        r.setDenoiseOptions(enabled=0)
        r.setMatteOptions(enabled=0)
        r.clearRenderRegion()
        r.setAdaptiveOptions(enabled=0)


def _finish(r, steps=(0,)):
    for n in steps:
        r.render(n)
        r.wait()
    return r.readbackFilm()


def _render(r, sc, steps=(0,), **kw):
    _start(r, sc, **kw)
    return _finish(r, steps)


def _assert_film(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.float32
    assert fl.same_bits(got, want), "%s: %s" % (what, fl.first_difference(got, want))


# ---- 1. the film equals the reference ------------------------------------------------------------------------------------------------------
def test_the_reference_populates_every_class(ref):
    L, hit, film = ref
    n = hit.sum(axis=0)
    full, none, part = int((n == SPP).sum()), int((n == 0).sum()), int(((n > 0) & (n < SPP)).sum())
    print("pixels hit by all %d samples: %d, by none: %d, fractional: %d" % (SPP, full, none, part))
    assert full >= 50 and none >= 50 and part >= 30
    assert (L[~hit][:, :3].sum(axis=-1) > 0).all()                   # every missed sample carries radiance: a fold that forgets the mask fails
    assert np.array_equal(film[..., 3] == 1.0, n == SPP) and np.array_equal(film[..., 3] == 0.0, n == 0)


@pytest.mark.parametrize("way", ["one_batch", "seven_in_flight", "one_sample_calls", "restarted"])
def test_film_equals_the_reference(r, sc, ref, way):
    want = ref[2]
    if way == "one_batch":
        got = _render(r, sc, sif=SPP)
        assert r.stats().batches == 1
    elif way == "seven_in_flight":     # batches of 7, 7 and 2: no multiple of 8, n0 != 0
        got = _render(r, sc, sif=7)
        assert r.stats().samples_in_flight == 7 and r.stats().batches == 3
    elif way == "one_sample_calls":
        got = _render(r, sc, steps=(1,) * SPP)
        assert r.stats().batches == SPP
    else:                              # a render left half way, then pt_start_render again: the film starts from 0
        half = _render(r, sc, steps=(8,))
        _assert_film(half, fl.np_fold(ref[0][:8], ref[1][:8]), "half way")
        got = _render(r, sc)
    _assert_film(got, want, way)


@pytest.mark.parametrize("size,spp", [((1, 1), 1), ((9, 7), 9)])
def test_small_frames_partial_tiles_and_a_batch_that_is_no_multiple_of_eight(r, sc, size, spp):
    L, hit = fl.reference_samples(sc, size, spp, BOUNCES)
    got = _render(r, sc, size=size, spp=spp, sif=spp)
    assert r.stats().batches == 1
    _assert_film(got, fl.np_fold(L, hit), "%dx%d x %d" % (size + (spp,)))


# ---- 2. cross-checks -----------------------------------------------------------------------------------------------------------------------
def test_coverage_is_the_normal_aovs_alpha_and_full_pixels_hold_the_accumulator(r, sc, ref):
    film = _render(r, sc, sif=5, aov=True)
    _assert_film(film, ref[2], "with AOVs")
    acc, normal = r.readbackAccumulator(), r.readbackAov(abi.AOV_NORMAL)
    assert fl.same_bits(film[..., 3], normal[..., 3])
    n = ref[1].sum(axis=0)
    assert fl.same_bits(film[n == SPP][:, :3], acc[n == SPP][:, :3])
    assert not film[n == 0].any() and acc[n == 0][:, :3].all()


# ---- 3. nothing else moves -----------------------------------------------------------------------------------------------------------------
def _everything_else(r, sc, film, **kw):
    _start(r, sc, sif=5, film=film, aov=True, matte=True, **kw)
    r.render(0)
    r.wait()
    st = r.stats()
    out = [r.readbackAccumulator()] + [r.readbackAov(k) for k in AOVS]
    r.setDenoiseOptions(enabled=1)      # (the filter's options are read when the image is asked for)
    out.append(r.readbackDenoised())
    r.setDenoiseOptions(enabled=0)
    slots = [r.readbackMatteSlots(layer) for layer in (abi.MATTE_INSTANCE, abi.MATTE_MATERIAL)]
    r.setFilmOptions(backdrop=abi.BACKDROP_SCENE)
    return out, slots, r.readbackSampleCounts(), r.readbackRenderTarget(), (st.closest_rays, st.shadow_rays, st.shaded_hits, st.paths, st.nonfinite_samples, st.batches)


@pytest.mark.parametrize("gmon", [False, True])
def test_every_other_output_is_the_same_bits_with_the_film_on(r, sc, ref, gmon):
    kw = dict(flags=abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON, gmonBuckets=4) if gmon else {}
    off = _everything_else(r, sc, False, **kw)
    assert r._lib.pt_read_film(r._h, np.empty((H, W, 4), f32).ctypes.data) == BAD_STATE
    on = _everything_else(r, sc, True, **kw)
    _assert_film(r.readbackFilm(), ref[2], "GMoN %s" % gmon)          # (under GMoN the film is the plain running mean)
    assert on[4] == off[4] and on[4][3] == W * H * SPP
    assert np.array_equal(on[2], off[2]) and np.array_equal(on[3], off[3]) and (on[3][..., 3] == 255).all()
    for a, b in zip(on[1], off[1]):
        assert np.array_equal(a, b)
    for a, b in zip(on[0], off[0]):
        assert np.any(a != 0) and al.same_bits_or_both_nan(a, b).all()


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


def test_fused_and_walked_camera_rays_give_the_same_film(r, sc, ref):
    for k in SWITCHES:
        assert os.environ.get(k, "0") in ("", "0"), "this test compares the switches' two sides"
    others = [_renderer_under({"PTAMD_NO_CAMERA_LISTS": "1"})]
    try:
        built = []
        for x, what in zip([r] + others, ("fused", "no lists")):
            _start(x, sc, sif=SPP)
            built.append(x.cameraListStats().built)
            _assert_film(_finish(x), ref[2], what)
        assert built == [1, 0]
    finally:
        for x in others:
            x.close()


# ---- 4. regions and adaptive renders -------------------------------------------------------------------------------------------------------
REGION = (5, 3, 19, 14)      # not tile-aligned


def _inside(rect=REGION):
    m = np.zeros((H, W), bool)
    m[rect[1]:rect[3], rect[0]:rect[2]] = True
    return m


def test_a_region_keeps_the_full_frame_bits_inside_and_zero_outside(r, sc, ref):
    got = _render(r, sc, sif=7, region=REGION)
    inside = _inside()
    assert fl.same_bits(got[inside], ref[2][inside]) and not got[~inside].any()
    assert ref[2][~inside].any()


def test_an_adaptive_tile_holds_the_film_of_a_uniform_render_of_its_own_count(r):
    kind, _size, bounces, _spp, min_spp, interval, threshold = al.CONFIGS["textured99"]
    sc, size, spp = al.config_scene(kind), (33, 19), 64
    got = _render(r, sc, size=size, spp=spp, bounces=bounces, adaptive=(min_spp, interval, threshold))
    counts = r.readbackSampleCounts()
    classes = sorted(set(counts.ravel().tolist()))
    print("sample counts:", al.histogram(counts))
    assert len(classes) > 1 and classes[-1] <= spp and classes[0] >= min_spp, classes
    L, hit = fl.reference_samples(sc, size, spp, bounces)
    want = fl.np_fold(L, hit, counts=counts)
    _assert_film(got, want, "adaptive")
    assert ((want[..., 3] > 0) & (want[..., 3] < 1)).any()


# ---- 5. non-finite samples -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [abi.NONFINITE_PROPAGATE, abi.NONFINITE_ZERO])
def test_non_finite_samples_under_both_policies(r, policy):
    """Seed 996 of tests/test_gpu_nonfinite.py at 71x45 x 24 spp: NaN samples 0 of pixel (7, 34) and 20 of pixel (30, 43), both on camera rays
    that hit.  (None of the seeded scenes yields a NaN on a camera ray that missed: with an environment a miss is the environment's finite
    radiance.  That half of the case is held on the host, tests/test_film_host.py, where a missed NaN folds as {0, 0, 0, 0}.)"""
    seed, size, spp = 996, (71, 45), 24
    scn, bounces = scenes.random_scene(seed), 3 + seed % 7
    L, hit = fl.reference_samples(scn, size, spp, bounces)
    for s, x, y in NAN_SAMPLES[seed]:
        assert np.isnan(L[s, y, x, :3]).all() and hit[s, y, x]
    want = fl.np_fold(L, hit, policy)
    got = _render(r, scn, size=size, spp=spp, bounces=bounces, sif=5, nonfinite_policy=policy)
    bad = ~al.same_bits_or_both_nan(got, want)
    assert not bad.any(), "policy %d: %d values differ, first %s" % (policy, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    nan = np.isnan(got).any(axis=-1)
    if policy == abi.NONFINITE_PROPAGATE:
        assert sorted((int(x), int(y)) for y, x in np.argwhere(nan)) == sorted((x, y) for _s, x, y in NAN_SAMPLES[seed])
        assert np.isfinite(got[..., 3]).all()                      # the coverage of a NaN sample that hit is still 1
    else:
        assert not nan.any()
    assert r.stats().nonfinite_samples == len(NAN_SAMPLES[seed])    # counted once, by k_accumulate
    assert not got[hit.sum(axis=0) == 0].any()
    acc = r.readbackAccumulator()
    full = hit.sum(axis=0) == spp
    assert al.same_bits_or_both_nan(got[full][:, :3], acc[full][:, :3]).all()


# ---- 6. the display chain ------------------------------------------------------------------------------------------------------------------
def _target_of(r, sc, src, alpha=None, exposure=False, bloom=False):
    """The oracle's post-process of what the chain shows of the composed source `src`, with the alpha bytes of the quantised `alpha`."""
    img = src
    if exposure:
        img = _scaled(img, r.readbackExposureMeter().gain)
    if bloom:
        img = bl.host_bloom(img, r.bloomOptions())
    want = _oracle_target(sc, r.size, img, r.postProcessOptions(), r.tonemapOptions())
    if alpha is not None:
        want = want.copy()
        want[..., 3] = fl.np_quantise(alpha)
    return want


def _assert_read_and_presented(r, want, what):
    got = r.readbackRenderTarget()
    bad = (got != want).any(axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first (y, x) %s: device %s, expected %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:2].tolist(), want[bad][:2].tolist())
    assert np.array_equal(_present(r), want), what + ", presented"


def test_color_and_transparent_backdrops_and_a_change_without_a_restart(r, sc, ref):
    film = _render(r, sc)
    _assert_film(film, ref[2])
    acc = r.readbackAccumulator()
    scene_target = _target_of(r, sc, acc)
    _assert_read_and_presented(r, scene_target, "scene")
    # COLOR
    r.setFilmOptions(backdrop=abi.BACKDROP_COLOR, backdrop_rgb=GREY)
    src = fl.np_compose(film, film[..., 3], fl.COLOR, GREY)
    want = _target_of(r, sc, src)
    assert (want[..., 3] == 255).all() and (want != scene_target).any()
    _assert_read_and_presented(r, want, "color")
    # TRANSPARENT, without a restart: straight alpha
    r.setFilmOptions(backdrop=abi.BACKDROP_TRANSPARENT)
    src = fl.np_compose(film, film[..., 3], fl.TRANSPARENT)
    want = _target_of(r, sc, src, alpha=film[..., 3])
    _assert_read_and_presented(r, want, "transparent")
    zero = film[..., 3] == 0
    black = _target_of(r, sc, np.zeros_like(film))
    assert (want[zero][:, 3] == 0).all() and np.array_equal(want[zero][:, :3], black[zero][:, :3])      # rgb of alpha = 0 pixels: post(0)
    assert (want[film[..., 3] == 1][:, 3] == 255).all() and len(np.unique(want[..., 3])) > 5
    # another colour, then back to the scene: today's chain
    r.setFilmOptions(backdrop=abi.BACKDROP_COLOR, backdrop_rgb=(2.0, 0.0, 0.0))
    _assert_read_and_presented(r, _target_of(r, sc, fl.np_compose(film, film[..., 3], fl.COLOR, (2.0, 0.0, 0.0))), "red")
    r.setFilmOptions(backdrop=abi.BACKDROP_SCENE)
    _assert_read_and_presented(r, scene_target, "scene again")
    assert fl.same_bits(r.readbackFilm(), film) and fl.same_bits(r.readbackAccumulator(), acc)


@pytest.mark.parametrize("mode", [fl.COLOR, fl.TRANSPARENT])
def test_auto_exposure_bloom_and_the_meter_take_the_composed_source(r, sc, mode):
    film = _render(r, sc)
    r.setFilmOptions(backdrop=mode, backdrop_rgb=GREY)
    src = fl.np_compose(film, film[..., 3], mode, GREY)
    r.setExposureOptions(enabled=1)
    r.setBloomOptions(**BLOOM_ON)
    meter = r.readbackExposureMeter()
    want_meter, _ = el.host_meter(src, None, r.exposureOptions(), scaled=False)
    el.assert_same_record(meter, want_meter, "the meter of the composed source")
    if mode == fl.TRANSPARENT:
        assert meter.below >= int((film[..., 3] == 0).sum())           # the alpha = 0 pixels are 0: below the metered range
    r.setFilmOptions(backdrop=abi.BACKDROP_SCENE)
    assert r.readbackExposureMeter().gain != meter.gain
    r.setFilmOptions(backdrop=mode)
    want = _target_of(r, sc, src, alpha=film[..., 3] if mode == fl.TRANSPARENT else None, exposure=True, bloom=True)
    _assert_read_and_presented(r, want, "exposure + bloom, backdrop %d" % mode)


@pytest.mark.parametrize("mode", [fl.COLOR, fl.TRANSPARENT])
def test_apply_to_target_filters_the_film_in_place_of_the_accumulator(r, sc, mode):
    film = _render(r, sc, aov=True)
    a, n, m = (r.readbackAov(k) for k in AOVS)
    acc = r.readbackAccumulator()
    r.setDenoiseOptions(enabled=1, apply_to_target=1)
    r.setFilmOptions(backdrop=mode, backdrop_rgb=GREY)
    base = dl.host_filter(film, a, n, m, SPP)
    assert not fl.same_bits(base[..., :3], film[..., :3])
    want = _target_of(r, sc, fl.np_compose(base, film[..., 3], mode, GREY), alpha=film[..., 3] if mode == fl.TRANSPARENT else None)
    _assert_read_and_presented(r, want, "apply_to_target, backdrop %d" % mode)
    den = r.readbackDenoised()                                          # stays the filter of the accumulator
    assert al.same_bits_or_both_nan(den, dl.host_filter(acc, a, n, m, SPP)).all()
    r.setFilmOptions(backdrop=abi.BACKDROP_SCENE)
    _assert_read_and_presented(r, _target_of(r, sc, den), "apply_to_target, scene")


@pytest.mark.parametrize("mode", [fl.COLOR, fl.TRANSPARENT])
def test_inside_a_region_the_backdrop_and_outside_it_nothing(r, sc, ref, mode):
    film = _render(r, sc, region=REGION)
    r.setFilmOptions(backdrop=mode, backdrop_rgb=GREY)
    src = fl.np_compose(film, film[..., 3], mode, GREY, rect=REGION)
    assert not src[~_inside()].any()
    want = _target_of(r, sc, src, alpha=src[..., 3] if mode == fl.TRANSPARENT else None)
    _assert_read_and_presented(r, want, "region, backdrop %d" % mode)
    if mode == fl.TRANSPARENT:
        assert (want[~_inside()][:, 3] == 0).all()


def test_the_selection_overlay_draws_after_the_alpha_byte_and_leaves_it(r, sc):
    film = _render(r, sc, matte=True)
    r.setFilmOptions(backdrop=abi.BACKDROP_TRANSPARENT)
    plain = r.readbackRenderTarget()
    assert np.array_equal(plain[..., 3], fl.np_quantise(film[..., 3]))
    ids = [0, 1]
    r.setSelectionOptions(enabled=1, width=2.0, fill_rgba=(0.0, 0.4, 1.0, 0.5))
    r.setSelection(ids)
    cov = r.readbackMatte(abi.MATTE_INSTANCE, ids)
    assert cov.any() and not cov.all()
    want = sl.host_overlay(plain, cov, r.selectionOptions())
    assert (want[..., :3] != plain[..., :3]).any() and np.array_equal(want[..., 3], plain[..., 3])
    _assert_read_and_presented(r, want, "overlay over a transparent film")


def test_a_render_without_the_film_shows_the_accumulator_under_every_backdrop(r, sc):
    _start(r, sc, film=False)
    r.render(0)
    r.wait()
    want = _target_of(r, sc, r.readbackAccumulator())
    meters = []
    for mode in (abi.BACKDROP_SCENE, abi.BACKDROP_COLOR, abi.BACKDROP_TRANSPARENT):
        r.setFilmOptions(backdrop=mode, backdrop_rgb=GREY)
        _assert_read_and_presented(r, want, "no film, backdrop %d" % mode)
        meters.append(el.record(r.readbackExposureMeter()))
    assert (want[..., 3] == 255).all()
    assert all(np.array_equal(m["bins"], meters[0]["bins"]) for m in meters)


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------------
def test_error_codes(r, sc):
    L, h = r._lib, r._h
    out = np.empty((H, W, 4), f32)
    _render(r, sc)
    assert L.pt_read_film(h, None) == INVALID
    assert L.pt_read_film(h, out.ctypes.data) == 0
    for bad, word in ((dict(backdrop=3), b"backdrop"), (dict(backdrop_rgb=(0.0, -1.0, 0.0)), b"backdrop_rgb"),
                      (dict(backdrop_rgb=(float("nan"), 0.0, 0.0)), b"backdrop_rgb"), (dict(backdrop_rgb=(0.0, 0.0, float("inf"))), b"backdrop_rgb")):
        o = fl.options(**bad)
        assert L.pt_set_film_options(h, C.byref(o)) == INVALID and word in L.pt_last_error(), bad
    assert L.pt_set_film_options(h, None) == INVALID
    assert bytes(r.filmOptions()) == bytes(fl.options())                # a refused struct changes nothing
    fresh = Renderer(device=0)
    try:
        for started in (False, True):      # before pt_start_render; then a render started without the film
            if started:
                fresh.startRender(scenes.cornell_scene("bench"), (8, 8), 1, max_bounces=2)
            assert fresh._lib.pt_read_film(fresh._h, out.ctypes.data) == BAD_STATE
            assert b"film" in fresh._lib.pt_last_error()
    finally:
        fresh.close()
    g = Renderer(devices=[0, 0])
    try:
        o = g.filmOptions()
        o.enabled = 1
        assert g._lib.pt_set_film_options(g._h, C.byref(o)) == UNSUPPORTED and b"a device group does not keep a film" in g._lib.pt_last_error()
        o.enabled = 0
        o.backdrop = abi.BACKDROP_COLOR
        assert g._lib.pt_set_film_options(g._h, C.byref(o)) == 0
        o.backdrop = 7
        assert g._lib.pt_set_film_options(g._h, C.byref(o)) == INVALID
        assert g._lib.pt_read_film(g._h, out.ctypes.data) == BAD_STATE
    finally:
        g.close()
