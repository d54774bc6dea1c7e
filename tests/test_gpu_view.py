"""GPU: pass views.  pt_debug_view against the host build of pt_view.h on the crafted cards of tests/view_lib.py, byte for
byte with its stats; the target of real renders (read and presented) against the float32 numpy restatement fed from the renderer's own
read-backs, on a full-frame, a region, an adaptive and a many-instance render; ALBEDO against the oracle's post-process; the exposure
smoothing state under a data view; BEAUTY and the unavailable views; a device group; the selection overlay on top; and every other output
unchanged."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import view_lib as vl  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer  # noqa: E402
from test_gpu_bloom import ON as BLOOM_ON, _oracle_target, _present  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZE, SPP, BOUNCES = (33, 31), 8, 4          # five tile columns, the last one pixel wide; a last tile row of seven
W, H = SIZE
INVALID, BAD_STATE = -1, -5
AOVS = (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)
LAYERS = (abi.MATTE_INSTANCE, abi.MATTE_MATERIAL)
NAMES = abi.VIEW_NAMES


def _defaults(r):
    r.setViewOptions(vl.options())
    r.setSelectionOptions(enabled=0)
    r.setSelection([])
    r.setFilmOptions(enabled=0, backdrop=abi.BACKDROP_SCENE)
    r.setExposureOptions(enabled=0, smoothing=0.0)
    r.setBloomOptions(enabled=0)
    r.setDenoiseOptions(enabled=0, apply_to_target=0)
    r.setMatteOptions(enabled=0)
    r.setAdaptiveOptions(enabled=0)
    r.clearRenderRegion()
    r.resetExposure()


@pytest.fixture
def r(gpu_renderer):
    _defaults(gpu_renderer)
    yield gpu_renderer
    _defaults(gpu_renderer)      # the session's renderer goes on showing the beauty


@pytest.fixture(scope="module")
def cornell():
    return scenes.cornell_scene("bench")


def _start(r, sc, size=SIZE, spp=SPP, bounces=BOUNCES, aov=True, matte=True, film=True, region=None, adaptive=None, **kw):
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
    try:
        r.startRender(sc, size, spp, max_bounces=bounces, **kw)
    finally:   # (these options are read at startRender: the renderer goes back to its defaults for whoever uses it next)
        r.setDenoiseOptions(enabled=0)
        r.setMatteOptions(enabled=0)
        r.setFilmOptions(enabled=0)
        r.clearRenderRegion()
        r.setAdaptiveOptions(enabled=0)
    r.render(0)
    r.wait()


def _inputs(r, spp, layer=abi.MATTE_INSTANCE, aov=True, matte=True, film=True):
    """What the restatement reads, from the renderer's own read-backs."""
    inp = dict(counts=r.readbackSampleCounts(), spp=spp)
    if aov:
        inp["normal"], inp["moments"] = r.readbackAov(abi.AOV_NORMAL), r.readbackAov(abi.AOV_MOMENTS)
    if film:
        inp["film"] = r.readbackFilm()
    if matte:
        inp["slots"] = r.readbackMatteSlots(layer)
    return inp


def _assert_same(got, want, what):
    bad = (got != want).any(axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first (y, x) %s: device %s, expected %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:2].tolist(), want[bad][:2].tolist())


def _assert_view(r, inp, fields, rect=None, what=""):
    """The target under `fields`, read and presented, and the stats, against the restatement of `inp`.  Returns the bytes."""
    o = vl.options(**fields)
    r.setViewOptions(o)
    want, want_stats = vl.np_view(inp, o, rect)
    what = "%s %s %r" % (what, NAMES[o.view], fields)
    got = r.readbackRenderTarget()
    _assert_same(got, want, what)
    _assert_same(_present(r), want, what + ", presented")
    stats = vl.stats_tuple(r.viewStats())
    assert vl.same_stats(stats, want_stats), (what, stats, want_stats)
    return got


def _all_option_sets(view):
    return [dict(f, layer=l) for f in vl.option_sets(view)[:1] for l in LAYERS] if view == abi.VIEW_MATTE else vl.option_sets(view)


# ---- 1. pt_debug_view against the host build ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,kind,first", vl.cases(), ids=["%dx%d-%s-%d" % (s + (k, f)) for s, k, f in vl.cases()])
def test_debug_view_equals_the_host_build_byte_for_byte(r, size, kind, first):
    inp = vl.card(size, kind, first)
    w, h = size
    rects = [None] if w == 1 else [None, (3, 2, 11, 7)]
    for view in vl.DATA_VIEWS:
        for fields in vl.option_sets(view):
            for rect in rects if view == abi.VIEW_DEPTH else [None]:
                o = vl.options(**fields)
                want, want_stats = vl.host_view(inp, o, rect)
                needs = dict(counts=inp["counts"])                          # only what the view reads is handed over
                if view in (abi.VIEW_NORMAL, abi.VIEW_DEPTH):
                    needs["normal"] = inp["normal"]
                if view in (abi.VIEW_DEPTH, abi.VIEW_NOISE):
                    needs["moments"] = inp["moments"]
                if view == abi.VIEW_ALPHA:
                    needs["film"] = inp["film"]
                if view == abi.VIEW_MATTE:
                    needs["slots"] = inp["slots"]
                got, stats = r.debugView(size, options=o, rect=rect, spp=inp["spp"], **needs)
                _assert_same(got, want, "%s %r rect %r" % (NAMES[view], fields, rect))
                assert vl.same_stats(vl.stats_tuple(stats), want_stats), (NAMES[view], fields, rect, vl.stats_tuple(stats), want_stats)
    assert bytes(r.viewOptions()) == bytes(vl.options())                    # the renderer's own options are left alone


# ---- 2. a render that keeps everything ------------------------------------------------------------------------------------------------------
@pytest.fixture
def full(r, cornell):
    _start(r, cornell)
    return r


@pytest.mark.parametrize("view", vl.DATA_VIEWS, ids=[NAMES[v] for v in vl.DATA_VIEWS])
def test_every_data_view_of_a_render_equals_the_restatement_of_its_read_backs(full, view):
    r = full
    seen = []
    for fields in _all_option_sets(view):
        inp = _inputs(r, SPP, fields.get("layer", abi.MATTE_INSTANCE))
        if fields.get("auto_range") == 0:
            d, valid = vl.np_depth(inp)
            lo, hi = float(d[valid].min()), float(d[valid].max())
            fields = dict(fields, depth_min=lo + 0.25 * (hi - lo), depth_max=lo + 0.75 * (hi - lo))                 # both ends clamp
        seen.append(_assert_view(r, inp, fields))
    assert all((img[..., 3] == 255).all() for img in seen)
    assert len({img.tobytes() for img in seen}) == len(seen) or view in (abi.VIEW_NORMAL, abi.VIEW_ALPHA)        # the options matter
    if view in (abi.VIEW_NORMAL, abi.VIEW_DEPTH, abi.VIEW_NOISE, abi.VIEW_MATTE):                                  # (one instance, several materials)
        assert len(np.unique(seen[-1].reshape(-1, 4), axis=0)) > 3
    if view == abi.VIEW_DEPTH:
        st = r.viewStats()
        assert 0 < st.depth_pixels <= W * H and 0 <= st.depth_min < st.depth_max


def test_the_view_changes_without_a_restart_and_back_to_the_beauty(full):
    r = full
    beauty = r.readbackRenderTarget()
    assert r.viewStats().shown == abi.VIEW_BEAUTY
    inp = _inputs(r, SPP)
    for view in (abi.VIEW_MATTE, abi.VIEW_DEPTH, abi.VIEW_NORMAL):
        img = _assert_view(r, inp, dict(view=view))
        assert (img != beauty).any()
    r.setViewOptions(view=abi.VIEW_BEAUTY)
    _assert_same(r.readbackRenderTarget(), beauty, "beauty again")
    _assert_same(_present(r), beauty, "beauty again, presented")


# ---- 3. regions, adaptive renders, many instances ---------------------------------------------------------------------------------------------
REGION = (5, 3, 29, 26)       # not aligned to 8 at any side


def test_a_region_render_is_black_outside_and_ranges_over_the_rectangle(r, cornell):
    _start(r, cornell, region=REGION)
    inside = np.zeros((H, W), bool)
    inside[REGION[1]:REGION[3], REGION[0]:REGION[2]] = True
    for view in vl.DATA_VIEWS:
        for fields in _all_option_sets(view)[:2]:
            inp = _inputs(r, SPP, fields.get("layer", abi.MATTE_INSTANCE))
            assert not inp["counts"][~inside].any() and (inp["counts"][inside] == SPP).all()
            img = _assert_view(r, inp, fields, rect=REGION, what="region")
            assert not img[~inside][:, :3].any() and (img[..., 3] == 255).all()
            if fields.get("auto_range", 1):                                  # (the card's manual range ends in front of this box: all far, black)
                assert img[inside][:, :3].any()


def test_an_adaptive_render_shows_its_sample_counts_and_its_noise(r):
    kind, size, bounces, spp, min_spp, interval, threshold = al.CONFIGS["cornell67"]
    sc = al.config_scene(kind)
    _start(r, sc, size=size, spp=spp, bounces=bounces, matte=False, film=False, adaptive=(min_spp, interval, threshold))
    inp = _inputs(r, spp, matte=False, film=False)
    classes = sorted(set(inp["counts"].ravel().tolist()))
    print("sample counts:", al.histogram(inp["counts"]))
    assert len(classes) >= 3 and classes[-1] <= spp
    with_aovs = {}
    for view in (abi.VIEW_SAMPLES, abi.VIEW_NOISE):
        for fields in vl.option_sets(view):
            img = _assert_view(r, inp, fields, what="adaptive")
            with_aovs[repr(fields)] = img
    heat = with_aovs[repr(vl.option_sets(abi.VIEW_SAMPLES)[1])]
    assert len(np.unique(heat.reshape(-1, 4), axis=0)) == len(classes)          # one colour per tile count
    # the same render without AOVs: NOISE reads the adaptive moments, the same bits
    _start(r, sc, size=size, spp=spp, bounces=bounces, aov=False, matte=False, film=False, adaptive=(min_spp, interval, threshold))
    assert np.array_equal(r.readbackSampleCounts(), inp["counts"])
    for view in (abi.VIEW_SAMPLES, abi.VIEW_NOISE):
        for fields in vl.option_sets(view):
            r.setViewOptions(vl.options(**fields))
            assert r.viewStats().shown == view
            _assert_same(r.readbackRenderTarget(), with_aovs[repr(fields)], "adaptive without AOVs, %r" % fields)
    r.setViewOptions(vl.options(view=abi.VIEW_NORMAL))
    assert r.viewStats().shown == abi.VIEW_BEAUTY


def test_pixels_with_more_than_eight_instances_darken(r):
    """The field scene at 24x17 x 64 spp: some pixels see up to 13 instances, whose late ids found no slot."""
    size, spp = (24, 17), 64
    _start(r, scenes.field_scene(32), size=size, spp=spp, aov=False, film=False)
    for layer in LAYERS:
        inp = _inputs(r, spp, layer, aov=False, film=False)
        total = inp["slots"]["count"].sum(axis=-1)
        assert (total < spp).sum() >= 20 and (total == spp).any()
        img = _assert_view(r, inp, dict(view=abi.VIEW_MATTE, layer=layer), what="field")
        assert len(np.unique(img.reshape(-1, 4), axis=0)) > 50


# ---- 4. ALBEDO, and the exposure smoothing state ----------------------------------------------------------------------------------------------
def test_albedo_is_the_post_process_of_the_albedo_aov(full, cornell):
    r = full
    albedo = r.readbackAov(abi.AOV_ALBEDO)
    want = _oracle_target(cornell, r.size, albedo, r.postProcessOptions(), r.tonemapOptions())
    beauty = r.readbackRenderTarget()
    for exposure, bloom, backdrop in ((0, False, abi.BACKDROP_SCENE), (1, True, abi.BACKDROP_TRANSPARENT)):   # neither is applied to the albedo
        r.setExposureOptions(enabled=exposure)
        r.setBloomOptions(**(BLOOM_ON if bloom else dict(enabled=0)))
        r.setFilmOptions(backdrop=backdrop)
        r.setViewOptions(view=abi.VIEW_ALBEDO, ramp=abi.RAMP_HEAT)
        assert r.viewStats().shown == abi.VIEW_ALBEDO
        _assert_same(r.readbackRenderTarget(), want, "albedo")
        _assert_same(_present(r), want, "albedo, presented")
    assert (want != beauty).any() and (want[..., 3] == 255).all()


@pytest.mark.parametrize("view", [abi.VIEW_DEPTH, abi.VIEW_ALBEDO], ids=["depth", "albedo"])
def test_a_view_between_two_beauty_reads_does_not_advance_the_exposure_smoothing(full, view):
    r = full
    r.setExposureOptions(enabled=1, smoothing=0.7, target_log2=-1.0)

    def two_reads(between):
        r.resetExposure()
        r.setExposureOptions(target_log2=-1.0)
        first = r.readbackRenderTarget()
        r.setExposureOptions(target_log2=-4.0)       # the target moves: the second read is one smoothing step towards it
        if between:
            r.setViewOptions(view=view)
            assert r.viewStats().shown == view
            r.readbackRenderTarget()
            _present(r)
            r.setViewOptions(view=abi.VIEW_BEAUTY)
        return first, r.readbackRenderTarget(), r.readbackRenderTarget()

    a1, a2, a3 = two_reads(False)
    b1, b2, b3 = two_reads(True)
    assert (a1 != a2).any() and (a2 != a3).any()     # the state does advance with every beauty read
    _assert_same(b1, a1, "first")
    _assert_same(b2, a2, "second")
    _assert_same(b3, a3, "third")


# ---- 5. BEAUTY with the other fields set, and the views a render cannot show --------------------------------------------------------------------
def test_beauty_ignores_the_other_fields_and_a_data_view_leaves_no_trace(r, cornell):
    """A renderer of its own that never leaves BEAUTY (and so never allocates the record or launches a view kernel) shows the same bytes
    whatever the other fields say; the session's renderer shows them before and after a data view."""
    fresh = Renderer(device=0)
    try:
        _start(fresh, cornell)
        base, base_acc = fresh.readbackRenderTarget(), fresh.readbackAccumulator()
        _present(fresh)
        fresh.setViewOptions(view=abi.VIEW_BEAUTY, layer=abi.MATTE_MATERIAL, ramp=abi.RAMP_HEAT, auto_range=0, depth_min=2.0, depth_max=3.0, noise_max=7.0)
        assert fresh.viewStats().shown == abi.VIEW_BEAUTY
        _assert_same(fresh.readbackRenderTarget(), base, "beauty, fields set")
        _assert_same(_present(fresh), base, "beauty, fields set, presented")
    finally:
        fresh.close()
    _start(r, cornell)
    assert np.array_equal(r.readbackAccumulator().view(np.uint32), base_acc.view(np.uint32))
    _assert_same(r.readbackRenderTarget(), base, "the session's renderer")
    r.setViewOptions(view=abi.VIEW_DEPTH, ramp=abi.RAMP_HEAT)
    assert (r.readbackRenderTarget() != base).any()
    r.setViewOptions(vl.options(view=abi.VIEW_BEAUTY, ramp=abi.RAMP_HEAT, auto_range=0, depth_min=0.5, depth_max=0.75))
    _assert_same(r.readbackRenderTarget(), base, "after a data view")
    _assert_same(_present(r), base, "after a data view, presented")


def test_a_view_the_render_cannot_show_is_the_beauty(r, cornell):
    keeps = {abi.VIEW_ALBEDO: "aov", abi.VIEW_NORMAL: "aov", abi.VIEW_DEPTH: "aov", abi.VIEW_ALPHA: "film", abi.VIEW_MATTE: "matte", abi.VIEW_NOISE: "aov"}
    for have in ({}, dict(aov=True), dict(film=True), dict(matte=True)):
        kw = dict(dict(aov=False, matte=False, film=False), **have)
        _start(r, cornell, **kw)
        r.setViewOptions(vl.options())
        beauty = r.readbackRenderTarget()
        for view in range(abi.VIEW_COUNT):
            r.setViewOptions(vl.options(view=view, ramp=abi.RAMP_HEAT))
            available = view in (abi.VIEW_BEAUTY, abi.VIEW_SAMPLES) or kw[keeps[view]]
            assert r.viewStats().shown == (view if available else abi.VIEW_BEAUTY), (have, view)
            got = r.readbackRenderTarget()
            if available and view != abi.VIEW_BEAUTY:
                assert (got != beauty).any(), (have, view)
            else:
                _assert_same(got, beauty, "%r view %s" % (have, NAMES[view]))
                _assert_same(_present(r), beauty, "%r view %s, presented" % (have, NAMES[view]))
    inp = _inputs(r, SPP, aov=False, film=False, matte=False)                 # SAMPLES needs nothing: a uniform render is one colour
    img = _assert_view(r, inp, dict(view=abi.VIEW_SAMPLES, ramp=abi.RAMP_HEAT))
    assert (img == np.array([255, 0, 0, 255], np.uint8)).all()


def test_before_a_render_and_null_arguments(r, cornell):
    fresh = Renderer(device=0)
    try:
        st = abi.ViewStats()
        assert fresh._lib.pt_read_view_stats(fresh._h, C.byref(st)) == BAD_STATE and b"pt_read_view_stats" in fresh._lib.pt_last_error()
        fresh.setViewOptions(view=abi.VIEW_DEPTH)                             # the setter needs no render
        img, stats = fresh.debugView((1, 1), options=vl.options(view=abi.VIEW_SAMPLES), spp=4, counts=np.array([[2]], np.uint32))
        assert img.tolist() == [[[128, 128, 128, 255]]] and stats.shown == abi.VIEW_SAMPLES       # pt_debug_view needs only pt_create
    finally:
        fresh.close()
    _start(r, cornell)
    assert r._lib.pt_read_view_stats(r._h, None) == INVALID
    bad = vl.options()
    bad.view = abi.VIEW_COUNT
    assert r._lib.pt_set_view_options(r._h, C.byref(bad)) == INVALID and b"view" in r._lib.pt_last_error()
    assert r._lib.pt_set_view_options(r._h, None) == INVALID
    assert bytes(r.viewOptions()) == bytes(vl.options())                      # a refused struct changes nothing
    assert r.viewStats().shown == abi.VIEW_BEAUTY


# ---- 6. a device group ------------------------------------------------------------------------------------------------------------------------
def test_a_group_takes_the_options_and_shows_the_beauty(cornell):
    g = Renderer(devices=[0, 0])
    try:
        g.startRender(cornell, SIZE, SPP, max_bounces=BOUNCES)
        g.render(0)
        g.wait()
        beauty = g.readbackRenderTarget()
        for view in range(abi.VIEW_COUNT):
            g.setViewOptions(vl.options(view=view, ramp=abi.RAMP_HEAT))           # never refused
            assert g.viewStats().shown == abi.VIEW_BEAUTY
            _assert_same(g.readbackRenderTarget(), beauty, "group, view %s" % NAMES[view])
        bad = vl.options()
        bad.ramp = 2
        assert g._lib.pt_set_view_options(g._h, C.byref(bad)) == INVALID
        img, stats = g.debugView((1, 1), options=vl.options(view=abi.VIEW_SAMPLES), spp=1, counts=np.array([[1]], np.uint32))
        assert img.tolist() == [[[255, 255, 255, 255]]]
    finally:
        g.close()


# ---- 7. the selection overlay on top ------------------------------------------------------------------------------------------------------------
def test_the_selection_overlay_draws_over_the_matte_view(full):
    r = full
    layer = abi.MATTE_MATERIAL                                                # (the box is one instance of several materials)
    inp = _inputs(r, SPP, layer)
    plain = _assert_view(r, inp, dict(view=abi.VIEW_MATTE, layer=layer))
    first = inp["slots"]["id"][..., 0]
    ids = sorted(set(first.ravel().tolist()) - {abi.MATTE_NONE}, key=lambda i: int((first == i).sum()))[:1]      # the smallest material
    r.setSelectionOptions(enabled=1, layer=layer, width=2.0, fill_rgba=(0.0, 0.4, 1.0, 0.5))
    r.setSelection(ids)
    cov = r.readbackMatte(layer, ids)
    assert cov.any() and not cov.all()
    want = r.debugSelectionOverlay(plain, cov, r.selectionOptions())
    assert (want[..., :3] != plain[..., :3]).any() and (want[..., 3] == 255).all()
    _assert_same(r.readbackRenderTarget(), want, "overlay over the matte view")
    _assert_same(_present(r), want, "overlay over the matte view, presented")
    r.setViewOptions(view=abi.VIEW_DEPTH)                                      # and over any other data view
    r.setSelectionOptions(enabled=0)
    depth = r.readbackRenderTarget()
    r.setSelectionOptions(enabled=1)
    _assert_same(r.readbackRenderTarget(), r.debugSelectionOverlay(depth, cov, r.selectionOptions()), "overlay over the depth view")


# ---- 8. nothing else moves ----------------------------------------------------------------------------------------------------------------------
def _everything(r):
    out = [r.readbackAccumulator()] + [r.readbackAov(k) for k in AOVS] + [r.readbackFilm()]
    slots = [r.readbackMatteSlots(layer) for layer in LAYERS]
    return out, slots, r.readbackSampleCounts(), bytes(r.readbackExposureMeter())


def _assert_unmoved(a, b, what):
    for x, y in zip(a[0], b[0]):
        assert al.same_bits_or_both_nan(x, y).all(), what
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y), what
    assert np.array_equal(a[2], b[2]) and a[3] == b[3], what


def test_every_other_output_keeps_its_bits_under_every_view(r, cornell):
    _start(r, cornell)
    base = _everything(r)
    beauty = r.readbackRenderTarget()
    for view in range(1, abi.VIEW_COUNT):
        r.setViewOptions(vl.options(view=view, ramp=abi.RAMP_HEAT))
        r.readbackRenderTarget()
        _present(r)
        r.viewStats()
        _assert_unmoved(_everything(r), base, NAMES[view])
    # a render started, stepped and presented under a view from its first sample on
    r.setViewOptions(vl.options(view=abi.VIEW_DEPTH))
    r.setDenoiseOptions(enabled=1); r.setMatteOptions(enabled=1); r.setFilmOptions(enabled=1)
    r.startRender(cornell, SIZE, SPP, max_bounces=BOUNCES)
    r.setDenoiseOptions(enabled=0); r.setMatteOptions(enabled=0); r.setFilmOptions(enabled=0)
    for _ in range(SPP):
        r.render(1)
        r.presentRenderTarget()
    r.wait()
    _assert_unmoved(_everything(r), base, "rendered under a view")
    r.setViewOptions(vl.options())
    _assert_same(r.readbackRenderTarget(), beauty, "the beauty after a render under a view")
