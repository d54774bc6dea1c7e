"""GPU: the selection overlay (include/ptamd.h pt_selection_options, platinum_amd/csrc/selection.hip).
pt_debug_selection_overlay equals the host build of pt_selection.h (tests/emu/selection_emu.cpp) byte for byte over sizes, widths, cards and
option sets; on renders the target with the overlay on, read and presented, equals the host overlay of (the same renderer's target with the
overlay off, pt_read_matte of the set); the chain, a region, an adaptive render, the material layer, the background; state and ordering;
everything else the render produces stays the bits it is without the overlay; errors.  Every image is at most 300x3 or 258x20 and every
render at most 64 spp."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import matte_lib as ml  # noqa: E402
import selection_lib as sl  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = ml.NONE
SIZE, SPP, BOUNCES = (24, 17), 64, 4     # the matte tests' render: a partial tile row, and a 1-pixel-high edge tile
INVALID, BAD_STATE, UNSUPPORTED = -1, -5, -6
ON = dict(enabled=1, width=2.0, fill_rgba=sl.BLUE + (0.4,))     # an outline and a tint


def _defaults(r):
    r.setSelectionOptions(sl.options())
    r.setSelection([])
    r.setMatteOptions(enabled=0)
    r.setAdaptiveOptions(enabled=0)
    r.clearRenderRegion()
    for struct, default, setter in ((abi.BloomOptions, "pt_default_bloom_options", r.setBloomOptions),
                                    (abi.ExposureOptions, "pt_default_exposure_options", r.setExposureOptions),
                                    (abi.DenoiseOptions, "pt_default_denoise_options", r.setDenoiseOptions)):
        o = struct()
        getattr(r._lib, default)(C.byref(o))
        setter(o)
    r.resetExposure()


@pytest.fixture
def r(gpu_renderer):
    _defaults(gpu_renderer)
    yield gpu_renderer
    _defaults(gpu_renderer)      # the session's renderer goes on with the overlay disabled and no selection


@pytest.fixture(scope="module")
def field():
    return scenes.field_scene(32)


@pytest.fixture(scope="module")
def field_ref(field):
    """The reference of the 24x17 x 64 spp field render, computed once and read only: the instance layer's slots, and the id set of the
    tests below chosen on them: every instance but the ground plane (id 0) that covers a pixel of its own completely."""
    ids = ml.reference_ids(field, SIZE, SPP)
    slots = ml.fold_image(ids[abi.MATTE_INSTANCE])
    slots.flags.writeable = False
    first, count = slots["id"][..., 0], slots["count"][..., 0]
    chosen = sorted(set(int(i) for i in first[(count == SPP) & (first != 0) & (first != NONE)]))
    return slots, chosen


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _start(r, sc, size=SIZE, spp=SPP, bounces=BOUNCES, matte=True, aov=False, apply_to_target=0, region=None, adaptive=None, **kw):
    r.setMatteOptions(enabled=1 if matte else 0)
    r.setDenoiseOptions(enabled=1 if aov else 0, apply_to_target=apply_to_target)
    if region:
        r.setRenderRegion(*region)
    else:
        r.clearRenderRegion()
    if adaptive:
        r.setAdaptiveOptions(enabled=1, min_spp=adaptive[0], interval=adaptive[1], threshold=adaptive[2])
    else:
        r.setAdaptiveOptions(enabled=0)
    r.startRender(sc, size, spp, max_bounces=bounces, **kw)
    r.render(0)
    r.wait()


def _copy_off(r, ptr):
    """The device image a present returned, copied to the host."""
    hip = abi.load_library()
    w, h = r.size
    got = np.empty((h, w, 4), np.uint8)
    assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), C.c_void_p(ptr), C.c_size_t(got.nbytes), 2) == 0  # hipMemcpyDeviceToHost
    return got


def _present(r):
    ptr, stream = r.presentRenderTarget()
    assert ptr and stream
    assert abi.load_library().hipStreamSynchronize(C.c_void_p(stream)) == 0
    return _copy_off(r, ptr)


def _assert_same(got, want, what):
    bad = (got != want).any(axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first (y, x) %s: device %s, host %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:2].tolist(), want[bad][:2].tolist())


def _base_and_overlay(r, ids, options, what, reset_exposure=False):
    """The target with the overlay off, then on: the second, read and presented, must be the host overlay of the first under pt_read_matte's
    coverage of the set.  Returns (base, coverage, drawn target)."""
    off = sl.options(**options)
    off.enabled = 0
    r.setSelectionOptions(off)
    r.setSelection(ids)
    if reset_exposure:
        r.resetExposure()
    base = r.readbackRenderTarget()
    cov = r.readbackMatte(r.selectionOptions().layer, ids)
    r.setSelectionOptions(enabled=1)
    if reset_exposure:
        r.resetExposure()
    got = r.readbackRenderTarget()
    want = sl.host_overlay(base, cov, r.selectionOptions())
    _assert_same(got, want, what)
    if reset_exposure:
        r.resetExposure()
    _assert_same(_present(r), want, what + ", presented")
    return base, cov, got


# ---- pt_debug_selection_overlay against the host build -------------------------------------------------------------------------------------
# selection_lib.SIZES, and 258x20, 254x20: a width one block more and one block less than a multiple of 16 blocks ... 17 and 16 blocks a row,
# the last one 2 and 14 pixels wide
DEBUG_SIZES = sl.SIZES + [(258, 20), (254, 20)]


def _assert_debug_equals_host(r, W, H, width):
    n = 0
    for cname in sl.COVERAGE_CARDS:
        cov = sl.coverage_card(cname, W, H)
        for tname in sl.TARGET_CARDS:
            target = sl.target_card(tname, W, H)
            for setname, f in sl.OPTION_SETS.items():
                o = sl.options(width=width, **f)
                _assert_same(r.debugSelectionOverlay(target, cov, o), sl.host_overlay(target, cov, o),
                             "%s on %s, %dx%d, width %g, %s" % (cname, tname, W, H, width, setname))
                n += 1
    return n


@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("W,H", DEBUG_SIZES)
def test_debug_overlay_equals_the_host_build(r, W, H, width):
    assert _assert_debug_equals_host(r, W, H, width) == 80


def test_debug_overlay_needs_no_render_and_leaves_the_renderer_alone():
    fresh = Renderer(device=0)
    try:
        assert _assert_debug_equals_host(fresh, 67, 45, 7.25) == 80      # before any render
        fresh.setMatteOptions(enabled=1)
        fresh.startRender(scenes.cornell_sphere_scene(), (33, 19), 8, max_bounces=4)
        fresh.render(0)
        fresh.wait()
        fresh.setSelectionOptions(**ON)
        fresh.setSelection([0])
        acc, target = fresh.readbackAccumulator(), fresh.readbackRenderTarget()
        o = sl.options(width=16.0, fill_rgba=sl.BLUE + (1.0,))
        fresh.debugSelectionOverlay(sl.target_card("random", 67, 45), sl.coverage_card("random", 67, 45), o)
        assert np.array_equal(fresh.readbackRenderTarget(), target) and np.array_equal(_bits(fresh.readbackAccumulator()), _bits(acc))
        assert bytes(fresh.selectionOptions()) == bytes(sl.options(**ON)) and fresh.selection().tolist() == [0]
    finally:
        fresh.close()


# ---- a rendered field ----------------------------------------------------------------------------------------------------------------------
def test_the_reference_populates_every_class(field_ref):
    slots, chosen = field_ref
    cov = ml.coverage(slots, chosen, SPP)
    full, outline, fractional, untouched = sl.pixel_classes(cov, sl.options(**ON))
    print("selection %s: %d pixels fully covered, %d outline only, %d fractional, %d untouched" % (
        chosen, full.sum(), outline.sum(), fractional.sum(), untouched.sum()))
    assert len(chosen) >= 1 and full.any() and outline.any() and fractional.any() and untouched.any()


def test_rendered_target_is_the_host_overlay_of_the_plain_target(r, field, field_ref):
    slots, chosen = field_ref
    _start(r, field)
    base, cov, got = _base_and_overlay(r, chosen, ON, "field")
    assert np.array_equal(_bits(cov), _bits(ml.coverage(slots, chosen, SPP)))      # the device's coverage is the reference's
    full, outline, fractional, untouched = sl.pixel_classes(cov, r.selectionOptions())
    assert np.array_equal(got[untouched], base[untouched])
    assert (got[outline] != base[outline]).any() and (got[full] != base[full]).any()
    assert (got[..., 3] == 255).all()
    for width in (1.0, 7.25, 16.0):      # the halo wider than the frame's blocks
        _base_and_overlay(r, chosen, dict(ON, width=width), "field, width %g" % width)


# ---- chain and render variants ---------------------------------------------------------------------------------------------------------------
def test_overlay_after_exposure_bloom_and_the_denoised_target(r, field, field_ref):
    _slots, chosen = field_ref
    _start(r, field, aov=True, apply_to_target=1)
    plain = r.readbackRenderTarget()
    r.setExposureOptions(enabled=1)
    r.setBloomOptions(enabled=1, intensity=0.35, threshold=0.25, knee=0.125, scatter=0.8, levels=5)
    meter = r.readbackExposureMeter()
    base, _cov, got = _base_and_overlay(r, chosen, ON, "exposure, bloom, apply_to_target", reset_exposure=True)
    assert not np.array_equal(base, plain) and not np.array_equal(got, base)
    assert bytes(r.readbackExposureMeter()) == bytes(meter)      # the meter does not see the overlay


def test_a_region_that_is_not_tile_aligned(r, field, field_ref):
    slots, _chosen = field_ref
    x0, y0, x1, y1 = 5, 3, 19, 14
    window = slots["id"][8:13, 3:8, 0]                               # the instances seen first in a window across the region's left edge
    ids = sorted(set(int(i) for i in window.ravel() if i not in (0, NONE)))
    inside = np.zeros(SIZE[::-1], bool)
    inside[y0:y1, x0:x1] = True
    whole = ml.coverage(slots, ids, SPP)
    assert len(ids) >= 4 and whole[~inside].any() and whole[inside].any()
    _start(r, field, region=(x0, y0, x1, y1), samples_in_flight=16)
    base, cov, got = _base_and_overlay(r, ids, ON, "region")
    assert not cov[~inside].any() and np.array_equal(_bits(cov[inside]), _bits(whole[inside]))      # nothing selected outside the region, whatever is there
    R = 2
    near = np.zeros_like(inside)
    for y, x in np.argwhere(cov > 0):
        near[max(0, y - R):y + R + 1, max(0, x - R):x + R + 1] = True
    assert np.array_equal(got[~near], base[~near]) and (got[near] != base[near]).any()      # the outline stops where the coverage does


def test_an_adaptive_render_whose_tiles_stop_at_different_counts(r):
    kind, _size, bounces, _spp, min_spp, interval, threshold = al.CONFIGS["textured99"]
    sc = al.config_scene(kind)
    _start(r, sc, (33, 19), 64, bounces=bounces, adaptive=(min_spp, interval, threshold))
    counts = r.readbackSampleCounts()
    assert len(set(counts.ravel().tolist())) > 1
    seen = np.unique(r.readbackMatteSlots(abi.MATTE_INSTANCE)["id"])
    ids = [int(i) for i in seen if i != NONE][:2]
    _base, cov, _got = _base_and_overlay(r, ids, ON, "adaptive")
    assert cov.any() and ((cov > 0) & (cov < 1)).any()


def test_the_material_layer_and_the_background(r):
    sc = scenes.cornell_sphere_scene()      # one shell instance with several materials, and camera rays that miss
    _start(r, sc, (33, 19), 16, bounces=6, samples_in_flight=5)
    mat = r.readbackMatteSlots(abi.MATTE_MATERIAL)
    ids = [int(i) for i in np.unique(mat["id"][mat["count"] != 0]) if i != NONE][1:3]
    _base, cov_m, got_m = _base_and_overlay(r, ids, dict(ON, layer=abi.MATTE_MATERIAL), "material layer")
    assert cov_m.any() and not cov_m.all()
    _base, cov_i, _got = _base_and_overlay(r, ids, dict(ON, layer=abi.MATTE_INSTANCE), "the same ids on the instance layer")
    assert not np.array_equal(cov_i, cov_m)
    _base, cov_bg, got_bg = _base_and_overlay(r, [NONE], ON, "the background")
    assert cov_bg.any() and (cov_bg == 0).any() and not np.array_equal(got_bg, got_m)


# ---- state and ordering ----------------------------------------------------------------------------------------------------------------------
def test_options_and_set_change_without_a_restart(r, field, field_ref):
    _slots, chosen = field_ref
    _start(r, field)
    _b, _c, a = _base_and_overlay(r, chosen, ON, "first")
    _b, _c, b = _base_and_overlay(r, chosen, dict(ON, width=5.0, outline_rgba=(0.0, 1.0, 1.0, 0.7)), "other options")
    _b, _c, c = _base_and_overlay(r, chosen[:1] + [0, 0, chosen[0]], ON, "other set, unsorted with duplicates")
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    assert r.selection().tolist() == sorted(set(chosen[:1] + [0]))
    _start(r, field, spp=8)                     # the set and the options survive pt_start_render
    assert r.selection().tolist() == sorted(set(chosen[:1] + [0])) and r.selectionOptions().enabled == 1
    r.setSelectionOptions(enabled=0)
    plain = r.readbackRenderTarget()
    r.setSelectionOptions(enabled=1)
    _assert_same(r.readbackRenderTarget(), sl.host_overlay(plain, r.readbackMatte(abi.MATTE_INSTANCE, r.selection()), r.selectionOptions()), "after a restart")


def test_a_present_draws_the_set_and_coverage_it_was_enqueued_with(r, field, field_ref):
    _slots, chosen = field_ref
    _start(r, field)
    _base, _cov, want = _base_and_overlay(r, chosen, ON, "the first set")
    ptr, _stream = r.presentRenderTarget()
    r.setSelection([0])                                              # after the present: its bytes are the first set's
    got = _copy_off(r, ptr)
    _assert_same(got, want, "a set change after a present")
    assert not np.array_equal(r.readbackRenderTarget(), want)        # (the next target shows the ground plane selected)
    r.setSelection(chosen)
    ptr, stream = r.presentRenderTarget()
    other = r.readbackMatte(abi.MATTE_INSTANCE, [0])                 # another set through pt_read_matte's own buffers
    assert other.any()
    assert abi.load_library().hipStreamSynchronize(C.c_void_p(stream)) == 0
    _assert_same(_copy_off(r, ptr), want, "a pt_read_matte between a present and its read-back")
    _assert_same(r.readbackRenderTarget(), want, "and the next read")


# ---- nothing else moves ----------------------------------------------------------------------------------------------------------------------
def _everything_else(r):
    st = r.stats()
    out = [r.readbackAccumulator()] + [r.readbackAov(k) for k in (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)]
    slots = [r.readbackMatteSlots(layer) for layer in (abi.MATTE_INSTANCE, abi.MATTE_MATERIAL)]
    return out, slots, r.readbackSampleCounts(), (st.closest_rays, st.shadow_rays, st.shaded_hits, st.paths, st.nonfinite_samples, st.batches)


def test_every_other_output_is_the_same_bits_with_the_overlay_on(r):
    sc = scenes.cornell_sphere_scene()
    _start(r, sc, (33, 19), 16, bounces=6, samples_in_flight=5, aov=True)
    off = _everything_else(r)
    plain = r.readbackRenderTarget()
    r.setSelectionOptions(**ON)
    r.setSelection([0, NONE])
    _start(r, sc, (33, 19), 16, bounces=6, samples_in_flight=5, aov=True)
    drawn, presented = r.readbackRenderTarget(), _present(r)
    on = _everything_else(r)
    assert not np.array_equal(drawn, plain) and np.array_equal(presented, drawn)
    assert on[3] == off[3] and np.array_equal(on[2], off[2])
    for a, b in zip(on[0], off[0]):
        assert np.any(a != 0) and al.same_bits_or_both_nan(a, b).all()
    for a, b in zip(on[1], off[1]):
        assert np.array_equal(a, b)


def test_disabled_empty_and_matte_less_renders_show_the_plain_target(r, field, field_ref):
    _slots, chosen = field_ref
    fresh = Renderer(device=0)      # never hears of a selection
    try:
        _start(fresh, field)
        plain, plain_acc = fresh.readbackRenderTarget(), fresh.readbackAccumulator()
    finally:
        fresh.close()
    _start(r, field)
    r.setSelection(chosen)
    r.setSelectionOptions(**dict(ON, enabled=0, width=9.0))
    before, before_presented = r.readbackRenderTarget(), _present(r)
    r.setSelectionOptions(enabled=1)
    on = r.readbackRenderTarget()
    r.setSelectionOptions(enabled=0, width=3.0)
    after, after_presented = r.readbackRenderTarget(), _present(r)
    for img in (before, before_presented, after, after_presented):
        assert np.array_equal(img, plain)
    assert not np.array_equal(on, plain)
    assert np.array_equal(_bits(r.readbackAccumulator()), _bits(plain_acc))
    r.setSelectionOptions(enabled=1)
    r.setSelection([])                                               # enabled, nothing selected
    assert np.array_equal(r.readbackRenderTarget(), plain) and np.array_equal(_present(r), plain)
    r.setSelection(chosen)
    assert not np.array_equal(r.readbackRenderTarget(), plain)
    _start(r, field, matte=False)                                    # enabled, a set, a render without mattes: silently no overlay
    assert np.array_equal(r.readbackRenderTarget(), plain) and np.array_equal(_present(r), plain)


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------
def test_error_codes(r, field):
    L, h = r._lib, r._h
    _start(r, field, spp=4)
    r.setSelectionOptions(**ON)
    r.setSelection([3, 1])
    shown = r.readbackRenderTarget()
    for bad in (dict(layer=2), dict(width=0.5), dict(width=16.5), dict(width=float("nan")), dict(outline_rgba=(0.0, 0.0, 0.0, 1.5)),
                dict(fill_rgba=(float("nan"), 0.0, 0.0, 0.0)), dict(fill_rgba=(0.0, -0.1, 0.0, 0.0))):
        o = sl.options(enabled=1, **bad)
        assert L.pt_set_selection_options(h, C.byref(o)) == INVALID, bad
    assert L.pt_set_selection_options(h, None) == INVALID
    ids = np.array([5, 6], np.uint32)
    n = C.c_uint32()
    assert L.pt_set_selection(h, None, 2) == INVALID and b"null id set" in L.pt_last_error()
    assert L.pt_get_selection(h, None, 0, None) == INVALID
    assert L.pt_get_selection(h, None, 2, C.byref(n)) == INVALID
    assert L.pt_get_selection(h, ids.ctypes.data, 1, C.byref(n)) == 0 and n.value == 2 and ids.tolist() == [1, 6]      # capacity 1 of 2
    img, cov, out = np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4), np.float32), np.zeros((4, 4, 4), np.uint8)
    o = sl.options()
    assert L.pt_debug_selection_overlay(h, None, cov.ctypes.data, 4, 4, C.byref(o), out.ctypes.data) == INVALID
    assert L.pt_debug_selection_overlay(h, img.ctypes.data, None, 4, 4, C.byref(o), out.ctypes.data) == INVALID
    assert L.pt_debug_selection_overlay(h, img.ctypes.data, cov.ctypes.data, 4, 4, None, out.ctypes.data) == INVALID
    assert L.pt_debug_selection_overlay(h, img.ctypes.data, cov.ctypes.data, 4, 4, C.byref(o), None) == INVALID
    assert L.pt_debug_selection_overlay(h, img.ctypes.data, cov.ctypes.data, 0, 4, C.byref(o), out.ctypes.data) == INVALID
    assert L.pt_debug_selection_overlay(h, img.ctypes.data, cov.ctypes.data, 1 << 15, (1 << 13) + 1, C.byref(o), out.ctypes.data) == INVALID
    o.width = 17.0
    assert L.pt_debug_selection_overlay(h, img.ctypes.data, cov.ctypes.data, 4, 4, C.byref(o), out.ctypes.data) == INVALID
    # nothing above changed what the renderer holds or shows
    assert r.selection().tolist() == [1, 3] and bytes(r.selectionOptions()) == bytes(sl.options(**ON))
    assert np.array_equal(r.readbackRenderTarget(), shown)
    assert L.pt_set_selection(h, None, 0) == 0 and r.selection().size == 0
    g = Renderer(devices=[0, 0])
    try:
        o = g.selectionOptions()
        o.enabled = 1
        assert g._lib.pt_set_selection_options(g._h, C.byref(o)) == UNSUPPORTED and b"device group" in g._lib.pt_last_error()
        o.enabled = 0
        o.width = 3.0
        assert g._lib.pt_set_selection_options(g._h, C.byref(o)) == 0
        assert g._lib.pt_set_selection_options(g._h, None) == INVALID
        g.setSelection([2, 1])
        assert g.selection().tolist() == [1, 2]
        g.startRender(scenes.cornell_scene("bench"), (16, 8), 2, max_bounces=2)
        g.render(0)
        g.wait()
        plain = g.readbackRenderTarget()
        assert plain.shape == (8, 16, 4) and np.array_equal(_present(g), plain)      # a group shows no overlay
    finally:
        g.close()
