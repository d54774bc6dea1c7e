"""GPU: ID mattes against an independent reference — the oracle's trace_primary(s) for s = 0 .. n - 1, folded by the plain
Python restatement of the rule in tests/matte_lib.py, the material id taken from the scene's own material_slots and the prefix sum of its
instances' material counts.  Slot equality is exact: id, count and slot order.  Every image is at most 33x19 and every render at most 64 spp."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import matte_lib as ml  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = ml.NONE
LAYERS = (abi.MATTE_INSTANCE, abi.MATTE_MATERIAL)
SIZE, SPP, BOUNCES = (24, 17), 64, 4     # 24x17: a partial tile row, and a 1-pixel-high edge tile
INVALID, BAD_STATE, UNSUPPORTED = -1, -5, -6
SWITCHES = ("PTAMD_NO_CAMERA_LISTS", "PTAMD_TEST_CAMLIST_CAP")


@pytest.fixture(scope="module")
def r():
    rr = Renderer(device=0)
    yield rr
    rr.close()


@pytest.fixture(scope="module")
def field():
    return scenes.field_scene(32)


@pytest.fixture(scope="module")
def field_ref(field):
    """(ids per layer (SPP, H, W), reference slots per layer (H, W, 8)), computed once and read only"""
    ids = ml.reference_ids(field, SIZE, SPP)
    slots = tuple(ml.fold_image(v) for v in ids)
    for s in slots:
        s.flags.writeable = False
    return ids, slots


def _start(r, sc, size, spp, bounces=BOUNCES, sif=0, matte=True, aov=False, region=None, adaptive=None, **kw):
    r.setMatteOptions(enabled=1 if matte else 0)
    r.setDenoiseOptions(enabled=1 if aov else 0)
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
    finally:   # (the options are read at startRender: the renderer goes back to its defaults for whoever uses it next)
        r.setMatteOptions(enabled=0)
        r.setDenoiseOptions(enabled=0)
        r.clearRenderRegion()
        r.setAdaptiveOptions(enabled=0)


def _finish(r, steps=(0,)):
    for n in steps:
        r.render(n)
        r.wait()
    return tuple(r.readbackMatteSlots(layer) for layer in LAYERS)


def _render(r, sc, size, spp, steps=(0,), **kw):
    _start(r, sc, size, spp, **kw)
    return _finish(r, steps)


def _assert_slots(got, want, what=""):
    for layer in LAYERS:
        g, w = got[layer], want[layer]
        assert g.shape == w.shape and g.dtype == w.dtype
        bad = np.argwhere((g["id"] != w["id"]) | (g["count"] != w["count"]))
        assert bad.size == 0, "%s layer %d: %d slots differ, the first at (y, x, slot) = %s: device %s, reference %s" % (
            what, layer, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])


# ---- slots equal the reference ------------------------------------------------------------------------------------------------------------
def test_the_reference_populates_every_class(field_ref):
    ids, slots = field_ref
    for layer in LAYERS:
        d = ml.distinct_ids(ids[layer])
        many, some, one = int((d > 8).sum()), int(((d >= 2) & (d <= 8)).sum()), int((d == 1).sum())
        print("layer %d: %d pixels with more than 8 distinct ids (max %d), %d with 2-8, %d with one" % (layer, many, d.max(), some, one))
        assert many >= 20 and some >= 100 and one >= 50
        total = slots[layer]["count"].sum(axis=-1)
        assert (total <= SPP).all() and np.array_equal(total == SPP, d <= 8)


@pytest.mark.parametrize("way", ["one_batch", "seven_in_flight", "one_sample_calls", "restarted"])
def test_slots_equal_the_reference(r, field, field_ref, way):
    ids, want = field_ref
    if way == "one_batch":
        got = _render(r, field, SIZE, SPP, sif=SPP)
        assert r.stats().batches == 1
    elif way == "seven_in_flight":     # nine batches of 7 and a tail of 1: no multiple of 8 anywhere, n0 != 0
        got = _render(r, field, SIZE, SPP, sif=7)
        assert r.stats().samples_in_flight == 7 and r.stats().batches == 10
    elif way == "one_sample_calls":
        got = _render(r, field, SIZE, SPP, steps=(1,) * SPP)
        assert r.stats().batches == SPP
    else:                              # a render left half way, then pt_start_render again: the slots start empty
        half = _render(r, field, SIZE, SPP, steps=(24,))
        assert (half[0]["count"].sum(axis=-1) == 24).any()
        got = _render(r, field, SIZE, SPP)
    _assert_slots(got, want, way)
    for layer in LAYERS:
        total = got[layer]["count"].sum(axis=-1)
        assert (total <= SPP).all()
        assert np.array_equal(total == SPP, ml.distinct_ids(ids[layer]) <= 8)   # other = n - sum: 0 exactly where every id found a slot


# ---- misses and material slots ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_sphere", "textured"])
def test_misses_take_a_slot_and_materials_separate_the_shell(r, name):
    sc = scenes.cornell_sphere_scene() if name == "cornell_sphere" else scenes.textured_scene()
    size, spp = (33, 19), 16
    ids = ml.reference_ids(sc, size, spp)
    misses = int((ids[0] == NONE).sum())
    print(name, "miss samples in the reference:", misses)
    assert misses >= 1000 and np.array_equal(ids[0] == NONE, ids[1] == NONE)
    want = tuple(ml.fold_image(v) for v in ids)
    got = _render(r, sc, size, spp, bounces=6, sif=5)
    _assert_slots(got, want, name)
    for layer in LAYERS:
        bg = np.where((got[layer]["id"] == NONE), got[layer]["count"], 0).sum()
        assert int(bg) == misses                                      # the background is counted, in a slot of its own
        assert (got[layer]["count"].sum(axis=-1) == spp).all()        # (at most 8 ids per pixel here: nothing went to `other`)
    if name == "cornell_sphere":
        # the Cornell shell is ONE instance with several material slots: pixels that see two of its walls hold one instance and two materials
        occupied = [(got[layer]["count"] != 0).sum(axis=-1) for layer in LAYERS]
        shell_only = (occupied[0] == 1) & (got[0]["id"][..., 0] == 0)
        assert (shell_only & (occupied[1] >= 2)).sum() >= 5
        assert len(sc.nodes[0].materials) > 1 and set(np.unique(ids[1][ids[0] == 0]).tolist()) <= set(range(len(sc.nodes[0].materials)))
        assert np.unique(ids[1][ids[0] == 0]).size >= 3


# ---- nothing else moves ---------------------------------------------------------------------------------------------------------------------
def _everything_else(r, sc, matte, **kw):
    _start(r, sc, (33, 19), 16, bounces=6, sif=5, matte=matte, aov=True, **kw)
    r.render(0)
    r.wait()
    st = r.stats()
    out = [r.readbackAccumulator()] + [r.readbackAov(k) for k in (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)]
    r.setDenoiseOptions(enabled=1)      # (the filter's options are read when the image is asked for)
    out.append(r.readbackDenoised())
    r.setDenoiseOptions(enabled=0)
    return out, r.readbackSampleCounts(), (st.closest_rays, st.shadow_rays, st.shaded_hits, st.paths, st.nonfinite_samples, st.batches)


@pytest.mark.parametrize("gmon", [False, True])
def test_every_other_output_is_the_same_bits_with_mattes_on(r, gmon):
    sc = scenes.cornell_sphere_scene()
    kw = dict(flags=abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON, gmonBuckets=4) if gmon else {}
    off = _everything_else(r, sc, False, **kw)
    on = _everything_else(r, sc, True, **kw)
    slots = r.readbackMatteSlots(abi.MATTE_INSTANCE)
    assert (slots["count"].sum(axis=-1) == 16).all()                 # (mattes were on, and GMoN renders keep them too)
    assert on[2] == off[2] and on[2][3] == 33 * 19 * 16
    assert np.array_equal(on[1], off[1])
    for a, b in zip(on[0], off[0]):
        assert np.any(a != 0) and al.same_bits_or_both_nan(a, b).all()


# ---- the two camera paths -------------------------------------------------------------------------------------------------------------------
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


def test_fused_and_walked_camera_rays_give_the_same_slots(r, field, field_ref):
    for k in SWITCHES:
        assert os.environ.get(k, "0") in ("", "0"), "this test compares the switches' two sides"
    _ids, want = field_ref
    others = [_renderer_under({"PTAMD_NO_CAMERA_LISTS": "1"})]
    try:
        built = []
        for rr, what in zip([r] + others, ("fused", "no lists")):
            _start(rr, field, SIZE, SPP, sif=SPP)
            built.append(rr.cameraListStats().built)
            _assert_slots(_finish(rr), want, what)
        assert built == [1, 0]
    finally:
        for rr in others:
            rr.close()


# ---- render regions -------------------------------------------------------------------------------------------------------------------------
def test_a_region_keeps_the_full_frame_bits_inside_and_empty_slots_outside(r, field, field_ref):
    _ids, want = field_ref
    x0, y0, x1, y1 = 5, 3, 19, 14      # not tile-aligned
    got = _render(r, field, SIZE, SPP, sif=16, region=(x0, y0, x1, y1))
    inside = np.zeros(SIZE[::-1], bool)
    inside[y0:y1, x0:x1] = True
    for layer in LAYERS:
        g, w = got[layer], want[layer]
        assert np.array_equal(g[inside], w[inside])
        assert (g["id"][~inside] == NONE).all() and (g["count"][~inside] == 0).all()
        everything = np.unique(w["id"])
        cov = r.readbackMatte(layer, everything)
        assert not cov[~inside].any() and (cov[inside] > 0).all()
        assert np.array_equal(cov.view(np.uint32), ml.coverage(g, everything, np.where(inside, SPP, 0)).view(np.uint32))
    for x, y, n in ((0, 0, 0), (4, 3, 0), (5, 2, 0), (19, 13, 0), (18, 14, 0), (23, 16, 0), (5, 3, SPP), (18, 13, SPP)):
        p = r.pick(x, y)
        assert p.samples == n, (x, y)
        if n == 0:
            assert (p.instance, p.instance_count, p.material, p.material_count) == (NONE, 0, NONE, 0)
            assert (p.material_instance, p.material_slot) == (NONE, NONE)


# ---- adaptive sampling ------------------------------------------------------------------------------------------------------------------------
def test_an_adaptive_tile_holds_the_slots_of_a_uniform_render_of_its_own_count(r):
    kind, _size, bounces, _spp, min_spp, interval, threshold = al.CONFIGS["textured99"]
    sc, size, spp = al.config_scene(kind), (33, 19), 64
    got = _render(r, sc, size, spp, bounces=bounces, adaptive=(min_spp, interval, threshold))
    counts = r.readbackSampleCounts()
    classes = sorted(set(counts.ravel().tolist()))
    print("sample counts:", al.histogram(counts))
    assert len(classes) > 1 and classes[-1] <= spp and classes[0] >= min_spp, classes
    ids = ml.reference_ids(sc, size, spp)
    want = tuple(ml.fold_image(v, counts) for v in ids)
    _assert_slots(got, want, "adaptive")
    for layer in LAYERS:
        assert np.array_equal(got[layer]["count"].sum(axis=-1), counts)     # (at most 8 ids per pixel in this scene)
        some = np.unique(want[layer]["id"])[:2]
        cov = r.readbackMatte(layer, some)                                   # the resolve divides by the tile's own count
        assert np.array_equal(cov.view(np.uint32), ml.coverage(got[layer], some, counts).view(np.uint32))
    x, y = np.unravel_index(np.argmin(counts), counts.shape)[::-1]
    assert r.pick(int(x), int(y)).samples == counts.min()


# ---- pt_read_matte and pt_pick ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(field, field_ref):
    """a renderer of its own that holds the finished 24x17 x 64 spp render of the field scene"""
    rr = Renderer(device=0)
    slots = _render(rr, field, SIZE, SPP)
    _assert_slots(slots, field_ref[1], "full")
    yield rr, slots
    rr.close()


def test_read_matte_equals_the_numpy_resolve_of_the_device_slots(full, field):
    rr, slots = full
    inst = slots[abi.MATTE_INSTANCE]
    seen = np.unique(inst["id"][inst["count"] != 0])
    seen = seen[seen != NONE]
    rng = np.random.default_rng(7)
    absent = next(i for i in range(len(field.nodes)) if i not in set(seen.tolist()))
    sets = {
        "one instance": [int(seen[len(seen) // 2])],
        "300 instances": list(rng.permutation(len(field.nodes))[:290]) + list(seen[:10]),     # unsorted, with duplicates among them or not
        "the background": [NONE],
        "the empty set": [],
        "an id in no slot": [absent],
        "far out of range": [0x7FFFFFFF, 0xFFFFFFFE],
    }
    assert len(sets["300 instances"]) == 300
    for what, ids in sets.items():
        got = rr.readbackMatte(abi.MATTE_INSTANCE, ids)
        want = ml.coverage(inst, ids, SPP)
        assert got.dtype == np.float32 and got.shape == SIZE[::-1]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
        if what in ("one instance", "300 instances"):
            assert got.any() and (got <= 1).all()
        if what in ("the empty set", "an id in no slot", "far out of range"):
            assert not got.any()
    mat = slots[abi.MATTE_MATERIAL]
    ids = list(np.unique(mat["id"])[::3]) * 2
    assert np.array_equal(rr.readbackMatte(abi.MATTE_MATERIAL, ids).view(np.uint32), ml.coverage(mat, ids, SPP).view(np.uint32))
    # every instance and the background: 1 exactly where no sample went to `other`
    cov = rr.readbackMatte(abi.MATTE_INSTANCE, list(range(len(field.nodes))) + [NONE])
    assert np.array_equal(cov == 1.0, inst["count"].sum(axis=-1) == SPP)


def test_pick_is_the_argmax_of_the_slots_at_every_pixel(full, field):
    rr, slots = full
    base = ml.material_bases(field)
    ties = 0
    for y in range(SIZE[1]):
        for x in range(SIZE[0]):
            p = rr.pick(x, y)
            si, sm = slots[abi.MATTE_INSTANCE][y, x], slots[abi.MATTE_MATERIAL][y, x]
            assert (p.instance, p.instance_count) == ml.pick(si), (x, y)
            assert (p.material, p.material_count) == ml.pick(sm), (x, y)
            assert p.samples == SPP and p._pad == 0
            ties += int((si["count"] == si["count"].max()).sum() > 1)
            if p.material == NONE:
                assert (p.material_instance, p.material_slot) == (NONE, NONE)
            else:
                assert p.material_instance < len(field.nodes) and p.material_slot < len(field.nodes[p.material_instance].materials)
                assert int(base[p.material_instance]) + p.material_slot == p.material
    print("pixels whose largest instance count is shared by several slots:", ties)


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------
def test_error_codes(full, field):
    rr, _slots = full
    L, h = rr._lib, rr._h
    W, H = SIZE
    slots = np.empty((H, W, 8), ml.SLOT_DTYPE)
    cov = np.empty((H, W), np.float32)
    ids = np.zeros(1, np.uint32)
    pr = abi.PickResult()
    assert L.pt_read_matte_slots(h, 2, slots.ctypes.data) == INVALID
    assert L.pt_read_matte_slots(h, abi.MATTE_MATERIAL, None) == INVALID
    assert L.pt_read_matte(h, 2, ids.ctypes.data, 1, cov.ctypes.data) == INVALID
    assert L.pt_read_matte(h, abi.MATTE_INSTANCE, None, 1, cov.ctypes.data) == INVALID
    assert L.pt_read_matte(h, abi.MATTE_INSTANCE, ids.ctypes.data, 1, None) == INVALID
    assert L.pt_read_matte(h, abi.MATTE_INSTANCE, None, 0, cov.ctypes.data) == 0        # (no ids, no pointer needed)
    assert L.pt_pick(h, W, 0, C.byref(pr)) == INVALID
    assert L.pt_pick(h, 0, H, C.byref(pr)) == INVALID
    assert L.pt_pick(h, 0, 0, None) == INVALID
    assert L.pt_pick(h, W - 1, H - 1, C.byref(pr)) == 0
    fresh = Renderer(device=0)
    try:
        for started in (False, True):      # before pt_start_render; then a render started without mattes
            if started:
                fresh.startRender(scenes.cornell_scene("bench"), (8, 8), 1, max_bounces=2)
            assert fresh._lib.pt_read_matte_slots(fresh._h, abi.MATTE_INSTANCE, slots.ctypes.data) == BAD_STATE
            assert fresh._lib.pt_read_matte(fresh._h, abi.MATTE_INSTANCE, ids.ctypes.data, 1, cov.ctypes.data) == BAD_STATE
            assert fresh._lib.pt_pick(fresh._h, 0, 0, C.byref(pr)) == BAD_STATE
            assert b"mattes" in fresh._lib.pt_last_error()
    finally:
        fresh.close()
    g = Renderer(devices=[0, 0])
    try:
        o = g.matteOptions()
        o.enabled = 1
        assert g._lib.pt_set_matte_options(g._h, C.byref(o)) == UNSUPPORTED
        o.enabled = 0
        assert g._lib.pt_set_matte_options(g._h, C.byref(o)) == 0
        assert g._lib.pt_read_matte_slots(g._h, abi.MATTE_INSTANCE, slots.ctypes.data) == BAD_STATE
        assert g._lib.pt_pick(g._h, 0, 0, C.byref(pr)) == BAD_STATE
    finally:
        g.close()
