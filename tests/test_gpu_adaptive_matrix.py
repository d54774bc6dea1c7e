"""GPU: tile-adaptive sampling and the first-hit AOVs against a prediction made without the device (adaptive_lib.reference_render, which
tests/test_adaptive_reference.py ties to the oracle), bit for bit, where the virtual tile -> segment -> Lbuf window -> image tile mapping
is not the trivial one: partial edge tiles on both axes, several tiles per segment, band counts that do not divide the tile grid,
checkpoint grids the batch does not divide, first_sample != 0, the SIMPLE integrator; and in the middle of what a viewport does with a
running adaptive render: blocking reads, debug and measure batches, restarts of other sizes and kinds, a restart over a checkpoint in flight.
At full size, where the planner itself chooses several tiles per segment, the reference is the same renderer's uniform renders (and the
oracle on probe pixels)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import denoise_lib as dl  # noqa: E402
import oracle_lib  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer, make_params  # noqa: E402

pytestmark = pytest.mark.gpu

AOVS = (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)
KEYS = ("acc", "albedo", "normal", "moments")


def _restore(r):
    o = abi.AdaptiveOptions()
    r._lib.pt_default_adaptive_options(C.byref(o))
    r.setAdaptiveOptions(o)
    d = abi.DenoiseOptions()
    r._lib.pt_default_denoise_options(C.byref(d))
    r.setDenoiseOptions(d)
    r.selectKernel(abi.INTEGRATOR_MIS)


@pytest.fixture
def r(gpu_renderer):
    gpu_renderer.selectKernel(abi.INTEGRATOR_MIS)
    yield gpu_renderer
    _restore(gpu_renderer)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _drive(r, step):
    """step = 0: everything at once; else render(step) until the render is done."""
    if step == 0:
        r.render(0)
    else:
        while r.status() & abi.STATUS_DONE == 0:
            r.render(step)


def _start(r, name, min_spp=None, interval=None, adaptive=True, aov=True, **kw):
    kind, size, B, spp, m, i, thr = al.CONFIGS[name]
    m, i = (m, i) if min_spp is None else (min_spp, interval)
    r.setDenoiseOptions(enabled=1 if aov else 0)
    r.setAdaptiveOptions(enabled=1 if adaptive else 0, threshold=thr, min_spp=m, interval=i)
    r.startRender(al.config_scene(kind), size, spp, max_bounces=B, **kw)


def _state(r, aov=True):
    """Blocking reads (they flush what is pending): the counts first, so that every image belongs to them."""
    out = dict(counts=r.readbackSampleCounts(), acc=r.readbackAccumulator())
    if aov:
        for key, k in zip(KEYS[1:], AOVS):
            out[key] = r.readbackAov(k)
        out["denoised"] = r.readbackDenoised()
    out["paths"] = r.stats().paths
    return out


def _assert_is_reference(got, ref, what=""):
    assert np.array_equal(got["counts"], ref["counts"]), "%s counts: device %s, reference %s" % (what, al.histogram(got["counts"]), al.histogram(ref["counts"]))
    for key in KEYS:
        if key in got:
            bad = (_bits(got[key]) != _bits(ref[key])).any(axis=-1)
            assert not bad.any(), "%s %s: %d pixels differ, first (y, x) %s" % (what, key, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert got["paths"] == int(ref["counts"].astype(np.uint64).sum()), what
    if "denoised" in got:
        want = al.host_filter_counts(ref["acc"], ref["albedo"], ref["normal"], ref["moments"], ref["counts"])
        assert np.array_equal(_bits(got["denoised"]), _bits(want)), what + " denoised"


def _populated(name, ref):
    _kind, (W, H), _B, spp, _m, _i, _t = al.CONFIGS[name]
    al.check_populated(ref["counts"], spp, W, H)


# ---- B. the device equals the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(al.CONFIGS))
def test_adaptive_render_equals_the_host_reference(r, name):
    ref = al.reference(name)
    _populated(name, ref)
    _start(r, name)
    _drive(r, 0)
    r.wait()
    assert r.status() & abi.STATUS_DONE
    _assert_is_reference(_state(r), ref, name)


@pytest.mark.parametrize("kind,size,B,spp,kw", [("cornell", (64, 48), 4, 16, dict(samples_in_flight=5)),
                                                ("textured", (96, 54), 6, 8, dict(first_sample=1000))])
def test_uniform_aovs_of_several_samples_equal_the_host_render(r, kind, size, B, spp, kw):
    sc = al.config_scene(kind)
    first = kw.get("first_sample", 0)
    want = dl.HostScene(sc, make_params(size[0], size[1], spp, B, first_sample=first)).render(first, spp)
    r.setDenoiseOptions(enabled=1)
    r.setAdaptiveOptions(enabled=0)
    r.startRender(sc, size, spp, max_bounces=B, **kw)
    r.render(0)
    r.wait()
    got = [r.readbackAccumulator()] + [r.readbackAov(k) for k in AOVS]
    assert (r.readbackSampleCounts() == spp).all()
    for key, g, w in zip(KEYS, got, want):
        bad = (_bits(g) != _bits(w)).any(axis=-1)
        assert not bad.any(), "%s: %d pixels differ, first (y, x) %s" % (key, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert want[2][..., :3].any() and want[3][..., 1].any()


# (min_spp, interval) x samples_in_flight x how the render is driven: a Latin square, every value three times
SCHEDULES = [((2, 1), 1, 0), ((2, 1), 3, 1), ((2, 1), 128, 5),
             ((5, 7), 1, 5), ((5, 7), 3, 0), ((5, 7), 128, 1),
             ((16, 16), 1, 1), ((16, 16), 3, 5), ((16, 16), 128, 0)]


@pytest.mark.parametrize("schedule,sif,step", SCHEDULES)
def test_schedules_and_batchings_equal_the_host_reference(r, schedule, sif, step):
    name = "cornell67"
    ref = al.reference(name, *schedule)
    _populated(name, ref)
    _start(r, name, *schedule, samples_in_flight=sif)
    assert r.stats().samples_in_flight == min(sif, al.CONFIGS[name][3])
    _drive(r, step)
    r.wait()
    assert r.status() & abi.STATUS_DONE
    _assert_is_reference(_state(r), ref, "%s sif %d step %d" % (schedule, sif, step))


def test_first_sample_1000_equals_the_host_reference(r):
    name = "cornell67"
    ref = al.reference(name, first_sample=1000)
    tc = al.tile_counts(ref["counts"])
    assert (tc < 96).any() and (tc == 96).any() and len(np.unique(tc)) >= 3
    assert not np.array_equal(_bits(ref["acc"]), _bits(al.reference(name)["acc"]))
    _start(r, name, first_sample=1000)
    _drive(r, 0)
    r.wait()
    _assert_is_reference(_state(r), ref, "first_sample 1000")


def test_simple_integrator_equals_the_host_reference(r):
    name = "textured99"   # (without light sampling the Cornell configurations have two classes only: black tiles and tiles that never converge)
    ref = al.reference(name, integrator=abi.INTEGRATOR_SIMPLE)
    tc = al.tile_counts(ref["counts"])
    assert (tc < 64).any() and (tc == 64).any() and len(np.unique(tc)) >= 3
    assert not np.array_equal(_bits(ref["acc"]), _bits(al.reference(name)["acc"]))
    r.selectKernel(abi.INTEGRATOR_SIMPLE)
    try:
        _start(r, name)
        _drive(r, 0)
        r.wait()
        got = _state(r)
    finally:
        r.selectKernel(abi.INTEGRATOR_MIS)
    _assert_is_reference(got, ref, "SIMPLE")


# ---- C. queue layouts -------------------------------------------------------------------------------------------------------------------
def _plan(w, h, spp, sif=0, tps=0, bands=4, free=200 << 30):
    q = abi.QueuePlan()
    lib = abi.load_library()
    abi.check(lib, lib.pt_plan_queues(w, h, spp, sif, free, tps, bands, C.byref(q)))
    return q


@pytest.mark.parametrize("bands", [1, 4, 7])
@pytest.mark.parametrize("tps", [3, 16])
def test_queue_layouts_equal_the_host_reference(tps, bands):
    """3 and 7 are coprime to the 17 x 12 tile grid and to each other: segments straddle tile rows, the last segment of a band is partly
    empty, and the adaptive list's virtual tiles fall into segments that hold other image tiles at every checkpoint."""
    preset = [v for v in ("PTAMD_TILES_PER_SEG", "PTAMD_SEG_BANDS") if v in os.environ]
    if preset:
        pytest.skip("preset for the whole session: " + ", ".join(preset))
    name = "cornell131"
    _kind, (W, H), _B, spp, _m, _i, _t = al.CONFIGS[name]
    ref = al.reference(name)
    _populated(name, ref)
    q = _plan(W, H, spp, 0, tps, bands)
    assert q.tiles_per_seg == tps and q.nseg % bands == 0 and q.nseg * tps >= 17 * 12
    assert q.samples_in_flight <= (64 if tps == 16 else 128)
    os.environ["PTAMD_TILES_PER_SEG"], os.environ["PTAMD_SEG_BANDS"] = str(tps), str(bands)
    try:
        rr = Renderer(device=0)
    finally:
        del os.environ["PTAMD_TILES_PER_SEG"], os.environ["PTAMD_SEG_BANDS"]
    try:
        _start(rr, name)
        assert rr.stats().samples_in_flight == q.samples_in_flight
        _drive(rr, 0)
        rr.wait()
        got = _state(rr)
    finally:
        rr.close()
    _assert_is_reference(got, ref, "tiles_per_seg %d, bands %d" % (tps, bands))


# ---- D. interaction with a running adaptive render --------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [40, 32])
def test_reads_in_the_middle_of_a_render(r, at):
    name = "cornell131"
    mid, ref = al.reference(name, stop_at=at), al.reference(name)
    assert set(np.unique(mid["counts"]).tolist()) == {16, 32, at}
    _start(r, name)
    r.render(at)
    _assert_is_reference(_state(r), mid, "after %d samples" % at)
    assert r.renderProgress() == (at, 128) and r.status() & abi.STATUS_DONE == 0
    r.render(0)
    r.wait()
    _assert_is_reference(_state(r), ref, "finished after reads at %d" % at)


def _debug_calls(r):
    prim = r.tracePrimary(3)
    rad, hits = r.debugSample(3)
    r.measureTraversal(0)
    st = r.stats()
    return prim.tobytes(), rad.tobytes(), hits.tobytes(), (st.nodes_per_closest_ray, st.tris_per_closest_ray, st.nodes_per_shadow_ray, st.tris_per_shadow_ray)


def test_debug_and_measure_batches_in_the_middle_of_a_render(r):
    name = "cornell131"
    ref = al.reference(name)
    _start(r, name, adaptive=False, aov=False)
    r.render(40)
    r.wait()
    want = _debug_calls(r)
    assert want[3][0] > 0 and any(want[1])
    _start(r, name)
    r.render(40)
    r.wait()
    got = _debug_calls(r)
    assert got == want
    r.render(0)
    r.wait()
    _assert_is_reference(_state(r), ref, "after debug batches")


def test_restarts_of_other_sizes_and_kinds_on_one_renderer(r):
    for step, name in enumerate(("cornell131", "cornell67")):
        _start(r, name)
        _drive(r, 0)
        r.wait()
        _assert_is_reference(_state(r), al.reference(name), "restart %d" % (step + 1))
    # 3. uniform, AOVs off
    name = "cornell131"
    kind, (W, H), _B, spp, _m, _i, _t = al.CONFIGS[name]
    _start(r, name, adaptive=False, aov=False)
    _drive(r, 0)
    r.wait()
    o = oracle_lib.OracleScene(al.config_scene(kind), al.config_params(name))
    try:
        want = o.render(0, spp)
    finally:
        o.close()
    assert np.array_equal(_bits(r.readbackAccumulator()), _bits(want))
    assert (r.readbackSampleCounts() == spp).all() and r.stats().paths == spp * W * H
    buf = np.zeros((H, W, 4), np.float32)
    assert r._lib.pt_read_aov(r._h, abi.AOV_MOMENTS, buf.ctypes.data) == -5     # PT_ERR_BAD_STATE
    for step, name in enumerate(("textured99", "cornell131")):
        _start(r, name)
        _drive(r, 0)
        r.wait()
        _assert_is_reference(_state(r), al.reference(name), "restart %d" % (step + 4))


def test_restart_over_a_checkpoint_in_flight(r):
    first, second = "cornell131", "cornell67"
    ref = al.reference(second)
    _start(r, first)
    r.render(0)                      # no wait: batches and checkpoints of this render are still in flight
    _start(r, second)
    assert r.status() & abi.STATUS_DONE == 0 and r.renderProgress() == (0, al.CONFIGS[second][3])
    r.render(0)
    r.wait()
    assert r.status() & abi.STATUS_DONE and r.renderProgress() == (96, 96)
    _assert_is_reference(_state(r), ref, "second render")


# ---- E. full size: the planner's own several tiles per segment ----------------------------------------------------------------------------
# Thresholds: chosen once, on an MI355X, from the UNIFORM renders' moments with adaptive_lib.host_tiles (the reference criterion, not the
# adaptive path): the first value of the ladder 0.05, 0.1, 0.2, 0.3, 0.5 that stops between 15 % and 85 % of the tiles before spp.  The
# tests assert that share and at least 3 distinct counts; they never pick a value.
# Cornell 2051x1029, 4 bounces, spp 64 / 16 / 16, tiles by count (of 33 153):
#   0.05: 16: 7353, 32: 10, 48: 4, 64: 25786 (22.2 % early)  <- chosen
#   0.1 : 16: 7373, 32: 79, 48: 103, 64: 25598 (22.8 %);  0.2: 16: 8714, 32: 1822, 48: 1814, 64: 20803 (37.3 %)
FULL_CORNELL_THRESHOLD = 0.05
# The atrium (C5) at 3840x2160, 12 bounces, spp 48 / 16 / 16, tiles by count (of 129 600): no value of the ladder lies in the band,
#   0.05: 16: 3015, 32: 118, 48: 126467 (2.4 %);  0.3: 16: 3256, 32: 560, 48: 125784 (2.9 %);  0.5: 16: 5435, 32: 10912, 48: 113253 (12.6 %)
# and neither does the ladder continued (1.0: 16: 95333, 32: 30084, 48: 4183, 96.8 %; 2.0: all but 3 tiles at 16): the scene's error
# distribution is steep between 0.5 and 1.  0.7, the one value tried in between, by the same rule from the same uniform moments:
#   0.7 : 16: 24508, 32: 29680, 48: 75412 (41.8 % early)  <- chosen
FULL_C5_THRESHOLD = 0.7


def _uniform(r, sc, size, B, n):
    r.setDenoiseOptions(enabled=1)
    r.setAdaptiveOptions(enabled=0)
    r.startRender(sc, size, n, max_bounces=B)
    r.render(0)
    r.wait()
    return [r.readbackAccumulator()] + [r.readbackAov(k) for k in AOVS]


def _full_size_case(r, sc, W, H, B, spp, m, i, thr, tps):
    """The adaptive render against the same renderer's uniform renders of every count, the host criterion on their moments against
    every verdict, paths against the counts.  Returns (counts, accumulator)."""
    assert _plan(W, H, spp).tiles_per_seg == tps
    cps = al.checkpoints(spp, m, i)
    r.setDenoiseOptions(enabled=1)
    r.setAdaptiveOptions(enabled=1, threshold=thr, min_spp=m, interval=i)
    r.startRender(sc, (W, H), spp, max_bounces=B)
    r.render(0)
    r.wait()
    counts, acc = r.readbackSampleCounts(), r.readbackAccumulator()
    aov = [r.readbackAov(k) for k in AOVS]
    assert r.stats().paths == int(counts.astype(np.uint64).sum())
    tc = al.tile_counts(counts)
    assert np.array_equal(np.kron(tc, np.ones((8, 8), np.uint32))[:H, :W], counts)
    distinct = sorted(set(tc.ravel().tolist()))
    early = float((tc < spp).mean())
    print("%dx%d threshold %g: tiles by count %s, %.1f %% stop early" % (W, H, thr, al.histogram(counts), 100 * early))
    assert len(distinct) >= 3 and distinct[-1] == spp and set(distinct) <= set(cps) | {spp}, distinct
    assert 0.15 <= early <= 0.85, early
    open_ = np.ones(tc.shape, bool)
    for n in cps + [spp]:
        u = _uniform(r, sc, (W, H), B, n)
        sel = counts == n
        for k, (g, w) in enumerate(zip([acc] + aov, u)):
            assert np.array_equal(_bits(g[sel]), _bits(w[sel])), (n, KEYS[k])
        if n < spp:
            verdict = al.host_tiles(u[3], n, thr)
            assert np.array_equal(verdict & open_, tc == n), n
            open_ &= ~verdict
        del u
    assert np.array_equal(open_, tc == spp)
    return counts, acc


def test_full_size_cornell_two_tiles_per_segment(r):
    t0 = time.perf_counter()
    W, H = 2051, 1029
    assert ((W + 7) // 8, (H + 7) // 8) == (257, 129)
    _full_size_case(r, al.config_scene("cornell"), W, H, 4, 64, 16, 16, FULL_CORNELL_THRESHOLD, 2)
    print("Cornell %dx%d adaptive == uniform renders of each count, %.1f s" % (W, H, time.perf_counter() - t0))


def test_full_size_c5_four_tiles_per_segment(r, tmp_path):
    from test_gpu_full_size import _probe_pixels
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))
    import export_gltf
    t0 = time.perf_counter()
    _factory, W, H, _spp, B = scenes.CONFIGS["c5"]
    assert (W, H, B) == (3840, 2160, 12)
    sc = export_gltf.atrium_through_ingestion(str(tmp_path))
    spp = 48
    counts, acc = _full_size_case(r, sc, W, H, B, spp, 16, 16, FULL_C5_THRESHOLD, 4)
    # probe pixels against the oracle, grouped by their count
    r.setAdaptiveOptions(enabled=0)
    r.setDenoiseOptions(enabled=0)
    r.startRender(sc, (W, H), 1, max_bounces=B)
    ids = r.tracePrimary(0)["instance"]
    px = {tuple(p) for p in _probe_pixels(W, H, ids)[::4].tolist()}
    # both sides of borders between tiles of different counts
    tc = al.tile_counts(counts)
    ys, xs = np.nonzero(tc[:, :-1] != tc[:, 1:])
    rng = np.random.default_rng(11)
    borders = 0
    for k in rng.choice(len(xs), size=min(24, len(xs)), replace=False):
        y = min(H - 1, 8 * int(ys[k]) + int(rng.integers(0, 8)))
        px.update({(8 * int(xs[k]) + 7, y), (8 * int(xs[k]) + 8, y)})
        borders += 1
    ys, xs = np.nonzero(tc[:-1, :] != tc[1:, :])
    for k in rng.choice(len(xs), size=min(24, len(xs)), replace=False):
        x = min(W - 1, 8 * int(xs[k]) + int(rng.integers(0, 8)))
        px.update({(x, 8 * int(ys[k]) + 7), (x, 8 * int(ys[k]) + 8)})
        borders += 1
    assert borders >= 32
    xy = np.array(sorted(px), dtype=np.uint32)
    assert 250 <= len(xy) <= 450, len(xy)
    o = oracle_lib.OracleScene(sc, make_params(W, H, spp, B))
    try:
        n_of = counts[xy[:, 1], xy[:, 0]]
        assert len(np.unique(n_of)) >= 3
        for n in np.unique(n_of):
            sel = xy[n_of == n]
            want = o.render_pixels(sel, 0, int(n))
            got = acc[sel[:, 1], sel[:, 0]]
            bad = ~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))).all(axis=1)
            assert not bad.any(), "count %d, pixels %s: HIP %s oracle %s" % (n, sel[bad][:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())
    finally:
        o.close()
    print("C5 %dx%d adaptive == uniform renders of each count, %d probe pixels == oracle, %.1f s" % (W, H, len(xy), time.perf_counter() - t0))
