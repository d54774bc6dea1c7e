"""GPU: NaN samples on the device under both values of pt_render_params.nonfinite_policy.  The three seeded scenes that yield NaN samples
at 71x45 (tests/test_nonfinite_reference.py ties the host references used here to the oracle, and states conditions (a)-(e) of
adaptive_lib.NONFINITE_CONFIGS) through every kernel that writes the policy branch out: k_accumulate (however the samples are batched),
k_accumulate_aov, k_accumulate_gmon and k_gmon's resolve, k_accumulate_adaptive / k_accumulate_aov_adaptive and the criterion behind
them, the denoiser's prep and a-trous passes, k_postprocess, and the device group's merge.  Every image is compared with "the same bits,
or NaN on both sides"; pt_stats.nonfinite_samples is compared exactly."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import denoise_lib as dl  # noqa: E402
import oracle_lib  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer, make_params  # noqa: E402
from test_nonfinite_reference import NAN_SAMPLES  # noqa: E402  (the (sample, x, y) of the NaN samples, found there with the oracle)

pytestmark = pytest.mark.gpu

W, H = 71, 45
SEEDS = (24, 648, 996)
POLICIES = (abi.NONFINITE_PROPAGATE, abi.NONFINITE_ZERO)
AOVS = (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)
KEYS = ("acc", "albedo", "normal", "moments")


@pytest.fixture
def r(gpu_renderer):
    gpu_renderer.selectKernel(abi.INTEGRATOR_MIS)
    yield gpu_renderer
    o = abi.AdaptiveOptions()
    gpu_renderer._lib.pt_default_adaptive_options(C.byref(o))
    gpu_renderer.setAdaptiveOptions(o)
    d = abi.DenoiseOptions()
    gpu_renderer._lib.pt_default_denoise_options(C.byref(d))
    gpu_renderer.setDenoiseOptions(d)
    gpu_renderer.setPostProcessOptions(gpu_renderer.postProcessOptions())
    gpu_renderer.setTonemapOptions(gpu_renderer.tonemapOptions())
    gpu_renderer.setGmonOptions(cap=1.0)
    gpu_renderer.selectKernel(abi.INTEGRATOR_MIS)


def _bounces(seed):
    return 3 + seed % 7


def _assert_same(got, want, what):
    bad = ~al.same_bits_or_both_nan(got, want)
    if bad.ndim == 3:
        bad = bad.any(axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first (y, x) %s: device %s, reference %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:2].tolist(), want[bad][:2].tolist())


def _drive(r, step):
    """step = 0: everything at once; 1: render(1) until done; 5: uneven steps (5, 1, 3, 5, 1, 3, ...)."""
    if step == 0:
        r.render(0)
    else:
        k = 0
        while r.status() & abi.STATUS_DONE == 0:
            r.render(step if step == 1 else (5, 1, 3)[k % 3])
            k += 1
    r.wait()
    assert r.status() & abi.STATUS_DONE


def _oracle(seed, spp, integrator, policy, first=0, **kw):
    """(accumulator, non-finite count) of samples [first, first + spp) in the oracle."""
    o = oracle_lib.OracleScene(scenes.random_scene(seed), make_params(W, H, spp, _bounces(seed), integrator=integrator, nonfinite_policy=policy, **kw))
    try:
        acc = o.render(first, spp)
        return acc, int(o.stats().nonfinite)
    finally:
        o.close()


def _uniform(r, seed, spp, policy, aov=False, **kw):
    r.setAdaptiveOptions(enabled=0)
    r.setDenoiseOptions(enabled=1 if aov else 0)
    r.startRender(scenes.random_scene(seed), (W, H), spp, max_bounces=_bounces(seed), nonfinite_policy=policy, **kw)
    assert r.stats().nonfinite_samples == 0     # (the counter restarts with the render)


# ---- uniform renders: k_accumulate ---------------------------------------------------------------------------------------------------------
# samples_in_flight x how the render is driven, all nine pairs
BATCHINGS = [(1, 0), (3, 1), (128, 5), (1, 5), (3, 0), (128, 1), (1, 1), (3, 5), (128, 0)]


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("integrator", [abi.INTEGRATOR_SIMPLE, abi.INTEGRATOR_MIS])
@pytest.mark.parametrize("seed", SEEDS)
def test_uniform_render_and_counter_equal_the_oracle_however_batched(r, seed, integrator, policy):
    spp = 24
    want, n = _oracle(seed, spp, integrator, policy)
    assert n >= 1 and n == sum(1 for s, _x, _y in NAN_SAMPLES[seed] if s < spp)
    assert np.isfinite(want).all() == (policy == abi.NONFINITE_ZERO)
    r.selectKernel(integrator)
    # every seed under three of the nine pairs (each value of either axis once), seed 996 under all nine
    k = SEEDS.index(seed) * 3
    for sif, step in BATCHINGS if seed == 996 else BATCHINGS[k:k + 3]:
        _uniform(r, seed, spp, policy, samples_in_flight=sif)
        assert r.stats().samples_in_flight == min(sif, spp)
        _drive(r, step)
        what = "seed %d integrator %d policy %d sif %d step %d" % (seed, integrator, policy, sif, step)
        _assert_same(r.readbackAccumulator(), want, what)
        assert r.stats().nonfinite_samples == n, what
        assert r.stats().paths == spp * W * H
    # a restart sets the counter back; one sample of it counts what that sample holds
    _uniform(r, seed, 1, policy)
    _drive(r, 0)
    assert r.stats().nonfinite_samples == sum(1 for s, _x, _y in NAN_SAMPLES[seed] if s == 0)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("first,ends_on", [(17, True), (16, False)])
def test_nan_sample_at_the_end_and_at_the_start_of_a_batch(r, first, ends_on, policy):
    """Seed 996's second NaN is sample 20 of pixel (30, 43).  Batches of four from first_sample 17 end exactly on it ([17, 20], [21, 24]);
    from first_sample 16 the second batch begins on it ([16, 19], [20, 23])."""
    seed, spp = 996, 8
    want, n = _oracle(seed, spp, abi.INTEGRATOR_MIS, policy, first=first)
    assert n == 1 and (20 - first) % 4 == (3 if ends_on else 0)
    _uniform(r, seed, spp, policy, first_sample=first, samples_in_flight=4)
    assert r.stats().samples_in_flight == 4
    for _ in range(2):
        r.render(4)
        r.wait()
    assert r.status() & abi.STATUS_DONE and r.stats().batches == 2
    acc = r.readbackAccumulator()
    _assert_same(acc, want, "first_sample %d policy %d" % (first, policy))
    assert r.stats().nonfinite_samples == 1
    assert bool(np.isnan(acc[43, 30, :3]).all()) == (policy == abi.NONFINITE_PROPAGATE) and int(np.isnan(acc).any(axis=-1).sum()) == (1 - policy)


# ---- first-hit AOVs: k_accumulate_aov ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("seed,sif", [(996, 5), (648, 128)])
def test_uniform_aovs_equal_the_host_render_under_both_policies(r, seed, sif, policy):
    spp = 24
    hs = dl.HostScene(scenes.random_scene(seed), make_params(W, H, spp, _bounces(seed), nonfinite_policy=policy))
    want = hs.render(0, spp)
    pixels = sorted({(x, y) for _s, x, y in NAN_SAMPLES[seed]})
    assert hs.nonfinite == len(NAN_SAMPLES[seed]) >= 1
    _uniform(r, seed, spp, policy, aov=True, samples_in_flight=sif)
    _drive(r, 0)
    got = [r.readbackAccumulator()] + [r.readbackAov(k) for k in AOVS]
    for key, g, w in zip(KEYS, got, want):
        _assert_same(g, w, "%s seed %d policy %d" % (key, seed, policy))
    assert r.stats().nonfinite_samples == hs.nonfinite
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    nan = np.zeros((H, W), bool)
    for x, y in pixels:
        nan[y, x] = True
        m = got[3][y, x]
        if policy == abi.NONFINITE_PROPAGATE:
            assert np.isfinite(m[0]) and np.isnan(m[1]) and np.isnan(m[2]) and np.isnan(got[0][y, x, :3]).all()
        else:
            assert np.isfinite(m).all() and np.isfinite(got[0][y, x]).all()
    assert np.isfinite(got[0][~nan]).all() and np.isfinite(got[3][~nan]).all()
    # AOVs off: the same accumulator, the same counter
    _uniform(r, seed, spp, policy, aov=False, samples_in_flight=sif)
    _drive(r, 0)
    _assert_same(r.readbackAccumulator(), got[0], "AOVs off")
    assert r.stats().nonfinite_samples == hs.nonfinite


# ---- GMoN: k_accumulate_gmon and k_gmon ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("seed,spp,buckets,sif", [(996, 24, 6, 5), (996, 24, 24, 3), (648, 5, 5, 128)])
def test_gmon_buckets_resolve_and_counter_equal_the_oracle(r, seed, spp, buckets, sif, policy):
    """Sample f goes to bucket f / ceil(spp / buckets) with the running-mean weight f / buckets (the reference's, k_accumulate_gmon): a
    sample whose weight is 0 REPLACES what its bucket holds.  Seed 996, six buckets of four: NaN sample 20 stays in bucket 5 (weights 3),
    NaN sample 0 is overwritten by samples 1-3 of bucket 0 (weights 0) but still counted.  One sample per bucket (24 of 24, 5 of 5): every
    NaN sample is its bucket, so the resolve sorts a NaN bucket."""
    flags = abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON
    spb = -(-spp // buckets)
    o = oracle_lib.OracleScene(scenes.random_scene(seed), make_params(W, H, spp, _bounces(seed), flags=flags, gmon_buckets=buckets, nonfinite_policy=policy))
    try:
        ob, oresolved = o.render_gmon(spp)
        n = int(o.stats().nonfinite)
        assert n == len(NAN_SAMPLES[seed])
        for s, x, y in NAN_SAMPLES[seed]:
            nan_buckets = [b for b in range(buckets) if np.isnan(ob[b, y, x, :3]).any()]
            stays = all(f // buckets > 0 for f in range(s + 1, min(spp, (s // spb + 1) * spb)))
            assert nan_buckets == ([s // spb] if policy == abi.NONFINITE_PROPAGATE and stays else []), (s, x, y)
            assert stays == ((seed, buckets, s) != (996, 6, 0))
        for step in (0, 1):
            _uniform(r, seed, spp, policy, flags=flags, gmonBuckets=buckets, samples_in_flight=sif)
            _drive(r, step)
            for b in range(buckets):
                _assert_same(r.readGmonBucket(b), ob[b], "bucket %d policy %d step %d" % (b, policy, step))
            _assert_same(r.readbackAccumulator(), oresolved, "resolve policy %d step %d" % (policy, step))
            assert r.stats().nonfinite_samples == n
        r.setGmonOptions(cap=0.25)
        _uniform(r, seed, spp, policy, flags=flags, gmonBuckets=buckets, samples_in_flight=sif)
        _drive(r, 0)
        _assert_same(r.readbackAccumulator(), o.gmon_resolve(ob, (spp - 1) // spb + 1, cap=0.25), "resolve cap 0.25 policy %d" % policy)
    finally:
        o.close()


# ---- adaptive: k_accumulate_adaptive, k_accumulate_aov_adaptive, the criterion --------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    """The host references of every non-finite configuration, and the conditions (a)-(e) they are there for."""
    out = {name: al.reference(name) for name in sorted(al.NONFINITE_CONFIGS)}
    al.check_nonfinite_table({name: al.check_nonfinite_reference(name, ref) for name, ref in out.items()})
    return out


def _start_adaptive(r, name, **kw):
    kind, size, B, spp, m, i, thr, policy = al.config(name)
    r.setDenoiseOptions(enabled=1)
    r.setAdaptiveOptions(enabled=1, threshold=thr, min_spp=m, interval=i)
    r.startRender(al.config_scene(kind), size, spp, max_bounces=B, nonfinite_policy=policy, **kw)
    assert r.stats().nonfinite_samples == 0


def _assert_is_reference(r, ref, what):
    """tests/test_gpu_adaptive_matrix.py's rules, NaN-aware, and the counter.  Blocking reads: the counts first."""
    counts = r.readbackSampleCounts()
    assert np.array_equal(counts, ref["counts"]), "%s counts: device %s, reference %s" % (what, al.histogram(counts), al.histogram(ref["counts"]))
    got = dict(zip(KEYS, [r.readbackAccumulator()] + [r.readbackAov(k) for k in AOVS]))
    for key in KEYS:
        _assert_same(got[key], ref[key], "%s %s" % (what, key))
    st = r.stats()
    assert st.paths == int(ref["counts"].astype(np.uint64).sum()), what
    assert st.nonfinite_samples == int(ref["nonfinite"].sum()), what
    want = al.host_filter_counts(ref["acc"], ref["albedo"], ref["normal"], ref["moments"], ref["counts"])
    _assert_same(r.readbackDenoised(), want, what + " denoised")
    return got


@pytest.mark.parametrize("name", sorted(al.NONFINITE_CONFIGS))
def test_adaptive_render_with_nan_samples_equals_the_host_reference(r, refs, name):
    _start_adaptive(r, name)
    _drive(r, 0)
    got = _assert_is_reference(r, refs[name], name)
    assert bool(np.isnan(got["acc"]).any()) == (al.config(name)[7] == abi.NONFINITE_PROPAGATE)


@pytest.mark.parametrize("sif,step", BATCHINGS)
@pytest.mark.parametrize("name", ["nan996", "zero996"])
def test_adaptive_batchings_with_nan_samples_equal_the_host_reference(r, refs, name, sif, step):
    _start_adaptive(r, name, samples_in_flight=sif)
    assert r.stats().samples_in_flight == min(sif, al.config(name)[3])
    _drive(r, step)
    _assert_is_reference(r, refs[name], "%s sif %d step %d" % (name, sif, step))


def test_a_tile_that_stops_before_its_nan_counts_none(r, refs):
    """Threshold 2.0 on seed 996: the tile of (30, 43) stops at 4 samples, long before its NaN sample 20; the other NaN (sample 0) counts."""
    ref = refs["nan996_early"]
    assert ref["counts"][43, 30] == 4 and ref["nonfinite"][43, 30] == 0 and int(ref["nonfinite"].sum()) == 1
    _start_adaptive(r, "nan996_early", samples_in_flight=3)
    _drive(r, 1)
    got = _assert_is_reference(r, ref, "nan996_early sif 3 step 1")
    assert np.isfinite(got["acc"][40:, 24:32]).all() and np.isfinite(got["moments"][40:, 24:32]).all()
    assert r.stats().nonfinite_samples == 1


# ---- the denoiser: k_dn_prep / k_dn_prep_counts / k_atrous -----------------------------------------------------------------------------------
def _check_denoised(r, want_fn, nan_pixels, what):
    acc = r.readbackAccumulator()
    nan = np.isnan(acc).any(axis=-1)
    assert sorted((int(x), int(y)) for y, x in np.argwhere(nan)) == sorted(nan_pixels), what
    for iters in (1, 5):
        r.setDenoiseOptions(iterations=iters)
        den = r.readbackDenoised()
        _assert_same(den, want_fn(acc, iters), "%s iterations %d" % (what, iters))
        # a NaN pixel keeps its accumulator value; nothing else is NaN or inf
        _assert_same(den[nan][:, :3], acc[nan][:, :3], what + " NaN pixels")
        assert (den[nan][:, 3] == 1.0).all() and np.isfinite(den[~nan]).all(), what
        # the filter did run next to it: a finite pixel within its support (2 * (2^iters - 1) pixels) differs from its raw value
        reach = 2 * ((1 << iters) - 1)
        for x, y in nan_pixels:
            near = np.zeros((H, W), bool)
            near[max(0, y - reach):y + reach + 1, max(0, x - reach):x + reach + 1] = True
            near &= ~nan
            assert (den[near][:, :3] != acc[near][:, :3]).any(), (what, iters, x, y)


@pytest.mark.parametrize("seed", [996, 648])
def test_denoiser_on_a_uniform_render_with_nan_pixels(r, seed):
    spp = 24
    _uniform(r, seed, spp, abi.NONFINITE_PROPAGATE, aov=True)
    _drive(r, 0)
    a, n, m = (r.readbackAov(k) for k in AOVS)
    assert r.renderProgress()[0] == spp
    _check_denoised(r, lambda acc, iters: dl.host_filter(acc, a, n, m, spp, iterations=iters),
                    {(x, y) for _s, x, y in NAN_SAMPLES[seed]}, "uniform seed %d" % seed)


@pytest.mark.parametrize("name", ["nan996", "nan648"])
def test_denoiser_on_an_adaptive_render_with_nan_pixels(r, refs, name):
    _start_adaptive(r, name)
    _drive(r, 0)
    counts = r.readbackSampleCounts()
    assert np.array_equal(counts, refs[name]["counts"]) and len(np.unique(counts)) >= 5
    a, n, m = (r.readbackAov(k) for k in AOVS)
    seed = int(al.config(name)[0][6:])
    _check_denoised(r, lambda acc, iters: al.host_filter_counts(acc, a, n, m, counts, iterations=iters),
                    {(x, y) for _s, x, y in NAN_SAMPLES[seed]}, name)


# ---- the post-process: k_postprocess -------------------------------------------------------------------------------------------------------
def _present(r):
    ptr, stream = r.presentRenderTarget()
    assert ptr and stream
    r.wait()
    hip = abi.load_library()
    got = np.empty((H, W, 4), np.uint8)
    assert hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
    assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), C.c_void_p(ptr), C.c_size_t(got.nbytes), 2) == 0  # hipMemcpyDeviceToHost
    return got


@pytest.mark.parametrize("seed", [996, 648])
def test_postprocess_of_a_nan_accumulator_is_the_oracles_bytes(r, seed):
    spp = 24
    sc = scenes.random_scene(seed)
    _uniform(r, seed, spp, abi.NONFINITE_PROPAGATE, aov=True)
    _drive(r, 0)
    acc = r.readbackAccumulator()
    nan = np.isnan(acc).any(axis=-1)
    assert int(nan.sum()) == len(NAN_SAMPLES[seed])
    o = oracle_lib.OracleScene(sc, make_params(W, H, spp, _bounces(seed)))
    try:
        base = {}
        for tm in (abi.TONEMAP_NONE, abi.TONEMAP_AGX, abi.TONEMAP_KHRONOS_PBR, abi.TONEMAP_FLIM):
            for ca in (0.0, 40.0):
                po, to = r.postProcessOptions(), r.tonemapOptions()
                to.tonemapper = tm
                po.ca_amount = ca
                if tm in (abi.TONEMAP_KHRONOS_PBR, abi.TONEMAP_FLIM):     # non-default grading on two of them
                    po.exposure, po.contrast, po.saturation = 0.7, 12.0, -8.0
                    po.blacks, po.shadows, po.highlights, po.whites = 5.0, -10.0, 8.0, -4.0
                    po.vig_amount, po.vig_midpoint = -1.5, 10.0
                r.setPostProcessOptions(po)
                r.setTonemapOptions(to)
                r.setDenoiseOptions(apply_to_target=0)
                got = r.readbackRenderTarget()
                want = o.postprocess(acc, po, to)
                bad = (got != want).any(axis=-1)
                assert not bad.any(), "tonemapper %d ca %g: %d pixels differ, first (y, x) %s: device %s, oracle %s" % (
                    tm, ca, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:2].tolist(), want[bad][:2].tolist())
                assert np.array_equal(_present(r), want), (tm, ca)
                # chromatic aberration reads neighbours: with it, the NaN reaches pixels whose own accumulator is finite
                if ca == 0.0:
                    base[tm] = (po, to)
                else:
                    clean = np.where(nan[..., None], np.float32(0.0), acc)
                    hit = (o.postprocess(clean, po, to) != want).any(axis=-1)
                    assert (hit & ~nan).any(), tm
                # the denoised image as the target: the filter's NaN pixels through the same chain
                r.setDenoiseOptions(apply_to_target=1)
                den = r.readbackDenoised()
                assert np.array_equal(np.isnan(den).any(axis=-1), nan)
                want = o.postprocess(den, po, to)
                assert np.array_equal(r.readbackRenderTarget(), want), (tm, ca, "apply_to_target")
                assert np.array_equal(_present(r), want), (tm, ca, "apply_to_target, presented")
    finally:
        o.close()
        r.setDenoiseOptions(apply_to_target=0)


# ---- the device group: multi_device.hip ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_device_group_counts_and_merges_nan_samples(policy):
    """Two members on device 0 render samples [0, 12) and [12, 24) of seed 996: each of them meets one NaN sample (0 and 20), at pixels of
    its own."""
    seed, spp = 996, 24
    sc = scenes.random_scene(seed)
    lib = abi.load_library()
    first, count = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    abi.check(lib, lib.pt_group_partition(spp, 2, abi.FLAG_MULTISCATTER_GGX, 1, first, count, None, None))
    assert list(first) == [0, 12] and list(count) == [12, 12]
    single = Renderer(device=0)
    try:
        single.startRender(sc, (W, H), spp, max_bounces=_bounces(seed), nonfinite_policy=policy)
        single.render(0)
        single.wait()
        ref, n = single.readbackAccumulator(), single.stats().nonfinite_samples
        parts = []
        for f, c in zip(first, count):
            single.startRender(sc, (W, H), c, max_bounces=_bounces(seed), first_sample=f, nonfinite_policy=policy)
            single.render(0)
            single.wait()
            parts.append((single.readbackAccumulator(), single.stats().nonfinite_samples))
    finally:
        single.close()
    assert n == 2 and [p[1] for p in parts] == [1, 1]
    g = Renderer(devices=[0, 0])
    try:
        g.startRender(sc, (W, H), spp, max_bounces=_bounces(seed), nonfinite_policy=policy)
        assert g.stats().nonfinite_samples == 0
        g.render(0)
        g.wait()
        got, st = g.readbackAccumulator(), g.stats()
    finally:
        g.close()
    assert st.nonfinite_samples == n and st.paths == spp * W * H
    member_nan = np.isnan(parts[0][0]).any(axis=-1) | np.isnan(parts[1][0]).any(axis=-1)
    if policy == abi.NONFINITE_PROPAGATE:
        assert sorted((int(x), int(y)) for y, x in np.argwhere(member_nan)) == sorted((x, y) for _s, x, y in NAN_SAMPLES[seed])
        assert np.array_equal(np.isnan(got[..., :3]).all(axis=-1), member_nan) and np.array_equal(np.isnan(got).any(axis=-1), member_nan)
        assert np.array_equal(np.isnan(ref).any(axis=-1), member_nan)
    else:
        assert not member_nan.any() and np.isfinite(got).all() and np.isfinite(ref).all()
    assert not np.isinf(got).any()
    ok = ~member_nan
    np.testing.assert_allclose(got[ok][:, :3], ref[ok][:, :3], rtol=2e-6, atol=1e-6)     # (fp32 summation order, as tests/test_device_group.py)
    assert (got[..., 3] == 1.0).all()
