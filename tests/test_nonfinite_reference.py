"""CPU: NaN samples under both values of pt_render_params.nonfinite_policy, with no GPU in the loop.  The host render
(denoise_lib.HostScene, tests/emu/denoise_emu.cpp) against the oracle on the three seeded scenes that yield NaN samples at 71x45, image
and counter; and adaptive_lib.NONFINITE_CONFIGS, the adaptive renders tests/test_gpu_nonfinite.py compares the device with: what each of
them is there for (conditions (a)-(e) below), the oracle per count class under the same policy, and the verdicts on the NaN pixels.

The conditions a non-finite configuration's reference meets before anything is compared with it:
 (a) the oracle sees >= 1 non-finite sample among the samples the render draws (and the reference counted exactly those, per pixel);
 (b) under propagate, a tile that drew a NaN sample holds counts == spp, its NaN pixels NaN in the accumulator and in moments .g / .b;
 (c) over the table, some tile stops before its first non-finite sample and is finite everywhere;
 (d) some configuration has >= 5 count classes and a NaN pixel in a partial edge tile;
 (e) under PT_NONFINITE_ZERO the accumulator and the moments are finite everywhere and >= 1 sample was zeroed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import denoise_lib as dl  # noqa: E402
import oracle_lib  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import make_params  # noqa: E402

SEEDS = (24, 648, 996)
W, H = 71, 45
# the NaN samples (sample, x, y) of the first 24 (seed 24), 32 (648) and 48 (996) samples, as found when the configurations were chosen
NAN_SAMPLES = {24: ((1, 16, 4), (7, 3, 0)), 648: ((0, 68, 23),), 996: ((0, 7, 34), (20, 30, 43))}
# tiles by count of each reference when it was chosen, its non-finite count, and the conditions it carries.  zero996: the configuration
# of nan996; both tiles of a zeroed sample now stop (at 32 and 40).  zero648: the first threshold of 0.6, 0.8, 1.0 under which the
# PT_NONFINITE_ZERO render has more count classes than nan648 (1.0 stops every tile at the first checkpoint).
HISTOGRAMS = {
    "nan996": ({4: 15, 8: 2, 12: 6, 16: 2, 20: 7, 24: 4, 28: 4, 32: 3, 44: 4, 48: 7}, 2, "abd"),
    "nan996_early": ({4: 53, 48: 1}, 1, "abc"),
    "nan24": ({2: 53, 24: 1}, 1, "abc"),
    "nan648": ({8: 1, 11: 1, 14: 2, 17: 2, 26: 2, 32: 46}, 1, "abd"),
    "zero996": ({4: 15, 8: 2, 12: 6, 16: 2, 20: 7, 24: 4, 28: 4, 32: 4, 40: 1, 44: 4, 48: 5}, 2, "ade"),
    "zero648": ({5: 5, 8: 2, 11: 3, 14: 2, 17: 2, 20: 3, 23: 6, 26: 5, 29: 10, 32: 16}, 1, "ade"),
}


@pytest.mark.parametrize("policy", [abi.NONFINITE_PROPAGATE, abi.NONFINITE_ZERO])
@pytest.mark.parametrize("integrator", [abi.INTEGRATOR_SIMPLE, abi.INTEGRATOR_MIS])
@pytest.mark.parametrize("seed", SEEDS)
def test_host_render_equals_the_oracle_under_both_policies(seed, integrator, policy):
    sc, B, spp = scenes.random_scene(seed), 3 + seed % 7, 24
    p = make_params(W, H, spp, B, integrator=integrator, nonfinite_policy=policy)
    o = oracle_lib.OracleScene(sc, p)
    try:
        want = o.render(0, spp)
        n = int(o.stats().nonfinite)
    finally:
        o.close()
    assert n >= 1
    hs = dl.HostScene(sc, p)
    px = np.zeros((H, W), np.uint32)
    got = hs.render(0, spp, nonfinite=px)
    assert al.same_bits_or_both_nan(got[0], want).all()
    assert hs.nonfinite == n and int(px.sum()) == n
    expect = [(x, y) for s, x, y in NAN_SAMPLES[seed] if s < spp]
    assert sorted((int(x), int(y)) for y, x in np.argwhere(px)) == sorted(expect)
    if policy == abi.NONFINITE_ZERO:
        assert all(np.isfinite(g).all() for g in got)
        # the other pixels are the propagating render's; the NaN pixels differ from it in the accumulator and the luminance moments only
        prop = dl.HostScene(sc, make_params(W, H, spp, B, integrator=integrator)).render(0, spp)
        nan = np.isnan(prop[0]).any(axis=-1)
        assert sorted((int(x), int(y)) for y, x in np.argwhere(nan)) == sorted(expect)
        for g, w in zip(got, prop):
            assert np.array_equal(g[~nan].view(np.uint32), w[~nan].view(np.uint32))
        assert np.array_equal(got[1][nan], prop[1][nan]) and np.array_equal(got[2][nan], prop[2][nan])
        assert np.array_equal(got[3][nan][:, 0], prop[3][nan][:, 0])
    else:
        nan = np.isnan(got[0][..., :3]).all(axis=-1)
        assert sorted((int(x), int(y)) for y, x in np.argwhere(nan)) == sorted(expect)
        assert np.isnan(got[3][nan][:, 1:3]).all() and np.isfinite(got[3][~nan]).all()
        assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all() and np.isfinite(got[0][~nan]).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_the_scenes_still_yield_the_recorded_nan_samples(seed):
    name = {24: "nan24", 648: "nan648", 996: "nan996"}[seed]
    assert al.oracle_nonfinite_samples(name) == NAN_SAMPLES[seed]
    kind, _size, B, spp, _m, _i, _t, _p = al.config(name)
    # none of them is an inf: the oracle's propagating render of all spp samples is NaN there
    o = oracle_lib.OracleScene(al.config_scene(kind), make_params(W, H, spp, B))
    try:
        acc = o.render(0, spp)
    finally:
        o.close()
    assert not np.isinf(acc).any() and int(np.isnan(acc).any(axis=-1).sum()) == len(NAN_SAMPLES[seed])


def _facts():
    return {name: al.check_nonfinite_reference(name, al.reference(name)) for name in sorted(al.NONFINITE_CONFIGS)}


def test_conditions_of_the_non_finite_configurations():
    facts = _facts()
    al.check_nonfinite_table(facts)
    for name, (classes, spared, edge) in facts.items():
        ref = al.reference(name)
        hist, nonfinite, carries = HISTOGRAMS[name]
        tc = al.tile_counts(ref["counts"])
        print("%s: tiles by count %s; %d non-finite; spared tiles %s; NaN pixels in partial edge tiles %s" %
              (name, al.histogram(ref["counts"]), int(ref["nonfinite"].sum()), spared, edge))
        assert {n: int((tc == n).sum()) for n in classes} == hist, name
        assert int(ref["nonfinite"].sum()) == nonfinite, name
        assert ("c" in carries) == bool(spared) and ("d" in carries) == (len(classes) >= 5 and bool(edge)), name
        assert ("b" in carries) == (al.config(name)[7] == abi.NONFINITE_PROPAGATE) and ("e" in carries) != ("b" in carries), name
    # (c) by name: threshold 2.0 on seed 996 spares the tile of (30, 43), seed 24 the tile of (3, 0)
    assert facts["nan996_early"][1] == [(5, 3)] and facts["nan24"][1] == [(0, 0)]
    assert facts["nan996"][2] == [(30, 43)]
    # the policy changes the render: the tiles of both zeroed samples of seed 996 stop before spp
    z, n = al.reference("zero996")["counts"], al.reference("nan996")["counts"]
    assert (n[34, 7], n[43, 30]) == (48, 48) and (z[34, 7], z[43, 30]) == (32, 40)
    assert int((al.tile_counts(z) != al.tile_counts(n)).sum()) == 2


@pytest.mark.parametrize("name", sorted(al.NONFINITE_CONFIGS))
def test_non_finite_reference_equals_the_oracle_per_count_class(name):
    kind, _size, _B, _spp, _m, _i, _t, policy = al.config(name)
    ref = al.reference(name)
    classes, _spared, _edge = al.check_nonfinite_reference(name, ref)
    o = oracle_lib.OracleScene(al.config_scene(kind), al.config_params(name))     # (the configuration's policy)
    try:
        assert o.params.nonfinite_policy == policy
        for n in classes:
            sel = ref["counts"] == n
            want = o.render(0, n)
            assert al.same_bits_or_both_nan(ref["acc"][sel], want[sel]).all(), n
            if policy == abi.NONFINITE_ZERO:
                assert np.isfinite(want).all()
    finally:
        o.close()


@pytest.mark.parametrize("name", sorted(n for n, c in al.NONFINITE_CONFIGS.items() if c[7] == abi.NONFINITE_PROPAGATE))
def test_a_nan_pixel_is_never_converged_and_keeps_its_tile_open(name):
    _kind, _size, _B, spp, m, i, thr, _policy = al.config(name)
    ref = al.reference(name)
    al.check_nonfinite_reference(name, ref)
    trace = ref["trace"]
    assert [c for c, _, _ in trace] == al.checkpoints(spp, m, i)
    drawn = [(s, x, y) for s, x, y in al.oracle_nonfinite_samples(name) if s < ref["counts"][y, x]]
    judged = 0
    for s, x, y in drawn:
        for c, mom, active in trace:
            m1, m2 = mom[y, x, 1], mom[y, x, 2]
            if c <= s:
                assert np.isfinite(m1) and np.isfinite(m2)
                continue
            judged += 1
            assert np.isnan(m1) and np.isnan(m2)
            assert not al.np_converged(m1, m2, c, thr) and not (al.np_error(m1, m2, c) <= thr)
            assert not (al.host_error(np.float32([m1]), np.float32([m2]), c)[0] <= np.float32(thr))
            assert not al.host_tiles(mom, c, thr)[y // 8, x // 8] and active[y // 8, x // 8]
    assert judged >= 1
    # the float64 verdicts on every other pixel of those tiles would have closed some of them: it is the NaN that keeps them open
    if name == "nan996":
        closed = 0
        for s, x, y in drawn:
            t = al.tile_view(ref["counts"], H, W)[y // 8][x // 8]
            for c, mom, _active in trace:
                if c > s:
                    v = al.np_converged(mom[t][..., 1], mom[t][..., 2], c, thr)
                    closed += int(v.sum() == v.size - 1)
        assert closed >= 1


def test_host_filter_keeps_exactly_the_nan_pixels():
    for name in sorted(al.NONFINITE_CONFIGS):
        ref = al.reference(name)
        den = al.host_filter_counts(ref["acc"], ref["albedo"], ref["normal"], ref["moments"], ref["counts"])
        nan = np.isnan(ref["acc"]).any(axis=-1)
        assert np.array_equal(np.isnan(den).any(axis=-1), nan) and np.isfinite(den[~nan]).all(), name
        assert (al.config(name)[7] == abi.NONFINITE_PROPAGATE) == bool(nan.any())
