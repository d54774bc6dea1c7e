"""CPU: adaptive_lib.reference_render, the prediction of a whole tile-adaptive render (counts, accumulator, AOVs) with no GPU in the
loop, checked against the oracle (oracle/pt_oracle.cpp) per count class, against the float64 restatement of the criterion per pixel and
checkpoint, and in its degenerate cases.  tests/test_gpu_adaptive_matrix.py compares the device with the same reference."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import denoise_lib as dl  # noqa: E402
import oracle_lib  # noqa: E402
from platinum_amd.renderer import make_params  # noqa: E402

# the tile histograms the three configurations gave when they were chosen (tiles by count)
HISTOGRAMS = {
    "cornell131": {16: 41, 32: 7, 48: 13, 64: 5, 80: 5, 96: 5, 112: 3, 128: 125},
    "textured99": {8: 29, 16: 7, 24: 3, 32: 5, 40: 4, 48: 5, 56: 2, 64: 36},
}
EARLY_EDGE_TILES = {"cornell131": 23, "cornell67": 14, "textured99": 15}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _populated(name, ref):
    _kind, (W, H), _B, spp, _m, _i, _t = al.CONFIGS[name]
    distinct, early, early_edge = al.check_populated(ref["counts"], spp, W, H)
    print("%s: tiles by count %s; %.0f %% stop early, %d in the last tile row / column" % (name, al.histogram(ref["counts"]), 100 * early, early_edge))
    return distinct, early_edge


@pytest.mark.parametrize("name", sorted(al.CONFIGS))
def test_reference_equals_the_oracle_per_count_class(name):
    kind, (W, H), _B, spp, _m, _i, _t = al.CONFIGS[name]
    ref = al.reference(name)
    distinct, early_edge = _populated(name, ref)
    tc = al.tile_counts(ref["counts"])
    if name in HISTOGRAMS:
        assert {n: int((tc == n).sum()) for n in distinct} == HISTOGRAMS[name]
    else:
        assert len(distinct) == 13 and int((tc == spp).sum()) == 18 and tc.size == 54
    assert early_edge == EARLY_EDGE_TILES[name]
    o = oracle_lib.OracleScene(al.config_scene(kind), al.config_params(name))
    try:
        for n in distinct:
            sel = ref["counts"] == n
            want = o.render(0, n)
            assert np.array_equal(_bits(ref["acc"][sel]), _bits(want[sel])), n
    finally:
        o.close()


@pytest.mark.parametrize("name", sorted(al.CONFIGS))
def test_verdicts_equal_the_float64_restatement(name):
    """Per pixel and checkpoint: the fp32 host verdict against the float64 one, except where the error lies within 1e-3 relative of the
    threshold (at most 0.5 % of the pairs); and the counts are the ones the float64 verdicts give, for every tile whose verdicts never hang
    on such a pixel alone."""
    _kind, (W, H), _B, spp, m, i, thr = al.CONFIGS[name]
    ref = al.reference(name)
    _populated(name, ref)
    trace = ref["trace"]
    assert [c for c, _, _ in trace] == al.checkpoints(spp, m, i)
    tv = al.tile_view(ref["counts"], H, W)
    actual = al.tile_counts(ref["counts"]).astype(np.int64)
    pairs = excluded = 0
    predicted = np.full(actual.shape, spp, np.int64)
    decided = np.ones(actual.shape, bool)
    for c, mom, active in trace:
        assert np.array_equal(active, actual >= c)
        m1, m2 = mom[..., 1], mom[..., 2]
        err64 = al.np_error(m1, m2, c)
        far = ~(np.abs(err64 - thr) <= 1e-3 * thr)
        got = al.host_error(m1, m2, c) <= np.float32(thr)
        want = al.np_converged(m1, m2, c, thr)
        pix_active = np.kron(active, np.ones((8, 8), bool))[:H, :W]
        pairs += int(pix_active.sum())
        excluded += int((pix_active & ~far).sum())
        assert np.array_equal(got[pix_active & far], want[pix_active & far]), c
        for (ty, tx), a in np.ndenumerate(active):
            s = tv[ty][tx]
            if not a or predicted[ty, tx] != spp or not decided[ty, tx] or (far[s] & ~want[s]).any():
                continue                    # stopped before, or a pixel that is clearly open keeps the tile active
            if far[s].all():
                predicted[ty, tx] = c
            else:
                decided[ty, tx] = False     # only pixels too close to the threshold are open: float64 does not predict this tile
    print("%s: %d (pixel, checkpoint) pairs, %.3f %% within 1e-3 of the threshold" % (name, pairs, 100.0 * excluded / pairs))
    assert excluded <= 0.005 * pairs, (excluded, pairs)
    print("%s: float64 predicts %d of %d tiles" % (name, int(decided.sum()), decided.size))
    assert set(actual[decided].tolist()) == set(actual.ravel().tolist())     # every count class takes part
    assert np.array_equal(predicted[decided], actual[decided])


def test_no_checkpoint_below_spp_gives_the_uniform_render():
    kind, (W, H), B, _spp, m, i, thr = al.CONFIGS["cornell67"]
    sc = al.config_scene(kind)
    for spp in (m - 2, m):
        p = make_params(W, H, spp, B)
        got = al.reference_render(sc, p, thr, m, i)
        want = dl.HostScene(sc, p).render(0, spp)
        assert (got[0] == spp).all()
        for g, w in zip(got[1:], want):
            assert np.array_equal(_bits(g), _bits(w)), spp


def test_stop_at_a_checkpoint_and_one_sample_after_it():
    kind, (W, H), B, spp, m, i, thr = al.CONFIGS["cornell67"]
    sc, p = al.config_scene(kind), al.config_params("cornell67")
    full = al.reference("cornell67")
    cps = al.checkpoints(spp, m, i)
    c = cps[2]
    at = al.reference_render(sc, p, thr, m, i, stop_at=c)
    after = al.reference_render(sc, p, thr, m, i, stop_at=c + 1)
    uniform = {n: dl.HostScene(sc, p).render(0, n) for n in (c, c + 1)}
    assert set(np.unique(at[0]).tolist()) == set(cps[:3]) and set(np.unique(after[0]).tolist()) == set(cps[:3]) | {c + 1}
    # tiles that stopped up to the checkpoint hold what the whole render leaves in them; the others the uniform render of stop_at samples
    for got, n in ((at, c), (after, c + 1)):
        stopped = full["counts"] <= c
        assert stopped.any() and not stopped.all()
        assert np.array_equal(got[0][stopped], full["counts"][stopped]) and (got[0][~stopped] == n).all()
        for k, key in enumerate(("acc", "albedo", "normal", "moments")):
            assert np.array_equal(_bits(got[1 + k][stopped]), _bits(full[key][stopped])), (n, key)
            assert np.array_equal(_bits(got[1 + k][~stopped]), _bits(uniform[n][k][~stopped])), (n, key)
    # stop_at = spp (and beyond) is the whole render
    whole = al.reference_render(sc, p, thr, m, i, stop_at=spp + 5)
    assert np.array_equal(whole[0], full["counts"]) and np.array_equal(_bits(whole[1]), _bits(full["acc"]))
