"""CPU: the oracle's post-process chain and GMoN resolve against independent references.

The oracle's chain (oracle/post_oracle.inc) is the product's (pt_post.h) under other names, so "device bytes == oracle bytes" proves that
two compilers agree, not that the chain is the right one.  Here the oracle is held against tests/post_ref.py, a float64 numpy restatement
written from the chain's formulas, over synthetic test cards and the whole option sweep of post_lib: every field at both ends of its range,
64 random combinations per tonemapper, three output spaces, landscape / portrait / square / one-pixel-wide cards.

The bound is measured, not chosen: post_ref's own code run in float32 against itself in float64 (post_lib.PRECISION, ILL, UNSTABLE), times 4.
"""
import numpy as np
import pytest

import oracle_lib
import post_lib as pl
import post_ref
from platinum_amd import abi, scenes
from platinum_amd.renderer import make_params

WORKING = scenes.colorspace(scenes.BT2020)
CARD_IDS = ["%dx%d" % s for s in pl.CARD_SIZES]
TM_IDS = [pl.TONEMAPPER_NAMES[t] for t in pl.TONEMAPPERS]


@pytest.fixture(scope="module")
def cards():
    return {s: pl.card(*s) for s in pl.CARD_SIZES}


@pytest.fixture(scope="module")
def oracles():
    """One oracle handle per card size (the scene is irrelevant to orc_postprocess: it reads the size and the working space)."""
    out = {s: oracle_lib.OracleScene(scenes.cornell_scene(), make_params(s[0], s[1], 1, 1)) for s in pl.CARD_SIZES}
    yield out
    for o in out.values():
        o.close()


# ---- the cards ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", pl.CARD_SIZES, ids=CARD_IDS)
def test_card_contains_every_regime_and_is_informative(cards, size):
    acc = cards[size]
    assert acc.shape == (size[1], size[0], 4) and np.isfinite(acc).all() and (acc[..., :3] >= 0).all()
    if size[0] * size[1] >= 37:
        found = pl.regimes(acc[..., :3])
        print(size, found)
        assert all(found[k] > 0 for k in found), found
        assert found["stops"] >= pl.STOPS
    # on the reference alone, under the default options: few channel values next to a rounding boundary, most of them off the rails
    po, to = pl.defaults()
    display, _ = post_ref.postprocess(acc, po, to, WORKING)
    near, informative = pl.card_statistics(display, pl.bound(to.tonemapper))
    print(size, "excusable %.3f, in 1..254 %.3f" % (near, informative))
    assert near <= 0.10 and informative >= 0.5


def test_output_transform_from_chromaticities():
    """The reference's own ODT: identity for the working space, white stays white, and the textbook BT.2020 -> BT.709 matrix."""
    spaces = {k: post_ref.options(scenes.colorspace(v)) for k, v in pl.OUTPUT_SPACES.items()}
    np.testing.assert_allclose(post_ref.output_transform(spaces["bt2020"], spaces["bt2020"]), np.eye(3), atol=1e-12)
    for name in ("display_p3", "bt709"):
        np.testing.assert_allclose(post_ref.output_transform(spaces["bt2020"], spaces[name]) @ np.ones(3), np.ones(3), atol=1e-9)
    # ITU-R BT.2087 annex: BT.2020 to BT.709 (float32 chromaticities in the struct: 1e-4)
    bt2087 = [[1.6605, -0.5876, -0.0728], [-0.1246, 1.1329, -0.0083], [-0.0182, -0.1006, 1.1187]]
    np.testing.assert_allclose(post_ref.output_transform(spaces["bt2020"], spaces["bt709"]), bt2087, atol=2e-4)


# ---- the sweep -------------------------------------------------------------------------------------------------------------------------
def compare(cfg, acc, got_bytes, got_float=None, working=WORKING):
    """The violations of `cfg` on `acc`: (float channels out of tolerance or NaN on one side only, bytes that break the RGBA8 rule)."""
    po, to = cfg.structs()
    display, _ = post_ref.postprocess(acc, po, to, working)
    tol = pl.tolerance(cfg, acc, display, working)
    bad_float = 0
    if got_float is not None:
        want, got = pl.clipped(display), pl.clipped(got_float)
        with np.errstate(invalid="ignore"):
            wrong = (np.abs(want - got) > tol) | (np.isnan(want) != np.isnan(got))
        bad_float = int((wrong & np.isfinite(tol)).sum())
    return bad_float, int(pl.rgba8_violations(got_bytes, display, tol).sum())


@pytest.mark.parametrize("tm", pl.TONEMAPPERS, ids=TM_IDS)
@pytest.mark.parametrize("size", pl.CARD_SIZES, ids=CARD_IDS)
def test_oracle_matches_the_float64_reference_over_the_sweep(cards, oracles, size, tm):
    acc, o = cards[size], oracles[size]
    failures = []
    for cfg in pl.sweep(tm):
        if cfg.name in pl.EXCUSED:
            continue
        po, to = cfg.structs()
        got_bytes, got_float = o.postprocess(acc, po, to, want_float=True)
        bad_float, bad_bytes = compare(cfg, acc, got_bytes, got_float)
        if bad_float or bad_bytes:
            failures.append((cfg.name, bad_float, bad_bytes))
    assert not failures, "%d configurations (name, float channels, byte channels): %s" % (len(failures), failures[:12])


@pytest.mark.parametrize("tm", pl.TONEMAPPERS, ids=TM_IDS)
def test_precision_tables_are_what_the_reference_measures(tm):
    """PRECISION, UNSTABLE: post_ref in float32 against post_ref in float64, nothing else."""
    own = pl.measure_precision(tm)
    unstable = {n for n, v in own.items() if v > pl.ILL}
    tn = pl.TONEMAPPER_NAMES[tm]
    assert unstable == {n for n in pl.UNSTABLE if n.startswith(tn + "/")}
    assert set(pl.EXCUSED) <= set(pl.UNSTABLE)
    measured = max(v for n, v in own.items() if n not in unstable)
    print(tn, "measured %.4g, table %.4g, bound %.4g" % (measured, pl.PRECISION[tm], pl.bound(tm)))
    assert measured == pytest.approx(pl.PRECISION[tm], rel=5e-3)


# ---- overflow: an overbright pixel is white ---------------------------------------------------------------------------------------------
OVERBRIGHT = (1e7, 1e20, 1e30, 1e36, 3e38, np.inf)


@pytest.mark.parametrize("tm", pl.TONEMAPPERS, ids=TM_IDS)
def test_overbright_pixels_are_white_or_flims_white_cap(tm):
    """exp2 / powr past the float range give +inf, not the -0 of (n + 127) << 23 run into the sign bit, and what the contrast pass hands on
    is capped (pt_post.h kPostCeiling) so that no inf - inf follows: pixels of 1e7 .. 3e38 and inf are white under no tonemapper, AgX and
    Khronos, and flim's white cap under flim, for contrast 0 / 12 / 50 / 100 and midtone offset 0 / 8, in the oracle and in the reference.
    Before the guard a pixel of inf or 3e38 was black, 1e36 from contrast 12 on, 1e30 from contrast 50 on."""
    n = len(OVERBRIGHT)
    acc = np.ones((1, n + 1, 4), np.float32)
    acc[0, :n, :3] = np.array(OVERBRIGHT, np.float32)[:, None]
    acc[0, n, :3] = 0.18                                                       # a mid-grey pixel, so that the image is not all white
    o = oracle_lib.OracleScene(scenes.cornell_scene(), make_params(n + 1, 1, 1, 1))
    for contrast in (0.0, 12.0, 50.0, 100.0):
        for midtone in (0.0, 8.0):
            po, to = pl.defaults()
            po.contrast, to.tonemapper, to.midtone_offset = contrast, tm, midtone
            got = o.postprocess(acc, po, to)
            _display, want = post_ref.postprocess(acc, po, to, WORKING)
            if tm == abi.TONEMAP_FLIM:
                chain = post_ref._Chain(np.float64)
                cap = chain.grade_and_encode(post_ref.flim_white_cap(to)[None, None, :], post_ref.options(to), post_ref.options(WORKING))
                white = post_ref.quantise(cap)[0, 0]
                assert white[:3].min() >= 250                                  # (flim's cap is white to within its print density)
            else:
                white = np.array([255, 255, 255, 255], np.uint8)
            what = "contrast %g midtone %g" % (contrast, midtone)
            assert (want[0, :n] == white).all(), (what, want[0, :n].tolist())
            assert (got[0, :n] == white).all(), (what, got[0, :n].tolist())
            assert 0 < got[0, n, 0] < 255 and abs(int(got[0, n, 0]) - int(want[0, n, 0])) <= 1, what
    o.close()


def test_negative_and_minus_inf_pixels_are_what_the_reference_says():
    """log2 of a value <= 0 is -inf, so a negative or -inf channel leaves the contrast pass as exp2(-inf) - eps < 0, clamped to 0: such a
    pixel is displayed like a black one, in the reference and in the oracle, under every tonemapper."""
    acc = np.ones((1, 4, 4), np.float32)
    acc[0, :, :3] = np.array([-np.inf, -1.0, -1e-3, 0.0], np.float32)[:, None]
    o = oracle_lib.OracleScene(scenes.cornell_scene(), make_params(4, 1, 1, 1))
    for tm in pl.TONEMAPPERS:
        po, to = pl.defaults()
        to.tonemapper = tm
        got = o.postprocess(acc, po, to)
        _display, want = post_ref.postprocess(acc, po, to, WORKING)
        assert (want[0, :3] == want[0, 3]).all() and want[0, 3, :3].max() <= 1, (tm, want.tolist())
        assert np.array_equal(got, want), (tm, got.tolist(), want.tolist())
    o.close()


# ---- the GMoN resolve ----------------------------------------------------------------------------------------------------------------------
GMON_W, GMON_H = 12, 5
GMON_CAPS = (0.0, 0.25, 1.0, 1e-30, float(np.nextafter(np.float32(1), np.float32(0))))


def gmon_stack(n, kind):
    """Bucket means [n, H, W, 4] of one kind; the first row is all black (G = 0 / 0)."""
    rng = np.random.default_rng(n * 10 + len(kind))
    colour = rng.uniform(0.05, 2.0, size=(GMON_H, GMON_W, 3))
    if kind == "equal":
        b = np.broadcast_to(colour, (n,) + colour.shape).copy()
    elif kind == "increasing":
        b = colour[None] * (1.0 + np.arange(n))[:, None, None, None]
    elif kind == "decreasing":
        b = colour[None] * (1.0 + np.arange(n))[::-1, None, None, None]
    elif kind == "outlier":
        b = colour[None] * rng.uniform(0.9, 1.1, size=(n, GMON_H, GMON_W, 1))
        b[n // 2] *= 1000.0
    elif kind == "ties":       # equal lumas, different colours: only a stable sort keeps their order
        b = np.broadcast_to(colour, (n,) + colour.shape).copy()
        b[1::2, ..., 0] += 0.7152
        b[1::2, ..., 1] -= 0.2126
    else:
        b = rng.uniform(0.0, 1.0, size=(n, GMON_H, GMON_W, 3)) ** 4 * 8.0
    out = np.ones((n, GMON_H, GMON_W, 4), np.float32)
    out[..., :3] = b
    out[:, 0, :, :3] = 0.0
    return out


def same_bits_or_both_nan(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("n", [1, 2, 3, 8, 31, 32])
def test_gmon_resolve_equals_the_numpy_restatement_and_the_definition(n):
    flags = abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON
    o = oracle_lib.OracleScene(scenes.cornell_scene(), make_params(GMON_W, GMON_H, n, 1, flags=flags, gmon_buckets=n))
    for kind in ("equal", "increasing", "decreasing", "outlier", "ties", "random"):
        stack = gmon_stack(n, kind)
        for cap in GMON_CAPS:
            what = "%s n %d cap %g" % (kind, n, cap)
            got = o.gmon_resolve(stack, n, cap=cap)
            want = pl.gmon_resolve(stack, cap)
            assert same_bits_or_both_nan(got, want).all(), what
            # the right quantities: the Gini coefficient from its definition and the trimmed mean, in float64.  The distance of the same
            # code in float32 from itself in float64 is what single precision costs; 4 x that (at least 4 ulp of the largest mean) is
            # allowed, on the pixels whose trim count is the same in both runs (G * (n / 2) at an integer is a coin toss).
            G, mean, c, cf = pl.gmon_quantities(stack, cap)
            _G32, mean32, c32, _cf32 = pl.gmon_quantities(stack, cap, dtype=np.float32)
            lit = np.isfinite(mean).all(axis=-1) & np.isfinite(got[..., :3]).all(axis=-1)
            settled = lit & (c == c32)
            assert settled[1:].mean() >= 0.9, what
            cost = np.abs(mean32.astype(np.float64) - mean)[settled].max(initial=0.0)
            tol = 4.0 * max(cost, float(np.spacing(np.float32(stack.max()))))
            assert np.abs(got[..., :3] - mean)[settled].max(initial=0.0) <= tol, what
            if kind == "equal":
                assert (G[1:] < 1e-12).all() and (c[1:] == 0).all() and np.allclose(got[1:], stack[0, 1:], rtol=n * 6e-8, atol=0), what
            if kind == "outlier" and n >= 8 and cap >= 0.25:
                assert (c[1:] >= 1).all() and (got[1:, :, :3] < stack[n // 2, 1:, :, :3] / 100).all(), what     # the outlier is trimmed
            if kind == "ties":
                assert np.allclose(G[1:], 0, atol=1e-7)
            # an all-black pixel: G = 0 / 0, min(NaN, cap) = cap, so c = int(cap * (n / 2)) buckets go from either end; 0 / 0 when none is left
            black = got[0, :, :3]
            assert (np.isnan(black).all() if n - 2 * int(np.float32(cap) * np.float32(n // 2)) == 0 else (black == 0).all()), what
    o.close()
