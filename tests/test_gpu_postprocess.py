"""GPU: k_postprocess and k_gmon against independent references (tests/post_ref.py, post_lib.gmon_resolve), not only against the oracle.

The device renders its own test card (post_lib.card_scene: emissive patches, 1 spp, one bounce) at six sizes; the accumulator read back
is the common input of device, oracle and float64 reference.  Each option set of the sweep of tests/test_postprocess_reference.py is then
applied with setPostProcessOptions / setTonemapOptions + readbackRenderTarget, which re-runs k_postprocess only."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import post_lib as pl
import post_ref
from platinum_amd import abi, scenes
from platinum_amd.renderer import make_params
from test_postprocess_reference import compare, same_bits_or_both_nan

pytestmark = pytest.mark.gpu

WORKING_SPACE = pl.GPU_WORKING_SPACE
WORKING = scenes.colorspace(WORKING_SPACE)
SIZE_IDS = ["%dx%d" % s for s in pl.GPU_SIZES]
TM_IDS = [pl.TONEMAPPER_NAMES[t] for t in pl.TONEMAPPERS]


@pytest.fixture
def r(gpu_renderer):
    gpu_renderer.selectKernel(abi.INTEGRATOR_MIS)
    yield gpu_renderer
    gpu_renderer.setPostProcessOptions(gpu_renderer.postProcessOptions())
    gpu_renderer.setTonemapOptions(gpu_renderer.tonemapOptions())
    gpu_renderer.setGmonOptions(cap=1.0)
    gpu_renderer.selectKernel(abi.INTEGRATOR_MIS)


_cards = {}


def rendered_card(r, size):
    """(accumulator read back from the device, oracle handle) of the card at `size`; the device is left holding that render."""
    w, h = size
    sc = pl.card_scene(w, h)
    r.startRender(sc, size, 1, workingSpace=WORKING_SPACE, max_bounces=1)
    r.render(0)
    r.wait()
    acc = r.readbackAccumulator()
    if size not in _cards:
        o = oracle_lib.OracleScene(sc, make_params(w, h, 1, 1, working_space=WORKING_SPACE))
        want = o.render(0, 1)
        if w * h >= 240:                 # every regime of the host cards, in the oracle's render, before the device's is trusted with it
            found = pl.regimes(want[..., :3], zero=1e-12)
            assert all(found[k] > 0 for k in found) and found["stops"] >= pl.STOPS, found
            po, to = pl.defaults()
            display, _ = post_ref.postprocess(want, po, to, WORKING)
            near, informative = pl.card_statistics(display, pl.bound(to.tonemapper))
            assert near <= 0.10 and informative >= 0.5, (near, informative)
        _cards[size] = (o, want)
    o, want = _cards[size]
    assert np.array_equal(acc.view(np.uint32), want.view(np.uint32))
    return acc, o


@pytest.mark.parametrize("tm", pl.TONEMAPPERS, ids=TM_IDS)
@pytest.mark.parametrize("size", pl.GPU_SIZES, ids=SIZE_IDS)
def test_device_bytes_equal_the_oracle_and_follow_the_reference_over_the_sweep(r, size, tm):
    acc, o = rendered_card(r, size)
    unequal, failures = [], []
    for cfg in pl.sweep(tm):
        po, to = cfg.structs()
        r.setPostProcessOptions(po)
        r.setTonemapOptions(to)
        got = r.readbackRenderTarget()
        if not np.array_equal(got, o.postprocess(acc, po, to)):                   # (a) the oracle's bytes, exactly
            unequal.append(cfg.name)
        if cfg.name not in pl.EXCUSED:                                            # (b) the float64 reference's, under the RGBA8 rule
            _f, bad = compare(cfg, acc, got, working=WORKING)
            if bad:
                failures.append((cfg.name, bad))
    assert not unequal, "device != oracle: %s" % unequal[:12]
    assert not failures, "%d configurations break the RGBA8 rule (name, channels): %s" % (len(failures), failures[:12])


def test_presented_bytes_are_the_read_back_ones(r):
    """(c) presentRenderTarget at 96x64 under non-default options of every pass."""
    size = (96, 64)
    rendered_card(r, size)
    hip = abi.load_library()
    for tm in pl.TONEMAPPERS:
        for cfg in pl.random_configs(tm, 2):
            po, to = cfg.structs()
            r.setPostProcessOptions(po)
            r.setTonemapOptions(to)
            ptr, stream = r.presentRenderTarget()
            assert ptr and stream
            want = r.readbackRenderTarget()                                        # (synchronises the renderer's stream)
            got = np.empty((size[1], size[0], 4), np.uint8)
            assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), C.c_void_p(ptr), C.c_size_t(got.nbytes), 2) == 0    # hipMemcpyDeviceToHost
            assert np.array_equal(got, want), cfg.name


@pytest.mark.parametrize("tm", pl.TONEMAPPERS, ids=TM_IDS)
def test_overflow_on_the_device_is_white(r, tm):
    """exposure = 120 makes every channel above 256 +inf in the exposure pass, and leaves black at 0 * 2^120 = 0.  A patch whose three
    channels overflow is white (flim: its white cap); every other pixel has the reference's bytes."""
    size = (96, 64)
    acc, o = rendered_card(r, size)
    po, to = pl.defaults()
    po.exposure, to.tonemapper = 120.0, tm
    r.setPostProcessOptions(po)
    r.setTonemapOptions(to)
    got = r.readbackRenderTarget()
    assert np.array_equal(got, o.postprocess(acc, po, to))
    display, want = post_ref.postprocess(acc, po, to, WORKING)
    with np.errstate(over="ignore"):
        overflowed = np.isinf(acc[..., :3] * np.float32(2.0 ** 120)).all(axis=-1)
    assert overflowed.sum() >= 20 and (acc[..., :3] == 0).all(axis=-1).sum() >= 20
    if tm == abi.TONEMAP_FLIM:
        chain = post_ref._Chain(np.float64)
        cap = chain.grade_and_encode(post_ref.flim_white_cap(to)[None, None, :], post_ref.options(to), post_ref.options(WORKING))
        white = post_ref.quantise(cap)[0, 0]
    else:
        white = np.array([255, 255, 255, 255], np.uint8)
    assert (got[overflowed] == white).all(), got[overflowed][:4].tolist()
    assert (got[(acc[..., :3] == 0).all(axis=-1)][:, :3] <= 1).all()
    assert not pl.rgba8_violations(got, display, pl.bound(tm)).any()


# ---- the GMoN resolve ----------------------------------------------------------------------------------------------------------------------
GMON_SIZE = (33, 17)
GMON_PAIRS = [(1, 1), (2, 2), (32, 32), (33, 32), (5, 8), (31, 3)]     # (spp, buckets); (5, 8): fewer full buckets than allocated; (31, 3): ragged last bucket


@pytest.mark.parametrize("spp,buckets", GMON_PAIRS)
def test_gmon_resolve_on_the_device_equals_the_numpy_restatement(r, spp, buckets):
    sc = scenes.cornell_sphere_scene()
    flags = abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON
    spb = (spp + buckets - 1) // buckets
    full = (spp - 1) // spb + 1
    for cap in (1.0, 0.25, 0.0):
        r.setGmonOptions(cap=cap)
        r.startRender(sc, GMON_SIZE, spp, gmonBuckets=buckets, flags=flags, max_bounces=4, samples_in_flight=3)
        r.render(0)
        r.wait()
        stack = np.stack([r.readGmonBucket(b) for b in range(full)])
        got = r.readbackAccumulator()
        want = pl.gmon_resolve(stack, cap)
        assert same_bits_or_both_nan(got, want).all(), (spp, buckets, cap)
        assert np.isfinite(got).mean() > 0.5          # (not a comparison of NaN with NaN: at two buckets a pixel black in both is 0 / 0)


def test_gmon_cap_outside_0_1_is_refused(r):
    for cap in (-1e-6, 1.000001, float("inf"), float("nan"), 1e30):
        with pytest.raises(abi.PtamdError, match="error -1: .*cap"):
            r.setGmonOptions(cap=cap)
    for cap in (0.0, 1.0):
        r.setGmonOptions(cap=cap)
