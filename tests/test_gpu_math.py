"""GPU: pt_debug_math (include/ptamd.h, platinum_amd/csrc/math_probe.hip) runs the math layer on the device on its own.  The device must be
the same bits as the host build of the same headers and as the oracle's twin on every in-domain input of tests/math_lib.py's sets, the
denormal exp2 results and every Halton boundary included, and is held directly to the float64 references with the bounds measured on the
oracle.  One launch per function."""
import ctypes as C

import numpy as np
import pytest

import math_lib as M
from platinum_amd import abi

pytestmark = pytest.mark.gpu
F32, U32, F64 = np.float32, np.uint32, np.float64
f = lambda w: w.view(F32)


@pytest.fixture(scope="module")
def r(gpu_renderer):
    return gpu_renderer


def three(r, fn, a, b=None):
    """device words, after asserting device == host build == oracle"""
    d, h, o = r.debugMath(fn, a, b), M.host(fn, a, b), M.oracle(fn, a, b)
    assert M.same_bits(d, h), "device / host build: " + M.first_difference(d, h, a, b)
    assert M.same_bits(d, o), "device / oracle: " + M.first_difference(d, o, a, b)
    return d


@pytest.mark.parametrize("name", list(M.ACCURACY_CASES))
def test_device_equals_host_build_and_oracle_and_meets_the_float64_bounds(r, name):
    c = M.ACCURACY_CASES[name]()
    d = three(r, c.fn, c.a, c.b)
    e = M.check_accuracy(name, d)
    print(name, {k: "%.3g (bound %.3g)" % (v, M.BOUNDS[(name, k)][1]) for k, v in e.items()})


def test_device_cos_is_the_cosine_of_sincos(r):
    c = M.sincos_case()
    a = c.a[c.classes["call"]]
    assert np.array_equal(three(r, abi.PT_MATH_COS, a)[0], r.debugMath(abi.PT_MATH_SINCOS, a)[1])


def test_device_exp2_gives_denormals_and_exact_powers(r):
    """[-126.5, -126): the kernels are built without fp32 denormal flushing; integers give exactly 2^k, powers of two exactly k"""
    c = M.exp2_case()
    v = f(r.debugMath(c.fn, c.a)[0])
    den = v[c.classes["denormal"]]
    assert np.all(den > 0) and np.all(den < M.MIN_NORMAL)
    k = np.arange(-126, 128)
    assert np.array_equal(v[c.classes["ints"]], np.exp2(k.astype(F64)).astype(F32))
    c = M.log2_case()
    assert np.array_equal(f(r.debugMath(c.fn, c.a[c.classes["pow2"]])[0]), k.astype(F32))


def test_device_halton_equals_host_build_oracle_and_the_numpy_restatement(r):
    c = M.halton_case()
    d = three(r, c.fn, c.a, c.b)
    want = M.halton_reference(c.a, c.b)
    assert np.array_equal(f(d[0]), want), M.first_difference(d, (want.view(U32), None), c.a, c.b)
    assert np.all(f(d[0]) >= 0) and np.all(f(d[0]) < 1)


def test_device_halton_offset(r):
    c = M.halton_offset_case()
    d = three(r, c.fn, c.a, c.b)
    assert np.array_equal(d[0][c.classes["kat"]], c.kat_want)


@pytest.mark.parametrize("k", range(len(M.guard_sets())), ids=[g[0] for g in M.guard_sets()])
def test_device_guards_and_special_values(r, k):
    name, fn, a, b = M.guard_sets()[k]
    v = f(three(r, fn, a, b)[0])
    if name == "pp_exp2":
        assert np.all(v[a >= 128] == np.inf) and np.all(v[a < -127] == 0) and not np.any(np.signbit(v))
    elif name == "pp_exp2s":
        assert np.all(v[a > 125] == np.inf) and np.all(v[a < -125] == 0)
    elif name == "dn_exp2":
        assert np.all(v[~(a > F32(-125))] == F32(2.0 ** -125))
    elif name == "pp_log2":
        assert np.all(v[~(a > 0)] == -np.inf)
    elif name == "pp_powr":
        p = b.astype(F64) * np.log2(np.where(a > 0, a, 1).astype(F64))
        assert np.all(v[(a > 0) & (p >= 128)] == np.inf) and np.all(v[(a > 0) & (p < -127)] == 0) and np.all(v[~(a > 0)] == 0)
    elif name == "dn_powr":
        assert np.all(v[~(a > 0)] == 0) and np.all(v[a > 0] >= F32(2.0 ** -125))
        assert np.all(v[-9:] < F32(2.0 ** 24))      # a base rounded above 1 at the largest sigma_n the host passes on
    else:   # the thin-lens radius: finite and inside the unit disk, or 0
        assert np.all(np.isfinite(v)) and np.all(v >= 0) and np.all(v <= 1) and np.all(v[a == 0] == 0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1 << 22])
def test_probe_sizes_at_the_wave_and_grid_edges(r, n):
    """one lane, a wave less one, a wave, a wave and one, and more elements than the grid has lanes (the grid-stride loop)"""
    c = M.sincos_case()
    a = np.resize(c.a[c.classes["call"]], n)
    d = r.debugMath(abi.PT_MATH_SINCOS, a)
    assert M.same_bits(d, M.host(abi.PT_MATH_SINCOS, a))
    c = M.warp_case(abi.PT_MATH_SAMPLE_COSINE_HEMISPHERE)      # the function with 2n words in out1
    ua, ub = np.resize(c.a, n), np.resize(c.b, n)
    d = r.debugMath(c.fn, ua, ub)
    assert d[1].size == 2 * n and M.same_bits(d, M.host(c.fn, ua, ub))


def test_debug_math_refusals(r):
    lib = abi.load_library()
    a = np.zeros(4, F32); o = np.zeros(8, U32)
    pa, po = a.ctypes.data, o.ctypes.data
    bad = lambda *args: lib.pt_debug_math(*args) == -1
    assert bad(r._h, abi.PT_MATH_COUNT, 4, pa, pa, po, po) and b"unknown function" in lib.pt_last_error()
    assert bad(r._h, 0xffffffff, 4, pa, pa, po, po)
    assert bad(r._h, abi.PT_MATH_COS, 0, pa, pa, po, po) and b"2^24" in lib.pt_last_error()
    assert bad(r._h, abi.PT_MATH_COS, (1 << 24) + 1, pa, pa, po, po)
    assert bad(r._h, abi.PT_MATH_COS, 4, None, pa, po, po) and b"null argument" in lib.pt_last_error()
    assert bad(r._h, abi.PT_MATH_COS, 4, pa, pa, None, po)
    assert bad(r._h, abi.PT_MATH_ATAN2, 4, pa, None, po, po)
    assert bad(r._h, abi.PT_MATH_SINCOS, 4, pa, pa, po, None)
    assert bad(None, abi.PT_MATH_COS, 4, pa, pa, po, po) and b"null renderer" in lib.pt_last_error()
    # a function of one argument and one result needs neither b nor out1
    assert lib.pt_debug_math(r._h, abi.PT_MATH_COS, 4, pa, None, po, None) == 0 and np.all(f(o[:4]) == 1.0)


@pytest.mark.parametrize("bokeh_power", [6.0, 200.0])
def test_device_thin_lens_render_outside_the_ui_range_equals_the_oracle(r, bokeh_power):
    """k_raygen with the guarded thin-lens power and a blade count of 0 (counts as 3): the accumulator is the oracle's, bit for bit, and finite"""
    import oracle_lib
    from platinum_amd import scenes
    from platinum_amd.renderer import make_params
    sc = scenes.cornell_sphere_scene(transmission=0.0)
    sc.camera.aperture = 2.8; sc.camera.focus_distance = 12.0; sc.camera.roundness = 0.3; sc.camera.bokeh_power = bokeh_power
    sc.camera.aperture_blades = 0
    w, h, spp, bounces = 48, 27, 2, 3
    r.startRender(sc, (w, h), spp, max_bounces=bounces)
    r.render(0)
    acc = r.readbackAccumulator()
    want = oracle_lib.OracleScene(sc, make_params(w, h, spp, bounces)).render(0, spp)
    assert np.all(np.isfinite(want)) and acc.tobytes() == want.tobytes()


def test_device_denoiser_with_the_largest_sigma_normal_is_the_capped_one(r):
    """pt_denoise_options.sigma_normal may be any finite float; the host passes min(sigma_normal, 2^24) on, which keeps dn_powr's exponent
    inside exp2_det's domain where a dot product of unit normals rounds above 1: the filtered image is finite and the bits of 2^24's"""
    from platinum_amd import scenes
    keep = r.denoiseOptions()
    try:
        r.setDenoiseOptions(enabled=1)
        r.startRender(scenes.cornell_scene("bench"), (64, 48), 4, max_bounces=3)
        r.render(0)
        r.wait()
        r.setDenoiseOptions(sigma_normal=float(np.finfo(F32).max))
        big = r.readbackDenoised()
        r.setDenoiseOptions(sigma_normal=2.0 ** 24)
        capped = r.readbackDenoised()
        r.setDenoiseOptions(sigma_normal=128.0)
        assert np.all(np.isfinite(big)) and big.tobytes() == capped.tobytes() and big.tobytes() != r.readbackDenoised().tobytes()
    finally:
        r.setDenoiseOptions(keep)
