"""CPU: the math layer (pt_math.h, pt_sampler.h, the guards of pt_post.h / pt_denoise.h) against independent float64 references
(tests/math_lib.py).  The oracle's twin (oracle/oracle_math.h) and the host build of the product's headers must be the same bits on every
in-domain input; the accuracy is measured on the oracle, which the product is bound to by that equality; the bounds are math_lib.BOUNDS
(DESIGN.md section 2).  tests/test_gpu_math.py holds the device to the same sets."""
import os
import subprocess

import numpy as np
import pytest

import math_lib as M
from platinum_amd import abi

F32, U32, F64 = np.float32, np.uint32, np.float64
f = lambda w: w.view(F32)


@pytest.fixture(scope="module")
def results():
    """{case: (oracle words, host words)}, computed once"""
    out = {}
    for name, make in M.ACCURACY_CASES.items():
        c = make()
        out[name] = (M.oracle(c.fn, c.a, c.b), M.host(c.fn, c.a, c.b))
    return out


# ---- same bits ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(M.ACCURACY_CASES))
def test_oracle_twin_equals_the_host_build(results, name):
    c = M.ACCURACY_CASES[name]()
    o, h = results[name]
    assert M.same_bits(o, h), M.first_difference(o, h, c.a, c.b)


def test_cos_is_the_cosine_of_sincos(results):
    c = M.sincos_case()
    o, h = M.oracle(abi.PT_MATH_COS, c.a), M.host(abi.PT_MATH_COS, c.a)
    assert np.array_equal(o[0], h[0]) and np.array_equal(o[0], results["sincos"][0][1])


# ---- accuracy against float64, measured on the oracle's implementation -------------------------------------------------------------------

@pytest.mark.parametrize("name", list(M.ACCURACY_CASES))
def test_accuracy_against_float64(results, name):
    e = M.check_accuracy(name, results[name][0])
    print(name, {k: "%.3g (measured %.3g, bound %.3g)" % ((v,) + M.BOUNDS[(name, k)]) for k, v in e.items()})


def test_bounds_stay_inside_what_the_suite_asserted_before():
    """test_oracle_kat.py::test_deterministic_transcendentals_accuracy: 3e-7 absolute for sincos on [0, 2 pi], 3e-6 for log2 and exp2"""
    assert M.BOUNDS[("sincos", "call")][1] <= 3e-7
    assert all(M.BOUNDS[("log2", k)][1] <= 3e-6 for k in ("pow2", "near1", "all"))
    assert all(M.BOUNDS[("exp2", k)][1] <= 3e-6 for k in ("ints", "normal", "denormal"))


# ---- exact properties --------------------------------------------------------------------------------------------------------------------

def test_log2_of_a_power_of_two_and_exp2_of_an_integer_are_exact(results):
    c = M.log2_case()
    k = np.arange(-126, 128)
    assert np.array_equal(f(results["log2"][0][0])[c.classes["pow2"]], k.astype(F32))
    c = M.exp2_case()
    assert np.array_equal(f(results["exp2"][0][0])[c.classes["ints"]], np.exp2(k.astype(F64)).astype(F32))


def test_exp2_reaches_the_denormals(results):
    """[-126.5, -126) gives denormal results, not zeros: the fp32 contract has no flush to zero"""
    c = M.exp2_case()
    v = f(results["exp2"][0][0])[c.classes["denormal"]]
    assert v.size > 1000 and np.all(v > 0) and np.all(v < M.MIN_NORMAL)


def test_sincos_symmetry_on_the_bits():
    c = M.sincos_case()
    x = np.abs(c.a)
    p, n = M.oracle(abi.PT_MATH_SINCOS, x), M.oracle(abi.PT_MATH_SINCOS, -x)
    nz = f(p[0]) != 0          # sin is odd on the bits; a zero sine is +0 on both sides (r = x - k * DP1 ... gives -0 - -0 = +0)
    assert np.array_equal(f(p[0]), -f(n[0])) and np.array_equal((p[0] ^ U32(0x80000000))[nz], n[0][nz])
    assert np.array_equal(p[1], n[1])                                                               # cos is even


def test_warp_properties(results):
    c = M.warp_case(abi.PT_MATH_SAMPLE_DISK)
    n = c.a.size
    x, y = (f(w).astype(F64) for w in results["disk"][0])
    assert np.abs(np.hypot(x, y) - np.sqrt(c.a.astype(F64))).max() <= M.UNIT_LENGTH_BOUND
    o = results["cosine_hemisphere"][0]
    x, y, z = f(o[0]).astype(F64), f(o[1][:n]).astype(F64), f(o[1][n:]).astype(F64)
    assert np.abs(np.sqrt(x * x + y * y + z * z) - 1).max() <= M.UNIT_LENGTH_BOUND
    assert np.all(z > 0)
    b0, b1 = (f(w) for w in results["tri_uniform"][0])
    assert np.all(b0 >= 0) and np.all(b1 >= 0) and np.all(b0.astype(F64) + b1.astype(F64) <= 1.0)
    # the two sides of the diagonal are mirror images
    d = c.classes["diagonal"]
    m = M.oracle(abi.PT_MATH_SAMPLE_TRI_UNIFORM, c.b[d], c.a[d])
    assert np.array_equal(f(m[0]), b1[d]) and np.array_equal(f(m[1]), b0[d])


# ---- Halton ------------------------------------------------------------------------------------------------------------------------------

def test_halton_host_build_equals_oracle_equals_the_numpy_restatement():
    c = M.halton_case()
    o, h = M.oracle(c.fn, c.a, c.b), M.host(c.fn, c.a, c.b)
    want = M.halton_reference(c.a, c.b)
    assert np.array_equal(o[0], h[0]), M.first_difference(o, h, c.a, c.b)
    assert np.array_equal(f(o[0]), want), M.first_difference(o, (want.view(U32), None), c.a, c.b)
    v = f(o[0])
    assert np.all(v >= 0) and np.all(v < 1) and v[c.a == 0].max() == 0
    assert len(c.classes) == 3 and c.classes["boundaries"].stop - c.classes["boundaries"].start > 20 * 620


def test_halton_offset_equals_the_known_answers_and_the_oracle():
    c = M.halton_offset_case()
    o, h = M.oracle(c.fn, c.a, c.b), M.host(c.fn, c.a, c.b)
    assert np.array_equal(o[0], h[0])
    assert np.array_equal(h[0][c.classes["kat"]], c.kat_want)


# ---- the guards: DESIGN.md section 2's conventions at and around each cut-off -----------------------------------------------------------------

def both(fn, a, b=None):
    o, h = M.oracle(fn, a, b), M.host(fn, a, b)
    assert M.same_bits(o, h), M.first_difference(o, h, a, b)
    return f(h[0])


def expect_exp2_guard(x, v, zero_below, inf_from, inclusive_inf):
    """v = guard(x): +inf from the upper cut-off, 0 below the lower one, exp2 within 3e-7 relative between them (0 / inf where exp2_det's own
    2^n leaves the floats: n = -127, 128)"""
    x64 = x.astype(F64)
    hi = x64 >= inf_from if inclusive_inf else x64 > inf_from
    lo = x64 < zero_below
    assert np.all(v[hi] == np.inf) and np.all(v[lo] == 0) and not np.any(np.signbit(v))
    mid = ~hi & ~lo & (x64 >= -126.5) & (x64 < 127.5)
    assert np.all(np.abs(v[mid].astype(F64) - np.exp2(x64[mid])) <= 3e-7 * np.exp2(x64[mid]))
    assert np.all(v[~hi & ~lo & (x64 < -126.5)] == 0) and np.all(v[~hi & ~lo & (x64 >= 127.5)] == np.inf)


def test_pp_exp2_guard():
    x = M.guard_inputs([-127.0, 128.0, -126.5, 127.5], nan=False)
    expect_exp2_guard(x, both(abi.PT_MATH_PP_EXP2, x), -127.0, 128.0, True)


def test_pp_exp2s_guard():
    x = M.guard_inputs([-125.0, 125.0], nan=False)
    expect_exp2_guard(x, both(abi.PT_MATH_PP_EXP2S, x), -125.0, 125.0, False)


def test_dn_exp2_guard():
    """exponents not above -125 count as -125, a NaN too; no upper guard (a weight's exponent stays below 24: pt_denoise.h)"""
    x = M.guard_inputs([-125.0], nan=True)
    x = x[~(x >= F32(127.5))]
    v = both(abi.PT_MATH_DN_EXP2, x)
    low = ~(x > F32(-125.0))
    assert np.all(v[low] == F32(2.0 ** -125)) and np.isnan(x[low]).any()
    assert np.all(np.abs(v[~low].astype(F64) - np.exp2(x[~low].astype(F64))) <= 3e-7 * np.exp2(x[~low].astype(F64)))


def test_pp_log2_guard():
    """log2 of a value not > 0 is -inf (a NaN too); denormals are read as 2^-126 .. 2^-127 (log2_det ignores the missing leading bit)"""
    x = M._cat([M.ulps(F32(0.0), 4), M.SPECIALS, [M.NAN]])
    v = both(abi.PT_MATH_PP_LOG2, x)
    not_pos = ~(x > 0)
    assert np.all(v[not_pos] == -np.inf)
    den = (x > 0) & (x < M.MIN_NORMAL)
    assert den.sum() >= 5 and np.all((v[den] >= -127) & (v[den] <= -126))
    norm = (x >= M.MIN_NORMAL) & np.isfinite(x)
    assert np.all(np.abs(v[norm].astype(F64) - np.log2(x[norm].astype(F64))) <= 3e-7 * np.maximum(1, np.abs(np.log2(x[norm].astype(F64)))))
    assert v[x == np.inf][0] == 128.0      # the bits of +inf read as 2^128


PRODUCT_CUTS = M.PRODUCT_CUTS


@pytest.mark.parametrize("fn,exp2_fn", [(abi.PT_MATH_PP_POWR, abi.PT_MATH_PP_EXP2), (abi.PT_MATH_DN_POWR, abi.PT_MATH_DN_EXP2)])
def test_guarded_powers_at_the_products_that_cross_the_cut_offs(fn, exp2_fn):
    """x = 2 and x = 4 have exact logarithms: powr(2, y) is the guarded exp2 of y, powr(4, y / 2) as well, bit for bit"""
    y = M.ulps(F32(PRODUCT_CUTS), 4)
    if fn == abi.PT_MATH_DN_POWR:
        y = y[y < F32(127.5)]
    want = both(exp2_fn, y)
    assert np.array_equal(both(fn, np.full(y.size, 2.0, F32), y).view(U32), want.view(U32))
    assert np.array_equal(both(fn, np.full(y.size, 4.0, F32), y * F32(0.5)).view(U32), want.view(U32))
    if fn == abi.PT_MATH_PP_POWR:
        assert np.all(want[y >= 128] == np.inf) and np.all(want[y < -127] == 0)
    # powr(x <= 0, .) = 0
    x = F32([0.0, -0.0, -1.0, -np.inf, -1e-40])
    assert np.all(both(fn, x, np.full(x.size, 2.5, F32)) == 0)


def test_accuracy_cases_respect_the_conventions_past_the_float_range(results):
    c = M.pp_powr_case()
    v = f(results["pp_powr"][0][0])
    p = c.b.astype(F64) * np.log2(c.a.astype(F64))
    assert np.all(v[p > 128.001] == np.inf) and np.all(v[p < -127.001] == 0) and (p > 128.001).sum() > 1000 and (p < -127.001).sum() > 1000
    assert not np.any(np.isnan(v)) and not np.any(np.signbit(v))
    c = M.dn_powr_case()
    v = f(results["dn_powr"][0][0])
    with np.errstate(all="ignore"):
        p = np.where(c.a > 0, c.b.astype(F64) * np.log2(np.maximum(c.a, M.MIN_NORMAL).astype(F64)), 0.0)
    assert np.all(v[(c.a > 0) & (p < -125.001)] == F32(2.0 ** -125)) and np.all(v[c.a <= 0] == 0)
    assert np.all(np.isfinite(v)) and np.all(v <= 1)


# ---- the thin-lens power is total ---------------------------------------------------------------------------------------------------------

lens_inputs = M.lens_samples


@pytest.mark.parametrize("bokeh_power", M.BOKEH_POWERS)
def test_thin_lens_radius_is_finite_and_inside_the_unit_disk(bokeh_power):
    u = lens_inputs()
    r = both(abi.PT_MATH_BOKEH_POWR, u, np.full(u.size, bokeh_power, F32))
    assert np.all(np.isfinite(r)) and np.all(r >= 0) and np.all(r <= 1) and np.all(r[u == 0] == 0)
    x = np.sqrt(u.astype(F64))
    with np.errstate(all="ignore"):
        e = 1.0 if np.isnan(bokeh_power) else np.exp2(F64(bokeh_power))          # a NaN bokehPower counts as 0
        p = e * np.log2(x)
        want = np.where(x > 0, np.exp2(np.where(x > 0, p, 0.0)), 0.0)
    # where the true value is a normal float it is met; below the range the radius is 0
    ok = (x > 0) & (p > -125) & np.isfinite(p)
    assert np.all(np.abs(r[ok] - want[ok]) <= 1e-5 * want[ok])
    assert np.all(r[(x > 0) & (p < -127.001)] == 0)


def test_thin_lens_radius_keeps_the_unguarded_bits_inside_the_range():
    """wherever both arguments of exp2_det lie in [-126.5, 127.5) the guarded form is powr_det(x, exp2_det(bokehPower)), bit for bit"""
    rng = np.random.default_rng(113)
    n = 1 << 16
    u = F32(np.exp2(rng.uniform(-32, 0, n))).clip(F32(2.0 ** -32), M.ONE_MINUS_EPS)
    bp = F32(rng.uniform(-6, 6, n))
    x = np.sqrt(u)          # IEEE: the same float as sqrtf
    e = f(M.host(abi.PT_MATH_EXP2, bp)[0])
    p = e.astype(F64) * np.log2(x.astype(F64))
    inside = (p >= -126.4) & (p < 127.4)
    assert inside.sum() > n // 3 and (bp[inside] > 3).any() and (bp[inside] < -3).any()
    want = M.host(abi.PT_MATH_POWR, x[inside], e[inside])[0]
    got = M.host(abi.PT_MATH_BOKEH_POWR, u[inside], bp[inside])[0]
    assert np.array_equal(got, want)
    assert np.array_equal(M.oracle(abi.PT_MATH_BOKEH_POWR, u[inside], bp[inside])[0], want)


def test_debug_math_refusals_come_before_the_renderer():
    """unknown fn, n = 0, n > 2^24 and null pointers are refused before the renderer is looked at; a null renderer after that"""
    lib = abi.load_library()
    a = np.zeros(4, F32); o = np.zeros(8, U32)
    pa, po = a.ctypes.data, o.ctypes.data
    for args, word in (((abi.PT_MATH_COUNT, 4, pa, pa, po, po), b"unknown function"), ((abi.PT_MATH_COS, 0, pa, pa, po, po), b"2^24"),
                       ((abi.PT_MATH_COS, (1 << 24) + 1, pa, pa, po, po), b"2^24"), ((abi.PT_MATH_COS, 4, None, pa, po, po), b"null argument"),
                       ((abi.PT_MATH_COS, 4, pa, pa, None, po), b"null argument"), ((abi.PT_MATH_POWR, 4, pa, None, po, po), b"null argument"),
                       ((abi.PT_MATH_SAMPLE_DISK, 4, pa, pa, po, None), b"null argument"), ((abi.PT_MATH_COS, 4, pa, None, po, None), b"null renderer")):
        assert lib.pt_debug_math(None, *args) == -1 and word in lib.pt_last_error(), args


def test_every_guard_set_agrees_between_oracle_and_host_build():
    for name, fn, a, b in M.guard_sets():
        both(fn, a, b)


# ---- the stand-alone sanitizer program ---------------------------------------------------------------------------------------------------

def test_math_emu_main_runs_every_function_over_its_domain(tmp_path):
    """tests/emu/math_emu.cpp with -DMATH_EMU_MAIN: the program a sanitizer build runs; here a plain build, to keep it
    compiling and ending with status 0."""
    exe = str(tmp_path / "math_emu_main")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-DMATH_EMU_MAIN", "-o", exe,
                           os.path.join(root, "tests", "emu", "math_emu.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    assert {int(line.split()[1].rstrip(":")) for line in out.strip().splitlines()} == set(range(abi.PT_MATH_COUNT))


# ---- the guarded call sites inside a render ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bokeh_power", [-8.0, 3.0, 6.0, 200.0])
def test_thin_lens_render_outside_the_ui_range_is_finite_and_equals_the_oracle(bokeh_power):
    """A thin-lens camera with a bokeh power far outside the reference UI's [-1, 1] and no blades at all (fewer than 3 count as 3): the
    product's stage functions and the oracle agree on every byte, and no camera ray is lost to a NaN origin."""
    import emu_lib
    import oracle_lib
    from platinum_amd import scenes
    from platinum_amd.renderer import make_params
    sc = scenes.cornell_sphere_scene(transmission=0.0)
    sc.camera.aperture = 2.8; sc.camera.focus_distance = 12.0; sc.camera.roundness = 0.3; sc.camera.bokeh_power = bokeh_power
    sc.camera.aperture_blades = 0
    p = make_params(48, 27, 1, 3)
    o, e = oracle_lib.OracleScene(sc, p), emu_lib.EmuScene(sc, p)
    assert bytes(o.constants()) == bytes(e.constants()) and o.constants().camera.apertureBlades == 3
    assert o.trace_primary(0).tobytes() == e.trace_primary(0).tobytes()
    sc.camera.bokeh_power = 0.0                                     # a ray with a NaN origin hits nothing: as many hits as at bokeh_power = 0
    hits0 = (oracle_lib.OracleScene(sc, p).trace_primary(0)["instance"] >= 0).mean()
    assert hits0 > 0.5 and abs((o.trace_primary(0)["instance"] >= 0).mean() - hits0) < 0.05
    ro, ho = o.debug_sample(0)
    re_, he = e.debug_sample(0)
    assert np.array_equal(ho, he) and ro.tobytes() == re_.tobytes() and np.all(np.isfinite(ro))
