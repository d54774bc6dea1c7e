"""Bloom without a GPU: the host build of pt_bloom.h (tests/emu/bloom_emu.cpp) against an independent numpy restatement
in float64, pt_plan_bloom against an enumeration, the properties the arithmetic promises (fixed point, energy, identity below the
threshold, exact scaling, non-finite pixels, alpha), the ABI through libptamd.so, the C++ accessor and a stand-alone
sanitizer build of the host code."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bloom_lib as bl
from platinum_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _set(name):
    return bl.options(**bl.OPTION_SETS[name])


# ---- the float32 bound ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def measured():
    return bl.measure_float32_error()


def test_the_recorded_bound_is_four_times_the_float32_restatements_own_error(measured):
    print("numpy float32 against float64: %.4g (recorded %.4g, bound %.4g)" % (measured, bl.BOUNDS["measured"], bl.BOUNDS["bound"]))
    assert bl.BOUNDS["bound"] == 4 * bl.BOUNDS["measured"]
    assert 0.99 * bl.BOUNDS["measured"] <= measured <= bl.BOUNDS["measured"]


# ---- host build against the float64 restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setname", list(bl.OPTION_SETS))
@pytest.mark.parametrize("W,H", bl.SIZES)
@pytest.mark.parametrize("name", bl.CARDS)
def test_host_build_matches_the_float64_restatement(name, W, H, setname):
    o = _set(setname)
    img = bl.card(name, W, H)
    out, pyr = bl.host_bloom(img, o, pyramid=True)
    ref, U = bl.np_bloom(img, o, np.float64, pyramid=True)
    L, _, _, total = bl.np_plan(W, H, o.levels)
    assert pyr.shape == (total, 4) and len(U) == L
    e_img = bl.rel_err(out[..., :3], ref[..., :3])
    e_pyr = bl.rel_err(pyr[:, :3], bl.np_pyramid_flat(U)) if L else 0.0
    print("%s %dx%d %s: image %.3g pyramid %.3g (bound %.3g)" % (name, W, H, setname, e_img, e_pyr, bl.BOUNDS["bound"]))
    assert e_img <= bl.BOUNDS["bound"] and e_pyr <= bl.BOUNDS["bound"]
    assert np.array_equal(bl.bits(out[..., 3]), bl.bits(img[..., 3]))
    assert not pyr[:, 3].any()


def test_bright_pass_special_values():
    """Threshold 0 with knee 0 is w = 1 exactly; non-finite, non-positive and overflowing luminances scatter nothing; the cap is 2^64."""
    def bright(px, **f):
        o = bl.options(**f)
        a = np.array(list(px) + [1.0], np.float32)
        b = np.zeros(3, np.float32)
        bl.lib().bl_host_bright(a.ctypes.data, C.byref(o), b.ctypes.data)
        return b
    rng = np.random.default_rng(5)
    for _ in range(200):
        px = np.exp2(rng.uniform(-20, 20, 3)).astype(np.float32)
        assert np.array_equal(bl.bits(bright(px)), bl.bits(px))
    for px in ((np.nan, 1, 1), (1, np.inf, 1), (1, 1, -np.inf), (0, 0, 0), (-1, -1, -1), (3.3e38, 3.3e38, 3.3e38), (-5, 0.1, 0.1)):
        assert not bright(px).any(), px
    assert np.array_equal(bright((1e30, 1e30, 1e30)), np.full(3, 2.0 ** 64, np.float32))
    assert np.array_equal(bright((-1.0, 4.0, 1.0)), np.array([0.0, 4.0, 1.0], np.float32))   # a negative channel under a positive luminance
    # below threshold - knee nothing, above threshold + knee the hard curve, between them the quadratic
    Y = lambda v: (f32(0.2126) * f32(v) + f32(0.7152) * f32(v)) + f32(0.0722) * f32(v)
    assert not bright((0.4, 0.4, 0.4), threshold=1.0, knee=0.5).any()
    y = Y(2.0)
    assert np.array_equal(bright((2.0, 2.0, 2.0), threshold=1.0, knee=0.5), np.full(3, f32(2.0) * ((y - f32(1.0)) / y), np.float32))
    y = Y(1.0)
    s = (y - f32(1.0)) + f32(0.5)
    assert np.array_equal(bright((1.0, 1.0, 1.0), threshold=1.0, knee=0.5), np.full(3, f32(1.0) * (((s * s) / (f32(4.0) * f32(0.5) + f32(1e-6))) / y), np.float32))


def test_norm_is_the_running_sum_of_the_running_power():
    for L in range(0, 13):
        for s in (1.0, 0.6, 0.5, 1e-3):
            n, p = f32(0), f32(1)
            for _ in range(L):
                n = f32(n + p)
                p = f32(p * f32(s))
            assert bl.lib().bl_host_norm(L, s) == n
    assert bl.lib().bl_host_norm(12, 1.0) == 12.0


# ---- pt_plan_bloom -------------------------------------------------------------------------------------------------------------------------
PLAN_SIZES = bl.SIZES + [(1920, 1080), (3840, 2160), (8192, 1), (258, 128), (254, 128)]


@pytest.mark.parametrize("W,H", PLAN_SIZES)
def test_plan_matches_an_enumeration(W, H):
    lib = abi.load_library()
    for levels in range(1, 13):
        L, lv, offs, total = bl.np_plan(W, H, levels)
        exported = abi.BloomPlan()
        assert lib.pt_plan_bloom(W, H, levels, C.byref(exported)) == 0
        for p in (bl.host_plan(W, H, levels), exported):
            assert (p.levels, p.total_texels) == (L, total), (W, H, levels)
            assert list(p.width)[:L + 1] == [w for w, _ in lv] and list(p.height)[:L + 1] == [h for _, h in lv]
            assert list(p.offset)[:L + 1] == offs
            assert not any(list(p.width)[L + 1:]) and not any(list(p.height)[L + 1:]) and not any(list(p.offset)[L + 1:])
        assert L == min(levels, max(W - 1, H - 1).bit_length())
        assert (L >= 1) == (W * H > 1)


def test_plan_refusals():
    lib = abi.load_library()
    p = abi.BloomPlan()
    assert lib.pt_plan_bloom(4, 4, 6, None) == -1
    for W, H, levels in ((0, 4, 6), (4, 0, 6), (1 << 15, (1 << 13) + 1, 6), (4, 4, 0), (4, 4, 13)):
        assert lib.pt_plan_bloom(W, H, levels, C.byref(p)) == -1, (W, H, levels)
    assert lib.pt_plan_bloom(1 << 14, 1 << 14, 12, C.byref(p)) == 0 and p.total_texels == sum((1 << (14 - l)) ** 2 for l in range(1, 13))


# ---- properties of the host build ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setname", list(bl.OPTION_SETS))
@pytest.mark.parametrize("W,H", bl.SIZES)
def test_a_constant_image_stays_constant(W, H, setname):
    img = bl.card("constant", W, H)
    out = bl.host_bloom(img, _set(setname))
    assert bl.rel_err(out[..., :3], img[..., :3].astype(np.float64)) <= bl.BOUNDS["bound"]


@pytest.mark.parametrize("N,levels", [(64, 3), (128, 4)])
def test_an_impulse_keeps_its_energy(N, levels):
    """The footprint stays inside the image (rows and columns 17..46 of 64 at 3 levels), so no clamped tap folds light back: the float64
    sum of every channel is the input's, as closely as the float32 restatement itself keeps it (x 4)."""
    img = bl.card("impulse", N, N)
    for f in (dict(levels=levels), dict(levels=levels, intensity=1.0, scatter=0.6), dict(levels=levels, intensity=0.3, threshold=0.5, knee=0.25)):
        o = bl.options(**f)
        out = bl.host_bloom(img, o)
        ref32 = bl.np_bloom(img, o, np.float32)
        lit = np.argwhere(out[..., :3].any(axis=-1))
        lo, hi = (17, 46) if N == 64 else (1, N - 2)   # (no lit pixel on the border: no tap was clamped on the way)
        assert lit.min() >= lo and lit.max() <= hi, (lit.min(), lit.max())
        for c in range(3):
            want = float(img[..., c].astype(np.float64).sum())
            dev_np = abs(float(ref32[..., c].astype(np.float64).sum()) - want)
            dev = abs(float(out[..., c].astype(np.float64).sum()) - want)
            print("N %d %s channel %d: host build off by %.3g, float32 restatement by %.3g" % (N, f, c, dev, dev_np))
            assert dev <= 4 * dev_np


def test_below_the_threshold_an_image_keeps_its_bits():
    rng = np.random.default_rng(11)
    img = np.exp2(rng.uniform(-12.0, -1.01, (45, 67, 4))).astype(np.float32)   # luminance < 0.5 = threshold - knee
    img[3, 4, :3] = 0.0
    img[5, 6, :3] = [-0.25, 0.1, 0.0]
    for f in (dict(threshold=1.0, knee=0.5), dict(threshold=0.5, knee=0.0, intensity=1.0, levels=12)):
        out = bl.host_bloom(img, bl.options(**f))
        assert np.array_equal(bl.bits(out), bl.bits(img))


@pytest.mark.parametrize("k", [-3, 3])
@pytest.mark.parametrize("name", ["loguniform", "edge", "impulse"])
def test_at_threshold_zero_bloom_commutes_with_a_power_of_two(name, k):
    img = bl.card(name, 67, 45)
    g = f32(2.0 ** k)
    scaled = img.copy()
    scaled[..., :3] *= g
    for f in ({}, dict(scatter=0.6, levels=12, intensity=1.0)):
        o = bl.options(**f)
        a, pa = bl.host_bloom(scaled, o, pyramid=True)
        b, pb = bl.host_bloom(img, o, pyramid=True)
        b = b.copy()
        b[..., :3] *= g
        assert np.array_equal(bl.bits(a), bl.bits(b))
        assert np.array_equal(bl.bits(pa), bl.bits(pb * g))


@pytest.mark.parametrize("setname", list(bl.OPTION_SETS))
@pytest.mark.parametrize("W,H", bl.SIZES)
def test_a_nan_and_an_infinite_pixel_scatter_nothing(W, H, setname):
    o = _set(setname)
    img = bl.card("nonfinite", W, H)
    bad = sorted(set(bl.nonfinite_pixels(W, H)))
    black = img.copy()
    black.reshape(-1, 4)[bad, :3] = 0.0
    out, pyr = bl.host_bloom(img, o, pyramid=True)
    ref, pyr_ref = bl.host_bloom(black, o, pyramid=True)
    flat, flat_in, flat_ref = out.reshape(-1, 4), img.reshape(-1, 4), ref.reshape(-1, 4)
    assert np.array_equal(bl.bits(flat[bad]), bl.bits(flat_in[bad]))
    rest = np.setdiff1d(np.arange(W * H), bad)
    assert np.isfinite(flat[rest]).all() and np.isfinite(pyr).all()
    assert np.array_equal(bl.bits(flat[rest]), bl.bits(flat_ref[rest]))
    assert np.array_equal(bl.bits(pyr), bl.bits(pyr_ref))


def test_a_one_pixel_image_keeps_its_bits_and_alpha_is_always_copied():
    for px in ((0.3, 7.0, 2.0, 0.25), (np.nan, 1.0, np.inf, -0.0), (-0.0, -1.0, 1e38, np.nan)):
        img = np.array(px, np.float32).reshape(1, 1, 4)
        for setname in bl.OPTION_SETS:
            assert np.array_equal(bl.bits(bl.host_bloom(img, _set(setname))), bl.bits(img))
    rng = np.random.default_rng(2)
    img = bl.card("loguniform", 33, 31).copy()
    img[..., 3] = rng.integers(0, 2 ** 32, (31, 33), dtype=np.uint32).view(np.float32)   # any bits: NaN payloads, -0, denormals
    for setname in bl.OPTION_SETS:
        assert np.array_equal(bl.bits(bl.host_bloom(img, _set(setname))[..., 3]), bl.bits(img[..., 3]))


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
def test_bloom_structs_abi():
    lay = bl.layout()
    O, P = abi.BloomOptions, abi.BloomPlan
    assert lay[0] == C.sizeof(O) == 24
    assert lay[1:7] == [getattr(O, n).offset for n, _ in O._fields_] == [0, 4, 8, 12, 16, 20]
    assert lay[7] == C.sizeof(P) == 8 + 3 * 13 * 4
    assert lay[8:13] == [getattr(P, n).offset for n, _ in P._fields_] == [0, 4, 8, 60, 112]
    assert lay[13] == abi.BLOOM_MAX_LEVELS == 12
    lib = abi.load_library()
    o = O(7, 7.0, 7.0, 7.0, 7.0, 7)
    lib.pt_default_bloom_options(C.byref(o))
    d = bl.options()
    assert [getattr(o, n) for n, _ in O._fields_] == [getattr(d, n) for n, _ in O._fields_]
    assert (o.enabled, o.intensity, o.threshold, o.knee, o.scatter, o.levels) == (0, f32(0.05), 0.0, 0.0, 1.0, 6)
    lib.pt_default_bloom_options(None)


GOOD = [{}, dict(enabled=1), dict(intensity=0.0), dict(intensity=1.0), dict(threshold=1e30, knee=1e30), dict(scatter=1e-6), dict(scatter=1.0),
        dict(levels=1), dict(levels=12)]
BAD = [(dict(intensity=-0.01), b"intensity"), (dict(intensity=1.01), b"intensity"), (dict(intensity=float("nan")), b"intensity"),
       (dict(threshold=-1.0), b"threshold"), (dict(threshold=float("inf")), b"threshold"), (dict(threshold=float("nan")), b"threshold"),
       (dict(knee=-0.5), b"knee"), (dict(knee=float("inf")), b"knee"), (dict(knee=float("nan")), b"knee"),
       (dict(scatter=0.0), b"scatter"), (dict(scatter=-0.5), b"scatter"), (dict(scatter=1.5), b"scatter"), (dict(scatter=float("nan")), b"scatter"),
       (dict(levels=0), b"levels"), (dict(levels=13), b"levels")]


def test_validation_before_the_renderer():
    """The options are checked before the renderer: a valid struct reaches the null-renderer test, an invalid one does not."""
    lib = abi.load_library()
    img = np.ones((2, 2, 4), np.float32)
    out = np.zeros((2, 2, 4), np.float32)
    for f in GOOD:
        o = bl.options(**f)
        assert bl.lib().bl_host_options_valid(C.byref(o)) == 1
        assert lib.pt_set_bloom_options(None, C.byref(o)) == -1 and b"null renderer" in lib.pt_last_error(), f
        assert lib.pt_debug_bloom(None, img.ctypes.data, 2, 2, C.byref(o), out.ctypes.data, None) == -1 and b"null renderer" in lib.pt_last_error(), f
    for f, word in BAD:
        for en in (0, 1):
            o = bl.options(**f)
            o.enabled = en
            assert bl.lib().bl_host_options_valid(C.byref(o)) == 0
            assert lib.pt_set_bloom_options(None, C.byref(o)) == -1 and word in lib.pt_last_error(), f   # PT_ERR_INVALID_ARGUMENT
            assert lib.pt_debug_bloom(None, img.ctypes.data, 2, 2, C.byref(o), out.ctypes.data, None) == -1 and word in lib.pt_last_error(), f
    assert lib.pt_set_bloom_options(None, None) == -1
    o = bl.options()
    assert lib.pt_debug_bloom(None, None, 2, 2, C.byref(o), out.ctypes.data, None) == -1
    assert lib.pt_debug_bloom(None, img.ctypes.data, 2, 2, None, out.ctypes.data, None) == -1
    assert lib.pt_debug_bloom(None, img.ctypes.data, 2, 2, C.byref(o), None, None) == -1
    assert lib.pt_debug_bloom(None, img.ctypes.data, 0, 2, C.byref(o), out.ctypes.data, None) == -1 and b"pixels" in lib.pt_last_error()
    assert lib.pt_debug_bloom(None, img.ctypes.data, 1 << 15, (1 << 13) + 1, C.byref(o), out.ctypes.data, None) == -1 and b"pixels" in lib.pt_last_error()


def test_cpp_accessor_round_trips_the_options_and_python_has_the_accessors(tmp_path):
    exe = tmp_path / "bloom_accessors"
    libdir = os.path.join(ROOT, "platinum_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bloom_accessors.cpp"), "-o", str(exe), "-L" + libdir, "-lptamd", "-Wl,-rpath," + libdir])
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
    from platinum_amd.renderer import Renderer
    for member in ("bloomOptions", "setBloomOptions", "debugBloom"):
        assert callable(getattr(Renderer, member)), member


# ---- the host code under sanitizers, stand-alone -------------------------------------------------------------------------------------------
def test_host_build_runs_clean_under_asan_and_ubsan_as_a_program_of_its_own(tmp_path):
    """tests/emu/bloom_emu.cpp with its own main, over the sizes above and 8192 x 1 with 12 levels.  (Nothing loaded into Python runs
    under a sanitizer.)"""
    exe = tmp_path / "bloom_emu_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DBLOOM_EMU_MAIN", "-o", str(exe), bl.SRC])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]
    assert "8192 x 1, 12 levels (8190 texels)" in p.stdout
