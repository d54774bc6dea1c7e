"""CPU: the auto-exposure meter (platinum_amd/csrc/pt_exposure.h, built for the host by tests/emu/exposure_emu.cpp) against an independent
numpy restatement of DESIGN.md §3d (np.frexp bins, np.cumsum ranks, float64 resolve): classification, the integer outputs exactly, the
float outputs, the properties, the pt_exposure_options / pt_exposure_meter ABI with its validation, the C++ shim,
and the whole chain on an oracle render."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exposure_lib as ex  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import make_params  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
KEYS = {"below": 256, "above": 257, "nonfinite": 258}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _grey(y, alpha=1.0):
    return np.array([[[y, y, y, alpha]]], np.float32)


# ---- classification ------------------------------------------------------------------------------------------------------------------------
def _np_counter(y):
    b, below, above, nonfinite = ex.np_classify(np.array([y], np.float32))
    return "below" if below[0] else "above" if above[0] else "nonfinite" if nonfinite[0] else int(b[0])


@pytest.mark.parametrize("y,where", ex.SPECIAL_Y + ex.bin_edges())
def test_classification_of_one_luminance(y, where):
    assert ex.lib().ex_host_classify(float(y)) == KEYS.get(where, where)
    assert _np_counter(y) == where     # the restatement agrees with the stated counter


def test_special_card_pixel_by_pixel():
    """One pixel each: every pixel of the special card metered alone lands in the one counter the restatement names."""
    card = ex.special_card()
    assert card.shape[1] == len(ex.SPECIAL_Y) + 512 + 1
    for i in range(card.shape[1]):
        px = card[:, i:i + 1]
        m, _ = ex.host_meter(px, scaled=False)
        b, below, above, nonfinite = ex.np_classify(ex.np_lum(px))
        want = np.zeros(259, np.uint32)
        want[int(b[0, 0]) if b[0, 0] >= 0 else (256 if below[0, 0] else 257 if above[0, 0] else 258)] = 1
        got = np.array(m.bins[:] + [m.below, m.above, m.nonfinite], np.uint32)
        assert np.array_equal(got, want), (i, card[0, i].tolist())
    m, _ = ex.host_meter(card, scaled=False)
    ex.assert_matches_numpy(m, card, None, ex.options(), what="special card")
    assert m.below and m.above and m.nonfinite >= 3 and m.metered > 500


def test_finite_channels_cannot_overflow_the_luminance():
    """The largest finite rgb has Y = FLT_MAX, not inf (the weights sum to 1): it is counted `above`, and nothing finite reaches `nonfinite`."""
    y = ex.np_lum(np.array(ex.LARGEST_RGB, np.float32))
    assert y == ex.FLT_MAX and ex.lib().ex_host_lum(*[float(v) for v in ex.LARGEST_RGB]) == ex.FLT_MAX
    m, _ = ex.host_meter(np.array([[list(ex.LARGEST_RGB) + [1.0]]], np.float32), scaled=False)
    assert (m.above, m.nonfinite, m.metered) == (1, 0, 0)
    for rgb in ((np.inf, 0, 0), (0, -np.inf, 0), (np.inf, -np.inf, 0), (0, 0, np.nan)):     # an inf or NaN channel does
        m, _ = ex.host_meter(np.array([[list(rgb) + [1.0]]], np.float32), scaled=False)
        assert (m.nonfinite, m.above, m.below, m.metered) == (1, 0, 0, 0), rgb


def test_alpha_is_ignored():
    img = ex.log_uniform_card(23, 11, seed=3)
    a, _ = ex.host_meter(img)
    img[..., 3] = np.nan
    b, _ = ex.host_meter(img)
    ex.assert_same_record(a, b)


# ---- integer outputs -----------------------------------------------------------------------------------------------------------------------
FRACTIONS = [(0.10, 0.95), (0.0, 1.0), (0.5, 0.5000001), (0.0, 0.001), (0.999, 1.0), (0.3, 0.7)]


@pytest.mark.parametrize("low,high", FRACTIONS)
@pytest.mark.parametrize("w,h,seed", [(1, 1, 0), (2, 1, 1), (3, 1, 2), (17, 33, 3), (67, 45, 4), (256, 4, 5)])
def test_meter_matches_numpy_on_log_uniform_images(w, h, seed, low, high):
    img = ex.log_uniform_card(w, h, seed, lo=-14.0, hi=14.0) if w * h <= 3 else ex.log_uniform_card(w, h, seed)
    o = ex.options(low_fraction=low, high_fraction=high)
    m, scaled = ex.host_meter(img, o=o)
    ex.assert_matches_numpy(m, img, None, o, what="%dx%d %g..%g" % (w, h, low, high))
    assert m.metered + m.below + m.above + m.nonfinite == w * h
    want = img.copy()
    want[..., :3] *= f32(m.gain)
    assert np.array_equal(_bits(scaled), _bits(want))


def test_constant_image_and_few_pixels():
    o = ex.options()
    img = np.tile(_grey(0.37, 0.5), (64, 64, 1))
    m, _ = ex.host_meter(img, o=o)
    want = ex.assert_matches_numpy(m, img, None, o, what="constant")
    assert m.metered == 4096 and np.count_nonzero(np.array(m.bins[:])) == 1 and m.kept == want["kept"] == 3891 - 409
    # n = 0: nothing metered -> mean_log2 = target_ev = 0, gain 1
    for px in (_grey(0.0), _grey(np.nan), _grey(1e9)):
        m, s = ex.host_meter(px, o=o)
        assert (m.metered, m.kept, m.weighted, m.mean_log2, m.target_ev, m.ev, m.gain) == (0, 0, 0, 0.0, 0.0, 0.0, 1.0)
        ex.assert_matches_numpy(m, px, None, o, what="n = 0")
    # n = 1: lo = hi = 0 -> the fallback keeps the pixel; n = 2: lo = 0, hi = 1 keeps the darker one
    m, _ = ex.host_meter(_grey(0.5), o=o)
    assert (m.metered, m.kept) == (1, 1) and m.mean_log2 == -1.0 + 1.0 / 16.0
    two = np.concatenate([_grey(0.5), _grey(4.0)], axis=1)
    m, _ = ex.host_meter(two, o=o)
    assert (m.metered, m.kept) == (2, 1) and m.mean_log2 == -1.0 + 1.0 / 16.0
    ex.assert_matches_numpy(m, two, None, o, what="n = 2")


def test_boundary_ranks_split_a_bin():
    """Three bins of 10 pixels, fractions 0.15 / 0.85: ranks [4, 25) keep 6 of the first bin, all of the second, 5 of the third."""
    bins = np.zeros(256, np.uint64)
    bins[[100, 101, 130]] = 10
    o = ex.options(low_fraction=0.15, high_fraction=0.85)
    m = ex.host_resolve(bins, o)
    assert (m.metered, m.kept, m.weighted) == (30, 21, 6 * 201 + 10 * 203 + 5 * 261)
    want = ex.np_resolve(bins, o)
    assert (m.kept, m.weighted) == (want["kept"], want["weighted"]) and abs(m.mean_log2 - want["mean_log2"]) <= 1e-5
    # the fallback: fractions that round to the same rank keep everything
    o = ex.options(low_fraction=0.5, high_fraction=0.51)
    m = ex.host_resolve(bins, o)
    assert (m.kept, m.weighted) == (30, 10 * (201 + 203 + 261))
    # counts that do not fit 32 bits in the sums: 256 bins of 2^24 pixels
    big = np.full(256, 1 << 24, np.uint64)
    m = ex.host_resolve(big, ex.options(low_fraction=0.0, high_fraction=1.0))
    want = ex.np_resolve(big, ex.options(low_fraction=0.0, high_fraction=1.0))
    assert m.weighted == want["weighted"] == (1 << 24) * 256 * 256 and m.mean_log2 == 0.0


# ---- float outputs -------------------------------------------------------------------------------------------------------------------------
def test_clamps_and_gain_bits():
    img = ex.log_uniform_card(31, 17, seed=9, lo=-3.0, hi=1.0)
    for lo_ev, hi_ev in ((-16.0, 16.0), (-0.25, 0.25), (3.0, 5.0), (-5.0, -3.0), (0.0, 0.0), (-32.0, 32.0)):
        for target in (-2.4739313, 8.0, -12.0, 32.0, -32.0):
            o = ex.options(min_ev=lo_ev, max_ev=hi_ev, target_log2=target)
            m, _ = ex.host_meter(img, o=o, scaled=False)
            want = ex.assert_matches_numpy(m, img, None, o, what=str((lo_ev, hi_ev, target)))
            assert lo_ev <= m.target_ev <= hi_ev and m.ev == m.target_ev
            assert np.isfinite(m.gain) and m.gain > 0.0 and abs(m.gain / want["gain"] - 1.0) <= 1e-5


def test_smoothing_sequence_and_reset():
    imgs = [ex.log_uniform_card(16, 16, seed=s, lo=c - 2.0, hi=c + 2.0) for s, c in ((1, -6.0), (2, 3.0), (3, 0.0), (4, 9.0))]
    o = ex.options(smoothing=0.75)
    prev, prev64 = None, None
    for k, img in enumerate(imgs):
        m, _ = ex.host_meter(img, o=o, prev_ev=prev)
        want = ex.assert_matches_numpy(m, img, None, o, prev_ev=prev, what="step %d" % k)
        if k == 0:
            assert m.ev == m.target_ev            # the first use starts from its own target
        else:
            assert m.ev == f32(prev) + (f32(1.0) - f32(0.75)) * (f32(m.target_ev) - f32(prev))     # the recurrence, in float32
            prev64 = prev64 + 0.25 * (want["target_ev"] - prev64)
            assert abs(m.ev - prev64) <= 1e-5 * (k + 1)
        prev, prev64 = m.ev, (want["target_ev"] if k == 0 else prev64)
    m, _ = ex.host_meter(imgs[0], o=o, prev_ev=None)      # a reset: the next one starts from its own target again
    assert m.ev == m.target_ev
    # smoothing 0 ignores the state
    m, _ = ex.host_meter(imgs[1], o=ex.options(), prev_ev=5.0)
    assert m.ev == m.target_ev


# ---- properties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-6, -1, 1, 5])
def test_scaling_by_a_power_of_two_moves_the_mean_by_its_exponent(k):
    img = ex.log_uniform_card(41, 23, seed=11, lo=-9.0, hi=9.0)     # stays inside [2^-16, 2^16) for |k| <= 6
    a, sa = ex.host_meter(img)
    scaled_in = img.copy()
    scaled_in[..., :3] *= f32(2.0 ** k)
    b, sb = ex.host_meter(scaled_in)
    assert a.metered == b.metered == 41 * 23 and (a.kept, a.below, a.above) == (b.kept, 0, 0)
    assert b.mean_log2 == a.mean_log2 + k and b.weighted == a.weighted + 16 * k * a.kept
    assert b.mean_log2 + b.ev == a.mean_log2 + a.ev
    assert np.array_equal(np.roll(np.array(a.bins[:]), 8 * k), np.array(b.bins[:]))
    assert np.array_equal(_bits(sa), _bits(sb))        # the scaled images are the same image


def test_meter_of_a_region_is_the_meter_of_the_crop():
    img = ex.special_card().reshape(-1, 4)
    img = np.concatenate([img, ex.log_uniform_card(67 * 45 - len(img), 1, seed=5).reshape(-1, 4)]).reshape(45, 67, 4)
    for rect in ((3, 2, 14, 9), (0, 0, 67, 45), (66, 44, 67, 45), (5, 0, 6, 45), (1, 7, 66, 8)):
        x0, y0, x1, y1 = rect
        o = ex.options(smoothing=0.5)
        a, sa = ex.host_meter(img, rect=rect, o=o, prev_ev=1.5)
        b, _ = ex.host_meter(img[y0:y1, x0:x1], o=o, prev_ev=1.5)
        ex.assert_same_record(a, b, str(rect))
        ex.assert_matches_numpy(a, img, rect, o, prev_ev=1.5, what=str(rect))
        want = img.copy()                          # the whole frame is scaled, not the rectangle alone
        with np.errstate(all="ignore"):
            want[..., :3] *= f32(a.gain)
        same = (_bits(sa) == _bits(want)) | (np.isnan(sa) & np.isnan(want))
        assert same.all()


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
def test_exposure_structs_abi():
    lay = ex.layout()
    O, M = abi.ExposureOptions, abi.ExposureMeter
    assert lay[0] == C.sizeof(O) == 28
    assert lay[1:8] == [getattr(O, n).offset for n, _ in O._fields_] == [0, 4, 8, 12, 16, 20, 24]
    assert lay[8] == C.sizeof(M) == 1072
    names = ("bins", "below", "above", "nonfinite", "metered", "kept", "weighted", "mean_log2", "target_ev", "ev", "gain")
    assert lay[9:20] == [getattr(M, n).offset for n in names] == [0, 1024, 1028, 1032, 1036, 1040, 1048, 1056, 1060, 1064, 1068]
    lib = abi.load_library()
    o = O(7, 7.0, 7.0, 7.0, 7.0, 7.0, 7.0)
    lib.pt_default_exposure_options(C.byref(o))
    d = ex.options()
    assert [getattr(o, n) for n, _ in O._fields_] == [getattr(d, n) for n, _ in O._fields_]
    assert (o.enabled, o.target_log2, o.low_fraction, o.high_fraction, o.min_ev, o.max_ev, o.smoothing) == (
        0, f32(-2.4739313), f32(0.10), f32(0.95), -16.0, 16.0, 0.0)
    assert abs(o.target_log2 - np.log2(0.18)) < 1e-6
    lib.pt_default_exposure_options(None)


GOOD = [{}, dict(enabled=1), dict(target_log2=32.0), dict(target_log2=-32.0), dict(low_fraction=0.0, high_fraction=1.0), dict(min_ev=-32.0, max_ev=32.0),
        dict(min_ev=2.0, max_ev=2.0), dict(smoothing=0.999), dict(low_fraction=0.94)]
BAD = [(dict(target_log2=32.5), b"target_log2"), (dict(target_log2=float("nan")), b"target_log2"), (dict(target_log2=float("inf")), b"target_log2"),
       (dict(low_fraction=-0.01), b"fraction"), (dict(low_fraction=0.95), b"fraction"), (dict(low_fraction=0.96), b"fraction"),
       (dict(high_fraction=1.01), b"fraction"), (dict(high_fraction=float("nan")), b"fraction"), (dict(low_fraction=float("nan")), b"fraction"),
       (dict(min_ev=-33.0), b"min_ev"), (dict(max_ev=33.0), b"min_ev"), (dict(min_ev=1.0, max_ev=0.5), b"min_ev"),
       (dict(min_ev=float("nan")), b"min_ev"), (dict(max_ev=float("inf")), b"min_ev"), (dict(min_ev=float("-inf")), b"min_ev"),
       (dict(smoothing=1.0), b"smoothing"), (dict(smoothing=-0.1), b"smoothing"), (dict(smoothing=float("nan")), b"smoothing")]


def test_validation_before_the_renderer():
    """The options are checked before the renderer: a valid struct reaches the null-renderer test, an invalid one does not."""
    lib = abi.load_library()
    for f in GOOD:
        for en in (0, 1):
            o = ex.options(**f)
            o.enabled = en
            assert ex.lib().ex_host_options_valid(C.byref(o)) == 1
            assert lib.pt_set_exposure_options(None, C.byref(o)) == -1 and b"null renderer" in lib.pt_last_error(), f
    img = np.ones((2, 2, 4), np.float32)
    m = abi.ExposureMeter()
    for f, word in BAD:
        for en in (0, 1):
            o = ex.options(**f)
            o.enabled = en
            assert ex.lib().ex_host_options_valid(C.byref(o)) == 0
            assert lib.pt_set_exposure_options(None, C.byref(o)) == -1 and word in lib.pt_last_error(), f   # PT_ERR_INVALID_ARGUMENT
            assert lib.pt_debug_exposure(None, img.ctypes.data, 2, 2, None, C.byref(o), C.byref(m), None) == -1 and word in lib.pt_last_error(), f
    assert lib.pt_set_exposure_options(None, None) == -1
    assert lib.pt_reset_exposure(None) == -1 and lib.pt_read_exposure_meter(None, C.byref(m)) == -1
    # pt_debug_exposure: nulls, an empty image, rectangles that are empty or do not fit, all before the renderer
    o = ex.options()
    assert lib.pt_debug_exposure(None, None, 2, 2, None, C.byref(o), C.byref(m), None) == -1
    assert lib.pt_debug_exposure(None, img.ctypes.data, 2, 2, None, None, C.byref(m), None) == -1
    assert lib.pt_debug_exposure(None, img.ctypes.data, 2, 2, None, C.byref(o), None, None) == -1
    assert lib.pt_debug_exposure(None, img.ctypes.data, 0, 2, None, C.byref(o), C.byref(m), None) == -1 and b"pixels" in lib.pt_last_error()
    for rect in ((0, 0, 3, 2), (0, 0, 2, 3), (1, 0, 1, 2), (0, 2, 2, 2), (2, 0, 1, 1)):
        r = (C.c_uint32 * 4)(*rect)
        assert lib.pt_debug_exposure(None, img.ctypes.data, 2, 2, C.addressof(r), C.byref(o), C.byref(m), None) == -1 and b"rectangle" in lib.pt_last_error(), rect
    assert lib.pt_debug_exposure(None, img.ctypes.data, 2, 2, None, C.byref(o), C.byref(m), None) == -1 and b"null renderer" in lib.pt_last_error()


def test_cpp_shim_round_trips_the_options_and_python_has_the_accessors(tmp_path):
    tu = tmp_path / "exposure_accessors.cpp"
    tu.write_text('#include "ptamd_renderer.hpp"\n'
                  '#include <cstddef>\n'
                  "int main() {\n"
                  "  pt_exposure_options o;\n"
                  "  pt_default_exposure_options(&o);\n"
                  "  if (o.enabled != 0u || o.high_fraction != 0.95f || o.max_ev != 16.0f) return 2;\n"
                  "  o.enabled = 1u; o.smoothing = 0.5f; o.target_log2 = -3.0f;\n"
                  "  ptamd::renderer_pt::Renderer* r = nullptr;\n"
                  "  if (r) {\n"
                  "    pt_exposure_options& e = r->exposureOptions();\n"
                  "    e = o;\n"
                  "    if (r->exposureOptions().smoothing != 0.5f) return 3;\n"
                  "    r->resetExposure();\n"
                  "    pt_exposure_meter m;\n"
                  "    if (!r->readExposureMeter(&m)) return 4;\n"
                  "  }\n"
                  "  if (pt_set_exposure_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 5;   // valid options, no renderer\n"
                  "  o.smoothing = 1.0f;\n"
                  "  if (pt_set_exposure_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 6;\n"
                  "  static_assert(sizeof(pt_exposure_options) == 28 && sizeof(pt_exposure_meter) == 1072, \"auto exposure structs\");\n"
                  "  static_assert(offsetof(pt_exposure_meter, weighted) == 1048 && offsetof(pt_exposure_meter, gain) == 1068, \"pt_exposure_meter\");\n"
                  "  return 0;\n"
                  "}\n")
    exe = tmp_path / "exposure_accessors"
    libdir = os.path.join(ROOT, "platinum_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tu), "-o", str(exe),
                           "-L" + libdir, "-lptamd", "-Wl,-rpath," + libdir])
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
    from platinum_amd.renderer import Renderer
    for member in ("exposureOptions", "setExposureOptions", "resetExposure", "readbackExposureMeter", "debugExposure"):
        assert callable(getattr(Renderer, member)), member


# ---- the whole chain on the oracle ---------------------------------------------------------------------------------------------------------
def _srgb_decode(c):
    c = np.asarray(c, np.float64)
    return np.where(c < 12.92 * 0.0031308, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def test_metered_oracle_render_lands_on_the_target():
    """Cornell `bench` 64x64, 16 spp from the oracle; metered over all binned pixels (fractions 0 / 1: "the metered pixels" are then the kept
    ones), scaled, and post-processed by the oracle.  The image entering the tonemapper is recovered from the oracle's float display: no
    tonemapper, the working space as the output space (identity), and the user's exposure at -10 EV as compensation so that nothing clips at
    display white; the sRGB encoding is inverted in float64 and the 10 EV are added back.  Its mean log2 luminance over the metered pixels
    equals target_log2 to within one bin width, 1/8 EV: a pixel's bin centre is within 1/16 EV of an eighth-octave edge, and the bins are
    linear in the mantissa, which puts them at most 0.086 EV from the logarithmic eighths; measured here: 0.059 EV above the target."""
    import oracle_lib
    import post_lib
    sc = scenes.cornell_scene("bench")
    o = oracle_lib.OracleScene(sc, make_params(64, 64, 16, 4))
    try:
        acc = o.render(0, 16, threads=oracle_lib.host_threads())
        for target in (-2.4739313, 0.0):
            opts = ex.options(enabled=1, target_log2=target, low_fraction=0.0, high_fraction=1.0)
            m, scaled = ex.host_meter(acc, o=opts)
            assert m.metered > 3000 and m.target_ev == m.ev and -16.0 < m.ev < 16.0
            po, to = post_lib.defaults()
            po.exposure = -10.0
            to.tonemapper = abi.TONEMAP_NONE
            to.output_space = scenes.colorspace(scenes.BT2020)
            _rgba8, display = o.postprocess(scaled, po, to, want_float=True)
            assert display.max() < 1.0
            b, _below, _above, _nonfinite = ex.np_classify(ex.np_lum(acc))
            lin = _srgb_decode(display)
            Y = lin @ np.array([0.2126, 0.7152, 0.0722])
            mean = float(np.mean(np.log2(Y[b >= 0]))) + 10.0
            print("target %g: metered %d, ev %.4f, display mean log2 luminance %.4f (off by %.4f EV)" % (target, m.metered, m.ev, mean, mean - target))
            assert abs(mean - target) <= 0.125
    finally:
        o.close()
