"""CPU: the denoiser's firefly clamp (platinum_amd/csrc/pt_denoise.h dn_despeckle_pixel, built for the host by tests/emu/despeckle_emu.cpp)
against a float64 restatement of DESIGN.md §3a "Firefly clamp", its properties bit for bit, the pt_despeckle_options ABI and its
validation, and its quality on Cornell against the oracle.  (The kernel's register budget: tests/test_kernel_resources.py.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_lib as dl  # noqa: E402
import despeckle_lib as ds  # noqa: E402
from test_denoise_host import random_inputs  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import make_params  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def spiky_inputs(seed, H, W):
    """random_inputs with 3 % of the pixels multiplied by 50-5000: single samples far brighter than their neighbours."""
    rng = np.random.default_rng(seed)
    acc, a, n, m, N = random_inputs(rng, H, W)
    spike = rng.random((H, W)) < 0.03
    acc[..., :3] = np.where(spike[..., None], acc[..., :3] * rng.uniform(50.0, 5000.0, (H, W, 1)).astype(np.float32), acc[..., :3])
    return acc, a, n, m, N, spike


# the shapes of test_denoise_host.py's comparison with its restatement
SHAPES = [(1, 1, 0), (7, 13, 1), (17, 9, 2), (33, 21, 3), (24, 40, 4), (19, 23, 5), (12, 12, 6), (29, 11, 7), (40, 31, 8), (41, 37, 9)]


@pytest.mark.parametrize("threshold", [1.0, 2.0, 8.0])
@pytest.mark.parametrize("H,W,seed", SHAPES)
def test_host_stage_matches_float64_restatement(H, W, seed, threshold):
    acc, a, n, m, N, spike = spiky_inputs(seed, H, W)
    got = ds.host_stage(acc, a, n, m, N, threshold=threshold)
    col, L, lim, used = ds.np_stage(acc, a, n, m, N, threshold=threshold)
    # a pixel whose luminance lies within a relative 1e-5 of its limit may fall on either side of the comparison in float32
    with np.errstate(invalid="ignore"):
        near = used & (np.abs(L - lim) <= 1e-5 * np.abs(lim))
    share = float(near.mean())
    print("%dx%d threshold %g: %d clamped, %d within 1e-5 of the limit (share %.4f)" % (
        W, H, threshold, int((used & (L > lim) & (L > 0)).sum()), int(near.sum()), share))
    assert share <= 0.005
    if H * W > 1:
        assert (used & (L > lim)).any()     # the clamp is exercised
    np.testing.assert_allclose(got[~near], col[~near], rtol=1e-4, atol=1e-6)


def test_disabled_stage_is_the_prep():
    acc, a, n, m, N, _ = spiky_inputs(21, 15, 22)
    I, v, valid, _geo = ds.np_prep(acc, a, n, m, N)
    got = ds.host_stage(acc, a, n, m, N, enabled=0)
    np.testing.assert_allclose(got, np.concatenate([I, v[..., None]], -1), rtol=1e-5, atol=1e-7)


# ---- properties, bit for bit -------------------------------------------------------------------------------------------------------------
def flat_inputs(H, W, value=0.25):
    """A constant geometry image with albedo 1: the prep's demodulated colour is the accumulator's bits."""
    acc = np.empty((H, W, 4), np.float32)
    acc[..., :3] = value
    acc[..., 3] = 1.0
    a = np.ones((H, W, 4), np.float32)
    n = np.broadcast_to(np.array([0.0, 0.0, 1.0, 1.0], np.float32), (H, W, 4)).copy()
    m = np.zeros((H, W, 4), np.float32)
    m[..., 0] = 5.0
    m[..., 1] = value
    m[..., 2] = value * value + 0.5
    return acc, a, n, m, 4


def test_image_without_outliers_is_unchanged():
    rng = np.random.default_rng(31)
    acc, a, n, m, N = random_inputs(rng, 23, 19)
    # colours in [1, 1.9] over albedo in [0.05, 0.95]: the luminance ratio of two neighbours can reach 36, so use threshold 64
    acc[..., :3] = rng.uniform(1.0, 1.9, (23, 19, 3)).astype(np.float32)
    off = ds.host_stage(acc, a, n, m, N, enabled=0)
    on = ds.host_stage(acc, a, n, m, N, enabled=1, threshold=64.0)
    _col, L, lim, used = ds.np_stage(acc, a, n, m, N, threshold=64.0)
    assert used.any() and not (used & (L > 0.99 * lim)).any()    # (the premise, with a margin float32 cannot cross)
    assert np.array_equal(_bits(on), _bits(off))
    for it in (1, 5):
        assert np.array_equal(_bits(ds.host_filter(acc, a, n, m, N, iterations=it, enabled=1, threshold=64.0)),
                              _bits(dl.host_filter(acc, a, n, m, N, iterations=it)))


@pytest.mark.parametrize("threshold", [1.0, 2.0, 8.0])
def test_single_spike_in_a_constant_field_becomes_threshold_times_the_field(threshold):
    acc, a, n, m, N = flat_inputs(9, 11)
    acc[4, 5, :3] = [100.0, 300.0, 700.0]
    off = ds.host_stage(acc, a, n, m, N, enabled=0)
    on = ds.host_stage(acc, a, n, m, N, enabled=1, threshold=threshold)
    keep = np.ones((9, 11), bool)
    keep[4, 5] = False
    assert np.array_equal(_bits(on[keep]), _bits(off[keep]))       # its neighbours see a brighter neighbour: they are not above it
    assert _bits(on[4, 5, 3]) == _bits(off[4, 5, 3])                # v is kept
    # I * (lim / L), one IEEE division and three multiplications in float32, with dn_lum's association
    f = np.float32
    I = off[4, 5, :3]
    L = (f(0.2126) * I[0] + f(0.7152) * I[1]) + f(0.0722) * I[2]
    M = (f(0.2126) * f(0.25) + f(0.7152) * f(0.25)) + f(0.0722) * f(0.25)
    k = (f(threshold) * M) / L
    assert np.array_equal(_bits(on[4, 5, :3]), _bits(I * k))
    # and its luminance is threshold x the field's, to float32 rounding
    Lc = float(on[4, 5, :3].astype(np.float64) @ ds.LUM)
    assert abs(Lc - threshold * 0.25) <= 4e-7 * threshold


def test_grey_spike_becomes_exactly_threshold_times_the_field():
    """Powers of two everywhere: every operation is exact, so the clamped pixel is threshold x the field in every channel."""
    acc, a, n, m, N = flat_inputs(5, 5, value=0.25)
    acc[2, 2, :3] = 64.0
    on = ds.host_stage(acc, a, n, m, N, enabled=1, threshold=2.0)
    L = np.float32(0.2126) * np.float32(64) + np.float32(0.7152) * np.float32(64) + np.float32(0.0722) * np.float32(64)
    M = np.float32(0.2126) * np.float32(0.25) + np.float32(0.7152) * np.float32(0.25) + np.float32(0.0722) * np.float32(0.25)
    assert L == np.float32(256) * M     # (scaling by a power of two commutes with every rounding)
    assert np.array_equal(_bits(on[2, 2, :3]), _bits(np.full(3, 0.5, np.float32)))


def test_nan_pixel_keeps_its_value_and_is_never_a_neighbour():
    acc, a, n, m, N = flat_inputs(7, 7)
    acc[3, 3, :3] = np.nan
    acc[3, 4, :3] = 50.0        # a spike beside it: its limit comes from the field, not from the NaN
    on = ds.host_stage(acc, a, n, m, N, enabled=1, threshold=2.0)
    assert np.array_equal(_bits(on[3, 3]), _bits(np.array([0, 0, 0, -1], np.float32)))     # the prep's mark, copied
    assert np.isfinite(on).all()
    np.testing.assert_allclose(on[3, 4, :3], 0.5, rtol=1e-6)
    den = ds.host_filter(acc, a, n, m, N, enabled=1, threshold=2.0)
    assert np.isnan(den[3, 3, :3]).all()        # the filter returns the accumulator's value there
    rest = np.ones((7, 7), bool)
    rest[3, 3] = False
    assert np.isfinite(den[rest]).all()
    # a pixel whose every neighbour is NaN has no neighbour: copied
    acc2, a2, n2, m2, N2 = flat_inputs(3, 3)
    acc2[..., :3] = np.nan
    acc2[1, 1, :3] = 1000.0
    off2 = ds.host_stage(acc2, a2, n2, m2, N2, enabled=0)
    on2 = ds.host_stage(acc2, a2, n2, m2, N2, enabled=1, threshold=1.0)
    assert np.array_equal(_bits(on2), _bits(off2))


def test_geometry_pixel_ringed_by_background_is_copied():
    acc, a, n, m, N = flat_inputs(5, 5)
    n[..., 3] = 0.0             # background everywhere ...
    m[..., 0] = 0.0
    n[2, 2, 3] = 1.0            # ... but one geometry pixel, a thousand times brighter
    m[2, 2, 0] = 5.0
    acc[2, 2, :3] = 250.0
    off = ds.host_stage(acc, a, n, m, N, enabled=0)
    on = ds.host_stage(acc, a, n, m, N, enabled=1, threshold=1.0)
    assert np.array_equal(_bits(on), _bits(off))
    # the same pixel as background is clamped
    n[2, 2, 3] = 0.0
    m[2, 2, 0] = 0.0
    on = ds.host_stage(acc, a, n, m, N, enabled=1, threshold=1.0)
    np.testing.assert_allclose(on[2, 2, :3], 0.25, rtol=1e-6)


def test_one_pixel_image_is_copied():
    acc, a, n, m, N = flat_inputs(1, 1, value=1000.0)
    assert np.array_equal(_bits(ds.host_stage(acc, a, n, m, N, enabled=1, threshold=1.0)), _bits(ds.host_stage(acc, a, n, m, N, enabled=0)))
    for it in (0, 1, 5):
        assert np.array_equal(_bits(ds.host_filter(acc, a, n, m, N, iterations=it, enabled=1, threshold=1.0)),
                              _bits(dl.host_filter(acc, a, n, m, N, iterations=it)))


@pytest.mark.parametrize("H,W,iters,seed", [(7, 13, 1, 1), (33, 21, 5, 3), (19, 23, 0, 5), (41, 37, 7, 9)])
def test_disabled_gives_the_bits_of_dn_host_filter(H, W, iters, seed):
    acc, a, n, m, N, _ = spiky_inputs(seed, H, W)
    want = dl.host_filter(acc, a, n, m, N, iterations=iters)
    assert np.array_equal(_bits(ds.host_filter(acc, a, n, m, N, iterations=iters, enabled=0, threshold=2.0)), _bits(want))
    on = ds.host_filter(acc, a, n, m, N, iterations=iters, enabled=1, threshold=2.0)
    assert np.array_equal(_bits(on), _bits(want)) == (iters == 0)     # iterations 0: the accumulator either way


def test_region_and_counts_of_the_host_filter_are_those_of_the_crop():
    """The twin's rectangle is launch_denoise's: the rectangle filtered as an image of its own, zeros outside; its counts are per tile of the
    frame."""
    acc, a, n, m, N, _ = spiky_inputs(41, 29, 35)
    rect = (5, 3, 30, 27)
    x0, y0, x1, y1 = rect
    crop = lambda img: img[y0:y1, x0:x1]
    got = ds.host_filter(acc, a, n, m, N, enabled=1, rect=rect)
    want = ds.host_filter(crop(acc), crop(a), crop(n), crop(m), N, enabled=1)
    assert np.array_equal(_bits(crop(got)), _bits(want))
    outside = np.ones((29, 35), bool)
    outside[y0:y1, x0:x1] = False
    assert not got[outside].any()
    counts = np.full((29, 35), N, np.uint32)
    assert np.array_equal(_bits(ds.host_filter(acc, a, n, m, 1, enabled=1, rect=rect, counts=counts)), _bits(got))
    tiles = np.kron(np.arange(4 * 5, dtype=np.uint32).reshape(4, 5) % 7 + 1, np.ones((8, 8), np.uint32))[:29, :35]
    import adaptive_lib as al
    for en in (0, 1):
        full = ds.host_filter(acc, a, n, m, 1, enabled=en, counts=tiles)
        if en == 0:
            assert np.array_equal(_bits(full), _bits(al.host_filter_counts(acc, a, n, m, tiles)))
        else:
            assert not np.array_equal(_bits(full), _bits(al.host_filter_counts(acc, a, n, m, tiles)))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_despeckle_options_abi():
    layout = ds.options_layout()
    assert layout[0] == C.sizeof(abi.DespeckleOptions) == 8
    assert layout[1] == abi.DespeckleOptions.enabled.offset == 0 and layout[2] == abi.DespeckleOptions.threshold.offset == 4
    lib = abi.load_library()
    o = abi.DespeckleOptions(7, 7.0)
    lib.pt_default_despeckle_options(C.byref(o))
    assert (o.enabled, o.threshold) == (0, 2.0)
    # the options are checked before the renderer: a valid struct reaches the null-renderer test, an invalid one does not
    assert lib.pt_set_despeckle_options(None, C.byref(o)) == -1 and b"null renderer" in lib.pt_last_error()
    for t in (1.0, 1.5, 3.0e38):
        ok = abi.DespeckleOptions(1, t)
        assert lib.pt_set_despeckle_options(None, C.byref(ok)) == -1 and b"null renderer" in lib.pt_last_error(), t
    for t in (0.999, 0.0, -2.0, float("inf"), float("-inf"), float("nan")):
        for en in (0, 1):
            bad = abi.DespeckleOptions(en, t)
            assert lib.pt_set_despeckle_options(None, C.byref(bad)) == -1, t   # PT_ERR_INVALID_ARGUMENT
            assert b"threshold" in lib.pt_last_error(), t
    assert lib.pt_set_despeckle_options(None, None) == -1


def test_cpp_header_and_python_wrapper_have_the_accessors(tmp_path):
    tu = tmp_path / "despeckle_accessors.cpp"
    tu.write_text('#include "ptamd_renderer.hpp"\n'
                  "int main() {\n"
                  "  ptamd::renderer_pt::Renderer* r = nullptr;\n"
                  "  if (r) {\n"
                  "    pt_despeckle_options& d = r->despeckleOptions();\n"
                  "    d.enabled = 1;\n"
                  "    pt_despeckle_options o;\n"
                  "    pt_default_despeckle_options(&o);\n"
                  "    r->setDespeckleOptions(o);\n"
                  "  }\n"
                  "  static_assert(sizeof(pt_despeckle_options) == 8, \"pt_despeckle_options\");\n"
                  "  return 0;\n"
                  "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(tu)])
    from platinum_amd.renderer import Renderer
    for member in ("despeckleOptions", "setDespeckleOptions"):
        assert callable(getattr(Renderer, member)), member


# ---- quality -----------------------------------------------------------------------------------------------------------------------------------
def rel_mse(x, ref):
    x, ref = np.asarray(x, np.float64)[..., :3], np.asarray(ref, np.float64)[..., :3]
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


def test_clamp_on_cornell_against_the_1024spp_oracle():
    """Cornell (`bench` camera, 4 bounces) at 128x128: relMSE = mean((x - ref)^2 / (ref^2 + 1e-2)) over RGB against the oracle's 1024 spp, of
    the default filter with the clamp (threshold 2) over the filter alone.  At 1 spp the clamp at least halves it; at 4 / 16 / 64 spp it is
    neutral (<= 1.05).  Measured with this float32 host build: 0.1128 / 0.9220 / 0.9787 / 1.0029."""
    import oracle_lib
    sc = scenes.cornell_scene("bench")
    ref = oracle_lib.OracleScene(sc, make_params(128, 128, 1024, 4)).render(0, 1024, threads=oracle_lib.host_threads())
    hs = dl.HostScene(sc, make_params(128, 128, 64, 4))
    imgs, done, ratios = None, 0, {}
    for spp in (1, 4, 16, 64):
        imgs = hs.render(done, spp - done, n0=done, into=imgs)
        done = spp
        alone = rel_mse(ds.host_filter(*imgs, spp, enabled=0, **dl.DEFAULTS), ref)
        clamped = rel_mse(ds.host_filter(*imgs, spp, enabled=1, threshold=2.0, **dl.DEFAULTS), ref)
        ratios[spp] = clamped / alone
        print("cornell 128x128 %2d spp: relMSE filter alone %.6g, clamp + filter %.6g, ratio %.4f" % (spp, alone, clamped, ratios[spp]))
    assert ratios[1] <= 0.5, ratios
    for spp in (4, 16, 64):
        assert ratios[spp] <= 1.05, ratios
