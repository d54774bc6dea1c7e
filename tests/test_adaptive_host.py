"""CPU: the tile-adaptive sampling criterion (platinum_amd/csrc/pt_adaptive.h, built for the host by tests/emu/adaptive_emu.cpp) against a
float64 restatement of DESIGN.md §3b, its edge cases, the denoiser's per-pixel-N prep, and the pt_adaptive_options ABI.  (The adaptive
kernels' resource budgets: tests/test_kernel_resources.py.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
import denoise_lib as dl  # noqa: E402
from test_denoise_host import random_inputs  # noqa: E402
from platinum_amd import abi  # noqa: E402


@pytest.mark.parametrize("n,seed", [(2, 0), (3, 1), (16, 2), (33, 3), (256, 4), (4096, 5)])
def test_criterion_matches_float64_restatement(n, seed):
    rng = np.random.default_rng(seed)
    m1 = np.concatenate([rng.uniform(0.0, 3.0, 4000), rng.uniform(0.0, 2e-3, 500), np.zeros(50)]).astype(np.float32)
    m2 = (m1.astype(np.float64) ** 2 + rng.uniform(0.0, 2.0, m1.size) * rng.choice([0.0, 1e-6, 1e-2, 1.0], m1.size)).astype(np.float32)
    m2[:100] = (m1[:100].astype(np.float64) ** 2 * 0.999).astype(np.float32)   # rounding leaves m2 < m1^2: the variance clamps to 0
    got = al.host_error(m1, m2, n)
    want = al.np_error(m1, m2, n)
    # m2 - m1^2 cancels in fp32: compare where the difference keeps at least 10 bits, and where it clamps to 0
    d = m2.astype(np.float64) - m1.astype(np.float64) ** 2
    ok = (d > 1e-3 * m2) | (d < -1e-3 * m2)
    assert ok.sum() > 2000 and (d < -1e-3 * m2).sum() >= 100
    np.testing.assert_allclose(got[ok], want[ok], rtol=2e-4, atol=0)
    for thr in (0.005, 0.02, 0.1):
        far = ok & (np.abs(want - thr) > 1e-3 * thr)
        assert np.array_equal((got <= thr)[far], al.np_converged(m1, m2, n, thr)[far])


def _moments(H, W, m1, m2):
    m = np.zeros((H, W, 4), np.float32)
    m[..., 1], m[..., 2] = m1, m2
    return m


def test_all_black_tile_converges():
    assert al.host_tiles(_moments(8, 8, 0.0, 0.0), 2, 1e-6).all()
    assert al.host_error(np.zeros(1), np.zeros(1), 32)[0] == 0.0


def test_nan_pixel_keeps_its_tile_active():
    m = _moments(16, 16, 0.5, 0.25)           # zero variance: every tile converges
    assert al.host_tiles(m, 32, 0.02).all()
    for field in (1, 2):
        mm = m.copy()
        mm[9, 3, field] = np.nan                 # tile (1, 0)
        got = al.host_tiles(mm, 32, 0.02)
        assert not got[1, 0] and got.sum() == 3, field
        assert np.isnan(al.host_error(mm[9, 3, 1:2], mm[9, 3, 2:3], 32)[0])


def test_pixels_outside_the_image_are_ignored():
    H, W = 13, 19                              # edge tiles hold 5 rows / 3 columns of image pixels
    m = _moments(H, W, 0.5, 0.25)
    got = al.host_tiles(m, 32, 0.02)
    assert got.shape == (2, 3) and got.all()
    m[12, 18, 2] = 10.0                        # the one image pixel of the corner tile's last row and column: now noisy
    got = al.host_tiles(m, 32, 0.02)
    assert not got[1, 2] and got.sum() == 5


def test_fewer_than_two_samples_never_converge():
    m = _moments(8, 8, 0.0, 0.0)
    for n in (0, 1):
        assert not al.host_tiles(m, n, 1e30).any(), n
    assert al.host_tiles(m, 2, 1e-30).all()


def test_relative_error_is_the_standard_error_of_the_mean():
    # 0/1 samples with mean p: var = p (1 - p) n / (n - 1), err = sqrt(var / n) / p
    n, p = 64, 0.25
    err = al.host_error(np.float32([p]), np.float32([p]), n)[0]
    assert abs(err - np.sqrt(p * (1 - p) / (n - 1)) / p) < 1e-6


@pytest.mark.parametrize("H,W,seed", [(17, 23, 0), (24, 40, 1), (9, 8, 2)])
def test_filter_with_per_pixel_counts(H, W, seed):
    rng = np.random.default_rng(seed)
    acc, a, n, m, _ = random_inputs(rng, H, W)
    tiles = rng.integers(2, 300, ((H + 7) // 8, (W + 7) // 8)).astype(np.uint32)
    counts = np.kron(tiles, np.ones((8, 8), np.uint32))[:H, :W].copy()
    got = al.host_filter_counts(acc, a, n, m, counts)
    np.testing.assert_allclose(got, dl.np_filter(acc, a, n, m, counts.astype(np.float64)), rtol=1e-4, atol=1e-6)
    # uniform counts: the filter of a non-adaptive render, bit for bit
    uni = np.full((H, W), 37, np.uint32)
    assert np.array_equal(al.host_filter_counts(acc, a, n, m, uni).view(np.uint32), dl.host_filter(acc, a, n, m, 37).view(np.uint32))


def test_adaptive_options_abi():
    layout = al.options_layout()
    assert layout[0] == C.sizeof(abi.AdaptiveOptions) == 16
    for name, off in zip(("enabled", "threshold", "min_spp", "interval"), layout[1:]):
        assert getattr(abi.AdaptiveOptions, name).offset == off, name
    lib = abi.load_library()
    o = abi.AdaptiveOptions(7, 7.0, 7, 7)
    lib.pt_default_adaptive_options(C.byref(o))
    assert (o.enabled, o.threshold, o.min_spp, o.interval) == (0, np.float32(0.02), 32, 32)
    assert abi.PT_ABI_VERSION == 5
    # validation runs before the renderer is looked at: with a null renderer, valid options get as far as "null renderer"
    assert lib.pt_set_adaptive_options(None, C.byref(o)) == -1 and b"null renderer" in lib.pt_last_error()
    for field, value, word in (("threshold", 0.0, b"threshold"), ("threshold", -1.0, b"threshold"), ("threshold", float("inf"), b"threshold"),
                               ("threshold", float("nan"), b"threshold"), ("min_spp", 1, b"min_spp"), ("min_spp", 0, b"min_spp"),
                               ("interval", 0, b"interval")):
        bad = abi.AdaptiveOptions(1, 0.02, 32, 32)
        setattr(bad, field, value)
        assert lib.pt_set_adaptive_options(None, C.byref(bad)) == -1, field
        assert word in lib.pt_last_error(), (field, lib.pt_last_error())
