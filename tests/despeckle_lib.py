"""Host side of the firefly-clamp tests (DESIGN.md §3a "Firefly clamp"): the ctypes wrapper of tests/emu/despeckle_emu.cpp (the host build of
pt_denoise.h dn_despeckle_pixel and of the filter with it, a library of its own built by tests/host_build.py) and a float64 numpy
restatement of the prep -> clamp stage.  TEST HARNESS, never imported by platinum_amd."""
import ctypes as C
import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import host_build  # noqa: E402

SRC = os.path.join(_ROOT, "tests", "emu", "despeckle_emu.cpp")
LIB = os.path.join(_ROOT, "tests", "_build", "libptamd_despeckle.so")
LUM = np.array([0.2126, 0.7152, 0.0722])


@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load(src=SRC, lib=LIB)
    L.ds_host_stage.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 4 + [C.c_float, C.c_void_p]
    L.ds_host_filter.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 4 + [C.c_float] * 3 + [C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
    L.ds_host_options_layout.argtypes = [C.POINTER(C.c_uint32 * 3)]
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def host_stage(acc, albedo, normal, moments, N, enabled=1, threshold=2.0):
    """prep -> clamp (pt_denoise.h) built for the host: (H, W, 4) float32 {I.rgb, v}, what the first a-trous step reads."""
    imgs = [_f32(x) for x in (acc, albedo, normal, moments)]
    H, W = imgs[0].shape[:2]
    out = np.zeros((H, W, 4), np.float32)
    lib().ds_host_stage(*[x.ctypes.data for x in imgs], W, H, N, enabled, threshold, out.ctypes.data)
    return out


def host_filter(acc, albedo, normal, moments, N, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0, enabled=1, threshold=2.0, rect=None,
                counts=None):
    """The whole filter as the device runs it, built for the host: (H, W, 4) float32 images of the frame in, the denoised frame out.
    rect = (x0, y0, x1, y1): filter that rectangle as an image of its own, zeros outside (a region render).  counts = (H, W) uint32
    per-pixel sample counts, each 8x8 tile of the frame uniform inside rect (an adaptive render); otherwise N everywhere."""
    imgs = [_f32(x) for x in (acc, albedo, normal, moments)]
    H, W = imgs[0].shape[:2]
    out = np.zeros((H, W, 4), np.float32)
    r = None if rect is None else (C.c_uint32 * 4)(*rect)
    tn = None
    if counts is not None:
        counts = np.asarray(counts, np.uint32)
        x0, y0, x1, y1 = (0, 0, W, H) if rect is None else rect
        ty, tx = (H + 7) // 8, (W + 7) // 8
        tn = np.zeros(ty * tx, np.uint32)
        for j in range(y0 // 8, (y1 - 1) // 8 + 1):
            for i in range(x0 // 8, (x1 - 1) // 8 + 1):
                v = np.unique(counts[max(y0, j * 8):min(y1, j * 8 + 8), max(x0, i * 8):min(x1, i * 8 + 8)])
                assert v.size == 1, (j, i, v)
                tn[j * tx + i] = v[0]
    lib().ds_host_filter(*[x.ctypes.data for x in imgs], W, H, N, iterations, sigma_l, sigma_n, sigma_z, out.ctypes.data, enabled, threshold,
                         None if r is None else C.addressof(r), None if tn is None else tn.ctypes.data)
    return out


def options_layout():
    o = (C.c_uint32 * 3)()
    lib().ds_host_options_layout(C.byref(o))
    return list(o)


# ---- float64 restatement of prep -> clamp (DESIGN.md §3 "Denoiser", §3a "Firefly clamp") ----------------------------------------------
def np_prep(acc, albedo, normal, moments, N):
    """(I (H, W, 3), v, valid, geo): demodulated colour, its variance, which pixels are taps, which are geometry."""
    acc, albedo, normal, moments = (np.asarray(x, np.float64) for x in (acc, albedo, normal, moments))
    c, a = acc[..., :3], albedo[..., :3]
    geo = normal[..., 3] >= 0.5
    with np.errstate(all="ignore"):
        I = c / np.maximum(a, 1e-3)
        la = np.maximum(a @ LUM, 1e-3)
        v = np.maximum(0.0, moments[..., 2] - moments[..., 1] ** 2) / (N * la * la)
        valid = np.isfinite(c).all(-1) & np.isfinite(I).all(-1) & np.isfinite(v)
    return np.where(valid[..., None], I, 0.0), np.where(valid, v, -1.0), valid, geo


def np_clamp(I, v, valid, geo, threshold):
    """The clamp on the prep's output.  Returns (col (H, W, 4) float64 = {I', v}, L, lim, used): lim = threshold * the largest luminance among
    the valid 3x3 neighbours of the pixel's class (nan where `used` is false: no such neighbour, or the pixel itself is not a tap)."""
    H, W = v.shape
    L = I @ LUM
    M = np.full((H, W), -np.inf)
    for cls in (True, False):    # per class: the largest of the 8 neighbours' luminances, -inf for a pixel that is no tap of the class
        Lc = np.pad(np.where(valid & (geo == cls), L, -np.inf), 1, constant_values=-np.inf)
        Mc = np.max([Lc[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)], axis=0)
        M = np.where(geo == cls, Mc, M)
    used = valid & np.isfinite(M)
    lim = np.where(used, threshold * np.where(used, M, 0.0), np.nan)
    with np.errstate(all="ignore"):
        hit = used & (L > lim) & (L > 0)
        k = np.where(hit, lim / np.where(hit, L, 1.0), 1.0)
    col = np.concatenate([I * k[..., None], v[..., None]], -1)
    return col, L, lim, used


def np_stage(acc, albedo, normal, moments, N, threshold=2.0):
    """prep -> clamp in float64: (col, L, lim, used) of np_clamp."""
    return np_clamp(*np_prep(acc, albedo, normal, moments, N), threshold)
