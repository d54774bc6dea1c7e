"""Host side of the adaptive-sampling tests: the ctypes loader of tests/_build/libadaptive_emu.so (the host build of
platinum_amd/csrc/pt_adaptive.h and of the denoiser's per-pixel-N prep, tests/emu/adaptive_emu.cpp) and a float64 numpy restatement of
the criterion as DESIGN.md §3b states it.  TEST HARNESS, never imported by platinum_amd."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

SRC = os.path.join(_ROOT, "tests", "emu", "adaptive_emu.cpp")
LIB = os.path.join(_ROOT, "tests", "_build", "libadaptive_emu.so")
LUM_FLOOR = 1e-3
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    csrc = os.path.join(_ROOT, "platinum_amd", "csrc")
    emu = os.path.join(_ROOT, "tests", "emu")
    deps = [os.path.join(emu, f) for f in os.listdir(emu)] + [os.path.join(_ROOT, "include", "ptamd.h")]
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        tmp = LIB + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-shared", "-o", tmp, SRC])
        os.replace(tmp, LIB)
    L = C.CDLL(LIB)
    L.ad_host_error.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
    L.ad_host_tiles.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
    L.ad_host_filter_counts.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 2 + [C.c_void_p, C.c_uint32] + [C.c_float] * 3 + [C.c_void_p]
    L.ad_host_options_layout.argtypes = [C.POINTER(C.c_uint32 * 5)]
    _lib = L
    return L


def host_error(m1, m2, n):
    m1, m2 = np.ascontiguousarray(m1, np.float32), np.ascontiguousarray(m2, np.float32)
    err = np.zeros(m1.shape, np.float32)
    lib().ad_host_error(m1.ctypes.data, m2.ctypes.data, m1.size, n, err.ctypes.data)
    return err


def host_tiles(moments, n, threshold):
    """(tilesY, tilesX) bool: the tiles of a (H, W, 4) PT_AOV_MOMENTS image that converge after n samples."""
    moments = np.ascontiguousarray(moments, np.float32)
    H, W = moments.shape[:2]
    out = np.zeros(((H + 7) // 8, (W + 7) // 8), np.uint8)
    lib().ad_host_tiles(moments.ctypes.data, W, H, n, threshold, out.ctypes.data)
    return out.astype(bool)


def host_filter_counts(acc, albedo, normal, moments, counts, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0):
    """The denoiser of an adaptive render (per-pixel N = counts, (H, W) uint32) built for the host."""
    imgs = [np.ascontiguousarray(x, np.float32) for x in (acc, albedo, normal, moments)]
    counts = np.ascontiguousarray(counts, np.uint32)
    H, W = imgs[0].shape[:2]
    out = np.zeros((H, W, 4), np.float32)
    lib().ad_host_filter_counts(*[x.ctypes.data for x in imgs], W, H, counts.ctypes.data, iterations, sigma_l, sigma_n, sigma_z, out.ctypes.data)
    return out


def options_layout():
    o = (C.c_uint32 * 5)()
    lib().ad_host_options_layout(C.byref(o))
    return list(o)


# ---- float64 restatement ----------------------------------------------------------------------------------------------
def np_error(m1, m2, n):
    m1, m2 = np.asarray(m1, np.float64), np.asarray(m2, np.float64)
    with np.errstate(all="ignore"):
        var = np.maximum(m2 - m1 * m1, 0.0) * n / (n - 1)
        return np.sqrt(var / n) / np.maximum(m1, LUM_FLOOR)


def np_converged(m1, m2, n, threshold):
    if n < 2:
        return np.zeros(np.shape(m1), bool)
    with np.errstate(invalid="ignore"):
        return np_error(m1, m2, n) <= threshold


def tile_view(img, H, W):
    """(tilesY, tilesX) list of the tiles' slices of an (H, W, ...) image."""
    return [[(slice(ty * 8, min(H, ty * 8 + 8)), slice(tx * 8, min(W, tx * 8 + 8))) for tx in range((W + 7) // 8)] for ty in range((H + 7) // 8)]
