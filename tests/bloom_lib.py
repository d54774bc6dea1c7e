"""Host side of the bloom tests: the ctypes wrapper of tests/emu/bloom_emu.cpp (the host build of pt_bloom.h, a library
of its own built by tests/host_build.py), an independent numpy restatement of the whole pyramid (np.clip index arrays over whole levels,
parametrised by dtype: no code shared with the header) and the test cards.  TEST HARNESS, never imported by platinum_amd."""
import ctypes as C
import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import host_build  # noqa: E402
from platinum_amd import abi  # noqa: E402

SRC = os.path.join(_ROOT, "tests", "emu", "bloom_emu.cpp")
LIB = os.path.join(_ROOT, "tests", "_build", "libptamd_bloom.so")
f32 = np.float32

SIZES = [(1, 1), (2, 1), (1, 7), (3, 2), (16, 16), (17, 15), (33, 31), (67, 45), (256, 128)]   # (W, H)
OPTION_SETS = {
    "defaults": {},
    "soft-knee": dict(threshold=1.0, knee=0.5, scatter=0.6, levels=4),
    "hard-full": dict(threshold=0.5, knee=0.0, intensity=1.0, levels=12),
    "levels-1": dict(levels=1),
    "levels-2": dict(levels=2),
}
CARDS = ("loguniform", "constant", "impulse", "edge")

# How far a second float32 implementation of this arithmetic may lie from the first.  `measured` is the largest relative error (with a
# floor of 1e-3 in the denominator) of np_bloom in float32 against np_bloom in float64 over CARDS x SIZES x OPTION_SETS
# (measure_float32_error(); test_bloom_host.py re-measures it); `bound` is 4 x that, the margin the post-process reference uses for the
# same reason: the other implementation may round each operation the other way.
# The worst case is the impulse at 256 x 128 with intensity 1 and threshold 0.5: out = in + (B - b) cancels most of the impulse.
BOUNDS = {"measured": 2.2453e-6, "bound": 4 * 2.2453e-6}


@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load(src=SRC, lib=LIB)
    L.bl_host_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(abi.BloomPlan)]
    L.bl_host_norm.argtypes = [C.c_uint32, C.c_float]
    L.bl_host_norm.restype = C.c_float
    L.bl_host_options_valid.argtypes = [C.POINTER(abi.BloomOptions)]
    L.bl_host_options_valid.restype = C.c_uint32
    L.bl_host_bright.argtypes = [C.c_void_p, C.POINTER(abi.BloomOptions), C.c_void_p]
    L.bl_host_bloom.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(abi.BloomOptions), C.c_void_p, C.c_void_p]
    L.bl_host_layout.argtypes = [C.POINTER(C.c_uint32 * 14)]
    return L


def options(**fields):
    """pt_bloom_options with the defaults DESIGN.md §3e states, then `fields`."""
    o = abi.BloomOptions(0, 0.05, 0.0, 0.0, 1.0, 6)
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def host_plan(W, H, levels):
    p = abi.BloomPlan()
    lib().bl_host_plan(W, H, levels, C.byref(p))
    return p


def host_bloom(img, o=None, pyramid=False):
    """pt_bloom.h built for the host on an (H, W, 4) float32 image: the bloomed image, or (image, U_1..U_L as (total_texels, 4))."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    H, W = img.shape[:2]
    o = options() if o is None else o
    out = np.empty((H, W, 4), np.float32)
    pyr = np.zeros((host_plan(W, H, o.levels).total_texels, 4), np.float32) if pyramid else None
    lib().bl_host_bloom(img.ctypes.data, W, H, C.byref(o), out.ctypes.data, None if pyr is None or pyr.size == 0 else pyr.ctypes.data)
    return (out, pyr) if pyramid else out


def layout():
    o = (C.c_uint32 * 14)()
    lib().bl_host_layout(C.byref(o))
    return list(o)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------------
def np_levels(W, H, levels):
    """[(w, h)] of the levels 0..L."""
    out = [(W, H)]
    while len(out) - 1 < levels and out[-1] != (1, 1):
        w, h = out[-1]
        out.append(((w + 1) // 2, (h + 1) // 2))
    return out


def np_plan(W, H, levels):
    """(L, [(w, h)], [offset], total) by enumeration."""
    lv = np_levels(W, H, levels)
    L = len(lv) - 1
    offs, total = [0], 0
    for w, h in lv[1:]:
        offs.append(total)
        total += w * h
    return L, lv, offs, total


def np_bright(rgb, threshold, knee, dt):
    """(H, W, 3) of dtype dt -> the scattered light; the constants are the float32 ones in every dtype."""
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    Y = (dt(f32(0.2126)) * r + dt(f32(0.7152)) * g) + dt(f32(0.0722)) * b
    dead = ~(np.abs(Y) <= dt(f32(3.0e38))) | ~np.isfinite(rgb).all(axis=-1) | ~(Y > 0)
    Ys = np.where(dead, dt(1), Y)
    d = Ys - threshold
    s = np.minimum(np.maximum(d + knee, dt(0)), dt(2) * knee)
    soft = (s * s) / (dt(4) * knee + dt(f32(1e-6)))
    w = np.maximum(soft, d) / Ys
    out = np.minimum(np.maximum(np.where(np.isfinite(rgb), rgb, dt(0)), dt(0)) * w[..., None], dt(2.0 ** 64))
    return np.where(dead[..., None], dt(0), out)


def np_down(src, dt):
    h, w = src.shape[:2]
    dh, dw = (h + 1) // 2, (w + 1) // 2
    k = np.array([1, 3, 3, 1], dt) / dt(8)
    ys, xs = 2 * np.arange(dh) - 1, 2 * np.arange(dw) - 1
    acc = np.zeros((dh, dw, 3), dt)
    for j in range(4):
        rows = src[np.clip(ys + j, 0, h - 1)]
        for i in range(4):
            acc = acc + (k[j] * k[i]) * rows[:, np.clip(xs + i, 0, w - 1)]
    return acc


def _up_axis(n_fine, n_coarse, dt):
    x = np.arange(n_fine)
    c, even = x >> 1, (x & 1) == 0
    a = np.clip(np.where(even, c - 1, c), 0, n_coarse - 1)
    b = np.clip(np.where(even, c, c + 1), 0, n_coarse - 1)
    return a, b, np.where(even, dt(0.25), dt(0.75)).astype(dt), np.where(even, dt(0.75), dt(0.25)).astype(dt)


def np_up(coarse, fw, fh, dt):
    ch, cw = coarse.shape[:2]
    xa, xb, wxa, wxb = _up_axis(fw, cw, dt)
    ya, yb, wya, wyb = _up_axis(fh, ch, dt)
    ra, rb = coarse[ya], coarse[yb]
    W = lambda wy, wx: (wy[:, None] * wx[None, :])[..., None]
    return ((W(wya, wxa) * ra[:, xa] + W(wya, wxb) * ra[:, xb]) + W(wyb, wxa) * rb[:, xa]) + W(wyb, wxb) * rb[:, xb]


def np_bloom(img, o, dtype=np.float64, pyramid=False):
    """The whole arithmetic of DESIGN.md §3e in `dtype` on an (H, W, 4) image; the options are the struct's float32 values."""
    dt = np.dtype(dtype).type
    a = np.asarray(img, np.float32).astype(dt)
    H, W = a.shape[:2]
    intensity, threshold, knee, scatter = (dt(f32(v)) for v in (o.intensity, o.threshold, o.knee, o.scatter))
    lv = np_levels(W, H, o.levels)
    L = len(lv) - 1
    if L == 0:
        return (a.copy(), []) if pyramid else a.copy()
    with np.errstate(all="ignore"):
        rgb = a[..., :3]
        b = np_bright(rgb, threshold, knee, dt)
        D = [b]
        for _ in range(L):
            D.append(np_down(D[-1], dt))
        U = [None] * (L + 1)
        U[L] = D[L]
        for l in range(L - 1, 0, -1):
            U[l] = D[l] + scatter * np_up(U[l + 1], lv[l][0], lv[l][1], dt)
        norm, p = dt(0), dt(1)
        for _ in range(L):
            norm = norm + p
            p = p * scatter
        B = np_up(U[1], W, H, dt) / norm
        out = a.copy()
        out[..., :3] = np.where(np.isfinite(rgb), rgb + intensity * (B - b), rgb)
    return (out, U[1:]) if pyramid else out


def np_pyramid_flat(U):
    """U_1..U_L as (total_texels, 3), in the plan's order."""
    return np.concatenate([u.reshape(-1, 3) for u in U]) if U else np.zeros((0, 3))


def rel_err(x, ref):
    """max |x - ref| / max(|ref|, 1e-3) over the finite entries of ref; the others must match in kind"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(x), np.isnan(ref)) and np.array_equal(np.isinf(x), np.isinf(ref))
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(x[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-3)))


# ---- the cards -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _card(name, W, H):
    rng = np.random.default_rng(1000 * W + H)
    img = np.zeros((H, W, 4), np.float32)
    img[..., 3] = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)   # alpha is copied, whatever it holds
    if name in ("loguniform", "nonfinite"):
        img[..., :3] = np.exp2(rng.uniform(-8.0, 6.0, (H, W, 3))).astype(np.float32)
        if name == "nonfinite":   # one NaN pixel and one +inf pixel, apart from each other where the image has room
            p = img.reshape(-1, 4)
            p[(W * H) // 3, :3] = np.float32("nan")
            p[nonfinite_pixels(W, H)[1], :3] = np.float32("inf")
    elif name == "constant":
        img[..., :3] = np.array([0.7, 1.3, 0.4], np.float32)
    elif name == "impulse":
        img[H // 2, W // 2, :3] = np.array([50.0, 20.0, 5.0], np.float32)
    elif name == "edge":
        img[..., :3] = 0.05
        img[:, W // 2:, :3] = np.array([4.0, 3.0, 5.0], np.float32)
    else:
        raise KeyError(name)
    img.setflags(write=False)
    return img


def card(name, W, H):
    """A read-only (H, W, 4) float32 test card, computed once."""
    return _card(name, W, H)


def nonfinite_pixels(W, H):
    """Flat indices of the NaN pixel and the +inf pixel of card("nonfinite", W, H) (the same pixel, +inf, in a 1 x 1 image)."""
    return (W * H) // 3, ((2 * W * H) // 3 if W * H >= 3 else W * H - 1)


def measure_float32_error():
    """BOUNDS["measured"]: np_bloom in float32 against itself in float64 over the cards, sizes and option sets of the host test."""
    worst = 0.0
    for name in CARDS:
        for W, H in SIZES:
            for f in OPTION_SETS.values():
                o = options(**f)
                worst = max(worst, rel_err(np_bloom(card(name, W, H), o, np.float32)[..., :3], np_bloom(card(name, W, H), o, np.float64)[..., :3]))
    return worst
