"""Host side of the film tests: a float32 numpy restatement of the per-sample fold, of both compose modes and of the alpha
byte; the independent reference of the GPU tests, the oracle's debug_sample(s) masked by trace_primary(s)["instance"] >= 0 and folded by
that restatement; and the ctypes wrapper of tests/emu/film_emu.cpp (the host build of platinum_amd/csrc/pt_film.h, a library of its own).
TEST HARNESS, never imported by platinum_amd."""
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

SRC = os.path.join(_ROOT, "tests", "emu", "film_emu.cpp")
LIB = os.path.join(_ROOT, "tests", "_build", "libptamd_film.so")
f32 = np.float32
KEEP, ZERO = 0, 1                       # pt_render_params.nonfinite_policy
SCENE, COLOR, TRANSPARENT = abi.BACKDROP_SCENE, abi.BACKDROP_COLOR, abi.BACKDROP_TRANSPARENT


def options(**fields):
    o = abi.FilmOptions()
    for k, v in fields.items():
        setattr(o, k, (C.c_float * 3)(*v) if k == "backdrop_rgb" else v)
    return o


# ---- the rule, restated in float32 numpy (every numpy float32 operation is one IEEE operation) -----------------------------------------------
def np_sample(L, hit, policy):
    """x_s: L (..., 3 or 4) float32 radiance, hit (...) bool -> (..., 4)."""
    L = np.asarray(L, f32)[..., :3]
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(L) <= f32(3.0e38)).all(axis=-1)          # the product's non-finite test (NaN compares false)
    if policy == ZERO:
        L = np.where(bad[..., None], f32(0), L)
    x = np.concatenate([L, np.ones(L.shape[:-1] + (1,), f32)], axis=-1)
    return np.where(np.asarray(hit, bool)[..., None], x, f32(0)).astype(f32)      # a select: a missed NaN is 0


def np_fold(L, hit, policy=KEEP, n0=0, film=None, counts=None):
    """The film after folding samples L[s], hit[s] (sample-major: (ns, ..., 3|4) and (ns, ...)) in order onto `film`, the mean of n0
    samples.  counts (...): each pixel folds its first counts[...] samples only (an adaptive render)."""
    L = np.asarray(L, f32)
    ns = L.shape[0]
    film = np.zeros(L.shape[1:-1] + (4,), f32) if film is None else np.array(film, f32)
    for s in range(ns):
        n = n0 + s
        x = np_sample(L[s], hit[s], policy)
        with np.errstate(all="ignore"):
            nxt = x if n == 0 else ((x + film * f32(n)) / f32(n + 1)).astype(f32)
        film = nxt if counts is None else np.where((np.asarray(counts) > s)[..., None], nxt, film)
    return film


def np_compose(base, alpha, backdrop, rgb=(0.0, 0.0, 0.0), rect=None):
    """The display chain's source: base (H, W, 3|4), alpha (H, W); 0 outside rect = (x0, y0, x1, y1).  (H, W, 4)."""
    base = np.asarray(base, f32)[..., :3]
    a = np.asarray(alpha, f32)
    H, W = a.shape
    with np.errstate(all="ignore"):
        if backdrop == COLOR:
            k = (f32(1) - a).astype(f32)
            rgb_out = (base + (np.asarray(rgb, f32) * k[..., None]).astype(f32)).astype(f32)
            w = np.ones_like(a)
        else:
            assert backdrop == TRANSPARENT
            pos = a > 0
            rgb_out = np.where(pos[..., None], (base / np.where(pos, a, f32(1))[..., None]).astype(f32), f32(0))
            w = a
    out = np.concatenate([rgb_out, w[..., None]], axis=-1).astype(f32)
    if rect is not None:
        inside = np.zeros((H, W), bool)
        inside[rect[1]:rect[3], rect[0]:rect[2]] = True
        out = np.where(inside[..., None], out, f32(0))
    return out


def np_quantise(v):
    """pp_pack_rgba8's quantiser: <= 0 or NaN -> 0, >= 1 -> 255, else (uint32)(v * 255 + 0.5) in float32."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        mid = (v * f32(255) + f32(0.5)).astype(f32)
        return np.where(~(v > 0), 0, np.where(v >= 1, 255, np.where(v > 0, mid, 0).astype(np.uint32))).astype(np.uint8)


# ---- the reference: the oracle, sample by sample ------------------------------------------------------------------------------------------
def reference_samples(scene, size, spp, bounces=4):
    """(L (spp, H, W, 4) float32, hit (spp, H, W) bool), read only: the oracle's debug_sample(s) and trace_primary(s)["instance"] >= 0."""
    import oracle_lib
    from platinum_amd.renderer import make_params
    W, H = size
    o = oracle_lib.OracleScene(scene, make_params(W, H, spp, bounces))
    L = np.empty((spp, H, W, 4), f32)
    hit = np.empty((spp, H, W), bool)
    try:
        for s in range(spp):
            L[s] = o.debug_sample(s)[0]
            hit[s] = o.trace_primary(s)["instance"] >= 0
    finally:
        o.close()
    L.flags.writeable = False
    hit.flags.writeable = False
    return L, hit


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


def first_difference(a, b):
    bad = np.argwhere(np.ascontiguousarray(a, f32).view(np.uint32) != np.ascontiguousarray(b, f32).view(np.uint32))
    return "%d values differ, the first at %s: %r against %r" % (len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]) if len(bad) else "equal"


# ---- the host build of pt_film.h -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load(src=SRC, lib=LIB)
    L.film_host_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    L.film_host_compose.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(abi.FilmOptions), C.c_void_p]
    L.film_host_alpha.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.film_host_options_valid.argtypes = [C.POINTER(abi.FilmOptions)]
    L.film_host_options_valid.restype = C.c_uint32
    L.film_host_layout.argtypes = [C.POINTER(C.c_uint32 * 4)]
    return L


def host_fold(L, hit, policy=KEEP, n0=0, film=None):
    """film_fold(film_sample(...)) over sample-major L (ns, ..., 4) and hit (ns, ...), onto `film`: the same shapes as np_fold."""
    L = np.asarray(L, f32)
    ns, shape = L.shape[0], L.shape[1:-1]
    npix = int(np.prod(shape, dtype=np.int64))
    Lp = np.ascontiguousarray(np.moveaxis(L.reshape(ns, npix, 4), 0, 1))                                  # [pixel][sample][4]
    Fp = np.ascontiguousarray(np.moveaxis(np.asarray(hit).reshape(ns, npix), 0, 1).astype(np.uint32))     # [pixel][sample]
    out = np.zeros((npix, 4), f32) if film is None else np.array(film, f32).reshape(npix, 4)
    lib().film_host_fold(out.ctypes.data, Lp.ctypes.data, Fp.ctypes.data, npix, ns, n0, policy)
    return out.reshape(shape + (4,))


def host_compose(base, film, o, rect=None):
    base = np.ascontiguousarray(base, f32)
    film = np.ascontiguousarray(film, f32)
    H, W = film.shape[:2]
    assert base.shape == film.shape == (H, W, 4)
    r = (C.c_uint32 * 4)(*(rect if rect is not None else (0, 0, W, H)))
    out = np.empty((H, W, 4), f32)
    lib().film_host_compose(base.ctypes.data, film.ctypes.data, W, H, C.addressof(r), C.byref(o), out.ctypes.data)
    return out


def host_alpha(rgba8, composed):
    """(H, W, 4) uint8 target with its alpha bytes replaced by the quantised .w of the composed source."""
    t = np.ascontiguousarray(rgba8, np.uint8)
    c = np.ascontiguousarray(composed, f32)
    out = np.empty_like(t)
    lib().film_host_alpha(t.ctypes.data, c.ctypes.data, t.shape[0] * t.shape[1], out.ctypes.data)
    return out


def layout():
    o = (C.c_uint32 * 4)()
    lib().film_host_layout(C.byref(o))
    return list(o)
