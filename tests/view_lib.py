"""Host side of the pass-view tests: a float32 numpy restatement of every data view, written operation by operation (the
independent reference of the host and GPU tests); the crafted cards both run on; and the ctypes wrapper of tests/emu/view_emu.cpp (the
host build of platinum_amd/csrc/pt_view.h, a library of its own).  TEST HARNESS, never imported by platinum_amd."""
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

SRC = os.path.join(_ROOT, "tests", "emu", "view_emu.cpp")
LIB = os.path.join(_ROOT, "tests", "_build", "libptamd_view.so")
f32 = np.float32
u32 = np.uint32
FLT_MAX = f32(3.4028234663852886e38)
SLOT = np.dtype(abi.MATTE_SLOT_DTYPE)
DATA_VIEWS = (abi.VIEW_NORMAL, abi.VIEW_DEPTH, abi.VIEW_ALPHA, abi.VIEW_MATTE, abi.VIEW_SAMPLES, abi.VIEW_NOISE)
RAMPS = (abi.RAMP_GREY, abi.RAMP_HEAT)
HEAT_STOPS = np.array([[0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 1, 0], [1, 0, 0]], f32)     # blue, cyan, green, yellow, red
LUM_FLOOR = f32(1e-3)                                                                  # pt_adaptive.h kAdaptiveLumFloor


def options(**fields):
    o = abi.ViewOptions()
    abi.load_library().pt_default_view_options(C.byref(o))
    for k, v in fields.items():
        setattr(o, k, v)
    return o


# ---- the rule, restated in float32 numpy (every numpy float32 operation is one IEEE operation) -----------------------------------------------
def np_quantise(v):
    """pp_pack_rgba8's quantiser: <= 0 or NaN -> 0, >= 1 -> 255, else (uint32)(v * 255 + 0.5) in float32."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        mid = (v * f32(255) + f32(0.5)).astype(f32)
        return np.where(~(v > 0), 0, np.where(v >= 1, 255, np.where(v > 0, mid, 0).astype(u32))).astype(np.uint8)


def np_ramp(v, ramp):
    """(...) float32 in [0, 1] or NaN -> (..., 3)."""
    v = np.asarray(v, f32)
    v = np.where(np.isnan(v), f32(1), v).astype(f32)
    if ramp == abi.RAMP_GREY:
        return np.stack([v, v, v], -1)
    s = (v * f32(4)).astype(f32)
    k = np.minimum(s.astype(np.int32), 3)
    f = (s - k.astype(f32)).astype(f32)
    a, b = HEAT_STOPS[k], HEAT_STOPS[k + 1]
    return (a + ((b - a).astype(f32) * f[..., None]).astype(f32)).astype(f32)


def py_hash(x):
    """The id hash in Python integers."""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def np_id_colour(ids):
    """(...) uint32 -> (..., 3): MATTE_NONE is black, every other id a colour in [0.25, 1]."""
    ids = np.asarray(ids, u32)
    x = ids.astype(np.uint64)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    byte = np.stack([(x >> np.uint64(8 * c)) & np.uint64(255) for c in range(3)], -1).astype(f32)
    col = (((byte / f32(255)).astype(f32) * f32(0.75)).astype(f32) + f32(0.25)).astype(f32)
    return np.where((ids == abi.MATTE_NONE)[..., None], f32(0), col).astype(f32)


def np_depth(inp):
    """(d, valid): d = r / h where the pixel is valid (n > 0, h > 0, d finite and >= 0)."""
    h = np.asarray(inp["normal"], f32)[..., 3]
    r = np.asarray(inp["moments"], f32)[..., 0]
    with np.errstate(all="ignore"):
        d = (r / h).astype(f32)
        valid = (np.asarray(inp["counts"]) > 0) & (h > 0) & (d >= 0) & (d <= FLT_MAX)
    return d, valid


def np_range(inp, o, rect=None):
    """(z0, z1, depth_pixels) as the depth view uses them: the min and max of the valid depths of `rect` = (x0, y0, x1, y1), or the options'."""
    d, valid = np_depth(inp)
    if rect is not None:
        inside = np.zeros(valid.shape, bool)
        inside[rect[1]:rect[3], rect[0]:rect[2]] = True
        valid = valid & inside
    n = int(valid.sum())
    if not o.auto_range:
        return f32(o.depth_min), f32(o.depth_max), n
    if n == 0:
        return f32(0), f32(0), 0
    dv = np.abs(d[valid])                  # (-0 is a valid depth, and counts as 0)
    return f32(dv.min()), f32(dv.max()), n


def np_adaptive_error(m1, m2, n):
    """pt_adaptive.h adaptive_error, operation by operation; both selects keep a NaN."""
    with np.errstate(all="ignore"):
        nf = np.asarray(n).astype(f32)
        d = (m2 - (m1 * m1).astype(f32)).astype(f32)
        var = (np.where(d < 0, f32(0), d).astype(f32) * (nf / (nf - f32(1))).astype(f32)).astype(f32)
        den = np.where(m1 < LUM_FLOOR, LUM_FLOOR, m1).astype(f32)
        return (np.sqrt((var / nf).astype(f32)).astype(f32) / den).astype(f32)


def np_view(inp, o, rect=None):
    """One data view of the inputs `inp` (a dict: counts (H, W); normal, moments, film (H, W, 4); slots (H, W, 8) of one layer; spp):
    ((H, W, 4) uint8, (shown, depth_pixels, z0, z1))."""
    n = np.asarray(inp["counts"], u32)
    H, W = n.shape
    view = o.view
    stats = (view, 0, f32(0), f32(0))
    with np.errstate(all="ignore"):
        nf = n.astype(f32)
        if view == abi.VIEW_NORMAL:
            N = np.asarray(inp["normal"], f32)[..., :3]
            c = ((N * f32(0.5)).astype(f32) + f32(0.5)).astype(f32)
        elif view == abi.VIEW_DEPTH:
            z0, z1, count = np_range(inp, o, rect)
            stats = (view, count, z0, z1)
            d, valid = np_depth(inp)
            t = ((d - z0).astype(f32) / (z1 - z0)).astype(f32) if z1 > z0 else np.zeros_like(d)
            t = np.where(t < 0, f32(0), t)
            t = np.where(t > 1, f32(1), t).astype(f32)
            c = np.where(valid[..., None], np_ramp((f32(1) - t).astype(f32), o.ramp), f32(0))
        elif view == abi.VIEW_ALPHA:
            c = np_ramp(np.asarray(inp["film"], f32)[..., 3], abi.RAMP_GREY)
        elif view == abi.VIEW_MATTE:
            s = np.asarray(inp["slots"])
            c = np.zeros((H, W, 3), f32)
            for k in range(abi.MATTE_SLOTS):
                cnt = s["count"][..., k]
                w = (cnt.astype(f32) / nf).astype(f32)
                term = (w[..., None] * np_id_colour(s["id"][..., k])).astype(f32)
                c = np.where((cnt != 0)[..., None], (c + term).astype(f32), c)
        elif view == abi.VIEW_SAMPLES:
            v = (nf / f32(inp["spp"])).astype(f32)
            c = np_ramp(np.where(v < 1, v, f32(1)), o.ramp)
        elif view == abi.VIEW_NOISE:
            M = np.asarray(inp["moments"], f32)
            err = np_adaptive_error(M[..., 1], M[..., 2], n)
            v = (err / f32(o.noise_max)).astype(f32)
            v = np.where(v < 1, v, f32(1))
            v = np.where((n < 2) | np.isnan(err), f32(1), v)
            c = np_ramp(v, o.ramp)
        else:
            raise ValueError("not a data view: %r" % view)
    rgb = np.where((n == 0)[..., None], np.uint8(0), np_quantise(c))
    return np.concatenate([rgb, np.full((H, W, 1), 255, np.uint8)], -1).astype(np.uint8), stats


def stats_tuple(s):
    """abi.ViewStats -> what np_view returns beside the image."""
    return (s.shown, s.depth_pixels, f32(s.depth_min), f32(s.depth_max))


def same_stats(a, b):
    return a[:2] == b[:2] and f32(a[2]).tobytes() == f32(b[2]).tobytes() and f32(a[3]).tobytes() == f32(b[3]).tobytes()


# ---- the crafted cards -------------------------------------------------------------------------------------------------------------------------
SPP = 64
SIZES = [(1, 1), (17, 9), (33, 31)]
KINDS = ["mixed", "one_depth", "no_depth"]
MANUAL_RANGE = (1.0, 5.0)      # under it the card's depths 1, 2, 3, 4, 5 fall on the ramp's stops exactly
NAN, INF = float("nan"), float("inf")


@functools.lru_cache(maxsize=None)
def card(size, kind="mixed", first=0):
    """The inputs of one card, read only.  Random pixels (depths in [1, 5], fractional hit fractions, 1 .. 8 slots) with the special pixels
    written over the first ones, starting with special number `first` (a 1 x 1 card holds that one alone):
    n in {0, 1, 2, many}; NaN, infinite, negative and -0 depths; h = 0 and NaN; the depths 1 .. 5 (the ramp's stops under MANUAL_RANGE and
    under the card's own range); n / spp at the stops and past 1; moments with err = 0, 1/4, 1/2, 3/4, 1 exactly (n = 2, m1 = 1), NaN and
    negative moments; alpha at 0, 1, between, outside and NaN; eight full slots whose counts sum to less than n, MATTE_NONE slots, empty slots.
    one_depth: exactly one pixel has a valid depth; no_depth: none."""
    W, H = size
    npix = W * H
    rng = np.random.default_rng(1000 * W + H)
    normal = np.empty((npix, 4), f32)
    v = rng.normal(size=(npix, 3))
    normal[:, :3] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    normal[:, 3] = rng.choice(np.array([1.0, 0.5, 0.75, 1.0 / 3.0], f32), npix)
    depth = rng.uniform(1.0, 5.0, npix).astype(f32)
    moments = np.empty((npix, 4), f32)
    moments[:, 0] = (depth * normal[:, 3]).astype(f32)
    moments[:, 1] = rng.gamma(2.0, 0.5, npix).astype(f32)
    moments[:, 2] = (moments[:, 1] ** 2 * rng.uniform(0.98, 1.6, npix)).astype(f32)     # now and then m2 < m1^2: the variance clamps to 0
    moments[:, 3] = 0
    film = rng.random((npix, 4)).astype(f32)
    counts = rng.choice(np.array([1, 2, 3, 16, 37, 64], u32), npix).astype(u32)
    slots = np.zeros((npix, abi.MATTE_SLOTS), SLOT)
    slots["id"] = abi.MATTE_NONE
    for p in range(npix):
        k = int(rng.integers(1, min(int(counts[p]), abi.MATTE_SLOTS) + 1))
        share = rng.multinomial(int(counts[p]) - k, np.ones(k) / k) + 1               # k slots, every count >= 1, summing to n
        slots["id"][p, :k] = rng.integers(0, 40, k, dtype=u32) * 7919 + np.arange(k, dtype=u32)
        slots["count"][p, :k] = share
        if rng.random() < 0.2:
            slots["id"][p, int(rng.integers(0, k))] = abi.MATTE_NONE                  # a camera ray that missed takes a slot like any id

    def special(i, n=None, r=None, h=None, N=None, m1=None, m2=None, a=None, sl=None):
        if i >= npix:
            return
        if n is not None: counts[i] = n
        if h is not None: normal[i, 3] = h
        if N is not None: normal[i, :3] = N
        if r is not None: moments[i, 0] = r
        if m1 is not None: moments[i, 1] = m1
        if m2 is not None: moments[i, 2] = m2
        if a is not None: film[i, 3] = a
        if sl is not None:
            slots["id"][i] = [s[0] for s in sl] + [abi.MATTE_NONE] * (8 - len(sl))
            slots["count"][i] = [s[1] for s in sl] + [0] * (8 - len(sl))

    full = [(11 * k + 3, k + 1) for k in range(8)]                                     # counts sum to 36
    specials = [
        dict(n=0, r=2.0, h=1.0, a=1.0, sl=full),                                       # no sample: black whatever it holds
        dict(n=1, r=NAN, h=1.0, m1=1.0, m2=1.0, a=0.0),
        dict(n=2, r=INF, h=1.0, m1=1.0, m2=1.0, a=1.0),
        dict(n=SPP, r=1.0, h=0.0, N=(0.0, 0.0, 0.0), a=0.5),                           # every sample missed: mid grey, no depth
        dict(n=100, r=3.0, h=1.0, sl=full, a=NAN),                                     # eight full slots, 64 samples found none
        dict(n=8, sl=[(abi.MATTE_NONE, 3), (5, 5)], r=-1.0, h=1.0, a=-0.25),           # the background's slot; a negative depth
        dict(n=8, sl=[(7, 3)], r=-0.0, h=1.0, a=1.5),                                  # five samples to no slot; depth -0
        dict(n=4000000000, sl=[(0, 4000000000)], r=2.0, h=NAN, m1=NAN, m2=1.0),
        dict(n=3, sl=[(abi.MATTE_NONE - 1, 1), (0, 1), (1, 1)], r=0.5, h=0.5, m1=-1.0, m2=2.0),
    ]
    for q in range(5):                                                                  # the ramp's stops, three ways
        specials.append(dict(n=max(SPP * q // 4, 1) if q else 1, r=float(q + 1), h=1.0, m1=1.0, m2=1.0 + (q / 4.0) ** 2))
        specials.append(dict(n=2, r=(q + 1) * 0.5, h=0.5, m1=1.0, m2=1.0 + (q / 4.0) ** 2, a=q / 4.0))
        specials.append(dict(n=SPP * q // 4 if q else SPP + 1, r=float(q + 1), h=1.0))
    specials += [dict(n=2, m1=0.0, m2=0.0), dict(n=2, m1=1e-4, m2=1.0), dict(n=2, m1=1.0, m2=NAN), dict(n=2, m1=1.0, m2=INF)]
    for i in range(len(specials)):
        special(i, **specials[(i + first) % len(specials)])
    if kind != "mixed":
        normal[:, 3] = 0                                                                # nothing was hit ...
        if kind == "one_depth":
            i = npix // 2                                                               # ... but here
            normal[i, 3], moments[i, 0], counts[i] = 1.0, 2.75, max(int(counts[i]), 1)
    out = dict(normal=normal.reshape(H, W, 4), moments=moments.reshape(H, W, 4), film=film.reshape(H, W, 4),
               slots=slots.reshape(H, W, abi.MATTE_SLOTS), counts=counts.reshape(H, W), spp=SPP)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return out


def cases():
    """(size, kind, first) of every card the host and GPU parity tests run: each kind at each size, and at 1 x 1 every special pixel's
    neighbourhood through a few rotations."""
    out = [(s, k, 0) for s in SIZES for k in KINDS]
    out += [((1, 1), "mixed", f) for f in (1, 3, 4, 5, 6, 7, 9, 10, 11, 24)]
    return out


def option_sets(view):
    """The options a view is tested under: both ramps where it has one, the card's own range and MANUAL_RANGE, two noise scales."""
    if view == abi.VIEW_DEPTH:
        return [dict(view=view, ramp=r, **k) for r in RAMPS
                for k in (dict(auto_range=1), dict(auto_range=0, depth_min=MANUAL_RANGE[0], depth_max=MANUAL_RANGE[1]))]
    if view == abi.VIEW_NOISE:
        return [dict(view=view, ramp=r, noise_max=m) for r in RAMPS for m in (1.0, 0.1)]
    if view == abi.VIEW_MATTE:
        return [dict(view=view, ramp=r, layer=l) for r in RAMPS for l in (abi.MATTE_INSTANCE, abi.MATTE_MATERIAL)][:3]
    return [dict(view=view, ramp=r) for r in RAMPS]


# ---- the host build of pt_view.h ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load(src=SRC, lib=LIB)
    L.view_host_pass.argtypes = [C.POINTER(abi.ViewInputs), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(abi.ViewOptions), C.c_void_p,
                                 C.POINTER(abi.ViewStats)]
    L.view_host_pass.restype = None
    L.view_host_hash.argtypes = [C.c_uint32]
    L.view_host_hash.restype = C.c_uint32
    L.view_host_options_valid.argtypes = [C.POINTER(abi.ViewOptions)]
    L.view_host_options_valid.restype = C.c_uint32
    L.view_host_shown.argtypes = [C.c_uint32] + [C.c_int] * 5
    L.view_host_shown.restype = C.c_uint32
    L.view_host_layout.argtypes = [C.POINTER(C.c_uint32 * 24)]
    return L


def host_view(inp, o, rect=None):
    """pt_debug_view on the host: ((H, W, 4) uint8, stats tuple)."""
    counts = np.ascontiguousarray(inp["counts"], u32)
    H, W = counts.shape
    keep = [counts]

    def ptr(name, dtype):
        a = np.ascontiguousarray(inp[name], dtype)
        keep.append(a)
        return a.ctypes.data

    vi = abi.ViewInputs(None, ptr("normal", f32), ptr("moments", f32), ptr("film", f32), ptr("slots", SLOT), counts.ctypes.data, inp["spp"])
    r = (C.c_uint32 * 4)(*(rect if rect is not None else (0, 0, W, H)))
    out = np.empty((H, W, 4), np.uint8)
    st = abi.ViewStats()
    lib().view_host_pass(C.byref(vi), W, H, C.addressof(r), C.byref(o), out.ctypes.data, C.byref(st))
    return out, stats_tuple(st)


def layout():
    o = (C.c_uint32 * 24)()
    lib().view_host_layout(C.byref(o))
    return list(o)


def first_difference(a, b):
    bad = np.argwhere(np.asarray(a) != np.asarray(b))
    return "%d bytes differ, the first at %s: %r against %r" % (len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]) if len(bad) else "equal"
