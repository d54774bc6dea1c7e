"""Host side of the auto-exposure tests: the ctypes wrapper of tests/emu/exposure_emu.cpp (the host build of
pt_exposure.h, a library of its own built by tests/host_build.py), an independent numpy restatement of the meter (np.frexp for the bins,
np.cumsum for the ranks, float64 for the resolve: no code shared with the header) and the test cards.  TEST HARNESS, never imported by
platinum_amd."""
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

SRC = os.path.join(_ROOT, "tests", "emu", "exposure_emu.cpp")
LIB = os.path.join(_ROOT, "tests", "_build", "libptamd_exposure.so")
f32 = np.float32
LUM_MIN, LUM_MAX = f32(2.0 ** -16), f32(2.0 ** 16)
INT_FIELDS = ("below", "above", "nonfinite", "metered", "kept", "weighted")
FLOAT_FIELDS = ("mean_log2", "target_ev", "ev", "gain")


@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load(src=SRC, lib=LIB)
    L.ex_host_meter.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(abi.ExposureOptions), C.c_float, C.c_uint32,
                                C.POINTER(abi.ExposureMeter), C.c_void_p]
    L.ex_host_resolve.argtypes = [C.POINTER(abi.ExposureMeter), C.POINTER(abi.ExposureOptions), C.c_float, C.c_uint32]
    L.ex_host_classify.argtypes = [C.c_float]
    L.ex_host_classify.restype = C.c_uint32
    L.ex_host_lum.argtypes = [C.c_float] * 3
    L.ex_host_lum.restype = C.c_float
    L.ex_host_exp2s.argtypes = [C.c_float]
    L.ex_host_exp2s.restype = C.c_float
    L.ex_host_options_valid.argtypes = [C.POINTER(abi.ExposureOptions)]
    L.ex_host_options_valid.restype = C.c_uint32
    L.ex_host_layout.argtypes = [C.POINTER(C.c_uint32 * 20)]
    return L


def options(**fields):
    """pt_exposure_options with the defaults DESIGN.md §3d states, then `fields`."""
    o = abi.ExposureOptions(0, -2.4739313, 0.10, 0.95, -16.0, 16.0, 0.0)
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def host_meter(img, rect=None, o=None, prev_ev=None, scaled=True):
    """pt_exposure.h built for the host on an (H, W, 4) float32 image: (abi.ExposureMeter, image * gain or None).  prev_ev: the smoothing
    state the resolve starts from (None: none)."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    H, W = img.shape[:2]
    o = options() if o is None else o
    r = None if rect is None else (C.c_uint32 * 4)(*rect)
    m = abi.ExposureMeter()
    out = np.empty((H, W, 4), np.float32) if scaled else None
    lib().ex_host_meter(img.ctypes.data, W, H, None if r is None else C.addressof(r), C.byref(o), 0.0 if prev_ev is None else prev_ev,
                        0 if prev_ev is None else 1, C.byref(m), None if out is None else out.ctypes.data)
    return m, out


def host_resolve(bins, o, prev_ev=None):
    m = abi.ExposureMeter()
    for b, v in enumerate(bins):
        m.bins[b] = int(v)
    lib().ex_host_resolve(C.byref(m), C.byref(o), 0.0 if prev_ev is None else prev_ev, 0 if prev_ev is None else 1)
    return m


def host_exp2s(x):
    return lib().ex_host_exp2s(x)


def layout():
    o = (C.c_uint32 * 20)()
    lib().ex_host_layout(C.byref(o))
    return list(o)


def record(m):
    """An ExposureMeter as comparable Python values: bins as an array, integers, and the floats' bit patterns."""
    d = {"bins": np.array(m.bins[:], np.uint32)}
    for k in INT_FIELDS:
        d[k] = int(getattr(m, k))
    for k in FLOAT_FIELDS:
        d[k] = int(np.array(getattr(m, k), np.float32).view(np.uint32))
    return d


def assert_same_record(got, want, what=""):
    g, w = record(got), record(want)
    assert np.array_equal(g["bins"], w["bins"]), "%s: bins differ at %s" % (what, np.flatnonzero(g["bins"] != w["bins"])[:8].tolist())
    for k in INT_FIELDS + FLOAT_FIELDS:
        assert g[k] == w[k], "%s: %s: %r != %r" % (what, k, getattr(got, k), getattr(want, k))


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------------
def np_lum(img):
    """Y in float32 with dn_lum's order of operations (numpy rounds every float32 operation on its own)."""
    a = np.asarray(img, np.float32)
    with np.errstate(all="ignore"):
        return (f32(0.2126) * a[..., 0] + f32(0.7152) * a[..., 1]) + f32(0.0722) * a[..., 2]


def np_classify(Y):
    """(bin (-1 where not binned), below, above, nonfinite) of float32 luminances, through np.frexp: Y = m * 2^e with m in [0.5, 1) lies in
    octave e - 1, and in its eighth floor((2 m - 1) * 8)."""
    Y = np.asarray(Y, np.float32)
    nonfinite = ~np.isfinite(Y)
    with np.errstate(invalid="ignore"):
        below = ~nonfinite & (Y < LUM_MIN)
        above = ~nonfinite & (Y >= LUM_MAX)
    binned = ~(nonfinite | below | above)
    m, e = np.frexp(np.where(binned, Y, f32(1.0)).astype(np.float64))
    b = (e.astype(np.int64) - 1 + 16) * 8 + np.floor((2.0 * m - 1.0) * 8.0).astype(np.int64)
    return np.where(binned, b, -1), below, above, nonfinite


def np_histogram(img, rect=None):
    a = np.asarray(img, np.float32)
    if rect is not None:
        x0, y0, x1, y1 = rect
        a = a[y0:y1, x0:x1]
    b, below, above, nonfinite = np_classify(np_lum(a))
    assert b.max(initial=0) <= 255
    return np.bincount(b[b >= 0].ravel(), minlength=256).astype(np.uint64), int(below.sum()), int(above.sum()), int(nonfinite.sum())


def np_resolve(bins, o, prev_ev=None):
    """dict(metered, kept, weighted, mean_log2, target_ev, ev, gain): the resolve of DESIGN.md §3d in Python integers and float64."""
    bins = np.asarray(bins, np.uint64).astype(object)      # Python integers: no overflow, no rounding
    n = int(bins.sum())
    lo = int(np.float64(n) * np.float64(f32(o.low_fraction)))
    hi = min(n, int(np.float64(n) * np.float64(f32(o.high_fraction))))
    if hi <= lo:
        lo, hi = 0, n
    c1 = np.cumsum(bins)
    c0 = c1 - bins
    kept = [max(0, min(int(b1), hi) - max(int(b0), lo)) for b0, b1 in zip(c0, c1)]
    K, S = hi - lo, sum(k * (2 * b + 1) for b, k in enumerate(kept))
    assert sum(kept) == K
    if n == 0:
        mean = target = 0.0
    else:
        mean = S / (16.0 * K) - 16.0
        target = min(max(float(f32(o.target_log2)) - mean, float(f32(o.min_ev))), float(f32(o.max_ev)))
    ev = target if prev_ev is None else prev_ev + (1.0 - float(f32(o.smoothing))) * (target - prev_ev)
    return dict(metered=n, kept=K, weighted=S, mean_log2=mean, target_ev=target, ev=ev, gain=2.0 ** ev)


def assert_matches_numpy(m, img, rect, o, prev_ev=None, what=""):
    """The integers exactly; mean_log2 / target_ev / ev within 1e-5 of float64 (three roundings of values of magnitude <= 32, at most 1e-6
    each); gain = the host's pp_exp2s(ev) on the bits."""
    bins, below, above, nonfinite = np_histogram(img, rect)
    want = np_resolve(bins, o, prev_ev)
    assert np.array_equal(np.array(m.bins[:], np.uint64), bins), what
    assert (m.below, m.above, m.nonfinite) == (below, above, nonfinite), what
    assert (m.metered, m.kept, m.weighted) == (want["metered"], want["kept"], want["weighted"]), what
    for k in ("mean_log2", "target_ev", "ev"):
        assert abs(getattr(m, k) - want[k]) <= 1e-5, (what, k, getattr(m, k), want[k])
    assert f32(m.gain).view(np.uint32) == f32(host_exp2s(m.ev)).view(np.uint32), what
    return want


# ---- cards -----------------------------------------------------------------------------------------------------------------------------
def log_uniform_card(w, h, seed=0, lo=-20.0, hi=20.0):
    """Channels 2^u, u uniform in [lo, hi): with the defaults a tenth of the pixels falls off either end of the metered range."""
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(lo, hi, (h, w, 4))).astype(np.float32)
    img[..., 3] = rng.random((h, w)).astype(np.float32)
    return img


def bin_edges():
    """[(value, bin)]: the smallest and the largest float32 of every bin."""
    out = []
    for b in range(256):
        first = np.array((b + 888) << 20, np.uint32).view(np.float32)
        last = np.array(((b + 889) << 20) - 1, np.uint32).view(np.float32)
        out += [(first, b), (last, b)]
    return out


FLT_MAX = np.finfo(np.float32).max
# luminances and the counter each belongs to: a bin, or "below" / "above" / "nonfinite"
SPECIAL_Y = [(LUM_MIN, 0), (np.nextafter(LUM_MIN, f32(0)), "below"), (np.nextafter(LUM_MAX, f32(0)), 255), (LUM_MAX, "above"),
             (f32(0.0), "below"), (f32(-1.0), "below"), (f32(1e-40), "below"), (f32(np.nan), "nonfinite"), (f32(np.inf), "nonfinite"),
             (f32(-np.inf), "nonfinite")]
# The largest finite rgb.  Y cannot overflow from finite channels: the three float32 weights sum to 1 and Y grows with every channel, so
# its maximum is this pixel's, which float32 rounds to FLT_MAX itself (test_exposure_host.py checks that): the pixel is counted `above`.
LARGEST_RGB = (FLT_MAX, FLT_MAX, FLT_MAX)


def special_card():
    """(1, n, 4): SPECIAL_Y and both edges of every bin as greys (a grey's Y lands on, just below or just above the value: the restatement
    says where), and LARGEST_RGB; alpha carries values the meter must ignore."""
    greys = [v for v, _ in SPECIAL_Y] + [v for v, _ in bin_edges()]
    img = np.zeros((1, len(greys) + 1, 4), np.float32)
    img[0, :-1, :3] = np.array(greys, np.float32)[:, None]
    img[0, -1, :3] = LARGEST_RGB
    img[0, :, 3] = np.resize(np.array([1.0, 0.0, np.nan, np.inf, -3.0], np.float32), img.shape[1])
    return img
