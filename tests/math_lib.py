"""The independent witness of the math layer (platinum_amd/csrc/pt_math.h, pt_sampler.h, the guards of pt_post.h / pt_denoise.h): float64
numpy references written from the functions' definitions, the input sets placed where the algorithms break, each function's domain, and
the error bounds measured on the oracle ("The math layer has an independent witness").  tests/test_math_host.py and
tests/test_gpu_math.py run the three implementations (oracle twin, host build, device) over these sets.  TEST HARNESS: shares no code with
any implementation."""
import ctypes as C
import functools
import json
import os

import numpy as np

import host_build
import oracle_lib
from platinum_amd import abi

F32, U32, F64 = np.float32, np.uint32, np.float64
PI = np.pi
ONE_MINUS_EPS = F32(1) - F32(2.0 ** -24)    # defs.metal:22
FLT_MAX = np.finfo(F32).max
MIN_NORMAL = F32(2.0 ** -126)
TWO_OUT = (abi.PT_MATH_SINCOS, abi.PT_MATH_SAMPLE_DISK, abi.PT_MATH_SAMPLE_COSINE_HEMISPHERE, abi.PT_MATH_SAMPLE_TRI_UNIFORM)


# ---- the implementations, as batch calls --------------------------------------------------------------------------------------------------

def _batch(call, fn, a, b):
    a = np.ascontiguousarray(a)
    b = None if b is None else np.ascontiguousarray(b)
    n = a.size
    out0 = np.zeros(n, U32)
    out1 = np.zeros(2 * n if fn == abi.PT_MATH_SAMPLE_COSINE_HEMISPHERE else n, U32) if fn in TWO_OUT else None
    call(fn, n, a.ctypes.data, None if b is None else b.ctypes.data, out0.ctypes.data, None if out1 is None else out1.ctypes.data)
    return out0, out1


def oracle(fn, a, b=None):
    """orc_math_batch: (out0, out1) as uint32 words"""
    return _batch(oracle_lib.lib().orc_math_batch, fn, a, b)


def host(fn, a, b=None):
    """emu_math_batch, the host build of pt_math_probe.h: (out0, out1) as uint32 words"""
    L = host_build.load()
    L.emu_math_batch.restype = None
    L.emu_math_batch.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return _batch(L.emu_math_batch, fn, a, b)


def same_bits(x, y):
    """Bit equality of two result tuples; NaNs equal one another whatever their payload."""
    for p, q in zip(x, y):
        if p is None and q is None:
            continue
        pf, qf = p.view(F32), q.view(F32)
        both_nan = np.isnan(pf) & np.isnan(qf)
        if not np.array_equal(p[~both_nan], q[~both_nan]):
            return False
    return True


def first_difference(x, y, a, b=None):
    """For a failure message: the first element at which two result tuples differ."""
    for k, (p, q) in enumerate(zip(x, y)):
        if p is None:
            continue
        bad = np.nonzero(p != q)[0]
        if bad.size:
            i = int(bad[0]) % a.size
            return "out%d[%d]: %08x != %08x at a = %08x, b = %s (%d differ)" % (k, bad[0], p[bad[0]], q[bad[0]], a.view(U32)[i],
                                                                               None if b is None else "%08x" % b.view(U32)[i], bad.size)
    return "equal"


# ---- helpers for the input sets -----------------------------------------------------------------------------------------------------------

def ulps(x, k):
    """x and its k float32 neighbours on each side"""
    x = np.atleast_1d(np.asarray(x, F32))
    out, up, dn = [x], x, x
    for _ in range(k):
        up = np.nextafter(up, F32(np.inf)); dn = np.nextafter(dn, F32(-np.inf))
        out += [up, dn]
    return np.concatenate(out)


def _cat(parts):
    return np.concatenate([np.asarray(p, F32).ravel() for p in parts])


class Case:
    """One function's inputs: float32 (or uint32) arrays a, b and the classes {name: slice} the error bounds are stated for."""
    def __init__(self, fn, parts):
        self.fn = fn
        self.classes, a, b, at = {}, [], [], 0
        for name, pa, pb in parts:
            pa = np.ascontiguousarray(pa).ravel()
            a.append(pa)
            if pb is not None:
                pb = np.ascontiguousarray(pb).ravel()
                assert pb.shape == pa.shape
                b.append(pb)
            self.classes[name] = slice(at, at + pa.size)
            at += pa.size
        self.a = np.concatenate(a)
        self.b = np.concatenate(b) if b else None
        assert self.a.size <= 1 << 22 and self.a.dtype.itemsize == 4


# ---- input sets: at most 2^22 elements per function, fixed seeds ----------------------------------------------------------------------------
# DOMAINS (the raw functions convert rint(x) to int: outside these the host build is undefined, so nothing outside goes to them):
#   sincos_det / cos_det   finite |x| <= 8192            atan2_det   every pair of finite floats (the quotient may overflow: atan(inf) = pi/2)
#   acos_det               every finite float (clamped)  log2_det    positive normal floats
#   exp2_det               [-126.5, 127.5)               powr_det    x <= 0, or y * log2(x) in exp2_det's domain
#   pp_log2, dn_exp2 (NaN included, below 127.5), bokeh_powr: every float.  pp_exp2 / pp_exp2s: every float but NaN.
#   pp_powr / dn_powr      x <= 0, or a product y * log2(x) that is a number (dn_powr: below 127.5; the host caps sigma_n at 2^24 for that)
SINCOS_MAX = 8192.0
EXP2_LO, EXP2_HI = -126.5, 127.5


@functools.lru_cache(None)
def sincos_case():
    rng = np.random.default_rng(101)
    quarter = F32(np.arange(-32, 33, dtype=F64) * (PI / 4))      # every quadrant switch ((2k + 1) pi / 4: the rintf ties) and every k pi / 2
    tiny = _cat([[0.0, -0.0], ulps(MIN_NORMAL, 2), -ulps(MIN_NORMAL, 2), F32(2.0 ** -149) * F32([1, 2, 1000, -1, -1000]), F32(2.0 ** -140)])
    return Case(abi.PT_MATH_SINCOS, [
        # every call site stays inside [-8, 8]: 2 pi u, pi u, and the polygon term fmodf(...) - pi / n
        ("call", _cat([rng.uniform(-8, 8, 1 << 20), ulps(quarter[np.abs(quarter) <= 8], 4), tiny, [8.0, -8.0]]), None),
        ("wide", _cat([rng.uniform(-SINCOS_MAX, SINCOS_MAX, 1 << 20), ulps(quarter, 4), [SINCOS_MAX, -SINCOS_MAX],
                       ulps(F32(np.arange(-5000, 5001, 250, dtype=F64) * (PI / 4) + PI / 4), 2)]), None)])


def _directions(rng, n):
    v = rng.normal(size=(n, 3))
    d = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
    return np.concatenate([d, axes, F32([[0.0, 1.0, -0.0], [-0.0, -1.0, 0.0], [1e-30, 1.0, 1e-30], [1e-4, -1.0, -1e-4]])])


@functools.lru_cache(None)
def atan2_case():
    rng = np.random.default_rng(102)
    n = 1 << 18
    mag = lambda: F32(np.exp2(rng.uniform(-20, 20, n)) * rng.choice([-1.0, 1.0], n))   # all four quadrants
    v = F32([1.0, 3.5, 1e-30, 1e30, MIN_NORMAL])
    z = F32([0.0, -0.0])
    axes_y = _cat([np.repeat(v, 2), -np.repeat(v, 2), np.tile(z, 5), np.tile(z, 5), [0.0, 0.0, -0.0, -0.0]])
    axes_x = _cat([np.tile(z, 5), np.tile(z, 5), np.repeat(v, 2), -np.repeat(v, 2), [0.0, -0.0, 0.0, -0.0]])
    # atan_det's two branch points: |y / x| at tan(pi / 8) and tan(3 pi / 8), +- 0 .. 4 ulp, in every quadrant, at x = 1 and x = 3
    t = ulps(F32([np.tan(PI / 8), np.tan(3 * PI / 8)]), 4)
    br_y = _cat([s * t * x for s in (1, -1) for x in (1.0, 3.0) for _ in (0, 1)])
    br_x = _cat([np.full(t.size, sx * x, F32) for s in (1, -1) for x in (1.0, 3.0) for sx in (1, -1)])
    k = np.arange(-60, 61)
    ratio_y = _cat([F32(np.exp2(k) * m) * s for m in (1.0, 1.37) for s in (1, -1)])
    ratio_x = _cat([np.full(k.size, s, F32) for m in (1.0, 1.37) for s in (1, -1)])
    d = _directions(rng, 1 << 18)     # pt_shade.h rayDirToUv: atan2_det(-dir.z, -dir.x)
    return Case(abi.PT_MATH_ATAN2, [("quadrants", _cat([mag(), axes_y, br_y, ratio_y]), _cat([mag(), axes_x, br_x, ratio_x])),
                                    ("directions", -d[:, 2], -d[:, 0])])


@functools.lru_cache(None)
def acos_case():
    rng = np.random.default_rng(103)
    d = _directions(rng, 1 << 18)     # pt_shade.h rayDirToUv: acos_det(dir.y)
    edge = _cat([ulps(F32([1.0, -1.0]), 64), [0.0, -0.0, 2.0, -2.0, 1e30, -1e30, 1e-30, MIN_NORMAL], ulps(F32([0.5, -0.5, np.sqrt(0.5)]), 4)])
    return Case(abi.PT_MATH_ACOS, [("range", _cat([rng.uniform(-1, 1, 1 << 18), edge]), None), ("directions", d[:, 1], None)])


@functools.lru_cache(None)
def log2_case():
    rng = np.random.default_rng(104)
    k = np.arange(-126, 128)
    fold = ulps(F32(np.sqrt(0.5) * np.exp2(np.arange(-125, 128, dtype=F64))), 4)      # the mantissa fold, in every binade
    near1 = ulps(F32(1.0), 64)
    normal = rng.integers(0x00800000, 0x7f800000, 1 << 20, dtype=np.uint32).view(F32)
    return Case(abi.PT_MATH_LOG2, [("pow2", F32(np.exp2(k.astype(F64))), None),
                                   ("near1", _cat([near1, rng.uniform(0.5, 1.5, 1 << 18)]), None),     # |x - 1| <= 1/2: absolute error
                                   ("all", _cat([normal, fold, [FLT_MAX, MIN_NORMAL]]), None)])      # relative error (absolute inside near1's range)


@functools.lru_cache(None)
def exp2_case():
    rng = np.random.default_rng(105)
    k = np.arange(-126, 128, dtype=F64)
    ties = ulps(F32(np.arange(-127, 127, dtype=F64) + 0.5), 2)          # rintf's round-to-even ties
    ties = ties[(ties >= F32(-126.0)) & (ties < F32(EXP2_HI))]
    den = _cat([rng.uniform(-126.5, -126.0, 1 << 16), ulps(F32(-126.5), 2), ulps(F32(-126.0), 2)])
    den = den[(den >= F32(EXP2_LO)) & (den < F32(-126.0))]              # denormal results, on purpose
    return Case(abi.PT_MATH_EXP2, [("ints", F32(k), None),
                                   ("normal", _cat([rng.uniform(-126, EXP2_HI, 1 << 20).astype(F32).clip(-126, np.nextafter(F32(EXP2_HI), F32(0))), ties]), None),
                                   ("denormal", den, None)])


# Call-site ranges of the powers, each derived from the code beside it.
@functools.lru_cache(None)
def powr_case():
    rng = np.random.default_rng(106)
    n = 1 << 19
    # thin lens (pt_shade.h stage_raygen): x = sqrt(u) with u a Halton sample in [2^-32, 1), so x in [2^-16, 1); y = 2^bokehPower with the
    # reference UI's bokehPower in [-1, 1]: y in [1/2, 2]
    lens = (F32(np.exp2(rng.uniform(-16, 0, n))).clip(F32(2.0 ** -16), ONE_MINUS_EPS), F32(rng.uniform(0.5, 2.0, n)))
    return Case(abi.PT_MATH_POWR, [("lens", lens[0], lens[1])])


@functools.lru_cache(None)
def pp_powr_case():
    rng = np.random.default_rng(107)
    n = 1 << 19
    # the post chain (pt_post.h): the base is a colour after the contrast pass' clamp to [0, kPostCeiling = 2^64], or a ratio in (0, 1]; the
    # exponents are 2.2, 1 / 2.4, 1 / gamma, agx_power, the toe / shoulder powers and vig_power / 100..: (0, 8] covers what the option ranges give
    x = _cat([np.exp2(rng.uniform(-64, 64, n)), [2.0 ** 64, 1.0, MIN_NORMAL]])
    y = _cat([rng.uniform(1.0 / 16, 8.0, n), [2.2, 1 / 2.4, 8.0]])
    return Case(abi.PT_MATH_PP_POWR, [("post", x, y)])


@functools.lru_cache(None)
def dn_powr_case():
    rng = np.random.default_rng(108)
    n = 1 << 19
    # pt_denoise.h: wn = dn_powr(max(0, n . n'), sigma_n): x in [0, 1] up to the rounding of a dot product of unit normals, sigma_n > 0 and at
    # most 2^24 (pt_set_denoise_options accepts every finite value; the host passes min(sigma_normal, kDnSigmaNormalMax) on), default 128
    x = _cat([rng.uniform(0, 1, n), 1 - np.exp2(rng.uniform(-24, -1, n)), [0.0, 1.0, -0.0]])
    y = _cat([np.exp2(rng.uniform(-4, 12, 2 * n)), [128.0, 2.0 ** 24, 128.0]])
    return Case(abi.PT_MATH_DN_POWR, [("normal_weight", x, y)])


def _stratified(rng, n):
    j = (np.arange(n)[:, None] + rng.random((n, n))) / n
    i = (np.arange(n)[None, :] + rng.random((n, n))) / n
    return F32(np.minimum(i, ONE_MINUS_EPS)).ravel(), F32(np.minimum(j, ONE_MINUS_EPS)).ravel()


@functools.lru_cache(None)
def warp_inputs():
    rng = np.random.default_rng(109)
    gx, gy = _stratified(rng, 1024)
    t = F32(np.minimum(np.arange(1024) / 1024 + rng.random(1024) / 1024, ONE_MINUS_EPS))
    e0, e1 = np.zeros(1024, F32), np.full(1024, ONE_MINUS_EPS, F32)
    edge_x = _cat([e0, e1, t, t, [0, 0, ONE_MINUS_EPS, ONE_MINUS_EPS]])
    edge_y = _cat([t, t, e0, e1, [0, ONE_MINUS_EPS, 0, ONE_MINUS_EPS]])
    diag = F32(rng.random(4096)).clip(F32(2.0 ** -20), np.nextafter(ONE_MINUS_EPS, F32(0)))     # sampleTriUniform's branch: u.x = u.y +- 1 ulp
    diag_x = _cat([diag, diag, diag])
    diag_y = _cat([diag, np.nextafter(diag, F32(2)), np.nextafter(diag, F32(-1))])
    return [("grid", gx, gy), ("edges", edge_x, edge_y), ("diagonal", diag_x, diag_y)]


def warp_case(fn):
    return Case(fn, warp_inputs())


def primes():
    out, c = [], 2
    while len(out) < 620:
        if all(c % d for d in range(2, int(c ** 0.5) + 1)):
            out.append(c)
        c += 1
    return np.array(out, np.uint64)


@functools.lru_cache(None)
def halton_case():
    rng = np.random.default_rng(110)
    P = primes()
    i_rand = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64)
    d_rand = rng.integers(0, 620, 1 << 20, dtype=np.uint64)
    bi, bd = [], []
    for d, p in enumerate(int(x) for x in P):
        chunk, digits = p, 1
        while chunk * p < (1 << 22):      # the largest power of the prime below 2^22: what one magic division peels
            chunk *= p; digits += 1
        idx = [0, 1, chunk - 1, chunk, chunk + 1, chunk * chunk - 1, chunk * chunk, chunk * chunk + 1, (1 << 32) - 1, (1 << 32) - 2,
               ((1 << 32) // chunk) * chunk - 1, ((1 << 32) // chunk) * chunk, (1 << 21) - 1, 1 << 21, (1 << 21) + 1]
        for j in range(digits + 1):       # a leading part of 1 .. digits digits (the TOP early exit), above a zero and a full remainder
            for lead in (p ** j, p ** (j + 1) - 1, p ** j + 1):
                idx += [lead * chunk, lead * chunk + chunk - 1, lead * chunk + p - 1, lead * chunk * chunk + 1]
        for r in (chunk - p, chunk - p - 1, chunk - p + 1, p * (p - 1), p * p - 1):   # digit splits on the fp32 rounding boundary
            idx += [r, chunk + r, ((1 << 32) // chunk - 1) * chunk + r]
        idx = [i for i in idx if 0 <= i < (1 << 32)]
        bi += idx; bd += [d] * len(idx)
    ends = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)
    return Case(abi.PT_MATH_HALTON, [("random", i_rand.astype(U32), d_rand.astype(U32)),
                                     ("boundaries", np.array(bi, np.uint64).astype(U32), np.array(bd, np.uint64).astype(U32)),
                                     ("first_last", np.concatenate([ends, ends]).astype(U32), np.repeat(U32([0, 619]), ends.size))])


def halton_reference(i, d):
    """The reference's loop (samplers.metal:168-184) in float32 with real integer division: f *= 1/b; r += f * (i % b); i //= b; min(r, 1 - eps)"""
    b = primes()[d.astype(np.int64)]
    i = i.astype(np.uint64)
    inv = F32(1) / b.astype(F32)
    f, r = np.ones(i.size, F32), np.zeros(i.size, F32)
    while np.any(i > 0):
        live = i > 0
        f = np.where(live, f * inv, f).astype(F32)
        r = np.where(live, r + (f * (i % b).astype(F32)).astype(F32), r).astype(F32)
        i = i // b
    return np.minimum(r, ONE_MINUS_EPS)


@functools.lru_cache(None)
def halton_offset_case():
    kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "sampler_kat.json")))["offsets"]
    rng = np.random.default_rng(111)
    x, y = rng.integers(0, 1 << 16, 1 << 16, dtype=np.uint64), rng.integers(0, 1 << 16, 1 << 16, dtype=np.uint64)
    s = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)
    kx, ky, ks = (np.array([k[j] for k in kat], np.uint64) for j in range(3))
    assert kx.max() < 65536 and ky.max() < 65536
    c = Case(abi.PT_MATH_HALTON_OFFSET, [("kat", (kx | (ky << np.uint64(16))).astype(U32), ks.astype(U32)),
                                         ("random", (x | (y << np.uint64(16))).astype(U32), s.astype(U32))])
    c.kat_want = np.array([k[3] for k in kat], np.uint64).astype(U32)
    return c


# ---- the guards: cut-offs +- 0 .. 4 ulp and the special values ------------------------------------------------------------------------------
SPECIALS = _cat([[np.inf, -np.inf, FLT_MAX, -FLT_MAX, 0.0, -0.0, -1.0, -1e-30, 1e-40, -1e-40, 2.0 ** -149], [MIN_NORMAL, 1.0, 300.0, -300.0]])
NAN = F32(np.nan)


def guard_inputs(cutoffs, nan):
    x = _cat([ulps(F32(cutoffs), 4), SPECIALS] + ([[NAN]] if nan else []))
    return x


# ---- float64 references ---------------------------------------------------------------------------------------------------------------------

def ref_sincos(x):
    x = x.astype(F64)
    return np.sin(x), np.cos(x)


def ref_atan2(y, x):
    """the usual quadrant rules on the values, the sign of a zero ignored; atan2(0, 0) = 0"""
    y, x = y.astype(F64) + 0.0, x.astype(F64) + 0.0
    y, x = np.where(y == 0, 0.0, y), np.where(x == 0, 0.0, x)
    return np.where((x == 0) & (y == 0), 0.0, np.arctan2(y, x))


def ref_acos(x):
    return np.arccos(np.clip(x.astype(F64), -1.0, 1.0))


def ref_exp2_guarded(x):
    """+inf above the float range, 0 below it"""
    with np.errstate(over="ignore", under="ignore"):
        v = np.exp2(x.astype(F64))
    return np.where(v > F64(FLT_MAX), np.inf, np.where(v < 2.0 ** -150, 0.0, v))


def ref_powr(x, y):
    """powr(x <= 0, .) = 0"""
    x, y = x.astype(F64), y.astype(F64)
    with np.errstate(all="ignore"):
        return np.where(x <= 0, 0.0, np.power(np.where(x <= 0, 1.0, x), y))


def ref_disk(ux, uy):
    ux, uy = ux.astype(F64), uy.astype(F64)
    r, th = np.sqrt(ux), 2 * PI * uy
    return r * np.cos(th), r * np.sin(th)


def ref_cosine_hemisphere(ux, uy):
    ux, uy = ux.astype(F64), uy.astype(F64)
    phi, st = 2 * PI * ux, np.sqrt(uy)
    return np.cos(phi) * st, np.sin(phi) * st, np.sqrt(1 - uy)


def ref_tri_uniform(ux, uy):
    ux, uy = ux.astype(F64), uy.astype(F64)
    lo = ux < uy
    b0 = np.where(lo, ux * 0.5, ux - uy * 0.5)
    b1 = np.where(lo, uy - ux * 0.5, uy * 0.5)
    return b0, b1


def rel(got, want):
    return np.abs(got.astype(F64) - want) / np.abs(want)


# ---- errors per class -----------------------------------------------------------------------------------------------------------------------

def errors(name, out):
    """{class: largest error} of results `out` = (out0, out1) words of one implementation on the case `name`, in the measure of DESIGN.md
    section 2's table: absolute for sincos / atan2 / acos / the warps, relative for exp2 / powr, log2 absolute in |x - 1| < 1/2 and relative
    elsewhere."""
    f = lambda w: w.view(F32).astype(F64)
    e = {}
    if name == "sincos":
        c = sincos_case()
        s, co = ref_sincos(c.a)
        err = np.maximum(np.abs(f(out[0]) - s), np.abs(f(out[1]) - co))
    elif name == "atan2":
        c = atan2_case()
        err = np.abs(f(out[0]) - ref_atan2(c.a, c.b))
    elif name == "acos":
        c = acos_case()
        err = np.abs(f(out[0]) - ref_acos(c.a))
    elif name == "log2":
        c = log2_case()
        want = np.log2(c.a.astype(F64))
        with np.errstate(all="ignore"):
            err = np.where(np.abs(c.a.astype(F64) - 1) <= 0.5, np.abs(f(out[0]) - want), rel(out[0].view(F32), want))
    elif name == "exp2":
        c = exp2_case()
        err = rel(out[0].view(F32), np.exp2(c.a.astype(F64)))
    elif name in ("powr", "pp_powr", "dn_powr"):
        c = {"powr": powr_case, "pp_powr": pp_powr_case, "dn_powr": dn_powr_case}[name]()
        want = ref_powr(c.a, c.b)
        # relative error where the true power is a normal float with room to spare; the conventions past the range are asserted apart
        lo = 2.0 ** -120 if name == "dn_powr" else 2.0 ** -125
        ok = (want > lo) & (want < 2.0 ** 127)
        with np.errstate(all="ignore"):
            err = np.where(ok, rel(out[0].view(F32), want), 0.0)
    elif name in ("disk", "cosine_hemisphere", "tri_uniform"):
        c = warp_case(WARPS[name][0])
        want = WARPS[name][1](c.a, c.b)
        n = c.a.size
        got = [f(out[0]), f(out[1][:n])] + ([f(out[1][n:])] if name == "cosine_hemisphere" else [])
        err = np.max([np.abs(g - w) for g, w in zip(got, want)], axis=0)
    else:
        raise KeyError(name)
    for k, sl in c.classes.items():
        e[k] = float(np.max(err[sl]))
    return e


WARPS = {"disk": (abi.PT_MATH_SAMPLE_DISK, ref_disk), "cosine_hemisphere": (abi.PT_MATH_SAMPLE_COSINE_HEMISPHERE, ref_cosine_hemisphere),
         "tri_uniform": (abi.PT_MATH_SAMPLE_TRI_UNIFORM, ref_tri_uniform)}
# every case with a float64 accuracy bound: name -> its Case
ACCURACY_CASES = {"sincos": sincos_case, "atan2": atan2_case, "acos": acos_case, "log2": log2_case, "exp2": exp2_case, "powr": powr_case,
                  "pp_powr": pp_powr_case, "dn_powr": dn_powr_case, "disk": lambda: warp_case(abi.PT_MATH_SAMPLE_DISK),
                  "cosine_hemisphere": lambda: warp_case(abi.PT_MATH_SAMPLE_COSINE_HEMISPHERE),
                  "tri_uniform": lambda: warp_case(abi.PT_MATH_SAMPLE_TRI_UNIFORM)}

# The bounds: for each function and class, twice the largest error of the ORACLE's implementation against the float64 reference on these very
# inputs, rounded up to one significant digit (measured: see the table in DESIGN.md section 2).  The product is bound to the oracle by bit
# equality, so the same bounds hold for the host build and the device.
#   (function, class): (measured on the oracle, bound asserted)
BOUNDS = {
    ("sincos", "call"): (7.75e-08, 2e-07), ("sincos", "wide"): (7.73e-08, 2e-07),                       # absolute
    ("atan2", "quadrants"): (2.65e-07, 6e-07), ("atan2", "directions"): (2.69e-07, 6e-07),              # absolute
    ("acos", "range"): (2.77e-07, 6e-07), ("acos", "directions"): (2.80e-07, 6e-07),                    # absolute
    ("log2", "pow2"): (0.0, 0.0), ("log2", "near1"): (7.91e-08, 2e-07), ("log2", "all"): (1.08e-07, 3e-07),   # absolute in |x - 1| <= 1/2, else relative
    ("exp2", "ints"): (0.0, 0.0), ("exp2", "normal"): (9.93e-08, 2e-07), ("exp2", "denormal"): (1.39e-07, 3e-07),   # relative
    ("powr", "lens"): (1.34e-06, 3e-06), ("pp_powr", "post"): (7.27e-06, 2e-05), ("dn_powr", "normal_weight"): (1.17e-05, 3e-05),   # relative
    ("disk", "grid"): (4.15e-07, 9e-07), ("disk", "edges"): (4.07e-07, 9e-07), ("disk", "diagonal"): (4.08e-07, 9e-07),           # absolute
    ("cosine_hemisphere", "grid"): (4.12e-07, 9e-07), ("cosine_hemisphere", "edges"): (4.07e-07, 9e-07),
    ("cosine_hemisphere", "diagonal"): (4.09e-07, 9e-07),
    ("tri_uniform", "grid"): (2.98e-08, 6e-08), ("tri_uniform", "edges"): (2.98e-08, 6e-08), ("tri_uniform", "diagonal"): (0.0, 0.0),
}
# | length - 1 | of the cosine hemisphere and | length - sqrt(u.x) | of the disk: measured 1.09e-7 and 1.11e-7 on the oracle
UNIT_LENGTH_BOUND = 3e-07


def check_accuracy(name, out):
    """Asserts every class of the case `name` inside its bound; returns the errors."""
    e = errors(name, out)
    for k, v in e.items():
        assert v <= BOUNDS[(name, k)][1], "%s / %s: error %.3g above the bound %.3g" % (name, k, v, BOUNDS[(name, k)][1])
    return e


PRODUCT_CUTS = [-127.0, -126.0, -125.0, 125.0, 127.5, 128.0]
BOKEH_POWERS = [-8.0, 3.0, 6.0, 200.0, -200.0, float("inf"), float("-inf"), float("nan")]


def lens_samples():
    """lens samples u down to 2^-32 (the smallest non-zero Halton value of base 2), 0 and 1 - eps"""
    u = _cat([np.exp2(-np.arange(0, 33, dtype=F64)) * (1 - 2.0 ** -24), np.exp2(-np.arange(1, 33, dtype=F64)) * 1.5, [0.0, ONE_MINUS_EPS],
              np.random.default_rng(112).random(4096) * (1 - 2.0 ** -24)])
    return u[(u == 0) | (u >= F32(2.0 ** -32))]


def guard_sets():
    """[(name, fn, a, b)]: every guarded form over its cut-offs +- 0 .. 4 ulp and the special values, inside its domain (see DOMAINS)"""
    y = ulps(F32(PRODUCT_CUTS), 4)
    yd = y[y < F32(127.5)]
    dn = guard_inputs([-125.0], nan=True)
    u = lens_samples()
    out = [("pp_exp2", abi.PT_MATH_PP_EXP2, guard_inputs([-127.0, 128.0, -126.5, 127.5], nan=False), None),
           ("pp_exp2s", abi.PT_MATH_PP_EXP2S, guard_inputs([-125.0, 125.0], nan=False), None),
           ("dn_exp2", abi.PT_MATH_DN_EXP2, dn[~(dn >= F32(127.5))], None),
           ("pp_log2", abi.PT_MATH_PP_LOG2, _cat([ulps(F32(0.0), 4), SPECIALS, [NAN]]), None),
           ("pp_powr", abi.PT_MATH_PP_POWR, _cat([np.full(y.size, 2.0), np.full(y.size, 4.0), [0.0, -0.0, -1.0, -np.inf, -1e-40]]),
            _cat([y, y * F32(0.5), np.full(5, 2.5)])),
           ("dn_powr", abi.PT_MATH_DN_POWR, _cat([np.full(yd.size, 2.0), np.full(yd.size, 4.0), [0.0, -0.0, -1.0, -np.inf, -1e-40], ulps(F32(1.0), 4)]),
            _cat([yd, yd * F32(0.5), np.full(5, 2.5), np.full(9, 2.0 ** 24)]))]   # (a dot product of unit normals rounded above 1, at the largest sigma_n the host passes on)
    for bp in BOKEH_POWERS:
        out.append(("bokeh_powr(%g)" % bp, abi.PT_MATH_BOKEH_POWR, u, np.full(u.size, bp, F32)))
    return out
