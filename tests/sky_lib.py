"""Host side of the sun-and-sky tests: the ctypes wrapper of tests/emu/sky_emu.cpp (the host build of pt_sky.h, a library of
its own built by tests/host_build.py), and a vectorised numpy restatement of the model that shares no code with the header.  In float64 it
is the WITNESS: positions are vectors, heights are |p| - Rg, chords come from the quadratic of the ray-sphere intersection and the disc's
test is d.s >= cos(alpha) -- the mathematics as DESIGN.md states it, with none of the header's rearrangements.  In float32 it takes the
rearranged expressions (a float32 quadratic cannot tell a height of one metre from none), and its distance from the witness is the figure
BOUNDS records: what float32 arithmetic costs this model.  TEST HARNESS, never imported by platinum_amd."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import host_build  # noqa: E402
from platinum_amd import abi  # noqa: E402

SRC = os.path.join(_ROOT, "tests", "emu", "sky_emu.cpp")
LIB = os.path.join(_ROOT, "tests", "_build", "libptamd_sky.so")
f32 = np.float32

RG, RA = 6360.0, 6460.0
BETA_R = (5.802e-3, 13.558e-3, 33.1e-3)
BETA_MS, BETA_ME = 3.996e-3, 8.396e-3
BETA_O = (0.650e-3, 1.881e-3, 0.085e-3)
HR, HM, G = 8.0, 1.2, 0.8
NV, NL = 32, 8

HOST_SIZES = [(64, 32), (37, 19), (8, 4)]                               # (w, h)
GPU_SIZES = [(1, 1), (8, 4), (37, 19), (64, 32), (256, 128)]
OPTION_SETS = {
    "default": {},                                   # the sun at e = 0.5
    "low-sun": dict(sun_elevation=0.05),
    "zenith": dict(sun_elevation=math.pi / 2),
    "twilight": dict(sun_elevation=-0.1),
    "azimuth-negative": dict(sun_azimuth=-2.2),
    "azimuth-wrapped": dict(sun_azimuth=7.5),
    "altitude-10": dict(altitude_km=10.0),
    "no-air": dict(air_density=0.0),
    "no-dust": dict(dust_density=0.0),
    "no-ozone": dict(ozone_density=0.0),
    "vacuum": dict(air_density=0.0, dust_density=0.0, ozone_density=0.0),
    "albedo-0": dict(ground_albedo=0.0),
    "albedo-1": dict(ground_albedo=1.0),
    "disc-off": dict(sun_disc=0),
}
HORIZON_CLEARANCE = 1e-3     # no texel centre of a compared map lies nearer the geometric horizon than this (radians)
LEFT_OUT_CAP = 0.005         # at most this share of a map's texels may be left out for a ground / blocked decision that fell the other way

# How far a second float32 implementation of this arithmetic may lie from the float64 witness.  `measured` is the largest relative error
# per channel (the denominator floored at FLOOR times the map's brightest sky channel: a channel near zero beside a bright one is not held
# to its own size) of np_sky in float32 against np_sky in float64 over OPTION_SETS x HOST_SIZES, the texels left out whose decisions
# differ (measure_float32_error(); test_sky_host.py re-measures it); `bound` is 4 x that, the margin bloom_lib uses for the same reason:
# another implementation may round each operation the other way.
# The worst case is the twilight set at 37 x 19: the little light left has crossed some twenty optical depths, and an error of the depth is
# an error of the light as large.  (A float32 prototype with the naive expressions lay at 2e-4.)
FLOOR = 1e-3
BOUNDS = {"measured": 1.1857e-5, "bound": 4 * 1.1857e-5}


@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load(src=SRC, lib=LIB)
    L.sk_host_valid.argtypes = [C.POINTER(abi.SkyOptions), C.c_uint32, C.c_uint32]
    L.sk_host_valid.restype = C.c_uint32
    L.sk_host_generate.argtypes = [C.POINTER(abi.SkyOptions), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(abi.SkyStats), C.c_void_p]
    L.sk_host_generate.restype = C.c_int
    L.sk_host_coverage.argtypes = [C.POINTER(abi.SkyOptions), C.c_uint32, C.c_uint32, C.c_void_p]
    L.sk_host_layout.argtypes = [C.POINTER(C.c_uint32 * 17)]
    return L


def options(**fields):
    """pt_sky_options with the defaults include/ptamd.h states, then `fields`."""
    o = abi.SkyOptions(0.5, 0.0, 0.004712, 1.0, 1, 0.001, 1.0, 1.0, 1.0, 0.3)
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def horizon_clear(altitude_km, h):
    """Does every texel centre of an h-row map lie at least HORIZON_CLEARANCE from the geometric horizon seen from this altitude?"""
    horizon = math.pi / 2 + math.acos(RG / (RG + altitude_km))
    rows = (np.arange(h) + 0.5) * math.pi / h
    return bool(np.all(np.abs(rows - horizon) >= HORIZON_CLEARANCE))


def case_options(name, w, h):
    """The option set `name` for a w x h map.  A map with a row of texel centres ON the horizon (an odd h) cannot be compared at the default
    altitude of one metre, whose horizon dips 0.56 mrad: such a map stands at ten metres (1.8 mrad) wherever the set leaves the altitude
    alone."""
    f = dict(OPTION_SETS[name])
    if "altitude_km" not in f and not horizon_clear(0.001, h):
        f["altitude_km"] = 0.01
    o = options(**f)
    assert horizon_clear(float(o.altitude_km), h), (name, w, h)
    return o


def host_sky(o, w, h):
    """pt_sky.h built for the host: (image (h, w, 4) float32, abi.SkyStats, flags (h, w) uint64)."""
    out = np.empty((h, w, 4), np.float32)
    flags = np.zeros((h, w), np.uint64)
    st = abi.SkyStats()
    assert lib().sk_host_generate(C.byref(o), w, h, out.ctypes.data, C.byref(st), flags.ctypes.data) == 0
    return out, st, flags


def host_coverage(o, w, h):
    out = np.zeros((h, w), np.uint32)
    lib().sk_host_coverage(C.byref(o), w, h, out.ctypes.data)
    return out


def layout():
    o = (C.c_uint32 * 17)()
    lib().sk_host_layout(C.byref(o))
    return list(o)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(axis=-1)


def _fn(f, x):
    """f(x) in x's own dtype.  For float32 it is the float64 result rounded once: the correctly rounded float32 value (but for a rare
    halfway case), whatever vector routine this numpy build would have picked for float32 -- the recorded figure must not move with it."""
    x = np.asarray(x)
    return f(x) if x.dtype == np.float64 else f(x.astype(np.float64)).astype(x.dtype)


def _dirs(w, h, fx, fy, dt):
    """(h, w, 3): uvToRayDir of ((x + fx) / w, (y + fy) / h)."""
    u = (np.arange(w, dtype=dt) + dt(fx)) / dt(w)
    v = (np.arange(h, dtype=dt) + dt(fy)) / dt(h)
    phi, th = (dt(2) * dt(np.pi)) * u[None, :], dt(np.pi) * v[:, None]
    st = _fn(np.sin, th)
    return np.stack([-_fn(np.cos, phi) * st, _fn(np.cos, th) + 0 * phi, -_fn(np.sin, phi) * st], axis=-1).astype(dt)


class _VectorRays:
    """Rays as the model states them: an origin vector, a unit direction, the quadratic of the sphere.  float64 only."""

    def __init__(self, P, D):
        self.P, self.D = P, D
        self.b = _dot(P, D)
        self.pp = _dot(P, P)

    def _disc(self, R):
        return self.b * self.b - (self.pp - R * R)

    def ground(self):
        return (self.b < 0) & (self._disc(RG) > 0)

    def t_top(self):
        return -self.b + np.sqrt(np.maximum(self._disc(RA), 0))

    def t_ground(self):
        return -self.b - np.sqrt(np.maximum(self._disc(RG), 0))

    def at(self, t):
        """Points at distance t: (height >= 0, toward(s) -> rays from them along s)."""
        Q = self.P + t[..., None] * self.D
        r = np.sqrt(_dot(Q, Q))
        return np.maximum(r - RG, 0), (lambda s: (_VectorRays(Q, np.broadcast_to(s, Q.shape)), _dot(Q, s) / r))


class _ScalarRays:
    """Rays by radius, height and the cosine to the local zenith, in the rearranged expressions of pt_sky.h's header comment (restated,
    not shared), in the dtype of its arguments; `ps0`, `mu` let a view ray give p.s along itself."""

    def __init__(self, r, h, mu, dt, ps0=None, mus=None):
        self.r, self.h, self.mu, self.dt, self.ps0, self.mus = r, h, mu, dt, ps0, mus
        sn = np.sqrt((dt(1) - mu) * (dt(1) + mu))
        q, e = r * sn, r * (mu * mu) / (dt(1) + sn)          # R - q = (R - r) + e, with R - r from the height
        self.ground2 = (e - h) * (dt(RG) + q)
        self.top2 = ((dt(RA - RG) - h) + e) * (dt(RA) + q)

    def ground(self):
        return (self.mu < 0) & (self.ground2 > 0)

    def t_top(self):
        return -self.r * self.mu + np.sqrt(np.maximum(self.top2, self.dt(0)))

    def t_ground(self):
        dt = self.dt
        with np.errstate(all="ignore"):
            return self.h * (self.r + dt(RG)) / (-self.r * self.mu + np.sqrt(np.maximum(self.ground2, dt(0))))

    def at(self, t):
        dt = self.dt
        w = t * (t + dt(2) * self.r * self.mu)
        rr = np.sqrt(self.r * self.r + w)
        hh = np.maximum(self.h + w / (rr + self.r), dt(0))

        def toward(s):
            mus = np.clip((self.ps0 + t * self.mus) / rr, dt(-1), dt(1))
            return _ScalarRays(rr, hh, mus, dt), mus
        return hh, toward


def _density(o, h, dt):
    """(..., 3): Rayleigh, Mie, ozone at height h."""
    return np.stack([dt(o.air_density) * _fn(np.exp, -h / dt(HR)), dt(o.dust_density) * _fn(np.exp, -h / dt(HM)),
                     dt(o.ozone_density) * np.maximum(dt(0), dt(1) - np.abs(h - dt(25)) / dt(15))], axis=-1)


def _transmittance(tau, dt):
    """(..., 3 depths) -> (..., 3 channels)"""
    bR, bO = np.array(BETA_R, dt), np.array(BETA_O, dt)
    return _fn(np.exp, -((bR * tau[..., 0:1] + dt(BETA_ME) * tau[..., 1:2]) + bO * tau[..., 2:3]))


def _sun_depth(o, rays, dt):
    """D (…, 3) and blocked (…) of rays towards the sun."""
    blocked = rays.ground()
    dl = rays.t_top() / dt(NL)
    D = np.zeros(dl.shape + (3,), dt)
    for j in range(NL):
        hj, _ = rays.at((dt(j) + dt(0.5)) * dl)
        D = D + _density(o, hj, dt) * dl[..., None]
    return D, blocked


def np_sky(o, w, h, dtype=np.float64):
    """The model of DESIGN.md §3m in `dtype` (the options are the struct's float32 values).  Returns a dict: img (h, w, 4), ground (h, w),
    blocked (h, w, NV + 1: the view steps, then the ray's end), coverage (h, w) in [0, 1], omega (the discrete solid angle of every texel,
    (h, w)), omega_d, t_view (h, w, 3: T(tau_view)), alpha_eff."""
    dt = np.dtype(dtype).type
    exact = dt is np.float64
    a, e = dt(f32(o.sun_azimuth)), dt(f32(o.sun_elevation))
    sa, ca, se, ce = (dt(_fn(f, v)) for f, v in ((np.sin, a), (np.cos, a), (np.sin, e), (np.cos, e)))
    s = np.array([-ca * ce, se, -sa * ce], dt)
    alt, I = dt(f32(o.altitude_km)), dt(f32(o.sun_intensity))
    r0 = dt(RG) + alt
    d = _dirs(w, h, 0.5, 0.5, dt)
    mu = _dot(d, s)
    if exact:
        view = _VectorRays(np.broadcast_to(np.array([0, r0, 0], dt), d.shape), d)
    else:
        view = _ScalarRays(np.broadcast_to(r0, mu.shape), np.broadcast_to(alt, mu.shape), d[..., 1], dt, ps0=r0 * s[1], mus=mu)
    ground = view.ground()
    with np.errstate(all="ignore"):
        t_end = np.where(ground, view.t_ground(), view.t_top())
    ds = t_end / dt(NV)
    tau = np.zeros(d.shape, dt)
    AR, AM = np.zeros(d.shape, dt), np.zeros(d.shape, dt)
    blocked_all = np.zeros(mu.shape + (NV + 1,), bool)
    for i in range(NV):
        hi, toward = view.at((dt(i) + dt(0.5)) * ds)
        rho = _density(o, hi, dt)
        D, blocked = _sun_depth(o, toward(s)[0], dt)
        blocked_all[..., i] = blocked
        T = _transmittance(tau + dt(0.5) * rho * ds[..., None] + D, dt)
        lit = np.where(blocked, dt(0), dt(1))
        AR = AR + T * (rho[..., 0] * ds * lit)[..., None]
        AM = AM + T * (rho[..., 1] * ds * lit)[..., None]
        tau = tau + rho * ds[..., None]
    PR = dt(3) / (dt(16) * dt(np.pi)) * (dt(1) + mu * mu)
    gb = dt(1) + dt(G) * dt(G) - dt(2) * dt(G) * mu
    PM = (dt(1) - dt(G) * dt(G)) / (dt(4) * dt(np.pi) * (gb * np.sqrt(gb)))
    L = I * (np.array(BETA_R, dt) * PR[..., None] * AR + dt(BETA_MS) * PM[..., None] * AM)
    Tv = _transmittance(tau, dt)
    # the ground
    _, toward = view.at(t_end)
    rays_end, ns = toward(s)
    De, blocked_end = _sun_depth(o, rays_end, dt)
    blocked_all[..., NV] = blocked_end
    c = np.where(ground & ~blocked_end, np.maximum(ns, dt(0)), dt(0))
    L = L + Tv * (dt(f32(o.ground_albedo)) / dt(np.pi) * I) * _transmittance(De, dt) * c[..., None]
    # the disc
    alpha = max(dt(f32(o.sun_angular_radius)), dt(np.pi) / dt(h))
    cov = np.zeros(mu.shape, dt)
    for j in range(4):
        for i in range(4):
            dsub = _dirs(w, h, (i + 0.5) / 4, (j + 0.5) / 4, dt)
            if exact:
                inside = _dot(dsub, s) >= np.cos(alpha)     # (float64)
            else:
                inside = _dot(dsub - s, dsub - s) <= (dt(2) * dt(_fn(np.sin, dt(0.5) * alpha))) ** 2
            cov = cov + inside
    cov = cov / dt(16)
    rows = np.arange(h + 1, dtype=np.float64) * np.pi / h
    omega = np.broadcast_to(((2 * np.pi / w) * (np.cos(rows[:-1]) - np.cos(rows[1:])))[:, None], mu.shape)
    omega_d = float((cov.astype(np.float64) * omega).sum())
    if o.sun_disc and omega_d > 0:
        L = L + np.where(ground, dt(0), cov)[..., None] * I * Tv / dt(omega_d)
    img = np.concatenate([L, np.ones(mu.shape + (1,), dt)], axis=-1)
    return dict(img=img, ground=ground, blocked=blocked_all, coverage=cov, omega=omega, omega_d=omega_d, t_view=Tv, alpha_eff=float(alpha), s=s)


@functools.lru_cache(maxsize=None)
def witness(name, w, h):
    """np_sky in float64 of case_options(name, w, h), computed once and left alone."""
    out = np_sky(case_options(name, w, h), w, h, np.float64)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def unpack_flags(flags):
    """sk_host_generate's flags -> (ground (h, w), blocked (h, w, NV + 1))"""
    ground = (flags & np.uint64(1)) != 0
    blocked = ((flags[..., None] >> np.arange(1, NV + 1, dtype=np.uint64)) & np.uint64(1)) != 0
    end = ((flags >> np.uint64(33)) & np.uint64(1)) != 0
    return ground, np.concatenate([blocked, end[..., None]], axis=-1)


def compared(ground, blocked, wit):
    """(h, w) mask of the texels whose decisions agree with the witness's.  The end's decision counts only on the ground (it is selected
    away elsewhere)."""
    steps = (blocked[..., :NV] == wit["blocked"][..., :NV]).all(axis=-1)
    end = ~wit["ground"] | (blocked[..., NV] == wit["blocked"][..., NV])
    return (ground == wit["ground"]) & steps & end


def rel_err(img, wit, mask):
    """The largest relative error per channel over the texels of `mask`; the denominator has the floor BOUNDS describes.  Alpha must be 1."""
    ref = wit["img"][..., :3]
    x = np.asarray(img, np.float64)
    assert np.all(x[..., 3] == 1.0)
    sky = ref[wit["coverage"] == 0]
    floor = FLOOR * (float(sky.max()) if sky.size and sky.max() > 0 else float(ref.max()) if ref.max() > 0 else 1.0)
    err = np.abs(x[..., :3] - ref) / np.maximum(np.abs(ref), floor)
    return float(err[mask].max()) if mask.any() else 0.0


def measure_float32_error():
    """(BOUNDS["measured"], the largest share of texels left out): np_sky in float32 against the witness over OPTION_SETS x HOST_SIZES."""
    worst, left = 0.0, 0.0
    for w, h in HOST_SIZES:
        for name in OPTION_SETS:
            wit = witness(name, w, h)
            lo = np_sky(case_options(name, w, h), w, h, np.float32)
            mask = compared(lo["ground"], lo["blocked"], wit)
            left = max(left, 1.0 - float(mask.mean()))
            worst = max(worst, rel_err(lo["img"], wit, mask))
    return worst, left
