"""Host side of the denoiser tests: the ctypes wrapper of the dn_* functions of the host harness (tests/host_build.py; the host build of
platinum_amd/csrc/pt_denoise.h, tests/emu/denoise_emu.cpp) and a float64 numpy restatement of the filter as DESIGN.md §3 states it.
TEST HARNESS, never imported by platinum_amd."""
import ctypes as C
import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
from platinum_amd import abi  # noqa: E402

import emu_lib  # noqa: E402

DEFAULTS = dict(iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0)


@functools.lru_cache(maxsize=None)
def lib():
    L = emu_lib.lib()   # (HostScene creates its scene with emu_create)
    L.dn_host_filter.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 4 + [C.c_float] * 3 + [C.c_void_p]
    L.dn_host_stage_aov.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dn_host_lum.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.dn_host_render.restype = C.c_uint64
    L.dn_host_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5
    L.dn_host_options_layout.argtypes = [C.POINTER(C.c_uint32 * 7)]
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def host_filter(acc, albedo, normal, moments, N, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0):
    """The filter's own arithmetic (pt_denoise.h) built for the host: (H, W, 4) float32 images in, (H, W, 4) float32 out."""
    acc, albedo, normal, moments = _f32(acc), _f32(albedo), _f32(normal), _f32(moments)
    H, W = acc.shape[:2]
    out = np.zeros((H, W, 4), dtype=np.float32)
    lib().dn_host_filter(acc.ctypes.data, albedo.ctypes.data, normal.ctypes.data, moments.ctypes.data, W, H, N, iterations,
                         sigma_l, sigma_n, sigma_z, out.ctypes.data)
    return out


def host_lum(rgba):
    rgba = _f32(rgba)
    n = rgba.size // 4
    lum, lum2 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    lib().dn_host_lum(rgba.ctypes.data, n, lum.ctypes.data, lum2.ctypes.data)
    return lum.reshape(rgba.shape[:-1]), lum2.reshape(rgba.shape[:-1])


class HostScene:
    """A scene on the host build (wavefront_emu.cpp's host BVH + the product's stage functions)."""

    def __init__(self, scene, params):
        self.L = lib()
        self.snapshot = scene.snapshot()
        blob = open(abi.LUT_PATH, "rb").read()
        self._blob = C.create_string_buffer(blob, len(blob))
        self.h = self.L.emu_create(C.byref(self.snapshot.struct), C.byref(params), self._blob, len(blob))
        if not self.h:
            raise RuntimeError("emu_create failed")
        self.W, self.H = params.width, params.height
        self.nonfinite = 0      # non-finite samples met by render() so far (under either params.nonfinite_policy)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.emu_destroy(self.h)
            self.h = None

    def stage_aov(self, sample, hits):
        """stage_aov on the given hit records ((H, W) structured array of pt_hit_record): ({albedo, t}, {normal, hit}) images."""
        hits = np.ascontiguousarray(hits)
        a = np.zeros((self.H, self.W, 4), np.float32)
        n = np.zeros((self.H, self.W, 4), np.float32)
        self.L.dn_host_stage_aov(self.h, sample, hits.ctypes.data, a.ctypes.data, n.ctypes.data)
        return a, n

    def render(self, first, ns, n0=0, into=None, nonfinite=None):
        """Samples [first, first + ns): (accumulator, albedo, normal, moments) as the device folds them, under the nonfinite_policy of the
        params the scene was created with.  `into` = four (H, W, 4) float32 images that already hold the running means of `n0` samples: the
        new samples are folded into them in place.  `nonfinite` = an (H, W) uint32 image, incremented where a sample was NaN / inf;
        self.nonfinite grows by their number."""
        imgs = [np.zeros((self.H, self.W, 4), np.float32) for _ in range(4)] if into is None else list(into)
        for i in imgs:
            assert i.dtype == np.float32 and i.shape == (self.H, self.W, 4) and i.flags.c_contiguous
        if nonfinite is not None:
            assert nonfinite.dtype == np.uint32 and nonfinite.shape == (self.H, self.W) and nonfinite.flags.c_contiguous
        self.nonfinite += self.L.dn_host_render(self.h, first, ns, n0, *[i.ctypes.data for i in imgs],
                                                None if nonfinite is None else nonfinite.ctypes.data)
        return imgs


# ---- float64 restatement of the filter (DESIGN.md §3 "Denoiser") -------------------------------------------------------------------
LUM = np.array([0.2126, 0.7152, 0.0722])


def _exp(x):
    # exp(x) = 2^(x log2 e), with the exponent floored at -125 (pt_denoise.h dn_exp2: a NaN argument counts as the floor too)
    y = x * np.log2(np.e)
    y = np.where(y > -125.0, y, -125.0)
    return np.exp2(y)


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside the image."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if H - abs(dy) > 0 and W - abs(dx) > 0:
        b[yd, xd] = a[ys, xs]
    return b


def np_filter(acc, albedo, normal, moments, N, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_z=1.0):
    acc, albedo, normal, moments = (np.asarray(x, np.float64) for x in (acc, albedo, normal, moments))
    H, W = acc.shape[:2]
    c = acc[..., :3]
    if iterations == 0:
        out = np.ones((H, W, 4))
        out[..., :3] = c
        return out
    a = albedo[..., :3]
    h = normal[..., 3]
    geo = h >= 0.5
    with np.errstate(all="ignore"):
        z = np.where(geo, moments[..., 0] / np.where(geo, h, 1.0), 0.0)
        nl = np.sqrt((normal[..., :3] ** 2).sum(-1))
        n = np.where((geo & (nl > 0))[..., None], normal[..., :3] / np.where(nl > 0, nl, 1.0)[..., None], 0.0)
        am = np.maximum(a, 1e-3)
        I = c / am
        la = np.maximum(a @ LUM, 1e-3)
        v = np.maximum(0.0, moments[..., 2] - moments[..., 1] ** 2) / (N * la * la)
        valid = np.isfinite(c).all(-1) & np.isfinite(I).all(-1) & np.isfinite(v)
    # depth gradient: central differences, one-sided at the border and next to background
    g = []
    for dy, dx in ((0, 1), (1, 0)):
        zp, hp = _shift(z, dy, dx, 0.0), _shift(geo, dy, dx, False)
        zm, hm = _shift(z, -dy, -dx, 0.0), _shift(geo, -dy, -dx, False)
        g.append(np.where(hm & hp, np.abs(zp - zm) * 0.5, np.where(hp, np.abs(zp - z), np.where(hm, np.abs(z - zm), 0.0))))
    gz = np.where(geo, np.maximum(g[0], g[1]), 0.0)
    I = np.where(valid[..., None], I, 0.0)
    v = np.where(valid, v, 0.0)
    k5 = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    k3 = [0.25, 0.5, 0.25]
    for it in range(iterations):
        s = 1 << it
        # 3x3 binomial blur of v over the valid pixels of the centre's class
        sw3 = np.zeros((H, W))
        sv3 = np.zeros((H, W))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vq, okq, gq = _shift(v, dy, dx, 0.0), _shift(valid, dy, dx, False), _shift(geo, dy, dx, False)
                inside = _shift(np.ones((H, W), bool), dy, dx, False)
                use = inside & okq & (gq == geo)
                w = k3[dx + 1] * k3[dy + 1]
                sw3 += np.where(use, w, 0.0)
                sv3 += np.where(use, w * vq, 0.0)
        with np.errstate(all="ignore"):
            dl = sigma_l * np.sqrt(sv3 / sw3) + 1e-6
        lp = I @ LUM
        sw = np.zeros((H, W))
        sI = np.zeros((H, W, 3))
        sv = np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                inside = _shift(np.ones((H, W), bool), dy * s, dx * s, False)
                okq = _shift(valid, dy * s, dx * s, False)
                gq = _shift(geo, dy * s, dx * s, False)
                use = inside & okq & (gq == geo)
                Iq, vq = _shift(I, dy * s, dx * s, 0.0), _shift(v, dy * s, dx * s, 0.0)
                nq, zq = _shift(n, dy * s, dx * s, 0.0), _shift(z, dy * s, dx * s, 0.0)
                with np.errstate(all="ignore"):
                    d = np.maximum(0.0, (n * nq).sum(-1))
                    wn = np.where(d > 0, np.exp2(np.maximum(sigma_n * np.log2(np.where(d > 0, d, 1.0)), -125.0)), 0.0)
                    wz = _exp(-(np.abs(z - zq) / (sigma_z * gz * s * np.sqrt(dx * dx + dy * dy) + 1e-6)))
                    wn = np.where(geo, wn, 1.0)
                    wz = np.where(geo, wz, 1.0)
                    wl = _exp(-(np.abs(lp - Iq @ LUM) / dl))
                w = np.where(use, k5[dx + 2] * k5[dy + 2] * wn * wz * wl, 0.0)
                sw += w
                sI += w[..., None] * Iq
                sv += w * w * vq
        with np.errstate(all="ignore"):
            keep = (sw > 0) & valid
            I = np.where(keep[..., None], sI / np.where(keep, sw, 1.0)[..., None], I)
            v = np.where(keep, sv / np.where(keep, sw * sw, 1.0), v)
    out = np.ones((H, W, 4))
    out[..., :3] = np.where(valid[..., None], I * am, c)
    return out


def options_layout():
    o = (C.c_uint32 * 7)()
    lib().dn_host_options_layout(C.byref(o))
    return list(o)
