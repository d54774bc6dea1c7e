"""Host side of the render-region tests: reference_region_render, a whole region render on the host, adaptive or
uniform, built from what exists (denoise_lib.HostScene renders, adaptive_lib.host_error judges), and the numpy enumeration of the
tiles a rectangle touches; the ctypes wrapper of the rg_* functions of the host harness (tests/host_build.py,
tests/emu/region_emu.cpp).  No GPU in the loop.  TEST HARNESS, never imported by platinum_amd."""
import ctypes as C
import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import adaptive_lib as al  # noqa: E402
import host_build  # noqa: E402


@functools.lru_cache(maxsize=None)
def lib():
    """tests/emu/region_emu.cpp built for the host (part of the one harness library)."""
    L = host_build.load()
    L.rg_host_region_layout.argtypes = [C.POINTER(C.c_uint32 * 6)]
    L.rg_host_mask.argtypes = [C.c_uint32] * 6 + [C.c_void_p]
    return L


def region_layout():
    o = (C.c_uint32 * 6)()
    lib().rg_host_region_layout(C.byref(o))
    return list(o)


def host_mask(W, H, rect):
    """(H, W) bool: pt_layout.h rect_contains, the kernels' validity test, built for the host."""
    out = np.zeros((H, W), np.uint8)
    lib().rg_host_mask(W, H, *rect, out.ctypes.data)
    return out.astype(bool)


# the rectangles (x0, y0, x1, y1) the adaptive configurations of adaptive_lib.CONFIGS / NONFINITE_CONFIGS are rendered with
REGIONS = {
    "cornell67": (5, 3, 45, 30),
    "textured99": (11, 5, 90, 50),
    "nan996": (5, 3, 70, 44),
}


def np_region_tiles(W, H, rect):
    """The 8x8 image tiles (row-major) that hold a pixel of rect = (x0, y0, x1, y1), ascending: a plain enumeration over the pixels."""
    x0, y0, x1, y1 = rect
    inside = np.zeros((H, W), bool)
    inside[y0:y1, x0:x1] = True
    tx = (W + 7) // 8
    ys, xs = np.nonzero(inside)
    return np.unique((ys // 8) * tx + xs // 8).astype(np.uint32)


def mask(W, H, rect):
    x0, y0, x1, y1 = rect
    m = np.zeros((H, W), bool)
    m[y0:y1, x0:x1] = True
    return m


def tile_slices(W, H, rect):
    """{(ty, tx): (slice y, slice x)} of every tile rect touches: the tile's pixels inside rect."""
    x0, y0, x1, y1 = rect
    out = {}
    for ty in range(y0 // 8, (y1 - 1) // 8 + 1):
        for tx in range(x0 // 8, (x1 - 1) // 8 + 1):
            out[(ty, tx)] = (slice(max(y0, ty * 8), min(y1, ty * 8 + 8)), slice(max(x0, tx * 8), min(x1, tx * 8 + 8)))
    return out


def region_render(scene, params, rect, threshold=None, min_spp=None, interval=None, info=None):
    """The render of `scene` under `params` restricted to rect on the host.  With a threshold it samples adaptively: samples are folded
    cumulatively, adaptive_lib.host_error(m1, m2, n) <= threshold judges each pixel at every checkpoint below spp (a NaN is not converged),
    a tile of the rectangle converges when all its pixels inside the rectangle do, and its accumulator, AOVs and count freeze there, as in
    adaptive_lib.reference_render.  Everything outside the rectangle is zero.  Returns (counts, acc, albedo, normal, moments); `info`
    receives "nonfinite", the NaN / inf samples drawn per pixel."""
    import denoise_lib as dl
    hs = dl.HostScene(scene, params)
    H, W = hs.H, hs.W
    spp, first = int(params.spp), int(params.first_sample)
    live = [np.zeros((H, W, 4), np.float32) for _ in range(4)]
    out = [np.zeros((H, W, 4), np.float32) for _ in range(4)]
    counts = np.zeros((H, W), np.uint32)
    live_nf, out_nf = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
    active = dict(tile_slices(W, H, rect))

    def freeze(keys, n):
        for k in keys:
            s = active.pop(k)
            counts[s] = n
            for o, l in zip(out + [out_nf], live + [live_nf]):
                o[s] = l[s]

    done = 0
    cps = al.checkpoints(spp, min_spp, interval) if threshold is not None else []
    for c in cps + [spp]:
        if not active:
            break
        hs.render(first + done, c - done, n0=done, into=live, nonfinite=live_nf)
        done = c
        if c < spp:
            with np.errstate(invalid="ignore"):
                ok = al.host_error(live[3][..., 1], live[3][..., 2], c) <= np.float32(threshold)   # (a NaN error compares false)
            freeze([k for k, s in active.items() if ok[s].all()], c)
    freeze(list(active), spp)
    if info is not None:
        info["nonfinite"] = out_nf
    return (counts,) + tuple(out)


@functools.lru_cache(maxsize=None)
def reference_region_render(name, rect=None):
    """region_render of adaptive_lib's configuration `name` with rect (default REGIONS[name]), once per process: a dict of counts / acc /
    albedo / normal / moments / nonfinite (read only) and paths, the paths the render starts."""
    rect = REGIONS[name] if rect is None else tuple(rect)
    kind, _size, _B, _spp, m, i, thr, _policy = al.config(name)
    info = {}
    out = region_render(al.config_scene(kind), al.config_params(name), rect, thr, m, i, info=info)
    for a in out + (info["nonfinite"],):
        a.flags.writeable = False
    return dict(zip(("counts", "acc", "albedo", "normal", "moments"), out), nonfinite=info["nonfinite"], paths=int(out[0].astype(np.uint64).sum()))


def tile_count_map(W, H, rect, counts):
    """{(ty, tx): count} of the tiles rect touches (every pixel of a tile inside rect holds the tile's count: asserted)."""
    out = {}
    for k, s in tile_slices(W, H, rect).items():
        v = np.unique(counts[s])
        assert v.size == 1, (k, v)
        out[k] = int(v[0])
    return out
