"""Host side of the selection-overlay tests: the ctypes wrapper of tests/emu/selection_emu.cpp (the host build of
pt_selection.h, per pixel and block by block as the kernel stages it; a library of its own built by tests/host_build.py), an independent
float32 numpy restatement (whole-image shifted arrays and np.maximum: no code shared with the header) and the test cards.  TEST HARNESS,
never imported by platinum_amd."""
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

SRC = os.path.join(_ROOT, "tests", "emu", "selection_emu.cpp")
LIB = os.path.join(_ROOT, "tests", "_build", "libptamd_selection.so")
f32 = np.float32
BLOCK = 16

# 1x1 .. 3x2: smaller than any halo; 16x16, 17x15: one block, a partial second one; 33x31: three blocks a side; 67x45; 300x3: many blocks in
# a row under a halo taller than the image
SIZES = [(1, 1), (2, 1), (1, 7), (3, 2), (16, 16), (17, 15), (33, 31), (67, 45), (300, 3)]   # (W, H)
WIDTHS = [1.0, 1.5, 2.0, 7.25, 16.0]      # R = 1, 1, 2, 7, 16: 16 is a halo wider than a block and than most of these images
RADII = {1.0: 1, 1.5: 1, 2.0: 2, 7.25: 7, 16.0: 16}
COVERAGE_CARDS = ("empty", "full", "centre", "corners", "halfplane", "checker", "random", "halo_only")
TARGET_CARDS = ("random", "white")
BLUE = (0.2, 0.4, 1.0)
OPTION_SETS = {
    "defaults": {},
    "fill-half": dict(fill_rgba=BLUE + (0.5,)),
    "outline-0.3": dict(outline_rgba=(1.0, 0.55, 0.0, 0.3)),
    "both-1": dict(fill_rgba=BLUE + (1.0,), outline_rgba=(0.1, 0.9, 0.3, 1.0)),
    "both-0": dict(fill_rgba=BLUE + (0.0,), outline_rgba=(1.0, 0.55, 0.0, 0.0)),
}


@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load(src=SRC, lib=LIB)
    O = C.POINTER(abi.SelectionOptions)
    L.sel_host_radius.argtypes = [C.c_float]
    L.sel_host_radius.restype = C.c_int32
    L.sel_host_weight.argtypes = [C.c_float, C.c_int32, C.c_int32]
    L.sel_host_weight.restype = C.c_float
    L.sel_host_options_valid.argtypes = [O]
    L.sel_host_options_valid.restype = C.c_uint32
    L.sel_host_pack.argtypes = [C.c_void_p]
    L.sel_host_pack.restype = C.c_uint32
    L.sel_host_block.restype = C.c_uint32
    L.sel_host_tile_pixel.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.sel_host_tile_pixel.restype = C.c_uint32
    L.sel_host_tile_texel.argtypes = [C.c_int32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32]
    L.sel_host_tile_texel.restype = C.c_uint32
    L.sel_host_alphas.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, O, C.c_void_p, C.c_void_p]
    L.sel_host_overlay.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, O, C.c_void_p]
    L.sel_host_overlay_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, O, C.c_uint32, C.c_void_p, C.c_void_p]
    L.sel_host_overlay_blocks.restype = C.c_int32
    L.sel_host_layout.argtypes = [C.POINTER(C.c_uint32 * 11)]
    return L


def options(**fields):
    """pt_selection_options with the defaults DESIGN.md §3h states, then `fields` (a colour as a 4-tuple)."""
    o = abi.SelectionOptions(0, abi.MATTE_INSTANCE, 2.0, 0.0, (C.c_float * 4)(1.0, 0.55, 0.0, 1.0), (C.c_float * 4)(1.0, 0.55, 0.0, 0.0))
    for k, v in fields.items():
        setattr(o, k, (C.c_float * 4)(*v) if k in ("outline_rgba", "fill_rgba") else v)
    return o


def _args(rgba8, cov):
    img = np.ascontiguousarray(rgba8, dtype=np.uint8)
    cov = np.ascontiguousarray(cov, dtype=np.float32)
    H, W = cov.shape
    assert img.shape == (H, W, 4)
    return img, cov, W, H


def host_overlay(rgba8, cov, o=None):
    """pt_selection.h built for the host, the per-pixel definition: (H, W, 4) uint8 target and (H, W) float32 coverage -> the target drawn."""
    img, cov, W, H = _args(rgba8, cov)
    o = options() if o is None else o
    out = np.empty_like(img)
    lib().sel_host_overlay(img.ctypes.data, cov.ctypes.data, W, H, C.byref(o), out.ctypes.data)
    return out


def host_overlay_blocks(rgba8, cov, o=None, early_out=True):
    """The same block by block as k_selection_overlay stages it: (target, (blocks, returned early, tint only))."""
    img, cov, W, H = _args(rgba8, cov)
    o = options() if o is None else o
    out = np.empty_like(img)
    blocks = np.zeros(3, np.uint32)
    rc = lib().sel_host_overlay_blocks(img.ctypes.data, cov.ctypes.data, W, H, C.byref(o), 1 if early_out else 0, out.ctypes.data, blocks.ctypes.data)
    assert rc == 0, "an address fell outside the tile or the weight table"
    return out, tuple(int(b) for b in blocks)


def host_alphas(cov, o=None):
    """(fill alpha, outline alpha), each (H, W) float32, by the definition."""
    cov = np.ascontiguousarray(cov, dtype=np.float32)
    H, W = cov.shape
    o = options() if o is None else o
    af, ao = np.empty((H, W), np.float32), np.empty((H, W), np.float32)
    lib().sel_host_alphas(cov.ctypes.data, W, H, C.byref(o), af.ctypes.data, ao.ctypes.data)
    return af, ao


def host_pack(rgb):
    a = np.array(rgb, np.float32)
    return int(lib().sel_host_pack(a.ctypes.data))


def layout():
    o = (C.c_uint32 * 11)()
    lib().sel_host_layout(C.byref(o))
    return list(o)


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------------------
def np_radius(width):
    lim = f32(width) + f32(0.5)
    return int(np.ceil(lim)) - 1


def np_weight(width, dx, dy):
    lim = f32(width) + f32(0.5)
    return f32(min(max(f32(lim - np.sqrt(f32(dx * dx + dy * dy))), f32(0)), f32(1)))


def np_dilate(cov, width):
    """D: the running np.maximum over the (2R + 1)^2 whole-image shifts of the zero-padded coverage, each times its weight."""
    m = np.asarray(cov, np.float32)
    H, W = m.shape
    R = np_radius(width)
    pad = np.zeros((H + 2 * R, W + 2 * R), np.float32)
    pad[R:R + H, R:R + W] = m
    D = np.zeros((H, W), np.float32)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            k = np_weight(width, dx, dy)
            if k > 0:       # (a zero weight contributes max(D, 0) = D)
                D = np.maximum(D, pad[R + dy:R + dy + H, R + dx:R + dx + W] * k)
    return D


def np_overlay(rgba8, cov, o, D=None):
    """The whole arithmetic of DESIGN.md §3h in float32 on an (H, W, 4) uint8 target; D may be handed in (np_dilate of cov at o.width)."""
    img = np.asarray(rgba8, np.uint8)
    m = np.asarray(cov, np.float32)
    D = np_dilate(m, o.width) if D is None else D
    fill, outline = np.array(list(o.fill_rgba), np.float32), np.array(list(o.outline_rgba), np.float32)
    af = (m * fill[3])[..., None]
    ao = ((D - m) * outline[3])[..., None]
    c = img[..., :3].astype(np.float32) / f32(255)
    c1 = c * (f32(1) - af) + fill[:3] * af
    c2 = c1 * (f32(1) - ao) + outline[:3] * ao
    assert c2.dtype == np.float32
    with np.errstate(invalid="ignore"):
        q = np.where(~(c2 > 0), 0, np.where(c2 >= 1, 255, (np.clip(c2, f32(0), f32(1)) * f32(255) + f32(0.5)).astype(np.uint32))).astype(np.uint8)
    out = img.copy()
    drawn = ~((af[..., 0] == 0) & (ao[..., 0] == 0))
    out[drawn, :3] = q[drawn]
    return out


def pixel_classes(cov, o):
    """(fully covered, outline only, fractional, untouched) boolean maps of the restatement's alphas with fill alpha taken as 1."""
    m = np.asarray(cov, np.float32)
    D = np_dilate(m, o.width)
    return m == 1, (m == 0) & (D > 0), (m > 0) & (m < 1), (m == 0) & (D == 0)


# ---- the cards -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coverage_card(name, W, H):
    """A read-only (H, W) float32 coverage card, computed once."""
    rng = np.random.default_rng(7000 * W + H)
    m = np.zeros((H, W), np.float32)
    if name == "empty":
        pass
    elif name == "full":
        m[:] = 1
    elif name == "centre":
        m[H // 2, W // 2] = 1
    elif name == "corners":
        m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = 1
    elif name == "halfplane":       # the edge lies on the first block border where the image has one
        m[:, (BLOCK if W > BLOCK else W // 2):] = 1
    elif name == "checker":
        m[(np.add.outer(np.arange(H), np.arange(W)) & 1) == 0] = 1
    elif name == "random":
        m[:] = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    elif name == "halo_only":       # one pixel of block (1, 0) (or (0, 1)): block (0, 0) sees coverage in its halo only
        if W > BLOCK:
            m[0, BLOCK] = 0.75
        elif H > BLOCK:
            m[BLOCK, 0] = 0.75
        else:
            m[H - 1, W - 1] = 0.75
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def target_card(name, W, H):
    """A read-only (H, W, 4) uint8 target card: random bytes (alpha included: the overlay never changes it) or all 255."""
    if name == "random":
        t = np.random.default_rng(9000 * W + H).integers(0, 256, (H, W, 4), dtype=np.uint8)
    elif name == "white":
        t = np.full((H, W, 4), 255, np.uint8)
    else:
        raise KeyError(name)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def card_dilation(name, W, H, width):
    D = np_dilate(coverage_card(name, W, H), width)
    D.setflags(write=False)
    return D
