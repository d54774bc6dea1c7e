"""The selection overlay without a GPU: the host build of pt_selection.h (tests/emu/selection_emu.cpp), per pixel and block
by block as the kernel stages it, against each other and against an independent float32 numpy restatement, byte for byte; the properties
the arithmetic promises on the bits; the tile map enumerated; the ABI through libptamd.so; and a stand-alone sanitizer build of the host
code."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import selection_lib as sl
from platinum_amd import abi

f32 = np.float32
INVALID = -1


def _set(name, width=2.0):
    return sl.options(width=width, **sl.OPTION_SETS[name])


# ---- radius and weight ---------------------------------------------------------------------------------------------------------------------
def test_radius_and_weight():
    assert [sl.lib().sel_host_radius(w) for w in (1.0, 1.5, 2.0, 16.0)] == [1, 1, 2, 16]
    for w in sl.WIDTHS:
        R = sl.lib().sel_host_radius(w)
        assert R == sl.RADII[w] == sl.np_radius(w)
        for dy in range(-R - 1, R + 2):
            for dx in range(-R - 1, R + 2):
                k = sl.lib().sel_host_weight(w, dx, dy)
                assert f32(k).view(np.uint32) == sl.np_weight(w, dx, dy).view(np.uint32), (w, dx, dy)
                if max(abs(dx), abs(dy)) > R:
                    assert k == 0.0      # nothing outside the square of taps has a weight: the square holds the whole disc
        assert sl.lib().sel_host_weight(w, 0, 0) == 1.0


# ---- the two host paths and the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", sl.WIDTHS)
@pytest.mark.parametrize("W,H", sl.SIZES)
def test_host_paths_and_the_numpy_restatement_agree_byte_for_byte(W, H, width):
    checked = early = tint = 0
    for cname in sl.COVERAGE_CARDS:
        cov = sl.coverage_card(cname, W, H)
        D = sl.card_dilation(cname, W, H, width)
        for tname in sl.TARGET_CARDS:
            target = sl.target_card(tname, W, H)
            for setname in sl.OPTION_SETS:
                o = _set(setname, width)
                what = "%s on %s, %dx%d, width %g, %s" % (cname, tname, W, H, width, setname)
                a = sl.host_overlay(target, cov, o)
                b, blocks = sl.host_overlay_blocks(target, cov, o)
                c, _ = sl.host_overlay_blocks(target, cov, o, early_out=False)
                ref = sl.np_overlay(target, cov, o, D)
                assert np.array_equal(a, b), what + ": block by block against per pixel"
                assert np.array_equal(a, c), what + ": without the early out"
                bad = (a != ref).any(axis=-1)
                assert not bad.any(), "%s: %d pixels differ from numpy, first (y, x) %s: host %s, numpy %s" % (
                    what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), a[bad][:2].tolist(), ref[bad][:2].tolist())
                assert np.array_equal(a[..., 3], target[..., 3])
                nb = ((W + 15) // 16) * ((H + 15) // 16)
                assert blocks[0] == nb
                if cname == "empty":
                    assert blocks[1] == nb and np.array_equal(a, target)
                if cname == "halo_only" and W > sl.BLOCK:
                    assert blocks[1] <= nb - 2      # neither the covered pixel's block nor block (0, 0), which sees it in its halo only
                checked += 1
                early += blocks[1]
                tint += blocks[2]
    print("%dx%d width %g: %d combinations, %d blocks returned early, %d tinted only" % (W, H, width, checked, early, tint))


# ---- properties, on the bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", sl.WIDTHS)
def test_a_single_pixel_gives_the_disc_of_weights_as_outline_alpha(width):
    W, H = 67, 45
    cov = sl.coverage_card("centre", W, H)
    af, ao = sl.host_alphas(cov, sl.options(width=width, fill_rgba=sl.BLUE + (1.0,)))
    cy, cx = H // 2, W // 2
    R = sl.RADII[width]
    for y in range(H):
        for x in range(W):
            dx, dy = x - cx, y - cy
            if (dx, dy) == (0, 0):
                assert af[y, x] == 1.0 and ao[y, x] == 0.0
            else:
                k = sl.np_weight(width, dx, dy) if max(abs(dx), abs(dy)) <= R else f32(0)
                assert af[y, x] == 0.0 and f32(ao[y, x]).view(np.uint32) == f32(k).view(np.uint32), (x, y)


def test_alpha_one_gives_the_packed_colour_and_alpha_zero_keeps_the_bytes():
    """Alpha 1 gives pp_pack_rgba8(colour) exactly; both alphas 0 keep every byte, whatever the coverage."""
    W, H = 33, 31
    target = sl.target_card("random", W, H)
    cov = sl.coverage_card("halfplane", W, H)      # 1 from x = 16 on
    fill, outline = (0.2, 0.4, 1.0), (0.1, 0.9, 0.3)
    out = sl.host_overlay(target, cov, sl.options(width=2.0, fill_rgba=fill + (1.0,), outline_rgba=outline + (1.0,)))

    def packed(rgb):
        v = sl.host_pack(rgb)
        assert v >> 24 == 255
        return [v & 255, (v >> 8) & 255, (v >> 16) & 255]

    assert (out[:, 16:, :3] == packed(fill)).all()                       # fill alpha 1 * coverage 1
    assert (out[:, 15, :3] == packed(outline)).all()                     # k(1, 0) = 1: D = 1 over m = 0, outline alpha 1
    assert (out[:, 14] != target[:, 14]).any()                           # k(2, 0) = 0.5: a blend
    assert np.array_equal(out[:, :14], target[:, :14])                   # farther than R = 2 from any covered pixel
    assert np.array_equal(out[..., 3], target[..., 3])
    both0 = sl.options(width=16.0, fill_rgba=fill + (0.0,), outline_rgba=outline + (0.0,))
    for cname in sl.COVERAGE_CARDS:
        assert np.array_equal(sl.host_overlay(target, sl.coverage_card(cname, W, H), both0), target)


def test_a_block_that_sees_coverage_in_its_halo_only_still_draws():
    for width in sl.WIDTHS:
        cov = sl.coverage_card("halo_only", 33, 31)                      # pixel (16, 0) alone
        assert np.count_nonzero(cov) == 1 and cov[0, sl.BLOCK] > 0
        target = sl.target_card("white", 33, 31)
        out, blocks = sl.host_overlay_blocks(target, cov, sl.options(width=width))
        assert (out[0, sl.BLOCK - 1] != target[0, sl.BLOCK - 1]).any()   # in block (0, 0), one step from the covered pixel
        assert blocks[1] <= blocks[0] - 2


@pytest.mark.parametrize("width", sl.WIDTHS)
def test_untouched_pixels_and_the_full_card(width):
    W, H = 67, 45
    R = sl.RADII[width]
    o = sl.options(width=width, fill_rgba=sl.BLUE + (0.5,))
    for tname in sl.TARGET_CARDS:
        target = sl.target_card(tname, W, H)
        assert np.array_equal(sl.host_overlay(target, sl.coverage_card("empty", W, H), o), target)
        # the full card: D = m = 1 everywhere, no outline anywhere, the tint alone
        af, ao = sl.host_alphas(sl.coverage_card("full", W, H), o)
        assert not ao.any() and (af == 0.5).all()
        no_outline = sl.options(width=width, fill_rgba=sl.BLUE + (0.5,), outline_rgba=(0.0, 1.0, 0.0, 0.0))
        assert np.array_equal(sl.host_overlay(target, sl.coverage_card("full", W, H), o), sl.host_overlay(target, sl.coverage_card("full", W, H), no_outline))
        # farther than R (Chebyshev) from every covered pixel: the bytes are kept
        cov = sl.coverage_card("corners", W, H)
        out = sl.host_overlay(target, cov, o)
        ys, xs = np.nonzero(cov)
        far = np.ones((H, W), bool)
        for y, x in zip(ys, xs):
            far[max(0, y - R):y + R + 1, max(0, x - R):x + R + 1] = False
        assert np.array_equal(out[far], target[far]) and (width == 16.0 or far.any())
        assert (out[..., 3] == target[..., 3]).all()
        if tname == "white":
            assert (out[..., 3] == 255).all()


def test_byte_round_trip_of_the_quantiser():
    """q(byte / 255) == byte for all 256 bytes: a pixel that is composited with weights that leave it alone keeps its bytes."""
    for b in range(256):
        v = f32(b) / f32(255)
        assert sl.host_pack((v, v, v)) == (b | b << 8 | b << 16 | 255 << 24)


# ---- the tile map --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", sl.SIZES)
def test_the_tile_map_enumerated(W, H):
    L = sl.lib()
    B = L.sel_host_block()
    assert B == sl.BLOCK
    xy = (C.c_uint32 * 2)()
    for R in sorted(set(sl.RADII.values())):
        T = B + 2 * R
        assert T * T <= 48 * 48
        for by in range((H + B - 1) // B):
            for bx in range((W + B - 1) // B):
                seen = set()
                for t in range(T * T):
                    tx, ty = t % T, t // T
                    x, y = bx * B + tx - R, by * B + ty - R
                    inside = L.sel_host_tile_pixel(bx, by, R, t, W, H, xy)
                    assert bool(inside) == (0 <= x < W and 0 <= y < H), (bx, by, R, t)
                    if inside:
                        assert (xy[0], xy[1]) == (x, y)
                        seen.add((x, y))
                # every in-image pixel within R of the block is staged exactly once
                want = {(x, y) for y in range(max(0, by * B - R), min(H, by * B + B + R)) for x in range(max(0, bx * B - R), min(W, bx * B + B + R))}
                assert seen == want
        # a lane's taps stay inside the tile, and the centre is the lane's own pixel
        for lx, ly in ((0, 0), (B - 1, 0), (0, B - 1), (B - 1, B - 1), (7, 9)):
            for dx, dy in ((-R, -R), (R, -R), (-R, R), (R, R), (0, 0)):
                a = L.sel_host_tile_texel(R, lx, ly, dx, dy)
                assert a < T * T and (a % T, a // T) == (lx + R + dx, ly + R + dy)


# ---- validation and surface ----------------------------------------------------------------------------------------------------------------
def test_selection_options_abi():
    lay = sl.layout()
    O = abi.SelectionOptions
    assert lay[0] == C.sizeof(O) == 48
    assert lay[1:7] == [getattr(O, n).offset for n, _ in O._fields_] == [0, 4, 8, 12, 16, 32]
    assert lay[7:] == [16, 16, 48, 33]
    assert (48 * 48 + 33 * 33) * 4 <= 16384
    lib = abi.load_library()
    o = O(7, 7, 7.0, 7.0, (C.c_float * 4)(7, 7, 7, 7), (C.c_float * 4)(7, 7, 7, 7))
    lib.pt_default_selection_options(C.byref(o))
    d = sl.options()
    assert bytes(o) == bytes(d)
    assert (o.enabled, o.layer, o.width, o._pad) == (0, abi.MATTE_INSTANCE, 2.0, 0.0)
    assert list(o.outline_rgba) == [1.0, f32(0.55), 0.0, 1.0] and list(o.fill_rgba) == [1.0, f32(0.55), 0.0, 0.0]
    lib.pt_default_selection_options(None)


NAN, INF = float("nan"), float("inf")
GOOD = [{}, dict(enabled=1), dict(layer=abi.MATTE_MATERIAL), dict(width=1.0), dict(width=16.0), dict(width=7.25),
        dict(outline_rgba=(0.0, 0.0, 0.0, 0.0)), dict(fill_rgba=(1.0, 1.0, 1.0, 1.0))]
BAD = [(dict(layer=2), b"layer"), (dict(layer=0xFFFFFFFF), b"layer"),
       (dict(width=0.99), b"width"), (dict(width=16.01), b"width"), (dict(width=NAN), b"width"), (dict(width=INF), b"width"), (dict(width=-2.0), b"width")]
for _field in ("outline_rgba", "fill_rgba"):
    for _k in range(4):
        for _v in (-0.01, 1.01, NAN, INF, -INF):
            _c = [0.5, 0.5, 0.5, 0.5]
            _c[_k] = _v
            BAD.append(({_field: tuple(_c)}, _field.encode()))


def test_validation_before_the_renderer():
    """The options are checked before the renderer: a valid struct reaches the null-renderer test, an invalid one does not."""
    lib = abi.load_library()
    img = np.zeros((2, 2, 4), np.uint8)
    cov = np.zeros((2, 2), np.float32)
    out = np.zeros((2, 2, 4), np.uint8)
    dbg = lambda o, a=img, c=cov, w=2, h=2, res=out: lib.pt_debug_selection_overlay(
        None, None if a is None else a.ctypes.data, None if c is None else c.ctypes.data, w, h, None if o is None else C.byref(o),
        None if res is None else res.ctypes.data)
    for f in GOOD:
        o = sl.options(**f)
        assert sl.lib().sel_host_options_valid(C.byref(o)) == 1
        assert lib.pt_set_selection_options(None, C.byref(o)) == INVALID and b"null renderer" in lib.pt_last_error(), f
        assert dbg(o) == INVALID and b"null renderer" in lib.pt_last_error(), f
    for f, word in BAD:
        for en in (0, 1):
            o = sl.options(**f)
            o.enabled = en
            assert sl.lib().sel_host_options_valid(C.byref(o)) == 0, f
            assert lib.pt_set_selection_options(None, C.byref(o)) == INVALID and word in lib.pt_last_error(), f
            assert dbg(o) == INVALID and word in lib.pt_last_error(), f
    o = sl.options()
    assert lib.pt_set_selection_options(None, None) == INVALID
    assert dbg(None) == INVALID and dbg(o, a=None) == INVALID and dbg(o, c=None) == INVALID and dbg(o, res=None) == INVALID
    assert dbg(o, w=0) == INVALID and b"pixels" in lib.pt_last_error()
    assert dbg(o, w=1 << 15, h=(1 << 13) + 1) == INVALID and b"pixels" in lib.pt_last_error()
    ids = np.array([1, 2], np.uint32)
    n = C.c_uint32()
    assert lib.pt_set_selection(None, ids.ctypes.data, 2) == INVALID
    assert lib.pt_set_selection(None, None, 0) == INVALID
    assert lib.pt_get_selection(None, ids.ctypes.data, 2, C.byref(n)) == INVALID
    from platinum_amd.renderer import Renderer
    for member in ("selectionOptions", "setSelectionOptions", "setSelection", "selection", "debugSelectionOverlay"):
        assert callable(getattr(Renderer, member)), member


# ---- the host code under sanitizers, stand-alone -------------------------------------------------------------------------------------------
def test_host_build_runs_clean_under_asan_and_ubsan_as_a_program_of_its_own(tmp_path):
    """tests/emu/selection_emu.cpp with its own main: both host paths over the sizes and widths above, the LDS arrays at their real size.
    (Nothing loaded into Python runs under a sanitizer.)"""
    exe = tmp_path / "selection_emu_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DSELECTION_EMU_MAIN", "-o", str(exe), sl.SRC])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, (p.returncode, p.stderr[-2000:])
    assert "300 x 3, width 16 (R 16), card 3" in p.stdout and "1 x 1, width 1 (R 1), card 0" in p.stdout
