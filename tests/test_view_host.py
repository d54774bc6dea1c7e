"""Pass views without a GPU: the host build of pt_view.h (tests/emu/view_emu.cpp) against an independent float32 numpy
restatement of every data view, byte for byte, on crafted cards; the range over a rectangle; the id hash against Python integers; every
validation error and its order; the ABI through libptamd.so; and a stand-alone sanitizer build of the host code."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import view_lib as vl
from platinum_amd import abi

f32 = np.float32
INVALID = -1
NAN, INF = float("nan"), float("inf")


def _check(inp, fields, rect=None):
    o = vl.options(**fields)
    a, sa = vl.host_view(inp, o, rect)
    b, sb = vl.np_view(inp, o, rect)
    assert np.array_equal(a, b), (fields, vl.first_difference(a, b))
    assert vl.same_stats(sa, sb), (fields, sa, sb)
    return a, sa


# ---- the host build against the numpy restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", vl.DATA_VIEWS, ids=[abi.VIEW_NAMES[v] for v in vl.DATA_VIEWS])
@pytest.mark.parametrize("size,kind,first", vl.cases(), ids=["%dx%d-%s-%d" % (s + (k, f)) for s, k, f in vl.cases()])
def test_host_build_equals_the_numpy_restatement_byte_for_byte(size, kind, first, view):
    inp = vl.card(size, kind, first)
    for fields in vl.option_sets(view):
        img, stats = _check(inp, fields)
        assert (img[..., 3] == 255).all()
        assert not img[inp["counts"] == 0][:, :3].any()                      # no sample: black in every data view
        if view == abi.VIEW_DEPTH and fields["auto_range"]:
            want = {"one_depth": 1, "no_depth": 0}.get(kind)
            if want is not None:
                assert stats[1] == want and stats[2] == stats[3] == (f32(2.75) if want else f32(0))
                # z0 == z1: t = 0, so the one valid pixel is drawn at v = 1 and every other pixel is black
                lit = img[..., :3].any(axis=-1)
                assert lit.sum() == want


def test_the_cards_hold_what_they_promise():
    inp = vl.card((17, 9))
    n, d = inp["counts"].ravel(), vl.np_depth(inp)[0].ravel()
    h = inp["normal"][..., 3].ravel()
    assert {0, 1, 2}.issubset(set(n.tolist())) and n.max() > 1 << 31
    assert np.isnan(d).any() and np.isinf(d).any() and (h == 0).any() and np.isnan(h).any() and (d < 0).any() and np.signbit(d[d == 0]).any()
    s = inp["slots"].reshape(-1, 8)
    full = (s["count"] != 0).all(axis=1)
    assert (full & (s["count"].sum(axis=1) < n)).any()
    assert ((s["id"] == abi.MATTE_NONE) & (s["count"] != 0)).any()
    # the stops: depth under the manual range and under the card's own; n / spp; the noise at noise_max = 1
    o = vl.options(view=abi.VIEW_DEPTH, auto_range=1)
    z0, z1, count = vl.np_range(inp, o)
    assert (z0, z1) == (0.0, 5.0) and 0 < count < n.size                     # (the -0 pixel is the nearest)
    valid = vl.np_depth(inp)[1].ravel()
    for q in range(5):
        assert ((d == q + 1) & valid).any(), q
        assert (n == max(vl.SPP * q // 4, 1)).any(), q
    err = vl.np_adaptive_error(inp["moments"][..., 1].ravel(), inp["moments"][..., 2].ravel(), n)
    for q in range(5):
        assert ((err == f32(q / 4.0)) & (n == 2)).any(), q
    assert np.isnan(err[n >= 2]).any()
    a = inp["film"][..., 3].ravel()
    assert (a == 0).any() and (a == 1).any() and np.isnan(a).any() and (a < 0).any() and (a > 1).any()


def test_the_ramp_at_its_stops():
    """A one-row card of SAMPLES: n / spp = 0.25 k exactly gives the stop's own colour; the heat ramp is continuous across a stop."""
    spp = 1 << 20
    n = np.array([[1, spp // 4, spp // 2, 3 * spp // 4, spp, spp + 1, spp // 4 - 1, spp // 4 + 1]], np.uint32)
    inp = dict(vl.card((8, 1)), counts=n, spp=spp)
    heat, _ = _check(inp, dict(view=abi.VIEW_SAMPLES, ramp=abi.RAMP_HEAT))
    assert heat[0, 1:6, :3].tolist() == [[0, 255, 255], [0, 255, 0], [255, 255, 0], [255, 0, 0], [255, 0, 0]]
    assert heat[0, 0, :3].tolist() == [0, 0, 255] and heat[0, 6, :3].tolist() == [0, 255, 255] and heat[0, 7, :3].tolist() == [0, 255, 255]
    grey, _ = _check(inp, dict(view=abi.VIEW_SAMPLES, ramp=abi.RAMP_GREY))
    assert grey[0, :6, 0].tolist() == [0, 64, 128, 191, 255, 255]
    assert vl.np_ramp(f32(NAN), abi.RAMP_HEAT).tolist() == [1.0, 0.0, 0.0] and vl.np_ramp(f32(NAN), abi.RAMP_GREY).tolist() == [1.0, 1.0, 1.0]


# ---- the range over a rectangle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rect", [(3, 2, 11, 7), (0, 0, 1, 1), (16, 8, 17, 9), (5, 0, 6, 9), (0, 0, 17, 9)])
def test_the_range_is_taken_over_the_rectangle(rect):
    inp = vl.card((17, 9))
    for auto in (1, 0):
        fields = dict(view=abi.VIEW_DEPTH, ramp=abi.RAMP_HEAT, auto_range=auto, depth_min=0.5, depth_max=3.5)
        img, stats = _check(inp, fields, rect)
        d, valid = vl.np_depth(inp)
        inside = np.zeros(valid.shape, bool)
        inside[rect[1]:rect[3], rect[0]:rect[2]] = True
        assert stats[1] == int((valid & inside).sum())
        if auto and stats[1]:
            assert stats[2] == np.abs(d[valid & inside]).min() and stats[3] == d[valid & inside].max()
        if not auto:
            assert (stats[2], stats[3]) == (0.5, 3.5)
    whole = vl.host_view(inp, vl.options(view=abi.VIEW_DEPTH), None)[1]
    assert whole[1] >= stats[1]


# ---- the hash ---------------------------------------------------------------------------------------------------------------------------------
def test_the_id_hash_against_python_integers():
    ids = [0, 1, 2, 3, 255, 256, 65535, 65536, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF, 0xDEADBEEF] + list(range(1000, 1100))
    for x in ids:
        assert vl.lib().view_host_hash(x) == vl.py_hash(x), x
    assert vl.py_hash(0) == 0 and len({vl.py_hash(x) for x in ids}) == len(ids)          # (0 is the hash's fixed point; the hash is a bijection)
    col = vl.np_id_colour(np.array(ids, np.uint32))
    for x, c in zip(ids, col):
        h = vl.py_hash(x)
        want = [0.0] * 3 if x == abi.MATTE_NONE else [float(f32(f32(f32((h >> (8 * k)) & 255) / f32(255)) * f32(0.75)) + f32(0.25)) for k in range(3)]
        assert c.tolist() == want, x
    assert (col[:-1][np.array(ids[:-1]) != abi.MATTE_NONE] >= 0.25).all() and (col <= 1).all()
    # one slot holding every sample draws the id's own colour
    inp = dict(vl.card((1, 1)), counts=np.array([[5]], np.uint32))
    s = np.zeros((1, 1, 8), vl.SLOT)
    s["id"] = abi.MATTE_NONE
    s["id"][0, 0, 0], s["count"][0, 0, 0] = 77, 5
    img, _ = _check(dict(inp, slots=s), dict(view=abi.VIEW_MATTE))
    assert img[0, 0, :3].tolist() == vl.np_quantise(vl.np_id_colour(np.uint32(77))).tolist()


# ---- validation and surface -------------------------------------------------------------------------------------------------------------------
GOOD = [{}] + [dict(view=v) for v in range(abi.VIEW_COUNT)] + [
    dict(layer=abi.MATTE_MATERIAL), dict(ramp=abi.RAMP_HEAT), dict(auto_range=0), dict(auto_range=0, depth_min=0.0, depth_max=3.4e38),
    dict(auto_range=1, depth_min=NAN, depth_max=-1.0),                         # the manual range is not looked at under auto_range
    dict(noise_max=1e-30), dict(noise_max=3.4e38), dict(view=abi.VIEW_BEAUTY, ramp=abi.RAMP_HEAT, layer=1, auto_range=0, depth_min=2.0, depth_max=3.0)]
BAD = [(dict(view=abi.VIEW_COUNT), b"view"), (dict(view=0xFFFFFFFF), b"view"), (dict(layer=2), b"layer"), (dict(ramp=2), b"ramp"),
       (dict(auto_range=2), b"auto_range"),
       (dict(auto_range=0, depth_min=NAN), b"depth_min"), (dict(auto_range=0, depth_max=NAN), b"depth_min"),
       (dict(auto_range=0, depth_max=INF), b"depth_min"), (dict(auto_range=0, depth_min=-INF), b"depth_min"),
       (dict(auto_range=0, depth_min=-0.5), b"depth_min"), (dict(auto_range=0, depth_min=1.0, depth_max=1.0), b"depth_min"),
       (dict(auto_range=0, depth_min=2.0, depth_max=1.0), b"depth_min"),
       (dict(noise_max=0.0), b"noise_max"), (dict(noise_max=-1.0), b"noise_max"), (dict(noise_max=NAN), b"noise_max"), (dict(noise_max=INF), b"noise_max")]


def test_validation_before_the_renderer():
    """The options are checked before the renderer: a valid struct reaches the null-renderer test, an invalid one does not."""
    lib = abi.load_library()
    for f in GOOD:
        o = vl.options(**f)
        assert vl.lib().view_host_options_valid(C.byref(o)) == 1, f
        assert lib.pt_set_view_options(None, C.byref(o)) == INVALID and b"null renderer" in lib.pt_last_error(), f
    for f, word in BAD:
        o = vl.options(**f)
        assert vl.lib().view_host_options_valid(C.byref(o)) == 0, f
        assert lib.pt_set_view_options(None, C.byref(o)) == INVALID and word in lib.pt_last_error(), (f, lib.pt_last_error())
    assert lib.pt_set_view_options(None, None) == INVALID
    st = abi.ViewStats()
    assert lib.pt_read_view_stats(None, C.byref(st)) == INVALID


def test_debug_view_checks_its_arguments_before_the_renderer():
    lib = abi.load_library()
    inp = vl.card((17, 9))
    keep = {k: np.ascontiguousarray(v) for k, v in inp.items() if isinstance(v, np.ndarray)}
    out = np.empty((9, 17, 4), np.uint8)

    def call(o, w=17, h=9, rect=None, spp=64, **null):
        p = {k: (None if k in null else a.ctypes.data) for k, a in keep.items()}
        vi = abi.ViewInputs(None, p["normal"], p["moments"], p["film"], p["slots"], p["counts"], spp)
        r = None if rect is None else (C.c_uint32 * 4)(*rect)
        rc = lib.pt_debug_view(None, C.byref(vi), w, h, r, C.byref(o), out.ctypes.data, None)
        return rc, lib.pt_last_error()

    for view in vl.DATA_VIEWS:                                                  # everything valid: the null renderer is what is wrong
        rc, msg = call(vl.options(view=view))
        assert rc == INVALID and b"null renderer" in msg, view
    for view in (abi.VIEW_BEAUTY, abi.VIEW_ALBEDO):
        rc, msg = call(vl.options(view=view))
        assert rc == INVALID and b"post-process" in msg
    for f, word in BAD:
        rc, msg = call(vl.options(**dict(dict(view=abi.VIEW_DEPTH), **f)))
        assert rc == INVALID and word in msg, f
    o = vl.options(view=abi.VIEW_DEPTH)
    assert b"1..2^28" in call(o, w=0)[1] and b"1..2^28" in call(o, w=1 << 15, h=(1 << 13) + 1)[1]
    for rect in ((0, 0, 18, 9), (0, 0, 17, 10), (3, 3, 3, 4), (5, 4, 4, 5)):
        assert b"rectangle" in call(o, rect=rect)[1], rect
    needs = {abi.VIEW_NORMAL: ["normal"], abi.VIEW_DEPTH: ["normal", "moments"], abi.VIEW_ALPHA: ["film"], abi.VIEW_MATTE: ["slots"],
             abi.VIEW_SAMPLES: [], abi.VIEW_NOISE: ["moments"]}
    for view, names in needs.items():
        for name in names + ["counts"]:
            assert b"null input" in call(vl.options(view=view), **{name: 1})[1], (view, name)
        others = {k: 1 for k in ("normal", "moments", "film", "slots") if k not in names}
        assert b"null renderer" in call(vl.options(view=view), **others)[1], view   # what the view does not read may be NULL
    assert b"spp" in call(vl.options(view=abi.VIEW_SAMPLES), spp=0)[1]
    assert lib.pt_debug_view(None, None, 1, 1, None, C.byref(o), out.ctypes.data, None) == INVALID
    assert lib.pt_debug_view(None, C.byref(abi.ViewInputs()), 1, 1, None, None, out.ctypes.data, None) == INVALID


def test_view_abi_and_defaults():
    O, S, I = abi.ViewOptions, abi.ViewStats, abi.ViewInputs
    want = []
    for T in (O, S, I):
        want += [C.sizeof(T)] + [getattr(T, n).offset for n, _ in T._fields_]
    assert vl.layout()[:len(want)] == want
    assert want[:9] == [32, 0, 4, 8, 12, 16, 20, 24, 28] and want[9:14] == [16, 0, 4, 8, 12] and want[14] == 56
    assert (abi.VIEW_BEAUTY, abi.VIEW_ALBEDO, abi.VIEW_NORMAL, abi.VIEW_DEPTH, abi.VIEW_ALPHA, abi.VIEW_MATTE, abi.VIEW_SAMPLES, abi.VIEW_NOISE,
            abi.VIEW_COUNT) == tuple(range(9)) and (abi.RAMP_GREY, abi.RAMP_HEAT) == (0, 1) and len(abi.VIEW_NAMES) == abi.VIEW_COUNT
    lib = abi.load_library()
    o = O(7, 7, 7, 7, 7.0, 7.0, 7.0, 7)
    lib.pt_default_view_options(C.byref(o))
    assert (o.view, o.layer, o.ramp, o.auto_range, o.depth_min, o.depth_max, o._pad) == (abi.VIEW_BEAUTY, abi.MATTE_INSTANCE, abi.RAMP_GREY, 1, 0.0, 1.0, 0)
    assert f32(o.noise_max) == f32(0.1)
    lib.pt_default_view_options(None)
    from platinum_amd.renderer import Renderer
    for member in ("viewOptions", "setViewOptions", "viewStats", "debugView"):
        assert callable(getattr(Renderer, member)), member


def test_the_availability_rule():
    """shown(view, aov, film, matte, adaptive, merged): the view when the render keeps its data, else the beauty."""
    S = vl.lib().view_host_shown
    V = abi
    for view in range(abi.VIEW_COUNT):
        assert S(view, 1, 1, 1, 1, 1) == V.VIEW_BEAUTY                          # a group's merged image
        assert S(view, 1, 1, 1, 1, 0) == view
    assert [S(v, 0, 0, 0, 0, 0) for v in range(8)] == [0, 0, 0, 0, 0, 0, V.VIEW_SAMPLES, 0]
    assert [S(v, 1, 0, 0, 0, 0) for v in range(8)] == [0, V.VIEW_ALBEDO, V.VIEW_NORMAL, V.VIEW_DEPTH, 0, 0, V.VIEW_SAMPLES, V.VIEW_NOISE]
    assert [S(v, 0, 1, 0, 0, 0) for v in range(8)] == [0, 0, 0, 0, V.VIEW_ALPHA, 0, V.VIEW_SAMPLES, 0]
    assert [S(v, 0, 0, 1, 0, 0) for v in range(8)] == [0, 0, 0, 0, 0, V.VIEW_MATTE, V.VIEW_SAMPLES, 0]
    assert [S(v, 0, 0, 0, 1, 0) for v in range(8)] == [0, 0, 0, 0, 0, 0, V.VIEW_SAMPLES, V.VIEW_NOISE]
    assert S(8, 1, 1, 1, 1, 0) == V.VIEW_BEAUTY


# ---- the host code under sanitizers, stand-alone -------------------------------------------------------------------------------------------
def test_host_build_runs_clean_under_asan_and_ubsan_as_a_program_of_its_own(tmp_path):
    """tests/emu/view_emu.cpp with its own main: every view, ramp and range mode over a card of edge values and three rectangles.
    (Nothing loaded into Python runs under a sanitizer.)"""
    exe = tmp_path / "view_emu_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DVIEW_EMU_MAIN", "-o", str(exe), vl.SRC])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, (p.returncode, p.stderr[-2000:])
    assert "depth rect 1x1 auto 1" in p.stdout and "hash(0) = 00000000" in p.stdout
