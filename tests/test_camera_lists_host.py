"""The camera-ray leaf lists (platinum_amd/csrc/pt_camlist.h) on the host: tests/emu/camlist_emu.cpp builds every pixel's list as
camera_lists.hip does and holds it to the scalar walk.  The conservative part is proved by test here: every leaf-queue entry a camera ray's
walk makes must be in its pixel's list, node and mask bits both, and the list trace must return the walk's (tri, t, u, v) bit for bit.  No GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import emu_lib
import host_build
from platinum_amd import abi, scenes
from platinum_amd.renderer import make_params

ULP1 = float(np.nextafter(np.float32(1.0), np.float32(0.0)))   # 1 - ulp: the largest jitter the sampler can return


@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load(os.path.join(host_build.ROOT, "tests", "emu", "camlist_emu.cpp"), os.path.join(host_build.ROOT, "tests", "_build", "libptamd_camlist.so"))
    emu_lib.bind(L)
    L.cl_check.restype = C.c_int
    L.cl_check.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    for f in (L.cl_pixel_box_outside, L.cl_tile_box_outside):
        f.restype = C.c_int
        f.argtypes = [C.POINTER(abi.CameraData), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.cl_entry_dist.restype = C.c_float
    L.cl_entry_dist.argtypes = [C.POINTER(abi.CameraData), C.c_void_p, C.c_void_p]
    L.cl_margin.restype = C.c_double
    L.cl_default_capacity.restype = C.c_uint32
    return L


def jitters():
    rng = np.random.default_rng(20260718)
    corners = [(0.0, 0.0), (0.0, ULP1), (ULP1, 0.0), (ULP1, ULP1)]
    return np.array(corners + [tuple(v) for v in rng.random((28, 2), dtype=np.float32)], dtype=np.float32)


def wide6_emu(monkeypatch, scene, w, h):
    monkeypatch.setenv("EMU_WIDE6", "1")    # the product's 6-wide node form, two triangles per leaf slot
    monkeypatch.setenv("EMU_PAIRS", "1")
    return emu_lib.EmuScene(scene, make_params(w, h, 1, 2), L=lib())


def check(emu, cap):
    j = jitters()
    out = np.zeros(10, dtype=np.uint64)
    assert lib().cl_check(emu.h, cap, j.ctypes.data, len(j), out.ctypes.data) == 0
    keys = ("pixels", "flagged", "entries", "longest", "rays", "queue_entries", "violations", "mismatches", "hits", "bad_slots")
    return dict(zip(keys, (int(v) for v in out)))


# (the scenes and sizes the lists are proved on; 30x20 adds an image width that is no multiple of 8)
CASES = {
    "field-96x54": (lambda: scenes.field_scene(grid=4), 96, 54),
    "cornell-64x64": (lambda: scenes.cornell_scene("bench"), 64, 64),
    "cornell-30x20": (lambda: scenes.cornell_scene("bench"), 30, 20),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_leaf_the_walk_queues_is_on_the_pixels_list_and_the_list_trace_returns_the_walks_hit(monkeypatch, case):
    make, w, h = CASES[case]
    r = check(wide6_emu(monkeypatch, make(), w, h), lib().cl_default_capacity())
    print(case, r)
    assert r["pixels"] == w * h and r["bad_slots"] == 0
    # a test that falls back proves nothing: with the default capacity no pixel of these scenes is left to the walk
    assert r["flagged"] == 0 and r["longest"] <= lib().cl_default_capacity()
    assert r["rays"] == w * h * len(jitters()) and r["hits"] > r["rays"] // 4 and r["queue_entries"] >= r["hits"]
    assert r["violations"] == 0
    assert r["mismatches"] == 0


def test_a_tiny_capacity_flags_some_pixels_and_the_rest_still_agree(monkeypatch):
    make, w, h = CASES["field-96x54"]
    r = check(wide6_emu(monkeypatch, make(), w, h), 2)
    print(r)
    assert 0 < r["flagged"] < r["pixels"]
    assert r["rays"] == (r["pixels"] - r["flagged"]) * len(jitters())
    assert r["violations"] == 0 and r["mismatches"] == 0


def camera(position=(0.0, 0.0, 0.0)):
    """A pinhole at `position` looking down -z: the image plane z = -1 relative to it, 64 x 64 pixels of 1/32, x to the right, y down."""
    c = abi.CameraData()
    px, py, pz = position
    c.position = abi.Float3(px, py, pz, 0.0)
    c.topLeft = abi.Float3(px - 1.0, py + 1.0, pz - 1.0, 0.0)
    c.pixelDeltaU = abi.Float3(1.0 / 32, 0.0, 0.0, 0.0)
    c.pixelDeltaV = abi.Float3(0.0, -1.0 / 32, 0.0, 0.0)
    return c


def outside(cam, px, py, lo, hi, tile=False):
    lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    f = lib().cl_tile_box_outside if tile else lib().cl_pixel_box_outside
    return bool(f(C.byref(cam), px, py, lo.ctypes.data, hi.ctypes.data))


def test_cone_a_box_behind_the_camera_is_outside_and_one_in_front_is_not():
    cam = camera()
    # pixel (32, 32) looks along (1/64, -1/64, -1): a small box on that ray in front, and its mirror image behind the apex
    assert not outside(cam, 32, 32, (0.06, -0.10, -5.1), (0.10, -0.06, -4.9))
    assert outside(cam, 32, 32, (-0.10, 0.06, 4.9), (-0.06, 0.10, 5.1))
    assert outside(cam, 32, 32, (-0.10, 0.06, 4.9), (-0.06, 0.10, 5.1), tile=True)
    # a box beside the cone in front of the camera is outside the pixel's cone, but not the cone of a tile that covers it
    assert outside(cam, 32, 32, (0.50, -0.10, -5.1), (0.60, -0.06, -4.9))
    assert not outside(cam, 32, 32, (0.50, -0.10, -5.1), (0.60, -0.06, -4.9), tile=True)


def test_cone_a_box_that_holds_the_apex_is_never_outside():
    cam = camera((3.0, -2.0, 7.0))
    for px, py in ((0, 0), (63, 63), (17, 40)):
        assert not outside(cam, px, py, (2.5, -2.5, 6.5), (3.5, -1.5, 7.5))
        assert not outside(cam, px, py, (2.5, -2.5, 6.5), (3.5, -1.5, 7.5), tile=True)
    lo, hi = np.array((2.5, -2.5, 6.5)), np.array((3.5, -1.5, 7.5))
    assert lib().cl_entry_dist(C.byref(cam), lo.ctypes.data, hi.ctypes.data) == 0.0


def test_cone_a_box_touching_a_side_plane_within_the_margin_is_kept():
    cam = camera()
    m = lib().cl_margin()
    assert m == 1.0 / 16.0
    # pixel (32, 32) covers x in [0, 1/32] at z = -1; its right-hand plane with the margin passes x = (1 + m) / 32 there.  A thin box at
    # depth 1 whose left face lies half the margin beyond the pixel's own edge is kept, one two margins beyond is outside.
    edge = 1.0 / 32
    for beyond, expect in ((0.5 * m / 32, False), (2.0 * m / 32, True)):
        lo = (edge + beyond, -0.5 / 32 - 1e-3, -1.0)
        hi = (edge + beyond + 0.01, -0.5 / 32 + 1e-3, -1.0)
        assert outside(cam, 32, 32, lo, hi) is expect, (beyond, expect)


def test_entry_distance_is_a_lower_bound_of_the_euclidean_distance():
    cam = camera()
    lo, hi = np.array((3.0, 4.0, -13.0)), np.array((5.0, 6.0, -12.0))
    d = lib().cl_entry_dist(C.byref(cam), lo.ctypes.data, hi.ctypes.data)
    exact = 13.0   # the nearest corner (3, 4, -12)
    assert exact * (1 - 2e-6) <= d <= exact * (1 - 0.9e-6)
