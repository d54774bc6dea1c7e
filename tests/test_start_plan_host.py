"""CPU: the decisions pt_start_render takes before it touches the device (platinum_amd/csrc/host_scene.h, built for the host by
tests/emu/start_plan_probe.cpp, a part of the host harness of tests/host_build.py): the instance records of the two-level structure and
whether every instance is invertible, the choice between one BVH and the two-level structure, whether and at what size the camera-ray
lists are built, and the memory the path queues are planned for.  Every expectation here is exact: the inputs are chosen so that the
arithmetic has no rounding, and the budgets are integers."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import host_build

AUTO, ONE_BVH, TWO_LEVEL = 0, 1, 2    # include/ptamd.h PT_ACCEL_*
INFO = np.dtype([("c0", "3f4"), ("c1", "3f4"), ("c2", "3f4"), ("c3", "3f4"), ("mesh", "u4"), ("material_base", "u4"),
                 ("tri_global_base", "u4"), ("flags", "u4")])                                     # pt_device.h InstanceInfo
TRAV = np.dtype([("ic0", "3f4"), ("ic1", "3f4"), ("ic2", "3f4"), ("c", "3f4"), ("tri_base", "u4"), ("mesh", "u4"), ("pad", "2u4")])  # InstanceTrav


@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load()
    L.sp_instance_trav.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    L.sp_choose_accel.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_int)]
    L.sp_flat_bytes_per_tri.restype = C.c_uint64
    L.sp_camera_lists_wanted.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_float, C.c_int, C.c_int]
    L.sp_cam_entry_size.restype = C.c_uint64
    L.sp_cam_default_capacity.restype = C.c_uint32
    L.sp_camera_list_bytes.argtypes = [C.c_uint32] * 3
    L.sp_camera_list_bytes.restype = C.c_uint64
    L.sp_camera_lists_fit.argtypes = [C.c_uint64] * 3
    L.sp_queue_budget.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64]
    L.sp_queue_budget.restype = C.c_uint64
    return L


def _instances(mats):
    """InstanceInfo records from (3x3 matrix as rows, translation) pairs; mesh, tri_global_base and the rest get distinct values."""
    a = np.zeros(len(mats), INFO)
    for i, (m, t) in enumerate(mats):
        m = np.asarray(m, np.float32)
        a[i]["c0"], a[i]["c1"], a[i]["c2"], a[i]["c3"] = m[:, 0], m[:, 1], m[:, 2], np.asarray(t, np.float32)
        a[i]["mesh"], a[i]["material_base"], a[i]["tri_global_base"], a[i]["flags"] = 7 + i, 100 + i, 1000 * (i + 1), 1
    return a


def _trav(info):
    out = np.frombuffer(b"\xaa" * (TRAV.itemsize * len(info)), TRAV).copy()
    ok = lib().sp_instance_trav(info.ctypes.data, len(info), out.ctypes.data)
    return bool(ok), out


def _inverse(t):
    return np.stack([t["ic0"], t["ic1"], t["ic2"]], axis=1)   # columns -> a row-major 3x3


IDENTITY = np.eye(3)
DIAGONAL = np.diag([2.0, 0.5, 4.0])
QUARTER_TURN = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])   # x -> y, y -> -x: 90 degrees about z


def test_instance_records_hold_the_exact_inverse_and_copy_the_rest():
    info = _instances([(IDENTITY, (0, 0, 0)), (DIAGONAL, (1, 2, 3)), (QUARTER_TURN, (-5.5, 0.25, 8))])
    ok, trav = _trav(info)
    assert ok
    want = [IDENTITY, np.diag([0.5, 2.0, 0.25]), QUARTER_TURN.T]
    for i in range(3):
        # these inverses have no rounding, so the bits are compared; `+ 0.0` first: the sign of a zero entry is not part of the value
        got = _inverse(trav[i]) + np.float32(0.0)
        assert got.view(np.uint32).tolist() == want[i].astype(np.float32).view(np.uint32).tolist(), (i, got)
        assert trav[i]["c"].tobytes() == info[i]["c3"].tobytes()
        assert trav[i]["tri_base"] == info[i]["tri_global_base"] and trav[i]["mesh"] == info[i]["mesh"]
        assert trav[i]["pad"].tolist() == [0, 0]


@pytest.mark.parametrize("name,matrix", [
    ("a zero column", [[1, 0, 0], [0, 0, 0], [0, 0, 1]]),
    ("two equal columns", [[1, 1, 0], [2, 2, 0], [0, 0, 1]]),
    ("a NaN entry", [[1, 0, 0], [0, float("nan"), 0], [0, 0, 1]]),
])
def test_a_singular_or_non_finite_instance_is_not_invertible(name, matrix):
    assert not _trav(_instances([(matrix, (0, 0, 0))]))[0], name
    assert not _trav(_instances([(IDENTITY, (0, 0, 0)), (matrix, (0, 0, 0)), (DIAGONAL, (0, 0, 0))]))[0], name   # one bad instance is enough


def test_a_small_uniform_scale_is_invertible():
    """The determinant bound is relative to the cube of the largest entry: 1e-15 is a healthy determinant for a matrix of 1e-5."""
    ok, trav = _trav(_instances([(np.eye(3) * 1e-5, (0, 0, 0))]))
    assert ok
    np.testing.assert_allclose(_inverse(trav[0]), np.eye(3) * 1e5, rtol=1e-6, atol=0)


def _choose(invertible, tris, unique, free, accel, override):
    auto = C.c_int(-1)
    two = lib().sp_choose_accel(int(invertible), tris, unique, free, accel, override, C.byref(auto))
    return bool(two), bool(auto.value)


def test_structure_choice_truth_table():
    per_tri = lib().sp_flat_bytes_per_tri()
    assert per_tri == 292
    unique = 1000
    rows = 0
    for tris in (8 * unique - 1, 8 * unique, 8 * unique + 1):
        flat = per_tri * tris
        # flat > free / 2 (integer division): true up to free = 2 * flat - 1, false from 2 * flat on; 0 = no reading
        for free in (0, 1, 2 * flat - 2, 2 * flat - 1, 2 * flat, 2 * flat + 1, 1 << 40):
            by_budget = tris >= 8 * unique and free != 0 and flat > free // 2
            for invertible, override in itertools.product((False, True), (-1, 0, 1)):
                at = (tris, free, invertible, override)
                assert _choose(invertible, tris, unique, free, ONE_BVH, override) == (False, False), at
                assert _choose(invertible, tris, unique, free, TWO_LEVEL, override) == (invertible, False), at
                if override == 0:
                    want = (False, False)
                elif override == 1:
                    want = (invertible, False)
                else:
                    want = (invertible and by_budget,) * 2    # the only row that is "chosen automatically"
                assert _choose(invertible, tris, unique, free, AUTO, override) == want, at
                rows += 1
    assert rows == 3 * 7 * 6
    # both sides of each threshold, spelled out
    flat = per_tri * 8000
    assert _choose(True, 8000, unique, 2 * flat - 1, AUTO, -1) == (True, True)
    assert _choose(True, 8000, unique, 2 * flat, AUTO, -1) == (False, False)
    assert _choose(True, 7999, unique, 2, AUTO, -1) == (False, False)
    assert _choose(True, 8000, unique, 0, AUTO, -1) == (False, False)


def test_camera_lists_are_wanted_only_when_all_seven_terms_hold():
    good = dict(disabled=0, two_level=0, wide6=1, root_ref=0, aperture_radius=0.0, adaptive=0, region=0)
    order = list(good)

    def wanted(**change):
        return bool(lib().sp_camera_lists_wanted(*[dict(good, **change)[k] for k in order]))

    assert wanted()
    assert wanted(root_ref=12345)
    for change in (dict(disabled=1), dict(two_level=1), dict(wide6=0), dict(root_ref=0xffffffff), dict(root_ref=0x80000005),
                   dict(aperture_radius=0.01), dict(adaptive=1), dict(region=1)):
        assert not wanted(**change), change


def test_camera_list_bytes_and_the_sixteenth_bound():
    L = lib()
    entry, cap = L.sp_cam_entry_size(), L.sp_cam_default_capacity()
    for (w, h), c in itertools.product([(1920, 1080), (3840, 2160), (33, 17), (8, 8), (1, 1)], [cap, 1, 7]):
        slots = ((w + 7) // 8) * ((h + 7) // 8) * 64
        assert L.sp_camera_list_bytes(w, h, c) == slots * (c * entry + 4), (w, h, c)
    assert round(L.sp_camera_list_bytes(1920, 1080, cap) / 1e9, 1) == 2.1     # what the comment at the bound quotes
    assert round(L.sp_camera_list_bytes(3840, 2160, cap) / 1e9, 1) == 8.5
    b = L.sp_camera_list_bytes(1920, 1080, cap)
    assert L.sp_camera_lists_fit(b, 16 * b, 0) and not L.sp_camera_lists_fit(b, 16 * b - 1, 0)
    assert L.sp_camera_lists_fit(b, 15 * b, b) and not L.sp_camera_lists_fit(b, 15 * b - 1, b)   # lists already held count as free
    assert not L.sp_camera_lists_fit(b, 0, 1 << 50)     # no reading of free memory: no credit, no lists
    assert L.sp_camera_lists_fit(0, 1, 0)


def test_queue_budget():
    Q = lib().sp_queue_budget
    assert Q(1000, 200, 32, 0, 88) == 1232                    # AOVs off: the AOV buffer is not counted
    assert Q(1000, 200, 32, 1, 88) == 1320 // 232 * 200 == 1000
    assert Q(1000, 0, 0, 1, 0) == 800                         # 1000 // 232 = 4
    assert Q(231, 0, 0, 1, 0) == 0 and Q(232, 0, 0, 1, 0) == 200
    assert Q(1, 0, 0, 0, 0) == 1
    for aov in (0, 1):                                         # no reading of free memory: what is held earns no credit
        assert Q(0, 53 << 30, 2 << 30, aov, 7 << 30) == 0
    free, queues, lists, abuf = 200 * 10**9, 53 * 10**9 + 17, 2131660800, 7 * 10**9 + 3
    assert Q(free, queues, lists, 0, abuf) == free + queues + lists
    assert Q(free, queues, lists, 1, abuf) == (free + queues + lists + abuf) // 232 * 200
