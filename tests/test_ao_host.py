"""CPU: the ambient-occlusion pass of the host build of the product (tests/emu/ao_emu.cpp: pt_ao.h's stage_ao over traverse<true, false>)
against geometry (ao_witness.py: float64, brute force), against its own definition restated in numpy (origin, direction), against the
distribution a cosine-weighted hemisphere must give, under both tree forms of the host harness, and the fold, the resolve and the ABI's
checks that need no device.  Each test prints its figures before it asserts (pytest -s shows them)."""
import ctypes as C
import math

import numpy as np
import pytest

import ao_lib
import geometry_cases as gc
from platinum_amd import abi, scenes
from platinum_amd.renderer import make_params

INF, NAN = float("inf"), float("nan")
INVALID = -1
CASE_SIZES = [(n, s) for n in ao_lib.WITNESS_CASES for s in gc.SIZES]
IDS = ["%s-%dx%d" % (n, s[0], s[1]) for n, s in CASE_SIZES]
_direction_errors = {}


@pytest.mark.parametrize("name,size", CASE_SIZES, ids=IDS)
def test_ao_rays_match_their_definition_and_the_witness(name, size):
    """Origins bit for bit, directions within ao_lib.BOUNDS of the float64 restatement and at least 1e-4 above the surface, no state against
    the witness, at least 99 % of the AO rays decided by it; on cornell both answers are exercised."""
    W, H = size
    h = ao_lib.HostAo(gc.scene(name), make_params(W, H, 1024, 1))
    for s in gc.SAMPLES:
        cam, hits = h.camera_rays(s), h.trace_primary(s)
        rays = None
        for D in ao_lib.DISTANCES:
            ao = h.debug(s, D)
            what = "%s %dx%d sample %d" % (name, W, H, s)
            if rays is None:
                rays = ao
                ao_lib.check_origins(cam[0], cam[1], hits, ao[0], ao[2], what)
                _direction_errors[(name, size, s)] = ao_lib.check_directions(name, cam[1], cam[2], hits, ao[1], what)
            else:   # the rays do not depend on the distance
                assert np.array_equal(ao[0].view(np.uint32), rays[0].view(np.uint32)) and np.array_equal(ao[1].view(np.uint32), rays[1].view(np.uint32))
            _, occluded = ao_lib.check_witness(name, W, H, s, D, ao[0], ao[1], ao[2], what)
            if name == "cornell" and D == 2.0:
                assert 0.03 < occluded < 0.5, occluded
            if name == "cornell" and D == INF:
                assert occluded > 0.5, occluded


def test_the_measured_direction_error_is_the_one_written_down():
    """ao_lib.MEASURED is the worst of the host build over the cases above (taken from them when they ran in this process, else made here)."""
    for name, size in CASE_SIZES:
        missing = [s for s in gc.SAMPLES if (name, size, s) not in _direction_errors]
        if missing:
            h = ao_lib.HostAo(gc.scene(name), make_params(size[0], size[1], 1024, 1))
            for s in missing:
                cam = h.camera_rays(s)
                _direction_errors[(name, size, s)] = ao_lib.check_directions(name, cam[1], cam[2], h.trace_primary(s), h.debug(s, 1.0)[1], name)
    worst = max(_direction_errors.values())
    print("worst direction error of the host build %.3e at %s; written down %.3e" % (worst, max(_direction_errors, key=_direction_errors.get),
                                                                                  ao_lib.MEASURED["direction"]))
    assert 0.9 * ao_lib.MEASURED["direction"] <= worst <= ao_lib.MEASURED["direction"]


def test_the_directions_are_cosine_weighted():
    """mean(cos theta) = 2/3 +- 5 sqrt(1 / (18 N)) over the N AO rays of 48 x 32 x 16 samples: E[cos] = 2/3 and Var[cos] = 1/2 - 4/9 = 1/18
    under the density cos / pi.  cos theta is taken against the witness triangle's normal."""
    W, H, NS = 48, 32, 16
    name = "cornell"
    h = ao_lib.HostAo(gc.scene(name), make_params(W, H, 1024, 1))
    T = gc.triangles(name)
    cosines = []
    for s in range(NS):
        hits = h.trace_primary(s).reshape(-1)
        cam = h.camera_rays(s)
        _, d, st = h.debug(s, 1.0)
        hit = np.flatnonzero(hits["instance"] >= 0)
        n = ao_lib.tri_normals(name)[T.base[hits["instance"][hit]] + hits["primitive"][hit]]
        n = np.where(((n * cam[1].reshape(-1, 3)[hit]).sum(1) > 0)[:, None], -n, n)
        dd = d.reshape(-1, 3)[hit].astype(np.float64)
        cosines.append((dd * n).sum(1) / np.linalg.norm(dd, axis=1))
    c = np.concatenate(cosines)
    tol = 5.0 * math.sqrt(1.0 / (18.0 * c.size))
    print("mean cos theta %.5f over %d rays (2/3 +- %.5f)" % (c.mean(), c.size, tol))
    assert abs(c.mean() - 2.0 / 3.0) <= tol


def test_two_parallel_planes_leave_a_quarter_of_the_rays_open():
    """Floor and ceiling h = 1 apart, distance d = 2: an AO ray meets the ceiling at t = h / cos theta, so it is open iff cos theta < h / d,
    which a cosine-weighted direction is with probability (h / d)^2 = 0.25; +- 5 sqrt(p (1 - p) / N)."""
    W, H, NS = 48, 32, 16
    h = ao_lib.HostAo(ao_lib.planes_scene(), make_params(W, H, 1024, 1))
    c = h.counts(0, NS, ao_lib.PLANES_D)
    assert np.all(c[..., 0] == NS)                          # every camera ray looks at the floor
    o, _, _ = h.debug(0, ao_lib.PLANES_D)
    reach = math.sqrt(ao_lib.PLANES_D ** 2 - ao_lib.PLANES_H ** 2)
    assert np.abs(o[..., [0, 2]]).max() + reach < 20.0 and np.abs(o[..., 1]).max() < 1e-5   # the ceiling covers every AO ray's reach
    N = int(c[..., 0].sum())
    p = (ao_lib.PLANES_H / ao_lib.PLANES_D) ** 2
    tol = 5.0 * math.sqrt(p * (1 - p) / N)
    share = c[..., 1].sum() / N
    print("open share %.5f over %d rays (%.2f +- %.5f)" % (share, N, p, tol))
    assert abs(share - p) <= tol
    # short of the ceiling everything is open
    assert np.array_equal(h.counts(0, 4, 0.999 * ao_lib.PLANES_H)[..., 1], np.full((H, W), 4))


def test_a_single_plane_occludes_nothing():
    W, H, NS = 50, 35, 8
    sc = ao_lib.planes_scene(ceiling=False)
    sc.set_camera(sc.camera, scenes.Transform(translation=(0.0, 0.8, 1.5), target=(0, 0.9, 0), track=True))   # the horizon is in the image
    h = ao_lib.HostAo(sc, make_params(W, H, 1024, 1))
    c = h.counts(0, NS, INF)
    hit = sum((h.trace_primary(s)["instance"] >= 0).astype(np.uint32) for s in range(NS))
    assert np.array_equal(c[..., 1], c[..., 0]) and np.array_equal(c[..., 0], hit)
    assert 0 < hit.sum() < NS * W * H                      # hits and misses both
    v = ao_lib.ao_value(c)
    assert np.all(v == 1.0)


@pytest.mark.parametrize("name", ["cornell", "cornell_sphere", "textured"])
def test_the_states_do_not_depend_on_the_tree(name, monkeypatch):
    """The default tree of the host harness (4-wide, one triangle per slot) and the device's form (6-wide, pair slots) give the same rays and
    states; scenes.textured_scene() has alpha cut-outs, so the AO ray's own alpha-test draw is covered."""
    W, H = 24, 17
    sc = scenes.textured_scene() if name == "textured" else gc.scene(name)
    p = make_params(W, H, 1024, 1)
    a = ao_lib.HostAo(sc, p)
    monkeypatch.setenv("EMU_WIDE6", "1")
    monkeypatch.setenv("EMU_PAIRS", "1")
    b = ao_lib.HostAo(sc, p)
    monkeypatch.delenv("EMU_WIDE6")
    monkeypatch.delenv("EMU_PAIRS")
    seen = set()
    for s in (0, 1, 977):
        for D in (2.0, INF):
            ra, rb = a.debug(s, D), b.debug(s, D)
            for x, y in zip(ra, rb):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (name, s, D)
            seen |= set(np.unique(ra[2]).tolist())
    assert seen >= {abi.AO_OCCLUDED, abi.AO_OPEN}
    if name == "textured":
        assert abi.AO_MISS in seen                              # the open sky


def test_the_fold_does_not_depend_on_the_split():
    W, H, NS, D = 24, 17, 24, 2.0
    h = ao_lib.HostAo(gc.scene("cornell"), make_params(W, H, 1024, 1))
    whole = h.counts(3, NS, D)
    assert whole[..., 0].max() == NS and 0 < whole[..., 1].sum() < whole[..., 0].sum()
    for split in ((1,) * NS, (7, 8, 9), (8, 16), (23, 1), (5, 19)):
        assert sum(split) == NS
        c, first = None, 3
        for n in split:
            c = h.counts(first, n, D, c)
            first += n
        assert np.array_equal(c, whole), split
    # ... and is the sum of the per-sample states, through ao_fold and through its numpy restatement
    states = np.stack([h.debug(3 + s, D)[2] for s in range(NS)])
    a, b = np.zeros((H, W, 2), np.uint32), np.zeros((H, W, 2), np.uint32)
    for st in states:
        ao_lib.lib().ao_fold_states(W * H, np.ascontiguousarray(st).ctypes.data, a.ctypes.data)
        ao_lib.fold_states(st, b)
    assert np.array_equal(a, whole) and np.array_equal(b, whole)


def test_ao_value_edge_cases():
    L = ao_lib.lib()
    assert L.ao_value_of(0, 0) == 1.0                           # no camera ray hit: nothing is occluded
    assert L.ao_value_of(5, 0) == 0.0 and L.ao_value_of(5, 5) == 1.0
    assert L.ao_value_of(3, 1) == float(np.float32(1.0) / np.float32(3.0))
    big = 1 << 24
    assert L.ao_value_of(big + 1, big + 1) == 1.0               # counts beyond fp32's integers still resolve to [0, 1]
    c = np.array([[0, 0], [5, 0], [5, 5], [3, 1], [7, 2]], np.uint32)
    assert [float(v) for v in ao_lib.ao_value(c)] == [L.ao_value_of(int(a), int(b)) for a, b in c]


def test_the_ao_stream_is_its_own():
    L = ao_lib.lib()
    assert L.ao_salt() == ao_lib.AO_SALT
    off = np.array([0, 1, 0x12345678, 0xFFFFFFFF, 977], np.uint32)
    assert [L.ao_index_of(int(o)) for o in off] == [int(v) for v in ao_lib.ao_index(off)]
    assert len(set(int(v) for v in ao_lib.ao_index(off)) & set(int(o) for o in off)) == 0


def test_ao_options_abi():
    O, S = abi.AoOptions, abi.AoStats
    lay = (C.c_uint32 * 7)()
    ao_lib.lib().ao_layout(lay)
    assert list(lay) == [C.sizeof(O), O.enabled.offset, O.distance.offset, C.sizeof(S), S.rays.offset, S.ms_trace.offset, S.ms_fold.offset]
    assert list(lay) == [16, 0, 4, 16, 0, 8, 12]
    assert (abi.AO_MISS, abi.AO_OCCLUDED, abi.AO_OPEN) == (0, 1, 2)
    lib = abi.load_library()
    o = O(7, 7.0, (C.c_uint32 * 2)(7, 7))
    lib.pt_default_ao_options(C.byref(o))
    assert (o.enabled, o.distance, list(o._pad)) == (0, 1.0, [0, 0])
    lib.pt_default_ao_options(None)


GOOD = [{}, dict(enabled=1), dict(distance=INF), dict(enabled=1, distance=1e-30), dict(distance=3.4e38)]
BAD = [dict(enabled=2), dict(enabled=0xFFFFFFFF), dict(distance=0.0), dict(distance=-0.0), dict(distance=-1.0), dict(distance=NAN), dict(distance=-INF)]


def test_validation_before_the_renderer_and_the_errors_that_need_no_device():
    """The options are checked before the renderer: a valid struct reaches the null-renderer test, an invalid one does not.  Null pointers."""
    lib = abi.load_library()

    def options(**f):
        o = abi.AoOptions()
        lib.pt_default_ao_options(C.byref(o))
        for k, v in f.items():
            setattr(o, k, v)
        return o

    for f in GOOD:
        o = options(**f)
        assert ao_lib.lib().ao_refused(C.byref(o)) == 0
        assert lib.pt_set_ao_options(None, C.byref(o)) == INVALID and b"null renderer" in lib.pt_last_error(), f
    for f in BAD:
        o = options(**f)
        assert ao_lib.lib().ao_refused(C.byref(o)) == 1
        assert lib.pt_set_ao_options(None, C.byref(o)) == INVALID and b"null renderer" not in lib.pt_last_error(), f
    assert lib.pt_set_ao_options(None, None) == INVALID
    buf = (C.c_uint32 * 8)()
    assert lib.pt_read_ao(None, buf) == INVALID and lib.pt_read_ao_counts(None, buf) == INVALID
    assert lib.pt_debug_ao(None, 0, buf, buf, buf) == INVALID
    assert lib.pt_get_ao_stats(None, C.byref(abi.AoStats())) == INVALID


def test_the_automatic_batch_size_counts_four_more_bytes_per_path():
    Q = ao_lib.lib().ao_queue_budget
    Q.restype = C.c_uint64
    Q.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_uint64]
    free, held = 100 << 30, 7 << 30
    assert Q(free, held, 0, 0) == free + held                    # AO off: what it was
    assert Q(free, held, 0, 1 << 30) == free + held              # (an Obuf still held is released before the plan)
    assert Q(free, held, 1, 0) == (free + held) // 204 * 200     # 4 B beside the ~200 B of queue state per path
    assert Q(free, held, 1, 1 << 30) == (free + held + (1 << 30)) // 204 * 200
    assert Q(0, held, 1, 0) == 0                                 # unknown stays unknown
