"""Host side of the ambient-occlusion tests: the ctypes wrapper of tests/emu/ao_emu.cpp (the host build of pt_ao.h on top of
the host harness, a library of its own built by tests/host_build.py), a float64 numpy restatement of the AO ray's direction, the checks a
side's AO rays are held to (the host build and the device alike: no figure below comes from the device), and the scenes the host and GPU
tests share.  TEST HARNESS, never imported by platinum_amd."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.scenes import Camera, Material, Transform  # noqa: E402

import ao_witness as aw  # noqa: E402
import emu_lib  # noqa: E402
import geometry_cases as gc  # noqa: E402
import geometry_witness as gw  # noqa: E402
import host_build  # noqa: E402
import math_lib  # noqa: E402

SRC = os.path.join(_ROOT, "tests", "emu", "ao_emu.cpp")
LIB = os.path.join(_ROOT, "tests", "_build", "libptamd_ao.so")
F64 = np.float64
INF = float("inf")
AO_SALT = 0x414F5031                          # PT_AO_SALT (pt_ao.h), written down once more: test_ao_host holds the two to each other
WITNESS_CASES = ("cornell", "cornell_sphere", "truth", "uv_order", "tmin")   # geometry_cases without alpha cut-outs, ties or edge-on views
DISTANCES = (0.5, 2.0, INF)
# the smallest cosine the sampler can draw is sqrt(1 - (1 - 2^-24)) = 2.4e-4 (kOneMinusEpsilon, pt_sampler.h); the fp32 frame adds about 1e-6
MIN_COSINE = 1e-4

# Worst |dir - restated dir| over the components, the host build of the product against the float64 restatement below, over WITNESS_CASES at
# geometry_cases.SIZES and SAMPLES (test_ao_host.py measures it again and holds this figure to the result); asserted: 4 x, on the host build
# and on the device.  The error is sincos_det's (2e-7 asserted in math_lib) through two products, the fp32 frame (normalize of a cross product
# of a unit normal: a few 2^-24) and three products and two sums of localToWorld.
MEASURED = {"direction": 4.02e-7}   # tmin and cornell, sample 0
BOUNDS = {k: 4.0 * v for k, v in MEASURED.items()}


@functools.lru_cache(maxsize=None)
def lib():
    L = emu_lib.bind(host_build.load(src=SRC, lib=LIB))
    L.ao_refused.argtypes = [C.POINTER(abi.AoOptions)]
    L.ao_salt.restype = C.c_uint32
    L.ao_index_of.restype = C.c_uint32
    L.ao_index_of.argtypes = [C.c_uint32]
    L.ao_value_of.restype = C.c_float
    L.ao_value_of.argtypes = [C.c_uint32, C.c_uint32]
    L.ao_fold_states.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    L.ao_debug.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float] + [C.c_void_p] * 3
    L.ao_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p]
    L.ao_camera_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 3
    return L


class HostAo(emu_lib.EmuScene):
    """The host build of the AO pass: emu_lib.EmuScene over the AO library.  `proj` (abi.CameraProjection, default perspective) with the
    snapshot's camera, as tests/projection_lib.HostProjection."""

    def __init__(self, scene, params, proj=None):
        super().__init__(scene, params, L=lib())
        self.proj = proj
        self._cam = C.addressof(self.snapshot.struct.camera)

    def _proj(self):
        return (self._cam, C.addressof(self.proj)) if self.proj is not None else (None, None)

    def debug(self, sample, distance):
        """(origins, directions, state) as Renderer.debugAmbientOcclusion"""
        o, d = np.zeros((self.H, self.W, 3), np.float32), np.zeros((self.H, self.W, 3), np.float32)
        st = np.zeros((self.H, self.W), np.uint32)
        self.L.ao_debug(self.h, *self._proj(), sample, distance, o.ctypes.data, d.ctypes.data, st.ctypes.data)
        return o, d, st

    def counts(self, first, ns, distance, counts=None):
        """(H, W, 2) uint32 {hits, open}: samples [first, first + ns) folded into `counts` (default: zeros) with ao_fold"""
        c = np.zeros((self.H, self.W, 2), np.uint32) if counts is None else counts
        self.L.ao_counts(self.h, *self._proj(), first, ns, distance, c.ctypes.data)
        return c

    def camera_rays(self, sample):
        """(origins, directions, offset): the queue entries of one sample, (H, W, 3) float32 twice and (H, W) uint32"""
        o, d = np.zeros((self.H, self.W, 3), np.float32), np.zeros((self.H, self.W, 3), np.float32)
        off = np.zeros((self.H, self.W), np.uint32)
        self.L.ao_camera_rays(self.h, *self._proj(), sample, o.ctypes.data, d.ctypes.data, off.ctypes.data)
        return o, d, off


def ao_value(counts):
    """pt_ao.h ao_value in numpy float32: open / hits, 1 where hits = 0"""
    hits, opn = counts[..., 0].astype(np.float32), counts[..., 1].astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(counts[..., 0] != 0, (opn / hits).astype(np.float32), np.float32(1.0)).astype(np.float32)


def fold_states(states, counts=None):
    """ao_fold in numpy: hits += state != 0; open += state == 2"""
    c = np.zeros(states.shape + (2,), np.uint32) if counts is None else counts
    c[..., 0] += (states != abi.AO_MISS).astype(np.uint32)
    c[..., 1] += (states == abi.AO_OPEN).astype(np.uint32)
    return c


# ---- the float64 restatement of the direction (pt_ao.h stage_ao) ---------------------------------------------------------------------------------
def ao_index(offset):
    """pcg4d_x(offset, PT_AO_SALT, 0, 0) through geometry_witness's restatement of the sampler's integer part"""
    offset = np.asarray(offset, np.uint32)
    z = np.zeros(offset.shape, np.uint32)
    return gw._pcg4d_x(offset, np.full(offset.shape, AO_SALT, np.uint32), z, z.copy())


def restated_directions(n, index):
    """frame_from_normal(n).localToWorld(sampleCosineHemisphere(u)) in float64, u = the float32 Halton draws of `index` at dimensions 0, 1.
    n (R, 3) float64 unit normals facing the viewer."""
    index = np.asarray(index, np.uint32).ravel()
    ux = math_lib.halton_reference(index, np.zeros(index.size, np.uint32))
    uy = math_lib.halton_reference(index, np.ones(index.size, np.uint32))
    lx, ly, lz = math_lib.ref_cosine_hemisphere(ux, uy)
    a = np.where((np.abs(n[:, 0]) > 0.5)[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    b = np.cross(n, a)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    t = np.cross(n, b)
    return t * lx[:, None] + b * ly[:, None] + n * lz[:, None]


# ---- what a side's AO rays are held to -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tri_normals(name):
    return aw.normals(gc.triangles(name), gc.scene(name))


def check_origins(cam_o, cam_d, hits, origins, state, what):
    """Bit-identical to numpy float32 o + d * t, each operation rounded once, from the side's own camera rays and hit records"""
    h = np.asarray(hits).reshape(-1)
    o, d = cam_o.reshape(-1, 3).astype(np.float32), cam_d.reshape(-1, 3).astype(np.float32)
    want = (o + (d * h["t"].astype(np.float32)[:, None]).astype(np.float32)).astype(np.float32)
    hit = h["instance"] >= 0
    assert np.array_equal(hit, state.reshape(-1) != abi.AO_MISS), what
    got = origins.reshape(-1, 3)
    assert np.array_equal(got[hit].view(np.uint32), want[hit].view(np.uint32)), what
    assert np.all(got[~hit] == 0.0), what


def check_directions(name, cam_d, offset, hits, directions, what):
    """Against the float64 restatement on the witness triangle's normal; returns the worst error (printed before it is asserted)."""
    T = gc.triangles(name)
    h = np.asarray(hits).reshape(-1)
    hit = np.flatnonzero(h["instance"] >= 0)
    k = T.base[h["instance"][hit]] + h["primitive"][hit]
    n = tri_normals(name)[k]
    flip = (n * cam_d.reshape(-1, 3)[hit].astype(F64)).sum(1) > 0
    n = np.where(flip[:, None], -n, n)
    got = directions.reshape(-1, 3)[hit].astype(F64)
    want = restated_directions(n, ao_index(offset.reshape(-1)[hit]))
    err = float(np.abs(got - want).max())
    cos = (got * n).sum(1)
    print("%s: direction %.3e over %d rays; smallest dot(dir, n) %.3e" % (what, err, hit.size, cos.min()))
    assert err <= BOUNDS["direction"], (what, err)
    assert cos.min() >= MIN_COSINE, (what, cos.min())
    assert np.all(directions.reshape(-1, 3)[h["instance"] < 0] == 0.0), what
    return err


_classes = {}


def witness_classes(name, W, H, sample, origins, directions):
    """{distance: (must_occluded, must_open)} of a side's AO rays; one brute-force pass per distinct set of rays and process."""
    key = (name, W, H, sample, origins.tobytes(), directions.tobytes())
    if key not in _classes:
        _classes[key] = aw.classify(gc.triangles(name), origins.reshape(-1, 3), directions.reshape(-1, 3), DISTANCES)
    return _classes[key]


def check_witness(name, W, H, sample, distance, origins, directions, state, what):
    """No state contradicts the witness, and it decides at least DECIDED_SHARE of the AO rays; returns (decided share, occluded share)."""
    occ, opn = witness_classes(name, W, H, sample, origins, directions)[distance]
    st = state.reshape(-1)
    rays = st != abi.AO_MISS
    bad = np.flatnonzero(rays & (((st == abi.AO_OPEN) & occ) | ((st == abi.AO_OCCLUDED) & opn)))
    decided = float((occ | opn)[rays].mean())
    share = float((st[rays] == abi.AO_OCCLUDED).mean())
    print("%s distance %g: %d AO rays, decided %.4f, occluded %.3f" % (what, distance, rays.sum(), decided, share))
    assert bad.size == 0, "%s: %d states contradict the witness, first at ray %d (state %d)" % (what, bad.size, bad[0], st[bad[0]])
    assert decided >= aw.DECIDED_SHARE, (what, decided)
    return decided, share


def check_side(name, W, H, sample, distance, cam, hits, ao, what):
    """Every assertion on one sample of one side: cam = (origins, directions, offset) of its camera rays, hits its first-hit records,
    ao = (origins, directions, state) of its AO rays."""
    check_origins(cam[0], cam[1], hits, ao[0], ao[2], what)
    err = check_directions(name, cam[1], cam[2], hits, ao[1], what)
    check_witness(name, W, H, sample, distance, ao[0], ao[1], ao[2], what)
    return err


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------------
PLANES_H, PLANES_D = 1.0, 2.0


def planes_scene(ceiling=True):
    """Floor and ceiling PLANES_H apart (40 x 40: more than sqrt(d^2 - h^2) = 1.74 beyond every floor point the camera sees, which lie within
    3 of the origin), seen from between them looking down at the floor.  ceiling=False: the floor alone."""
    sc = scenes.Scene(name="ao_planes")
    quad = sc.add_mesh(scenes.plane(40.0))
    sc.add_instance(quad, Transform(), [Material(base_color=(0.7, 0.7, 0.7, 1.0))])
    if ceiling:
        sc.add_instance(quad, Transform(translation=(0, PLANES_H, 0), rotation=(math.pi, 0, 0)), [Material(base_color=(0.7, 0.7, 0.7, 1.0))])
    sc.set_camera(Camera.with_focal_length(35.0), Transform(translation=(0.0, 0.8, 1.5), target=(0, 0, 0), track=True))
    return sc


def thin_lens_scene():
    sc = scenes.cornell_scene("bench")
    sc.camera.aperture = 2.0
    return sc
