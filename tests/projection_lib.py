"""Host side of the camera-projection tests: the ctypes wrapper of tests/emu/projection_emu.cpp (the host build of
pt_projection.h on top of the host harness, a library of its own built by tests/host_build.py), a float64 numpy restatement of the three
projections written from include/ptamd.h's text and the scene's camera matrix, and the cameras and cases the host and GPU tests share.
TEST HARNESS, never imported by platinum_amd."""
import copy
import ctypes as C
import functools
import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
from platinum_amd import abi  # noqa: E402

import emu_lib  # noqa: E402
import geometry_cases as gc  # noqa: E402
import geometry_witness as gw  # noqa: E402
import host_build  # noqa: E402

SRC = os.path.join(_ROOT, "tests", "emu", "projection_emu.cpp")
LIB = os.path.join(_ROOT, "tests", "_build", "libptamd_projection.so")
F64 = np.float64
PI32 = float(np.float32(math.pi))          # the fp32 values the validation compares against
TWO_PI32 = float(np.float32(2.0) * np.float32(math.pi))
TINY = 1e-3                                # "tiny" field of view of the option sweep, radians

# The direction bound D per kind (absolute, per component of a unit vector).
#   ORTHOGRAPHIC  4 * 2^-23: -w is one normalisation of a float32 column, normalised once more.
#   EQUIRECT / FISHEYE  4e-6, a first-order sum: the angle carries <= ~1e-6 of float32 rounding (fx / W scaled by up to 2 pi, plus the
#   product), sincos_det adds its asserted 2e-7 (math_lib), two trig factors per component give 2.4e-6, three products and sums and the final
#   normalisation bring it to 2.9e-6, rounded up.
D = {abi.PROJ_ORTHOGRAPHIC: 4.0 * 2.0 ** -23, abi.PROJ_EQUIRECT: 4e-6, abi.PROJ_FISHEYE: 4e-6}
HIT_DTYPE = [("t", "f4"), ("u", "f4"), ("v", "f4"), ("instance", "i4"), ("primitive", "i4")]


def projection(kind, **fields):
    """abi.CameraProjection of `kind` with the library's defaults written down here (ptamd.h) and `fields` over them."""
    p = abi.CameraProjection(kind, 1.0, TWO_PI32, PI32, PI32)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def lib():
    L = emu_lib.bind(host_build.load(src=SRC, lib=LIB))
    L.pj_refused.argtypes = [C.POINTER(abi.CameraProjection)]
    L.pj_constants.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(abi.CameraProjection), C.c_void_p]
    L.pj_rays.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(abi.CameraProjection), C.c_uint32] + [C.c_void_p] * 4
    L.pj_trace_primary.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(abi.CameraProjection), C.c_uint32, C.c_void_p]
    L.pj_ray_dir_to_uv.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    L.pj_miss_radiance.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return L


class HostProjection(emu_lib.EmuScene):
    """The host build of the product under a projection: emu_lib.EmuScene over the projection library, with the snapshot's camera."""

    def __init__(self, scene, params, proj):
        super().__init__(scene, params, L=lib())
        self.proj = proj
        self._cam = C.addressof(self.snapshot.struct.camera)

    def rays(self, sample):
        """(origins, directions, offset, dim): (H, W, 3) float32 twice, (H, W) uint32 twice"""
        o, d = np.zeros((self.H, self.W, 3), np.float32), np.zeros((self.H, self.W, 3), np.float32)
        off, dim = np.zeros((self.H, self.W), np.uint32), np.zeros((self.H, self.W), np.uint32)
        self.L.pj_rays(self.h, self._cam, C.byref(self.proj), sample, o.ctypes.data, d.ctypes.data, off.ctypes.data, dim.ctypes.data)
        return o, d, off, dim

    def trace_primary(self, sample_idx=0):
        out = np.zeros(self.W * self.H, dtype=HIT_DTYPE)
        self.L.pj_trace_primary(self.h, self._cam, C.byref(self.proj), sample_idx, out.ctypes.data)
        return out.reshape(self.H, self.W)

    def miss_radiance(self, d):
        """(n, 3) float32: what a camera ray of direction d brings back when it leaves the scene (the environment lookup)"""
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        out = np.zeros((len(d), 3), np.float32)
        self.L.pj_miss_radiance(self.h, len(d), d.ctypes.data, out.ctypes.data)
        return out

    def projection_constants(self):
        """{topLeft, dU, dV, dir, pos, u, v, w}: the derived float32 constants"""
        out = np.zeros((8, 3), np.float32)
        self.L.pj_constants(self._cam, self.W, self.H, C.byref(self.proj), out.ctypes.data)
        return dict(zip(("topLeft", "dU", "dV", "dir", "pos", "u", "v", "w"), out))


def ray_dir_to_uv(d):
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    uv = np.zeros((len(d), 2), np.float32)
    lib().pj_ray_dir_to_uv(len(d), d.ctypes.data, uv.ctypes.data)
    return uv


# ---- the float64 restatement (include/ptamd.h "camera projections"): from the camera matrix and the options alone -------------------------------
def basis(camera_world):
    """(u, v, w, pos): the normalised columns 0..2 and column 3 of the float32 camera matrix [col][row], promoted"""
    M = np.asarray(camera_world, np.float32).astype(F64)
    u, v, w = (M[i, :3] / np.linalg.norm(M[i, :3]) for i in range(3))
    return u, v, w, M[3, :3].copy()


def restated_rays(camera_world, W, H, proj, sample):
    """(o (R, 3), d (R, 3), fx, fy) of every pixel, row-major, in float64; the sample positions are geometry_witness's."""
    u, v, w, pos = basis(camera_world)
    fx, fy = gw.sample_positions(W, H, sample)
    R = fx.size
    if proj.kind == abi.PROJ_ORTHOGRAPHIC:
        vh = float(proj.ortho_height)
        vw = vh * W / H
        vu, vv = u * vw, -v * vh
        top_left, dU, dV = pos - (vu + vv) * 0.5, vu / W, vv / H
        o = top_left + fx[:, None] * dU + fy[:, None] * dV
        d = np.tile(-w, (R, 1))
    elif proj.kind == abi.PROJ_EQUIRECT:
        phi = (fx / W - 0.5) * float(proj.fov_x)
        theta = math.pi / 2 + (fy / H - 0.5) * float(proj.fov_y)
        d = (np.sin(theta) * np.sin(phi))[:, None] * u + np.cos(theta)[:, None] * v - (np.sin(theta) * np.cos(phi))[:, None] * w
        o = np.tile(pos, (R, 1))
    elif proj.kind == abi.PROJ_FISHEYE:
        half = min(W, H) / 2.0
        x, y = (fx - W / 2.0) / half, (H / 2.0 - fy) / half
        r = np.sqrt(x * x + y * y)
        theta = np.minimum(r * float(proj.fisheye_fov) / 2.0, math.pi)
        rs = np.where(r > 0, r, 1.0)
        d = (np.sin(theta) * x / rs)[:, None] * u + (np.sin(theta) * y / rs)[:, None] * v - np.cos(theta)[:, None] * w
        d[r == 0] = -w
        o = np.tile(pos, (R, 1))
    else:
        raise ValueError(proj.kind)
    return o, d / np.linalg.norm(d, axis=1, keepdims=True), fx, fy


def origin_bound(camera_world, W, H, proj):
    """E_o: 8 * 2^-24 * (|topLeft|_inf + W |dU|_inf + H |dV|_inf) under ORTHOGRAPHIC (three float32 roundings of values of that size in
    topLeft + fx dU + fy dV, the roundings of the three constants themselves, with room); 0 elsewhere (o is the matrix's column, exactly)."""
    if proj.kind != abi.PROJ_ORTHOGRAPHIC:
        return 0.0
    u, v, w, pos = basis(camera_world)
    vh = float(proj.ortho_height)
    vu, vv = u * (vh * W / H), -v * vh
    return 8.0 * 2.0 ** -24 * (np.abs(pos - (vu + vv) * 0.5).max() + np.abs(vu).max() + np.abs(vv).max())


# ---- the cameras and cases of the witness tests -----------------------------------------------------------------------------------------------
WITNESS_SCENES = ("cornell", "cornell_sphere", "truth", "random1", "random3", "random8", "random12")
WITNESS_SIZES = ((50, 35), (64, 32))
FRACTIONS = (0.43, 0.55, 0.61)


def _rot(ax, a):
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])}[ax]


def inside_camera_world(name):
    """The camera of the witness cases: inside the scene at FRACTIONS of the triangles' bounding box, rotated 0.3 rad about x, then 0.7 about
    y.  float32 [col][row] as scenes.Scene.camera_world."""
    T = gc.triangles(name)
    lo, hi = T.v.reshape(-1, 3).min(0), T.v.reshape(-1, 3).max(0)
    pos = lo + np.array(FRACTIONS) * (hi - lo)
    Rm = _rot("y", 0.7) @ _rot("x", 0.3)          # [row][col]: x first, then y
    M = np.eye(4)
    M[:3, :3] = Rm
    M[:3, 3] = pos
    return np.ascontiguousarray(M.T, np.float32)  # [col][row]


def box_longest_side(name):
    T = gc.triangles(name)
    return float((T.v.reshape(-1, 3).max(0) - T.v.reshape(-1, 3).min(0)).max())


@functools.lru_cache(maxsize=None)
def witness_scene(name):
    """geometry_cases.scene(name) with the inside camera (a shallow copy: the cached scene keeps its own)"""
    sc = copy.copy(gc.scene(name))
    sc.camera_world = inside_camera_world(name)
    return sc


def witness_projections(name):
    """{label: projection} of the witness cases: ORTHOGRAPHIC 0.6 x the box's longest side, EQUIRECT 2 pi x pi, FISHEYE pi and 2 pi"""
    return {"ortho": projection(abi.PROJ_ORTHOGRAPHIC, ortho_height=0.6 * box_longest_side(name)),
            "equirect": projection(abi.PROJ_EQUIRECT),
            "fisheye_pi": projection(abi.PROJ_FISHEYE),
            "fisheye_2pi": projection(abi.PROJ_FISHEYE, fisheye_fov=TWO_PI32)}


# the option edges of the formula sweep
def sweep_projections():
    out = [("ortho", projection(abi.PROJ_ORTHOGRAPHIC, ortho_height=2.5))]
    for fx in (TINY, PI32, TWO_PI32):
        for fy in (TINY, PI32):
            out.append(("equirect %.4g x %.4g" % (fx, fy), projection(abi.PROJ_EQUIRECT, fov_x=fx, fov_y=fy)))
    for f in (TINY, PI32, TWO_PI32):
        out.append(("fisheye %.4g" % f, projection(abi.PROJ_FISHEYE, fisheye_fov=f)))
    return out


def sweep_cameras():
    """{label: camera_world}: a rotated camera, and one whose matrix also scales its axes (the scale must be removed)"""
    Rm = _rot("y", -1.1) @ _rot("x", 0.4)
    M = np.eye(4)
    M[:3, :3] = Rm
    M[:3, 3] = (1.25, -0.5, 3.0)
    S = M.copy()
    S[:3, :3] = Rm @ np.diag([2.5, 0.3, 7.0])
    return {"rotated": np.ascontiguousarray(M.T, np.float32), "scaled": np.ascontiguousarray(S.T, np.float32)}


def plus_x_camera_world(pos=(0.0, 0.0, 0.0)):
    """u = +z, v = +y, w = -x: looks along world +x with y up — the camera under which the default EQUIRECT inverts rayDirToUv"""
    M = np.zeros((4, 4), np.float32)   # [col][row]
    M[0, 2] = 1.0
    M[1, 1] = 1.0
    M[2, 0] = -1.0
    M[3, :3] = pos
    M[3, 3] = 1.0
    return M


_witnesses = {}


def witness(name, label, W, H, sample):
    """(witness, D, E_o) of a witness case: the restated rays of witness_projections(name)[label] through the inside camera, against the
    scene's triangles; built once per process and shared by every test."""
    import projection_witness as pw
    key = (name, label, W, H, sample)
    if key not in _witnesses:
        proj = witness_projections(name)[label]
        cw = inside_camera_world(name)
        o, d, _, _ = restated_rays(cw, W, H, proj, sample)
        _witnesses[key] = (pw.ProjectionWitness(gc.scene(name), o, d, W, H, sample, tris=gc.triangles(name)), D[proj.kind],
                           origin_bound(cw, W, H, proj))
    return _witnesses[key]


# ---- the light-probe bake ------------------------------------------------------------------------------------------------------------------------
def probe_scene():
    """The environment-only scene of test_textures_env_alpha (scenes.sky_environment(), one small quad far below) seen through the camera that
    looks along +x with y up: under the default EQUIRECT at the environment's resolution a pixel is a texel."""
    from platinum_amd import scenes
    sc = scenes.Scene(name="sky")
    q = sc.add_mesh(scenes.plane(1.0))
    sc.add_instance(q, scenes.Transform(translation=(0, -50, 0)), [scenes.Material()])
    sc.env_texture = sc.add_texture(scenes.sky_environment(), abi.TEX_RGBA32F)
    sc.set_camera(scenes.Camera.with_focal_length(20.0), plus_x_camera_world((0.0, 1.0, 0.0)))
    return sc


def check_probe(env, radiance, miss, sample, what):
    """radiance (H, W, >= 3) of a 1-sample default-EQUIRECT render at the environment's resolution against the float64 bilinear lookup at
    (fx / W, fy / H), on the pixels whose camera ray missed.  Tolerance: the environment's largest texel-to-texel difference (between
    neighbours under repeat addressing, per channel) x 2e-6 x max(W, H) — the uv bound of the host formula test pushed through the bilinear
    filter — plus 4 float32 roundings of the value.  Prints the worst excess before it asserts."""
    from texture_ref import _bilinear_repeat
    env = np.asarray(env, np.float64)
    Henv, Wenv = env.shape[:2]
    fx, fy = gw.sample_positions(Wenv, Henv, sample)
    step = max(np.abs(env - np.roll(env, 1, 0))[..., :3].max(), np.abs(env - np.roll(env, 1, 1))[..., :3].max())
    got = np.asarray(radiance, np.float64).reshape(-1, radiance.shape[-1])[:, :3]
    miss = np.asarray(miss).reshape(-1)
    worst, where = -np.inf, -1
    for i in np.flatnonzero(miss):
        want = _bilinear_repeat(env, fx[i] / Wenv, fy[i] / Henv)[:3]
        tol = step * 2e-6 * max(Wenv, Henv) + 4 * 2.0 ** -24 * np.abs(want)
        ex = float((np.abs(got[i] - want) - tol).max())
        if ex > worst:
            worst, where = ex, int(i)
    print("%s: %d of %d pixels missed; worst |L - env| - tol = %.3e at pixel %d (texel step %.3g)" % (what, miss.sum(), miss.size, worst, where, step))
    assert miss.mean() >= 0.99
    assert worst <= 0.0, (what, worst, where)
