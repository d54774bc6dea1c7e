"""The scenes and hits of the shading-frame witness (shading_witness.py) — TEST INFRASTRUCTURE.  Every scene is a few dozen triangles and is
started at 48 x 32; a probe batch holds at most 2^16 records.

CASES maps a name to a scene factory.  batches(name) gives the non-edge classes of records of a case ("lattice": a barycentric lattice with
u = 0, v = 0 and u + v = 1 on every triangle; "outside": points 1e-4 outside each edge, which the intersection contract admits; "random");
hit_records(...) turns a side's own first hits (pt_trace_primary) into records; edge_batches(name) is the "edges" class (bits,
admissibility and the finite / inf / NaN class only).

  frames      no textures: nine meshes (orthonormal n, t with sign +1 and -1; smooth normals that differ per vertex; three vertices that
              disagree on the sign; tangents 5, 25, 26 and 60 degrees off the normal — |n . t| on both sides of 0.9; normals with |n.x| on both
              sides of 0.5 under a tangent 10 degrees off) x four instances (identity, rotation + uniform scale, rotation + non-uniform
              scale + translation, mirrored)
  slots       every texture slot but the normal map fed one at a time by every texel format, and all at once; sizes 1x1, 2x1, 1x3, 5x7 and
              64x64; an R8 3x5 (15 bytes) placed first, so that the next base needs the 16-byte round-up; RGBA32F beside 8-bit textures,
              so that a native scene runs float textures through the format chain; 14 instances of ONE two-slot mesh with different
              material sets (material_base + slot); UVs over [-2.5, 3.5]
  normalmaps  RGBA32F and RGBA8 normal maps: flat, tilted, random, and one whose bilinear mix passes near (0.5, 0.5, 0.5); alone and with
              every other slot textured
  uvpoints    triangles of constant UV at exact texel centres, 0, 1, -1e-7 and 1 - eps
  edges       N = 0 exactly, a zero interpolated tangent, |uv size| at 2^23, 2^24, 2^31 - 128, 2^31 and 1e12 (edges class only)"""
import functools

import numpy as np

import geometry_witness as gw
import shading_witness as sw
from platinum_amd import abi, scenes
from platinum_amd.renderer import make_params
from platinum_amd.scenes import Camera, Material, Transform

F32, F64 = np.float32, np.float64
SIZE, SPP, BOUNCES = (48, 32), 1, 1
WORKING_SPACE = scenes.BT2020            # (the scene's colours are BT.709: idt is not the identity)
ONE_MINUS_EPS = float(np.nextafter(F32(1), F32(0)))
UV_CORNERS = [(-2.5, -2.5), (3.5, -2.5), (-2.5, 3.5), (3.5, 3.5)]
FORMATS = {"srgb8": abi.TEX_RGBA8_SRGB, "rgba8": abi.TEX_RGBA8, "rg8": abi.TEX_RG8, "r8": abi.TEX_R8, "f32": abi.TEX_RGBA32F}
SIZES = [(1, 1), (2, 1), (1, 3), (5, 7), (64, 64)]      # (w, h)
SLOTS = ("base_texture", "rm_texture", "transmission_texture", "clearcoat_texture", "emission_texture")
KINDS = {"identity": dict(), "rot_uniform": dict(rotation=(0.3, -0.4, 0.2), scale=(0.8, 0.8, 0.8)),
         "rot_nonuniform": dict(rotation=(-0.25, 0.35, -0.3), scale=(1.1, 0.7, 0.9)), "mirrored": dict(rotation=(0.2, 0.3, -0.15), scale=(-0.9, 0.9, 0.9))}
TRUTH_KINDS = ("identity", "rot_uniform")
TILT = 0.3                                # the angle the tilted normal texel encodes, about the bitangent


def _unit(v):
    v = np.asarray(v, F64)
    return v / np.linalg.norm(v)


def tangent_at(n, degrees, hint=(1.0, 0.0, 0.0)):
    """a unit tangent `degrees` off the unit normal n, in the plane of n and `hint`"""
    n = _unit(n)
    e = _unit(np.asarray(hint, F64) - n * (n @ np.asarray(hint, F64)))
    a = np.radians(degrees)
    return np.cos(a) * n + np.sin(a) * e


def quad(normals, tangents, signs, uvs=UV_CORNERS, slots=(0, 1)):
    """the unit square in the xy plane facing +z: triangles (0, 1, 2) and (2, 1, 3)"""
    v = [(-0.5, -0.5, 0), (0.5, -0.5, 0), (-0.5, 0.5, 0), (0.5, 0.5, 0)]
    t4 = np.concatenate([np.asarray(tangents, F64), np.asarray(signs, F64)[:, None]], axis=1)
    return scenes._make_mesh(v, normals, t4, uvs, [0, 1, 2, 2, 1, 3], list(slots))


N0 = _unit((0.3, 0.2, 1.0))
SMOOTH = [_unit(c) for c in ((-0.35, -0.25, 1), (0.35, -0.2, 1), (-0.3, 0.25, 1), (0.4, 0.3, 1))]
NXVAR = [_unit(c) for c in ((0.25, 0.1, 1), (0.95, 0.1, 1), (0.3, 0.1, 1), (1.2, 0.1, 1))]     # n.x = 0.24 .. 0.77


def meshes():
    m = {"ortho_p": quad([N0] * 4, [tangent_at(N0, 90)] * 4, [1] * 4), "ortho_n": quad([N0] * 4, [tangent_at(N0, 90)] * 4, [-1] * 4),
         "smooth": quad(SMOOTH, [tangent_at(n, 90) for n in SMOOTH], [1] * 4),
         "mixed": quad(SMOOTH, [tangent_at(n, 90, (0.2, 1, 0)) for n in SMOOTH], [1, -1, -1, 1])}     # triangle 0: + - -, triangle 1: - - +
    for a in (5, 25, 26, 60):
        m["ang%d" % a] = quad([N0] * 4, [tangent_at(N0, a)] * 4, [1, 1, -1, -1])
    m["nxvar"] = quad(NXVAR, [tangent_at(n, 10, (0, 1, 0)) for n in NXVAR], [1] * 4)
    return m


ORTHO = ("ortho_p", "ortho_n")


def _place(kind, col, row, cols, rows):
    return Transform(translation=((col - (cols - 1) / 2) * 1.25, (row - (rows - 1) / 2) * 1.25, 0.0), **KINDS[kind])


def _camera(sc, distance):
    """looks down -z at the grid of instances from `distance`: 28 mm on a 36 mm sensor sees 0.64 x distance to either side"""
    sc.set_camera(Camera.with_focal_length(28.0), Transform(translation=(0.0, 0.0, distance), target=(0.0, 0.0, 0.0), track=True))
    return sc


PLAIN = [Material(base_color=(0.7, 0.6, 0.5, 1.0), roughness=0.55, metallic=0.3, emission=(0.6, 0.9, 1.2), emission_strength=2.5),
         Material(base_color=(0.2, 0.9, 0.4, 1.0), roughness=0.25, transmission=0.6, ior=1.33, anisotropy=0.4, clearcoat_roughness=0.11)]


def frames_scene():
    sc = scenes.Scene(name="frames")
    sc.info = []                                     # (mesh name, kind) per instance
    ms = meshes()
    for col, (name, mesh) in enumerate(ms.items()):
        mi = sc.add_mesh(mesh)
        for row, kind in enumerate(KINDS):
            first = col == 0 and row == 0            # the one instance whose matrix is the identity, translation included
            sc.add_instance(mi, Transform() if first else _place(kind, col, row, len(ms), len(KINDS)), PLAIN)
            sc.info.append((name, kind))
    return _camera(sc, 9.5)


def _texels(rng, w, h, fmt):
    c = {abi.TEX_RG8: 2, abi.TEX_R8: 1}.get(fmt, 4)
    if fmt == abi.TEX_RGBA32F:
        return rng.uniform(0.0, 1.0, (h, w, 4)).astype(F32)
    return rng.integers(0, 256, (h, w, c), dtype=np.uint8)


def _texture_set(sc, rng):
    """the R8 3x5 first, then every format at every size: {(format name, (w, h)): id}"""
    ids = {("r8", (3, 5)): sc.add_texture(_texels(rng, 3, 5, abi.TEX_R8), abi.TEX_R8)}
    for fname, fmt in FORMATS.items():
        for w, h in SIZES:
            ids[(fname, (w, h))] = sc.add_texture(_texels(rng, w, h, fmt), fmt)
    return ids


def _textured(**slots):
    return Material(base_color=(0.7, 0.6, 0.5, 1.0), emission=(0.6, 0.9, 1.2), emission_strength=2.5, roughness=0.8, metallic=0.6,
                    transmission=0.4, clearcoat=0.3, clearcoat_roughness=0.07, anisotropy=0.2, ior=1.45, **slots)


def slots_scene():
    rng = np.random.default_rng(2301)
    sc = scenes.Scene(name="slots")
    ids = _texture_set(sc, rng)
    mats = []
    for si, slot in enumerate(SLOTS):
        for fi, fname in enumerate(FORMATS):
            mats.append(_textured(**{slot: ids[(fname, SIZES[(si + fi) % len(SIZES)])]}))
    mats.append(_textured(transmission_texture=ids[("r8", (3, 5))]))
    mats.append(_textured(base_texture=ids[("srgb8", (64, 64))], rm_texture=ids[("rg8", (5, 7))], transmission_texture=ids[("r8", (2, 1))],
                          clearcoat_texture=ids[("r8", (1, 3))], emission_texture=ids[("f32", (5, 7))]))
    mats.append(_textured(base_texture=ids[("f32", (64, 64))], rm_texture=ids[("rgba8", (64, 64))], transmission_texture=ids[("rg8", (1, 1))],
                          clearcoat_texture=ids[("f32", (2, 1))], emission_texture=ids[("srgb8", (5, 7))]))
    assert len(mats) == 28
    mi = sc.add_mesh(meshes()["smooth"])
    sc.info = []
    for k in range(14):
        kind = list(KINDS)[k % 4]
        sc.add_instance(mi, _place(kind, k % 7, k // 7, 7, 2), mats[2 * k:2 * k + 2])
        sc.info.append(("smooth", kind))
    return _camera(sc, 7.5)


def _encode(s):
    return (np.asarray(s, F64) + 1.0) / 2.0


def normal_textures(sc, rng):
    def rand(w, h, spread):
        s = np.concatenate([rng.uniform(-spread, spread, (h, w, 2)), np.ones((h, w, 1))], axis=2)
        return np.concatenate([_encode(s / np.linalg.norm(s, axis=2, keepdims=True)), np.ones((h, w, 1))], axis=2)
    f32 = lambda px: sc.add_texture(np.asarray(px, F32), abi.TEX_RGBA32F)
    u8 = lambda px: sc.add_texture(np.round(np.asarray(px) * 255.0).astype(np.uint8), abi.TEX_RGBA8)
    # two texels on opposite sides of (0.5, 0.5, 0.5): halfway between them s = 2 c - 1 = 0.05 a, |N| = 0.034; it crosses |N| = 0 nearby
    a = np.array([0.5, -0.3, 0.35])
    gray = [[[*(0.5 + a), 1.0], [*(0.5 - 0.95 * a), 1.0]]]
    return {"flat32": f32([[[0.5, 0.5, 1.0, 1.0]]]), "tilt32": f32([[[*_encode((np.sin(TILT), 0.0, np.cos(TILT))), 1.0]]]),
            "rand32": f32(rand(5, 7, 0.6)), "rand8": u8(rand(64, 64, 0.6)), "flat8": u8([[[128 / 255, 128 / 255, 1.0, 1.0]] * 2]), "gray32": f32(gray)}


def normalmaps_scene():
    rng = np.random.default_rng(2302)
    sc = scenes.Scene(name="normalmaps")
    ids = _texture_set(sc, rng)
    nm = normal_textures(sc, rng)
    sc.normal_ids = nm
    mats = [_textured(normal_texture=nm[k]) for k in ("flat32", "tilt32", "rand32", "rand8", "flat8", "gray32")]
    mats.append(_textured(normal_texture=nm["rand8"], base_texture=ids[("srgb8", (5, 7))], rm_texture=ids[("rg8", (64, 64))],
                          transmission_texture=ids[("r8", (5, 7))], clearcoat_texture=ids[("rgba8", (1, 3))], emission_texture=ids[("f32", (2, 1))]))
    mats.append(_textured(normal_texture=nm["rand32"], base_texture=ids[("rgba8", (5, 7))], rm_texture=ids[("f32", (5, 7))],
                          transmission_texture=ids[("r8", (3, 5))], clearcoat_texture=ids[("r8", (64, 64))], emission_texture=ids[("srgb8", (64, 64))]))
    ms = meshes()
    names = ("ortho_p", "ortho_n", "smooth", "nxvar")
    sc.info = []
    for col, name in enumerate(names):
        mi = sc.add_mesh(ms[name])
        for row, kind in enumerate(KINDS):
            p = (row - col) % 4                      # (ortho_p, identity) and (ortho_n, rot_uniform) get the flat and the tilted texel
            sc.add_instance(mi, _place(kind, col, row, 4, 4), mats[2 * p:2 * p + 2])
            sc.info.append((name, kind))
    return _camera(sc, 5.5)


def _const_uv_mesh(uvs):
    """one triangle per (u, v): its three vertices share the UV, so that every hit on it samples at exactly that UV when u = v = 0"""
    v, n, t, uv = [], [], [], []
    for k, c in enumerate(uvs):
        x = 0.6 * (k % 8) - 2.1
        y = 0.6 * (k // 8) - 0.6
        v += [(x, y, 0), (x + 0.5, y, 0), (x, y + 0.5, 0)]
        n += [N0] * 3
        t += [[*tangent_at(N0, 90), 1.0]] * 3
        uv += [c] * 3
    return scenes._make_mesh(v, n, t, uv, np.arange(len(v)), [0] * len(uvs))


def uvpoints_scene():
    rng = np.random.default_rng(2303)
    sc = scenes.Scene(name="uvpoints")
    ids = _texture_set(sc, rng)
    pts = [0.0, 1.0, -1e-7, ONE_MINUS_EPS]
    uvs = [(a, b) for a in pts for b in pts] + [((i + 0.5) / 5, (j + 0.5) / 7) for i in (0, 2, 4) for j in (0, 3, 6)] + [(-(i + 0.5) / 5, 1 + (j + 0.5) / 7) for i, j in ((0, 0), (4, 6))]
    sc.uvs = uvs
    mat = _textured(base_texture=ids[("srgb8", (5, 7))], rm_texture=ids[("rg8", (5, 7))], transmission_texture=ids[("r8", (3, 5))],
                    clearcoat_texture=ids[("f32", (5, 7))], emission_texture=ids[("rgba8", (5, 7))])
    sc.add_instance(sc.add_mesh(_const_uv_mesh(uvs)), Transform(), [mat])
    sc.info = [("const_uv", "identity")]
    return _camera(sc, 6.0)


HUGE = [2.0 ** 23, 2.0 ** 24, 2.0 ** 31 - 128, 2.0 ** 31, 1e12]      # |uv size|


def edges_scene():
    rng = np.random.default_rng(2304)
    sc = scenes.Scene(name="edges")
    ids = _texture_set(sc, rng)
    zero = sc.add_texture(np.array([[[0.5, 0.5, 0.5, 1.0]]], F32), abi.TEX_RGBA32F)
    # instance 0: N = 0 exactly on an orthonormal quad
    sc.add_instance(sc.add_mesh(meshes()["ortho_p"]), Transform(), [_textured(normal_texture=zero)] * 2)
    # instance 1: tangents that interpolate to zero at (u, v) = (1/2, 0)
    zt = scenes._make_mesh([(-0.5, -0.5, 0), (0.5, -0.5, 0), (-0.5, 0.5, 0)], [(0, 0, 1)] * 3, [(1, 0, 0, 1), (-1, 0, 0, 1), (0, 1, 0, 1)], UV_CORNERS[:3], [0, 1, 2], [0])
    sc.add_instance(sc.add_mesh(zt), Transform(translation=(1.5, 0, 0)), [PLAIN[0]])
    # instance 2: constant UVs whose product with a 64-texel axis is HUGE, and with a 5- and a 7-texel axis reaches 2^31
    vals = [s * h / 64.0 for h in HUGE for s in (1, -1)] + [2.0 ** 31 / 7, -(2.0 ** 31) / 7, 2.0 ** 31 / 5, -(2.0 ** 31) / 5]
    sc.huge_uvs = [(a, a) for a in vals] + [(vals[6], 0.3), (0.3, vals[7])]
    mat = _textured(base_texture=ids[("srgb8", (64, 64))], rm_texture=ids[("rg8", (5, 7))], transmission_texture=ids[("r8", (3, 5))],
                    clearcoat_texture=ids[("f32", (64, 64))], emission_texture=ids[("rgba8", (5, 7))])
    sc.huge_textures = dict(albedo=ids[("srgb8", (64, 64))], rm=ids[("rg8", (5, 7))], transmission=ids[("r8", (3, 5))], clearcoat=ids[("f32", (64, 64))],
                            emission=ids[("rgba8", (5, 7))])
    sc.add_instance(sc.add_mesh(_const_uv_mesh(sc.huge_uvs)), Transform(translation=(0, 2.0, 0)), [mat])
    sc.info = [("ortho_p", "identity"), ("zero_tangent", "identity"), ("const_uv", "identity")]
    return _camera(sc, 6.0)


CASES = {"frames": frames_scene, "slots": slots_scene, "normalmaps": normalmaps_scene, "uvpoints": uvpoints_scene, "edges": edges_scene}
WITNESSED = [n for n in CASES if n != "edges"]


@functools.lru_cache(maxsize=None)
def scene(name):
    return CASES[name]()


def params(name):
    return make_params(SIZE[0], SIZE[1], SPP, BOUNCES, integrator=abi.INTEGRATOR_MIS, working_space=WORKING_SPACE)


def witness(name, constants):
    return sw.Witness(scene(name), gw.idt_of(constants))


# ---- records ---------------------------------------------------------------------------------------------------------------------------------
def triangles(name):
    """[(instance, primitive, three world-space corners float64)] of a case"""
    out = []
    sc = scene(name)
    for i, node in enumerate(sc.nodes):
        mesh = sc.meshes[node.mesh]
        Wm = np.asarray(node.world, F32).astype(F64)
        P = np.asarray(mesh.positions, F32)[:, :3].astype(F64)
        Pw = P[:, 0:1] * Wm[0, :3] + P[:, 1:2] * Wm[1, :3] + P[:, 2:3] * Wm[2, :3] + Wm[3, :3]
        for p, idx in enumerate(np.asarray(mesh.indices, np.int64).reshape(-1, 3)):
            out.append((i, p, Pw[idx]))
    return out


EYE = np.array([0.3, -0.2, 14.0])


def records(name, uv):
    """one record per triangle of the case and per (u, v) of `uv` (n, 2): the ray from EYE through the point the barycentrics name"""
    tris = triangles(name)
    uv = np.asarray(uv, F32)
    rec = np.zeros(len(tris) * len(uv), abi.SHADE_PROBE_IN_DTYPE)
    k = 0
    for i, p, c in tris:
        u, v = uv[:, 0].astype(F64)[:, None], uv[:, 1].astype(F64)[:, None]
        P = (1 - u - v) * c[0] + u * c[1] + v * c[2]
        d = P - EYE
        t = np.linalg.norm(d, axis=1)
        r = rec[k:k + len(uv)]
        r["instance"], r["primitive"], r["u"], r["v"], r["o"], r["d"], r["t"] = i, p, uv[:, 0], uv[:, 1], EYE, d / t[:, None], t
        k += len(uv)
    return rec


def lattice_uv(m=8):
    return np.array([(a / m, b / m) for a in range(m + 1) for b in range(m + 1 - a)], F32)


OUTSIDE_UV = np.array([(-1e-4, 0.3), (0.3, -1e-4), (0.5 + 5e-5, 0.5 + 5e-5), (-1e-4, -1e-4), (1 + 1e-4, -1e-4)], F32)


@functools.lru_cache(maxsize=None)
def batches(name):
    """The non-edge classes of a witnessed case: {class: records}"""
    rng = np.random.default_rng(77)
    r = rng.uniform(0, 1, (24, 2))
    r = np.where((r.sum(1) > 1)[:, None], 1 - r, r)
    return {"lattice": records(name, lattice_uv()), "outside": records(name, OUTSIDE_UV), "random": records(name, r)}


def hit_records(constants, hits, sample):
    """A side's own first hits of sample `sample` ((H, W) records {t, u, v, instance, primitive}) with the camera rays that made them, as
    probe records; the rays are rebuilt from the side's camera constants in float64 and rounded once."""
    h = np.asarray(hits).reshape(-1)
    cam = gw.camera_of(constants)
    fx, fy = gw.sample_positions(SIZE[0], SIZE[1], sample)
    d = gw.ray_directions(cam, fx, fy)
    sel = np.flatnonzero(h["instance"] >= 0)
    rec = np.zeros(len(sel), abi.SHADE_PROBE_IN_DTYPE)
    rec["instance"], rec["primitive"], rec["u"], rec["v"], rec["t"] = h["instance"][sel], h["primitive"][sel], h["u"][sel], h["v"][sel], h["t"][sel]
    rec["o"], rec["d"] = cam[0], d[sel]
    return rec


def measure_list():
    """Every (case, class) the bounds are measured over ("hits": the oracle's own first hits of sample 0)"""
    return [(n, c) for n in WITNESSED for c in list(batches(n)) + ["hits"]]


@functools.lru_cache(maxsize=None)
def edge_batches(name="edges"):
    """The "edges" class: N = 0, the zero tangent (with controls beside it), and the huge UVs at u = v = 0 (the UV exactly) and inside"""
    rec = records("edges", np.array([(0, 0), (0.5, 0), (0.25, 0.25), (0.5, 0.25)], F32))
    inst = rec["instance"]
    return {"n_zero": rec[inst == 0], "zero_tangent": rec[inst == 1], "huge_uv": rec[inst == 2]}


def grid_sizes():
    """batch sizes that span the grid-stride tail of a 256-thread block"""
    return [1, 255, 256, 257, 1 << 16]
