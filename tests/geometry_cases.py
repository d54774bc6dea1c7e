"""The scenes of the geometric witness (geometry_witness.py) — TEST INFRASTRUCTURE.  Small, seeded, opaque, pinhole cameras: at most ~7000
triangles each and at most 3072 rays per test, so that the float64 brute force costs under two seconds per case.

CASES maps a name to a Case: the scene factory, whether the 99 % "decided by the witness alone" condition applies (it does everywhere but on
the scenes BUILT for ties and edge-on views) and whether the scene has more than one instance (the two-level structure is checked there)."""
import functools
from collections import namedtuple

import numpy as np

import geometry_witness as gw
from platinum_amd import abi, scenes
from platinum_amd.scenes import Camera, Material, Transform

Case = namedtuple("Case", "build coverage instanced")

SIZES = ((48, 32), (50, 35))     # 50x35: partial 8x8 tiles in both directions
SAMPLES = (0, 1, 977)
RANDOM_SEEDS = (1, 2, 3, 5, 8, 12)


def _opaque_random(seed):
    """scenes.random_scene without textures, every base-colour alpha forced to 1, pinhole camera.  The seeds are chosen to hold mirrored and
    strongly anisotropic instances: asserted here, so that a change of the generator cannot quietly take them away."""
    sc = scenes.random_scene(seed, textures=False)
    for n in sc.nodes:
        for m in n.materials:
            m.base_color = tuple(m.base_color[:3]) + (1.0,)
            assert m.base_texture < 0 and m.normal_texture < 0
    sc.camera.aperture = 0.0
    return sc


def _scale_facts(sc):
    """(lowest determinant, largest ratio of singular values) over the instances of the solid meshes (cube, sphere: a plane has no extent along
    its own y axis, so the floor's scale (6, 1, 6) stretches nothing)"""
    dets, ratios = [], []
    for n in sc.nodes:
        if n.mesh == 0:
            continue
        m = np.asarray(n.world, np.float64)[:3, :3]
        s = np.linalg.svd(m, compute_uv=False)
        dets.append(np.linalg.det(m)); ratios.append(s.max() / s.min())
    return min(dets), max(ratios)


@functools.lru_cache(maxsize=None)
def _check_random_seeds():
    facts = [_scale_facts(_opaque_random(s)) for s in RANDOM_SEEDS]
    for s, (d, r) in zip(RANDOM_SEEDS, facts):
        assert d < 0, "seed %d holds no mirrored solid instance" % s
    assert max(r for _, r in facts) >= 3.0, "no solid instance with an anisotropic scale ratio >= 3"
    return facts


def truth_scene():
    """Spheres and cubes under rotation + UNIFORM scale only: the forward-matrix normal is the true normal here."""
    sc = scenes.Scene(name="truth")
    cube, ball, floor = sc.add_mesh(scenes.cube(1.0)), sc.add_mesh(scenes.sphere(0.6, 10, 14)), sc.add_mesh(scenes.plane(2.0))
    sc.add_instance(floor, Transform(scale=(5, 5, 5)), [Material(base_color=(0.7, 0.7, 0.6, 1.0))])
    rng = np.random.default_rng(41)
    for i in range(7):
        s = float(rng.uniform(0.4, 1.6))
        sc.add_instance(cube if i % 2 else ball,
                        Transform(translation=tuple(rng.uniform((-3, 0.4, -3), (3, 2.5, 2))), rotation=tuple(rng.uniform(-3.1, 3.1, 3)), scale=(s, s, s)),
                        [Material(base_color=tuple(rng.uniform(0.1, 1.0, 3)) + (1.0,))])
    sc.set_camera(Camera.with_focal_length(24.0), Transform(translation=(1.5, 3.0, 6.5), target=(0, 1, 0), track=True))
    return sc


def textured_scene():
    """The UV-order case: one RGBA32F base texture, random 5 x 7 (symmetric under no permutation of a triangle's corners), on a rotated,
    non-uniformly scaled cube and sphere and on the floor."""
    sc = scenes.Scene(name="uv_order")
    rng = np.random.default_rng(77)
    px = rng.random((5, 7, 4), dtype=np.float32)
    px[..., 3] = 1.0
    tex = sc.add_texture(px, abi.TEX_RGBA32F)
    mat = lambda: [Material(base_color=(0.3, 0.9, 0.5, 1.0), base_texture=tex)]
    cube, ball, floor = sc.add_mesh(scenes.cube(1.0)), sc.add_mesh(scenes.sphere(0.7, 9, 13)), sc.add_mesh(scenes.plane(2.0))
    sc.add_instance(floor, Transform(scale=(4, 1, 3)), mat())
    sc.add_instance(cube, Transform(translation=(-1.2, 1.0, 0.2), rotation=(0.5, 0.8, -0.3), scale=(1.7, 0.6, 1.1)), mat())
    sc.add_instance(ball, Transform(translation=(1.3, 1.2, -0.3), rotation=(-0.7, 0.4, 1.1), scale=(0.8, 1.9, 1.2)), mat())
    sc.add_instance(cube, Transform(translation=(0.2, 0.5, 1.6), rotation=(0.2, -1.0, 0.6), scale=(-0.9, 0.7, 0.5)),
                    [Material(base_color=(0.8, 0.2, 0.1, 1.0))])   # one mirrored, untextured
    sc.set_camera(Camera.with_focal_length(30.0), Transform(translation=(0.8, 3.2, 5.5), target=(0, 0.8, 0), track=True))
    return sc


def _mesh_of(tris, normal=(0, 1, 0)):
    v = np.concatenate([np.asarray(t, np.float32) for t in tris])
    n = np.tile(np.array([normal], np.float32), (len(v), 1))
    tg = np.tile(np.array([[1, 0, 0, 1]], np.float32), (len(v), 1))
    uv = np.zeros((len(v), 2), np.float32)
    return scenes._make_mesh(v, n, tg, uv, np.arange(len(v)), np.zeros(len(tris)))


_QUAD = [[[-2, 0, -2], [-2, 0, 2], [2, 0, -2]], [[2, 0, -2], [-2, 0, 2], [2, 0, 2]]]


def _tie_scene(copies, instances):
    sc = scenes.Scene(name="ties")
    m = sc.add_mesh(_mesh_of(_QUAD * copies))
    for _ in range(instances):
        sc.add_instance(m, Transform(), [Material(base_color=(0.6, 0.5, 0.4, 1.0))])
    sc.set_camera(Camera.with_focal_length(28.0), Transform(translation=(0, 2, 5), target=(0, 0, 0), track=True))
    return sc


def edge_on_scene():
    """A horizontal quad at the camera's own height, seen exactly edge-on through the image centre, in front of a wall: the rays of the
    middle rows run (nearly) in the quad's plane — the in-plane class of the contract."""
    sc = scenes.Scene(name="edge_on")
    quad, wall = sc.add_mesh(scenes.plane(2.0)), sc.add_mesh(scenes.plane(2.0))
    sc.add_instance(quad, Transform(translation=(0, 1, 0), scale=(1.5, 1, 1.5)), [Material(base_color=(0.9, 0.2, 0.2, 1.0))])
    sc.add_instance(wall, Transform(translation=(0, 1, -4), rotation=(np.pi / 2, 0, 0), scale=(6, 1, 6)), [Material(base_color=(0.2, 0.3, 0.9, 1.0))])
    sc.set_camera(Camera.with_focal_length(35.0), Transform(translation=(0, 1, 6), target=(0, 1, 0), track=True))
    return sc


def tmin_scene():
    """The near limit: the camera looks straight at a wall 5e-3 away, through a second wall 9e-4 away.  Along the axis the near wall lies
    below tmin = 1e-3 and must be passed; t = 9e-4 / cos(angle) crosses 1e-3 inside the image, so towards the corners it is the hit."""
    # (everything sits at the origin and the walls are 0.04 wide: a coordinate of magnitude 1 would carry a float32 rounding of 6e-8, which is
    # 1e-4 of these distances — the scene would measure the flattening's rounding, not the near limit)
    sc = scenes.Scene(name="tmin")
    wall = sc.add_mesh(scenes.plane(2.0))
    s = (0.02, 0.02, 0.02)
    sc.add_instance(wall, Transform(translation=(0, 0, -5e-3), rotation=(np.pi / 2, 0, 0), scale=s), [Material(base_color=(0.2, 0.8, 0.3, 1.0))])
    sc.add_instance(wall, Transform(translation=(0, 0, -9e-4), rotation=(np.pi / 2, 0, 0), scale=s), [Material(base_color=(0.8, 0.3, 0.2, 1.0))])
    sc.set_camera(Camera.with_focal_length(28.0), Transform(translation=(0, 0, 0), target=(0, 0, -1), track=True))
    return sc


CASES = {
    "cornell": Case(lambda: scenes.cornell_scene("bench"), True, False),
    "cornell_sphere": Case(scenes.cornell_sphere_scene, True, True),
    "pairing": Case(scenes.pairing_edge_cases_scene, False, True),   # built for ties: duplicates with their corners in another order
    "truth": Case(truth_scene, True, True),
    "uv_order": Case(textured_scene, True, True),
    "tmin": Case(tmin_scene, True, True),
    "coincident_copies": Case(lambda: _tie_scene(40, 1), False, False),
    "three_instances_same_place": Case(lambda: _tie_scene(1, 3), False, True),
    "edge_on": Case(edge_on_scene, False, True),
}
for _s in RANDOM_SEEDS:
    CASES["random%d" % _s] = Case(functools.partial(_opaque_random, _s), True, True)
TRUTH_CASES = ("truth",)           # normals there are checked against the true normal as well
CAMERAS = {
    # name: (position, target, focal length, sensor)
    "bench": ((0, 5, 15), (0, 5, 0), 28.0, (36.0, 24.0)),
    "default": ((-5, 5, 5), (0, 0, 0), 28.0, (36.0, 24.0)),
    "long_oblique": ((7.5, 0.75, -3.25), (-1, 2.5, 0.5), 135.0, (36.0, 24.0)),
}


def camera_scene(name):
    pos, target, f, sensor = CAMERAS[name]
    sc = scenes.cornell_scene("bench")
    sc.set_camera(Camera.with_focal_length(f, sensor_size=sensor), Transform(translation=pos, target=target, track=True))
    return sc


@functools.lru_cache(maxsize=None)
def scene(name):
    if name.startswith("random"):
        _check_random_seeds()
    return CASES[name].build()


@functools.lru_cache(maxsize=None)
def triangles(name):
    return gw.Triangles(scene(name))


_witnesses = {}


def witness(name, constants, W, H, sample):
    """The witness of a case for a side's constants: built once per (case, size, sample, camera bits) and shared by every test of the session."""
    key = (name, W, H, sample, bytes(constants.camera), bytes(bytearray(constants.idt)))
    if key not in _witnesses:
        _witnesses[key] = gw.Witness(scene(name), constants, W, H, sample, tris=triangles(name))
    return _witnesses[key]
