#!/usr/bin/env python3
"""Scenes in which EVERY leaf slot of the BVH builder's input is visible — TEST INFRASTRUCTURE (tests/test_bvh_layouts_host.py,
tests/test_gpu_bvh_builder.py).

mosaic(n, layout): a pinhole camera looks down -z at an image divided into cols x rows cells of cell_px pixels; slot i is a right triangle
(paired=True: a quad of two triangles that share an edge) over cell i, its vertices ON the camera rays through the cell's corners at depth z_i.
The footprint of a slot in the image therefore does not depend on its depth, no slot hides another, and a primary hit on every primitive id
says that the builder lost no slot and gave none a box that is too small.  The layouts choose z_i (or the cell arrangement) so that the
builder's input is degenerate in one named way; the picture stays the same.

usage: python tests/bvh_layouts.py N LAYOUT [paired]     slot count, image size and the oracle's coverage of one case
       python tests/bvh_layouts.py traversal [N:LAYOUT ...]   (needs the GPU) the tree the product builds for each case and what walking it
                                                              costs: the record in DESIGN.md section 3 "Builder tests"
"""
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from platinum_amd import abi, scenes  # noqa: E402

LAYOUTS = ("scatter", "flat", "line", "expo", "outlier", "coincident", "negative", "straddle")
SAMPLES = (0, 1, 2, 3)            # the sample indices every test traces
MARGIN = 0.02                     # a slot covers its cell from corner offset MARGIN to 1 - MARGIN
_HX = 18.0 / 50.0                 # half the image plane's width at distance 1: a 36 mm sensor behind a 50 mm lens
NEGATIVE_SHIFT = (-500.0, -700.0, -900.0)

def _grid(n, layout):
    cols = n if layout == "line" else int(np.ceil(np.sqrt(n)))
    return cols, (n + cols - 1) // cols


def _depths(n, layout):
    rng = np.random.default_rng(1)
    i = np.arange(n, dtype=np.float64)
    if layout in ("scatter", "negative", "straddle"):
        return rng.uniform(2.0, 20.0, n)
    if layout in ("flat", "line", "coincident"):
        return np.full(n, 4.0)
    if layout == "expo":   # z_i = g^i from 1 up to 1e15 (|x|, |y| <= 0.36 z): fp32 cross products of such edges stay finite
        return np.minimum(np.exp(i * (np.log(1e15) / max(1, n - 1))), 1e15)
    if layout == "outlier":
        z = rng.uniform(2.0, 3.0, n)
        z[n // 2] = 4e6
        return z
    raise KeyError(layout)


def _shift(layout, z, shift):
    if layout == "negative":
        return NEGATIVE_SHIFT
    if layout == "straddle":   # x and y cross 0 already (the camera looks at the middle of the grid); z does once the camera stands mid-depth
        return (0.25, -0.25, float(np.round(0.5 * (z.min() + z.max()) * 4.0) / 4.0))
    return tuple(float(s) for s in shift)


def _camera(sc, W, H, shift):
    sc.set_camera(scenes.Camera.with_focal_length(50.0, sensor_size=(36.0, 36.0 * H / W), aperture=0.0), scenes.Transform(translation=shift))


def _finish(sc, v, indices, tris):
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (len(v), 1))
    tg = np.tile(np.array([[1, 0, 0, 1]], np.float32), (len(v), 1))
    return sc.add_mesh(scenes._make_mesh(v.astype(np.float32), nrm, tg, np.zeros((len(v), 2), np.float32), indices, np.zeros(tris)))


def _material():
    return scenes.Material(base_color=(0.6, 0.5, 0.4, 1.0))


def mosaic(n, layout, cell_px=4, shift=(0, 0, 0), paired=False):
    """-> (scene, W, H): n leaf slots (n triangles; 2n when paired), one mesh, one instance, one material, a small sky environment."""
    cols, rows = _grid(n, layout)
    W, H = cols * cell_px, rows * cell_px
    hx, hy = _HX, _HX * H / W
    z = _depths(n, layout)
    shift = _shift(layout, z, shift)
    i = np.arange(n)
    cx, cy = (i % cols).astype(np.float64), (i // cols).astype(np.float64)
    m = MARGIN
    corners = [(m, m), (1 - m, m), (m, 1 - m), (1 - m, 1 - m)] if paired else [(m, m), (1 - m, m), (m, 1 - m)]
    if layout == "coincident":   # the same triangle n times, over the whole image and beyond: the lowest id wins every pixel
        cx, cy = np.zeros(n), np.zeros(n)
        corners = [(-1.0 * cols, -1.0 * rows), (4.0 * cols, -1.0 * rows), (-1.0 * cols, 4.0 * rows)]
        assert not paired
    k = len(corners)
    v = np.zeros((n, k, 3))
    for c, (a, b) in enumerate(corners):   # the point of the image plane at film position (cx + a, cy + b) cells, pushed out to depth z
        x = (2.0 * (cx + a) / cols - 1.0) * hx
        y = (1.0 - 2.0 * (cy + b) / rows) * hy
        v[:, c, 0], v[:, c, 1], v[:, c, 2] = x * z, y * z, -z
    v = (v + np.asarray(shift, np.float64)).reshape(-1, 3)
    if paired:   # (0, 1, 2) and (1, 3, 2): two vertex INDICES in common, which is what makes the two one leaf slot
        idx = (np.arange(n)[:, None] * 4 + np.array([[0, 1, 2, 1, 3, 2]])).reshape(-1)
    else:
        idx = np.arange(3 * n)
    sc = scenes.Scene(name="mosaic_%s_%d" % (layout, n))
    mesh = _finish(sc, v, idx, len(idx) // 3)
    sc.add_instance(mesh, scenes.Transform(), [_material()])
    sc.env_texture = sc.add_texture(scenes.sky_environment(16, 8), abi.TEX_RGBA32F)
    _camera(sc, W, H, shift)
    return sc, W, H


def instance_mosaic(n, cell_px=4):
    """The scatter picture from ONE single-triangle mesh instanced n times (translation and uniform scale): slot i is instance i."""
    cols, rows = _grid(n, "scatter")
    W, H = cols * cell_px, rows * cell_px
    hx, hy = _HX, _HX * H / W
    z = _depths(n, "scatter")
    dx, dy = 2.0 * hx / cols, 2.0 * hy / rows
    m = MARGIN
    v = np.array([[dx * a, -dy * b, 0.0] for a, b in ((m, m), (1 - m, m), (m, 1 - m))])   # cell (0, 0)'s triangle at depth 1, from the cell's corner
    sc = scenes.Scene(name="instance_mosaic_%d" % n)
    mesh = _finish(sc, v, np.arange(3), 1)
    for i in range(n):
        x0, y0 = (2.0 * (i % cols) / cols - 1.0) * hx, (1.0 - 2.0 * (i // cols) / rows) * hy
        sc.add_instance(mesh, scenes.Transform(translation=(x0 * z[i], y0 * z[i], -z[i]), scale=(z[i],) * 3), [_material()])
    sc.env_texture = sc.add_texture(scenes.sky_environment(16, 8), abi.TEX_RGBA32F)
    _camera(sc, W, H, (0.0, 0.0, 0.0))
    return sc, W, H


def missing_ids(hits, count, field="primitive"):
    """The ids in [0, count) that no pixel of one tracePrimary / trace_primary record array hit."""
    seen = np.zeros(count, bool)
    ids = hits[field][hits["instance"] >= 0]
    seen[ids[(ids >= 0) & (ids < count)]] = True
    return np.flatnonzero(~seen)


def world_bounds(scene):
    """(lo, hi) of the world-space vertices (fp32 positions through the fp32 instance matrices, in float64: for assertions on the layout only)."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for node in scene.nodes:
        p = scene.meshes[node.mesh].positions[:, :3].astype(np.float64)
        w = np.asarray(node.world, np.float64)
        q = p @ w[:3, :3] + w[3, :3]
        lo, hi = np.minimum(lo, q.min(0)), np.maximum(hi, q.max(0))
    return lo, hi


def build(n, layout, paired=False):
    """-> (scene, W, H, ids, field): `ids` values of hit-record field `field` must each be seen; layout "instances" = instance_mosaic."""
    if layout == "instances":
        sc, W, H = instance_mosaic(n)
        return sc, W, H, n, "instance"
    sc, W, H = mosaic(n, layout, paired=paired)
    return sc, W, H, sc.triangle_count, "primitive"


def oracle_primary(scene, W, H, use_bvh):
    """The oracle's trace_primary records of SAMPLES (one thread per sample: the call is serial and leaves the interpreter lock)."""
    import oracle_lib
    from concurrent.futures import ThreadPoolExecutor
    from platinum_amd.renderer import make_params
    o = oracle_lib.OracleScene(scene, make_params(W, H, 1, 2), use_bvh=use_bvh)
    with ThreadPoolExecutor(len(SAMPLES)) as pool:
        return list(pool.map(o.trace_primary, SAMPLES))


TRAVERSAL_RECORD = ((1024, "scatter"), (1025, "scatter"), (4097, "scatter"), (2049, "expo"), (2049, "outlier"))


def traversal(cases):
    """pt_stats after startRender + measureTraversal(0) of each (n, layout) in the session's structure: a record, no assertion."""
    from platinum_amd import Renderer
    r = Renderer(device=0)
    print("| layout, n | `bvh_nodes` | `bvh_max_depth` | `nodes_per_closest_ray` | `tris_per_closest_ray` |\n|---|---|---|---|---|")
    for n, layout in cases:
        sc, W, H, _, _ = build(n, layout)
        r.startRender(sc, (W, H), 1, max_bounces=2)
        r.measureTraversal(0)
        st = r.stats()
        print("| `%s` %d | %d | %d | %.2f | %.2f |" % (layout, n, st.bvh_nodes, st.bvh_max_depth, st.nodes_per_closest_ray, st.tris_per_closest_ray), flush=True)
    r.close()


def main(argv):
    if argv[1] == "traversal":
        return traversal([(int(a.split(":")[0]), a.split(":")[1]) for a in argv[2:]] or TRAVERSAL_RECORD)
    import oracle_lib
    from platinum_amd.renderer import make_params
    n, layout = int(argv[1]), argv[2]
    sc, W, H, count, field = build(n, layout, len(argv) > 3 and argv[3] == "paired")
    lo, hi = world_bounds(sc)
    print("%s n=%d: %d leaf slots, %d triangles, %d instances, image %dx%d, bounds %s .. %s" % (layout, n, n, sc.triangle_count, len(sc.nodes), W, H, lo.tolist(), hi.tolist()))
    p = make_params(W, H, 1, 2)
    brute, tree = oracle_lib.OracleScene(sc, p, use_bvh=False), oracle_lib.OracleScene(sc, p, use_bvh=True)
    for s in SAMPLES:
        hb, ht = brute.trace_primary(s), tree.trace_primary(s)
        miss = missing_ids(hb, count, field)
        print("  sample %d: brute force sees %d of %d ids (missing %s), %.0f %% of the pixels hit, tree == brute force: %s" %
              (s, count - len(miss), count, miss[:8].tolist(), 100.0 * (hb["instance"] >= 0).mean(), hb.tobytes() == ht.tobytes()))


if __name__ == "__main__":
    main(sys.argv)
