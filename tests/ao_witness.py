"""A float64 geometric witness for ambient-occlusion rays — TEST INFRASTRUCTURE, plain numpy.

It imports nothing from oracle/, tests/emu/ or platinum_amd/csrc/; it reuses geometry_witness.Triangles (the scene's world-space triangles in
float64) and geometry_witness._tuvc (Moeller-Trumbore by Cramer's rule, no early exit, no guard of its own).

An AO ray (P, dir, distance) is an any-hit ray over t in [1e-3, distance] (pt_ao.h): its answer is one bit.  fp32 cannot decide a ray that
passes within rounding of an edge or of either limit, so with geometry_witness's guard m = 1e-4 the witness names what every correct
implementation must answer:

  must be occluded  some triangle has min(u, v, w) >= +m, 1e-3 (1 + m) <= t <= distance (1 - m) and conditioning >= 1e-4
  must be open      no triangle has min(u, v, w) >= -m and 1e-3 (1 - m) <= t <= distance (1 + m)
  undecided         otherwise: both answers are allowed

The rays are a side's own float32 rays, promoted: the origin and the direction are held to their definitions by other checks
(ao_lib.check_origins, ao_lib.check_directions).  t is in units of |dir|, as the kernel's is.

normals(): the forward-matrix geometric normal of a triangle, normalize(M3 @ normalize(cross(p1 - p0, p2 - p0))) with p the OBJECT-space
corners — the reference's definition, which under a non-uniform scale is not the true normal."""
import numpy as np

import geometry_witness as gw

F64 = np.float64
M_GUARD = gw.M_GUARD
T_MIN = 1e-3          # kAoTmin: the shadow rays' near limit
COND_STRICT = gw.COND_STRICT
DECIDED_SHARE = gw.DECIDED_SHARE


def classify(T, P, d, distances, chunk_bytes=64 << 20):
    """{distance: (must_occluded, must_open)}: two bool arrays over the rays P (R, 3), d (R, 3) against the triangles T (gw.Triangles), for
    every far limit in `distances` (the rays of a camera sample do not depend on it: one brute-force pass serves all)."""
    P, d = np.asarray(P, F64).reshape(-1, 3), np.asarray(d, F64).reshape(-1, 3)
    R = len(P)
    occluded = {D: np.zeros(R, bool) for D in distances}
    may_hit = {D: np.zeros(R, bool) for D in distances}
    if T.count:
        v0, v1, v2 = T.v[None, :, 0], T.v[None, :, 1], T.v[None, :, 2]
        step = max(1, chunk_bytes // (8 * 3 * T.count))
        for a in range(0, R, step):
            t, u, v, cond = gw._tuvc(P[a:a + step, None, :], d[a:a + step, None, :], v0, v1, v2)
            with np.errstate(invalid="ignore"):
                lo = np.minimum(np.minimum(u, v), 1.0 - u - v)
                strict = (lo >= M_GUARD) & (t >= T_MIN * (1 + M_GUARD)) & (cond >= COND_STRICT)
                wide = (lo >= -M_GUARD) & (t >= T_MIN * (1 - M_GUARD))
                for D in distances:
                    occluded[D][a:a + step] = (strict & (t <= D * (1 - M_GUARD))).any(1)
                    may_hit[D][a:a + step] = (wide & (t <= D * (1 + M_GUARD))).any(1)
    return {D: (occluded[D], ~may_hit[D]) for D in distances}


def normals(T, scene):
    """(T.count, 3): the forward-matrix geometric normal of every triangle, float64"""
    out = np.zeros((T.count, 3))
    for i, node in enumerate(scene.nodes):
        mesh = scene.meshes[node.mesh]
        idx = np.asarray(mesh.indices, np.int64).reshape(-1, 3)
        p = np.asarray(mesh.positions, np.float32)[:, :3].astype(F64)[idx]
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        M3 = np.asarray(node.world, np.float32).astype(F64)[:3, :3].T      # [row][col]
        w = n @ M3.T
        out[T.base[i]:T.base[i + 1]] = w / np.linalg.norm(w, axis=1, keepdims=True)
    return out
