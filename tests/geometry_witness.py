"""A float64 geometric witness for first hits and first-hit AOVs — TEST INFRASTRUCTURE, plain numpy.

Everything else that checks which triangle a camera ray hits compares two programs by the same author (device bits == oracle bits).  This
module answers the same question from the scene description alone: it reads a `scenes.Scene` (meshes, node matrices, materials, textures)
and a side's camera constants, builds the camera rays of one sample, and intersects every ray with every world-space triangle in float64,
brute force.  It imports nothing from oracle/, tests/emu/ or platinum_amd/csrc/; its ray / triangle test is Moeller-Trumbore written from the
paper's formulas (Cramer's rule on o + t d = (1-u-v) v0 + u v1 + v v2) in float64, with no early exit and no guard of its own.

Allowed answers.  fp32 cannot decide a ray that passes within rounding of an edge, of the near limit, or in a triangle's plane, so the
witness does not name one answer per ray but the SET of answers the intersection contract leaves open, with one guard
m = kCullSlack - 1 = 1e-4 (pt_bvh.h: the contract's own slack, not a measured value):

  S_strict  triangles with min(u, v, w) >= +m, t >= 1e-3 (1 + m) and conditioning |det| / (|e1|_1 |d x e2|_1) >= 1e-4 (100 x the kernel's
            in-plane guard of 1e-6): hits no correct fp32 implementation may lose
  S_wide    triangles with min(u, v, w) >= -m and t >= 1e-3 (1 - m): hits a correct implementation may report
  t_lo = min t over S_wide, t_hi = min t over S_strict (inf when empty)
  a hit on k is allowed  <=>  k in S_wide and t_lo <= t_k <= t_hi (1 + m)
  a miss is allowed      <=>  S_strict is empty
  exact ties: among allowed COINCIDENT COPIES (the same three world-space corners in the same order, float64 t equal to 1e-12 relative) only
            the lowest (instance, primitive) stays allowed — the contract's tie rule.  Copies are the one case in which every fp32
            implementation of the contract computes the same t bit for bit; two coplanar neighbours also share t along their common edge,
            and a duplicate with its corners in another order rounds differently: there the guard band decides, and both stay allowed
  a ray is DECIDED when exactly one answer is allowed.

What is compared for an allowed hit on triangle k: |t - t_k| / t_k, and the distance between the point rebuilt from the side's own float32
(u, v), (1-u-v) v0 + u v1 + v v2, and the witness point o + t_k d, relative to t_k.  Raw u and v are NOT compared: they are ill-conditioned
on thin triangles at grazing incidence (1.2e-3 absolute was seen on a well-behaved scene) while the point they describe is not.

AOVs of a hit on triangle k (materials without a normal map):
  normal  normalize(M3 @ (w* n0 + u* n1 + v* n2)) with M3 the FORWARD 3x3 of the node and (u*, v*) the witness barycentrics.  This is the
          reference's definition (transformVec, kernel.metal:150-162), NOT the inverse transpose: under a non-uniform scale it is not the
          true normal, and that is kept on purpose ("normals by the forward matrix").  Under rotation + uniform scale it
          is also the true normal; geometry_cases.truth_scene holds only such instances, so there the check is against truth.
  depth   t_k;  hit flag 1
  albedo  idt @ baseColor, or with a base texture (TEX_RGBA32F, no alpha) idt @ bilinear_repeat(texture, w* uv0 + u* uv1 + v* uv2)

Out of scope: alpha cut-outs (the alpha test drops hits by a random draw), thin-lens cameras, normal-mapped materials, hits of later bounces
and shadow rays (their rays cannot be observed through the ABI), the BSDF.

BOUNDS.  Each bound is 4 x the worst value of the ORACLE (oracle/pt_oracle.cpp: its tree and its brute force; the AOVs are HostScene.stage_aov
on the tree's hits) against this witness over every case of geometry_cases.CASES, sizes 48x32 and 50x35, samples 0, 1 and 977, measured on
the host; test_geometry_witness_host.py measures them again and holds MEASURED below to the result.  The factor is for scenes and samples
not in the list: fp32 error here scales with the conditioning of the worst triangle met, and a wider sweep meets somewhat worse ones.  The
host build of the product and the device are held to the same table; no figure in it comes from the device.

  quantity                                                            measured worst (oracle)   where                        asserted (4 x)
  ------------------------------------------------------------------  ------------------------  ---------------------------  --------------
  t        |t - t_k| / t_k   (the depth AOV is held to the same)       1.46e-5                   uv_order 50x35 sample 977    5.84e-5
  point    |P(u, v) - (o + t_k d)| / t_k                               1.49e-5                   uv_order 50x35 sample 977    5.96e-5
  normal   max |n - n*| over the components of a unit vector           5.67e-5                   truth 50x35 sample 1         2.27e-4
  albedo   max |a - a*| over rgb (textured; untextured is 7e-8)        3.03e-5                   uv_order 50x35 sample 1      1.21e-4
"""
import json
import os

import numpy as np

import math_lib
from texture_ref import _bilinear_repeat as bilinear_repeat

F64 = np.float64
M_GUARD = 1e-4        # kCullSlack - 1 (pt_bvh.h)
T_MIN = 1e-3          # the near limit of a camera ray (closest = min t in [1e-3, tmax])
COND_STRICT = 1e-4    # 100 x the in-plane guard 1e-6 of intersect_triangle
TIE_REL = 1e-12
DECIDED_SHARE = 0.99  # of the rays of every case not built for ties or edge-on views

# measured worst of the oracle against the witness (see the docstring), and the asserted bounds = 4 x
MEASURED = {"t": 1.46e-5, "point": 1.49e-5, "normal": 5.67e-5, "albedo": 3.03e-5}
BOUNDS = {k: 4.0 * v for k, v in MEASURED.items()}


# ---- the sampler's integer part, restated (samplers.metal:16-23, 154-156) and checked against tests/golden/sampler_kat.json on import ------
def _pcg4d_x(x, y, z, w):
    U = np.uint32
    with np.errstate(over="ignore"):
        x, y, z, w = (a.astype(U) * U(1664525) + U(1013904223) for a in (x, y, z, w))
        x = x + y * w; y = y + z * x; z = z + x * y; w = w + y * z
        x = x ^ (x >> U(16)); y = y ^ (y >> U(16)); z = z ^ (z >> U(16)); w = w ^ (w >> U(16))
        x = x + y * w
    return x


def halton_offset(px, py, sample):
    px, py = np.asarray(px, np.uint32), np.asarray(py, np.uint32)
    s = np.full(px.shape, sample, np.uint32)
    with np.errstate(over="ignore"):
        return _pcg4d_x(px, py, s, px + py)


def _check_offsets():
    kat = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_kat.json")))["offsets"]
    for x, y, s, want in kat:
        got = int(halton_offset(np.array([x]), np.array([y]), s)[0])
        assert got == want, (x, y, s, got, want)


_check_offsets()


# ---- scene -> world-space triangles ----------------------------------------------------------------------------------------------------------
class Triangles:
    """Every triangle of every node, in world space, float64; ids = (node index, triangle index inside the mesh)."""

    def __init__(self, scene):
        v, nrm, uv, inst, prim, m3, mat = [], [], [], [], [], [], []
        self.base = np.zeros(len(scene.nodes) + 1, np.int64)
        self.materials = []
        for i, node in enumerate(scene.nodes):
            mesh = scene.meshes[node.mesh]
            idx = np.asarray(mesh.indices, np.int64).reshape(-1, 3)
            P = np.asarray(mesh.positions, np.float32)[:, :3].astype(F64)
            Wm = np.asarray(node.world, np.float32).astype(F64)          # [col][row]
            c0, c1, c2, c3 = Wm[0, :3], Wm[1, :3], Wm[2, :3], Wm[3, :3]
            Pw = P[:, 0:1] * c0 + P[:, 1:2] * c1 + P[:, 2:3] * c2 + c3
            vd = np.asarray(mesh.vertex_data, np.float32).astype(F64)
            v.append(Pw[idx])                                            # (T, 3 corners, 3)
            nrm.append(vd[:, 0:3][idx])
            uv.append(vd[:, 8:10][idx])
            inst.append(np.full(len(idx), i, np.int64))
            prim.append(np.arange(len(idx), dtype=np.int64))
            m3.append(np.broadcast_to(np.stack([c0, c1, c2], axis=1), (len(idx), 3, 3)))   # M3[r][c] = column c, row r
            slots = np.asarray(mesh.material_slots, np.int64)
            mat.append(len(self.materials) + slots)
            self.materials += list(node.materials)
            self.base[i + 1] = self.base[i] + len(idx)
        cat = lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape)
        self.v = cat(v, (0, 3, 3))
        self.n = cat(nrm, (0, 3, 3))
        self.uv = cat(uv, (0, 3, 2))
        self.inst = cat(inst, (0,)).astype(np.int64)
        self.prim = cat(prim, (0,)).astype(np.int64)
        self.m3 = cat(m3, (0, 3, 3))
        self.mat = cat(mat, (0,)).astype(np.int64)
        self.count = len(self.v)
        self.textures = scene.textures


def camera_of(constants):
    """(o, topLeft, dU, dV) of a side's constants(): float32 inputs, promoted."""
    c = constants.camera
    assert c.apertureRadius == 0.0, "pinhole cameras only"
    g = lambda f: np.array([f.x, f.y, f.z], np.float32).astype(F64)
    return g(c.position), g(c.topLeft), g(c.pixelDeltaU), g(c.pixelDeltaV)


def idt_of(constants):
    return np.array([[v.x, v.y, v.z] for v in constants.idt], np.float32).astype(F64).T   # columns -> [row][col]


def sample_positions(W, H, sample):
    """(fx, fy) of every pixel, row-major: float32(px) + float32(jitter), formed in float32 — the definition of the sample position."""
    py, px = np.mgrid[0:H, 0:W]
    px, py = px.ravel(), py.ravel()
    off = halton_offset(px, py, sample)
    jx = math_lib.halton_reference(off, np.zeros(off.size, np.uint32))
    jy = math_lib.halton_reference(off, np.ones(off.size, np.uint32))
    fx = (px.astype(np.float32) + jx.astype(np.float32)).astype(np.float32)
    fy = (py.astype(np.float32) + jy.astype(np.float32)).astype(np.float32)
    return fx.astype(F64), fy.astype(F64)


def ray_directions(cam, fx, fy):
    o, tl, du, dv = cam
    d = tl + fx[:, None] * du + fy[:, None] * dv - o
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _tuvc(o, d, v0, v1, v2):
    """t, u, v and the conditioning number |det| / (|e1|_1 |d x e2|_1) for broadcastable rays d and triangles (v0, v1, v2): Cramer's rule on
    o + t d = v0 + u e1 + v e2 (Moeller & Trumbore 1997).  A zero determinant gives inf / nan, which no comparison below accepts."""
    e1, e2, s = v1 - v0, v2 - v0, o - v0
    p = _cross(d, e2)
    det = (e1 * p).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (s * p).sum(-1) / det
        q = _cross(s, e1)
        v = (d * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
        cond = np.abs(det) / (np.abs(e1).sum(-1) * np.abs(p).sum(-1))
    return t, u, v, cond


class Witness:
    """The allowed answers of every camera ray of sample `sample` at W x H, for the camera in `constants`."""

    def __init__(self, scene, constants, W, H, sample, tris=None, chunk_bytes=64 << 20):
        self.T = tris if tris is not None else Triangles(scene)
        self.W, self.H, self.sample = W, H, sample
        self.cam = camera_of(constants)
        self.idt = idt_of(constants)
        fx, fy = sample_positions(W, H, sample)
        self.o = self.cam[0]
        self.d = ray_directions(self.cam, fx, fy)
        R, T = len(self.d), self.T.count
        self.allow_miss = np.ones(R, bool)
        ray_ids, tri_ids, ts = [], [], []
        if T:
            v0, v1, v2 = self.T.v[None, :, 0], self.T.v[None, :, 1], self.T.v[None, :, 2]
            step = max(1, chunk_bytes // (8 * 3 * T))      # the (rays, T, 3) cross product is the largest temporary; ~12 such arrays live
            for a in range(0, R, step):
                d = self.d[a:a + step, None, :]
                t, u, v, cond = _tuvc(self.o, d, v0, v1, v2)
                with np.errstate(invalid="ignore"):
                    lo = np.minimum(np.minimum(u, v), 1.0 - u - v)
                    strict = (lo >= M_GUARD) & (t >= T_MIN * (1 + M_GUARD)) & (cond >= COND_STRICT)
                    wide = (lo >= -M_GUARD) & (t >= T_MIN * (1 - M_GUARD))
                    t_lo = np.where(wide, t, np.inf).min(1)
                    t_hi = np.where(strict, t, np.inf).min(1)
                    ok = wide & (t >= t_lo[:, None]) & (t <= (t_hi * (1 + M_GUARD))[:, None])
                self.allow_miss[a:a + step] = ~strict.any(1)
                r, k = np.nonzero(ok)
                ray_ids.append(r + a); tri_ids.append(k); ts.append(t[r, k])
        ray_ids = np.concatenate(ray_ids) if ray_ids else np.zeros(0, np.int64)
        tri_ids = np.concatenate(tri_ids) if tri_ids else np.zeros(0, np.int64)
        ts = np.concatenate(ts) if ts else np.zeros(0)
        keep = self._tie_rule(ray_ids, tri_ids, ts)
        self.ray_ids, self.tri_ids, self.ts = ray_ids[keep], tri_ids[keep], ts[keep]
        self.n_hits = np.bincount(self.ray_ids, minlength=R)
        self.decided = (self.n_hits + self.allow_miss) == 1
        # the decided answer: triangle index, or -1 for a decided miss (undefined where not decided)
        self.k = np.full(R, -1, np.int64)
        one = self.n_hits[self.ray_ids] == 1
        self.k[self.ray_ids[one]] = self.tri_ids[one]
        self.k[~self.decided] = -1
        self.decided_hit = self.decided & ~self.allow_miss
        self._keys = self.ray_ids * max(T, 1) + self.tri_ids

    def _tie_rule(self, ray_ids, tri_ids, ts):
        """Triangle indices grow with (instance, primitive).  Entries come sorted by ray, then by triangle: drop an entry when an earlier
        entry of the same ray is a coincident copy of it (the same three world-space corners in the same order) with the same t to TIE_REL."""
        keep = np.ones(len(ray_ids), bool)
        if not len(ray_ids):
            return keep
        starts = np.flatnonzero(np.r_[True, ray_ids[1:] != ray_ids[:-1]])
        ends = np.r_[starts[1:], len(ray_ids)]
        for a, b in zip(starts, ends):
            if b - a > 1:
                t, c = ts[a:b], self.T.v[tri_ids[a:b]].reshape(b - a, 9)
                same = (np.abs(t[:, None] - t[None, :]) <= TIE_REL * np.abs(t[:, None])) & (c[:, None, :] == c[None, :, :]).all(-1)
                keep[a:b] = ~np.tril(same, -1).any(1)
        return keep

    @property
    def decided_share(self):
        return float(self.decided.mean())

    # ---- a side's hit records against the allowed sets ----
    def pair(self, rays, k):
        """float64 (t, u, v) of ray r on triangle k, pairwise"""
        t, u, v, _ = _tuvc(self.o, self.d[rays], self.T.v[k, 0], self.T.v[k, 1], self.T.v[k, 2])
        return t, u, v

    def check_hits(self, hits):
        """hits: (H, W) records {t, u, v, instance, primitive}.  Returns (bad, err): `bad` = indices of rays whose answer is not allowed;
        `err` = {"t", "point"} worst errors over the hits, with the ray at which each occurs, and `k` = the answered triangle per ray (-1 = miss)."""
        h = np.asarray(hits).reshape(-1)
        assert h.size == self.W * self.H
        inst, prim = h["instance"].astype(np.int64), h["primitive"].astype(np.int64)
        miss = inst < 0
        k = np.where(miss, -1, self.T.base[np.clip(inst, 0, len(self.T.base) - 2)] + prim)
        rays = np.arange(h.size)
        allowed = np.where(miss, self.allow_miss, np.isin(rays * max(self.T.count, 1) + k, self._keys))
        in_mesh = miss | ((prim >= 0) & (k < self.T.base[np.clip(inst, 0, len(self.T.base) - 2) + 1]))
        bad = np.flatnonzero(~(allowed & in_mesh))
        hr = np.flatnonzero(~miss & allowed & in_mesh)
        err = {"t": (0.0, -1), "point": (0.0, -1), "k": k}
        if hr.size:
            kk = k[hr]
            tk, _, _ = self.pair(hr, kk)
            et = np.abs(h["t"][hr].astype(F64) - tk) / tk
            u, v = h["u"][hr].astype(F64)[:, None], h["v"][hr].astype(F64)[:, None]
            P = (1.0 - u - v) * self.T.v[kk, 0] + u * self.T.v[kk, 1] + v * self.T.v[kk, 2]
            ep = np.linalg.norm(P - (self.o + tk[:, None] * self.d[hr]), axis=1) / tk
            err["t"] = (float(et.max()), int(hr[et.argmax()]))
            err["point"] = (float(ep.max()), int(hr[ep.argmax()]))
        return bad, err

    def describe(self, ray, hits=None):
        a = self.ray_ids == ray
        s = "ray %d (x %d, y %d): allowed %s, miss allowed %s" % (ray, ray % self.W, ray // self.W, [
            (int(self.T.inst[k]), int(self.T.prim[k]), float(t)) for k, t in zip(self.tri_ids[a], self.ts[a])], bool(self.allow_miss[ray]))
        if hits is not None:
            s += "; answered %s" % (np.asarray(hits).reshape(-1)[ray],)
        return s

    # ---- AOVs ----
    def aov(self, rays, k):
        """Witness AOVs of rays `rays` hitting triangles `k`: dict of normal (n, 3), depth (n,), albedo (n, 3)."""
        T = self.T
        t, u, v = self.pair(rays, k)
        w = 1.0 - u - v
        n_os = w[:, None] * T.n[k, 0] + u[:, None] * T.n[k, 1] + v[:, None] * T.n[k, 2]
        n = np.einsum("nrc,nc->nr", T.m3[k], n_os)                       # the FORWARD matrix (kernel.metal:150-162), on purpose
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        uv = w[:, None] * T.uv[k, 0] + u[:, None] * T.uv[k, 1] + v[:, None] * T.uv[k, 2]
        for mat in {T.mat[j] for j in k}:
            mat = T.materials[mat]
            assert mat.normal_texture < 0 and not mat.base_texture_has_alpha and mat.base_color[3] >= 1.0, "out of scope for the witness"
        alb = np.array([T.materials[m].base_color[:3] for m in T.mat[k]], np.float32).astype(F64).reshape(len(k), 3)
        for j in np.flatnonzero([T.materials[m].base_texture >= 0 for m in T.mat[k]]):
            alb[j] = bilinear_repeat(T.textures[T.materials[T.mat[k[j]]].base_texture].pixels, uv[j, 0], uv[j, 1])[:3]
        return {"normal": n, "depth": t, "albedo": alb @ self.idt.T}


# ---- the assertions every side is held to ---------------------------------------------------------------------------------------------------------
def check_hits(w, hits, what):
    """The assertions every side is held to; returns the answered triangle per ray."""
    bad, err = w.check_hits(hits)
    print("%s: t %.3e (ray %d)  point %.3e (ray %d)  decided %.4f" % (what, err["t"][0], err["t"][1], err["point"][0], err["point"][1], w.decided_share))
    assert bad.size == 0, "%s: %d answers outside the allowed set; %s" % (what, bad.size, w.describe(int(bad[0]), hits))
    assert err["t"][0] <= BOUNDS["t"], (what, err["t"], w.describe(err["t"][1], hits))
    assert err["point"][0] <= BOUNDS["point"], (what, err["point"], w.describe(err["point"][1], hits))
    return err["k"]


def check_aovs(w, rays, k, albedo, normal, depth, what):
    """albedo / normal (n, 4 or 3) and depth (n,) of rays `rays` that hit triangles `k`"""
    ref = w.aov(rays, k)
    en = np.abs(normal[:, :3].astype(np.float64) - ref["normal"]).max(axis=1)
    ea = np.abs(albedo[:, :3].astype(np.float64) - ref["albedo"]).max(axis=1)
    ed = np.abs(depth.astype(np.float64) - ref["depth"]) / ref["depth"]
    print("%s: normal %.3e  albedo %.3e  depth %.3e  over %d hits" % (what, en.max(), ea.max(), ed.max(), rays.size))
    for name, e, bound in (("normal", en, BOUNDS["normal"]), ("albedo", ea, BOUNDS["albedo"]), ("depth", ed, BOUNDS["t"])):
        j = int(e.argmax())
        assert e[j] <= bound, (what, name, float(e[j]), w.describe(int(rays[j])), ref[name][j])


# ---- camera constants ------------------------------------------------------------------------------------------------------------------------
def check_camera(constants, W, H, position, target, sensor_size, focal_length, focus_distance=1.0, tol=2e-6):
    """A tracking camera's constants against the geometry they stand for.  `tol` is relative: a few float32 roundings of O(1) unit vectors and
    of the look-at basis (2^-23 = 1.2e-7 each; lookAt, its inverse and the scale removal chain about ten of them)."""
    o, tl, du, dv = camera_of(constants)
    position, target = np.asarray(position, np.float32).astype(F64), np.asarray(target, np.float32).astype(F64)
    assert np.abs(o - position).max() <= tol * max(1.0, np.abs(position).max()), (o, position)   # (it comes back through inverse(lookAt))
    c = tl + (W / 2.0) * du + (H / 2.0) * dv - o
    c /= np.linalg.norm(c)
    f = (target - position) / np.linalg.norm(target - position)
    assert np.abs(c - f).max() < tol, (c, f)
    # field of view: the sensor is cropped to the image's aspect when the image is wider (camera.hpp:47-50), vh = focus * cropped height / f
    aspect, sensor_aspect = W / H, sensor_size[0] / sensor_size[1]
    vh = focus_distance * (sensor_size[0] / max(sensor_aspect, aspect)) / focal_length
    nu, nv = np.linalg.norm(du), np.linalg.norm(dv)
    assert abs(nv * H / vh - 1) < tol and abs(nu * W / (vh * aspect) - 1) < tol, (nu * W, nv * H, vh)
    assert abs(du @ dv) / (nu * nv) < tol and abs(du @ c) / nu < tol and abs(dv @ c) / nv < tol
    # orientation: x grows to the camera's right, y grows DOWN the image (topLeft is the upper left corner): (dU, -dV, -centre) is right-handed,
    # and with the world's y axis as `up` the image's up direction has a positive y component
    assert (np.cross(du, -dv) @ -c) / (nu * nv) > 1 - tol
    if not (position[0] == target[0] and position[2] == target[2]):
        assert -dv[1] > 0
    # the distance of the image plane: (topLeft + W/2 dU + H/2 dV - o) has length `focus_distance`
    assert abs(np.linalg.norm(tl + (W / 2.0) * du + (H / 2.0) * dv - o) / focus_distance - 1) < tol
