"""The float64 geometric witness (geometry_witness.py) for rays that do not share an origin — TEST INFRASTRUCTURE, plain numpy.

ProjectionWitness takes the camera rays as arrays (origins and directions per ray, float64: projection_lib.restated_rays, written from the
header's text) and nothing of the product.  It subclasses geometry_witness.Witness and reuses its Triangles, its Moeller-Trumbore (_tuvc),
its guards (M_GUARD, T_MIN, COND_STRICT) and its tie rule; only the places that read the one origin are restated for an origin per ray.

What a side's hits are held to (check_hits below): the membership rule of geometry_witness on EVERY ray, and the t / point bounds on the
allowed hits whose incidence has tan <= 8 (angle between the ray and the triangle's normal): the projected cameras sit inside the scenes and
look everywhere, floors and walls at grazing angles included, where an error Delta in the ray moves the hit point along the surface by
Delta * t * tan.  The bounds, with D the direction bound of the kind (projection_lib.D) and E_o the origin bound:
    Delta = sqrt(3) * D + E_o / t          the ray's own error at the hit, relative to t (|d - d*|_2 <= sqrt(3) D)
    point <= BOUNDS["point"] + Delta
    t     <= BOUNDS["t"] + 8 * Delta       (t moves by Delta * tan, tan <= 8)
These hits must be at least 95 % of the decided hits, and the witness must decide at least 99 % of the rays."""
import numpy as np

import geometry_witness as gw
from geometry_witness import F64, M_GUARD, T_MIN, COND_STRICT, _tuvc

TAN_MAX = 8.0
BOUNDED_SHARE = 0.95


class ProjectionWitness(gw.Witness):
    """The allowed answers of rays (o[r], d[r]) over the triangles of `scene`.

    KEEP IN STEP with geometry_witness.py, which may not take a hook: __init__ below is Witness.__init__ from "R, T = len(self.d), ..." to
    "self._keys = ..." with `self.o` replaced by the chunk's origins self.o[a:a + step, None, :] (its lines 201-233); pair is Witness.pair
    with self.o[rays] (256-258); check_hits is Witness.check_hits (260-283) up to `hr`, then keeps the per-hit arrays where the original
    keeps their maxima.  The guards, the allowed-answer rule and the tie rule are the original's own: a change there must be repeated here."""

    def __init__(self, scene, o, d, W, H, sample, idt=None, tris=None, chunk_bytes=64 << 20):
        self.T = tris if tris is not None else gw.Triangles(scene)
        self.W, self.H, self.sample = W, H, sample
        self.idt = idt
        self.o = np.asarray(o, F64).reshape(-1, 3)
        self.d = np.asarray(d, F64).reshape(-1, 3)
        assert len(self.o) == len(self.d) == W * H
        R, T = len(self.d), self.T.count
        self.allow_miss = np.ones(R, bool)
        ray_ids, tri_ids, ts = [], [], []
        if T:
            v0, v1, v2 = self.T.v[None, :, 0], self.T.v[None, :, 1], self.T.v[None, :, 2]
            step = max(1, chunk_bytes // (8 * 3 * T))
            for a in range(0, R, step):
                t, u, v, cond = _tuvc(self.o[a:a + step, None, :], self.d[a:a + step, None, :], v0, v1, v2)
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
        self.k = np.full(R, -1, np.int64)
        one = self.n_hits[self.ray_ids] == 1
        self.k[self.ray_ids[one]] = self.tri_ids[one]
        self.k[~self.decided] = -1
        self.decided_hit = self.decided & ~self.allow_miss
        self._keys = self.ray_ids * max(T, 1) + self.tri_ids

    def pair(self, rays, k):
        t, u, v, _ = _tuvc(self.o[rays], self.d[rays], self.T.v[k, 0], self.T.v[k, 1], self.T.v[k, 2])
        return t, u, v

    def tan_incidence(self, rays, k):
        """tan of the angle between ray and triangle normal, pairwise"""
        n = np.cross(self.T.v[k, 1] - self.T.v[k, 0], self.T.v[k, 2] - self.T.v[k, 0])
        c = np.abs((n * self.d[rays]).sum(1))
        s = np.linalg.norm(np.cross(n, self.d[rays]), axis=1)
        with np.errstate(divide="ignore"):
            return s / c

    def check_hits(self, hits):
        """As geometry_witness.Witness.check_hits, with per-hit arrays: returns (bad, err) with err = {"k", "rays" (the allowed hits), "t",
        "point" (their relative errors), "tk" (the witness's t), "tan"}."""
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
        err = {"k": k, "rays": hr, "t": np.zeros(0), "point": np.zeros(0), "tk": np.zeros(0), "tan": np.zeros(0)}
        if hr.size:
            kk = k[hr]
            tk, _, _ = self.pair(hr, kk)
            u, v = h["u"][hr].astype(F64)[:, None], h["v"][hr].astype(F64)[:, None]
            P = (1.0 - u - v) * self.T.v[kk, 0] + u * self.T.v[kk, 1] + v * self.T.v[kk, 2]
            err.update(t=np.abs(h["t"][hr].astype(F64) - tk) / tk, tk=tk, tan=self.tan_incidence(hr, kk),
                       point=np.linalg.norm(P - (self.o[hr] + tk[:, None] * self.d[hr]), axis=1) / tk)
        return bad, err


def check_conditions(w, what):
    """What keeps a hit test from hiding failures, from the witness alone: it decides >= 99 % of the rays, and the decided hits whose
    incidence has tan <= 8 are >= 95 % of the decided hits.  Returns both shares."""
    rays = np.flatnonzero(w.decided_hit)
    share = float((w.tan_incidence(rays, w.k[rays]) <= TAN_MAX).mean()) if rays.size else 1.0
    print("%s: decided %.4f  decided hits %d, of them tan <= %g: %.4f" % (what, w.decided_share, rays.size, TAN_MAX, share))
    assert w.decided_share >= gw.DECIDED_SHARE, (what, w.decided_share)
    assert rays.size and share >= BOUNDED_SHARE, (what, rays.size, share)
    return w.decided_share, share


def check_hits(w, hits, what, D, E_o):
    """The assertions every side's first hits are held to under a projection; returns the answered triangle per ray.  Prints the worst
    values before it asserts."""
    bad, err = w.check_hits(hits)
    sel = err["tan"] <= TAN_MAX
    delta = np.sqrt(3.0) * D + E_o / err["tk"][sel]
    et, ep = err["t"][sel], err["point"][sel]
    rt = et - (gw.BOUNDS["t"] + TAN_MAX * delta)
    rp = ep - (gw.BOUNDS["point"] + delta)
    jt, jp = (int(rt.argmax()), int(rp.argmax())) if sel.any() else (-1, -1)
    if sel.any():   # the hit closest to (or furthest beyond) its own bound, and the largest error anywhere
        print("%s: t %.3e of %.3e (largest %.3e)  point %.3e of %.3e (largest %.3e)  over %d of %d hits" % (
            what, et[jt], gw.BOUNDS["t"] + TAN_MAX * delta[jt], et.max(), ep[jp], gw.BOUNDS["point"] + delta[jp], ep.max(), int(sel.sum()), sel.size))
    assert bad.size == 0, "%s: %d answers outside the allowed set; %s" % (what, bad.size, w.describe(int(bad[0]), hits))
    if sel.any():
        assert rt[jt] <= 0, (what, "t", float(et[jt]), w.describe(int(err["rays"][sel][jt]), hits))
        assert rp[jp] <= 0, (what, "point", float(ep[jp]), w.describe(int(err["rays"][sel][jp]), hits))
    return err["k"]


def check_aovs(w, rays, k, albedo, normal, depth, what, E_o):
    """geometry_witness.check_aovs for projected rays, on ALL the decided hits `rays`, grazing ones included: its quantities, and its bounds
    for the normal, the albedo and the depth.  Where the rays share the camera's position exactly (E_o = 0: EQUIRECT, FISHEYE) it IS
    geometry_witness.check_aovs.  Under ORTHOGRAPHIC the depth bound is widened by the origin term alone: an origin off by e moves t by up
    to |e| / cos(incidence), |e|_2 <= sqrt(3) E_o, so depth <= BOUNDS["t"] + sqrt(3) E_o sqrt(1 + tan^2) / t.  (It matters where a ray
    starts next to a surface: t = 2.6e-3 in the truth scene makes E_o / t = 2e-3, and the depth there came out 2.0e-4 off.)"""
    if E_o == 0.0:
        return gw.check_aovs(w, rays, k, albedo, normal, depth, what)
    ref = w.aov(rays, k)
    en = np.abs(normal[:, :3].astype(np.float64) - ref["normal"]).max(axis=1)
    ea = np.abs(albedo[:, :3].astype(np.float64) - ref["albedo"]).max(axis=1)
    ed = np.abs(depth.astype(np.float64) - ref["depth"]) / ref["depth"]
    tan = w.tan_incidence(rays, k)
    bd = gw.BOUNDS["t"] + np.sqrt(3.0) * E_o * np.sqrt(1.0 + tan * tan) / ref["depth"]
    j = int((ed - bd).argmax())
    print("%s: normal %.3e  albedo %.3e  depth %.3e (nearest its bound: %.3e of %.3e)  over %d hits" % (
        what, en.max(), ea.max(), ed.max(), ed[j], bd[j], rays.size))
    for name, e, bound in (("normal", en, gw.BOUNDS["normal"]), ("albedo", ea, gw.BOUNDS["albedo"]), ("depth", ed - bd, 0.0)):
        j = int(e.argmax())
        assert e[j] <= bound, (what, name, float(e[j]), w.describe(int(rays[j])), ref[name][j])
