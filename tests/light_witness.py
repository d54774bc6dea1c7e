"""A float64 witness for light sampling and the environment MIS weight — TEST INFRASTRUCTURE, plain numpy.

Everything else that checks where next-event estimation takes its light from compares programs by one author (device bits == host build
bits == oracle bits).  This module answers the same questions from the scene description alone: it reads a `scenes.Scene` (meshes, node
matrices, materials, the environment texture), the working-space matrix `idt` and — as DATA — the environment's alias table, and restates
the documented contract (kernel.metal:379-467 sampleLightPower / sampleAreaLight / sampleEnvironmentLight, :517-539 the miss branch,
:587-616 the choice between environment and area lights, renderer_pt.cpp:838-938 the light table) in float64.  It imports nothing from
oracle/, tests/emu/ or platinum_amd/csrc/.

What it computes
  lights    every triangle whose material is emissive, in (node, triangle) order: world-space corners M q + t, area = |e1 x e2| / 2 in WORLD
            space, emission = idt @ emission * strength, power = pi * area * emission.g, the running sum of the powers and its total
  choice    pInfinite = 1 without area lights, else envCount / (envCount + 1); a draw rz < pInfinite samples the environment, any other
            the area lights with rz' = (rz - pInfinite) / (1 - pInfinite)
  area      the light = the number of entries among the first n - 1 of the running sum that lie strictly below rz' * total (the strict `<`
            search over n - 1 entries); the point (1 - b0 - b1) v0 + b0 v1 + b1 v2 with (b0, b1) = sampleTriUniform(rl) (math_lib's own
            witness); lwi, dist, lpdf = dist^2 / (|n . lwi| area), pLight = (1 - pInfinite) power / total, Li = emission
  environment  texel i = min(n - 1, floor(rl.x n)), replaced by aliasIdx[i] when rl.y >= p[i]; (x, y) = (i % w, i / w); uv = (x / w, y / h);
            Li = the bilinear-repeat sample at uv (the average of the four texels that meet at the texel's upper left corner);
            wi = (-cos(2 pi u) sin(pi v), cos(pi v), -sin(2 pi u) sin(pi v)); pdf = pdf[i] / 4 pi; pLight = pInfinite; dist = |100 wi - P|
  miss      uv = (atan2(-d.z, -d.x) / 2 pi, acos(d.y) / pi); Le = the bilinear-repeat sample at uv; at bounce 0, after a specular sample or in
            the simple integrator L = Le; else texel (x, y) = (floor(max(w u, 0)), floor(max(h v, 0))) clamped into the map and
            L = Le lastPdf / (lastPdf + pdf[y w + x] / 4 pi)

Reference quirks, FOLLOWED here and not "fixed" (each is what kernel.metal does):
  * the environment density has no sin(theta): pdf / 4 pi is a density over uv, not over solid angle
  * the miss branch does not multiply the light density by pInfinite, and reads the alias table at a texel found from a NEGATIVE u on half
    of the sphere (clamped to column 0) while the radiance is sampled with repeat
  * the light's normal is the object-space cross product through the FORWARD matrix, normalised — not the inverse transpose
  * power uses the green channel of the working-space emission alone
  * Li of an area light is the material's emission constant: an emission texture is ignored by next-event estimation

Set-valued answers.  fp32 cannot decide a draw that lies within rounding of a boundary, so the witness names the SET of admissible answers:
  * area choice: the table's entries carry the fp32 rounding of the areas and of the running sum; with SELECT_SLACK = 2^-18 of the total
    (areas of triangles with coordinates of magnitude <= 8 and edges >= 0.2 round to about 1e-6 relative, the sum adds n 2^-24), every
    index between the answers for rz' total - slack and + slack is admissible, zero-power lights excepted
  * environment texel: rl.x n within 2^-22 relative of an integer admits both texels; rl.y >= p is exact (two floats)
  * miss texel: w u or h v within UV_SLACK (2e-6, the absolute error of the fp32 atan2 / acos: test_math_host.py) of an integer admits both
    texels; on the +x half-plane's seam (|phi| within slack of pi) both signs of phi; at the poles (d.x = d.z = 0) phi = 0, pi and -pi
The result must match one admissible answer.  Outside the "edges" class at most SET_VALUED_CAP = 1 % of a class may be set-valued.

BOUNDS.  Each bound is 4 x the worst error of the ORACLE (oracle/pt_oracle.cpp orc_light_sample / orc_env_miss) against this witness over
light_cases.measure_list(), measured on the host; test_light_witness_host.py measures them again and holds MEASURED to the result.  The factor
4 is the project's margin for inputs not in the list (geometry_witness.py).  The host build of the product and the device are held to
the same table; no figure in it comes from the device.

  quantity                                                              measured worst (oracle)  where                      asserted (4 x)
  --------------------------------------------------------------------  -----------------------  -------------------------  --------------
  lwi       max |lwi - lwi*| over the components                         %(lwi)s
  dist      |dist - dist*| / dist*  (area and environment samples)       %(dist)s
  lpdf      |lpdf - lpdf*| / lpdf*  where |n . lwi*| >= 0.05             %(lpdf)s
  lpdf_cos  | area* / (dist*^2 lpdf) - |n . lwi*| |  (every sample)      %(lpdf_cos)s
  pLight    |pLight - pLight*| / pLight*  (area; environment: exact)     %(pLight)s
  Li        max |Li - Li*| / max |Li*|  (area)                           %(Li)s
  env_wi    max |wi - wi*| over the components                           %(env_wi)s
  env_pdf   |pdf - pdf*| / pdf*                                          %(env_pdf)s
  env_Li    max |Li - Li*| / max(max |Li*|, 1)                           %(env_Li)s
  miss      max |L - L*| / max(max |L*|, 1e-6)                           %(miss)s
"""
import numpy as np

import math_lib

F64 = np.float64
PI = np.pi
SELECT_SLACK = 2.0 ** -18     # of the total power
TEXEL_SLACK = 2.0 ** -22      # relative, of rl.x * n
UV_SLACK = 2e-6               # absolute, of a uv coordinate computed from a direction in fp32
IDENT_TOL = 1e-3              # an answer is attributed to the admissible candidate it matches to this relative distance
SET_VALUED_CAP = 0.01
LUMA = np.array([0.2126, 0.7152, 0.0722])   # core/environment.cpp:5-91

# measured worst of the oracle against the witness: (value, where); the asserted bounds = 4 x
MEASURED = {
    "lwi": (5.03e-07, "n5 lattice"),
    "dist": (7.97e-07, "n5 lattice"),
    "lpdf": (5.01e-06, "n64 lattice"),
    "lpdf_cos": (1.52e-06, "n65 lattice"),
    "pLight": (1.57e-06, "n200 rz_grid"),
    "Li": (1.32e-07, "n65 rz_grid"),
    "env_wi": (3.26e-07, "env_sky env_grid"),
    "env_pdf": (8.33e-08, "env_sky env_grid"),
    "env_Li": (6.54e-08, "env_3x5 lattice"),
    "miss": (2.37e-05, "env_sky miss"),
}
BOUNDS = {k: 4.0 * v[0] for k, v in MEASURED.items()}
for _k, _v in MEASURED.items():   # the table above, filled from the one below
    __doc__ = __doc__.replace("%%(%s)s" % _k, "%-24.3g %-26s %.3g" % (_v[0], _v[1], 4.0 * _v[0]))


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def bilinear_repeat(px, u, v):
    """sampler(address::repeat, filter::linear) on the (h, w, c) float64 texels `px` at the float64 arrays (u, v): texel centres at
    (i + 1/2) / size."""
    h, w = px.shape[:2]
    x, y = u * w - 0.5, v * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    wx, wy = (x - x0)[:, None], (y - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    t = lambda xx, yy: px[yy % h, xx % w]
    a = t(x0, y0) * (1 - wx) + t(x0 + 1, y0) * wx
    b = t(x0, y0 + 1) * (1 - wx) + t(x0 + 1, y0 + 1) * wx
    return a * (1 - wy) + b * wy


class Lights:
    """The area lights of a scene in table order, float64 from the scene's float32 data."""

    def __init__(self, scene, idt):
        v, em, nrm = [], [], []
        for node in scene.nodes:
            if not any(m.is_emissive() for m in node.materials):
                continue
            mesh = scene.meshes[node.mesh]
            idx = np.asarray(mesh.indices, np.int64).reshape(-1, 3)
            P = np.asarray(mesh.positions, np.float32)[:, :3].astype(F64)
            Wm = np.asarray(node.world, np.float32).astype(F64)           # [col][row]
            M3 = np.stack([Wm[0, :3], Wm[1, :3], Wm[2, :3]], axis=1)     # M3[r][c] = column c, row r
            slots = np.asarray(mesh.material_slots, np.int64)
            for t, tri in enumerate(idx):
                mat = node.materials[slots[t]]
                if not mat.is_emissive():
                    continue
                q = P[tri]
                v.append(q @ M3.T + Wm[3, :3])
                e = np.asarray(mat.emission, np.float32).astype(F64)
                em.append((idt @ e) * F64(np.float32(mat.emission_strength)))
                nrm.append(_unit(M3 @ np.cross(q[1] - q[0], q[2] - q[0])))    # the FORWARD matrix (kernel.metal:420-423), on purpose
        self.n = len(v)
        self.v = np.array(v, F64).reshape(self.n, 3, 3)
        self.emission = np.array(em, F64).reshape(self.n, 3)
        self.normal = np.array(nrm, F64).reshape(self.n, 3)
        self.area = 0.5 * np.linalg.norm(np.cross(self.v[:, 1] - self.v[:, 0], self.v[:, 2] - self.v[:, 0]), axis=1)
        self.power = PI * self.area * self.emission[:, 1]                # green alone (renderer_pt.cpp:899)
        self.cum = np.cumsum(self.power)
        self.total = float(self.cum[-1]) if self.n else 0.0

    def identify(self, Li, chunk=4096):
        """(index, distance) of the light whose emission is nearest to each row of Li: max |Li - e| / max |e|"""
        idx, dist = np.zeros(len(Li), np.int64), np.zeros(len(Li))
        scale = np.abs(self.emission).max(1)
        for a in range(0, len(Li), chunk):
            with np.errstate(invalid="ignore"):
                d = np.abs(Li[a:a + chunk, None, :] - self.emission[None]).max(2) / scale[None]
            d = np.where(np.isnan(d), np.inf, d)
            idx[a:a + chunk] = d.argmin(1)
            dist[a:a + chunk] = d.min(1)
        return idx, dist

    def admissible(self, x):
        """(lo, hi): the lowest and highest index a correct fp32 search may return for the scaled draws x = rz' * total"""
        s = SELECT_SLACK * self.total
        head = self.cum[:-1]
        return np.searchsorted(head, x - s, "left"), np.searchsorted(head, x + s, "left")


class Env:
    """The environment map and its alias table (data: p, aliasIdx, pdf as the renderer holds them)."""

    def __init__(self, scene, alias):
        tex = scene.textures[scene.env_texture]
        assert tex.pixels.dtype == np.float32 and tex.pixels.shape[2] == 4, "RGBA32F environments only"
        self.px = tex.pixels.astype(F64)
        self.h, self.w = self.px.shape[:2]
        self.n = self.w * self.h
        assert len(alias) == self.n
        self.p32 = np.asarray(alias["p"], np.float32)
        self.p, self.pdf, self.alias = self.p32.astype(F64), np.asarray(alias["pdf"], np.float32).astype(F64), np.asarray(alias["aliasIdx"], np.int64)
        assert np.all((self.alias >= 0) & (self.alias < self.n))

    def luma_distribution(self):
        luma = (self.px[..., :3] @ LUMA).reshape(-1)
        return luma / luma.sum()

    def implied_distribution(self):
        """The probability of each texel under the alias table: (p_i + sum over j with alias_j = i of (1 - p_j)) / n"""
        q = self.p.copy()
        np.add.at(q, self.alias, 1.0 - self.p)
        return q / self.n

    def alias_errors(self):
        """(max |pdf_i / n - luma_i / sum|, max |implied_i - luma_i / sum|), both times n: in units of the mean probability"""
        want = self.luma_distribution()
        return float(np.abs(self.pdf / self.n - want).max() * self.n), float(np.abs(self.implied_distribution() - want).max() * self.n)

    def alias_bound(self):
        """What fp32 leaves of the table (Vose's method in float): the sum of n lumas rounds to n 2^-24 relative, and an entry that takes part
        in k pairings carries k roundings of 2^-24 times the largest importance; k <= n."""
        return (self.n + 8) * 2.0 ** -24 * max(1.0, float(self.pdf.max()))

    def texel(self, i):
        """Li, wi, pdf of a sample that ends on texel i (arrays)"""
        x, y = i % self.w, i // self.w
        u, v = x / self.w, y / self.h
        Li = bilinear_repeat(self.px, u.astype(F64), v.astype(F64))[:, :3]
        st, ct = np.sin(v * PI), np.cos(v * PI)
        wi = np.stack([-np.cos(u * 2 * PI) * st, ct, -np.sin(u * 2 * PI) * st], axis=1)
        return Li, _unit(wi), self.pdf[i] / (4 * PI)

    def counts(self, K):
        """The number of points of the (n K) x K grid (rl.x = (c + 1/2) / (n K), rl.y = (j + 1/2) / K, as float32) that end on each texel."""
        ry = ((np.arange(K, dtype=F64) + 0.5) / K).astype(np.float32)
        stay = (ry[None, :] < self.p32[:, None]).sum(1)        # rows of texel i that keep it
        c = (K * stay).astype(np.int64)
        np.add.at(c, self.alias, K * (K - stay))
        return c


def classes(a):
    """0 finite, 1 infinite, 2 NaN"""
    a = np.asarray(a, F64)
    return np.where(np.isnan(a), 2, np.where(np.isinf(a), 1, 0))


class Report:
    def __init__(self, n):
        self.bad = np.zeros(n, bool)            # the answer is not admissible
        self.set_valued = np.zeros(n, bool)
        self.chosen = np.full(n, -1, np.int64)  # area light k -> k; environment texel i -> -2 - i; nothing sampled -> -1
        self.err = {}                           # quantity -> (worst, element)
        self.why = ""

    def worst(self, q, e, where):
        e = np.where(np.isnan(e), np.inf, np.asarray(e, F64))     # (an error that is not a number is the worst there is)
        if e.size:
            j = int(e.argmax())
            if q not in self.err or e[j] > self.err[q][0]:
                self.err[q] = (float(e[j]), int(where[j]))

    def flag(self, idx, why):
        if len(idx):
            self.bad[idx] = True
            if not self.why:
                self.why = "%s (element %d)" % (why, int(idx[0]))

    @property
    def set_valued_share(self):
        return float(self.set_valued.mean())


class Witness:
    def __init__(self, scene, idt, alias=None, mis=True):
        self.L = Lights(scene, np.asarray(idt, F64))
        self.E = Env(scene, alias) if scene.env_texture >= 0 else None
        self.mis = mis
        self.env_count = 1 if self.E is not None else 0
        self.p_inf = 1.0 if self.L.n == 0 else self.env_count / (self.env_count + 1.0)

    # ---- PT_LIGHT_SAMPLE ----------------------------------------------------------------------------------------------------------
    def check_sample(self, rec, out, roughness=1.0, metallic=0.0, transmission=0.0, dim=0, edge=False):
        rec = np.asarray(rec, np.float32)
        n = len(rec)
        rep = Report(n)
        f32 = np.float32
        nee = self.mis and (f32(roughness) > 0 or f32(f32(metallic) + f32(transmission)) < 1)
        lit = nee and (self.L.n > 0 or self.env_count > 0)
        rep.flag(np.flatnonzero(out["dim"] != dim + (9 if nee else 6)), "dim")
        rep.flag(np.flatnonzero(out["lit"] != (1 if lit else 0)), "lit")
        if not lit:
            zero = (out["Li"] == 0).all(1) & (out["lwi"] == 0).all(1) & (out["lpdf"] == 0) & (out["pLight"] == 0) & (out["dist"] == 0)
            rep.flag(np.flatnonzero(~zero), "an unlit record holds values")
            return rep
        P, rl, rz = rec[:, :3].astype(F64), rec[:, 3:5], rec[:, 5].astype(F64)
        env = rz < self.p_inf
        ia, ie = np.flatnonzero(~env), np.flatnonzero(env)
        if ia.size:
            self._check_area(rep, ia, P[ia], rl[ia], rz[ia], out[ia], edge)
        if ie.size:
            self._check_env(rep, ie, P[ie], rl[ie], out[ie], edge)
        return rep

    def _check_area(self, rep, ids, P, rl, rz, out, edge):
        L = self.L
        x = (rz - self.p_inf) / (1.0 - self.p_inf) * L.total
        lo, hi = L.admissible(x)
        rep.set_valued[ids] = lo != hi
        # which light the side took: the one whose emission its Li is, among ALL lights (light_cases gives every light with power its own
        # colour) — then whether that light is admissible for the draw
        ident, best = L.identify(out["Li"].astype(F64))
        ok = (ident >= lo) & (ident <= hi) & ((L.power[ident] > 0) | (lo == hi)) & (best <= IDENT_TOL)
        rep.chosen[ids] = ident
        rep.flag(ids[~ok], "the emission is that of no admissible light")
        k = np.where(ok, ident, lo)
        b0, b1 = math_lib.ref_tri_uniform(rl[:, 0], rl[:, 1])
        pos = (1 - b0 - b1)[:, None] * L.v[k, 0] + b0[:, None] * L.v[k, 1] + b1[:, None] * L.v[k, 2]
        d = pos - P
        with np.errstate(divide="ignore", invalid="ignore"):
            dist = np.linalg.norm(d, axis=1)
            lwi = d / dist[:, None]
            cos = np.abs((L.normal[k] * lwi).sum(1))
            lpdf = dist * dist / (cos * L.area[k])
            pl = (1.0 - self.p_inf) * L.power[k] / L.total
            want = {"lwi": lwi, "dist": dist, "lpdf": lpdf, "pLight": pl, "Li": L.emission[k]}
            if edge:
                self._classes(rep, ids, out, want)
                return
            g = lambda f: out[f].astype(F64)
            rep.worst("lwi", np.abs(g("lwi") - lwi).max(1), ids)
            rep.worst("dist", np.abs(g("dist") - dist) / dist, ids)
            steep = cos >= 0.05
            rep.worst("lpdf", (np.abs(g("lpdf") - lpdf) / lpdf)[steep], ids[steep])
            rep.worst("lpdf_cos", np.abs(dist * dist / (g("lpdf") * L.area[k]) - cos), ids)
            rep.worst("pLight", np.abs(g("pLight") - pl) / pl, ids)
            rep.worst("Li", best, ids)

    def _env_candidates(self, rl):
        """(candidates (m, 2) of texel indices, set_valued): the first texel, or both neighbours when rl.x n lies on a boundary, each through
        the alias step"""
        E = self.E
        t = rl[:, 0].astype(F64) * E.n
        s = t * TEXEL_SLACK
        first = np.stack([np.floor(t - s), np.floor(t + s)], axis=1).clip(0, E.n - 1).astype(np.int64)
        flip = rl[:, 1].astype(np.float32)[:, None] >= E.p32[first]          # exact: two floats
        return np.where(flip, E.alias[first], first), first[:, 0] != first[:, 1]

    def _check_env(self, rep, ids, P, rl, out, edge):
        E = self.E
        cand, sv = self._env_candidates(rl)
        rep.set_valued[ids] = sv
        g = lambda f: out[f].astype(F64)
        best, pick = np.full(len(ids), np.inf), cand[:, 0].copy()
        for c in (cand[:, 0], cand[:, 1]):
            Li, wi, pdf = E.texel(c)
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.maximum(np.abs(g("lwi") - wi).max(1), np.abs(g("Li") - Li).max(1) / np.maximum(np.abs(Li).max(1), 1.0))
                d = np.maximum(d, np.where(pdf > 0, np.abs(g("lpdf") - pdf) / pdf, np.abs(g("lpdf"))))
            take = d < best
            best, pick = np.where(take, d, best), np.where(take, c, pick)
        rep.chosen[ids] = -2 - pick
        rep.flag(ids[~(best <= IDENT_TOL)], "the sample is that of no admissible texel")
        Li, wi, pdf = E.texel(pick)
        dist = np.linalg.norm(100.0 * wi - P, axis=1)
        if edge:
            self._classes(rep, ids, out, {"lwi": wi, "dist": dist, "lpdf": pdf, "pLight": np.full(len(ids), self.p_inf), "Li": Li})
            return
        rep.flag(ids[out["pLight"] != np.float32(self.p_inf)], "pLight of an environment sample is pInfinite / envCount")
        rep.worst("env_wi", np.abs(g("lwi") - wi).max(1), ids)
        pos = pdf > 0
        rep.worst("env_pdf", (np.abs(g("lpdf") - pdf)[pos] / pdf[pos]), ids[pos])
        rep.flag(ids[~pos][g("lpdf")[~pos] != 0], "a black texel's density is 0")
        rep.worst("env_Li", np.abs(g("Li") - Li).max(1) / np.maximum(np.abs(Li).max(1), 1.0), ids)
        rep.worst("dist", np.abs(g("dist") - dist) / dist, ids)

    def _classes(self, rep, ids, out, want):
        """the edges class: every field is finite, infinite or NaN as float64 predicts"""
        for f, w in want.items():
            got, w = classes(out[f]).reshape(len(ids), -1), classes(w).reshape(len(ids), -1)
            rep.flag(ids[(got != w).any(1)], "%s: finite / inf / NaN differs from float64's" % f)

    # ---- PT_LIGHT_ENV_MISS --------------------------------------------------------------------------------------------------------
    def check_miss(self, rec, out, bounce=1, lastSpecular=False, edge=False):
        E = self.E
        rec = np.asarray(rec, np.float32)
        n = len(rec)
        rep = Report(n)
        d, last = rec[:, :3].astype(F64), rec[:, 3].astype(F64)
        plain = (not self.mis) or bounce == 0 or lastSpecular
        phi = np.arctan2(-d[:, 2], -d[:, 0])
        pole = (d[:, 0] == 0) & (d[:, 2] == 0)
        seam = (PI - np.abs(phi)) <= UV_SLACK * 2 * PI
        phis = [np.where(pole, 0.0, phi), np.where(pole, PI, np.where(seam, -phi, phi)), np.where(pole, -PI, phi)]
        v = np.arccos(np.clip(d[:, 1], -1, 1)) / PI
        got = out["L"].astype(F64)
        best = np.full(n, np.inf)
        want_best = np.zeros((n, 3))
        keys = []
        for bi, ph in enumerate(phis):
            branch = np.where(ph != phis[0], bi, 0)
            u = ph / (2 * PI)
            Le = bilinear_repeat(E.px, u, v)[:, :3]
            fx, fy = E.w * u, E.h * v
            for sx in (-1, 1):
                for sy in (-1, 1):
                    x = np.floor(np.maximum(fx + sx * UV_SLACK * E.w, 0)).clip(0, E.w - 1).astype(np.int64)
                    y = np.floor(np.maximum(fy + sy * UV_SLACK * E.h, 0)).clip(0, E.h - 1).astype(np.int64)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        wgt = np.ones(n) if plain else last / (last + E.pdf[y * E.w + x] / (4 * PI))
                        want = Le * wgt[:, None]
                        e = np.abs(got - want).max(1) / np.maximum(np.abs(want).max(1), 1e-6)
                    if edge:   # an answer of the same class everywhere is compared where it is finite; a NaN or infinity matches its like
                        cg, cw = classes(got), classes(want)
                        same = (cg == cw).all(1)
                        fin = (cw == 0)
                        ef = np.where(fin, np.abs(got - np.where(fin, want, 0)) / np.maximum(np.abs(np.where(fin, want, 0)).max(1), 1e-6)[:, None], 0).max(1)
                        e = np.where(same, ef, np.inf)
                    keys.append((0 if plain else y * E.w + x) * 4 + branch)
                    take = e < best
                    best = np.where(take, e, best)
                    want_best = np.where(take[:, None], want, want_best)
        keys = np.stack(keys, axis=1)
        rep.set_valued = (keys != keys[:, :1]).any(1)
        rep.flag(np.flatnonzero(~(best <= IDENT_TOL)), "the radiance is that of no admissible texel")
        if not edge:
            rep.worst("miss", best, np.arange(n))
        return rep


def assert_report(rep, what, edge=False, quantities=None):
    """The assertions every side is held to (prints the figures first)."""
    print("%s: set-valued %.4f%s  %s" % (what, rep.set_valued_share, " (edges)" if edge else "",
                                        "  ".join("%s %.3e@%d" % (q, e[0], e[1]) for q, e in sorted(rep.err.items()))))
    assert not rep.bad.any(), "%s: %d answers not admissible; first: %s" % (what, int(rep.bad.sum()), rep.why)
    if edge:
        return
    assert rep.set_valued_share <= SET_VALUED_CAP, (what, rep.set_valued_share)
    for q, (e, j) in rep.err.items():
        if quantities is None or q in quantities:
            assert e <= BOUNDS[q], (what, q, e, BOUNDS[q], j)
