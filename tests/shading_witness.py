"""A float64 witness for the shading frame and the material context — TEST INFRASTRUCTURE, plain numpy.

Between a hit record and the BSDF every shaded hit and every AOV passes through one block of code (pt_shade.h shade_geometry, pt_bsdf.h
make_shading_context / tex_sample / tex_fetch; the oracle's getIntersectionData and ShadingContext).  Everything else that checks it compares
programs by one author.  This module answers from the scene description alone: it reads a `scenes.Scene` (meshes, node matrices, materials,
raw texture bytes) and the colour matrix idt, and restates the contract in float64.  It imports nothing from oracle/, tests/emu/ or
platinum_amd/csrc/.

THE CONTRACT, for a hit (instance, primitive, u, v) of a ray (o, d, t):
  weights      (1 - u - v, u, v) on the three vertices' normals, tangent xyz and UVs
  handedness   sgn = tangent[3] of vertex 0 of the triangle
  world n, t   n and t each go through the FORWARD 3x3 of the node and are then normalised.  A recorded quirk of the reference
               (kernel.metal:150-162), followed: under a non-uniform scale this is not the inverse transpose
  fromNT       |n . t| > 0.9: fromNormal(n);  otherwise y = sgn normalize(n x t), x = y x n, z = n
  fromNormal   a = z^ if |n.x| > 0.5 else x^;  y = normalize(n x a), x = n x y, z = n
  normal map   s = 2 c - 1 of the filtered texel c;  N = x s.x + y s.y + z s.z;  the frame becomes fromNormal(N) with N NOT normalised.
               A recorded quirk of the reference (kernel.metal:166-177), followed, not fixed: |z| = |x| = |N| and |y| = 1
  wo           (-d . x, -d . y, -d . z)
  hitPos       o + t d
  texels       sRGB8 colour channels through the piecewise EOTF in float64, alpha and UNORM8 i / 255, R8 -> (r, 0, 0, 1),
               RG8 -> (r, g, 0, 1), RGBA32F verbatim
  filter       bilinear, repeat addressing, taps at uv size - 0.5
  context      base texel rgb replaces the albedo; emission = emission x texel rgb, then idt, then the strength; idt on the albedo;
               transmission and clearcoat are texel .x; roughness x= rm.x, metallic x= rm.y; clearcoatRoughness, anisotropy, ior, the
               flags and every untextured term are verbatim
  class        3 clearcoat or a clearcoat / rm / transmission texture, else 2 transmission, else 1 metallic, else 0

SET-VALUED ANSWERS.  Only the two frame switches are discontinuous.  A hit is set-valued when ||n . t| - 0.9| <= 1e-5, or when
||v.x| - 0.5| <= 1e-6 for a vector v given to fromNormal; there either branch is admissible.  Bilinear filtering is continuous: texture
values are never set-valued.  Outside the "edges" class at most SET_VALUED_CAP = 1 % of a class may be set-valued.

ERRORS.  frame: max over the nine components of |F - F*|, for a normal-mapped hit relative to |N*|.  wo: max over the components, relative
to |d| and for a normal-mapped hit to |N*| (wo is linear in both).  Normal-mapped hits have figures of their own: the filtered texel carries
the fp32 rounding of the UV times the texture's gradient into the frame, which a frame without a map never sees.  hitPos: |P - P*| / |t|.
albedo, emission: max over rgb of |a - a*| / max(|a*|, 1).  roughness, metallic, transmission, clearcoat: absolute.  clearcoatRoughness,
anisotropy, ior, flags and the class are exact, as is every scalar of a material that no texture feeds.  Normal-mapped hits with
|N*| < N_MIN = 0.05 belong to the edges class; |N*| over the cases is 0.034 .. 1.36 (test_the_cases_cover_what_they_claim prints it).

BOUNDS.  Nothing is fixed in advance: each bound is 4 x the worst error of the ORACLE (oracle/pt_oracle.cpp orc_shade_probe) against this
witness over shading_cases.measure_list(), measured on the host; test_shading_witness_host.py measures them again and holds MEASURED to the
result.  The factor 4 is the project's margin for scenes not in the list (geometry_witness.py).  The host build of the product and the
device are held to the same table; no figure in it comes from the device.

  quantity                                                          measured worst (oracle)  where                          asserted (4 x)
  ----------------------------------------------------------------  -----------------------  -----------------------------  --------------
  frame      max |F - F*| over the axes' components, no normal map   %(frame)s
  frame_mapped  the same / |N*|, normal-mapped hits                  %(frame_mapped)s
  wo         max |wo - wo*| / |d|, no normal map                     %(wo)s
  wo_mapped  the same / |N*|, normal-mapped hits                     %(wo_mapped)s
  hitPos     |P - P*| / |t|                                          %(hitPos)s
  albedo     max |a - a*| / max(|a*|, 1)                             %(albedo)s
  emission   max |e - e*| / max(|e*|, 1)                             %(emission)s
  roughness  |r - r*|                                                %(roughness)s
  metallic   |m - m*|                                                %(metallic)s
  transmission                                                      %(transmission)s
  clearcoat                                                         %(clearcoat)s
"""
import numpy as np

F64 = np.float64
NT_SWITCH, NT_SLACK = 0.9, 1e-5
AXIS_SWITCH, AXIS_SLACK = 0.5, 1e-6
N_MIN = 0.05
SET_VALUED_CAP = 0.01
TEX_RGBA8_SRGB, TEX_RGBA8, TEX_RG8, TEX_R8, TEX_RGBA32F = range(5)     # include/ptamd.h PT_TEX_*
SCALARS = ("roughness", "metallic", "transmission", "clearcoat")
VERBATIM = ("clearcoatRoughness", "anisotropy", "ior")

# measured worst of the oracle against the witness: (value, where); the asserted bounds = 4 x
MEASURED = {
    "frame": (2.10e-07, "slots hits"),
    "frame_mapped": (1.83e-05, "normalmaps hits"),
    "wo": (2.47e-07, "frames lattice"),
    "wo_mapped": (1.30e-05, "normalmaps hits"),
    "hitPos": (4.98e-08, "frames hits"),
    "albedo": (7.63e-06, "slots random"),
    "emission": (3.26e-05, "normalmaps hits"),
    "roughness": (6.81e-06, "normalmaps hits"),
    "metallic": (4.99e-06, "normalmaps hits"),
    "transmission": (5.28e-06, "slots hits"),
    "clearcoat": (1.18e-05, "normalmaps outside"),
}
BOUNDS = {k: 4.0 * v[0] for k, v in MEASURED.items()}
for _k, _v in MEASURED.items():   # the table above, filled from the one below
    __doc__ = __doc__.replace("%%(%s)s" % _k, "%-24.3g %-30s %.3g" % (_v[0], _v[1], 4.0 * _v[0]))


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _unit(v):
    with np.errstate(divide="ignore", invalid="ignore"):
        return v / np.sqrt((v * v).sum(-1, keepdims=True))


def srgb_eotf(c):
    c = np.asarray(c, F64)
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def decode(pixels, fmt):
    """(H, W, 4) float64 linear texels of a texture as the scene holds it"""
    px = np.asarray(pixels)
    h, w = px.shape[:2]
    out = np.zeros((h, w, 4), F64)
    out[..., 3] = 1.0
    if fmt == TEX_RGBA32F:
        return px.astype(F64)
    q = px.astype(F64) / 255.0
    if fmt == TEX_RGBA8_SRGB:
        out[..., :3], out[..., 3] = srgb_eotf(q[..., :3]), q[..., 3]
    elif fmt == TEX_RGBA8:
        out[:] = q
    elif fmt == TEX_RG8:
        out[..., :2] = q
    else:
        out[..., 0] = q[..., 0]
    return out


def bilinear_repeat(tex, u, v):
    """tex (H, W, 4) float64, u and v (n,) float64 -> (n, 4): taps at uv size - 0.5, repeat addressing.  Integers are formed from float64
    floors through Python-width arithmetic (np.mod on floats), so no coordinate overflows."""
    h, w, _ = tex.shape
    x, y = u * w - 0.5, v * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    wx, wy = (x - x0)[:, None], (y - y0)[:, None]
    ix0, ix1 = np.mod(x0, w).astype(np.int64), np.mod(x0 + 1.0, w).astype(np.int64)
    iy0, iy1 = np.mod(y0, h).astype(np.int64), np.mod(y0 + 1.0, h).astype(np.int64)
    a = tex[iy0, ix0] * (1 - wx) + tex[iy0, ix1] * wx
    b = tex[iy1, ix0] * (1 - wx) + tex[iy1, ix1] * wx
    return a * (1 - wy) + b * wy


def material_class(m):
    if np.float32(m.clearcoat) > 0 or m.clearcoat_texture >= 0 or m.rm_texture >= 0 or m.transmission_texture >= 0:
        return 3
    if np.float32(m.transmission) > 0:
        return 2
    return 1 if np.float32(m.metallic) > 0 else 0


def _from_normal(n, axis_z):
    """fromNormal with the helper axis forced: z^ where axis_z, x^ elsewhere"""
    a = np.where(axis_z[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    y = _unit(_cross(n, a))
    return np.stack([_cross(n, y), y, n], axis=1)      # (n, 3 axes, 3)


def _from_normal_candidates(v, valid):
    """the admissible fromNormal(v) frames: [(frame, valid)] for a = z^ and a = x^"""
    with np.errstate(invalid="ignore"):
        ax = np.abs(v[:, 0])
        return [(_from_normal(v, np.ones(len(v), bool)), valid & (ax > AXIS_SWITCH - AXIS_SLACK)),
                (_from_normal(v, np.zeros(len(v), bool)), valid & ~(ax > AXIS_SWITCH + AXIS_SLACK))]


class Answer:
    """What the witness says about a batch of records: the admissible frames with their validity, and everything that has one value."""
    pass


class Witness:
    def __init__(self, scene, idt):
        """idt: the colour matrix as [row][col] float64 (from a side's constants: an input of the stage, not a result of it)"""
        self.scene, self.idt = scene, np.asarray(idt, F64)
        self.tex = [decode(t.pixels, t.format) for t in scene.textures]

    def _gather(self, inst, prim):
        """per record: the three vertices' (normal, tangent, uv), the forward 3x3 and the material"""
        n = len(inst)
        vn, vt, vuv, m3 = np.zeros((n, 3, 3)), np.zeros((n, 3, 4)), np.zeros((n, 3, 2)), np.zeros((n, 3, 3))
        mats = np.empty(n, object)
        for i in np.unique(inst):
            node = self.scene.nodes[i]
            mesh = self.scene.meshes[node.mesh]
            sel = np.flatnonzero(inst == i)
            idx = np.asarray(mesh.indices, np.int64).reshape(-1, 3)[prim[sel]]
            vd = np.asarray(mesh.vertex_data, np.float32).astype(F64)
            vn[sel], vt[sel], vuv[sel] = vd[:, 0:3][idx], vd[:, 4:8][idx], vd[:, 8:10][idx]
            Wm = np.asarray(node.world, np.float32).astype(F64)              # [col][row]
            m3[sel] = np.stack([Wm[0, :3], Wm[1, :3], Wm[2, :3]], axis=1)     # M3[r][c] = column c, row r
            slots = np.asarray(mesh.material_slots, np.int64)[prim[sel]]
            for j, s in zip(sel, slots):
                mats[j] = node.materials[s]
        return vn, vt, vuv, m3, mats

    def answer(self, rec):
        rec = np.asarray(rec).reshape(-1)
        n = len(rec)
        inst, prim = rec["instance"].astype(np.int64), rec["primitive"].astype(np.int64)
        u, v = rec["u"].astype(F64), rec["v"].astype(F64)
        o, d, t = rec["o"].astype(F64), rec["d"].astype(F64), rec["t"].astype(F64)
        vn, vt, vuv, m3, mats = self._gather(inst, prim)
        w3 = np.stack([1.0 - u - v, u, v], axis=1)[:, :, None]
        n_os, t_os, uv = (w3 * vn).sum(1), (w3 * vt[:, :, :3]).sum(1), (w3 * vuv).sum(1)
        sgn = vt[:, 0, 3]
        nw = _unit(np.einsum("nrc,nc->nr", m3, n_os))
        tw = _unit(np.einsum("nrc,nc->nr", m3, t_os))
        A = Answer()
        A.nw, A.tw, A.sgn, A.uv, A.mats, A.d = nw, tw, sgn, uv, mats, d
        with np.errstate(invalid="ignore"):
            dot = np.abs((nw * tw).sum(-1))
            y = sgn[:, None] * _unit(_cross(nw, tw))
            nt = np.stack([_cross(y, nw), y, nw], axis=1)
            use_nt = ~(dot > NT_SWITCH + NT_SLACK)            # (a NaN product takes the fromNT branch, as `>` does)
            use_fn = dot > NT_SWITCH - NT_SLACK
        base = [(nt, use_nt)] + _from_normal_candidates(nw, use_fn)
        # the normal map
        A.mapped = np.array([m.normal_texture >= 0 for m in mats], bool)
        A.texel_n = np.zeros((n, 4))
        for tid in {m.normal_texture for m in mats if m.normal_texture >= 0}:
            sel = np.flatnonzero([m.normal_texture == tid for m in mats])
            A.texel_n[sel] = bilinear_repeat(self.tex[tid], uv[sel, 0], uv[sel, 1])
        s = 2.0 * A.texel_n[:, :3] - 1.0
        cands = []
        for F, ok in base:
            cands.append((F, ok & ~A.mapped, np.ones(n)))
            N = F[:, 0] * s[:, 0:1] + F[:, 1] * s[:, 1:2] + F[:, 2] * s[:, 2:3]
            for F2, ok2 in _from_normal_candidates(N, ok & A.mapped):
                cands.append((F2, ok2, np.sqrt((N * N).sum(-1))))
        A.frames = np.stack([c[0] for c in cands])                    # (k, n, 3, 3)
        A.valid = np.stack([c[1] for c in cands])                     # (k, n)
        A.scale = np.stack([c[2] for c in cands])                     # (k, n): |N| of a mapped candidate, 1 otherwise
        A.set_valued = A.valid.sum(0) > 1
        assert np.all(A.valid.sum(0) >= 1)
        first = A.valid.argmax(0)
        A.frame = A.frames[first, np.arange(n)]                       # one admissible frame (the only one where not set-valued)
        A.N_len = A.scale[first, np.arange(n)]
        A.wo = -np.einsum("knac,nc->kna", A.frames, d)                # (k, n, 3)
        A.hitPos = o + t[:, None] * d
        A.t = t
        # the context
        f32 = lambda x: np.asarray(x, np.float32).astype(F64)
        alb = np.array([f32(m.base_color[:3]) for m in mats]).reshape(n, 3)
        emi = np.array([f32(m.emission) for m in mats]).reshape(n, 3)
        sc = {q: np.array([f32(getattr(m, a)) for m in mats]) for q, a in (
            ("roughness", "roughness"), ("metallic", "metallic"), ("transmission", "transmission"), ("clearcoat", "clearcoat"),
            ("clearcoatRoughness", "clearcoat_roughness"), ("anisotropy", "anisotropy"), ("ior", "ior"))}
        A.fed = {q: np.zeros(n, bool) for q in ("albedo", "emission") + SCALARS}     # which terms a texture feeds
        for slot in ("base_texture", "emission_texture", "transmission_texture", "clearcoat_texture", "rm_texture"):
            ids = np.array([getattr(m, slot) for m in mats])
            for tid in np.unique(ids[ids >= 0]):
                sel = np.flatnonzero(ids == tid)
                tx = bilinear_repeat(self.tex[tid], uv[sel, 0], uv[sel, 1])
                if slot == "base_texture":
                    alb[sel] = tx[:, :3]; A.fed["albedo"][sel] = True
                elif slot == "emission_texture":
                    emi[sel] = emi[sel] * tx[:, :3]; A.fed["emission"][sel] = True
                elif slot == "transmission_texture":
                    sc["transmission"][sel] = tx[:, 0]; A.fed["transmission"][sel] = True
                elif slot == "clearcoat_texture":
                    sc["clearcoat"][sel] = tx[:, 0]; A.fed["clearcoat"][sel] = True
                else:
                    sc["roughness"][sel] = sc["roughness"][sel] * tx[:, 0]; A.fed["roughness"][sel] = True
                    sc["metallic"][sel] = sc["metallic"][sel] * tx[:, 1]; A.fed["metallic"][sel] = True
        A.albedo = alb @ self.idt.T
        A.emission = (emi @ self.idt.T) * np.array([f32(m.emission_strength) for m in mats])[:, None]
        A.scalars = sc
        A.flags = np.array([m.to_gpu().flags for m in mats], np.int64)        # the flags cross the ABI as an input; the stage copies them
        A.cls = np.array([material_class(m) for m in mats], np.int64)
        return A


class Report:
    """err: {quantity: (worst, record index)} over the records that are not `edge`; bad: records whose answer is not admissible"""
    pass


def _kind(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    x = np.asarray(x, F64)
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0)))


def check(A, out, edge=False):
    """A side's records `out` (abi.SHADE_PROBE_OUT_DTYPE) against the answer A.  edge=True: no accuracy figure; the frame must have the
    finite / inf / NaN class of an admissible candidate, component for component."""
    out = np.asarray(out).reshape(-1)
    n = len(out)
    R = Report()
    F = np.stack([out["x"], out["y"], out["z"]], axis=1).astype(F64)            # (n, 3, 3)
    wo = out["wo"].astype(F64)
    dlen = np.sqrt((A.d * A.d).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        ef = np.abs(F[None] - A.frames).reshape(len(A.frames), n, 9).max(-1) / A.scale          # (k, n)
        ew = np.abs(wo[None] - A.wo).max(-1) / (A.scale * dlen)
        both = np.where(A.valid, np.maximum(ef, ew), np.inf)
        both = np.where(np.isnan(both), np.inf, both)
        pick = both.argmin(0)
        ar = np.arange(n)
        ef, ew = ef[pick, ar], ew[pick, ar]
        same_kind = ((_kind(F)[None] == _kind(A.frames)).reshape(len(A.frames), n, 9).all(-1) &
                     (_kind(wo)[None] == _kind(A.wo)).all(-1) & A.valid).any(0)
        # float64 predicts the class of fromNormal(N) where N is exactly 0 or clearly not; in between fp32 may round N to 0 or away from it
        same_kind |= A.mapped & (A.N_len > 0) & (A.N_len < 1e-6)
        ep = np.sqrt(((out["hitPos"].astype(F64) - A.hitPos) ** 2).sum(-1)) / np.abs(A.t)
        ea = (np.abs(out["albedo"].astype(F64) - A.albedo) / np.maximum(np.abs(A.albedo), 1.0)).max(-1)
        ee = (np.abs(out["emission"].astype(F64) - A.emission) / np.maximum(np.abs(A.emission), 1.0)).max(-1)
    errs = {"frame": ef, "frame_mapped": ef, "wo": ew, "wo_mapped": ew, "hitPos": ep, "albedo": ea, "emission": ee}
    over = {"frame": ~A.mapped, "frame_mapped": A.mapped, "wo": ~A.mapped, "wo_mapped": A.mapped}      # the records a figure is taken over
    for q in SCALARS:
        errs[q] = np.abs(out[q].astype(F64) - A.scalars[q])
    exact = np.ones(n, bool)
    for q in VERBATIM:
        exact &= out[q].astype(F64) == A.scalars[q]
    exact &= (out["flags"].astype(np.int64) == A.flags) & (out["material_class"].astype(np.int64) == A.cls) & (out["_pad"] == 0).all(-1)
    for q in SCALARS:       # a scalar no texture feeds is a copy (albedo and emission still go through idt)
        exact &= A.fed[q] | (errs[q] == 0)
    R.exact = exact
    R.kind_ok = same_kind
    R.set_valued = A.set_valued
    R.set_valued_share = float(A.set_valued.mean())
    R.N_len = A.N_len
    R.small_N = A.mapped & ~(A.N_len >= N_MIN)
    R.errs = errs
    keep = ~R.small_N if not edge else np.zeros(n, bool)
    R.err = {}
    for q, e in errs.items():
        k = keep & over.get(q, True)
        R.err[q] = (float(e[k].max()), int(np.flatnonzero(k)[e[k].argmax()])) if k.any() else (0.0, -1)
    R.bad = ~exact | ~same_kind
    return R


def assert_report(R, what, edge=False, bounds=None):
    bounds = BOUNDS if bounds is None else bounds
    print("%s: %s  set-valued %.5f  |N| %.3g..%.3g" % (what, "  ".join("%s %.3e" % (q, e) for q, (e, _) in R.err.items()), R.set_valued_share,
                                                        R.N_len.min(), R.N_len.max()))
    assert not R.bad.any(), "%s: %d records not admissible (exact terms or finite / inf / NaN class), first %d" % (
        what, int(R.bad.sum()), int(np.flatnonzero(R.bad)[0]))
    if edge:
        return
    assert R.set_valued_share <= SET_VALUED_CAP, (what, R.set_valued_share)
    for q, (e, i) in R.err.items():
        assert e <= bounds[q], (what, q, e, bounds[q], i)
