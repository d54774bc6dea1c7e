"""CPU: the stage between a hit record and the BSDF — the oracle's getIntersectionData and ShadingContext (orc_shade_probe) and the host build
of the product's shade_geometry / make_shading_context / tex_sample (tests/emu/shade_emu.cpp over pt_shade_probe.h) — against the float64
witness (shading_witness.py; scenes and hits in shading_cases.py).  Every other check of this code is "programs by one author agree"; this
one names the frame, wo and the context a hit must get, from the scene description.

Asserted: every answer is admissible; the frame, wo, hitPos, albedo, emission and the textured scalars lie within shading_witness.BOUNDS on
the non-edge classes; flags, the class, the untextured terms and the padding are exact; at most 1 % of a non-edge class is set-valued; the
host build equals the oracle bit for bit, in both texture storage forms; the truth checks on instances with rotation and uniform scale
only; on the edges class bits, admissibility and the finite / inf / NaN class.  Each test prints its figures before it asserts.

Out of scope: the BSDF lobes, shade_nee_eval, shadow-ray occlusion, alpha cut-outs."""
import functools

import numpy as np
import pytest

import emu_lib
import oracle_lib
import shading_cases as sc
import shading_witness as sw
from platinum_amd import abi

F32, F64 = np.float32, np.float64


def words(out):
    return np.ascontiguousarray(out).view(np.uint32).reshape(len(out), -1)


FLOAT_WORDS = np.r_[np.ones(28, bool), np.zeros(4, bool)]      # flags, class and padding are integers


def same_bits(a, b, nan_payload=False):
    """Records equal word for word.  nan_payload=True: two NaNs in one float field count as equal whatever their sign and payload (0 / 0 is a
    NaN of either sign depending on the machine)."""
    wa, wb = words(a), words(b)
    eq = wa == wb
    if nan_payload:
        isnan = lambda w: (w & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
        eq = eq | (isnan(wa) & isnan(wb) & FLOAT_WORDS[None, :])
    return bool(eq.all())


def first_difference(a, b):
    i = np.flatnonzero((words(a) != words(b)).any(1))
    return None if not i.size else (int(i[0]), a[i[0]], b[i[0]])


@functools.lru_cache(maxsize=None)
def oracle(name):
    return oracle_lib.OracleScene(sc.scene(name), sc.params(name))


def emu(name, native, monkeypatch):
    """the host build of the product on the case, its 8-bit textures kept native or decoded"""
    monkeypatch.setenv("PTAMD_TEX_NATIVE", "1" if native else "0")
    e = emu_lib.EmuScene(sc.scene(name), sc.params(name))
    monkeypatch.delenv("PTAMD_TEX_NATIVE")
    return e


@functools.lru_cache(maxsize=None)
def witness(name):
    return sc.witness(name, oracle(name).constants())


@functools.lru_cache(maxsize=None)
def records(name, cls):
    if cls == "hits":
        o = oracle(name)
        return sc.hit_records(o.constants(), o.trace_primary(0), 0)
    return (sc.edge_batches() if name == "edges" else sc.batches(name))[cls]


@functools.lru_cache(maxsize=None)
def answer(name, cls):
    return witness(name).answer(records(name, cls))


@functools.lru_cache(maxsize=None)
def oracle_out(name, cls):
    return oracle(name).debugShading(records(name, cls))


@functools.lru_cache(maxsize=None)
def oracle_report(name, cls):
    return sw.check(answer(name, cls), oracle_out(name, cls), edge=name == "edges")


@pytest.mark.parametrize("name", sc.WITNESSED)
def test_oracle_and_host_build_are_admissible_and_within_the_bounds(name, monkeypatch):
    sides = {native: emu(name, native, monkeypatch) for native in (False, True)}
    for cls in list(sc.batches(name)) + ["hits"]:
        rec = records(name, cls)
        assert 0 < len(rec) <= 1 << 16
        sw.assert_report(oracle_report(name, cls), "%s %s, oracle" % (name, cls))
        for native, e in sides.items():
            h = e.debugShading(rec)
            assert same_bits(h, oracle_out(name, cls)), (native, first_difference(h, oracle_out(name, cls)))
        sw.assert_report(sw.check(answer(name, cls), h), "%s %s, host build" % (name, cls))


def test_the_cases_cover_what_they_claim():
    A = answer("frames", "lattice")
    dot = np.abs((A.nw * A.tw).sum(-1))
    assert (dot > 0.9 + 1e-3).any() and (dot < 0.9 - 1e-3).any() and ((dot > 0.895) & (dot < 0.9)).any() and ((dot > 0.9) & (dot < 0.91)).any()
    ax = np.abs(A.nw[:, 0])
    assert ((dot > 0.9) & (ax > 0.5)).any() and ((dot > 0.9) & (ax < 0.5)).any()
    assert set(np.unique(A.sgn)) == {-1.0, 1.0}
    A = answer("normalmaps", "lattice")
    assert A.mapped.all() and (A.N_len < sw.N_MIN).any() and (A.N_len > 0.9).any()
    print("|N| over the normal-mapped lattice: %.4g .. %.4g; below N_MIN: %d of %d" % (A.N_len.min(), A.N_len.max(), (A.N_len < sw.N_MIN).sum(), len(A.N_len)))
    ax = np.abs(A.frame[:, 2, 0] )
    assert (ax > 0.5 * A.N_len).any() and (ax < 0.5).any()
    uv = answer("slots", "lattice").uv
    assert uv.min() == -2.5 and uv.max() == 3.5
    s = sc.scene("slots")
    assert s.textures[0].pixels.nbytes == 15 and s.textures[0].format == abi.TEX_R8
    assert {t.format for t in s.textures} == set(sc.FORMATS.values())
    for slot in sc.SLOTS:
        assert {s.textures[getattr(m, slot)].format for n in s.nodes for m in n.materials if getattr(m, slot) >= 0} == set(sc.FORMATS.values()), slot
    assert set(answer("slots", "lattice").cls) == {3} and set(answer("frames", "lattice").cls) == {1, 2}


# ---- checks against truth, independent of the restated formulas ------------------------------------------------------------------------------
def _truth_selection(name, cls, meshes=sc.ORTHO):
    rec = records(name, cls)
    info = sc.scene(name).info
    sel = np.array([info[i][0] in meshes and info[i][1] in sc.TRUTH_KINDS for i in rec["instance"]])
    return rec, np.flatnonzero(sel)


def _world(name, rec, v):
    """v (object space) rotated into the world of each record's instance: the node's 3x3 with its uniform scale divided out"""
    out = np.zeros((len(rec), 3))
    for k, i in enumerate(rec["instance"]):
        Wm = np.asarray(sc.scene(name).nodes[i].world, F32).astype(F64)
        M = np.stack([Wm[0, :3], Wm[1, :3], Wm[2, :3]], axis=1)
        s = np.cbrt(np.linalg.det(M))
        assert s > 0 and np.allclose(M.T @ M, s * s * np.eye(3), atol=1e-6)        # rotation and uniform scale only
        out[k] = (M / s) @ v
    return out


@pytest.mark.parametrize("side", ["witness", "oracle"])
def test_an_orthonormal_n_t_under_rotation_and_uniform_scale_gives_the_true_frame(side):
    """frame = (sgn t, sgn (n x t), n), right-handed and orthonormal"""
    rec, sel = _truth_selection("frames", "lattice")
    assert sel.size >= 4 * 2 * 45
    n, t = _world("frames", rec[sel], sc.N0), _world("frames", rec[sel], sc.tangent_at(sc.N0, 90))
    sgn = np.array([1.0 if sc.scene("frames").info[i][0] == "ortho_p" else -1.0 for i in rec["instance"][sel]])
    if side == "witness":
        F, tol = answer("frames", "lattice").frame[sel], 1e-6       # (the scene's float32 inputs are orthonormal to 1e-7)
    else:
        o = oracle_out("frames", "lattice")[sel]
        F, tol = np.stack([o["x"], o["y"], o["z"]], axis=1).astype(F64), 1e-6 + sw.BOUNDS["frame"]
    truth = np.stack([sgn[:, None] * t, sgn[:, None] * np.cross(n, t), n], axis=1)
    print(side, "frame against truth: %.3e" % np.abs(F - truth).max())
    assert np.abs(F - truth).max() <= tol
    assert np.abs(np.cross(F[:, 0], F[:, 1]) - F[:, 2]).max() <= 3 * tol                                  # right-handed
    assert np.abs(np.einsum("nac,nbc->nab", F, F) - np.eye(3)).max() <= 3 * tol                          # orthonormal


@pytest.mark.parametrize("side", ["witness", "oracle"])
def test_without_a_normal_map_every_frame_is_orthonormal(side):
    for cls in ("lattice", "random", "hits"):
        if side == "witness":
            F, tol = answer("frames", cls).frame, 1e-12
        else:
            o = oracle_out("frames", cls)
            F, tol = np.stack([o["x"], o["y"], o["z"]], axis=1).astype(F64), 3 * sw.BOUNDS["frame"]
        assert np.abs(np.einsum("nac,nbc->nab", F, F) - np.eye(3)).max() <= tol


@pytest.mark.parametrize("side", ["witness", "oracle"])
def test_flat_and_tilted_normal_texels_give_the_true_normal(side):
    """a float-exact texel (0.5, 0.5, 1) leaves frame.z = n; one that encodes a tilt theta about the bitangent gives z = cos n + sin x"""
    rec, sel = _truth_selection("normalmaps", "lattice")
    s = sc.scene("normalmaps")
    tex = np.array([s.nodes[i].materials[s.meshes[s.nodes[i].mesh].material_slots[p]].normal_texture for i, p in zip(rec["instance"][sel], rec["primitive"][sel])])
    n, t = _world("normalmaps", rec[sel], sc.N0), _world("normalmaps", rec[sel], sc.tangent_at(sc.N0, 90))
    sgn = np.array([1.0 if s.info[i][0] == "ortho_p" else -1.0 for i in rec["instance"][sel]])
    if side == "witness":
        z, tol = answer("normalmaps", "lattice").frame[sel][:, 2], 1e-6
    else:
        z, tol = oracle_out("normalmaps", "lattice")[sel]["z"].astype(F64), 1e-6 + sw.BOUNDS["frame_mapped"]
    flat, tilt = tex == s.normal_ids["flat32"], tex == s.normal_ids["tilt32"]
    assert flat.sum() >= 45 and tilt.sum() >= 45
    print(side, "flat %.3e  tilt %.3e" % (np.abs(z[flat] - n[flat]).max(), np.abs(z[tilt] - (np.cos(sc.TILT) * n + np.sin(sc.TILT) * sgn[:, None] * t)[tilt]).max()))
    assert np.abs(z[flat] - n[flat]).max() <= tol
    assert np.abs(z[tilt] - (np.cos(sc.TILT) * n + np.sin(sc.TILT) * sgn[:, None] * t)[tilt]).max() <= tol


def test_the_unnormalised_mapped_normal_is_a_recorded_quirk():
    """|z| = |x| = |N| and |y| = 1 after a normal map: the reference's behaviour, followed"""
    o = oracle_out("normalmaps", "lattice")
    A = answer("normalmaps", "lattice")
    keep = A.N_len >= sw.N_MIN
    ln = lambda v: np.linalg.norm(v.astype(F64), axis=1)
    assert np.abs(ln(o["z"]) / A.N_len - 1)[keep].max() < 1e-5 and np.abs(ln(o["x"]) / A.N_len - 1)[keep].max() < 1e-4 and np.abs(ln(o["y"]) - 1)[keep].max() < 1e-5
    assert (np.abs(A.N_len - 1) > 0.05).any()


# ---- the edges class ---------------------------------------------------------------------------------------------------------------------
def test_edges_have_equal_bits_and_the_class_float64_predicts(monkeypatch):
    sides = {native: emu("edges", native, monkeypatch) for native in (False, True)}
    for cls in sc.edge_batches():
        rec = records("edges", cls)
        sw.assert_report(oracle_report("edges", cls), "edges %s, oracle" % cls, edge=True)
        for native, e in sides.items():
            h = e.debugShading(rec)
            assert same_bits(h, oracle_out("edges", cls)), (cls, native, first_difference(h, oracle_out("edges", cls)))
    z = oracle_out("edges", "n_zero")
    assert np.all(z["z"] == 0) and np.isnan(z["x"]).all() and np.isnan(z["y"]).all()            # N = 0: recorded, not blessed
    t = oracle_out("edges", "zero_tangent")
    at_zero = (records("edges", "zero_tangent")["u"] == 0.5) & (records("edges", "zero_tangent")["v"] == 0)
    assert at_zero.sum() == 1 and np.isnan(t["x"][at_zero]).all() and np.isnan(t["y"][at_zero]).all() and np.isfinite(t["z"]).all()
    assert np.isfinite(t["x"][~at_zero]).all()


def check_huge_uv(out, idt):
    """Every textured term of the huge-UV records is finite and lies within its texture's range (a bilinear mix never leaves it)"""
    s = sc.scene("edges")
    rng = lambda tid, ch: (sw.decode(s.textures[tid].pixels, s.textures[tid].format)[..., ch].min(), sw.decode(s.textures[tid].pixels, s.textures[tid].format)[..., ch].max())
    T = s.huge_textures
    eps = 1e-5
    pre = out["albedo"].astype(F64) @ np.linalg.inv(idt).T              # the texel before the colour matrix
    for ch in range(3):
        lo, hi = rng(T["albedo"], ch)
        assert np.isfinite(pre).all() and pre[:, ch].min() >= lo - eps and pre[:, ch].max() <= hi + eps, ("albedo", ch)
    for q, tid, ch, scale in (("transmission", T["transmission"], 0, 1.0), ("clearcoat", T["clearcoat"], 0, 1.0), ("roughness", T["rm"], 0, 0.8), ("metallic", T["rm"], 1, 0.6)):
        lo, hi = rng(tid, ch)
        v = out[q].astype(F64) / F64(F32(scale))
        assert np.isfinite(v).all() and v.min() >= lo - eps and v.max() <= hi + eps, q
    assert np.isfinite(out["emission"]).all() and (out["emission"] >= -eps).all()


def test_huge_uvs_give_finite_in_range_texels_on_the_host():
    import geometry_witness as gw
    check_huge_uv(oracle_out("edges", "huge_uv"), gw.idt_of(oracle("edges").constants()))


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
def measure_oracle():
    """The worst error of the oracle against the witness over shading_cases.measure_list(): what shading_witness.MEASURED records."""
    worst = {}
    for name, cls in sc.measure_list():
        for q, (e, _) in oracle_report(name, cls).err.items():
            if q not in worst or e > worst[q][0]:
                worst[q] = (e, "%s %s" % (name, cls))
    return worst


def test_the_bounds_table_is_four_times_the_oracles_measured_worst():
    worst = measure_oracle()
    print("measured on the oracle:", worst)
    assert set(worst) == set(sw.MEASURED)
    for q, (m, where) in sw.MEASURED.items():
        assert worst[q][0] <= m <= 1.05 * worst[q][0], (q, worst[q], m)     # (recorded to three digits, rounded up)
        assert where == worst[q][1], (q, where, worst[q][1])
        assert sw.BOUNDS[q] == 4.0 * m


def test_set_valued_shares_stay_under_the_cap_on_the_oracle():
    shares = {(n, c): oracle_report(n, c).set_valued_share for n, c in sc.measure_list()}
    top = max(shares, key=shares.get)
    print("largest set-valued share: %.5f at %s" % (shares[top], top))
    assert shares[top] <= sw.SET_VALUED_CAP


def test_a_set_valued_hit_admits_both_branches():
    """the class exists: a tangent whose |n . t| is 0.9 to 1e-6 is answered by either frame, and by nothing else"""
    mesh = sc.scenes._make_mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 0, 1)] * 3, [[*sc.tangent_at((0, 0, 1), np.degrees(np.arccos(0.9 + 1e-6))), 1.0]] * 3,
                                [(0, 0)] * 3, [0, 1, 2], [0])
    s = sc.scenes.Scene()
    s.add_instance(s.add_mesh(mesh), sc.Transform(), [sc.PLAIN[0]])
    W = sw.Witness(s, np.eye(3))
    rec = np.zeros(1, abi.SHADE_PROBE_IN_DTYPE)
    rec["u"], rec["v"], rec["d"], rec["t"] = 0.25, 0.25, (0, 0, -1), 1.0
    A = W.answer(rec)
    assert A.set_valued.all() and A.valid.sum() == 2
    for k in np.flatnonzero(A.valid[:, 0]):
        out = np.zeros(1, abi.SHADE_PROBE_OUT_DTYPE)
        out["x"], out["y"], out["z"] = A.frames[k, 0]
        out["wo"], out["hitPos"] = A.wo[k, 0], A.hitPos[0]
        out["albedo"], out["emission"] = A.albedo[0], A.emission[0]
        for q in sw.SCALARS + sw.VERBATIM:
            out[q] = A.scalars[q][0]
        out["flags"], out["material_class"] = A.flags[0], A.cls[0]
        R = sw.check(A, out)
        assert not R.bad.any() and R.err["frame"][0] < 1e-6
    out["y"] = -out["y"]
    assert sw.check(A, out).err["frame"][0] > 0.5


def test_debug_shading_refuses_bad_arguments_before_the_renderer_is_looked_at():
    import ctypes as C
    lib = abi.load_library()
    rec = np.zeros(4, abi.SHADE_PROBE_IN_DTYPE)
    out = np.zeros((4, abi.PT_SHADE_PROBE_OUT_WORDS), np.uint32)
    pi, po = rec.ctypes.data, out.ctypes.data
    for call, word in (((0, pi, po), b"2^24"), (((1 << 24) + 1, pi, po), b"2^24"), ((4, None, po), b"null argument"), ((4, pi, None), b"null argument"),
                       ((4, pi, po), b"null renderer")):
        assert lib.pt_debug_shading(None, *call) == -1 and word in lib.pt_last_error(), (call, lib.pt_last_error())


def test_the_oracle_and_the_host_build_refuse_a_record_outside_the_scene(monkeypatch):
    rec = records("frames", "outside")[:4].copy()
    e = emu("frames", False, monkeypatch)
    for field, value in (("instance", len(sc.scene("frames").nodes)), ("primitive", 2)):
        bad = rec.copy()
        bad[field][2] = value
        with pytest.raises(RuntimeError):
            oracle("frames").debugShading(bad)
        with pytest.raises(RuntimeError):
            e.debugShading(bad)
