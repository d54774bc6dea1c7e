"""CPU: the light-sampling part of the shading stage — the oracle's sampleLightPower / sampleAreaLight / sampleEnvironmentLight / miss branch
(orc_light_sample, orc_env_miss) and the host build of the product's shade_nee_light / stage_miss (tests/emu/light_emu.cpp over
pt_light_probe.h) — against the float64 witness (light_witness.py; scenes and draws in light_cases.py).  Every other check of this code is
"programs by one author agree"; this one names the light a draw must select and the density it must report, from the scene description.

Asserted: every answer is admissible; lwi, dist, lpdf, pLight, Li, the environment's wi / pdf / Li and the miss radiance lie within
light_witness.BOUNDS on the non-edge classes; lit and dim are exact; at most 1 % of a non-edge class is set-valued; the stratified
selection counts and the environment counts; the alias table against the float64 luma distribution; on the edges class bits, admissibility
and the finite / inf / NaN class.  Each test prints its figures before it asserts (pytest -s shows them).

Out of scope: the BSDF and the NEE eval, normal-mapped frames, shadow-ray occlusion."""
import ctypes as C
import functools

import numpy as np
import pytest

import emu_lib
import light_cases as lc
import light_lib
import light_witness as lw
import oracle_lib
from platinum_amd import abi

F32, F64 = np.float32, np.float64
S, M = abi.PT_LIGHT_SAMPLE, abi.PT_LIGHT_ENV_MISS
LIGHT_CASES = [n for n in lc.WITNESSED if lc.CASES[n].kind != "env"]
ENV_CASES = [n for n in lc.WITNESSED if lc.CASES[n].kind != "lights"]


@functools.lru_cache(maxsize=None)
def sides(name, integrator=abi.INTEGRATOR_MIS):
    sc, p = lc.scene(name), lc.params(name, integrator)
    return oracle_lib.OracleScene(sc, p), emu_lib.EmuScene(sc, p)


@functools.lru_cache(maxsize=None)
def witness(name):
    o, _ = sides(name)
    return lc.witness(name, o.constants(), o.envAlias())


@functools.lru_cache(maxsize=None)
def oracle_out(name, cls):
    b = lc.batches(name)[cls]
    return sides(name)[0].debugLights(b.fn, b.rec, **b.args)


@functools.lru_cache(maxsize=None)
def oracle_report(name, cls):
    b, W = lc.batches(name)[cls], witness(name)
    return (W.check_sample if b.fn == S else W.check_miss)(b.rec, oracle_out(name, cls), **b.args)


def check(W, b, out, edge=False):
    args = {k: v for k, v in b.args.items() if k != "tables"}
    return (W.check_sample if b.fn == S else W.check_miss)(b.rec, out, edge=edge, **args)


def host_tables(e, b):
    """the host build's answer with the table in "HBM", after asserting that the staged form gives the same bits (or is refused: > 64 lights)"""
    h = e.debugLights(b.fn, b.rec, **b.args)
    if b.fn == S:
        if e.constants().lightCount <= 64:
            staged = e.debugLights(b.fn, b.rec, tables=abi.PT_LIGHT_TABLES_LDS, **b.args)
            assert light_lib.same_bits(h, staged), light_lib.first_difference(h, staged)
        else:
            with pytest.raises(RuntimeError):
                e.debugLights(b.fn, b.rec, tables=abi.PT_LIGHT_TABLES_LDS, **b.args)
    return h


@pytest.mark.parametrize("name", lc.WITNESSED)
def test_oracle_and_host_build_are_admissible_and_within_the_bounds(name):
    o, e = sides(name)
    assert bytes(o.constants())[:C.sizeof(abi.Constants)] == bytes(e.constants())[:C.sizeof(abi.Constants)]
    for cls, b in lc.batches(name).items():
        lw.assert_report(oracle_report(name, cls), "%s %s, oracle" % (name, cls))
        h = host_tables(e, b)
        assert light_lib.same_bits(h, oracle_out(name, cls)), light_lib.first_difference(h, oracle_out(name, cls))
        lw.assert_report(check(witness(name), b, h), "%s %s, host build" % (name, cls))


@pytest.mark.parametrize("name", LIGHT_CASES)
def test_stratified_draws_select_each_light_in_proportion_to_its_power(name):
    """On a stratified grid of M draws rz' = (j + 1/2) / M the lights' intervals [cum_{i-1}, cum_i) / total hold M power_i / total points
    each, to one grid point per interval end (2) and one more for the fp32 rounding of rz' * total against the table: |count - expected| <= 3.
    A light without power gets none."""
    W = witness(name)
    rep = oracle_report(name, "rz_grid")
    assert not rep.bad.any(), rep.why
    area = rep.chosen >= 0
    m = int(area.sum())
    assert m == (1 << 16 if W.p_inf == 0 else 1 << 15)
    count = np.bincount(rep.chosen[area], minlength=W.L.n)
    want = m * W.L.power / W.L.total
    print(name, "worst |count - expected| %.3f over %d lights" % (np.abs(count - want).max(), W.L.n))
    assert np.abs(count - want).max() <= 3, (count, want)
    assert np.all(count[W.L.power < 1e-12 * W.L.total] == 0)
    if name == "zero_between":
        assert (W.L.power < 1e-12 * W.L.total).sum() == 3
        cum = np.array([l.cumulativePower for l in sides(name)[0].lights()])
        assert (np.diff(cum) == 0).sum() == 3                       # ties in the table itself
    if name == "graded":
        assert np.allclose(W.L.power / W.L.power[0], [1, 2, 4, 8, 16], rtol=1e-6)


@pytest.mark.parametrize("name", ENV_CASES)
def test_environment_grid_lands_on_each_texel_as_often_as_the_table_implies(name):
    """The grid has n K columns (rl.x = (c + 1/2) / (n K)) and K rows (rl.y = (j + 1/2) / K).  rl.x n = (c + 1/2) / K is at least 1 / (2 K)
    from an integer, so texel i is the first pick of exactly K columns, K^2 points.  Of each column's K rows those with rl.y < p_i keep the
    texel and the others go to its alias; the number of rows below p_i is p_i K to within one row.  A texel's count therefore differs from
    K^2 (p_i + sum over j with alias_j = i of (1 - p_j)) by at most one row of K columns for itself and one for each entry that names it:
    K (1 + m_i).  The witness also counts the rows exactly (rl.y and p are floats, the comparison is exact): that count must be met."""
    W = witness(name)
    E = W.E
    K = lc.env_grid_k(E.n)
    rep = oracle_report(name, "env_grid")
    assert np.all(rep.chosen <= -2) and not rep.set_valued.any() and not rep.bad.any()
    count = np.bincount(-2 - rep.chosen, minlength=E.n)
    implied = K * K * E.n * E.implied_distribution()
    named = np.bincount(E.alias[E.p < 1], minlength=E.n)
    print(name, "K %d, worst |count - implied| / K %.3f" % (K, (np.abs(count - implied) / K).max()))
    assert np.all(np.abs(count - implied) <= K * (1 + named)), (count, implied)
    if len({tuple(t) for t in E.px.reshape(-1, 4).tolist()}) == E.n:       # (identical texels cannot be told apart by their sample: the sky's)
        assert np.array_equal(count, E.counts(K)), (count, E.counts(K))
    assert count.sum() == E.n * K * K


@pytest.mark.parametrize("name", ENV_CASES)
def test_the_alias_table_is_the_luma_distribution(name):
    """pdf_i = n luma_i / sum luma, and the distribution the table implies, (p_i + sum_{alias_j = i} (1 - p_j)) / n, is the same one: both to
    what Vose's method leaves in fp32 (light_witness.Env.alias_bound)."""
    o, e = sides(name)
    assert o.envAlias().tobytes() == e.envAlias().tobytes()
    E = witness(name).E
    e_pdf, e_implied = E.alias_errors()
    print(name, "pdf %.3e  implied %.3e  bound %.3e" % (e_pdf, e_implied, E.alias_bound()))
    assert e_pdf <= E.alias_bound() and e_implied <= E.alias_bound()
    assert np.all((E.p >= 0) & (E.p <= 1))
    if lc.scene(name).env_alias is not None:
        assert o.envAlias().tobytes() == np.ascontiguousarray(lc.scene(name).env_alias).tobytes()     # a host-supplied table is used as it comes
        own = oracle_lib.OracleScene(lc.env_scene("3x5", True), lc.params(name)).envAlias()
        assert own.tobytes() != o.envAlias().tobytes()                                                  # and it is another table than the renderer's own


@pytest.mark.parametrize("name", ["n5", "n65", "graded", "zero_between"])
def test_a_draw_that_meets_a_table_entry_exactly_selects_that_entry(name):
    """"Find the first light with cumulative power >= r" (kernel.metal:383): when rz' * total IS an entry of the running sum (the fp32 product
    equals the fp32 entry), that entry's light is the answer — the strict `<` of the search.  The float64 witness calls such a draw set-valued;
    here the side's own table decides.  (A zero-power light shares its entry with the light before it: the first of them is the answer.)"""
    for side in sides(name):
        ties = lc.tie_draws(side.lights(), side.constants().totalLightPower)
        assert len(ties) >= 2, ties
        rec = np.array([[*lc.HIT, 0.3, 0.6, rz] for _, rz in ties], F32)
        out = side.debugLights(S, rec, roughness=0.3, metallic=1.0, dim=5)
        rep = witness(name).check_sample(rec, out, roughness=0.3, metallic=1.0, dim=5)
        assert not rep.bad.any() and rep.set_valued.all()
        cum = np.array([l.cumulativePower for l in side.lights()], F32)
        first = np.array([int(np.flatnonzero(cum == cum[i])[0]) for i, _ in ties])
        assert np.array_equal(rep.chosen, first), (rep.chosen, first)


def test_a_black_texel_always_hands_the_draw_to_its_alias():
    """p = 0 exactly for a black texel: rl.y = 0 must take the alias (r.y >= p, not >)."""
    name = "env_black"
    o, e = sides(name)
    W = witness(name)
    black = np.flatnonzero(W.E.p32 == 0)
    assert black.size == 3 and np.all(W.E.pdf[black] == 0)
    rec = np.zeros((black.size * 2, 6), F32)
    rec[:, :3] = lc.HIT
    rec[:, 3] = np.repeat((black + 0.5) / W.E.n, 2)
    rec[:, 4] = np.tile([0.0, 0.5], black.size)
    for side in (o, e):
        out = side.debugLights(S, rec, roughness=0.3, metallic=1.0, dim=5)
        rep = W.check_sample(rec, out, roughness=0.3, metallic=1.0, dim=5)
        assert not rep.bad.any(), rep.why
        assert np.array_equal(-2 - rep.chosen, np.repeat(W.E.alias[black], 2)) and np.all(out["lpdf"] > 0)


@pytest.mark.parametrize("name", list(lc.CASES))
def test_edges_agree_in_bits_are_admissible_and_of_the_class_float64_predicts(name):
    o, e = sides(name)
    kind = lc.CASES[name].kind
    for cls, b in lc.edge_batches(name).items():
        a = o.debugLights(b.fn, b.rec, **b.args)
        h = host_tables(e, b)
        assert light_lib.same_bits(a, h), (cls, light_lib.first_difference(a, h))
        if kind in ("lights", "env", "env_lights"):
            lw.assert_report(check(witness(name), b, a, edge=True), "%s edges %s" % (name, cls), edge=True)
        elif kind == "zero":
            # totalLightPower == 0: rz' * 0 = 0 is below no entry, the search stays on light 0; pLight = (1 - 0) * 0 / 0 is a NaN
            assert o.constants().totalLightPower == 0.0 and o.constants().lightCount == 3
            first = witness_free_emission(name, 0)
            assert np.all(a["lit"] == 1) and np.all(np.isnan(a["pLight"])) and np.all(np.isfinite(a["lpdf"])) and np.allclose(a["Li"], first, rtol=1e-6)
        else:
            assert np.all(a["lit"] == 0) and np.all(a["dim"] == 5 + 9)
    if name == "exact":
        a = o.debugLights(*lc.edge_batches(name)["hits"][:2], **lc.edge_batches(name)["hits"].args)
        assert np.all(np.isnan(a["lwi"][0])) and a["dist"][0] == 0 and np.isnan(a["lpdf"][0])        # on the sampled point: 0 / 0
        assert np.isposinf(a["lpdf"][1]) and np.all(np.isfinite(a["lwi"][1]))                         # in the light's plane: x / 0
        assert np.isfinite(a["lpdf"][2]) and a["lpdf"][2] == F32(4.0 / 0.5)                           # straight below: dist 2, cos 1, area 1/2


def witness_free_emission(name, i):
    sc = lc.scene(name)
    m = sc.nodes[0].materials[i]
    return np.asarray(m.emission, F64) * m.emission_strength      # (BT709: the working space is the material's)


@pytest.mark.parametrize("gate", list(lc.GATES))
def test_the_gate_decides_lit_and_dim_exactly(gate):
    rough, metal, trans, plus = lc.GATES[gate]
    rec = lc.lattice()[:512]
    for name in ("n3", "env_3x5_lights", "none"):
        o, e = sides(name)
        kw = dict(roughness=rough, metallic=metal, transmission=trans, dim=7)
        a, h = o.debugLights(S, rec, **kw), e.debugLights(S, rec, **kw)
        assert light_lib.same_bits(a, h)
        assert np.all(a["dim"] == 7 + plus) and np.all(a["lit"] == (1 if plus == 9 and name != "none" else 0))
        if name != "none":
            lw.assert_report(witness(name).check_sample(rec, a, **kw), "%s gate %s" % (name, gate))
        else:
            assert not light_lib.words(a)[:, 1:10].any()
    # the simple integrator never samples a light: not lit, dim + 6, whatever the material
    o, e = sides("n3", abi.INTEGRATOR_SIMPLE)
    a, h = o.debugLights(S, rec, roughness=0.3, metallic=1.0, dim=7), e.debugLights(S, rec, roughness=0.3, metallic=1.0, dim=7)
    assert light_lib.same_bits(a, h) and np.all(a["dim"] == 13) and not a["lit"].any()


def test_the_witness_on_cases_worked_by_hand():
    """The witness's own pieces against answers known without it."""
    # a unit right triangle under scale (2, 1, 4): world area 4; power = pi * 4 * green; normal: cross((0,0,1), (1,0,0)) = +y through the forward matrix
    W = witness("graded")
    assert np.allclose(W.L.area, [0.5, 1, 2, 4, 8], rtol=1e-6) and W.L.n == 5 and W.p_inf == 0.0
    assert np.allclose(W.L.power, np.pi * W.L.area * 3.0, rtol=1e-6)
    # the search: with cum = 1, 3, 7, 15, 31 (x 0.5 pi 3) a draw at 3 / 31 exactly belongs to light 1 (strict <), just above it to light 2
    lo, hi = W.L.admissible(np.array([3.0 / 31 - 1e-3, 3.0 / 31 + 1e-3, 0.0, 0.999]) * W.L.total)
    assert lo.tolist() == [1, 2, 0, 4] and hi.tolist() == [1, 2, 0, 4]
    # bilinear-repeat at a texel's own uv = (x / w, y / h) is the mean of the four texels that meet at its upper left corner, wrapping
    px = np.arange(24, dtype=F64).reshape(2, 3, 4)
    got = lw.bilinear_repeat(px, np.array([0.0, 1 / 3]), np.array([0.0, 0.5]))
    assert np.allclose(got[0], (px[1, 2] + px[1, 0] + px[0, 2] + px[0, 0]) / 4) and np.allclose(got[1], (px[0, 0] + px[0, 1] + px[1, 0] + px[1, 1]) / 4)
    # the alias table of (1, 3): pdf = (0.5, 1.5), texel 0 keeps half of its draws: the implied distribution is (1/4, 3/4)
    E = witness("env_2x1").E
    t = lc.vose_fifo(np.array([[[1, 1, 1, 1], [3, 3, 3, 1]]], F32))
    assert t["pdf"].tolist() == [0.5, 1.5] and t["p"].tolist() == [0.5, 1.0] and t["aliasIdx"][0] == 1
    E2 = lw.Env.__new__(lw.Env)
    E2.p, E2.alias, E2.n = t["p"].astype(F64), t["aliasIdx"].astype(np.int64), 2
    assert np.allclose(E2.implied_distribution(), [0.25, 0.75]) and E.n == 2
    # directions: uv (0, 1/2) looks along -x, (1/4, 1/2) along -z, v = 0 is +y
    Ws = witness("env_sky").E
    _, wi, _ = Ws.texel(np.array([8 * 32 + 0, 8 * 32 + 8, 0]))
    assert np.allclose(wi, [[-1, 0, 0], [0, 0, -1], [0, 1, 0]], atol=1e-12)


def test_debug_lights_refusals_come_before_the_renderer():
    """unknown fn, n = 0, n > 2^24, null pointers, an unknown table, a draw outside [0, 1) and a direction outside the unit cube are refused
    before the renderer is looked at; a null renderer after that"""
    lib = abi.load_library()
    rec = np.zeros((4, 8), F32)
    out = np.zeros((4, 12), np.uint32)
    args = abi.LightProbeArgs(0.3, 1.0, 0.0, 5, abi.PT_LIGHT_TABLES_HBM, 1, 0)
    pa, pi, po = C.byref(args), rec.ctypes.data, out.ctypes.data
    bad_tables = abi.LightProbeArgs(0.3, 1.0, 0.0, 5, 2, 1, 0)
    one = rec.copy(); one[2, 5] = 1.0
    nan = rec.copy(); nan[1, 3] = np.nan
    far = np.zeros((4, 4), F32); far[3, 1] = 1.5
    for call, word in (((abi.PT_LIGHT_COUNT, 4, pa, pi, po), b"unknown function"), ((S, 0, pa, pi, po), b"2^24"), ((S, (1 << 24) + 1, pa, pi, po), b"2^24"),
                       ((S, 4, None, pi, po), b"null argument"), ((S, 4, pa, None, po), b"null argument"), ((S, 4, pa, pi, None), b"null argument"),
                       ((S, 4, C.byref(bad_tables), pi, po), b"tables"), ((S, 4, pa, one.ctypes.data, po), b"draw"), ((S, 4, pa, nan.ctypes.data, po), b"draw"),
                       ((M, 4, pa, far.ctypes.data, po), b"direction"), ((S, 4, pa, pi, po), b"null renderer"), ((M, 4, pa, pi, po), b"null renderer")):
        assert lib.pt_debug_lights(None, *call) == -1 and word in lib.pt_last_error(), (call, lib.pt_last_error())


def measure_oracle():
    """The worst error of the oracle against the witness over light_cases.measure_list(): what light_witness.MEASURED records."""
    worst = {}
    for name, cls in lc.measure_list():
        for q, (e, _) in oracle_report(name, cls).err.items():
            if q not in worst or e > worst[q][0]:
                worst[q] = (e, "%s %s" % (name, cls))
    return worst


def test_the_bounds_table_is_four_times_the_oracles_measured_worst():
    worst = measure_oracle()
    print("measured on the oracle:", worst)
    assert set(worst) == set(lw.MEASURED)
    for q, (m, where) in lw.MEASURED.items():
        assert worst[q][0] <= m <= 1.05 * worst[q][0], (q, worst[q], m)     # (recorded to three digits, rounded up)
        assert where == worst[q][1], (q, where, worst[q][1])
        assert lw.BOUNDS[q] == 4.0 * m


def test_set_valued_shares_stay_under_the_cap_on_the_oracle():
    shares = {(n, c): oracle_report(n, c).set_valued_share for n, c in lc.measure_list()}
    top = max(shares, key=shares.get)
    print("largest set-valued share: %.5f at %s" % (shares[top], top))
    assert shares[top] <= lw.SET_VALUED_CAP
    assert shares[("n200", "rz_grid")] > 0          # the class exists: the cap is not vacuous
