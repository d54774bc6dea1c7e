"""GPU: pt_debug_lights (include/ptamd.h, platinum_amd/csrc/light_probe.hip) runs the light-sampling part of the shading stage on the device
against a started render's scene.  The device must be the same bits as the host build of the same headers and as the oracle's twin, with
the light table read from HBM and staged in LDS, and is held directly to the float64 witness (light_witness.py) under the bounds measured on
the oracle.  Renders of the 64- and 65-light scenes and of an environment with lights hold the staged and unstaged tables inside k_shade
itself to the oracle's bytes.  Every scene is 8 x 8; a probe batch holds at most 2^16 elements."""
import ctypes as C

import numpy as np
import pytest

import light_cases as lc
import light_lib
import light_witness as lw
import test_light_witness_host as host
from platinum_amd import abi

pytestmark = pytest.mark.gpu
F32 = np.float32
S, M = abi.PT_LIGHT_SAMPLE, abi.PT_LIGHT_ENV_MISS


@pytest.fixture(scope="module")
def r(gpu_renderer):
    before = gpu_renderer.selectedKernel()
    yield gpu_renderer
    gpu_renderer.selectKernel(before)


def start(r, name, integrator=abi.INTEGRATOR_MIS):
    r.selectKernel(integrator)
    r.startRender(lc.scene(name), lc.SIZE, lc.SPP, workingSpace=lc.CASES[name].working_space, max_bounces=lc.BOUNCES)


def three(r, name, b, nan_payload=False):
    """the device's records, after asserting device (HBM table) == device (LDS table) == host build == oracle"""
    o, e = host.sides(name)
    d, h, a = r.debugLights(b.fn, b.rec, **b.args), e.debugLights(b.fn, b.rec, **b.args), o.debugLights(b.fn, b.rec, **b.args)
    assert light_lib.same_bits(h, a), ("host build / oracle", light_lib.first_difference(h, a))
    assert light_lib.same_bits(d, h, nan_payload), ("device / host build", light_lib.first_difference(d, h))
    if b.fn == S:
        if r.constants().lightCount <= 64:
            staged = r.debugLights(b.fn, b.rec, tables=abi.PT_LIGHT_TABLES_LDS, **b.args)
            assert light_lib.same_bits(d, staged), ("HBM / LDS table", light_lib.first_difference(d, staged))
        else:
            with pytest.raises(RuntimeError, match="64 lights"):
                r.debugLights(b.fn, b.rec, tables=abi.PT_LIGHT_TABLES_LDS, **b.args)
    return d


@pytest.mark.parametrize("name", lc.WITNESSED)
def test_device_equals_host_build_and_oracle_and_meets_the_witness_bounds(r, name):
    start(r, name)
    c, oc = r.constants(), host.sides(name)[0].constants()
    assert (c.lightCount, c.envLightCount, c.totalLightPower, bytes(c.idt)) == (oc.lightCount, oc.envLightCount, oc.totalLightPower, bytes(oc.idt))
    assert [bytes(l) for l in r.lights()] == [bytes(l) for l in host.sides(name)[0].lights()]
    if lc.CASES[name].kind != "lights":
        assert r.envAlias().tobytes() == host.sides(name)[0].envAlias().tobytes()
    W = lc.witness(name, r.constants(), r.envAlias())
    for cls, b in lc.batches(name).items():
        d = three(r, name, b)
        lw.assert_report(host.check(W, b, d), "%s %s, device" % (name, cls))


@pytest.mark.parametrize("name", list(lc.CASES))
def test_device_edges_equal_host_build_and_oracle_and_are_admissible(r, name):
    """The edges class: bits (two NaNs of one field count as equal: 0 / 0 has the other sign on the device), admissibility, and the finite /
    inf / NaN class float64 predicts."""
    start(r, name)
    kind = lc.CASES[name].kind
    for cls, b in lc.edge_batches(name).items():
        d = three(r, name, b, nan_payload=True)
        if kind in ("lights", "env", "env_lights"):
            W = lc.witness(name, r.constants(), r.envAlias())
            lw.assert_report(host.check(W, b, d, edge=True), "%s edges %s, device" % (name, cls), edge=True)
        elif kind == "zero":
            assert r.constants().totalLightPower == 0.0 and np.all(d["lit"] == 1) and np.all(np.isnan(d["pLight"]))
        else:
            assert np.all(d["lit"] == 0) and np.all(d["dim"] == 5 + 9)


@pytest.mark.parametrize("name", ["n5", "n65", "graded", "zero_between"])
def test_a_draw_that_meets_a_table_entry_exactly_selects_that_entry_on_the_device(r, name):
    """the strict `<` of the search, where the fp32 product rz' * total equals an entry of the device's own table (see the host test)"""
    start(r, name)
    ties = lc.tie_draws(r.lights(), r.constants().totalLightPower)
    assert len(ties) >= 2
    b = lc.Batch(S, np.array([[*lc.HIT, 0.3, 0.6, rz] for _, rz in ties], F32), dict(roughness=0.3, metallic=1.0, dim=5))
    d = three(r, name, b)
    rep = host.check(lc.witness(name, r.constants(), None), b, d)
    cum = np.array([l.cumulativePower for l in r.lights()], F32)
    assert not rep.bad.any() and np.array_equal(rep.chosen, [int(np.flatnonzero(cum == cum[i])[0]) for i, _ in ties])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1 << 16])
def test_probe_sizes(r, n):
    """one element, one below / at / above a wave, and the largest batch of the suite: every element is written, none beyond"""
    name = "env_3x5_lights"
    start(r, name)
    o, _ = host.sides(name)
    for b in (lc.batches(name)["rz_grid"], lc.Batch(M, np.resize(lc.miss_directions(), (1 << 16, 4)), dict(bounce=2, lastSpecular=False))):
        rec = b.rec[:n]
        d = r.debugLights(b.fn, rec, **b.args)
        assert len(d) == n and light_lib.same_bits(d, o.debugLights(b.fn, rec, **b.args))


@pytest.mark.parametrize("gate", list(lc.GATES))
def test_the_gate_on_the_device(r, gate):
    rough, metal, trans, plus = lc.GATES[gate]
    rec = lc.lattice()[:512]
    kw = dict(roughness=rough, metallic=metal, transmission=trans, dim=7)
    for name in ("n3", "none"):
        start(r, name)
        d = three(r, name, lc.Batch(S, rec, kw))
        assert np.all(d["dim"] == 7 + plus) and np.all(d["lit"] == (1 if plus == 9 and name != "none" else 0))
    start(r, "n3", abi.INTEGRATOR_SIMPLE)
    d = r.debugLights(S, rec, **kw)
    assert light_lib.same_bits(d, host.sides("n3", abi.INTEGRATOR_SIMPLE)[1].debugLights(S, rec, **kw)) and np.all(d["dim"] == 13) and not d["lit"].any()


def test_debug_lights_refusals(r):
    lib = r._lib
    rec = np.zeros((4, 8), F32)
    rec[:, 1] = 1.0
    out = np.zeros((4, 12), np.uint32)
    args = abi.LightProbeArgs(0.3, 1.0, 0.0, 5, abi.PT_LIGHT_TABLES_HBM, 1, 0)
    staged = abi.LightProbeArgs(0.3, 1.0, 0.0, 5, abi.PT_LIGHT_TABLES_LDS, 1, 0)
    pa, pi, po = C.byref(args), rec.ctypes.data, out.ctypes.data
    call = lambda h, *a: lib.pt_debug_lights(h, *a)
    from platinum_amd import Renderer
    fresh = Renderer(device=0)
    try:
        assert call(fresh._h, S, 4, pa, pi, po) == -5 and b"before pt_start_render" in lib.pt_last_error()
    finally:
        fresh.close()
    start(r, "n65")
    for a in ((abi.PT_LIGHT_COUNT, 4, pa, pi, po), (S, 0, pa, pi, po), (S, (1 << 24) + 1, pa, pi, po), (S, 4, None, pi, po), (S, 4, pa, None, po),
              (S, 4, pa, pi, None)):
        assert call(r._h, *a) == -1, a
    assert call(r._h, S, 4, C.byref(staged), pi, po) == -6 and b"64 lights" in lib.pt_last_error()      # 65 lights do not fit the staged table
    assert call(r._h, M, 4, pa, pi, po) == -6 and b"environment" in lib.pt_last_error()                  # no environment
    assert call(r._h, S, 4, pa, pi, po) == 0 and np.all(out[:, 0] == 1) and np.all(out[:, 10] == 14)
    start(r, "n64")
    assert call(r._h, S, 4, C.byref(staged), pi, po) == 0 and np.all(out[:, 0] == 1)                     # 64 do


@pytest.mark.parametrize("name", ["n64", "n65", "env_3x5_lights"])
def test_renders_with_staged_and_unstaged_light_tables_equal_the_oracle(r, name):
    """8 x 8, 2 spp, MIS: k_shade stages 64 lights in LDS and reads 65 from HBM (light_cdf); the accumulator must be the oracle's bytes"""
    start(r, name)
    r.render(0)
    acc = r.readbackAccumulator()
    ref = host.sides(name)[0].render(0, lc.SPP)
    assert np.isfinite(ref).all() and ref[..., :3].max() > 0
    assert acc.tobytes() == ref.tobytes(), np.abs(acc - ref).max()
    # the probe leaves the render's state alone: the same accumulator after a batch of probes
    b = lc.batches(name)["lattice"]
    r.debugLights(b.fn, b.rec, **b.args)
    assert r.readbackAccumulator().tobytes() == ref.tobytes()
