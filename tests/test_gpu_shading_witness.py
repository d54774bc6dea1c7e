"""GPU: pt_debug_shading (include/ptamd.h, platinum_amd/csrc/shade_probe.hip) runs the stage between a hit record and the BSDF on the device
against a started render's scene.  The device must be the same bits as the host build of the same headers and as the oracle's twin, with
the 8-bit textures kept native and decoded, and is held directly to the float64 witness (shading_witness.py) under the bounds measured on
the oracle.  One-sample renders with AOVs hold the production path (the AOV kernel's shade_geometry on the render's own first hits) to
the probe's bits and to the witness: the shading normal on normal-mapped materials, the albedo on 8-bit textures.  Every scene is 48 x 32;
a probe batch holds at most 2^16 records."""
import ctypes as C

import numpy as np
import pytest

import geometry_witness as gw
import shading_cases as sc
import shading_witness as sw
import test_shading_witness_host as host
from platinum_amd import abi

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def r(gpu_renderer):
    before = gpu_renderer.selectedKernel()
    yield gpu_renderer
    gpu_renderer.selectKernel(before)
    gpu_renderer.setDenoiseOptions(enabled=0)


def start(r, name, native, monkeypatch, aov=False):
    r.setDenoiseOptions(enabled=1 if aov else 0)
    r.clearRenderRegion()
    r.selectKernel(abi.INTEGRATOR_MIS)
    monkeypatch.setenv("PTAMD_TEX_NATIVE", "1" if native else "0")
    r.startRender(sc.scene(name), sc.SIZE, sc.SPP, workingSpace=sc.WORKING_SPACE, max_bounces=sc.BOUNCES)
    monkeypatch.delenv("PTAMD_TEX_NATIVE")


def same_constants(r, name):
    c, oc = r.constants(), host.oracle(name).constants()
    assert (bytes(c.idt), bytes(c.camera)) == (bytes(oc.idt), bytes(oc.camera))


@pytest.mark.parametrize("native", [False, True], ids=["decoded", "native"])
@pytest.mark.parametrize("name", sc.WITNESSED)
def test_device_equals_host_build_and_oracle_and_meets_the_witness_bounds(r, name, native, monkeypatch):
    start(r, name, native, monkeypatch)
    same_constants(r, name)
    e = host.emu(name, native, monkeypatch)
    classes = {cls: host.records(name, cls) for cls in sc.batches(name)}
    hits = r.tracePrimary(0)
    classes["device hits"] = sc.hit_records(r.constants(), hits, 0)
    assert len(classes["device hits"]) > 100
    W = sc.witness(name, r.constants())
    for cls, rec in classes.items():
        d, h = r.debugShading(rec), e.debugShading(rec)
        assert host.same_bits(d, h), ("device / host build", cls, host.first_difference(d, h))
        if cls in sc.batches(name):
            assert host.same_bits(h, host.oracle_out(name, cls)), ("host build / oracle", cls)
        sw.assert_report(sw.check(W.answer(rec), d), "%s %s %s, device" % (name, cls, "native" if native else "decoded"))


@pytest.mark.parametrize("native", [False, True], ids=["decoded", "native"])
def test_device_edges_equal_the_host_build_and_have_the_class_float64_predicts(r, native, monkeypatch):
    """The edges class: bits (two NaNs of one field count as equal: 0 / 0 has the other sign on the device), admissibility and the finite /
    inf / NaN class.  The huge UVs must give finite texels inside their textures' ranges, and the host's bits."""
    start(r, "edges", native, monkeypatch)
    e = host.emu("edges", native, monkeypatch)
    W = sc.witness("edges", r.constants())
    for cls, rec in sc.edge_batches().items():
        d, h = r.debugShading(rec), e.debugShading(rec)
        sw.assert_report(sw.check(W.answer(rec), d, edge=True), "edges %s, device" % cls, edge=True)
        if cls == "huge_uv":
            host.check_huge_uv(d, gw.idt_of(r.constants()))
            differ = np.flatnonzero((host.words(d) != host.words(h)).any(1))
            print("huge UVs: %d of %d records differ between device and host build: %s" % (differ.size, len(rec), [sc.scene("edges").huge_uvs[p] for p in np.unique(rec["primitive"][differ])]))
        assert host.same_bits(d, h, nan_payload=True), ("device / host build", cls, host.first_difference(d, h))


@pytest.mark.parametrize("n", sc.grid_sizes())
def test_probe_sizes(r, n, monkeypatch):
    """one record, one below / at / above a block, and the largest batch of the suite (the grid-stride tail): every record is written"""
    start(r, "normalmaps", True, monkeypatch)
    e = host.emu("normalmaps", True, monkeypatch)
    rec = np.resize(np.concatenate(list(sc.batches("normalmaps").values())), n)
    d = r.debugShading(rec)
    assert len(d) == n and host.same_bits(d, e.debugShading(rec))


def test_debug_shading_refusals(r, monkeypatch):
    lib = r._lib
    rec = sc.batches("frames")["outside"][:4].copy()
    out = np.zeros((4, abi.PT_SHADE_PROBE_OUT_WORDS), np.uint32)
    pi, po = rec.ctypes.data, out.ctypes.data
    from platinum_amd import Renderer
    fresh = Renderer(device=0)
    try:
        assert lib.pt_debug_shading(fresh._h, 4, pi, po) == -5 and b"before pt_start_render" in lib.pt_last_error()
    finally:
        fresh.close()
    start(r, "frames", False, monkeypatch)
    for a in ((0, pi, po), ((1 << 24) + 1, pi, po), (4, None, po), (4, pi, None)):
        assert lib.pt_debug_shading(r._h, *a) == -1, a
    assert lib.pt_debug_shading(r._h, 4, pi, po) == 0 and out.any()
    for field, value in (("instance", len(sc.scene("frames").nodes)), ("primitive", 2), ("instance", 0xffffffff), ("primitive", 0xffffffff)):
        bad = rec.copy()
        bad[field][2] = value
        out[:] = 0
        assert lib.pt_debug_shading(r._h, 4, bad.ctypes.data, po) == -1 and b"names no triangle" in lib.pt_last_error(), (field, value)
        assert not out.any()                                   # refused on the host: nothing was launched, nothing written


# ---- the production path ----------------------------------------------------------------------------------------------------------------------
def render_aovs(r, name, native, monkeypatch):
    """a one-sample render with AOVs, the device's own first hits of sample 0 as probe records, and the probe's answer to them"""
    start(r, name, native, monkeypatch, aov=True)
    r.render(0)
    r.wait()
    albedo, normal, moments = (r.readbackAov(k).reshape(-1, 4) for k in (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS))
    hits = r.tracePrimary(0).reshape(-1)
    px = np.flatnonzero(hits["instance"] >= 0)
    rec = sc.hit_records(r.constants(), hits, 0)
    probe = r.debugShading(rec)
    r.setDenoiseOptions(enabled=0)
    assert px.size > 100 and np.all(normal[px, 3] == 1.0) and np.all(normal[np.setdiff1d(np.arange(len(hits)), px), 3] == 0.0)
    assert np.array_equal(moments[px, 0], hits["t"][px])         # the render shaded the very hits pt_trace_primary reports
    return albedo[px], normal[px], rec, probe


@pytest.mark.parametrize("native", [False, True], ids=["decoded", "native"])
def test_the_normal_aov_of_normal_mapped_materials_meets_the_witness(r, native, monkeypatch):
    albedo, normal, rec, probe = render_aovs(r, "normalmaps", native, monkeypatch)
    assert np.array_equal(normal[:, :3].view(np.uint32), probe["z"].view(np.uint32)) and np.array_equal(albedo[:, :3].view(np.uint32), probe["albedo"].view(np.uint32))
    A = sc.witness("normalmaps", r.constants()).answer(rec)
    assert A.mapped.all()
    keep = A.N_len >= sw.N_MIN
    ez = (np.abs(normal[None, :, :3].astype(F64) - A.frames[:, :, 2]).max(-1) / A.scale)
    ez = np.where(A.valid, ez, np.inf).min(0)
    ea = (np.abs(albedo[:, :3].astype(F64) - A.albedo) / np.maximum(np.abs(A.albedo), 1.0)).max(-1)
    print("normal AOV %.3e over %d hits (|N| %.3g .. %.3g), albedo AOV %.3e" % (ez[keep].max(), keep.sum(), A.N_len.min(), A.N_len.max(), ea.max()))
    assert keep.sum() > 100 and ez[keep].max() <= sw.BOUNDS["frame_mapped"] and ea.max() <= sw.BOUNDS["albedo"]


@pytest.mark.parametrize("native", [False, True], ids=["decoded", "native"])
def test_the_albedo_aov_of_eight_bit_textures_meets_the_witness(r, native, monkeypatch):
    albedo, normal, rec, probe = render_aovs(r, "slots", native, monkeypatch)
    assert np.array_equal(albedo[:, :3].view(np.uint32), probe["albedo"].view(np.uint32)) and np.array_equal(normal[:, :3].view(np.uint32), probe["z"].view(np.uint32))
    A = sc.witness("slots", r.constants()).answer(rec)
    s = sc.scene("slots")
    eight = np.array([m.base_texture >= 0 and s.textures[m.base_texture].format != abi.TEX_RGBA32F for m in A.mats])
    formats = {s.textures[m.base_texture].format for m in A.mats[eight]}
    assert formats == {abi.TEX_RGBA8_SRGB, abi.TEX_RGBA8, abi.TEX_RG8, abi.TEX_R8}
    ea = (np.abs(albedo[:, :3].astype(F64) - A.albedo) / np.maximum(np.abs(A.albedo), 1.0)).max(-1)
    ez = np.abs(normal[:, :3].astype(F64) - A.frame[:, 2]).max(-1)
    print("albedo AOV %.3e over %d hits on 8-bit base textures (%.3e over all %d), normal AOV %.3e" % (ea[eight].max(), eight.sum(), ea.max(), len(ea), ez.max()))
    assert eight.sum() >= 20 and ea.max() <= sw.BOUNDS["albedo"] and ez.max() <= sw.BOUNDS["frame"]


def test_the_probe_leaves_the_render_alone(r, monkeypatch):
    start(r, "slots", True, monkeypatch)
    r.render(0)
    r.wait()
    acc = r.readbackAccumulator().tobytes()
    r.debugShading(sc.batches("slots")["lattice"])
    assert r.readbackAccumulator().tobytes() == acc
