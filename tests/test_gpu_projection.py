"""GPU: the camera projections (include/ptamd.h pt_camera_projection) on the device.

1. Ray bits: pt_debug_camera_rays — the render's own ray-generation kernel — equals the host build of pt_projection.h bit for bit under
   every kind (PERSPECTIVE, thin lens and pinhole, against stage_raygen), at 1x1, 5x3, 8x8, 50x35 (partial tiles both ways) and 64x32.
2. First hits: pt_trace_primary against the float64 projection witness (projection_witness.py) under the rule and bounds of the host test,
   on the 6-wide, 4-wide, two-level and radix-tree structures.
3. Renders under each new kind: first-hit AOVs against the witness, the film's coverage and pt_pick against its decided answers; N samples as
   one batch equal N batches of one; an adaptive render whose tiles all stay active and a region render against the uniform full frame; no
   camera-ray leaf lists; and PERSPECTIVE set explicitly is a renderer that never heard of projections.
4. The light-probe bake: default EQUIRECT at the environment's resolution is the environment, pixel for texel.
Each test prints its figures before it asserts (pytest -s shows them)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_cases as gc  # noqa: E402
import geometry_witness as gw  # noqa: E402
import projection_lib as pl  # noqa: E402
import projection_witness as pw  # noqa: E402
from conftest import skip_if_structure_env_preset  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer, make_params  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, BAD_STATE, UNSUPPORTED = -1, -5, -6
RAY_SIZES = ((1, 1), (5, 3), (8, 8), (50, 35), (64, 32))
LABELS = ("ortho", "equirect", "fisheye_pi", "fisheye_2pi")
AOVS = (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)
RENDER_SCENE, RENDER_SIZE = "truth", (50, 35)     # instanced, opaque, untextured: every AOV of the witness applies
LIT_SCENE = "cornell_sphere"                      # ... but unlit; the radiance comparisons render the box with its lamp and the glass sphere


@pytest.fixture(scope="module")
def rr():
    r = Renderer(device=0)
    yield r
    r.close()


def _defaults(r):
    r.setProjection(pl.projection(abi.PROJ_PERSPECTIVE))
    r.setDenoiseOptions(enabled=0)
    r.setMatteOptions(enabled=0)
    r.setFilmOptions(enabled=0)
    r.setAdaptiveOptions(enabled=0)
    r.clearRenderRegion()
    r.selectKernel(abi.INTEGRATOR_MIS)


@pytest.fixture
def r(rr):
    _defaults(rr)
    yield rr
    _defaults(rr)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. ray bits -----------------------------------------------------------------------------------------------------------------------------
def _sweep():
    yield "perspective pinhole", pl.projection(abi.PROJ_PERSPECTIVE), 0.0
    yield "perspective thin lens", pl.projection(abi.PROJ_PERSPECTIVE), 2.8
    for label, proj in pl.sweep_projections():
        yield label, proj, 0.0
    yield "equirect, aperture ignored", pl.projection(abi.PROJ_EQUIRECT), 2.8


@pytest.mark.parametrize("size", RAY_SIZES, ids=lambda s: "%dx%d" % s)
def test_camera_rays_are_the_host_builds_bit_for_bit(r, size):
    W, H = size
    for label, proj, aperture in _sweep():
        sc = scenes.cornell_scene("bench")
        sc.camera_world = pl.sweep_cameras()["scaled"]
        sc.camera.aperture = aperture
        r.setProjection(proj)
        r.startRender(sc, size, 4, max_bounces=1)
        got = r.renderProjection()
        assert bytes(got) == bytes(proj)
        host = pl.HostProjection(sc, make_params(W, H, 4, 1), proj)
        for s in (0, 977):
            o, d = r.debugCameraRays(s)
            ho, hd, _, _ = host.rays(s)
            assert _same_bits(o, ho) and _same_bits(d, hd), (label, size, s, np.abs(o - ho).max(), np.abs(d - hd).max())
        assert r.cameraListStats().built == 0 or proj.kind == abi.PROJ_PERSPECTIVE


def test_camera_rays_before_a_render_and_null_outputs(r):
    fresh = Renderer(device=0)
    try:
        out = np.zeros(3, np.float32)
        assert fresh._lib.pt_debug_camera_rays(fresh._h, 0, out.ctypes.data, out.ctypes.data) == BAD_STATE
        assert fresh._lib.pt_get_camera_projection(fresh._h, C.byref(abi.CameraProjection())) == BAD_STATE
    finally:
        fresh.close()
    r.setProjection(pl.projection(abi.PROJ_FISHEYE))
    r.startRender(scenes.cornell_scene("bench"), (5, 3), 1, max_bounces=1)
    o, d = r.debugCameraRays(0)
    d2 = np.zeros_like(d)
    assert r._lib.pt_debug_camera_rays(r._h, 0, None, d2.ctypes.data) == 0 and _same_bits(d, d2)
    assert r._lib.pt_debug_camera_rays(r._h, 0, None, None) == 0
    # the projection is read at pt_start_render: setting another one leaves the current render's alone
    r.setProjection(pl.projection(abi.PROJ_EQUIRECT))
    assert r.renderProjection().kind == abi.PROJ_FISHEYE and _same_bits(r.debugCameraRays(0)[1], d)
    # ... and what is refused leaves the held options alone
    assert r._lib.pt_set_camera_projection(r._h, C.byref(pl.projection(abi.PROJ_FISHEYE, fisheye_fov=7.0))) == INVALID
    r.startRender(scenes.cornell_scene("bench"), (5, 3), 1, max_bounces=1)
    assert r.renderProjection().kind == abi.PROJ_EQUIRECT


# ---- 2. first hits ---------------------------------------------------------------------------------------------------------------------------
def _start(r, name, label, size, spp=1, bounces=1, **kw):
    r.setProjection(pl.witness_projections(name)[label])
    r.startRender(pl.witness_scene(name), size, spp, max_bounces=bounces, **kw)


def _check_trace(r, name, label, size, what):
    w, D, E_o = pl.witness(name, label, size[0], size[1], 0)
    what = "%s %s %dx%d, %s" % (name, label, size[0], size[1], what)
    pw.check_conditions(w, what)                       # (properties of the witness, not of the device)
    pw.check_hits(w, r.tracePrimary(0), what, D, E_o)
    return w


@pytest.mark.parametrize("label", LABELS)
@pytest.mark.parametrize("name", pl.WITNESS_SCENES)
def test_first_hits_on_the_default_structure(r, name, label):
    for size in pl.WITNESS_SIZES:
        _start(r, name, label, size)
        assert r.cameraListStats().built == 0
        _check_trace(r, name, label, size, "default structure")


STRUCTURE_CASES = [(n, l) for n in ("cornell_sphere", "random8") for l in LABELS]


@pytest.mark.parametrize("name,label", STRUCTURE_CASES)
def test_first_hits_on_the_four_wide_form(r, name, label, monkeypatch):
    skip_if_structure_env_preset()
    monkeypatch.setenv("PTAMD_BVH4", "1")
    _start(r, name, label, pl.WITNESS_SIZES[0])
    monkeypatch.delenv("PTAMD_BVH4")
    _check_trace(r, name, label, pl.WITNESS_SIZES[0], "4-wide")


@pytest.mark.parametrize("name,label", STRUCTURE_CASES)
def test_first_hits_on_the_two_level_structure(r, name, label):
    _start(r, name, label, pl.WITNESS_SIZES[0], accel_structure=abi.ACCEL_TWO_LEVEL)
    assert r.stats().accel_two_level == 1
    _check_trace(r, name, label, pl.WITNESS_SIZES[0], "two-level")


@pytest.mark.parametrize("name,label", STRUCTURE_CASES)
def test_first_hits_on_the_radix_tree(r, name, label, monkeypatch):
    skip_if_structure_env_preset()
    monkeypatch.setenv("PTAMD_RADIX_TREE", "1")
    _start(r, name, label, pl.WITNESS_SIZES[0])
    monkeypatch.delenv("PTAMD_RADIX_TREE")
    _check_trace(r, name, label, pl.WITNESS_SIZES[0], "radix tree")


# ---- 3. renders ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", LABELS)
def test_a_one_sample_render_shows_the_witnesss_first_hits(r, label):
    name, (W, H) = RENDER_SCENE, RENDER_SIZE
    r.setDenoiseOptions(enabled=1)
    r.setMatteOptions(enabled=1)
    r.setFilmOptions(enabled=1)
    _start(r, name, label, (W, H))
    assert r.cameraListStats().built == 0
    r.render(0)
    r.wait()
    albedo, normal, moments = (r.readbackAov(k).reshape(-1, 4) for k in AOVS)
    film = r.readbackFilm().reshape(-1, 4)
    w, D, E_o = pl.witness(name, label, W, H, 0)
    w.idt = gw.idt_of(r.constants())
    what = "%s %s %dx%d render" % (name, label, W, H)
    hit = normal[:, 3]
    assert np.all((hit == 0.0) | (hit == 1.0))
    shown_miss, shown_hit = np.flatnonzero(hit == 0.0), np.flatnonzero(hit == 1.0)
    assert not (~w.allow_miss[shown_miss]).any(), what
    assert not (w.n_hits[shown_hit] == 0).any(), what
    # the film's coverage is the witness's decided hit flag
    assert np.array_equal(film[w.decided, 3], w.decided_hit[w.decided].astype(np.float32))
    rays = np.flatnonzero(w.decided_hit)
    assert rays.size and np.all(hit[rays] == 1.0)
    # AOVs on ALL the decided hits under geometry_witness's bounds (depth under ORTHOGRAPHIC with its origin term: projection_witness)
    pw.check_aovs(w, rays, w.k[rays], albedo[rays], normal[rays], moments[rays, 0], what, E_o)
    # pt_pick names the witness's instance (a 1-sample render: the pixel's one hit)
    picked = 0
    for ray in np.flatnonzero(w.decided)[:: max(1, W * H // 97)]:
        got = r.pick(int(ray % W), int(ray // W))
        want = abi.MATTE_NONE if w.k[ray] < 0 else int(w.T.inst[w.k[ray]])
        assert got.instance == want and got.samples == 1, (what, ray, got.instance, want)
        picked += 1
    assert picked >= 90


def _outputs(r):
    out = [r.readbackAccumulator()] + [r.readbackAov(k) for k in AOVS] + [r.readbackFilm()]
    slots = [r.readbackMatteSlots(layer) for layer in (abi.MATTE_INSTANCE, abi.MATTE_MATERIAL)]
    return out, slots, r.readbackSampleCounts()


def _full_render(r, label, size, spp, steps=(0,), sif=0, region=None, adaptive=None, bounces=3):
    r.setDenoiseOptions(enabled=1)
    r.setMatteOptions(enabled=1)
    r.setFilmOptions(enabled=1)
    if region:
        r.setRenderRegion(*region)
    else:
        r.clearRenderRegion()
    if adaptive:
        r.setAdaptiveOptions(enabled=1, min_spp=adaptive[0], interval=adaptive[1], threshold=adaptive[2])
    else:
        r.setAdaptiveOptions(enabled=0)
    _start(r, LIT_SCENE, label, size, spp=spp, bounces=bounces, samples_in_flight=sif)
    assert r.cameraListStats().built == 0
    for n in steps:
        r.render(n)
        r.wait()
    return _outputs(r)


def _assert_same(a, b, what, mask=None):
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        if mask is not None:
            x, y = x[mask], y[mask]
        assert np.any(x[..., :3] != 0) and _same_bits(x, y), (what, "image", k)
    for k, (x, y) in enumerate(zip(a[1], b[1])):
        if mask is not None:
            x, y = x[mask], y[mask]
        assert _same_bits(x, y), (what, "matte layer", k)


@pytest.mark.parametrize("label", LABELS)
def test_one_batch_of_n_equals_n_batches_of_one(r, label):
    N, size = 7, RENDER_SIZE
    one = _full_render(r, label, size, N, sif=N)                 # 7 in flight: no multiple of 64, nor of 8
    assert r.stats().batches == 1 and r.stats().samples_in_flight == N
    many = _full_render(r, label, size, N, steps=(1,) * N)
    assert r.stats().batches == N
    _assert_same(one, many, label)
    split = _full_render(r, label, size, N, sif=5)               # 5 + 2
    assert r.stats().batches == 2
    _assert_same(one, split, label)


@pytest.mark.parametrize("label", LABELS)
def test_adaptive_with_every_tile_active_and_a_region_hold_the_uniform_bits(r, label):
    N, size = 6, RENDER_SIZE
    W, H = size
    uniform = _full_render(r, label, size, N, sif=5)
    # min_spp = spp: no checkpoint comes before the render ends, so every tile stays active through every batch — the virtual-tile kernels
    # over the whole frame (a camera inside the box sees unlit texels too, which any threshold would retire)
    adaptive = _full_render(r, label, size, N, sif=5, adaptive=(N, 2, 0.05))
    assert np.all(adaptive[2] == N), np.unique(adaptive[2])
    _assert_same(uniform, adaptive, label + " adaptive")
    rect = (5, 3, 43, 30)                                        # not aligned to 8
    region = _full_render(r, label, size, N, sif=5, region=rect)
    inside = np.zeros((H, W), bool)
    inside[rect[1]:rect[3], rect[0]:rect[2]] = True
    _assert_same(uniform, region, label + " region", mask=inside)
    for img in region[0]:
        assert not img[~inside].any()
    assert np.all(region[2][inside] == N) and not region[2][~inside].any()


def test_perspective_set_explicitly_is_a_renderer_that_never_heard_of_projections(r):
    sc, size, N = scenes.cornell_sphere_scene(), (50, 35), 6
    results = []
    fresh = Renderer(device=0)
    try:
        for x, explicit in ((fresh, False), (r, True)):
            if explicit:
                x.setProjection(pl.projection(abi.PROJ_FISHEYE))            # ... even after a projected render
                x.startRender(sc, size, 1, max_bounces=1)
                x.setProjection(pl.projection(abi.PROJ_PERSPECTIVE, ortho_height=3.0, fov_x=1.0, fov_y=1.0, fisheye_fov=1.0))
            x.setDenoiseOptions(enabled=1)
            x.setMatteOptions(enabled=1)
            x.setFilmOptions(enabled=1)
            x.startRender(sc, size, N, max_bounces=4, samples_in_flight=5)
            lists = x.cameraListStats()
            x.render(0)
            x.wait()
            st = x.stats()
            results.append((_outputs(x), (st.closest_rays, st.shadow_rays, st.shaded_hits, st.paths, st.batches), lists.built, lists.pixels_listed,
                            x.tracePrimary(3), x.debugCameraRays(3)))
    finally:
        fresh.close()
    a, b = results
    _assert_same(a[0], b[0], "perspective")
    assert a[1] == b[1] and a[2] == b[2] and a[3] == b[3]
    if "PTAMD_NO_CAMERA_LISTS" not in os.environ and not any(v in os.environ for v in ("PTAMD_BVH4", "PTAMD_RADIX_TREE", "PTAMD_TWO_LEVEL")):
        assert a[2] == 1                                                     # lists built as ever
    assert _same_bits(a[4], b[4]) and _same_bits(a[5][0], b[5][0]) and _same_bits(a[5][1], b[5][1])


def test_a_device_group_refuses_every_kind_but_perspective():
    g = Renderer(devices=[0, 0])
    try:
        for kind in (abi.PROJ_ORTHOGRAPHIC, abi.PROJ_EQUIRECT, abi.PROJ_FISHEYE):
            assert g._lib.pt_set_camera_projection(g._h, C.byref(pl.projection(kind))) == UNSUPPORTED
        assert g._lib.pt_set_camera_projection(g._h, C.byref(pl.projection(abi.PROJ_PERSPECTIVE))) == 0
        assert g._lib.pt_set_camera_projection(g._h, C.byref(pl.projection(abi.PROJ_EQUIRECT, fov_x=-1.0))) == INVALID    # checked first
        assert g._lib.pt_set_camera_projection(g._h, C.byref(pl.projection(9))) == INVALID
        assert g._lib.pt_get_camera_projection(g._h, C.byref(abi.CameraProjection())) == BAD_STATE
    finally:
        g.close()


# ---- 4. the light-probe bake -----------------------------------------------------------------------------------------------------------------
def test_probe_bake_is_the_environment_pixel_for_texel(r):
    sc = pl.probe_scene()
    env = sc.textures[sc.env_texture].pixels
    H, W = env.shape[:2]
    r.setProjection(pl.projection(abi.PROJ_EQUIRECT))
    for s in (0, 977):
        r.startRender(sc, (W, H), 1, max_bounces=3, first_sample=s)
        miss = r.tracePrimary(s)["instance"] < 0
        r.render(0)
        r.wait()
        pl.check_probe(env, r.readbackAccumulator(), miss, s, "device, sample %d" % s)
