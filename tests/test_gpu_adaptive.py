"""GPU: tile-adaptive sampling (include/ptamd.h pt_adaptive_options, platinum_amd/csrc/adaptive.hip).
A tile that stopped after n samples equals a uniform render with spp = n on that tile, bit for bit (accumulator and AOVs), and the host
build of the criterion agrees with every verdict; paths count the work done; the result does not depend on the batching; degenerate
renders; the denoiser with per-pixel sample counts; refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_lib as al  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, BOUNCES, SPP = 128, 96, 4, 256
MIN_SPP = INTERVAL = 16
THRESHOLD = 0.1   # Cornell "bench" at 128x96: converged tiles at several checkpoints, the noisiest ones run to SPP
AOVS = (abi.AOV_ALBEDO, abi.AOV_NORMAL, abi.AOV_MOMENTS)


@pytest.fixture
def r(gpu_renderer):
    yield gpu_renderer
    o = abi.AdaptiveOptions()
    gpu_renderer._lib.pt_default_adaptive_options(C.byref(o))
    gpu_renderer.setAdaptiveOptions(o)
    d = abi.DenoiseOptions()
    gpu_renderer._lib.pt_default_denoise_options(C.byref(d))
    gpu_renderer.setDenoiseOptions(d)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _render(r, sc, spp, adaptive, aov=False, steps=None, threshold=THRESHOLD, w=W, h=H, **kw):
    r.setDenoiseOptions(enabled=1 if aov else 0)
    r.setAdaptiveOptions(enabled=1 if adaptive else 0, threshold=threshold, min_spp=MIN_SPP, interval=INTERVAL)
    r.startRender(sc, (w, h), spp, max_bounces=BOUNCES, **kw)
    if steps is None:
        r.render(0)
    else:
        while r.status() & abi.STATUS_DONE == 0:
            r.render(steps)
    r.wait()
    out = dict(acc=r.readbackAccumulator(), counts=r.readbackSampleCounts(), stats=r.stats())
    if aov:
        out["aov"] = [r.readbackAov(k) for k in AOVS]
    return out


def _tile_counts(counts):
    return counts[::8, ::8]


@pytest.fixture(scope="module")
def cornell():
    return scenes.cornell_scene("bench")


def test_tiles_equal_uniform_renders_of_their_count(r, cornell):
    ad = _render(r, cornell, SPP, True, aov=True)
    tc = _tile_counts(ad["counts"])
    distinct = sorted(set(tc.ravel().tolist()))
    assert len(distinct) >= 3 and distinct[-1] == SPP, distinct
    assert all(n >= MIN_SPP and (n == SPP or (n - MIN_SPP) % INTERVAL == 0) for n in distinct), distinct
    pix = np.kron(tc, np.ones((8, 8), np.uint32))[:H, :W]
    assert np.array_equal(pix, ad["counts"])
    checkpoints = list(range(MIN_SPP, SPP, INTERVAL))
    uniform = {}
    for n in sorted(set(checkpoints) | set(distinct)):
        uniform[n] = _render(r, cornell, n, False, aov=True)
    for n in distinct:
        sel = pix == n
        assert np.array_equal(_bits(ad["acc"][sel]), _bits(uniform[n]["acc"][sel])), n
        for k in range(3):
            assert np.array_equal(_bits(ad["aov"][k][sel]), _bits(uniform[n]["aov"][k][sel])), (n, k)
    # the host build of the criterion on the uniform renders' moments agrees with every verdict
    verdict = {c: al.host_tiles(uniform[c]["aov"][2], c, THRESHOLD) for c in checkpoints}
    for (ty, tx), n in np.ndenumerate(tc):
        for c in checkpoints:
            if c < n:
                assert not verdict[c][ty, tx], (ty, tx, n, c)
        if n < SPP:
            assert verdict[n][ty, tx], (ty, tx, n)


def test_paths_count_the_samples_taken(r, cornell):
    ad = _render(r, cornell, SPP, True)
    assert ad["stats"].paths == int(ad["counts"].astype(np.uint64).sum())
    assert ad["stats"].paths < SPP * W * H
    assert r.renderProgress() == (SPP, SPP) and r.status() & abi.STATUS_DONE


def test_result_does_not_depend_on_the_batching(r, cornell):
    runs = [_render(r, cornell, SPP, True), _render(r, cornell, SPP, True, samples_in_flight=8), _render(r, cornell, SPP, True, steps=5)]
    for k in (1, 2):
        assert np.array_equal(_bits(runs[0]["acc"]), _bits(runs[k]["acc"])), k
        assert np.array_equal(runs[0]["counts"], runs[k]["counts"]), k


def test_no_checkpoint_equals_the_uniform_render(r, cornell):
    for spp in (MIN_SPP - 3, MIN_SPP):
        ad = _render(r, cornell, spp, True, aov=True)
        un = _render(r, cornell, spp, False, aov=True)
        assert np.array_equal(_bits(ad["acc"]), _bits(un["acc"])), spp
        for k in range(3):
            assert np.array_equal(_bits(ad["aov"][k]), _bits(un["aov"][k])), (spp, k)
        assert (ad["counts"] == spp).all() and ad["stats"].paths == un["stats"].paths == spp * W * H


def _dark_box():
    sc = scenes.Scene(name="dark")
    box = sc.add_mesh(scenes.cornell_box())
    mats = scenes.cornell_materials()
    for m in mats:
        m.emission_strength = 0.0
    sc.add_instance(box, scenes.Transform(), mats)
    sc.set_camera(scenes.Camera.with_focal_length(28.0), scenes.Transform(translation=(0, 5, 15), target=(0, 5, 0), track=True))
    return sc


@pytest.mark.parametrize("steps", [None, 1])
def test_black_scene_converges_at_min_spp(r, steps):
    w, h, spp = 72, 40, 4096
    r.setAdaptiveOptions(enabled=1, threshold=THRESHOLD, min_spp=MIN_SPP, interval=INTERVAL)
    r.startRender(_dark_box(), (w, h), spp, max_bounces=BOUNCES)
    if steps is None:
        r.render(0)
    else:
        for _ in range(MIN_SPP):
            r.render(steps)
    r.wait()
    assert r.status() & abi.STATUS_DONE
    assert r.renderProgress() == (spp, spp)
    assert (r.readbackSampleCounts() == MIN_SPP).all()
    assert r.stats().paths == MIN_SPP * w * h
    assert not r.readbackAccumulator()[..., :3].any()


def test_denoised_uses_per_pixel_counts(r, cornell):
    ad = _render(r, cornell, SPP, True, aov=True)
    got = r.readbackDenoised()
    a, n, m = ad["aov"]
    want = al.host_filter_counts(ad["acc"], a, n, m, ad["counts"])
    assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(al.host_filter_counts(ad["acc"], a, n, m, np.full_like(ad["counts"], SPP))))


def test_non_adaptive_render_reports_uniform_counts(r, cornell):
    un = _render(r, cornell, 7, False)
    assert (un["counts"] == 7).all()


def test_refusals(r, cornell):
    r.setAdaptiveOptions(enabled=1)
    with pytest.raises(abi.PtamdError, match="error -6: .*GMON"):   # PT_ERR_UNSUPPORTED
        r.startRender(cornell, (32, 32), 64, max_bounces=BOUNCES, flags=abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON, gmonBuckets=4)
    g = Renderer(devices=[0, 0])
    try:
        o = g.adaptiveOptions()
        o.enabled = 1
        assert g._lib.pt_set_adaptive_options(g._h, C.byref(o)) == -6     # PT_ERR_UNSUPPORTED
        o.enabled = 0
        assert g._lib.pt_set_adaptive_options(g._h, C.byref(o)) == 0
    finally:
        g.close()
