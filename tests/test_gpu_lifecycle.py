"""Renderer lifetime on the GPU: pt_destroy gives back everything a renderer held (the BVH builder's kept scratch was once
freed by nothing).  Renderer::~Renderer (renderer_pt.hpp:34) releases its Metal objects through NS::SharedPtr; here every device array
is a DevBuf and the builder's scratch an LbvhScratch, whose destructors run when pt_destroy deletes the renderer; the acceleration
structure goes in pt_renderer::free_scene().  Also: what a restart keeps and releases, and the order of pt_start_render's refusals."""
import ctypes as C

import numpy as np
import pytest

from platinum_amd import Renderer, abi, scenes
from platinum_amd.renderer import make_params


@pytest.mark.gpu
def test_destroy_returns_all_device_memory_including_the_bvh_builder_scratch():
    import torch
    sc = scenes.field_scene(16)          # 259 k triangles: ~0.1 GB of builder scratch, ~70 MB of structure
    free = []
    for i in range(4):
        r = Renderer(device=0)
        r.startRender(sc, (256, 144), 4, max_bounces=4)
        r.render(0)
        r.readbackAccumulator()
        if i == 1:                       # a restart on the same renderer must not grow it either
            r.startRender(sc, (256, 144), 4, max_bounces=4)
            r.render(0)
            r.wait()
        r.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    # the first create may leave runtime-internal pools behind (code objects, signal pools); after that free memory must not drift
    assert abs(free[3] - free[1]) <= 8 << 20, [f / 2**20 for f in free]
    assert abs(free[2] - free[1]) <= 8 << 20, [f / 2**20 for f in free]


def _restart_sequence(r, sc):
    """full frame, a region that is not tile-aligned, adaptive sampling with the denoiser's AOVs, full frame again: the order in which the
    phases of pt_start_render keep and release the camera-ray lists, the tile lists, the checkpoint buffers and the AOV buffers."""
    size, spp, bounces = (64, 48), 4, 4
    built, frames = [], []

    def go():
        r.startRender(sc, size, spp, max_bounces=bounces)
        built.append(r.cameraListStats().built)
        r.render(0)
        frames.append(r.readbackAccumulator())

    go()
    r.setRenderRegion(5, 3, 29, 19)          # 24 x 16 pixels, no edge on a tile boundary
    go()
    r.clearRenderRegion()
    r.setAdaptiveOptions(enabled=1, min_spp=2, interval=1)
    r.setDenoiseOptions(enabled=1)
    go()
    r.setAdaptiveOptions(enabled=0)
    r.setDenoiseOptions(enabled=0)
    go()
    return built, frames


@pytest.mark.gpu
def test_restarts_through_region_adaptive_and_back_keep_and_release_the_right_things():
    import torch
    sc = scenes.cornell_scene("bench")
    warm = Renderer(device=0)                # (the first pass through every kernel may leave runtime-internal pools behind, as above)
    _restart_sequence(warm, sc)
    warm.close()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    r = Renderer(device=0)
    built, frames = _restart_sequence(r, sc)
    r.close()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info(0)[0]
    assert built == [1, 0, 0, 1]
    assert frames[3].tobytes() == frames[0].tobytes()
    assert np.isfinite(frames[0]).all() and frames[0][..., :3].max() > 0
    assert abs(after - before) <= 8 << 20, (before / 2**20, after / 2**20)


# params that are wrong in two ways: the refusal names the check that comes first (the single device and the group share the checks)
TWO_FAULTS = [
    (dict(spp=0, max_bounces=0), b"empty size or spp"),
    (dict(width=0, integrator=7), b"empty size or spp"),
    (dict(max_bounces=51, integrator=7), b"max_bounces must be 1..50"),
    (dict(max_bounces=0, width=1 << 15, height=1 << 15), b"max_bounces must be 1..50"),
    (dict(width=1 << 15, height=1 << 15, integrator=7), b"image too large"),
    (dict(integrator=7, nonfinite_policy=9), b"bad integrator"),
    (dict(nonfinite_policy=9, accel_structure=9), b"bad nonfinite_policy"),
    (dict(accel_structure=9, flags=abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON, gmon_buckets=33), b"bad accel_structure"),
]


def _refusal(r, snap, **fields):
    p = make_params(64, 48, 4, 4)
    for k, v in fields.items():
        setattr(p, k, v)
    rc = r._lib.pt_start_render(r._h, C.byref(snap.struct), C.byref(p))
    return rc, r._lib.pt_last_error()


@pytest.mark.gpu
def test_start_render_reports_the_first_failed_check_on_a_device_and_on_a_group():
    sc = scenes.cornell_scene("bench")
    snap = sc.snapshot()
    single, group = Renderer(device=0), Renderer(devices=[0, 0])
    try:
        for r in (single, group):
            for fields, message in TWO_FAULTS:
                rc, err = _refusal(r, snap, **fields)
                assert rc == -1 and message in err, (r is group, fields, err)
            assert r._lib.pt_start_render(r._h, C.byref(snap.struct), None) == -1 and b"null argument" in r._lib.pt_last_error()
        # the group's own check sits between the size and max_bounces (the stream is refused, never used)
        rc, err = _refusal(group, snap, stream=8, width=0)
        assert rc == -1 and b"empty size or spp" in err
        rc, err = _refusal(group, snap, stream=8, max_bounces=0)
        assert rc == -1 and b"caller stream" in err
        # the single device's own checks come after the shared ones
        single.setAdaptiveOptions(enabled=1)
        rc, err = _refusal(single, snap, integrator=7, flags=abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON, gmon_buckets=4)
        assert rc == -1 and b"bad integrator" in err
        rc, err = _refusal(single, snap, flags=abi.FLAG_MULTISCATTER_GGX | abi.FLAG_GMON, gmon_buckets=4)
        assert rc == -6 and b"adaptive sampling does not support PT_FLAG_GMON" in err
        single.setAdaptiveOptions(enabled=0)
        # nothing above left either renderer unable to render
        for r in (single, group):
            r.startRender(sc, (64, 48), 2, max_bounces=4)
            r.render(0)
            assert np.isfinite(r.readbackAccumulator()).all()
    finally:
        single.close()
        group.close()
