"""GPU: the display chain as a whole (platinum_amd/csrc/display.hip): source (accumulator, denoised image or a group's merged
image), then auto exposure, then bloom, then the post-process into the RGBA8 target.  test_gpu_exposure.py, test_gpu_bloom.py and
test_gpu_denoise.py hold the stages pairwise; here every on/off combination of the three is held at once against a host-built image, read
and presented, on one device and on a device group, and a present ahead of an adaptive render's checkpoints is shown to leave the
result alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bloom_lib as bl  # noqa: E402
from platinum_amd import abi, scenes  # noqa: E402
from platinum_amd.renderer import Renderer  # noqa: E402
from test_gpu_bloom import ON, SIZE, SPP, _bits, _oracle_target, _present, _render, _restore, _scaled  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def r(gpu_renderer):
    _restore(gpu_renderer)
    yield gpu_renderer
    gpu_renderer.setAdaptiveOptions(enabled=0)
    _restore(gpu_renderer)      # the session's renderer goes on with every stage disabled


def _expected(r, sc, src, exposure, bloom):
    """The oracle's post-process of what the chain shows of `src`: scaled by the meter's gain, then bloomed on the host."""
    img = src
    if exposure:
        img = _scaled(img, r.readbackExposureMeter().gain)
    if bloom:
        img = bl.host_bloom(img, r.bloomOptions())
    return _oracle_target(sc, SIZE, img, r.postProcessOptions(), r.tonemapOptions())


def _assert_read_and_presented(r, want, what):
    got = r.readbackRenderTarget()
    bad = (got != want).any(axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first (y, x) %s: device %s, oracle %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:2].tolist(), want[bad][:2].tolist())
    assert np.array_equal(_present(r), want), what + ", presented"


@pytest.mark.parametrize("bloom", [0, 1])
@pytest.mark.parametrize("exposure", [0, 1])
@pytest.mark.parametrize("apply_to_target", [0, 1])
def test_every_combination_of_the_stages(r, apply_to_target, exposure, bloom):
    sc = scenes.cornell_scene("bench")
    r.setDenoiseOptions(enabled=1, apply_to_target=apply_to_target)      # AOVs exist in every case; smoothing stays 0: reads are independent
    _render(r, sc)
    acc, den = r.readbackAccumulator(), r.readbackDenoised()
    assert not np.array_equal(_bits(den), _bits(acc))
    r.setExposureOptions(enabled=exposure)
    r.setBloomOptions(**dict(ON, enabled=bloom))
    want = _expected(r, sc, den if apply_to_target else acc, exposure, bloom)
    _assert_read_and_presented(r, want, "apply_to_target %d, exposure %d, bloom %d" % (apply_to_target, exposure, bloom))
    assert np.array_equal(_bits(r.readbackAccumulator()), _bits(acc)) and np.array_equal(_bits(r.readbackDenoised()), _bits(den))


def test_device_group_shows_the_merged_image_through_the_whole_chain():
    sc = scenes.cornell_scene("bench")
    g = Renderer(devices=[0, 0])
    try:
        _render(g, sc)
        acc = g.readbackAccumulator()
        g.setExposureOptions(enabled=1)
        g.setBloomOptions(**ON)
        assert g.readbackExposureMeter().gain != 1.0
        _assert_read_and_presented(g, _expected(g, sc, acc, 1, 1), "group")
        assert np.array_equal(_bits(g.readbackAccumulator()), _bits(acc))
    finally:
        g.close()


def test_present_does_not_wait_for_checkpoints(r):
    """A present enqueues behind whatever is accepted and returns: it neither waits for an adaptive render's checkpoints nor disturbs them.
    (No assertion about timing: only that it succeeds, shows an image of the frame's size, and that the finished render is the one a
    render without the present gives.)"""
    sc, spp = scenes.cornell_scene("bench"), 48
    r.setAdaptiveOptions(enabled=1, threshold=0.1, min_spp=16, interval=16)      # checkpoints after 16 and 32 samples

    def start():
        r.startRender(sc, SIZE, spp, max_bounces=4)
        while r.status() & abi.STATUS_DONE == 0:
            r.render(5)

    start()
    r.wait()
    base = r.readbackAccumulator()
    start()
    presented = _present(r)      # no wait() ahead of it
    assert presented.shape == (SIZE[1], SIZE[0], 4) and presented.dtype == np.uint8
    r.wait()
    acc = r.readbackAccumulator()
    assert np.array_equal(_bits(acc), _bits(base))
    want = _oracle_target(sc, SIZE, acc, r.postProcessOptions(), r.tonemapOptions())
    assert np.array_equal(r.readbackRenderTarget(), want)
