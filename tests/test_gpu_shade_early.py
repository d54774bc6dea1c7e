"""k_shade issues the energy-table taps of a hit early and waits for them once (pt_shade.h shade_issue / shade_land): the order of the loads
changes, no value does.  Small renders against the CPU oracle, bit for bit — the whole accumulator and the ray / shadow / hit counters —
over every material class, mixed passes at the end of a segment, a scene without lights (NEE skipped, its dimensions still consumed) and
light hits after the first bounce (the MIS branch that re-reads the queue).

All renders are 32x32 pixels, 8 bounces, MIS; batches of 1, 5 and 70 samples: a pass with one lane per segment slot, a partly filled
pass, and bins that fill and are refilled within a segment."""
import functools

import numpy as np
import pytest

from platinum_amd import abi, scenes
from platinum_amd.renderer import make_params

import oracle_lib

pytestmark = pytest.mark.gpu

W = H = 32
BOUNCES = 8
BATCHES = (1, 5, 70)


def _four_classes(emissive=True):
    """Cornell box with the GGX glass sphere (class 2) plus a metallic (1), a clearcoat (3) and a roughness-0 dielectric (0, smooth GGX)
    sphere; the walls are class 0 with roughness 1.  emissive=False: the ceiling light is a plain white panel — a scene without lights."""
    sc = scenes.Scene(name="four_classes")
    mats = scenes.cornell_materials()
    if not emissive:
        mats[3] = scenes.Material(name="panel", base_color=(1, 1, 1, 1))
    sc.add_instance(sc.add_mesh(scenes.cornell_box()), scenes.Transform(), mats)
    big = sc.add_mesh(scenes.sphere(1.0, 12, 16))
    sc.add_instance(big, scenes.Transform(translation=(0.5, 2.0, 0.0), scale=(2, 2, 2)),
                    [scenes.Material(name="glass", base_color=(1, 1, 1, 1), roughness=0.3, ior=1.5, transmission=1.0)])
    sc.add_instance(big, scenes.Transform(translation=(-3.0, 1.2, 1.5), scale=(1.2, 1.2, 1.2)),
                    [scenes.Material(name="metal", base_color=(0.9, 0.7, 0.3, 1), roughness=0.35, metallic=1.0)])
    sc.add_instance(big, scenes.Transform(translation=(3.2, 1.0, 2.0)),
                    [scenes.Material(name="coated", base_color=(0.2, 0.3, 0.8, 1), roughness=0.6, clearcoat=0.8, clearcoat_roughness=0.1)])
    sc.add_instance(big, scenes.Transform(translation=(-1.5, 6.5, -1.0)),
                    [scenes.Material(name="polished", base_color=(0.8, 0.8, 0.8, 1), roughness=0.0, ior=1.5)])
    sc.set_camera(scenes.Camera.with_focal_length(28.0), scenes.Transform(translation=(0, 5, 15), target=(0, 5, 0), track=True))
    return sc


def _emissive_box():
    """The camera inside a closed box whose every wall emits and reflects: a path meets a light at every bounce."""
    sc = scenes.Scene(name="emissive_box")
    glow = [scenes.Material(name="glow%d" % i, base_color=c, emission=(1, 1, 1), emission_strength=s)
            for i, (c, s) in enumerate([((0.8, 0.8, 0.8, 1), 0.5), ((0.7, 0.2, 0.2, 1), 1.0), ((0.2, 0.6, 0.2, 1), 2.0), ((0.5, 0.5, 0.5, 1), 8.0)])]
    sc.add_instance(sc.add_mesh(scenes.cornell_box()), scenes.Transform(), glow)
    sc.add_instance(sc.add_mesh(scenes.plane(10.0)), scenes.Transform(translation=(0, 5, 5), rotation=(-np.pi / 2, 0, 0)),
                    [scenes.Material(name="front", base_color=(0.6, 0.6, 0.9, 1), emission=(1, 1, 1), emission_strength=1.5, roughness=0.4)])
    sc.set_camera(scenes.Camera.with_focal_length(20.0), scenes.Transform(translation=(0, 5, 4.5), target=(0, 4, 0), track=True))
    return sc


SCENES = {
    "four_classes": _four_classes,
    "field4": lambda: scenes.field_scene(grid=4),
    "four_classes_no_light": lambda: _four_classes(emissive=False),
    "emissive_box": _emissive_box,
}


@functools.lru_cache(maxsize=None)
def _reference(name, spp):
    """The oracle's accumulator and counters, computed once per case."""
    sc = SCENES[name]()
    p = make_params(W, H, spp, BOUNCES, flags=abi.FLAG_MULTISCATTER_GGX, integrator=abi.INTEGRATOR_MIS, working_space=scenes.BT2020)
    o = oracle_lib.OracleScene(sc, p)
    acc = o.render(0, spp)
    acc.setflags(write=False)
    so = o.stats()
    return acc, (so.closest_rays, so.shadow_rays, so.shaded_hits, so.paths)


def _same_bits_or_both_nan(a, b):
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


@pytest.mark.parametrize("spp", BATCHES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_accumulator_and_counters_are_the_oracles(gpu_renderer, name, spp):
    ref, counts = _reference(name, spp)
    r = gpu_renderer
    r.selectKernel(abi.INTEGRATOR_MIS)
    r.startRender(SCENES[name](), (W, H), spp, workingSpace=scenes.BT2020, max_bounces=BOUNCES, samples_in_flight=spp)
    while r.status() & abi.STATUS_BUSY:
        r.render(0)
    acc = r.readbackAccumulator()
    st = r.stats()
    got = (st.closest_rays, st.shadow_rays, st.shaded_hits, st.paths)
    print(name, spp, "counters", got, "oracle", counts, "differing values", int((acc.view(np.uint32) != ref.view(np.uint32)).sum()))
    assert st.batches == 1 and got == counts
    assert _same_bits_or_both_nan(acc, ref)
    # what each scene is there for
    if name == "four_classes_no_light":
        assert st.shadow_rays == 0 and not acc[..., :3].any()
    else:
        assert st.shadow_rays > 0 and np.nanmax(acc[..., :3]) > 0
