#!/usr/bin/env python3
"""Cost of the first-hit AOVs and of the denoiser on the GPU (DESIGN.md §4 "Denoiser").

  1. C3 (1920x1080, 128 spp, 8 bounces): wall time of render_step(0) + wait with AOVs off and on, alternated, --runs each;
  2. the device time of the filter (prep + 5 a-trous steps + post-process, HIP events around pt_present_render_target with
     apply_to_target = 1, minus the same present without it) at 1920x1080 and 3840x2160, with the firefly clamp
     (pt_despeckle_options) off and on.

Run each invocation under its own time limit, e.g.  timeout -k 10 900 python tools/denoise_timing.py --json out.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from platinum_amd import Renderer, abi, scenes  # noqa: E402


def render_ms(r, sc, size, spp, bounces, aov):
    r.setDenoiseOptions(enabled=1 if aov else 0)
    r.startRender(sc, size, spp, max_bounces=bounces)
    t0 = time.perf_counter()
    r.render(0)
    r.wait()
    return (time.perf_counter() - t0) * 1e3


def present_device_ms(r, hip, apply, despeckle=False, reps=20):
    """Device time of one pt_present_render_target (HIP events on the renderer's stream), median of `reps`."""
    r.setDenoiseOptions(apply_to_target=1 if apply else 0)
    r.setDespeckleOptions(enabled=1 if despeckle else 0)
    _, stream = r.presentRenderTarget()
    s = C.c_void_p(stream)
    hip.hipStreamSynchronize(s)
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(e0))
    hip.hipEventCreate(C.byref(e1))
    times = []
    for _ in range(reps):
        hip.hipEventRecord(e0, s)
        r.presentRenderTarget()
        hip.hipEventRecord(e1, s)
        hip.hipEventSynchronize(e1)
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), e0, e1)
        times.append(ms.value)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--spp", type=int, default=128)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    hip = abi.load_library()   # (dlsym on the library's handle reaches the HIP runtime it renders with)
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    r = Renderer(device=0)
    sc = scenes.field_scene()
    out = {"render_ms": {"off": [], "on": []}}
    render_ms(r, sc, (1920, 1080), a.spp, 8, True)     # warm-up: allocations of both modes
    render_ms(r, sc, (1920, 1080), a.spp, 8, False)
    for _ in range(a.runs):
        for mode in ("off", "on"):
            out["render_ms"][mode].append(render_ms(r, sc, (1920, 1080), a.spp, 8, mode == "on"))
    med = {k: sorted(v)[len(v) // 2] for k, v in out["render_ms"].items()}
    out["render_median_ms"] = med
    out["aov_overhead_pct"] = 100.0 * (med["on"] / med["off"] - 1.0)
    print("C3 1920x1080 x %d spp: AOVs off %.2f ms, on %.2f ms (median of %d): %+.2f %%" % (a.spp, med["off"], med["on"], a.runs, out["aov_overhead_pct"]))
    out["filter_ms"] = {}
    for size, spp in (((1920, 1080), 16), ((3840, 2160), 4)):
        render_ms(r, sc, size, spp, 8, True)
        with_f = present_device_ms(r, hip, True)
        with_c = present_device_ms(r, hip, True, despeckle=True)
        without = present_device_ms(r, hip, False)
        key = "%dx%d" % size
        out["filter_ms"][key] = {"present_denoised": with_f, "present_despeckled": with_c, "present_plain": without, "filter": with_f - without,
                                 "filter_despeckle": with_c - without, "despeckle": with_c - with_f}
        print("%s: present with the filter %.3f ms, without %.3f ms: filter (5 iterations) %.3f ms; with the firefly clamp %.3f ms (%+.3f ms)" % (
            key, with_f, without, with_f - without, with_c - without, with_c - with_f))
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
