#!/usr/bin/env python3
"""Cost of bloom on the GPU (DESIGN.md §4 "Bloom").

Device time of one pt_present_render_target (HIP events on the renderer's stream) at 1920x1080 and 3840x2160 on Cornell `bench` at
1 spp, with pt_bloom_options.enabled = 0 and with enabled = 1 at 6 and at 10 levels.  Each figure is the median of --reps presents after
a warm-up; the spread is the min..max of --batches such medians.

--package-root DIR imports platinum_amd from DIR instead of this checkout: a build of another commit.  A library without bloom is timed
with what it has (the disabled column), so the same command measures the parent commit.

Run each invocation under its own time limit, e.g.  timeout -k 10 600 python tools/bloom_timing.py --json out.json
"""
import argparse
import ctypes as C
import json
import os
import sys


def present_ms(r, hip, reps, batches):
    """[median device ms of `reps` presents] for each of `batches` batches, after one warm-up present."""
    _, stream = r.presentRenderTarget()
    s = C.c_void_p(stream)
    hip.hipStreamSynchronize(s)
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip.hipEventCreate(C.byref(e0))
    hip.hipEventCreate(C.byref(e1))
    medians = []
    for _ in range(batches):
        times = []
        for _ in range(reps):
            hip.hipEventRecord(e0, s)
            r.presentRenderTarget()
            hip.hipEventRecord(e1, s)
            hip.hipEventSynchronize(e1)
            ms = C.c_float()
            hip.hipEventElapsedTime(C.byref(ms), e0, e1)
            times.append(ms.value)
        times.sort()
        medians.append(times[len(times) // 2])
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return medians


def summary(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    from platinum_amd import Renderer, abi, scenes

    hip = abi.load_library()   # (dlsym on the library's handle reaches the HIP runtime it renders with)
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    r = Renderer(device=0)
    has = hasattr(r, "setBloomOptions")
    sc = scenes.cornell_scene("bench")
    out = {"bloom": has, "present_ms": {}}
    for size in ((1920, 1080), (3840, 2160)):
        r.startRender(sc, size, 1, max_bounces=4)
        r.render(0)
        r.wait()
        key = "%dx%d" % size
        row = {}
        if has:
            r.setBloomOptions(enabled=0)
        row["disabled"] = summary(present_ms(r, hip, a.reps, a.batches))
        if has:
            for levels in (6, 10):
                r.setBloomOptions(enabled=1, levels=levels)
                row["%d levels" % levels] = summary(present_ms(r, hip, a.reps, a.batches))
            r.setBloomOptions(enabled=0)
        out["present_ms"][key] = row
        print("%s: present %s" % (key, ", ".join("%s %.4f ms (%.4f..%.4f)" % (k, v["median"], v["min"], v["max"]) for k, v in row.items())))
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
