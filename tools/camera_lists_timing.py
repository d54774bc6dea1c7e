#!/usr/bin/env python3
"""Camera-ray leaf lists on the GPU (DESIGN.md §3 "Camera rays from per-pixel leaf lists", §4 measurements): per workload the build's
device time, the share of pixels left to the ordinary traversal, and the histogram of list lengths (before the capacity is applied).
With --front-end: the event time of bounce 0's front end (raygen + closest classes of one render(0) call — all batches of the workload's
samples — traced to a single bounce): k_camera_primary, the table pass and the walk for flagged pixels.

Run each invocation under its own time limit, e.g.  timeout -k 10 300 python tools/camera_lists_timing.py --workloads c3 c2 c5 --json out.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from platinum_amd import Renderer, abi, scenes  # noqa: E402


def measure(r, name):
    make, w, h, spp, bounces = scenes.CONFIGS[name]
    sc = make()
    builds = []
    for _ in range(3):    # (the first start of a size allocates the lists; the build itself is timed with HIP events)
        r.startRender(sc, (w, h), spp, max_bounces=bounces, nonfinite_policy=abi.NONFINITE_ZERO)
        cl = r.cameraListStats()
        builds.append(cl.build_ms)
    hist = list(cl.length_histogram)
    pixels = cl.pixels_listed + cl.pixels_walk
    return {"workload": name, "size": [w, h], "built": cl.built, "capacity": cl.capacity, "build_ms": builds, "pixels": pixels,
            "pixels_walk": cl.pixels_walk, "walk_share": cl.pixels_walk / pixels if pixels else 0.0, "entries": cl.entries,
            "mean_length": cl.entries / cl.pixels_listed if cl.pixels_listed else 0.0, "length_histogram": hist,
            "samples_in_flight": r.stats().samples_in_flight}


def front_end_ms(r, name, repeats=3):
    """raygen + closest event time of one render(0) call traced to ONE bounce: the camera rays' generation, table pass and trace"""
    make, w, h, spp, _ = scenes.CONFIGS[name]
    sc = make()
    out = []
    for _ in range(repeats + 1):
        r.startRender(sc, (w, h), spp, max_bounces=1, nonfinite_policy=abi.NONFINITE_ZERO)
        r.setProfiling(True)
        r.render(0)
        r.wait()
        st = r.stats()
        r.setProfiling(False)
        out.append(st.ms_raygen + st.ms_closest)
    return out[1:]    # (the first pass warms the shape up)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--front-end", action="store_true", help="time bounce 0's front end")
    ap.add_argument("--workloads", nargs="+", default=["c3", "c2", "c5"], choices=sorted(scenes.CONFIGS))
    ap.add_argument("--json")
    args = ap.parse_args()
    r = Renderer(device=0)
    out = []
    for name in args.workloads:
        m = measure(r, name)
        out.append(m)
        print("%s %dx%d: built %d, capacity %d, build ms %s, samples in flight %d" % (name, m["size"][0], m["size"][1], m["built"], m["capacity"],
              " ".join("%.3f" % b for b in m["build_ms"]), m["samples_in_flight"]))
        print("  pixels %d, left to the walk %d (%.4f %%), entries %d, mean length %.2f" % (m["pixels"], m["pixels_walk"], 100 * m["walk_share"],
              m["entries"], m["mean_length"]))
        h = m["length_histogram"]
        print("  length histogram: " + " ".join("%d:%d" % (k, n) for k, n in enumerate(h) if n) + "   (64 = 64 or more)")
    if args.front_end:
        for m in out:
            m["front_end_ms"] = front_end_ms(r, m["workload"], 4)
            print("%s front end (raygen + closest of a one-bounce render): %s ms" % (m["workload"], " ".join("%.3f" % v for v in m["front_end_ms"])))
    r.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
