#!/usr/bin/env python3
"""Cost of the selection overlay on the GPU (DESIGN.md §4 "Selection overlay").

C3 (the 32 x 32 sphere field) at 1920x1080 and 3840x2160, a few samples rendered with mattes on, then pt_present_render_target timed on an
idle stream: the wall time of --presents presents and one stream synchronisation, divided by their number; the median of --reps such runs,
with the spread min..max.  Per size:
  * off            the overlay disabled: the launches of a build without the feature
  * small / large  the overlay on at widths 2 and 16, for SMALL (two rows of spheres in the middle of the field: a few percent of the frame)
                   and LARGE (instance 0, the floor and the walls: most of it); the fraction of pixels the set touches is measured and reported
--off-only times the first row alone and needs nothing of the feature: it runs against an older build too.

Run each invocation under its own time limit, e.g.  timeout -k 10 600 python tools/selection_timing.py --json out.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from platinum_amd import Renderer, abi, scenes  # noqa: E402

SMALL = list(range(497, 561))     # spheres 496 .. 559: rows 15 and 16 of the 32 x 32 field (instance i + 1 is sphere i)
LARGE = [0]                       # the enlarged Cornell shell: floor and walls
SIZES = [(1920, 1080), (3840, 2160)]


def summary(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def present_ms(r, presents, reps):
    """ms per present: `presents` presents and one synchronisation of their stream, `reps` times (after one warm-up run)"""
    hip = abi.load_library()
    out = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        for _ in range(presents):
            _ptr, stream = r.presentRenderTarget()
        assert hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
        out.append((time.perf_counter() - t0) * 1e3 / presents)
    return summary(out[1:])


def start(r, sc, size, spp, bounces, matte):
    if matte:
        r.setMatteOptions(enabled=1)
    r.startRender(sc, size, spp, max_bounces=bounces, samples_in_flight=spp, nonfinite_policy=abi.NONFINITE_ZERO)
    r.render(0)
    r.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presents", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert a.presents >= 50 and a.reps >= 5
    factory, _w, _h, _spp, bounces = scenes.CONFIGS["c3"]
    sc = factory()
    r = Renderer(device=0)
    out = {"presents": a.presents, "reps": a.reps, "sizes": {}}
    for size in SIZES:
        row = {}
        start(r, sc, size, a.spp, bounces, matte=not a.off_only)
        row["off"] = present_ms(r, a.presents, a.reps)
        if not a.off_only:
            for name, ids in (("small", SMALL), ("large", LARGE)):
                r.setSelection(ids)
                cov = r.readbackMatte(abi.MATTE_INSTANCE, ids)
                row[name + "_fraction_of_pixels"] = float((cov > 0).mean())
                for width in (2.0, 16.0):
                    r.setSelectionOptions(enabled=1, width=width)
                    row["%s_width_%g" % (name, width)] = present_ms(r, a.presents, a.reps)
                r.setSelectionOptions(enabled=0)
            row["off_again"] = present_ms(r, a.presents, a.reps)
        out["sizes"]["%dx%d" % size] = row
        print("%dx%d" % size, json.dumps(row), flush=True)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
