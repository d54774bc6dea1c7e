#!/usr/bin/env python3
"""Render regions on the GPU (DESIGN.md §3c "Render regions", §4 measurements).

  1. region scaling: C3 at 1920x1080 x 128 spp, the full frame against centred rectangles of 1/4 and 1/16 of the area: wall time around
     render_step(0) + pt_wait, median of 5, and its ratio to the full frame's beside the area ratio;
  2. checkpoint cost with the rectangle predicate: the device time of k_adaptive_check + the compaction per checkpoint at 1920x1080 (C3,
     every tile active, no region: tools/adaptive_timing.py's measurement), and with the 1/4 rectangle.

Run each invocation under its own time limit, e.g.  timeout -k 10 600 python tools/region_timing.py --json out.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from platinum_amd import Renderer, abi, scenes  # noqa: E402

SIZE, SPP, BOUNCES = (1920, 1080), 128, 8


def centred(size, share):
    """The centred rectangle with `share` of the area and the frame's aspect ratio."""
    w, h = int(round(size[0] * share ** 0.5)), int(round(size[1] * share ** 0.5))
    x0, y0 = (size[0] - w) // 2, (size[1] - h) // 2
    return (x0, y0, x0 + w, y0 + h)


def timed(r, sc, rect, repeats=5):
    if rect is None:
        r.clearRenderRegion()
    else:
        r.setRenderRegion(*rect)
    ms, paths = [], 0
    for _ in range(repeats + 1):      # (the first render of a kind is the warm-up)
        r.startRender(sc, SIZE, SPP, max_bounces=BOUNCES, nonfinite_policy=abi.NONFINITE_ZERO)
        t0 = time.perf_counter()
        r.render(0)
        r.wait()
        ms.append((time.perf_counter() - t0) * 1e3)
        paths = r.stats().paths
    return statistics.median(ms[1:]), paths


def checkpoint_cost(r, sc, rect, spp=18):
    if rect is None:
        r.clearRenderRegion()
    else:
        r.setRenderRegion(*rect)
    r.setProfiling(True)
    acc = []
    for min_spp in (2, spp):   # tiny threshold: no tile converges; min_spp = spp: the same one-sample batches, no checkpoint
        r.setAdaptiveOptions(enabled=1, threshold=1e-12, min_spp=min_spp, interval=1)
        r.startRender(sc, SIZE, spp, max_bounces=BOUNCES, samples_in_flight=1, nonfinite_policy=abi.NONFINITE_ZERO)
        r.render(0)
        r.wait()
        acc.append(r.stats().ms_accumulate)
    r.setProfiling(False)
    r.setAdaptiveOptions(enabled=0)
    return (acc[0] - acc[1]) / (spp - 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    r = Renderer(device=0)
    sc = scenes.field_scene()
    res = {"scaling": [], "checkpoint_ms": {}}
    full_ms = None
    for name, share in (("full frame", 1.0), ("1/4", 0.25), ("1/16", 0.0625)):
        rect = None if share == 1.0 else centred(SIZE, share)
        ms, paths = timed(r, sc, rect)
        full_ms = ms if full_ms is None else full_ms
        area = 1.0 if rect is None else (rect[2] - rect[0]) * (rect[3] - rect[1]) / (SIZE[0] * SIZE[1])
        row = dict(region=name, rect=rect, ms=round(ms, 2), paths=paths, area_share=round(area, 4), time_share=round(ms / full_ms, 4),
                   time_over_area=round(ms / full_ms / area, 2))
        res["scaling"].append(row)
        print("  ".join("%s=%s" % kv for kv in row.items()), flush=True)
    for name, rect in (("no region", None), ("1/4", centred(SIZE, 0.25))):
        res["checkpoint_ms"][name] = ms = checkpoint_cost(r, sc, rect)
        print("checkpoint (check + compaction) at %dx%d, %s: %.4f ms" % (SIZE + (name, ms)), flush=True)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
