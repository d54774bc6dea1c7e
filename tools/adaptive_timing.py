#!/usr/bin/env python3
"""Tile-adaptive sampling on the GPU (DESIGN.md §3b "Adaptive sampling", §4 measurements).

  1. checkpoint cost: the device time of k_adaptive_check + the compaction per checkpoint at 1920x1080 and 3840x2160 (C3, every tile active:
     a render with a checkpoint after every one-sample batch against the same batches without checkpoints, profiling on, K_ACCUM class);
  2. time to quality on Cornell (512x512, 4 bounces) and C3 (1920x1080, 8 bounces): wall time, paths and MSE against a 4096-spp uniform
     render, for uniform renders and adaptive ones at a few thresholds;
  3. throughput late in an adaptive render: paths per second of each checkpoint interval, as tiles drop out of fixed-width batches;
  4. --histogram: tile-count histograms of Cornell "bench" 128x96 (the GPU test's render) over thresholds.

Run each invocation under its own time limit, e.g.  timeout -k 10 1500 python tools/adaptive_timing.py --json out.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from platinum_amd import Renderer, abi, scenes  # noqa: E402


def run(r, sc, size, spp, bounces, threshold=None, min_spp=32, interval=32, sif=0):
    r.setAdaptiveOptions(enabled=0 if threshold is None else 1, threshold=threshold or 1.0, min_spp=min_spp, interval=interval)
    # (the zero policy, as bench.py: one NaN sample would make every MSE NaN)
    r.startRender(sc, size, spp, max_bounces=bounces, samples_in_flight=sif, nonfinite_policy=abi.NONFINITE_ZERO)
    t0 = time.perf_counter()
    r.render(0)
    r.wait()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, r.readbackAccumulator()[..., :3].astype(np.float64), r.stats()


def checkpoint_cost(r, size, spp=18):
    sc = scenes.field_scene()
    r.setProfiling(True)
    acc = []
    for min_spp in (2, spp):   # tiny threshold: no tile converges; min_spp = spp: the same one-sample batches, no checkpoint
        run(r, sc, size, spp, 8, threshold=1e-12, min_spp=min_spp, interval=1, sif=1)
        acc.append(r.stats().ms_accumulate)
    r.setProfiling(False)
    return (acc[0] - acc[1]) / (spp - 2)


def quality(r, name, sc, size, bounces, uniform_spp, thresholds, max_spp, ref_spp=4096):
    _, ref, _ = run(r, sc, size, ref_spp, bounces)
    rows = []
    for spp in uniform_spp:
        ms, img, st = run(r, sc, size, spp, bounces)
        rows.append(dict(scene=name, mode="uniform", spp=spp, ms=round(ms, 1), paths=st.paths, mse=float(((img - ref) ** 2).mean())))
    for t in thresholds:
        ms, img, st = run(r, sc, size, max_spp, bounces, threshold=t)
        n = r.readbackSampleCounts()
        rows.append(dict(scene=name, mode="adaptive", threshold=t, spp=max_spp, ms=round(ms, 1), paths=st.paths, mean_spp=float(n.mean()),
                         mse=float(((img - ref) ** 2).mean())))
    for row in rows:
        print("  ".join("%s=%s" % kv for kv in row.items()), flush=True)
    return rows


def late_throughput(r, size, threshold, max_spp=1024, interval=32):
    sc = scenes.field_scene()
    r.setAdaptiveOptions(enabled=1, threshold=threshold, min_spp=interval, interval=interval)
    r.startRender(sc, size, max_spp, max_bounces=8, nonfinite_policy=abi.NONFINITE_ZERO)
    out, done, last_paths = [], 0, 0
    while done < max_spp:
        t0 = time.perf_counter()
        r.render(interval)
        r.wait()
        dt = time.perf_counter() - t0
        paths = r.stats().paths
        done = r.renderProgress()[0]
        out.append(dict(upto=min(done, max_spp), mpaths_per_s=round((paths - last_paths) / dt / 1e6, 1), ms=round(dt * 1e3, 1),
                        paths=paths - last_paths))
        last_paths = paths
    for row in out:
        print("  late: " + "  ".join("%s=%s" % kv for kv in row.items()), flush=True)
    return out


def histogram(r, thresholds):
    sc = scenes.cornell_scene("bench")
    out = {}
    for t in thresholds:
        run(r, sc, (128, 96), 256, 4, threshold=t, min_spp=16, interval=16)
        n = r.readbackSampleCounts()[::8, ::8]
        vals, cnt = np.unique(n, return_counts=True)
        out[t] = dict(zip([int(v) for v in vals], [int(c) for c in cnt]))
        print("  histogram threshold %g: %s" % (t, out[t]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--histogram", action="store_true", help="only the tile-count histograms")
    a = ap.parse_args()
    r = Renderer(device=0)
    res = {}
    res["histogram"] = histogram(r, [0.03, 0.05, 0.08, 0.1, 0.12, 0.15, 0.2, 0.3])
    if not a.histogram:
        res["checkpoint_ms"] = {}
        for size in ((1920, 1080), (3840, 2160)):
            res["checkpoint_ms"]["%dx%d" % size] = ms = checkpoint_cost(r, size)
            print("checkpoint (check + compaction) at %dx%d: %.4f ms" % (size + (ms,)), flush=True)
        res["quality"] = quality(r, "cornell", scenes.cornell_scene("bench"), (512, 512), 4, [64, 128, 256, 512, 1024],
                                 [0.2, 0.1, 0.05, 0.03, 0.02], 1024)
        res["quality"] += quality(r, "c3", scenes.field_scene(), (1920, 1080), 8, [64, 128, 256, 512], [0.2, 0.1, 0.05, 0.03], 1024)
        res["late"] = late_throughput(r, (1920, 1080), 0.05)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
