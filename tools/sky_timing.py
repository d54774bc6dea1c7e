#!/usr/bin/env python3
"""Cost of the sun-and-sky generator on the GPU against the host build of the same functions (DESIGN.md §4 "Sun and sky").

Per map size (1024x512 and 2048x1024 by default), in ONE process:
  * device: after --warmup calls, --rounds rounds of --reps calls of pt_generate_sky; per round the median of pt_sky_stats.kernel_ms (k_sky
    between two events on the renderer's stream) and of the whole call's wall time (Omega_d on the host, the launch, the read-back of the
    map); the rounds' medians are printed, and their median is the figure;
  * host: tests/emu/sky_emu.cpp (pt_sky.h compiled -O2 for the host, the same per-texel functions) on one core, --host-reps runs after one
    warm-up run, their median; the two images are compared bit for bit on the way;
  * the ratio host / kernel_ms.
The sun moves between calls (a slider being dragged), so no call can reuse another's map.

Run under its own time limit, e.g.  timeout -k 10 900 python tools/sky_timing.py --json out.json
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1024x512", "2048x1024"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import numpy as np
    import sky_lib as sl
    from platinum_amd import Renderer

    r = Renderer(device=0)
    rows = []
    try:
        for size in a.sizes:
            w, h = (int(v) for v in size.lower().split("x"))
            elevations = [0.05 + 0.01 * k for k in range(a.warmup + a.rounds * a.reps)]
            for e in elevations[:a.warmup]:
                r.generateSky(width=w, height=h, sun_elevation=e)
            kernel, wall = [], []
            for k in range(a.rounds):
                km, wm = [], []
                for e in elevations[a.warmup + k * a.reps:a.warmup + (k + 1) * a.reps]:
                    t0 = time.perf_counter()
                    _, st = r.generateSky(width=w, height=h, stats=True, sun_elevation=e)
                    wm.append((time.perf_counter() - t0) * 1e3)
                    km.append(st.kernel_ms)
                kernel.append(median(km))
                wall.append(median(wm))
            o = sl.options(sun_elevation=0.5)
            got = r.generateSky(options=o, width=w, height=h)
            sl.host_sky(sl.options(sun_elevation=0.4), w, h)     # warm-up
            host = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                want, _, _ = sl.host_sky(o, w, h)
                host.append((time.perf_counter() - t0) * 1e3)
            same = bool(np.array_equal(sl.bits(got), sl.bits(want)))
            row = {"size": size, "kernel_ms_rounds": kernel, "kernel_ms": median(kernel), "call_ms_rounds": wall, "call_ms": median(wall),
                   "host_ms_runs": host, "host_ms": median(host), "ratio": median(host) / median(kernel), "bit_identical": same}
            rows.append(row)
            print("%s: k_sky %.3f ms (rounds %s), whole call %.2f ms; host build on one core %.0f ms (runs %s); host / kernel = %.0f; images %s"
                  % (size, row["kernel_ms"], ", ".join("%.3f" % v for v in kernel), row["call_ms"], row["host_ms"],
                     ", ".join("%.0f" % v for v in host), row["ratio"], "bit-identical" if same else "DIFFER"), flush=True)
    finally:
        r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0 if all(row["bit_identical"] for row in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
