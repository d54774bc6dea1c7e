#!/usr/bin/env python3
"""Cost of ID mattes on the GPU (DESIGN.md §4 "ID mattes").

Per workload (C3, C2, C5 at their benchmark sizes and bounce counts), with per-kernel HIP-event timing on:
  * the device time of k_matte_ids + k_accumulate_matte per batch of --samples samples: pt_stats.ms_accumulate of a render with mattes on
    minus the same render with mattes off (both matte kernels are timed in the accumulate class), per batch;
  * beside it, that batch's accumulate class with mattes off (k_accumulate) and, from a renderer created under
    PTAMD_NO_CAMERA_LISTS=1 (the default path generates the camera rays inside the bounce-0 trace), its k_raygen: the yardsticks, which
    move 16 and 68 bytes per path where the mattes move 8;
  * one pt_read_matte of a 300-id set on the instance layer: wall time of the call (the resolve kernel, the upload of the ids and the
    read-back of W*H floats), and one pt_pick.
Each figure is the median of --reps renders; the spread is min..max.

Run each invocation under its own time limit, e.g.  timeout -k 10 900 python tools/matte_timing.py --json out.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from platinum_amd import Renderer, abi, scenes  # noqa: E402


def summary(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def batch_ms(r, sc, size, bounces, samples, batches, matte):
    """(accumulate-class ms per batch, raygen-class ms per batch, wall ms per batch) of one render of `batches` batches of `samples`"""
    r.setMatteOptions(enabled=1 if matte else 0)
    r.startRender(sc, size, samples * batches, max_bounces=bounces, samples_in_flight=samples, nonfinite_policy=abi.NONFINITE_ZERO)
    t0 = time.perf_counter()
    r.render(0)
    r.wait()
    wall = (time.perf_counter() - t0) * 1e3
    st = r.stats()
    assert st.batches == batches and st.samples_in_flight == samples, (st.batches, st.samples_in_flight)
    return st.ms_accumulate / batches, st.ms_raygen / batches, wall / batches


def renderer_under(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Renderer(device=0)    # (the PTAMD_* switches are read at pt_create)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c3", "c2", "c5"])
    ap.add_argument("--samples", type=int, default=128, help="samples per batch (samples_in_flight)")
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    r = Renderer(device=0)
    plain = renderer_under({"PTAMD_NO_CAMERA_LISTS": "1"})
    r.setProfiling(True)
    plain.setProfiling(True)
    out = {"samples_per_batch": a.samples, "batches": a.batches, "reps": a.reps, "configs": {}}
    for name in a.configs:
        factory, w, h, _spp, bounces = scenes.CONFIGS[name]
        sc = factory()
        # no more samples per batch than the automatic choice gives this frame (C5 at 3840x2160 does not fit 128)
        r.setMatteOptions(enabled=1)
        r.startRender(sc, (w, h), a.samples * a.batches, max_bounces=bounces)
        samples = min(a.samples, r.stats().samples_in_flight)
        rows = {"off": [], "on": [], "raygen": []}
        for _ in range(a.reps + 1):     # (the first repetition warms up and is dropped)
            rows["off"].append(batch_ms(r, sc, (w, h), bounces, samples, a.batches, False))
            rows["on"].append(batch_ms(r, sc, (w, h), bounces, samples, a.batches, True))
        # the render above is still there, mattes on: one resolve and one pick
        ids = list(range(300))
        read_ms, pick_ms = [], []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            r.readbackMatte(abi.MATTE_INSTANCE, ids)
            read_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            r.pick(w // 2, h // 2)
            pick_ms.append((time.perf_counter() - t0) * 1e3)
        for _ in range(a.reps + 1):
            rows["raygen"].append(batch_ms(plain, sc, (w, h), bounces, samples, a.batches, False))
        off, on, ray = (v[1:] for v in (rows["off"], rows["on"], rows["raygen"]))
        row = {
            "size": [w, h], "bounces": bounces, "samples_per_batch": samples,
            "matte_kernels_ms_per_batch": summary([b[0] - a_[0] for a_, b in zip(off, on)]),
            "accumulate_ms_per_batch_mattes_off": summary([v[0] for v in off]),
            "raygen_ms_per_batch_unfused": summary([v[1] for v in ray]),
            "wall_ms_per_batch_mattes_off": summary([v[2] for v in off]),
            "wall_ms_per_batch_mattes_on": summary([v[2] for v in on]),
            "read_matte_300_ids_wall_ms": summary(read_ms[1:]),
            "pick_wall_ms": summary(pick_ms[1:]),
        }
        out["configs"][name] = row
        print(name, json.dumps(row), flush=True)
    r.close()
    plain.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
