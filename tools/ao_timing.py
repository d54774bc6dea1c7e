#!/usr/bin/env python3
"""Cost of the ambient-occlusion pass on the GPU (DESIGN.md §4 "Ambient occlusion").

Per workload (C3 by default, at its benchmark size and bounce count, 128 samples in flight), with per-kernel HIP-event timing on, in ONE
process after a warm-up render, alternating AO off / on at distance 1 / on at distance inf, --reps times:
  * the device-event time of a batch: the five kernel classes of pt_stats plus, with AO on, pt_ao_stats.ms_trace and ms_fold, per batch;
    AO on minus off in ms and as a share of the AO-off batch; the spread (min..max) of the repeated AO-off runs beside it;
  * ms_trace per batch and per AO ray (pt_ao_stats.rays), and ms_fold per batch;
  * beside them the AO-off batch's shadow class per shadow ray, the yardstick for an any-hit ray (all bounces; the bounce-0 figure is
    tools/per_bounce.sh's).
--against ROOT: the AO-off batch of this tree against the tree at ROOT (a checkout of another commit with its library built), in child
processes of this script (--off-only) that import platinum_amd from the tree they are given, alternating ROOT, here, ROOT, here ...
--rounds times; each side's median and spread of the per-batch device-event time.

Run each invocation under its own time limit, e.g.  timeout -k 10 900 python tools/ao_timing.py --json out.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def class_ms(st):
    return st.ms_raygen + st.ms_closest + st.ms_shade + st.ms_shadow + st.ms_accumulate


def one_render(r, sc, size, bounces, samples, batches, ao):
    """A render of `batches` batches of `samples`; ao: None (off) or the distance.  Uses nothing a library without AO lacks when ao is None."""
    if ao is not None:
        r.setAmbientOcclusionOptions(enabled=1, distance=ao)
    elif hasattr(r, "setAmbientOcclusionOptions"):
        r.setAmbientOcclusionOptions(enabled=0)
    r.startRender(sc, size, samples * batches, max_bounces=bounces, samples_in_flight=samples)
    t0 = time.perf_counter()
    r.render(0)
    r.wait()
    wall = (time.perf_counter() - t0) * 1e3
    st = r.stats()
    assert st.batches == batches and st.samples_in_flight == samples, (st.batches, st.samples_in_flight)
    row = {"device_ms": class_ms(st) / batches, "wall_ms": wall / batches, "shadow_ms": st.ms_shadow / batches, "shadow_rays": st.shadow_rays / batches,
           "closest_ms": st.ms_closest / batches}
    if ao is not None:
        a = r.ambientOcclusionStats()
        row.update(device_ms=row["device_ms"] + (a.ms_trace + a.ms_fold) / batches, trace_ms=a.ms_trace / batches, fold_ms=a.ms_fold / batches,
                   rays=a.rays / batches)
    return row


def off_only(a):
    """child mode: AO-off batches of the tree at a.root, one JSON line"""
    sys.path.insert(0, a.root)
    from platinum_amd import Renderer, scenes
    factory, w, h, _spp, bounces = scenes.CONFIGS[a.configs[0]]
    sc = factory()
    r = Renderer(device=0)
    r.setProfiling(True)
    rows = [one_render(r, sc, (w, h), bounces, a.samples, a.batches, None) for _ in range(a.reps + 1)][1:]   # (the first warms up)
    r.close()
    print(json.dumps({"root": a.root, "device_ms": [v["device_ms"] for v in rows], "wall_ms": [v["wall_ms"] for v in rows]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c3"])
    ap.add_argument("--samples", type=int, default=128, help="samples per batch (samples_in_flight)")
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--against", default=None, metavar="ROOT", help="a checkout of another commit, built: compare its AO-off batch with this tree's")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--off-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.off_only:
        return off_only(a)
    sys.path.insert(0, HERE)
    from platinum_amd import Renderer, scenes
    out = {"samples_per_batch": a.samples, "batches": a.batches, "reps": a.reps, "configs": {}}
    r = Renderer(device=0)
    r.setProfiling(True)
    modes = (("off", None), ("on_1", 1.0), ("on_inf", float("inf")))
    for name in a.configs:
        factory, w, h, _spp, bounces = scenes.CONFIGS[name]
        sc = factory()
        rows = {k: [] for k, _ in modes}
        for _ in range(a.reps + 1):     # (the first repetition warms up and is dropped)
            for k, d in modes:
                rows[k].append(one_render(r, sc, (w, h), bounces, a.samples, a.batches, d))
        rows = {k: v[1:] for k, v in rows.items()}
        off = summary([v["device_ms"] for v in rows["off"]])
        row = {"size": [w, h], "bounces": bounces, "samples_per_batch": a.samples, "device_ms_per_batch_off": off,
               "wall_ms_per_batch_off": summary([v["wall_ms"] for v in rows["off"]]),
               "shadow_ns_per_ray_off": summary([1e6 * v["shadow_ms"] / v["shadow_rays"] for v in rows["off"]])}
        for k in ("on_1", "on_inf"):
            diff = [b["device_ms"] - o["device_ms"] for o, b in zip(rows["off"], rows[k])]
            row[k] = {"device_ms_per_batch": summary([v["device_ms"] for v in rows[k]]), "on_minus_off_ms": summary(diff),
                      "on_minus_off_share": summary([d / o["device_ms"] for d, o in zip(diff, rows["off"])]),
                      "trace_ms_per_batch": summary([v["trace_ms"] for v in rows[k]]), "fold_ms_per_batch": summary([v["fold_ms"] for v in rows[k]]),
                      "rays_per_batch": rows[k][0]["rays"], "trace_ns_per_ray": summary([1e6 * v["trace_ms"] / v["rays"] for v in rows[k]])}
        out["configs"][name] = row
        print(name, json.dumps(row), flush=True)
    r.setAmbientOcclusionOptions(enabled=0)
    r.close()
    if a.against:
        sides = {"against": os.path.abspath(a.against), "here": HERE}
        got = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, root in sides.items():
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--off-only", "--root", root, "--configs", a.configs[0], "--samples",
                                    str(a.samples), "--batches", str(a.batches), "--reps", str(a.reps)], capture_output=True, text=True, timeout=600, cwd=root)
                if p.returncode != 0:
                    sys.exit("the child for %s failed (exit status %d):\n%s" % (root, p.returncode, p.stderr[-2000:]))
                got[k] += json.loads(p.stdout.strip().splitlines()[-1])["device_ms"]
        out["ao_off_against"] = {k: dict(summary(v), root=sides[k], runs=len(v)) for k, v in got.items()}
        print("ao_off_against", json.dumps(out["ao_off_against"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
