#!/usr/bin/env python3
"""Cost of the projected cameras' ray generation on the GPU (DESIGN.md §4 "Camera projections").

Per workload (C3 by default, at its benchmark size and bounce count, --samples samples in flight), with per-kernel HIP-event timing on, one
render of --batches batches under each projection: pt_stats' raygen class (the ray-generation kernel and the chunk-table pass behind it),
the bounce-0 closest-hit time (the closest-hit class of a ONE-bounce render of the same batches: pt_stats does not split the class by
bounce), and Msamples/s (pixels x samples / wall time) of the full-depth render.  The perspective rows are the yardsticks: "perspective" as a
render launches it by default (camera-ray leaf lists: bounce 0 in k_camera_primary, no k_raygen) and "perspective, tree walk" under
$PTAMD_NO_CAMERA_LISTS=1 — k_raygen and the same tree walk at bounce 0 that every projected render uses.
Each figure is the median of --reps repetitions; the spread is min..max.

Run each invocation under its own time limit, e.g.  timeout -k 10 900 python tools/projection_timing.py --json out.json
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from platinum_amd import Renderer, abi, scenes  # noqa: E402


def summary(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def one_render(r, sc, size, bounces, samples, batches):
    r.startRender(sc, size, samples * batches, max_bounces=bounces, samples_in_flight=samples, nonfinite_policy=abi.NONFINITE_ZERO)
    lists = r.cameraListStats().built
    t0 = time.perf_counter()
    r.render(0)
    r.wait()
    wall = time.perf_counter() - t0
    st = r.stats()
    assert st.batches == batches and st.samples_in_flight == samples, (st.batches, st.samples_in_flight)
    return {"raygen_ms_per_batch": st.ms_raygen / batches, "closest_ms_per_batch": st.ms_closest / batches,
            "msamples_per_s": size[0] * size[1] * samples * batches / wall / 1e6, "camera_lists": lists}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c3"])
    ap.add_argument("--samples", type=int, default=128, help="samples per batch (samples_in_flight)")
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert os.environ.get("PTAMD_NO_CAMERA_LISTS", "0") in ("", "0"), "this tool compares the switch's two sides"
    r = Renderer(device=0)
    os.environ["PTAMD_NO_CAMERA_LISTS"] = "1"      # (read at pt_create)
    try:
        walk = Renderer(device=0)
    finally:
        del os.environ["PTAMD_NO_CAMERA_LISTS"]
    for x in (r, walk):
        x.setProfiling(True)
    out = {"samples_per_batch": a.samples, "batches": a.batches, "reps": a.reps, "configs": {}}
    for name in a.configs:
        factory, w, h, _spp, bounces = scenes.CONFIGS[name]
        sc = factory()
        r.startRender(sc, (w, h), a.samples * a.batches, max_bounces=bounces)
        samples = min(a.samples, r.stats().samples_in_flight)
        # an orthographic view volume as high as the perspective image plane at the distance of the scene's middle, so that it frames
        # about what the perspective camera frames
        cam = sc.camera
        ortho_h = 20.0 * (cam.sensor_size[1] / cam.focal_length)
        kinds = [("perspective", r, dict(kind=abi.PROJ_PERSPECTIVE)), ("perspective, tree walk", walk, dict(kind=abi.PROJ_PERSPECTIVE)),
                 ("ortho", r, dict(kind=abi.PROJ_ORTHOGRAPHIC, ortho_height=ortho_h)),
                 ("equirect", r, dict(kind=abi.PROJ_EQUIRECT, fov_x=2 * math.pi, fov_y=math.pi)),
                 ("fisheye", r, dict(kind=abi.PROJ_FISHEYE, fisheye_fov=math.pi))]
        rows = {k: {"full": [], "one_bounce": []} for k, _, _ in kinds}
        for _ in range(a.reps + 1):     # (the first repetition warms up and is dropped)
            for label, x, fields in kinds:
                x.setProjection(**fields)
                rows[label]["full"].append(one_render(x, sc, (w, h), bounces, samples, a.batches))
                rows[label]["one_bounce"].append(one_render(x, sc, (w, h), 1, samples, a.batches))
        row = {"size": [w, h], "bounces": bounces, "samples_per_batch": samples, "ortho_height": ortho_h, "kinds": {}}
        for label, _, _ in kinds:
            full, one = rows[label]["full"][1:], rows[label]["one_bounce"][1:]
            row["kinds"][label] = {
                "camera_lists": full[0]["camera_lists"],
                "raygen_class_ms_per_batch": summary([v["raygen_ms_per_batch"] for v in full]),
                "bounce0_closest_ms_per_batch": summary([v["closest_ms_per_batch"] for v in one]),
                "closest_class_ms_per_batch_full_depth": summary([v["closest_ms_per_batch"] for v in full]),
                "msamples_per_s": summary([v["msamples_per_s"] for v in full]),
            }
            print(name, label, json.dumps(row["kinds"][label]), flush=True)
        out["configs"][name] = row
    for x in (r, walk):
        x.setProjection(kind=abi.PROJ_PERSPECTIVE)
        x.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
