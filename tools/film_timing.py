#!/usr/bin/env python3
"""Cost of the transparent film on the GPU (DESIGN.md §4 "Transparent film").

Per workload (C3 by default, at its benchmark size and bounce count), with per-kernel HIP-event timing on:
  * the device time of k_film_flags + k_accumulate_film per batch of --samples samples: pt_stats.ms_accumulate of a render with the film on
    minus the same render with the film off (both film kernels are timed in the accumulate class), per batch;
  * beside it, that batch's accumulate class with the film off (k_accumulate), the yardstick: it reads the same 16 B of Lbuf per path, where
    the film reads 20 (Lbuf and Fbuf) and k_film_flags moves 12 (word 3 of the hit record and of rayD, and the flag);
  * a present under each backdrop of the render with the film, and of the render without it: wall time of 50 pt_present_render_target
    calls and one wait for their stream, divided by 50, after a warm-up present.
Each figure is the median of --reps repetitions; the spread is min..max.

Run each invocation under its own time limit, e.g.  timeout -k 10 900 python tools/film_timing.py --json out.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from platinum_amd import Renderer, abi, scenes  # noqa: E402


def summary(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def batch_ms(r, sc, size, bounces, samples, batches, film):
    """(accumulate-class ms per batch, wall ms per batch) of one render of `batches` batches of `samples`"""
    r.setFilmOptions(enabled=1 if film else 0, backdrop=abi.BACKDROP_SCENE)
    r.startRender(sc, size, samples * batches, max_bounces=bounces, samples_in_flight=samples, nonfinite_policy=abi.NONFINITE_ZERO)
    t0 = time.perf_counter()
    r.render(0)
    r.wait()
    wall = (time.perf_counter() - t0) * 1e3
    st = r.stats()
    assert st.batches == batches and st.samples_in_flight == samples, (st.batches, st.samples_in_flight)
    return st.ms_accumulate / batches, wall / batches


def present_ms(r, hip, backdrop, presents=50):
    """wall ms per present: a warm-up present (it allocates the composed source), then `presents` of them and one wait, divided"""
    r.setFilmOptions(backdrop=backdrop, backdrop_rgb=(0.18, 0.18, 0.18))
    ptr, stream = r.presentRenderTarget()
    assert ptr and hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
    t0 = time.perf_counter()
    for _ in range(presents):
        r.presentRenderTarget()
    assert hip.hipStreamSynchronize(C.c_void_p(stream)) == 0
    return (time.perf_counter() - t0) * 1e3 / presents


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c3"])
    ap.add_argument("--samples", type=int, default=128, help="samples per batch (samples_in_flight)")
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    r = Renderer(device=0)
    r.setProfiling(True)
    hip = abi.load_library()
    backdrops = (("scene", abi.BACKDROP_SCENE), ("color", abi.BACKDROP_COLOR), ("transparent", abi.BACKDROP_TRANSPARENT))
    out = {"samples_per_batch": a.samples, "batches": a.batches, "reps": a.reps, "configs": {}}
    for name in a.configs:
        factory, w, h, _spp, bounces = scenes.CONFIGS[name]
        sc = factory()
        # no more samples per batch than the automatic choice gives this frame with the film on
        r.setFilmOptions(enabled=1)
        r.startRender(sc, (w, h), a.samples * a.batches, max_bounces=bounces)
        samples = min(a.samples, r.stats().samples_in_flight)
        rows = {"off": [], "on": []}
        present = {False: {k: [] for k, _ in backdrops}, True: {k: [] for k, _ in backdrops}}
        for _ in range(a.reps + 1):     # (the first repetition warms up and is dropped)
            for film in (False, True):
                rows["on" if film else "off"].append(batch_ms(r, sc, (w, h), bounces, samples, a.batches, film))
                for k, mode in backdrops:       # the render above is still there: one present under each backdrop
                    present[film][k].append(present_ms(r, hip, mode))
        off, on = rows["off"][1:], rows["on"][1:]
        row = {
            "size": [w, h], "bounces": bounces, "samples_per_batch": samples,
            "film_kernels_ms_per_batch": summary([b[0] - a_[0] for a_, b in zip(off, on)]),
            "accumulate_ms_per_batch_film_off": summary([v[0] for v in off]),
            "accumulate_ms_per_batch_film_on": summary([v[0] for v in on]),
            "wall_ms_per_batch_film_off": summary([v[1] for v in off]),
            "wall_ms_per_batch_film_on": summary([v[1] for v in on]),
            "present_wall_ms_film_on": {k: summary(v[1:]) for k, v in present[True].items()},
            "present_wall_ms_film_off": {k: summary(v[1:]) for k, v in present[False].items()},
        }
        out["configs"][name] = row
        print(name, json.dumps(row), flush=True)
    r.setFilmOptions(enabled=0, backdrop=abi.BACKDROP_SCENE)
    r.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
