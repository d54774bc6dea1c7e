#!/usr/bin/env python3
"""Device time of a present under each pass view (DESIGN.md §4 "Pass views").

One render (C3 by default, 1920x1080, a few samples, started with AOVs, ID mattes and the film so that every view is available), then per
view: warm-up presents (the first one under DEPTH allocates the range record), and --reps windows of --presents
pt_present_render_target calls between two HIP events recorded on the present's stream; a window's figure is its elapsed device time
divided by its presents, and a view's figure the median of its windows with min..max beside it.  The chain is all that runs in a window:
the render has finished, so a present enqueues the display chain and nothing else.

--parent-lib PATH compares the beauty present of this build with another build of libptamd.so (the parent commit's): each is measured in a
process of its own (one library per process), alternating, --rounds times each, with the same windows.  The default path is the same code on
both sides, so the two should agree within the spread.

Run each invocation under its own time limit, e.g.  timeout -k 10 600 python tools/view_timing.py --json out.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from platinum_amd import abi  # noqa: E402

VIEW_ENTRIES = ("pt_default_view_options", "pt_set_view_options", "pt_read_view_stats", "pt_debug_view")


def summary(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def window_ms(r, hip, presents):
    """device ms per present of one window: two events around `presents` presents on the stream they are enqueued on"""
    _ptr, stream = r.presentRenderTarget()
    stream = C.c_void_p(stream)
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    assert hip.hipStreamSynchronize(stream) == 0
    assert hip.hipEventRecord(e0, stream) == 0
    for _ in range(presents):
        r.presentRenderTarget()
    assert hip.hipEventRecord(e1, stream) == 0
    assert hip.hipEventSynchronize(e1) == 0
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
    hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    return ms.value / presents


def measure(a, views):
    """{view name: summary of ms per present} of one render in this process"""
    from platinum_amd import Renderer, scenes
    factory, _w, _h, _spp, bounces = scenes.CONFIGS[a.config]
    r = Renderer(device=0)
    hip = abi.load_library()
    r.setDenoiseOptions(enabled=1); r.setMatteOptions(enabled=1); r.setFilmOptions(enabled=1)
    r.startRender(factory(), tuple(a.size), a.spp, max_bounces=bounces)
    r.render(0)
    r.wait()
    out = {}
    for name in views:
        if name != "beauty":
            r.setViewOptions(view=abi.VIEW_NAMES.index(name.split("-")[0]), ramp=abi.RAMP_HEAT if name.endswith("-heat") else abi.RAMP_GREY)
            assert r.viewStats().shown == abi.VIEW_NAMES.index(name.split("-")[0]), name
        for _ in range(2):
            window_ms(r, hip, max(a.presents // 10, 1))      # warm-up: code objects, the view's buffers
        out[name] = summary([window_ms(r, hip, a.presents) for _ in range(a.reps)])
    r.close()
    return out


def child(a, lib):
    """the beauty present of the library `lib`, measured in a process of its own"""
    env = dict(os.environ, PTAMD_LIB=lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", a.config, "--size", str(a.size[0]), str(a.size[1]), "--spp", str(a.spp),
           "--presents", str(a.presents), "--reps", str(a.reps)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise SystemExit("the measurement of %s failed (%d): %s" % (lib, p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])["beauty"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--presents", type=int, default=200, help="presents per timed window")
    ap.add_argument("--reps", type=int, default=7, help="windows per view")
    ap.add_argument("--parent-lib", default=None, help="another build of libptamd.so whose beauty present is measured beside this build's")
    ap.add_argument("--rounds", type=int, default=3, help="with --parent-lib: processes per side, alternating")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.child:
        # (a build from before the pass views lacks their entry points: the beauty present needs none of them)
        probe = C.CDLL(abi.library_path())
        abi.SYMBOLS = [s for s in abi.SYMBOLS if s[0] not in VIEW_ENTRIES or hasattr(probe, s[0])]
        print(json.dumps(measure(a, ["beauty"])), flush=True)
        return
    out = {"config": a.config, "size": list(a.size), "spp": a.spp, "presents_per_window": a.presents, "windows": a.reps}
    if a.parent_lib:
        sides = {"parent": [], "this": []}
        for _ in range(a.rounds):
            sides["parent"].append(child(a, os.path.abspath(a.parent_lib)))
            sides["this"].append(child(a, abi.LIB_PATH))
        out["beauty_ms_by_process"] = sides
        for k, v in sides.items():
            print("beauty present, %s build: medians %s ms" % (k, ", ".join("%.4f" % s["median"] for s in v)), flush=True)
    views = ["beauty", "albedo", "normal", "depth", "depth-heat", "alpha", "matte", "samples", "samples-heat", "noise", "noise-heat"]
    out["present_ms"] = measure(a, views)
    for name in views:
        s = out["present_ms"][name]
        print("%-13s %.4f ms per present (min %.4f, max %.4f)" % (name, s["median"], s["min"], s["max"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
