"""The build of the view kernels (view.hip), no GPU: scratch, spills and LDS as tools/kernel_resources.sh reports them for the Makefile's
flags.  Neither kernel may touch scratch or spill (the heat ramp's stops and the slot loop are selects and unrolled loops, not tables indexed
at run time); k_view_range meets its four waves in LDS, three words each, and k_view_pass is a streaming kernel that uses none."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_view_kernels_stay_inside_their_budget():
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh")], capture_output=True, text=True, timeout=600).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"(.+?) VGPRs (\d+) scratch (\d+) spill (\d+) occ (\d+) LDS (\d+)", line.strip())
        if m:
            seen[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    for name in ("k_view_range", "k_view_pass"):
        assert name in seen, sorted(seen)
        vgprs, scratch, spill, occ, lds = seen[name]
        print(name, "VGPRs %d scratch %d spill %d occ %d LDS %d" % seen[name])
        assert scratch == 0 and spill == 0, (name, seen[name])
        assert vgprs <= 64, (name, seen[name])             # (eight waves per SIMD: both kernels live on loads in flight)
    assert 0 < seen["k_view_range"][4] <= 1024
    assert seen["k_view_pass"][4] == 0
