"""The build of the selection-overlay kernel (selection.hip), no GPU: scratch, spills and LDS as tools/kernel_resources.sh reports them for
the Makefile's flags.  k_selection_overlay stages a 16 x 16 block's coverage with a halo of up to 16 pixels (48^2 floats) beside a table of
up to 33^2 tap weights: both must sit in LDS (> 0: the kernel that was measured is the one that stages), inside 16 KB, and the tap loop must
not touch scratch or spill."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_overlay_kernel_stays_inside_its_budget():
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh")], capture_output=True, text=True, timeout=600).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"(.+?) VGPRs (\d+) scratch (\d+) spill (\d+) occ (\d+) LDS (\d+)", line.strip())
        if m:
            seen[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    name = "k_selection_overlay"
    assert name in seen, sorted(seen)
    vgprs, scratch, spill, occ, lds = seen[name]
    print(name, "VGPRs %d scratch %d spill %d occ %d LDS %d" % seen[name])
    assert scratch == 0 and spill == 0, seen[name]
    assert 0 < lds <= 16384, seen[name]
    assert lds >= (48 * 48 + 33 * 33) * 4      # the tile and the table at R = 16
