"""The build of the ID-matte kernels (matte.hip), no GPU: registers, scratch, spills, occupancy and LDS as tools/kernel_resources.sh reports
them for the Makefile's flags.  k_accumulate_matte and its adaptive twin hold both layers' 16 slots in registers across a batch: a slot
array that the compiler indexes at run time would sit in scratch (the fold is written as compare-selects, pt_matte.h), so they must not
touch scratch or spill, and they stay inside the budget row k_accumulate has in tests/test_kernel_resources.py.  k_matte_ids and
k_matte_resolve must not touch scratch either."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# k_accumulate's row of tests/test_kernel_resources.py: (max VGPRs, max scratch bytes, min waves per SIMD, max LDS bytes per block)
ACCUMULATE_BUDGET = (64, 0, 4, 40 * 1024)
FOLD_KERNELS = ("k_accumulate_matte", "k_accumulate_matte_adaptive")
OTHER_KERNELS = ("k_matte_ids", "k_matte_resolve")


def test_the_matte_kernels_keep_their_slots_in_registers():
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh")], capture_output=True, text=True, timeout=600).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"(.+?) VGPRs (\d+) scratch (\d+) spill (\d+) occ (\d+) LDS (\d+)", line.strip())
        if m:
            seen[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    vgpr, scratch, occ, lds = ACCUMULATE_BUDGET
    for name in FOLD_KERNELS:
        assert name in seen, (name, sorted(seen))
        v, s, sp, o, l = seen[name]
        print(name, "VGPRs %d scratch %d spill %d occ %d LDS %d" % seen[name])
        assert s == 0 and sp == 0, (name, seen[name])
        assert v <= vgpr and s <= scratch and o >= occ and l <= lds, (name, seen[name])
        assert l > 0   # (the staging area is there: the kernel that was measured is the one that stages through LDS)
    for name in OTHER_KERNELS:
        assert name in seen, (name, sorted(seen))
        print(name, "VGPRs %d scratch %d spill %d occ %d LDS %d" % seen[name])
        assert seen[name][1] == 0, (name, seen[name])
