"""The build of the fused bounce-0 kernel (k_camera_primary, kernels.hip), no GPU: registers, scratch, occupancy and LDS as
tools/kernel_resources.sh reports them for the Makefile's flags, and where in its code the scratch accesses lie.  The wave walk
(k_camera_primary<true>, batches of a multiple of 64 samples: the flagship's) holds the node in scalar registers and must not touch scratch
anywhere; the per-lane instantiation runs cam_trace_ray's loop (pt_camlist.h) inside that loop's budget, with every scratch access outside the
entry / triangle loop.  The kernels that were there before keep the lines they had."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (max VGPRs, max scratch bytes, max spilled VGPRs, min waves per SIMD, LDS bytes): the figures of the shipped build
BUDGET = {
    "void k_camera_primary<true>": (75, 0, 0, 6, 0),
    "void k_camera_primary<false>": (80, 32, 7, 6, 0),
}
# tools/kernel_resources.sh's lines of the bounce-0 kernels this one stands beside, as the commit before it printed them
UNCHANGED = (
    "k_raygen VGPRs 48 scratch 0 spill 0 occ 8 LDS 0",
    "k_raygen_adaptive VGPRs 48 scratch 0 spill 0 occ 8 LDS 0",
    "k_trace_closest_unlisted VGPRs 76 scratch 0 spill 0 occ 6 LDS 22528",
    "k_chunk_tables VGPRs 20 scratch 0 spill 0 occ 8 LDS 9220",
)


def test_the_fused_kernel_stays_inside_its_budgets_and_its_neighbours_keep_their_lines():
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh")], capture_output=True, text=True, timeout=600).stdout
    lines = [l.strip() for l in out.splitlines()]
    seen = {}
    for line in lines:
        m = re.match(r"(.+?) VGPRs (\d+) scratch (\d+) spill (\d+) occ (\d+) LDS (\d+)", line)
        if m:
            seen[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    for name, (vgpr, scratch, spill, occ, lds) in BUDGET.items():
        assert name in seen, (name, sorted(seen))
        v, s, sp, o, l = seen[name]
        print(name, "VGPRs %d scratch %d spill %d occ %d LDS %d" % seen[name])
        assert v <= vgpr and s <= scratch and sp <= spill and o >= occ and l == lds, (name, seen[name])
    assert seen["void k_camera_primary<true>"][3] >= 6   # the waves per SIMD of the list trace it took over
    for line in UNCHANGED:
        assert line in lines, line


def test_no_scratch_access_inside_the_entry_and_triangle_loops(tmp_path):
    """The device assembly of kernels.hip under the Makefile's flags: in both instantiations every scratch access lies at loop depth <= 2 (the
    unit loop and the iteration loop: a spill around the trace), none in the entry loop (depth 3) or the triangle loop inside it."""
    asm = tmp_path / "kernels.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mllvm",
                           "-disable-machine-licm", "--cuda-device-only", "-S", "kernels.hip", "-o", str(asm)],
                          cwd=os.path.join(ROOT, "platinum_amd", "csrc"), stderr=subprocess.DEVNULL)
    text = asm.read_text().splitlines()
    found = 0
    for flag in ("Lb1", "Lb0"):   # the mangled template argument: true, false
        start = [i for i, l in enumerate(text) if re.match(r"_ZN2pt16k_camera_primaryI%sEE.*:" % flag, l)]
        assert len(start) == 1, flag
        found += 1
        depth, deep_scratch, deepest = 0, [], 0
        for l in text[start[0]:]:
            if "s_endpgm" in l:
                break
            m = re.search(r"Depth=(\d+)", l)
            hdr = re.match(r"\s*;.*Loop Header: Depth=(\d+)", l)   # (a loop header's label line names its PARENT loop; its own depth follows)
            if l.startswith(".LBB") or hdr:
                depth = int((hdr or m).group(1)) if (hdr or m) else 0
                deepest = max(deepest, depth)
            elif "scratch_" in l and depth >= 3:
                deep_scratch.append(l.strip())
        assert deepest >= 3, (flag, deepest)   # the loops are there to be looked at
        assert not deep_scratch, (flag, deep_scratch[:5])
    assert found == 2
