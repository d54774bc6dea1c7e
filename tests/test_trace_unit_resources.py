"""The trace kernels' translation unit (platinum_amd/csrc/trace_kernels.hip: k_trace_closest, k_trace_shadow) is compiled without LLVM's SLP
vectoriser so that the closest-hit kernel fits a seventh wave per SIMD and the shadow kernel stays in reach of an eighth.  That is a property
of the BUILD (tools/kernel_resources.sh through tests/kernel_report.py: one cross-compile per process, no GPU):

  k_trace_closest<Walk6 | Walk4, false>   <= 72 VGPRs (7 waves per SIMD), no scratch, no spill
  k_trace_shadow<Walk6 | Walk4, false>    <= 64 VGPRs (8 waves per SIMD), no scratch, no spill
  the counting instantiations (<..., true>)   no scratch
  every one of them                       reported occupancy >= the blocks per CU of its launch bound, which is the member of the walk's
                                          description (pt_bvh.h) that trace_walk hands the renderer for that kernel's grid; LDS per block
                                          times those blocks <= the CU's 160 KB
  k_trace_closest_unlisted, k_trace_ao<Walk6>, k_camera_primary<true | false> (kernels.hip, built as before)   the report lines they had

The bounds are the hardware's: 512 VGPRs per SIMD lane in allocation steps of 8 leave a wave 72 at 7 waves and 64 at 8."""
import os
import re

import kernel_report
import test_kernel_resources as tkr

CSRC = os.path.join(kernel_report.ROOT, "platinum_amd", "csrc")
WALKS = ("Walk6", "Walk4")
LDS_PER_CU = 160 * 1024
# (k_trace_closest_unlisted's line is the one table's; the others are what the script printed for the commit before the unit was split off)
UNCHANGED = {
    "k_trace_closest_unlisted": tkr.TABLE["k_trace_closest_unlisted"].line,
    "void k_trace_ao<Walk6>": "void k_trace_ao<Walk6> VGPRs 80 scratch 0 spill 0 occ 6 LDS 22528",
    "void k_camera_primary<true>": "void k_camera_primary<true> VGPRs 75 scratch 0 spill 0 occ 6 LDS 0",
    "void k_camera_primary<false>": "void k_camera_primary<false> VGPRs 80 scratch 32 spill 7 occ 6 LDS 0",
}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _macro(src, name):
    """The integer a chain of `#define name value` / `constexpr int name = value;` of pt_bvh.h ends in (the #ifndef defaults: the build passes
    no -D)."""
    for _ in range(8):
        if re.fullmatch(r"\d+", name):
            return int(name)
        m = (re.search(r"^#define %s (\w+)\s*(?://.*)?$" % re.escape(name), src, re.M)
             or re.search(r"^constexpr int %s = (\w+);" % re.escape(name), src, re.M))
        assert m, name
        name = m.group(1)
    raise AssertionError(name)


def _walk_member(walk, member):
    """Walk::member of pt_bvh.h as an integer."""
    src = _read("pt_bvh.h")
    body = re.search(r"^struct %s \{.*?^\};" % walk, src, re.M | re.S)
    assert body, walk
    m = re.search(r"\b%s = (\w+)" % member, body.group(0))
    assert m, (walk, member)
    return _macro(src, m.group(1))


def _launch_members():
    """{(kernel, COUNT): the Walk member in its launch bound} as trace_kernels.hip states them."""
    src = _read("trace_kernels.hip")
    m = re.search(r"__launch_bounds__\(W::kThreads, COUNT \? W::(k\w+BlocksPerCu) : W::(k\w+BlocksPerCu)\)\s*\nk_trace_closest\(", src)
    assert m, "k_trace_closest's launch bound"
    s = re.search(r"__launch_bounds__\(W::kThreads, W::(k\w+BlocksPerCu)\)\s*\nk_trace_shadow\(", src)
    assert s, "k_trace_shadow's launch bound"
    return {("k_trace_closest", True): m.group(1), ("k_trace_closest", False): m.group(2),
            ("k_trace_shadow", True): s.group(1), ("k_trace_shadow", False): s.group(1)}


def _row(kernel, walk, count):
    seen = kernel_report.kernels()
    name = "void %s<%s, %s>" % (kernel, walk, "true" if count else "false")
    assert name in seen, (name, sorted(n for n in seen if "k_trace" in n))
    print(seen[name].line)
    return seen[name]


def test_the_render_instantiations_fit_seven_and_eight_waves_without_scratch():
    for walk in WALKS:
        for kernel, vgprs in (("k_trace_closest", 72), ("k_trace_shadow", 64)):
            row = _row(kernel, walk, False)
            assert row.vgprs <= vgprs and row.scratch == 0 and row.spill == 0, row.line


def test_the_counting_instantiations_use_no_scratch():
    for walk in WALKS:
        for kernel in ("k_trace_closest", "k_trace_shadow"):
            row = _row(kernel, walk, True)
            assert row.scratch == 0, row.line


def test_occupancy_and_lds_allow_the_blocks_per_cu_each_kernel_is_launched_with():
    members = _launch_members()
    # the renderer's grids come from trace_walk_of, which must hand out the same members in TraceWalk's order
    assert re.search(r"return \{\(uint32_t\)W::kThreads, \(uint32_t\)W::kClosestBlocksPerCu, \(uint32_t\)W::kClosestTraceBlocksPerCu, "
                     r"\(uint32_t\)W::kShadowBlocksPerCu,", _read("trace_kernels.hip"))
    assert members[("k_trace_closest", False)] == "kClosestTraceBlocksPerCu" and members[("k_trace_closest", True)] == "kClosestBlocksPerCu"
    assert members[("k_trace_shadow", False)] == "kShadowBlocksPerCu"
    for walk in WALKS:
        assert _walk_member(walk, "kThreads") == 256   # one wave per SIMD per block: blocks per CU = waves per SIMD
        for (kernel, count), member in members.items():
            blocks = _walk_member(walk, member)
            row = _row(kernel, walk, count)
            assert row.occ >= blocks, (row.line, member, blocks)
            assert row.lds * blocks <= LDS_PER_CU, (row.line, member, blocks)
    assert _walk_member("Walk6", "kClosestTraceBlocksPerCu") > _walk_member("Walk6", "kClosestBlocksPerCu")   # the seventh wave is what the unit is for


def test_the_walks_left_in_kernels_hip_keep_their_lines():
    seen = kernel_report.kernels()
    for name, line in UNCHANGED.items():
        assert name in seen, name
        assert seen[name].line == line, (seen[name].line, line)
    # ... and their launch bound is still the six-block one
    assert _walk_member("Walk6", "kClosestBlocksPerCu") == 6
    src = _read("kernels.hip")
    assert re.search(r"__launch_bounds__\(Walk6::kThreads, Walk6::kClosestBlocksPerCu\)\s*\nk_trace_closest_unlisted\(", src)
    assert "k_trace_closest(" not in src.split("namespace pt {", 1)[1] and "k_trace_shadow(" not in src.split("namespace pt {", 1)[1]
