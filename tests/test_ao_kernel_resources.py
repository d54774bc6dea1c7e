"""The ambient-occlusion kernels (k_trace_ao in kernels.hip; ao.hip) are held to budgets taken from the one table
(tests/test_kernel_resources.py), and the kernels a render without AO launches keep the report lines they had.  One cross-compile per process
(tests/kernel_report.py), no GPU.

  k_trace_ao<Walk6>            no scratch, no spills, inside k_trace_closest<Walk6, false>'s row (80 VGPRs, 6 waves, 23 KB of LDS) at the least;
                               its launch bound is the shadow kernel's when it also fits that kernel's row (72 VGPRs, 7 waves), else the
                               closest-hit kernel's, and the reported occupancy is what that bound asks for
  k_accumulate_ao(_adaptive)   k_accumulate_film's row with the staging area of 4-byte entries, 64 * 9 * 4 B exactly; no scratch, no spills
  k_ao_scatter                 full occupancy: 256 threads, no LDS, 64 VGPRs"""
import os
import re

import kernel_report
import test_kernel_resources as tkr

TRACE = "void k_trace_ao<Walk6>"
FOLDS = ("k_accumulate_ao", "k_accumulate_ao_adaptive")
LDS_FOLD = 64 * 9 * 4


def _inside(row, want):
    for bound, value in want.items():
        if value is not None:
            got = getattr(row, "lds" if bound == "lds_min" else bound)
            if not (got >= value if bound in ("occ", "lds_min") else got <= value):
                return False
    return True


def test_the_trace_kernel_stays_inside_the_closest_hit_budget_and_its_launch_bound_agrees():
    seen = kernel_report.kernels()
    assert sorted(n for n in seen if "k_trace_ao" in n) == sorted("void k_trace_ao<%s>" % w for w in ("Walk4", "Walk6", "WalkTwoLevel"))
    row = seen[TRACE]
    print(row.line)
    closest = dict(tkr.budget("void k_trace_closest<Walk6, false>"), spill=0)
    shadow = dict(tkr.budget("void k_trace_shadow<Walk6, false>"), spill=0)
    assert (closest["vgprs"], closest["scratch"], closest["occ"], closest["lds"]) == (80, 0, 6, 23 * 1024)
    assert (shadow["vgprs"], shadow["scratch"], shadow["occ"], shadow["lds"]) == (72, 0, 7, 23 * 1024)
    assert row.scratch == 0 and row.spill == 0, row.line
    assert _inside(row, closest), row.line
    # the launch bound in the source, and the grid the launcher takes: the shadow kernel's iff the build fits its row
    src = open(os.path.join(kernel_report.ROOT, "platinum_amd", "csrc", "kernels.hip")).read()
    m = re.search(r"__launch_bounds__\(W::kThreads, W::(k\w+BlocksPerCu)\)\s*\nk_trace_ao\(", src)
    assert m, "k_trace_ao's launch bound"
    fits_shadow = _inside(row, shadow)
    assert m.group(1) == ("kShadowBlocksPerCu" if fits_shadow else "kClosestBlocksPerCu"), (m.group(1), row.line)
    assert re.search(r"void launch_trace_ao\(hipStream_t s, uint32_t %s," % ("grid_shadow" if fits_shadow else "grid_closest"), src)
    # ... and the occupancy the compiler reports is the one that bound asks for (both walks are built for 6 and 7 blocks of 256 threads per CU)
    assert row.occ == (shadow if fits_shadow else closest)["occ"], row.line
    for other in ("void k_trace_ao<Walk4>", "void k_trace_ao<WalkTwoLevel>"):
        print(seen[other].line)
        assert seen[other].scratch == 0 and seen[other].spill == 0, seen[other].line


def test_the_fold_kernels_stage_four_byte_entries_and_touch_no_scratch():
    want = dict(tkr.budget("k_accumulate_film"), lds=LDS_FOLD, lds_min=LDS_FOLD)
    assert (want["vgprs"], want["scratch"], want["spill"]) == (128, 0, 0)
    seen = kernel_report.kernels()
    for name in FOLDS:
        print(seen[name].line)
        assert _inside(seen[name], want) and seen[name].lds == LDS_FOLD, seen[name].line


def test_the_scatter_kernel_is_built_for_full_occupancy():
    want = {b: getattr(tkr.FULL_OCCUPANCY, b) for b in tkr.BOUNDS}
    row = kernel_report.kernels()["k_ao_scatter"]
    print(row.line)
    assert _inside(row, want) and row.spill == 0, row.line
    assert "k_ao_rays" not in kernel_report.kernels()   # the fused form shipped: no generator kernel


def test_the_kernels_a_render_without_ao_launches_keep_their_lines():
    tkr.unchanged("k_raygen", "k_raygen_adaptive", "k_accumulate", "k_accumulate_aov", "k_trace_closest_unlisted", "k_chunk_tables", "k_dn_prep",
                  "k_dn_prep_counts", "k_atrous", "k_dn_copy")
    tkr.inside_budget("void k_trace_closest<Walk6, false>", "void k_trace_shadow<Walk6, false>", "k_shade", "void k_camera_primary<true>",
                      "void k_camera_primary<false>")
