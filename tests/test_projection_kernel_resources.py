"""The projected ray-generation kernels (projection.hip) are held to k_raygen's budget, taken from the one table
(tests/test_kernel_resources.py): 64 VGPRs, no scratch, no spilled VGPRs, 8 waves per SIMD, no LDS — for every instantiation; and the
kernels a perspective render launches keep the report lines they had.  One cross-compile per process (tests/kernel_report.py), no GPU."""
import kernel_report
import test_kernel_resources as tkr

INSTANTIATIONS = ("void k_raygen_projected<false>", "void k_raygen_projected<true>")


def test_every_instantiation_stays_inside_k_raygens_budget():
    want = dict(tkr.budget("k_raygen"), spill=0)
    assert want == dict(vgprs=64, scratch=0, spill=0, occ=8, lds=0, lds_min=None)
    seen = kernel_report.kernels()
    mine = sorted(n for n in seen if "k_raygen_projected" in n)
    assert mine == sorted(INSTANTIATIONS), mine          # a new instantiation gets the budget too
    for name in mine:
        row = seen[name]
        print(row.line)
        assert row.vgprs <= want["vgprs"] and row.scratch <= want["scratch"] and row.spill <= want["spill"], row.line
        assert row.occ >= want["occ"] and row.lds <= want["lds"], row.line
    tkr.inside_budget("k_raygen", "k_raygen_adaptive")   # (the rows themselves)


def test_the_scatter_kernel_of_the_debug_entry_point_uses_no_scratch():
    row = kernel_report.kernels()["k_camera_rays"]
    print(row.line)
    assert row.scratch == 0 and row.spill == 0 and row.lds == 0 and row.occ == 8


def test_the_kernels_a_perspective_render_launches_keep_their_lines():
    tkr.unchanged("k_raygen", "k_raygen_adaptive", "k_chunk_tables", "k_trace_closest_unlisted", "k_accumulate", "k_accumulate_aov")
