"""The occupancy the kernels are designed for is a property of the BUILD: registers, scratch, spills and LDS per kernel as LLVM's
kernel-resource-usage remarks report them for the Makefile's flags (tools/kernel_resources.sh through tests/kernel_report.py: one cross-compile
per process, no GPU).  A change that pushes a kernel over its budget costs 3-40 % on the MI355X (profiles/HISTORY.md)
without failing any parity test — so every budget is asserted here, from one table: a pull request that moves a kernel's numbers on purpose
changes that kernel's row and nothing else."""
import collections
import re

import kernel_report

# One row per kernel that a test below looks at, under the name tools/kernel_resources.sh prints.  What a row leaves out is not asserted.
#   vgprs, scratch, spill, lds   upper bounds: VGPRs, scratch bytes, spilled VGPRs, LDS bytes per block
#   occ                          lower bound: waves per SIMD
#   lds_min                      lower bound on the LDS bytes (with lds == lds_min: the exact size)
#   line                         the script's whole line, frozen: the kernel is one that a feature had to leave as it was
#   like                         the row whose bounds stand in for the ones this row leaves out: the kernel mirrors that one, or is its twin
# A test checks the bounds of its kernels (inside_budget) or their frozen lines (unchanged); the two are apart because a kernel may move inside
# its budget on purpose while the feature that froze its line still has to hear of it.
Budget = collections.namedtuple("Budget", "vgprs scratch spill occ lds lds_min line like", defaults=(None,) * 8)
BOUNDS = ("vgprs", "scratch", "spill", "occ", "lds", "lds_min")
K = 1024
FULL_OCCUPANCY = Budget(vgprs=64, scratch=0, spill=0, occ=8, lds=0)   # 256 threads, no LDS: 64 VGPRs is what 8 waves per SIMD leave a lane
TABLE = {
    # ---- the path tracer's hot kernels (test_hot_kernels_...) ----
    "void k_trace_closest<Walk6, false>": Budget(vgprs=80, scratch=0, occ=6, lds=23 * K),   # 6 blocks of 256 threads per CU
    "void k_trace_shadow<Walk6, false>": Budget(vgprs=72, scratch=0, occ=7, lds=23 * K),    # 7 blocks per CU
    "k_shade": Budget(vgprs=128, scratch=0, occ=4, lds=32 * K),                                     # 4 waves per SIMD
    # (the line: what a render without adaptive sampling, a region or camera lists launches is left as it was; the adaptive, region and
    # fused-camera tests)
    "k_raygen": Budget(vgprs=64, scratch=0, occ=8, lds=0, line="k_raygen VGPRs 48 scratch 0 spill 0 occ 8 LDS 0"),
    # (the line: the adaptive and region tests)
    "k_accumulate": Budget(vgprs=64, scratch=0, occ=4, lds=40 * K, line="k_accumulate VGPRs 54 scratch 0 spill 0 occ 4 LDS 36864"),

    # ---- adaptive sampling and render regions: the virtual-tile kernels mirror the full-frame kernels and stay inside their budgets (the
    # adaptive test; no spills: the region test; k_raygen_adaptive's line: the fused-camera test) ----
    "k_raygen_adaptive": Budget(like="k_raygen", spill=0, line="k_raygen_adaptive VGPRs 48 scratch 0 spill 0 occ 8 LDS 0"),
    "k_accumulate_adaptive": Budget(like="k_accumulate", spill=0),
    # k_accumulate_aov's budget is its own line, 150 VGPRs at 2 waves per SIMD with its 27 KB of staging (the region test)
    "k_accumulate_aov": Budget(vgprs=150, scratch=0, spill=0, occ=2, lds=27 * K,
                               line="k_accumulate_aov VGPRs 150 scratch 0 spill 0 occ 2 LDS 27648"),
    "k_accumulate_aov_adaptive": Budget(like="k_accumulate_aov"),
    # the convergence check and the filter's kernels, which took the rectangle predicate, a row pitch or an origin (the region test): launched
    # with 256 threads and no LDS and built for full occupancy.  (The lines: the filter's kernels as the commit before the firefly clamp
    # printed them; the despeckle test.)
    "k_adaptive_check": FULL_OCCUPANCY,
    "k_dn_prep": FULL_OCCUPANCY._replace(line="k_dn_prep VGPRs 29 scratch 0 spill 0 occ 8 LDS 0"),
    "k_dn_prep_counts": FULL_OCCUPANCY._replace(line="k_dn_prep_counts VGPRs 30 scratch 0 spill 0 occ 8 LDS 0"),
    "k_atrous": FULL_OCCUPANCY._replace(line="k_atrous VGPRs 43 scratch 0 spill 0 occ 8 LDS 0"),
    "k_dn_copy": FULL_OCCUPANCY._replace(line="k_dn_copy VGPRs 6 scratch 0 spill 0 occ 8 LDS 0"),
    "k_dn_despeckle": FULL_OCCUPANCY,   # the firefly clamp is one of them (the despeckle test)

    # ---- the fused bounce-0 kernel (kernels.hip; the fused-camera test).  The wave walk (<true>, batches of a multiple of 64 samples: the
    # flagship's) holds the node in scalar registers and must not touch scratch anywhere, at the 6 waves per SIMD of the list trace it took
    # over; the per-lane instantiation runs cam_trace_ray's loop (pt_camlist.h) inside that loop's budget, with every scratch access outside
    # the entry / triangle loop (test_no_scratch_access_...).  The bounds are the figures of the shipped build; the bounce-0 kernels it
    # stands beside keep the lines they had. ----
    "void k_camera_primary<true>": Budget(vgprs=75, scratch=0, spill=0, occ=6, lds=0),
    "void k_camera_primary<false>": Budget(vgprs=80, scratch=32, spill=7, occ=6, lds=0),
    "k_trace_closest_unlisted": Budget(line="k_trace_closest_unlisted VGPRs 76 scratch 0 spill 0 occ 6 LDS 22528"),
    "k_chunk_tables": Budget(line="k_chunk_tables VGPRs 20 scratch 0 spill 0 occ 8 LDS 9220"),

    # ---- the film kernels (film.hip; the film test).  k_accumulate_film stages eight samples of a tile's Lbuf (16 B) and Fbuf (4 B) entries
    # through LDS with kFoldRow = 9 slots per pixel: 64 * 9 * 20 B = 11520 B, which must be what the build holds (the kernel that was
    # measured is the one that stages), and the LDS of its one-wave blocks allows four waves per SIMD at least, so 128 VGPRs; neither fold
    # may touch scratch or spill, and the three per-ray / per-pixel kernels use no LDS at all. ----
    "k_accumulate_film": Budget(vgprs=128, scratch=0, spill=0, lds=64 * 9 * (16 + 4), lds_min=64 * 9 * (16 + 4)),
    "k_accumulate_film_adaptive": Budget(like="k_accumulate_film"),
    "k_film_flags": Budget(vgprs=64, scratch=0, spill=0, lds=0),
    "k_film_compose": Budget(like="k_film_flags"),
    "k_film_alpha": Budget(like="k_film_flags"),

    # ---- the ID-matte kernels (matte.hip; the matte test).  k_accumulate_matte and its adaptive twin hold both layers' 16 slots in registers
    # across a batch: a slot array that the compiler indexes at run time would sit in scratch (the fold is written as compare-selects,
    # pt_matte.h), so they must not touch scratch or spill; they stay inside k_accumulate's budget, and the staging area is there (the
    # kernel that was measured is the one that stages through LDS).  k_matte_ids and k_matte_resolve must not touch scratch either. ----
    "k_accumulate_matte": Budget(like="k_accumulate", spill=0, lds_min=1),
    "k_accumulate_matte_adaptive": Budget(like="k_accumulate_matte"),
    "k_matte_ids": Budget(scratch=0),
    "k_matte_resolve": Budget(scratch=0),

    # ---- the selection overlay (selection.hip; the overlay test).  It stages a 16 x 16 block's coverage with a halo of up to 16 pixels (48^2
    # floats) beside a table of up to 33^2 tap weights: both must sit in LDS (the kernel that was measured is the one that stages), inside
    # 16 KB, and the tap loop must not touch scratch or spill. ----
    "k_selection_overlay": Budget(scratch=0, spill=0, lds=16384, lds_min=(48 * 48 + 33 * 33) * 4),   # the tile and the table at R = 16

    # ---- the view kernels (view.hip; the view test).  Neither may touch scratch or spill (the heat ramp's stops and the slot loop are selects
    # and unrolled loops, not tables indexed at run time), and both live on loads in flight: eight waves per SIMD, 64 VGPRs.  k_view_range
    # meets its four waves in LDS, three words each; k_view_pass is a streaming kernel that uses none. ----
    "k_view_range": Budget(vgprs=64, scratch=0, spill=0, lds=1024, lds_min=1),
    "k_view_pass": Budget(vgprs=64, scratch=0, spill=0, lds=0),

    # ---- bloom (bloom.hip; the bloom test): full occupancy, and no more LDS than the 34 x 34 staged texels of 16 B ----
    "k_bloom_down0": Budget(scratch=0, spill=0, occ=8, lds=34 * 34 * 16),
    "k_bloom_down": Budget(like="k_bloom_down0"),
    "k_bloom_up": Budget(like="k_bloom_down0"),
    "k_bloom_composite": Budget(like="k_bloom_down0"),

    # ---- auto exposure (exposure.hip; the exposure test): full occupancy; the histogram's 259 counters, the resolve's record ----
    "k_exposure_histogram": Budget(vgprs=64, scratch=0, spill=0, occ=8, lds=259 * 4),
    "k_exposure_resolve": Budget(like="k_exposure_histogram", lds=1072),
    "k_exposure_apply": Budget(like="k_exposure_histogram", lds=0),
}


def budget(name):
    """{bound: value} of `name`'s row, the bounds it leaves out taken from the row it mirrors."""
    row = TABLE[name]
    own = {b: getattr(row, b) for b in BOUNDS}
    if row.like is None:
        return own
    return {b: v if own[b] is None else own[b] for b, v in budget(row.like).items()}


def inside_budget(*names):
    seen = kernel_report.kernels()
    for name in names:
        assert name in seen, (name, sorted(seen))
        print(seen[name].line)
        for bound, value in budget(name).items():
            if value is not None:
                got = getattr(seen[name], "lds" if bound == "lds_min" else bound)
                assert got >= value if bound in ("occ", "lds_min") else got <= value, "%s (%s %d)" % (seen[name].line, bound, value)


def unchanged(*names):
    seen = kernel_report.kernels()
    for name in names:
        assert name in seen, (name, sorted(seen))
        assert seen[name].line == TABLE[name].line, (seen[name].line, TABLE[name].line)


def test_hot_kernels_stay_inside_their_register_scratch_and_lds_budgets():
    inside_budget("void k_trace_closest<Walk6, false>", "void k_trace_shadow<Walk6, false>", "k_shade", "k_raygen", "k_accumulate")


def test_adaptive_kernels_stay_inside_the_budgets_of_the_kernels_they_mirror():
    inside_budget("k_raygen_adaptive", "k_accumulate_adaptive")
    unchanged("k_raygen", "k_accumulate")   # the kernels an adaptive-off render launches


def test_region_kernels_stay_inside_the_budgets_of_the_kernels_they_mirror():
    inside_budget("k_raygen_adaptive", "k_accumulate_adaptive", "k_accumulate_aov_adaptive", "k_adaptive_check", "k_dn_prep", "k_dn_prep_counts",
                  "k_atrous", "k_dn_copy")
    unchanged("k_accumulate_aov")          # the kernel k_accumulate_aov_adaptive mirrors: its budget is this line
    unchanged("k_raygen", "k_accumulate")   # what a render without a region and without adaptive sampling launches


def test_despeckle_kernel_budget_and_untouched_siblings():
    inside_budget("k_dn_despeckle")
    unchanged("k_dn_prep", "k_dn_prep_counts", "k_atrous", "k_dn_copy")


def test_the_fused_kernel_stays_inside_its_budgets_and_its_neighbours_keep_their_lines():
    inside_budget("void k_camera_primary<true>", "void k_camera_primary<false>")
    unchanged("k_raygen", "k_raygen_adaptive", "k_trace_closest_unlisted", "k_chunk_tables")


def test_no_scratch_access_inside_the_entry_and_triangle_loops():
    """The device assembly of kernels.hip under the Makefile's flags: in both instantiations every scratch access lies at loop depth <= 2 (the
    unit loop and the iteration loop: a spill around the trace), none in the entry loop (depth 3) or the triangle loop inside it."""
    text = kernel_report.asm("kernels").splitlines()
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


def test_the_film_kernels_stay_inside_their_budget():
    inside_budget("k_accumulate_film", "k_accumulate_film_adaptive", "k_film_flags", "k_film_compose", "k_film_alpha")


def test_the_matte_kernels_keep_their_slots_in_registers():
    inside_budget("k_accumulate_matte", "k_accumulate_matte_adaptive", "k_matte_ids", "k_matte_resolve")


def test_the_overlay_kernel_stays_inside_its_budget():
    inside_budget("k_selection_overlay")


def test_the_view_kernels_stay_inside_their_budget():
    inside_budget("k_view_range", "k_view_pass")


def test_bloom_kernels_stay_inside_their_budgets():
    inside_budget("k_bloom_down0", "k_bloom_down", "k_bloom_up", "k_bloom_composite")


def test_exposure_kernels_use_no_scratch():
    inside_budget("k_exposure_histogram", "k_exposure_resolve", "k_exposure_apply")
