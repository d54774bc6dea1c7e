"""The sun-and-sky kernel (k_sky, sky.hip) is held to what it was built for, and the kernels of every other unit keep the report lines and
budgets they had.  One cross-compile per process (tests/kernel_report.py), no GPU.

  k_sky   no scratch, no spills, no LDS.  It is bound by its exponentials, not by loads in flight, and its block of 256 threads fits eight
          waves per SIMD: 64 VGPRs at the most.  As built: 53 VGPRs, occupancy 8 (the line is printed; profiles/r26_sun_sky.md quotes it)."""
import kernel_report
import test_kernel_resources as tkr


def test_k_sky_touches_no_scratch_and_runs_at_full_occupancy():
    seen = kernel_report.kernels()
    assert "k_sky" in seen, sorted(seen)
    row = seen["k_sky"]
    print(row.line)
    assert row.scratch == 0 and row.spill == 0 and row.lds == 0, row.line
    assert row.vgprs <= tkr.FULL_OCCUPANCY.vgprs and row.occ >= tkr.FULL_OCCUPANCY.occ, row.line


def test_the_kernels_of_every_other_unit_keep_their_lines_and_budgets():
    tkr.unchanged(*[name for name, row in tkr.TABLE.items() if row.line is not None])
    tkr.inside_budget(*tkr.TABLE)
