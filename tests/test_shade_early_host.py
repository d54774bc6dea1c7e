"""The split energy-table lookups (platinum_amd/csrc/pt_bsdf.h lutN_fetch / lut_resolve) and the issue-early shading chain (pt_shade.h
shade_issue / shade_land) on the host, no GPU: tests/cpp/shade_early_check.cpp, a program of its own, holds them bit for bit to the
one-piece lookup formulas and to the plain BSDF calls.  It is built twice: as the product's host code is built, and under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "shade_early_check.cpp")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math"]


def run(exe):
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout


def check_output(out):
    # (a) 257 coordinates per axis: 128 + 128^2-grid + 32^2-grid + 32^3-grid lookups (+ the six coordinates that are no table coordinate)
    assert "lookup split: %d lookups, 0 mismatches" % (257 + 257 ** 2 + 257 ** 2 + 257 ** 3 + 6) in out
    # (b) 4096 inputs for each of the four material classes
    for cls in range(4):
        assert "phased chain, class %d: 4096 inputs, 0 mismatches" % cls in out
    assert "inputs do not cover" not in out and "shade_early_check: ok" in out


def test_split_lookups_and_phased_chain_match_the_plain_forms_bit_for_bit(tmp_path):
    exe = tmp_path / "shade_early_check"
    subprocess.check_call(["g++", "-O2"] + FLAGS + ["-o", str(exe), SRC])
    check_output(run(exe))


def test_the_same_program_runs_clean_under_asan_and_ubsan(tmp_path):
    """Stand-alone, nothing preloaded: speculative fetches form addresses from coordinates the plain code never looked up (a light below the
    horizon, the zero direction of a hit without NEE, NaN), so every float -> int conversion and every table read is checked here."""
    exe = tmp_path / "shade_early_check_san"
    subprocess.check_call(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                                                        "-static-libubsan", "-o", str(exe), SRC])
    check_output(run(exe))
