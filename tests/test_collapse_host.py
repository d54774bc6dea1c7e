"""CPU: the least-cost 6-wide collapse (platinum_amd/csrc/pt_collapse.h) on the host.  tests/cpp/collapse_check.cpp includes the header the
device build includes and holds the cost table and the walk over its decisions against an enumeration of every collapse of small binary trees
(optimal bit for bit, valid, never dearer than the area rule, the same tree on a rerun); see that file's head comment.  Built twice: as it is, and
with -fsanitize=address,undefined (a stand-alone program: the sanitizers' runtimes are linked into it)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "collapse_check.cpp")
HDRS = [os.path.join(ROOT, "platinum_amd", "csrc", h) for h in ("pt_collapse.h", "pt_math.h")]
BUILD = os.path.join(ROOT, "tests", "_build")


def _build(name, extra):
    exe = os.path.join(BUILD, name)
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + extra + [SRC, "-o", exe])
    return exe


@pytest.mark.parametrize("name,extra", [("collapse_check", []),
                                        ("collapse_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                         ids=["plain", "asan_ubsan"])
def test_the_cost_table_is_optimal_and_its_tree_valid(name, extra):
    r = subprocess.run([_build(name, extra)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().splitlines()[-1].startswith("collapse_check ok: 440 trees")
