"""pt_projection.h under AddressSanitizer and UndefinedBehaviorSanitizer, on the host: tests/cpp/projection_sanitize.cpp is a stand-alone
program (its own main, nothing loaded into Python, no GPU) that walks projection_error, derive_projection and stage_raygen_projected over
the option edges of the formula test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_projection_stage_runs_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "projection_sanitize"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unused-parameter",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "projection_sanitize.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and " rays" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
