"""Ambient occlusion through include/ptamd_renderer.hpp, no GPU: tests/cpp/ao_accessors.cpp compiled with -Wall -Wextra -pedantic -Werror
against libptamd.so and run (defaults, struct layouts, accessor types, the order of the entry points' checks)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_accessors_compile_and_hold(tmp_path):
    exe = tmp_path / "ao_accessors"
    libdir = os.path.join(ROOT, "platinum_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ao_accessors.cpp"), "-o", str(exe), "-L" + libdir, "-lptamd", "-Wl,-rpath," + libdir])
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
