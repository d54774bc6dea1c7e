"""The sun-and-sky generator through include/ptamd_renderer.hpp and the C ABI, no GPU and no Python around the code under test:
tests/cpp/sky_check.cpp compiled against libptamd.so and run (defaults, struct layouts, the accessor's type, the order of the entry
point's checks, the host build of pt_sky.h at the corners of its options); platinum_amd/abi.py's structs are held to the sizes and
offsets that program prints.  The same program, without the library, is compiled with -fsanitize=address,undefined and run."""
import ctypes as C
import os
import subprocess

from platinum_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sky_check.cpp")
FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas","-I" + os.path.join(ROOT, "include")]


def _layout(struct):
    return [C.sizeof(struct)] + [getattr(struct, n).offset for n, _ in struct._fields_]


def test_the_program_holds_and_abi_py_has_the_compilers_layout(tmp_path):
    exe = tmp_path / "sky_check"
    libdir = os.path.join(ROOT, "platinum_amd", "csrc")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", str(exe), "-L" + libdir, "-lptamd", "-Wl,-rpath," + libdir])
    p = subprocess.run([str(exe)], timeout=120, stdout=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    lines = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in p.stdout.splitlines() if l.startswith("pt_sky_")}
    assert lines["pt_sky_options"] == _layout(abi.SkyOptions)
    assert lines["pt_sky_stats"] == _layout(abi.SkyStats)


def test_the_host_build_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = tmp_path / "sky_check_san"
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSKY_CHECK_NO_LIBRARY", SRC, "-o", str(exe)])
    p = subprocess.run([str(exe)], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
