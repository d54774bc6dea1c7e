"""The one builder and loader of the host test harness: tests/emu/host_harness.cpp -> tests/_build/libptamd_host.so, the host build of
the product's stage functions and index maps that emu_lib, denoise_lib, adaptive_lib, region_lib and test_layout_host.py wrap (each sets
the argtypes of its own functions on the handle load() returns) and that bench.py's cpu_baseline times.  The archived probes
(tools/archive/emu_probes.cpp) are built by the same function with another source and output.  TEST HARNESS, never imported by
platinum_amd."""
import ctypes
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "host_harness.cpp")
LIB = os.path.join(ROOT, "tests", "_build", "libptamd_host.so")
# strict IEEE arithmetic: the parity tests compare bits with the oracle and with the device
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-shared"]
_loaded = {}


def dependencies():
    """Everything the harness is made of: a change to any of these files rebuilds the library."""
    return (glob.glob(os.path.join(ROOT, "tests", "emu", "*")) + glob.glob(os.path.join(ROOT, "platinum_amd", "csrc", "*.h"))
            + [os.path.join(ROOT, "include", "ptamd.h")])


def load(src=SRC, lib=LIB):
    """The ctypes handle of `lib`, compiled from `src` first when it is missing or older than `src` or a dependency; one handle per
    library and process.  The compiler writes to a file of this process's own and os.replace puts it in place, so a process that starts
    beside this one loads the old library or the new one, never a partial one."""
    if lib in _loaded:
        return _loaded[lib]
    deps = dependencies() + [src]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        tmp = "%s.%d.tmp" % (lib, os.getpid())
        try:
            subprocess.check_call(["g++"] + FLAGS + ["-o", tmp, src])
            os.replace(tmp, lib)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    _loaded[lib] = ctypes.CDLL(lib)
    return _loaded[lib]
