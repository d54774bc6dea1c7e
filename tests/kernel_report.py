"""The one runner and parser of tools/kernel_resources.sh: registers, scratch, spills, occupancy and LDS of every kernel as LLVM reports them
for the Makefile's flags (a cross-compile, no GPU), and the device assembly of one translation unit under the same flags.  Both are built once
per process and kept in this module; nothing is kept on disk (a stale report is worse than the 20 s it takes).  tests/test_kernel_resources.py
holds the budgets.  TEST HARNESS, never imported by platinum_amd."""
import collections
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tools", "kernel_resources.sh")
# the name is whatever the script prints before " VGPRs": a template instantiation ("void k_trace_closest<Walk6, false>") has blanks in it
LINE = re.compile(r"(.+?) VGPRs (\d+) scratch (\d+) spill (\d+) occ (\d+) LDS (\d+)$")
Row = collections.namedtuple("Row", "line vgprs scratch spill occ lds")
_lines = None
_asm = {}


def lines():
    """The script's output lines, stripped, from one run without extra flags."""
    global _lines
    if _lines is None:
        p = subprocess.run(["bash", SCRIPT], capture_output=True, text=True, timeout=600)
        out = [l.strip() for l in p.stdout.splitlines()]
        if p.returncode != 0 or not any(LINE.match(l) for l in out):
            raise RuntimeError("tools/kernel_resources.sh: exit status %d, %d lines\n%s" % (p.returncode, len(out), p.stderr[-4000:]))
        _lines = out
    return _lines


def kernels():
    """{name: Row(line, vgprs, scratch, spill, occ, lds)} of lines().  (rocPRIM's instantiations, whose names the script cuts short, share
    keys; the project's own kernels do not.)"""
    return {m.group(1): Row(m.group(0), *(int(x) for x in m.groups()[1:])) for m in map(LINE.match, lines()) if m}


def asm(unit):
    """The gfx950 assembly of platinum_amd/csrc/<unit>.hip, compiled by the script's own device_compile: the flags of the resource run."""
    if unit not in _asm:
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, unit + ".s")
            p = subprocess.run(["bash", "-c", 'source "$0" && device_compile "$1" -S -o "$2"', SCRIPT, unit, out], capture_output=True, text=True,
                               timeout=600)
            if p.returncode != 0:
                raise RuntimeError("device_compile %s: exit status %d\n%s" % (unit, p.returncode, p.stderr[-4000:]))
            with open(out) as f:
                _asm[unit] = f.read()
    return _asm[unit]
