"""The fused bounce-0 kernel (platinum_amd/csrc/kernels.hip k_camera_primary) on the host, no GPU: tests/emu/camfused_emu.cpp holds the
closed form that places a camera ray in its segment (pt_layout.h camera_rays_before) to k_raygen's own packing loop, and the per-lane list
trace the kernels share (pt_camlist.h cam_trace_ray) to cam_trace_list on the host trees of the field and Cornell scenes, bit for bit."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import emu_lib
import host_build
from platinum_amd.renderer import make_params
from test_camera_lists_host import CASES, jitters

SRC = os.path.join(host_build.ROOT, "tests", "emu", "camfused_emu.cpp")


@functools.lru_cache(maxsize=None)
def lib():
    L = host_build.load(SRC, os.path.join(host_build.ROOT, "tests", "_build", "libptamd_camfused.so"))
    emu_lib.bind(L)
    L.cf_slot_check.restype = C.c_int
    L.cf_slot_check.argtypes = [C.c_uint32] * 6 + [C.c_void_p]
    L.cf_trace_check.restype = C.c_int
    L.cf_trace_check.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    L.cl_default_capacity.restype = C.c_uint32
    return L


def slot_check(w, h, nseg, bands, tps, ns):
    out = np.zeros(5, dtype=np.uint64)
    assert lib().cf_slot_check(w, h, nseg, bands, tps, ns, out.ctypes.data) == 0
    return dict(zip(("rays", "bad_iterations", "bad_rays", "bad_counts", "segments"), (int(v) for v in out)))


@pytest.mark.parametrize("ns", [1, 46, 64, 130])
@pytest.mark.parametrize("tps", [1, 4])
def test_the_closed_form_slot_is_the_slot_k_raygens_packing_gives(tps, ns):
    # three tiles by two, the last column vw wide and the last row vh high: every valid rectangle of a tile, beside full tiles; with four tiles
    # per segment the second segment ends behind the image's last tile
    for vw in range(1, 9):
        for vh in range(1, 9):
            w, h = 16 + vw, 8 + vh
            nseg = (6 + tps - 1) // tps
            r = slot_check(w, h, nseg, 1, tps, ns)
            assert r["segments"] == nseg and r["rays"] == w * h * ns, (vw, vh, r)
            assert r["bad_iterations"] == 0 and r["bad_rays"] == 0 and r["bad_counts"] == 0, (vw, vh, r)


def test_the_closed_form_slot_over_bands_and_empty_segments():
    # 67 x 41 (the GPU tests' size): 9 x 6 tiles; 56 segments in 4 bands leave two segments behind the image
    for tps, nseg, bands in ((1, 56, 4), (4, 16, 4), (1, 54, 1), (2, 28, 2)):
        for ns in (1, 46, 64):
            r = slot_check(67, 41, nseg, bands, tps, ns)
            assert r["rays"] == 67 * 41 * ns and r["bad_iterations"] == 0 and r["bad_rays"] == 0 and r["bad_counts"] == 0, (tps, nseg, bands, ns, r)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_shared_trace_loop_returns_cam_trace_lists_hit_for_every_ray(monkeypatch, case):
    make, w, h = CASES[case]
    monkeypatch.setenv("EMU_WIDE6", "1")
    monkeypatch.setenv("EMU_PAIRS", "1")
    emu = emu_lib.EmuScene(make(), make_params(w, h, 1, 2), L=lib())
    j = jitters()
    for cap in (lib().cl_default_capacity(), 2):
        out = np.zeros(4, dtype=np.uint64)
        assert lib().cf_trace_check(emu.h, cap, j.ctypes.data, len(j), out.ctypes.data) == 0
        rays, mismatches, hits, flagged = (int(v) for v in out)
        print(case, cap, rays, mismatches, hits, flagged)
        assert rays == (w * h - flagged) * len(j) and mismatches == 0
        if cap > 2:
            assert flagged == 0 and hits > rays // 4


def test_host_code_runs_clean_under_asan_and_ubsan_as_a_program_of_its_own(tmp_path):
    """camfused_emu.cpp with its own main: every slot case above and the two trace loops on a small hand-made 6-wide tree.  (Nothing loaded
    into Python runs under a sanitizer.)"""
    exe = tmp_path / "camfused_emu_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-DCAMFUSED_EMU_MAIN", "-o", str(exe), SRC])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, (p.stdout[-2000:], p.stderr[-2000:])
    assert "slots: 512 cases" in p.stdout and "0 mismatches, 0 pixels left to the walk" in p.stdout
