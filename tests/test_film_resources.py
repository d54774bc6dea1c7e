"""The build of the film kernels (film.hip), no GPU: scratch, spills and LDS as tools/kernel_resources.sh reports them for the Makefile's
flags.  k_accumulate_film stages eight samples of a tile's Lbuf (16 B) and Fbuf (4 B) entries through LDS with kFoldRow = 9 slots per pixel:
64 * 9 * 20 B = 11520 B, which must be what the build holds (the kernel that was measured is the one that stages); neither fold may touch
scratch or spill, and the three per-ray / per-pixel kernels use no LDS at all."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_film_kernels_stay_inside_their_budget():
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh")], capture_output=True, text=True, timeout=600).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"(.+?) VGPRs (\d+) scratch (\d+) spill (\d+) occ (\d+) LDS (\d+)", line.strip())
        if m:
            seen[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    for name in ("k_accumulate_film", "k_accumulate_film_adaptive", "k_film_flags", "k_film_compose", "k_film_alpha"):
        assert name in seen, sorted(seen)
        vgprs, scratch, spill, occ, lds = seen[name]
        print(name, "VGPRs %d scratch %d spill %d occ %d LDS %d" % seen[name])
        assert scratch == 0 and spill == 0, (name, seen[name])
        if name.startswith("k_accumulate_film"):
            assert lds == 64 * 9 * (16 + 4), (name, seen[name])
            assert vgprs <= 128, (name, seen[name])        # (four waves per SIMD at least: the LDS of one-wave blocks allows no more)
        else:
            assert lds == 0 and vgprs <= 64, (name, seen[name])
