// TEST HARNESS ONLY (tests/emu) — the one translation unit of tests/_build/libptamd_host.so: the host build of the product's stage
// functions and index maps (platinum_amd/csrc/*.h, plain C++ under PT_HD) behind a C interface for the tests' ctypes wrappers
// (tests/emu_lib.py, denoise_lib.py, adaptive_lib.py, region_lib.py, test_layout_host.py, test_start_plan_host.py) and for bench.py's cpu_baseline.
// tests/host_build.py compiles it, once per change of any file it is made of.  Not part of libptamd.so, never loaded by platinum_amd,
// not a fallback.  The parts come in this order (a later one may use what an earlier one defines); their exported names do not clash:
#include "wavefront_emu.cpp"  // emu_*: host scene + BVH, the per-path loop, emu_render
#include "denoise_emu.cpp"    // dn_*:  the denoiser's arithmetic, first-hit AOVs, the render that folds them
#include "adaptive_emu.cpp"   // ad_*:  the adaptive-sampling criterion, the filter with per-pixel counts
#include "region_emu.cpp"     // rg_*:  pt_render_region's layout, the rectangle test
#include "layout_probe.cpp"   // lp_*:  the tile / segment / radiance-buffer index maps, plan_queues
#include "math_emu.cpp"       // emu_math_batch: the math layer as pt_debug_math evaluates it
#include "light_emu.cpp"      // emu_light_probe: the light sampling as pt_debug_lights evaluates it
#include "shade_emu.cpp"      // emu_shade_probe: the shading frame and context as pt_debug_shading evaluates them
#include "start_plan_probe.cpp"  // sp_*: the decisions of pt_start_render (host_scene.h): structure, camera lists, queue budget
