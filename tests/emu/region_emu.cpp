// TEST HARNESS ONLY (tests/emu) — how this compiler lays out pt_render_region (include/ptamd.h), and the host build of the rectangle
// arithmetic of platinum_amd/csrc/pt_layout.h, for tests/test_region_host.py.  Not part of libptamd.so, never loaded by platinum_amd.
// Fourth part of tests/emu/host_harness.cpp; not compiled alone.
#ifndef PTAMD_TESTS_EMU_REGION_EMU
#define PTAMD_TESTS_EMU_REGION_EMU
#include <cstddef>
#include <cstdint>

#include "../../include/ptamd.h"
#include "../../platinum_amd/csrc/pt_layout.h"

extern "C" {

// sizeof / offsetof of pt_render_region
void rg_host_region_layout(uint32_t out[6]) {
  out[0] = sizeof(pt_render_region);
  out[1] = offsetof(pt_render_region, enabled);
  out[2] = offsetof(pt_render_region, x0);
  out[3] = offsetof(pt_render_region, y0);
  out[4] = offsetof(pt_render_region, x1);
  out[5] = offsetof(pt_render_region, y1);
}

// rect_contains over a W x H image: inside[y * W + x]
void rg_host_mask(uint32_t W, uint32_t H, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint8_t* inside) {
  const pt::Rect r{x0, y0, x1, y1};
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++) inside[(size_t)y * W + x] = pt::rect_contains(r, x, y) ? 1 : 0;
}

}  // extern "C"

#endif  // PTAMD_TESTS_EMU_REGION_EMU
