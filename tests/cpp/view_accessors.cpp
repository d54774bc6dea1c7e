// TEST PROGRAM (tests/): pass views through include/ptamd_renderer.hpp and the C ABI without a GPU — the defaults, the struct layouts, the
// accessors' types, and the order of the entry points' checks (the options before the renderer).  tests/test_view_cpp.py compiles and runs
// it; it returns 0 when everything holds.
#include <cstddef>
#include <cstdint>
#include <limits>
#include <type_traits>

#include "ptamd_renderer.hpp"

using ptamd::renderer_pt::Renderer;

static_assert(sizeof(pt_view_options) == 32 && offsetof(pt_view_options, view) == 0 && offsetof(pt_view_options, layer) == 4 &&
                  offsetof(pt_view_options, ramp) == 8 && offsetof(pt_view_options, auto_range) == 12 && offsetof(pt_view_options, depth_min) == 16 &&
                  offsetof(pt_view_options, depth_max) == 20 && offsetof(pt_view_options, noise_max) == 24 && offsetof(pt_view_options, _pad) == 28,
              "pt_view_options");
static_assert(sizeof(pt_view_stats) == 16 && offsetof(pt_view_stats, shown) == 0 && offsetof(pt_view_stats, depth_pixels) == 4 &&
                  offsetof(pt_view_stats, depth_min) == 8 && offsetof(pt_view_stats, depth_max) == 12,
              "pt_view_stats");
static_assert(offsetof(pt_view_inputs, albedo) == 0 && offsetof(pt_view_inputs, normal) == sizeof(void*) && offsetof(pt_view_inputs, counts) == 5 * sizeof(void*) &&
                  offsetof(pt_view_inputs, spp) == 6 * sizeof(void*),
              "pt_view_inputs");
static_assert(PT_VIEW_BEAUTY == 0 && PT_VIEW_ALBEDO == 1 && PT_VIEW_NORMAL == 2 && PT_VIEW_DEPTH == 3 && PT_VIEW_ALPHA == 4 && PT_VIEW_MATTE == 5 &&
                  PT_VIEW_SAMPLES == 6 && PT_VIEW_NOISE == 7 && PT_VIEW_COUNT == 8 && PT_RAMP_GREY == 0 && PT_RAMP_HEAT == 1,
              "the views and the ramps");
static_assert(std::is_same<decltype(std::declval<Renderer&>().viewOptions()), pt_view_options&>::value, "viewOptions() hands out the struct itself");
static_assert(std::is_same<decltype(std::declval<const Renderer&>().viewStats()), pt_view_stats>::value, "viewStats() returns the struct");

int main() {
  pt_view_options o;
  o.view = o.layer = o.ramp = o.auto_range = o._pad = 7u;
  o.depth_min = o.depth_max = o.noise_max = 7.0f;
  pt_default_view_options(&o);
  if (o.view != PT_VIEW_BEAUTY || o.layer != PT_MATTE_INSTANCE || o.ramp != PT_RAMP_GREY || o.auto_range != 1u || o._pad != 0u) return 2;
  if (o.depth_min != 0.0f || o.depth_max != 1.0f || o.noise_max != 0.1f) return 3;
  pt_default_view_options(nullptr);
  Renderer* r = nullptr;
  if (r) {   // (compiled, not run: no GPU here)
    pt_view_options& v = r->viewOptions();
    v = o;
    v.view = PT_VIEW_MATTE;
    v.layer = PT_MATTE_MATERIAL;
    if (r->viewStats().shown != PT_VIEW_MATTE) return 4;
  }
  if (pt_set_view_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 5;   // valid options, no renderer
  if (pt_set_view_options(nullptr, nullptr) != PT_ERR_INVALID_ARGUMENT) return 6;
  const pt_view_options good = o;
  o.view = PT_VIEW_COUNT;
  if (pt_set_view_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 7;
  o = good; o.ramp = 2u;
  if (pt_set_view_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 8;
  o = good; o.auto_range = 0u; o.depth_max = std::numeric_limits<float>::infinity();
  if (pt_set_view_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 9;
  o = good; o.noise_max = 0.0f;
  if (pt_set_view_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 10;
  pt_view_stats st;
  if (pt_read_view_stats(nullptr, &st) != PT_ERR_INVALID_ARGUMENT) return 11;
  uint32_t counts[1] = {1u};
  uint8_t px[4];
  pt_view_inputs in{};
  in.counts = counts; in.spp = 1u;
  o = good; o.view = PT_VIEW_SAMPLES;
  if (pt_debug_view(nullptr, &in, 1u, 1u, nullptr, &o, px, &st) != PT_ERR_INVALID_ARGUMENT) return 12;
  o.view = PT_VIEW_BEAUTY;
  if (pt_debug_view(nullptr, &in, 1u, 1u, nullptr, &o, px, nullptr) != PT_ERR_INVALID_ARGUMENT) return 13;
  return 0;
}
