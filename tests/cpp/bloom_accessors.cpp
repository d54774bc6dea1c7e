// TEST PROGRAM (tests/): bloom through include/ptamd_renderer.hpp and the C ABI without a GPU — the defaults, the struct layouts, the
// accessor's type, pt_plan_bloom, and the order of pt_set_bloom_options' checks (the options before the renderer).  tests/test_bloom_host.py
// compiles and runs it; it returns 0 when everything holds.
#include <cstddef>
#include <type_traits>

#include "ptamd_renderer.hpp"

using ptamd::renderer_pt::Renderer;

static_assert(sizeof(pt_bloom_options) == 24 && offsetof(pt_bloom_options, levels) == 20, "pt_bloom_options");
static_assert(sizeof(pt_bloom_plan) == 164 && offsetof(pt_bloom_plan, width) == 8 && offsetof(pt_bloom_plan, offset) == 112, "pt_bloom_plan");
static_assert(std::is_same<decltype(std::declval<Renderer&>().bloomOptions()), pt_bloom_options&>::value, "bloomOptions() hands out the struct itself");

int main() {
  pt_bloom_options o;
  pt_default_bloom_options(&o);
  if (o.enabled != 0u || o.intensity != 0.05f || o.threshold != 0.0f || o.knee != 0.0f || o.scatter != 1.0f || o.levels != 6u) return 2;
  o.enabled = 1u; o.intensity = 0.25f; o.levels = 10u;
  Renderer* r = nullptr;
  if (r) {   // (compiled, not run: no GPU here)
    pt_bloom_options& b = r->bloomOptions();
    b = o;
    if (r->bloomOptions().levels != 10u) return 3;
  }
  if (pt_set_bloom_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 4;   // valid options, no renderer
  o.scatter = 0.0f;
  if (pt_set_bloom_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 5;
  pt_bloom_plan p;
  if (pt_plan_bloom(256u, 128u, 6u, &p) != PT_OK || p.levels != 6u || p.total_texels != 10920u || p.width[6] != 4u || p.height[6] != 2u) return 6;
  if (pt_plan_bloom(1u, 1u, 6u, &p) != PT_OK || p.levels != 0u || p.total_texels != 0u) return 7;
  return 0;
}
