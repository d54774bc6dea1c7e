// TEST PROGRAM (tests/): ambient occlusion through include/ptamd_renderer.hpp and the C ABI without a GPU — the defaults, the struct layouts,
// the accessors' types, and the order of the entry points' checks (the options before the renderer).  tests/test_ao_cpp.py compiles and runs
// it; it returns 0 when everything holds.
#include <cstddef>
#include <cstdint>
#include <limits>
#include <type_traits>
#include <vector>

#include "ptamd_renderer.hpp"

using ptamd::renderer_pt::Renderer;

static_assert(sizeof(pt_ao_options) == 16 && offsetof(pt_ao_options, enabled) == 0 && offsetof(pt_ao_options, distance) == 4, "pt_ao_options");
static_assert(sizeof(pt_ao_stats) == 16 && offsetof(pt_ao_stats, rays) == 0 && offsetof(pt_ao_stats, ms_trace) == 8 && offsetof(pt_ao_stats, ms_fold) == 12,
              "pt_ao_stats");
static_assert(PT_ABI_VERSION == 5u, "an additive extension: the version stays");
static_assert(std::is_same<decltype(std::declval<Renderer&>().ambientOcclusionOptions()), pt_ao_options&>::value,
              "ambientOcclusionOptions() hands out the struct itself");
static_assert(std::is_same<decltype(std::declval<const Renderer&>().readbackAmbientOcclusion()), std::vector<float>>::value, "W*H floats");
static_assert(std::is_same<decltype(std::declval<const Renderer&>().readbackAmbientOcclusionCounts()), std::vector<uint32_t>>::value, "W*H*2 words");

int main() {
  pt_ao_options o;
  o.enabled = 7u; o.distance = 7.0f; o._pad[0] = o._pad[1] = 7u;
  pt_default_ao_options(&o);
  if (o.enabled != 0u || o.distance != 1.0f || o._pad[0] != 0u || o._pad[1] != 0u) return 2;
  pt_default_ao_options(nullptr);
  Renderer* r = nullptr;
  if (r) {   // (compiled, not run: no GPU here)
    pt_ao_options& a = r->ambientOcclusionOptions();
    a = o;
    a.enabled = 1u;
    a.distance = std::numeric_limits<float>::infinity();
    r->setAmbientOcclusionOptions(a);
    if (!r->readbackAmbientOcclusion().empty() || !r->readbackAmbientOcclusionCounts().empty()) return 3;
    std::vector<float> origins, directions;
    std::vector<uint32_t> state;
    if (r->debugAmbientOcclusion(0u, origins, directions, state)) return 4;
  }
  if (pt_set_ao_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 5;   // valid options, no renderer
  if (pt_set_ao_options(nullptr, nullptr) != PT_ERR_INVALID_ARGUMENT) return 6;
  o.enabled = 2u;
  if (pt_set_ao_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 7;
  o.enabled = 1u;
  const float bad[4] = {0.0f, -1.0f, std::numeric_limits<float>::quiet_NaN(), -std::numeric_limits<float>::infinity()};
  for (float d : bad) {
    o.distance = d;
    if (pt_set_ao_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 8;
  }
  float px[3];
  uint32_t w[2];
  pt_ao_stats st;
  if (pt_read_ao(nullptr, px) != PT_ERR_INVALID_ARGUMENT) return 9;
  if (pt_read_ao_counts(nullptr, w) != PT_ERR_INVALID_ARGUMENT) return 10;
  if (pt_debug_ao(nullptr, 0u, px, px, w) != PT_ERR_INVALID_ARGUMENT) return 11;
  if (pt_get_ao_stats(nullptr, &st) != PT_ERR_INVALID_ARGUMENT) return 12;
  return 0;
}
