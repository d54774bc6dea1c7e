// TEST HARNESS ONLY (tests/emu) — the host build of the pass views (platinum_amd/csrc/pt_view.h): the range pass and the view pass over host
// images, as pt_debug_view runs them on the device; for tests/test_view_host.py and tests/test_gpu_view.py.
// Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// A translation unit of its own: tests/view_lib.py builds it into tests/_build/libptamd_view.so (tests/host_build.py load).
// With -DVIEW_EMU_MAIN it is a stand-alone program that drives every view over edge values (a sanitizer build runs it).
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../platinum_amd/csrc/pt_view.h"

using namespace pt;

namespace {

// what view_pixel fetches of pixel p of the host images
struct HostPx {
  const pt_view_inputs* in;
  size_t p;
  vec4 normal() const { const float* n = in->normal + 4 * p; return vec4{n[0], n[1], n[2], n[3]}; }
  vec3 moments() const { const float* m = in->moments + 4 * p; return vec3{m[0], m[1], m[2]}; }
  float alpha() const { return in->film[4 * p + 3]; }
  void slots(MatteSlots& m) const {
    for (uint32_t k = 0; k < kMatteSlots; k++) { m.id[k] = in->slots[p * kMatteSlots + k].id; m.count[k] = in->slots[p * kMatteSlots + k].count; }
  }
};

}  // namespace

extern "C" {

// pt_debug_view on the host: the range over rect = {x0, y0, x1, y1} (DEPTH only), then every pixel of the W x H image
void view_host_pass(const pt_view_inputs* in, uint32_t W, uint32_t H, const uint32_t* rect, const pt_view_options* o, uint32_t* rgba8_out,
                    pt_view_stats* stats) {
  const ViewParams P = view_params(*o, in->spp);
  ViewRecord rec{0u, 0u, 0u, 0u};
  if (o->view == PT_VIEW_DEPTH)
    for (uint32_t y = rect[1]; y < rect[3]; y++)
      for (uint32_t x = rect[0]; x < rect[2]; x++) {
        const size_t p = (size_t)y * W + x;
        float d;
        if (view_depth(in->moments[4 * p], in->normal[4 * p + 3], in->counts[p], &d)) view_range_fold(rec, view_depth_key(d));
      }
  float z0 = 0.0f, z1 = 0.0f;
  if (o->view == PT_VIEW_DEPTH) view_range(P, rec, &z0, &z1);
  for (size_t p = 0; p < (size_t)W * H; p++) rgba8_out[p] = view_pixel(P, z0, z1, in->counts[p], HostPx{in, p});
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->shown = o->view;
    if (o->view == PT_VIEW_DEPTH) { stats->depth_pixels = rec.count; stats->depth_min = z0; stats->depth_max = z1; }
  }
}

uint32_t view_host_hash(uint32_t x) { return view_hash(x); }

// 1 when pt_set_view_options would accept the options
uint32_t view_host_options_valid(const pt_view_options* o) { return view_options_error(*o) == nullptr; }

uint32_t view_host_shown(uint32_t view, int aov, int film, int matte, int adaptive, int merged) {
  return view_shown(view, aov != 0, film != 0, matte != 0, adaptive != 0, merged != 0);
}

// sizeof / offsetof of the structs as this compiler lays them out
void view_host_layout(uint32_t out[24]) {
  uint32_t k = 0;
  out[k++] = sizeof(pt_view_options);
  out[k++] = offsetof(pt_view_options, view); out[k++] = offsetof(pt_view_options, layer); out[k++] = offsetof(pt_view_options, ramp);
  out[k++] = offsetof(pt_view_options, auto_range); out[k++] = offsetof(pt_view_options, depth_min); out[k++] = offsetof(pt_view_options, depth_max);
  out[k++] = offsetof(pt_view_options, noise_max); out[k++] = offsetof(pt_view_options, _pad);
  out[k++] = sizeof(pt_view_stats);
  out[k++] = offsetof(pt_view_stats, shown); out[k++] = offsetof(pt_view_stats, depth_pixels); out[k++] = offsetof(pt_view_stats, depth_min);
  out[k++] = offsetof(pt_view_stats, depth_max);
  out[k++] = sizeof(pt_view_inputs);
  out[k++] = offsetof(pt_view_inputs, albedo); out[k++] = offsetof(pt_view_inputs, normal); out[k++] = offsetof(pt_view_inputs, moments);
  out[k++] = offsetof(pt_view_inputs, film); out[k++] = offsetof(pt_view_inputs, slots); out[k++] = offsetof(pt_view_inputs, counts);
  out[k++] = offsetof(pt_view_inputs, spp);
  while (k < 24) out[k++] = 0;
}

}  // extern "C"

#ifdef VIEW_EMU_MAIN
int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  // a 7 x 3 card: depths with NaN, infinity, h = 0, -0, a negative one; n in {0, 1, 2, many}; slots full, empty and of the background
  const uint32_t W = 7, H = 3, npix = W * H;
  std::vector<float> normal(npix * 4), moments(npix * 4), film(npix * 4);
  std::vector<pt_matte_slot> slots((size_t)npix * PT_MATTE_SLOTS);
  std::vector<uint32_t> counts(npix), out(npix);
  const float depths[] = {1.0f, 2.5f, nan, inf, -0.0f, -1.0f, 1000.0f};
  const uint32_t ns[] = {0u, 1u, 2u, 64u, 4000000000u};
  for (uint32_t p = 0; p < npix; p++) {
    const float h = p % 5 == 3 ? 0.0f : 0.5f + 0.5f * (float)(p % 2);
    normal[4 * p] = (float)(p % 3) - 1.0f; normal[4 * p + 1] = p == 4 ? nan : 0.25f; normal[4 * p + 2] = -0.5f; normal[4 * p + 3] = h;
    moments[4 * p] = depths[p % 7] * h; moments[4 * p + 1] = 0.5f * (float)(p % 4); moments[4 * p + 2] = p == 9 ? nan : 0.3f * (float)(p % 5);
    film[4 * p + 3] = p == 2 ? nan : (float)p / (float)(npix - 1) * 1.25f - 0.125f;
    counts[p] = ns[p % 5];
    for (uint32_t k = 0; k < PT_MATTE_SLOTS; k++) {
      pt_matte_slot& s = slots[(size_t)p * PT_MATTE_SLOTS + k];
      s.id = k == 2 ? PT_MATTE_NONE : p * 31u + k;
      s.count = (p % 3 == 0 || k < p % 4) ? 1u + k : 0u;
      if (s.count == 0u) s.id = PT_MATTE_NONE;
    }
  }
  pt_view_inputs in{nullptr, normal.data(), moments.data(), film.data(), slots.data(), counts.data(), 64u};
  const uint32_t rects[][4] = {{0, 0, W, H}, {1, 1, 4, 2}, {3, 0, 4, 1}};
  for (uint32_t view = PT_VIEW_NORMAL; view < PT_VIEW_COUNT; view++)
    for (uint32_t ramp = PT_RAMP_GREY; ramp <= PT_RAMP_HEAT; ramp++)
      for (uint32_t autor = 0; autor < 2; autor++)
        for (const auto& rc : rects) {
          pt_view_options o{view, view % 2u, ramp, autor, 0.5f, 900.0f, 0.05f, 0u};
          if (view_options_error(o)) return 2;
          pt_view_stats st;
          view_host_pass(&in, W, H, rc, &o, out.data(), &st);
          for (uint32_t p = 0; p < npix; p++) {
            if ((out[p] >> 24) != 255u) return 3;
            if (counts[p] == 0u && out[p] != 0xff000000u) return 4;
          }
          if (st.shown != view) return 5;
          if (view == PT_VIEW_DEPTH && !(st.depth_min <= st.depth_max && std::isfinite(st.depth_max))) return 6;
          if (view == PT_VIEW_DEPTH && rc[2] - rc[0] == 1u) printf("depth rect 1x1 auto %u: %u pixels, %g .. %g\n", autor, st.depth_pixels, st.depth_min, st.depth_max);
        }
  // the ramp at its stops, past them and at NaN
  const float vs[] = {0.0f, 0.25f, 0.5f, 0.75f, 1.0f, 0.999999f, 1e-30f, nan};
  for (float v : vs) {
    const vec3 g = view_ramp(PT_RAMP_GREY, v), c = view_ramp(PT_RAMP_HEAT, v);
    if (v == v && g.x != v) return 7;
    if (!(c.x >= 0.0f && c.x <= 1.0f && c.y >= 0.0f && c.y <= 1.0f && c.z >= 0.0f && c.z <= 1.0f)) return 8;
  }
  if (pp_pack_rgba8(view_ramp(PT_RAMP_HEAT, 0.0f)) != 0xffff0000u || pp_pack_rgba8(view_ramp(PT_RAMP_HEAT, 1.0f)) != 0xff0000ffu ||
      pp_pack_rgba8(view_ramp(PT_RAMP_HEAT, nan)) != 0xff0000ffu || pp_pack_rgba8(view_ramp(PT_RAMP_HEAT, 0.5f)) != 0xff00ff00u)
    return 9;
  printf("hash(0) = %08x, hash(1) = %08x, hash(0xfffffffe) = %08x\n", view_hash(0u), view_hash(1u), view_hash(0xfffffffeu));
  pt_view_options bad{PT_VIEW_COUNT, 0u, 0u, 1u, 0.0f, 1.0f, 0.1f, 0u};
  if (!view_options_error(bad)) return 10;
  bad.view = PT_VIEW_DEPTH; bad.auto_range = 0u; bad.depth_max = inf;
  if (!view_options_error(bad)) return 11;
  bad.depth_max = 1.0f; bad.noise_max = nan;
  if (!view_options_error(bad)) return 12;
  return 0;
}
#endif
