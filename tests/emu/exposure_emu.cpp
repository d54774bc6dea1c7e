// TEST HARNESS ONLY (tests/emu) — the host build of the auto-exposure meter (platinum_amd/csrc/pt_exposure.h) as exposure.hip runs it:
// histogram over a rectangle, resolve, apply; for tests/test_exposure_host.py and tests/test_gpu_exposure.py.
// Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// A translation unit of its own: tests/exposure_lib.py builds it into tests/_build/libptamd_exposure.so (tests/host_build.py load).
// With -DEXPOSURE_EMU_MAIN it is a stand-alone program that meters a special-value card and a random card (a sanitizer build runs it).
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../platinum_amd/csrc/pt_exposure.h"

using namespace pt;

extern "C" {

// The meter of the rectangle rect = {x0, y0, x1, y1} (null: the whole image) of a W x H RGBA32F image: the record, and (scaled_out may be
// null) the whole image * gain.  prev_ev / has_prev: the smoothing state the resolve starts from.
void ex_host_meter(const float* rgba, uint32_t W, uint32_t H, const uint32_t* rect, const pt_exposure_options* o, float prev_ev, uint32_t has_prev,
                   pt_exposure_meter* out, float* scaled_out) {
  const vec4* img = (const vec4*)rgba;
  const uint32_t x0 = rect ? rect[0] : 0u, y0 = rect ? rect[1] : 0u, x1 = rect ? rect[2] : W, y1 = rect ? rect[3] : H;
  pt_exposure_meter m{};
  uint32_t* counters = (uint32_t*)&m;
  for (uint32_t y = y0; y < y1; y++)
    for (uint32_t x = x0; x < x1; x++) counters[exposure_pixel_key(img[(size_t)y * W + x])]++;
  exposure_resolve(&m, *o, prev_ev, has_prev);
  *out = m;
  if (scaled_out) {
    vec4* s = (vec4*)scaled_out;
    for (size_t p = 0; p < (size_t)W * H; p++) s[p] = exposure_apply(img[p], m.gain);
  }
}

// the resolve alone, on counters the caller filled in
void ex_host_resolve(pt_exposure_meter* m, const pt_exposure_options* o, float prev_ev, uint32_t has_prev) { exposure_resolve(m, *o, prev_ev, has_prev); }

uint32_t ex_host_classify(float Y) { return exposure_classify(Y); }
float ex_host_lum(float r, float g, float b) { return dn_lum(v3(r, g, b)); }
float ex_host_exp2s(float x) { return pp_exp2s(x); }
// 1 when pt_set_exposure_options would accept the options
uint32_t ex_host_options_valid(const pt_exposure_options* o) { return exposure_options_error(*o) == nullptr; }

// sizeof / offsetof of both structs as this compiler lays them out
void ex_host_layout(uint32_t out[20]) {
  uint32_t k = 0;
  out[k++] = sizeof(pt_exposure_options);
  out[k++] = offsetof(pt_exposure_options, enabled); out[k++] = offsetof(pt_exposure_options, target_log2);
  out[k++] = offsetof(pt_exposure_options, low_fraction); out[k++] = offsetof(pt_exposure_options, high_fraction);
  out[k++] = offsetof(pt_exposure_options, min_ev); out[k++] = offsetof(pt_exposure_options, max_ev);
  out[k++] = offsetof(pt_exposure_options, smoothing);
  out[k++] = sizeof(pt_exposure_meter);
  out[k++] = offsetof(pt_exposure_meter, bins); out[k++] = offsetof(pt_exposure_meter, below); out[k++] = offsetof(pt_exposure_meter, above);
  out[k++] = offsetof(pt_exposure_meter, nonfinite); out[k++] = offsetof(pt_exposure_meter, metered); out[k++] = offsetof(pt_exposure_meter, kept);
  out[k++] = offsetof(pt_exposure_meter, weighted); out[k++] = offsetof(pt_exposure_meter, mean_log2); out[k++] = offsetof(pt_exposure_meter, target_ev);
  out[k++] = offsetof(pt_exposure_meter, ev); out[k++] = offsetof(pt_exposure_meter, gain);
}

}  // extern "C"

#ifdef EXPOSURE_EMU_MAIN
int main() {
  pt_exposure_options o{};
  o.target_log2 = -2.4739313f; o.low_fraction = 0.10f; o.high_fraction = 0.95f; o.min_ev = -16.0f; o.max_ev = 16.0f;
  // the special-value card: the range's edges, zero, a negative, a denormal, NaN, +-inf, a huge finite rgb (counted `above`)
  const float big = 3.0e38f;
  std::vector<float> vals = {1.52587890625e-05f, u2f(f2u(1.52587890625e-05f) - 1u), u2f(f2u(65536.0f) - 1u), 65536.0f, 0.0f, -1.0f, 1.0e-40f,
                             u2f(0x7fc00000u), kInf, -kInf};
  std::vector<float> card;
  for (float v : vals) { card.insert(card.end(), {v, v, v, 1.0f}); }
  card.insert(card.end(), {big, big, big, 1.0f});
  for (uint32_t b = 0; b < 256; b++) {   // both edges of every bin
    const float lo = u2f((b + 888u) << 20), hi = u2f(((b + 889u) << 20) - 1u);
    card.insert(card.end(), {lo, lo, lo, 0.0f});
    card.insert(card.end(), {hi, hi, hi, 0.0f});
  }
  const uint32_t n = (uint32_t)(card.size() / 4);
  pt_exposure_meter m;
  std::vector<float> scaled(card.size());
  ex_host_meter(card.data(), n, 1u, nullptr, &o, 0.0f, 0u, &m, scaled.data());
  printf("special card: %u pixels, metered %u below %u above %u nonfinite %u, ev %g gain %g\n", n, m.metered, m.below, m.above, m.nonfinite, m.ev, m.gain);
  if (m.metered + m.below + m.above + m.nonfinite != n) return 1;
  // a log-uniform random card, a rectangle of it, with a smoothing state
  const uint32_t W = 67, H = 45;
  std::vector<float> rnd((size_t)W * H * 4);
  uint32_t s = 12345u;
  for (float& v : rnd) { s = s * 1664525u + 1013904223u; v = pp_exp2s((float)(s >> 8) * (40.0f / 16777216.0f) - 20.0f); }
  const uint32_t rect[4] = {3, 2, 14, 9};
  o.smoothing = 0.5f;
  scaled.resize(rnd.size());
  ex_host_meter(rnd.data(), W, H, rect, &o, 1.0f, 1u, &m, scaled.data());
  printf("random card: metered %u kept %u weighted %llu mean_log2 %g ev %g\n", m.metered, m.kept, (unsigned long long)m.weighted, m.mean_log2, m.ev);
  if (m.metered + m.below + m.above + m.nonfinite != 11u * 7u) return 1;
  ex_host_meter(rnd.data(), W, H, nullptr, &o, 0.0f, 0u, &m, nullptr);
  return m.metered + m.below + m.above + m.nonfinite == W * H ? 0 : 1;
}
#endif
