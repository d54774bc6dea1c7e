// TEST HARNESS ONLY (tests/emu) — the host build of the denoiser's firefly clamp (platinum_amd/csrc/pt_denoise.h dn_despeckle_pixel) and of
// the whole filter with it, as denoise.hip launch_denoise runs it, for tests/test_despeckle_host.py and tests/test_gpu_despeckle.py.
// Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// A translation unit of its own: tests/despeckle_lib.py builds it into tests/_build/libptamd_despeckle.so (tests/host_build.py load).
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../platinum_amd/csrc/pt_denoise.h"

using namespace pt;

namespace {

// launch_denoise's steps up to the first a-trous one over the rectangle `rect` of a W x H frame: the prep (per-tile counts when tile_n is
// given), then the clamp when enabled.  Every pointer addresses the rectangle's first pixel; returns the buffer the a-trous steps start from.
vec4* prep_and_clamp(const vec4* acc, const vec4* albedo, const vec4* normal, const vec4* moments, const DenoiseParams& P, uint32_t pitch,
                     uint32_t x0, uint32_t y0, float N, const uint32_t* tile_n, uint32_t enabled, float threshold, vec4* guide, vec4* aux,
                     vec4* col0, vec4* col1) {
  for (uint32_t y = 0; y < P.H; y++)
    for (uint32_t x = 0; x < P.W; x++) {
      if (tile_n) dn_prep_pixel_counts(acc, albedo, normal, moments, P.W, P.H, pitch, x0, y0, x, y, tile_n, guide, col0, aux);
      else dn_prep_pixel(acc, albedo, normal, moments, P.W, P.H, pitch, x, y, N, guide, col0, aux);
    }
  if (!enabled) return col0;
  for (uint32_t y = 0; y < P.H; y++)
    for (uint32_t x = 0; x < P.W; x++) dn_despeckle_pixel(guide, col0, col1, P, pitch, x, y, threshold);
  return col1;
}

}  // namespace

extern "C" {

// prep -> clamp of a whole W x H image with a uniform sample count: col_out (W*H*4 floats) = {I.rgb, v} as the first a-trous step reads it
void ds_host_stage(const float* acc, const float* albedo, const float* normal, const float* moments, uint32_t W, uint32_t H, uint32_t N,
                   uint32_t enabled, float threshold, float* col_out) {
  const size_t npix = (size_t)W * H;
  std::vector<vec4> guide(npix), aux(npix), col0(npix), col1(npix);
  DenoiseParams P{};
  P.W = W; P.H = H;
  const vec4* c = prep_and_clamp((const vec4*)acc, (const vec4*)albedo, (const vec4*)normal, (const vec4*)moments, P, W, 0u, 0u, (float)N, nullptr,
                                 enabled, threshold, guide.data(), aux.data(), col0.data(), col1.data());
  vec4* o = (vec4*)col_out;
  for (size_t p = 0; p < npix; p++) o[p] = c[p];
}

// The filter as launch_denoise runs it: dn_host_filter's arguments, then the clamp's options, the rectangle {x0, y0, x1, y1} of the frame
// that is filtered as an image of its own (null: the whole frame) and the samples folded into each 8x8 tile of the frame (null: N
// everywhere).  Every image is W*H*4 floats; `out` is written inside the rectangle only.
void ds_host_filter(const float* acc, const float* albedo, const float* normal, const float* moments, uint32_t W, uint32_t H, uint32_t N,
                    uint32_t iterations, float sigma_l, float sigma_n, float sigma_z, float* out, uint32_t enabled, float threshold,
                    const uint32_t* rect, const uint32_t* tile_n) {
  const uint32_t pitch = W, x0 = rect ? rect[0] : 0u, y0 = rect ? rect[1] : 0u;
  const size_t npix = (size_t)W * H, org = (size_t)y0 * pitch + x0;
  DenoiseParams P;
  P.W = rect ? rect[2] - rect[0] : W; P.H = rect ? rect[3] - rect[1] : H;
  P.sigma_l = sigma_l; P.sigma_n = sigma_n; P.sigma_z = sigma_z;
  const vec4* a = (const vec4*)acc + org;
  vec4* o = (vec4*)out + org;
  if (iterations == 0) {
    for (uint32_t y = 0; y < P.H; y++)
      for (uint32_t x = 0; x < P.W; x++) {
        const size_t p = (size_t)y * pitch + x;
        o[p] = vec4{a[p].x, a[p].y, a[p].z, 1.0f};
      }
    return;
  }
  std::vector<vec4> guide(npix), aux(npix), col0(npix), col1(npix);
  vec4* g = guide.data() + org;
  vec4* ax = aux.data() + org;
  vec4* c0 = col0.data() + org;
  vec4* c1 = col1.data() + org;
  vec4* cin = prep_and_clamp(a, (const vec4*)albedo + org, (const vec4*)normal + org, (const vec4*)moments + org, P, pitch, x0, y0, (float)N,
                             tile_n, enabled, threshold, g, ax, c0, c1);
  vec4* cout = cin == c0 ? c1 : c0;
  for (uint32_t i = 0; i < iterations; i++) {
    for (uint32_t y = 0; y < P.H; y++)
      for (uint32_t x = 0; x < P.W; x++) dn_iterate_pixel(g, ax, cin, cout, a, o, P, pitch, x, y, 1u << i, i + 1 == iterations);
    std::swap(cin, cout);
  }
}

// sizeof / offsetof of pt_despeckle_options as this compiler lays it out
void ds_host_options_layout(uint32_t out[3]) {
  out[0] = sizeof(pt_despeckle_options);
  out[1] = offsetof(pt_despeckle_options, enabled);
  out[2] = offsetof(pt_despeckle_options, threshold);
}

}  // extern "C"
