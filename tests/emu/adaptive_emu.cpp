// TEST HARNESS ONLY (tests/emu) — the host build of the adaptive-sampling criterion (platinum_amd/csrc/pt_adaptive.h) and of the
// denoiser's prep with per-pixel sample counts (pt_denoise.h dn_prep_pixel_counts), for tests/test_adaptive_host.py and
// tests/test_gpu_adaptive.py.  Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// Third part of tests/emu/host_harness.cpp, after denoise_emu.cpp; not compiled alone.
#ifndef PTAMD_TESTS_EMU_ADAPTIVE_EMU
#define PTAMD_TESTS_EMU_ADAPTIVE_EMU
#include "../../platinum_amd/csrc/pt_adaptive.h"
#include "../../platinum_amd/csrc/pt_tilefold.h"

extern "C" {

// adaptive_error of `count` pixels after n samples
void ad_host_error(const float* m1, const float* m2, size_t count, uint32_t n, float* err) {
  for (size_t i = 0; i < count; i++) err[i] = adaptive_error(m1[i], m2[i], n);
}

// The verdict of every 8x8 tile of a W*H PT_AOV_MOMENTS image (g, b = m1, m2) after n samples, as k_adaptive_check reaches it:
// converged[tile] = 1 when every pixel of the tile inside the image passes adaptive_pixel_converged.
void ad_host_tiles(const float* moments, uint32_t W, uint32_t H, uint32_t n, float threshold, uint8_t* converged) {
  for (uint32_t t = 0; t < tile_count(W, H); t++) converged[t] = 1;
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++) {
      const float* m = moments + 4 * ((size_t)y * W + x);
      if (!adaptive_pixel_converged(m[1], m[2], n, threshold)) converged[tile_of_pixel(x, y, W)] = 0;
    }
}

// The filter of an adaptive render (launch_denoise with tile counts): dn_prep_pixel_counts, then the a-trous steps as dn_host_filter.
// counts: W*H per-pixel sample counts (pt_read_sample_counts); every pixel of a tile holds the same count.
void ad_host_filter_counts(const float* acc, const float* albedo, const float* normal, const float* moments, uint32_t W, uint32_t H,
                           const uint32_t* counts, uint32_t iterations, float sigma_l, float sigma_n, float sigma_z, float* out) {
  const size_t npix = (size_t)W * H;
  const vec4* a = (const vec4*)acc;
  vec4* o = (vec4*)out;
  if (iterations == 0) {
    for (size_t p = 0; p < npix; p++) o[p] = vec4{a[p].x, a[p].y, a[p].z, 1.0f};
    return;
  }
  std::vector<uint32_t> tile_n(tile_count(W, H));
  for (uint32_t t = 0; t < tile_n.size(); t++) {   // every pixel of a tile holds the same count: take its first (lane 0 is inside the image)
    const PixelXY p = fold_tile<false>(t, 0, W, H, nullptr, nullptr, Rect{}).q;
    tile_n[t] = counts[(size_t)p.y * W + p.x];
  }
  std::vector<vec4> guide(npix), aux(npix), col0(npix), col1(npix);
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++)
      dn_prep_pixel_counts(a, (const vec4*)albedo, (const vec4*)normal, (const vec4*)moments, W, H, x, y, tile_n.data(), guide.data(), col0.data(),
                           aux.data());
  DenoiseParams P;
  P.W = W; P.H = H; P.sigma_l = sigma_l; P.sigma_n = sigma_n; P.sigma_z = sigma_z;
  vec4* cin = col0.data();
  vec4* cout = col1.data();
  for (uint32_t i = 0; i < iterations; i++) {
    for (uint32_t y = 0; y < H; y++)
      for (uint32_t x = 0; x < W; x++) dn_iterate_pixel(guide.data(), aux.data(), cin, cout, a, o, P, x, y, 1u << i, i + 1 == iterations);
    std::swap(cin, cout);
  }
}

// sizeof / offsetof of pt_adaptive_options as this compiler lays it out
void ad_host_options_layout(uint32_t out[5]) {
  out[0] = sizeof(pt_adaptive_options);
  out[1] = offsetof(pt_adaptive_options, enabled);
  out[2] = offsetof(pt_adaptive_options, threshold);
  out[3] = offsetof(pt_adaptive_options, min_spp);
  out[4] = offsetof(pt_adaptive_options, interval);
}

}  // extern "C"

#endif  // PTAMD_TESTS_EMU_ADAPTIVE_EMU
