// TEST HARNESS ONLY (tests/emu) — the host build of the sun-and-sky generator (platinum_amd/csrc/pt_sky.h) as pt_generate_sky runs it:
// the options' test, sky_setup, Omega_d on the host, sky_texel per texel; for tests/test_sky_host.py, tests/test_gpu_sky.py and
// tools/sky_timing.py.  Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// A translation unit of its own: tests/sky_lib.py builds it into tests/_build/libptamd_sky.so (tests/host_build.py load);
// tests/cpp/sky_check.cpp includes it into a stand-alone program (a sanitizer build runs that).
#include <cstddef>
#include <cstdint>

#include "../../platinum_amd/csrc/pt_sky.h"

using namespace pt;

extern "C" {

// 1 when pt_generate_sky would accept the options and the size
uint32_t sk_host_valid(const pt_sky_options* o, uint32_t w, uint32_t h) { return sky_options_error(*o, w, h) == nullptr; }

// pt_generate_sky without the renderer: the image (w * h * 4 floats), the stats (kernel_ms = 0; may be null) and, per texel, the decisions
// sky_texel took (flags_out may be null: bit 0 ground, bit 1 + i blocked at view step i, bit 33 blocked at the ray's end).  -1 for what
// pt_generate_sky refuses.
int sk_host_generate(const pt_sky_options* o, uint32_t w, uint32_t h, float* rgba_out, pt_sky_stats* stats_out, uint64_t* flags_out) {
  if (!o || !rgba_out || sky_options_error(*o, w, h)) return -1;
  SkyParams P = sky_setup(*o, w, h);
  uint32_t texels = 0;
  const double omega = sky_solid_angle(P, &texels);
  P.omega = o->sun_disc ? (float)omega : 0.0f;
  vec4* out = (vec4*)rgba_out;
  for (uint32_t y = 0; y < h; y++)
    for (uint32_t x = 0; x < w; x++) {
      const size_t i = (size_t)y * w + x;
      out[i] = sky_texel(P, x, y, flags_out ? flags_out + i : nullptr);
    }
  if (stats_out) {
    stats_out->sun_direction[0] = P.s.x; stats_out->sun_direction[1] = P.s.y; stats_out->sun_direction[2] = P.s.z;
    stats_out->sun_radius_used = P.alpha_eff;
    stats_out->sun_solid_angle = omega;
    stats_out->sun_texels = texels;
    stats_out->kernel_ms = 0.0f;
  }
  return 0;
}

// the coverage of every texel in sixteenths, as the kernel and Omega_d count it
void sk_host_coverage(const pt_sky_options* o, uint32_t w, uint32_t h, uint32_t* out) {
  const SkyParams P = sky_setup(*o, w, h);
  for (uint32_t y = 0; y < h; y++)
    for (uint32_t x = 0; x < w; x++) out[(size_t)y * w + x] = sky_coverage(P, x, y, sky_texel_dir(P, x, y, 0.5f, 0.5f));
}

// sizeof / offsetof of both structs as this compiler lays them out
void sk_host_layout(uint32_t out[17]) {
  uint32_t k = 0;
  out[k++] = sizeof(pt_sky_options);
  out[k++] = offsetof(pt_sky_options, sun_elevation); out[k++] = offsetof(pt_sky_options, sun_azimuth); out[k++] = offsetof(pt_sky_options, sun_angular_radius);
  out[k++] = offsetof(pt_sky_options, sun_intensity); out[k++] = offsetof(pt_sky_options, sun_disc); out[k++] = offsetof(pt_sky_options, altitude_km);
  out[k++] = offsetof(pt_sky_options, air_density); out[k++] = offsetof(pt_sky_options, dust_density); out[k++] = offsetof(pt_sky_options, ozone_density);
  out[k++] = offsetof(pt_sky_options, ground_albedo);
  out[k++] = sizeof(pt_sky_stats);
  out[k++] = offsetof(pt_sky_stats, sun_direction); out[k++] = offsetof(pt_sky_stats, sun_radius_used); out[k++] = offsetof(pt_sky_stats, sun_solid_angle);
  out[k++] = offsetof(pt_sky_stats, sun_texels); out[k++] = offsetof(pt_sky_stats, kernel_ms);
}

}  // extern "C"
