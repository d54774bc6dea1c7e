// TEST HARNESS ONLY (tests/emu) — the host build of bloom (platinum_amd/csrc/pt_bloom.h) as bloom.hip runs it, level by level: bright
// pass and down, down, up in place, composite; for tests/test_bloom_host.py and tests/test_gpu_bloom.py.
// Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// A translation unit of its own: tests/bloom_lib.py builds it into tests/_build/libptamd_bloom.so (tests/host_build.py load).
// With -DBLOOM_EMU_MAIN it is a stand-alone program that blooms random and special-value cards at the tests' sizes (a sanitizer build
// runs it).
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../platinum_amd/csrc/pt_bloom.h"

using namespace pt;

extern "C" {

void bl_host_plan(uint32_t W, uint32_t H, uint32_t levels, pt_bloom_plan* out) { bloom_plan(W, H, levels, out); }
float bl_host_norm(uint32_t L, float scatter) { return bloom_norm(L, scatter); }
// 1 when pt_set_bloom_options would accept the options
uint32_t bl_host_options_valid(const pt_bloom_options* o) { return bloom_options_error(*o) == nullptr; }
void bl_host_bright(const float* rgba, const pt_bloom_options* o, float* out3) {
  const vec3 b = bloom_bright(vec4{rgba[0], rgba[1], rgba[2], rgba[3]}, o->threshold, o->knee);
  out3[0] = b.x; out3[1] = b.y; out3[2] = b.z;
}

// The bloom of a W x H RGBA32F image into `out`; pyramid_out (may be null) receives U_1..U_L as the plan lays them out, 4 floats per
// texel with .w = 0.  `enabled` is not looked at.
void bl_host_bloom(const float* rgba, uint32_t W, uint32_t H, const pt_bloom_options* o, float* out, float* pyramid_out) {
  const vec4* img = (const vec4*)rgba;
  vec4* dst = (vec4*)out;
  pt_bloom_plan plan;
  bloom_plan(W, H, o->levels, &plan);
  const uint32_t L = plan.levels;
  const size_t npix = (size_t)W * H;
  if (L == 0) {
    for (size_t p = 0; p < npix; p++) dst[p] = img[p];
    return;
  }
  std::vector<vec3> pyr(plan.total_texels);
  auto level = [&](uint32_t l) { return pyr.data() + plan.offset[l]; };
  {  // D_1 from the bright pass of the frame
    vec3* d = level(1);
    const uint32_t dw = plan.width[1], dh = plan.height[1];
    for (uint32_t y = 0; y < dh; y++)
      for (uint32_t x = 0; x < dw; x++)
        d[(size_t)y * dw + x] = bloom_down_texel([&](uint32_t ux, uint32_t uy) { return bloom_bright(img[(size_t)uy * W + ux], o->threshold, o->knee); }, W, H, x, y);
  }
  for (uint32_t l = 1; l < L; l++) {
    const vec3* s = level(l);
    vec3* d = level(l + 1);
    const uint32_t sw = plan.width[l], sh = plan.height[l], dw = plan.width[l + 1], dh = plan.height[l + 1];
    for (uint32_t y = 0; y < dh; y++)
      for (uint32_t x = 0; x < dw; x++) d[(size_t)y * dw + x] = bloom_down_texel([&](uint32_t ux, uint32_t uy) { return s[(size_t)uy * sw + ux]; }, sw, sh, x, y);
  }
  for (uint32_t l = L; l-- > 1u;) {  // U_l over D_l, l = L-1..1
    vec3* f = level(l);
    const vec3* c = level(l + 1);
    const uint32_t fw = plan.width[l], fh = plan.height[l], cw = plan.width[l + 1], ch = plan.height[l + 1];
    for (uint32_t y = 0; y < fh; y++)
      for (uint32_t x = 0; x < fw; x++) {
        const vec3 up = bloom_up_texel([&](uint32_t ux, uint32_t uy) { return c[(size_t)uy * cw + ux]; }, cw, ch, x, y);
        f[(size_t)y * fw + x] = bloom_combine(f[(size_t)y * fw + x], up, o->scatter);
      }
  }
  const float norm = bloom_norm(L, o->scatter);
  const vec3* u1 = level(1);
  const uint32_t cw = plan.width[1], ch = plan.height[1];
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++) {
      const vec3 up = bloom_up_texel([&](uint32_t ux, uint32_t uy) { return u1[(size_t)uy * cw + ux]; }, cw, ch, x, y);
      dst[(size_t)y * W + x] = bloom_composite(img[(size_t)y * W + x], up, norm, *o);
    }
  if (pyramid_out)
    for (size_t e = 0; e < pyr.size(); e++) { pyramid_out[4 * e] = pyr[e].x; pyramid_out[4 * e + 1] = pyr[e].y; pyramid_out[4 * e + 2] = pyr[e].z; pyramid_out[4 * e + 3] = 0.0f; }
}

// sizeof / offsetof of both structs as this compiler lays them out
void bl_host_layout(uint32_t out[14]) {
  uint32_t k = 0;
  out[k++] = sizeof(pt_bloom_options);
  out[k++] = offsetof(pt_bloom_options, enabled); out[k++] = offsetof(pt_bloom_options, intensity); out[k++] = offsetof(pt_bloom_options, threshold);
  out[k++] = offsetof(pt_bloom_options, knee); out[k++] = offsetof(pt_bloom_options, scatter); out[k++] = offsetof(pt_bloom_options, levels);
  out[k++] = sizeof(pt_bloom_plan);
  out[k++] = offsetof(pt_bloom_plan, levels); out[k++] = offsetof(pt_bloom_plan, total_texels);
  out[k++] = offsetof(pt_bloom_plan, width); out[k++] = offsetof(pt_bloom_plan, height); out[k++] = offsetof(pt_bloom_plan, offset);
  out[k++] = PT_BLOOM_MAX_LEVELS;
}

}  // extern "C"

#ifdef BLOOM_EMU_MAIN
int main() {
  const uint32_t sizes[][2] = {{1, 1}, {2, 1}, {1, 7}, {3, 2}, {16, 16}, {17, 15}, {33, 31}, {67, 45}, {256, 128}, {8192, 1}};
  const pt_bloom_options sets[] = {{1u, 0.05f, 0.0f, 0.0f, 1.0f, 6u}, {1u, 0.05f, 1.0f, 0.5f, 0.6f, 4u}, {1u, 1.0f, 0.5f, 0.0f, 1.0f, 12u},
                                   {1u, 0.05f, 0.0f, 0.0f, 1.0f, 1u}, {1u, 0.05f, 0.0f, 0.0f, 1.0f, 2u}};
  uint32_t s = 12345u;
  for (const auto& wh : sizes)
    for (const auto& o : sets) {
      const uint32_t W = wh[0], H = wh[1];
      std::vector<float> img((size_t)W * H * 4), out(img.size());
      for (float& v : img) { s = s * 1664525u + 1013904223u; v = pp_exp2s((float)(s >> 8) * (14.0f / 16777216.0f) - 8.0f); }
      if (W * H > 4) { img[4] = u2f(0x7fc00000u); img[9] = kInf; img[14] = -1.0f; }   // a NaN, an infinity, a negative channel
      pt_bloom_plan plan;
      bloom_plan(W, H, o.levels, &plan);
      std::vector<float> pyr((size_t)plan.total_texels * 4 + 4);
      bl_host_bloom(img.data(), W, H, &o, out.data(), pyr.data());
      double sum = 0.0;
      uint32_t bad = 0;
      for (size_t p = 0; p < (size_t)W * H; p++) {
        for (int c = 0; c < 3; c++) { if (bloom_finite(out[4 * p + c])) sum += out[4 * p + c]; else bad++; }
        if (f2u(out[4 * p + 3]) != f2u(img[4 * p + 3])) return 1;
      }
      printf("%u x %u, %u levels (%u texels): sum %g, %u non-finite channels\n", W, H, plan.levels, plan.total_texels, sum, bad);
      if (bad > 2u) return 1;
    }
  return 0;
}
#endif
