// pt_denoise.h — first-hit AOVs and the edge-avoiding a-trous denoiser (DESIGN.md §3 "Denoiser").
//
//   stage_aov        : what one camera ray's first hit contributes to the AOV images (albedo, shading normal, distance)
//   dn_prep_pixel    : demodulation, variance, depth gradient -> the filter's per-pixel inputs (dn_prep_pixel_counts: per-pixel N)
//   dn_despeckle_pixel : the optional firefly clamp on the prep's output (pt_despeckle_options)
//   dn_iterate_pixel : one 5x5 a-trous step (SVGF's spatial filter, Dammertz et al. 2010 / Schied et al. 2017, no temporal part)
//
// Written once, as plain C++ under PT_HD: denoise.hip runs it on the device, tests/emu/denoise_emu.cpp on the host, and the two
// agree bit for bit (-ffp-contract=off, IEEE divide / sqrt, the deterministic exp2 / log2 of pt_math.h).  Taps are summed in a fixed
// order (row-major over dy, then dx).
//
// Every image is addressed as y * pitch + x with (x, y) inside W x H.  pitch = W for a whole image; a render region is
// filtered as an image of its own by passing pointers to its first pixel and the frame's width as the pitch.
//
// Per-pixel buffers of the filter (W*H vec4 each):
//   guide {n.xyz, z}  normalised mean shading normal and mean first-hit distance; z = -1 marks a BACKGROUND pixel (h < 0.5)
//   col   {I.rgb, v}  demodulated colour and its variance; v = -1 marks a pixel that is never a tap (its colour is not finite)
//   aux   {max(a, 1e-3).rgb, gz}  the remodulation albedo and the depth gradient (read for the centre pixel only)
#pragma once
#include "pt_layout.h"
#include "pt_shade.h"

namespace pt {

// ---- AOVs -------------------------------------------------------------------------------------------------------
struct AovSample { vec3 albedo, normal; float t; };
// A camera ray's first hit: ShadingContext::albedo (base texture included) and the shading normal (normal map included), exactly as
// k_shade computes them for bounce 0.
PT_HD AovSample stage_aov(const DeviceScene& S, const ShadeIn& in) {
  ShadeGeom g;
  ShadingContext ctx;
  shade_geometry(S, in, g, ctx);
  return {ctx.albedo, g.frame.z, in.t};
}
PT_HD AovSample aov_miss() { return {v3(1.0f), v3(0.0f), 0.0f}; }

PT_HD float dn_lum(vec3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
// k_accumulate's running-mean step (kernel.metal:672-684): `a` holds the mean of n samples
PT_HD vec3 aov_fold(vec3 a, vec3 x, uint32_t n) {
  if (n == 0) return x;
  return (x + a * (float)n) / (float)(n + 1);
}
PT_HD float aov_fold(float a, float x, uint32_t n) {
  if (n == 0) return x;
  return (x + a * (float)n) / (float)(n + 1);
}

// ---- filter arithmetic ------------------------------------------------------------------------------------------------
struct DenoiseParams {
  uint32_t W, H;
  float sigma_l, sigma_n, sigma_z;
};
constexpr float kDnAlbedoMin = 1e-3f;
constexpr float kDnEps = 1e-6f;
constexpr float kDnLog2e = 1.44269504088896340736f;
constexpr float kDnSigmaNormalMax = 16777216.0f;  // 2^24: what a larger pt_denoise_options.sigma_normal counts as (see dn_exp2)

// exp2_det builds 2^n from the exponent bits: valid down to n = -126.  Weights below 2^-125 are taken as 2^-125 (a NaN argument too),
// so that a tap is never dropped by an underflow and the sum never sees a denormal.  There is no upper guard: a weight's exponent is
// never positive, except sigma_n * log2(n . n') when the dot product of two unit normals rounds above 1 (by less than 2^-20), and the
// host caps sigma_n at kDnSigmaNormalMax, which keeps that product below 24.
PT_HD float dn_exp2(float y) { return exp2_det(y > -125.0f ? y : -125.0f); }
PT_HD float dn_exp(float x) { return dn_exp2(x * kDnLog2e); }
PT_HD float dn_powr(float x, float y) { return x <= 0.0f ? 0.0f : dn_exp2(y * log2_det(x)); }
PT_HD bool dn_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }

// depth of a pixel for the gradient: z = t / h of a geometry pixel; false for background
PT_HD bool dn_depth(const vec4* normal, const vec4* moments, uint32_t pitch, uint32_t x, uint32_t y, float* z) {
  const size_t p = (size_t)y * pitch + x;
  const float h = normal[p].w;
  if (!(h >= 0.5f)) return false;
  *z = moments[p].x / h;
  return true;
}

// Prep pass for pixel (x, y): `acc` = the accumulator (GMoN-resolved when GMoN is on), N = samples folded into the AOVs.
PT_HD void dn_prep_pixel(const vec4* acc, const vec4* albedo, const vec4* normal, const vec4* moments, uint32_t W, uint32_t H,
                         uint32_t pitch, uint32_t x, uint32_t y, float N, vec4* guide, vec4* col, vec4* aux) {
  const size_t p = (size_t)y * pitch + x;
  const vec4 c4 = acc[p], a4 = albedo[p], n4 = normal[p], m4 = moments[p];
  const vec3 c = v3(c4.x, c4.y, c4.z), a = v3(a4.x, a4.y, a4.z);
  const vec3 am = v3(fmaxf(a.x, kDnAlbedoMin), fmaxf(a.y, kDnAlbedoMin), fmaxf(a.z, kDnAlbedoMin));
  const vec3 I = c / am;
  const float la = fmaxf(dn_lum(a), kDnAlbedoMin);
  const float v = fmaxf(0.0f, m4.z - m4.y * m4.y) / (N * (la * la));
  float z = 0.0f, gz = 0.0f;
  const bool geo = dn_depth(normal, moments, pitch, x, y, &z);
  vec3 n = v3(0.0f);
  if (geo) {
    const vec3 nn = v3(n4.x, n4.y, n4.z);
    const float l2 = dot(nn, nn);
    if (l2 > 0.0f) n = nn / sqrtf(l2);
    // the larger absolute central difference of z in x and y; one-sided at the border and next to background
    float g[2];
    for (int axis = 0; axis < 2; axis++) {
      float zm = 0.0f, zp = 0.0f;
      const bool hm = axis == 0 ? (x > 0 && dn_depth(normal, moments, pitch, x - 1, y, &zm)) : (y > 0 && dn_depth(normal, moments, pitch, x, y - 1, &zm));
      const bool hp = axis == 0 ? (x + 1 < W && dn_depth(normal, moments, pitch, x + 1, y, &zp)) : (y + 1 < H && dn_depth(normal, moments, pitch, x, y + 1, &zp));
      g[axis] = hm && hp ? fabsf(zp - zm) * 0.5f : hp ? fabsf(zp - z) : hm ? fabsf(z - zm) : 0.0f;
    }
    gz = fmaxf(g[0], g[1]);
  }
  const bool valid = dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z) && dn_finite(I.x) && dn_finite(I.y) && dn_finite(I.z) && dn_finite(v);
  guide[p] = vec4{n.x, n.y, n.z, geo ? z : -1.0f};
  col[p] = valid ? vec4{I.x, I.y, I.z, v} : vec4{0.0f, 0.0f, 0.0f, -1.0f};
  aux[p] = vec4{am.x, am.y, am.z, gz};
}
PT_HD void dn_prep_pixel(const vec4* acc, const vec4* albedo, const vec4* normal, const vec4* moments, uint32_t W, uint32_t H,
                         uint32_t x, uint32_t y, float N, vec4* guide, vec4* col, vec4* aux) {
  dn_prep_pixel(acc, albedo, normal, moments, W, H, W, x, y, N, guide, col, aux);
}

// The prep of an adaptive render: N = the pixel's own sample count, that of its 8x8 tile (tile_n[tile_of_pixel]);
// otherwise dn_prep_pixel's arithmetic, unchanged.
// (x0, y0): where the image's first pixel lies in the frame the tiles are cut from, `pitch` that frame's width (a render region).
PT_HD void dn_prep_pixel_counts(const vec4* acc, const vec4* albedo, const vec4* normal, const vec4* moments, uint32_t W, uint32_t H,
                                uint32_t pitch, uint32_t x0, uint32_t y0, uint32_t x, uint32_t y, const uint32_t* tile_n, vec4* guide,
                                vec4* col, vec4* aux) {
  const float N = (float)tile_n[tile_of_pixel(x0 + x, y0 + y, pitch)];
  dn_prep_pixel(acc, albedo, normal, moments, W, H, pitch, x, y, N, guide, col, aux);
}
PT_HD void dn_prep_pixel_counts(const vec4* acc, const vec4* albedo, const vec4* normal, const vec4* moments, uint32_t W, uint32_t H,
                                uint32_t x, uint32_t y, const uint32_t* tile_n, vec4* guide, vec4* col, vec4* aux) {
  dn_prep_pixel_counts(acc, albedo, normal, moments, W, H, W, 0u, 0u, x, y, tile_n, guide, col, aux);
}

// 3x3 binomial blur of v at (x, y) over the valid pixels of the centre's class, normalised by the weights used
PT_HD float dn_blur_variance(const vec4* guide, const vec4* col, const DenoiseParams& P, uint32_t pitch, uint32_t x, uint32_t y, bool geo) {
  const float k3[3] = {0.25f, 0.5f, 0.25f};
  float sw = 0.0f, sv = 0.0f;
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = (int)x + dx, qy = (int)y + dy;
      if (qx < 0 || qy < 0 || qx >= (int)P.W || qy >= (int)P.H) continue;
      const size_t q = (size_t)qy * pitch + (uint32_t)qx;
      const float vq = col[q].w;
      if (!(vq >= 0.0f) || (guide[q].w >= 0.0f) != geo) continue;
      const float w = k3[dx + 1] * k3[dy + 1];
      sw += w;
      sv += w * vq;
    }
  return sv / sw;  // (the centre is always used)
}

// The firefly clamp at pixel (x, y), between the prep and the first a-trous step (DESIGN.md §3a "Firefly clamp"): a valid pixel whose
// luminance exceeds `threshold` times the brightest of its 3x3 neighbours (valid, of its own class, inside W x H; row-major over dy,
// then dx) is scaled down to that limit, its variance kept.  Every other pixel is copied.  Reads col_in only.
PT_HD void dn_despeckle_pixel(const vec4* guide, const vec4* col_in, vec4* col_out, const DenoiseParams& P, uint32_t pitch, uint32_t x,
                              uint32_t y, float threshold) {
  const size_t p = (size_t)y * pitch + x;
  const vec4 cp = col_in[p];
  if (!(cp.w >= 0.0f)) { col_out[p] = cp; return; }  // not finite: never a tap, keeps its value
  const bool geo = guide[p].w >= 0.0f;
  bool any = false;
  float M = 0.0f;
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      if (dx == 0 && dy == 0) continue;
      const int qx = (int)x + dx, qy = (int)y + dy;
      if (qx < 0 || qy < 0 || qx >= (int)P.W || qy >= (int)P.H) continue;
      const size_t q = (size_t)qy * pitch + (uint32_t)qx;
      const vec4 cq = col_in[q];
      if (!(cq.w >= 0.0f) || (guide[q].w >= 0.0f) != geo) continue;
      const float lq = dn_lum(v3(cq.x, cq.y, cq.z));
      if (!any || lq > M) M = lq;
      any = true;
    }
  vec4 o = cp;
  if (any) {
    const float L = dn_lum(v3(cp.x, cp.y, cp.z)), lim = threshold * M;
    if (L > lim && L > 0.0f) {
      const float k = lim / L;
      o = vec4{cp.x * k, cp.y * k, cp.z * k, cp.w};
    }
  }
  col_out[p] = o;
}

// One a-trous step at pixel (x, y) with step `s`.  `last`: remodulate, out[p] = colour (alpha 1); `acc` supplies the value of a pixel
// that is not a tap.  Otherwise col_out[p] = {I', v'}.
PT_HD void dn_iterate_pixel(const vec4* guide, const vec4* aux, const vec4* col_in, vec4* col_out, const vec4* acc, vec4* out,
                            const DenoiseParams& P, uint32_t pitch, uint32_t x, uint32_t y, uint32_t s, bool last) {
  const size_t p = (size_t)y * pitch + x;
  const vec4 cp = col_in[p];
  if (!(cp.w >= 0.0f)) {  // not finite: keeps its value, never a tap
    if (last) { const vec4 c = acc[p]; out[p] = vec4{c.x, c.y, c.z, 1.0f}; }
    else col_out[p] = cp;
    return;
  }
  const vec4 gp = guide[p];
  const bool geo = gp.w >= 0.0f;
  const vec3 np = v3(gp.x, gp.y, gp.z);
  const float gz = aux[p].w;
  const float lp = dn_lum(v3(cp.x, cp.y, cp.z));
  const float dl = P.sigma_l * sqrtf(dn_blur_variance(guide, col_in, P, pitch, x, y, geo)) + kDnEps;
  const float k5[5] = {1.0f / 16.0f, 0.25f, 0.375f, 0.25f, 1.0f / 16.0f};
  float sw = 0.0f, sv = 0.0f;
  vec3 sI = v3(0.0f);
  for (int dy = -2; dy <= 2; dy++)
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = (int)x + dx * (int)s, qy = (int)y + dy * (int)s;
      if (qx < 0 || qy < 0 || qx >= (int)P.W || qy >= (int)P.H) continue;
      const size_t q = (size_t)qy * pitch + (uint32_t)qx;
      const vec4 cq = col_in[q];
      if (!(cq.w >= 0.0f)) continue;
      const vec4 gq = guide[q];
      if ((gq.w >= 0.0f) != geo) continue;
      float wn = 1.0f, wz = 1.0f;
      if (geo) {
        wn = dn_powr(fmaxf(0.0f, dot(np, v3(gq.x, gq.y, gq.z))), P.sigma_n);
        const float dist = sqrtf((float)(dx * dx + dy * dy));
        wz = dn_exp(-(fabsf(gp.w - gq.w) / (((P.sigma_z * gz) * (float)s) * dist + kDnEps)));
      }
      const float wl = dn_exp(-(fabsf(lp - dn_lum(v3(cq.x, cq.y, cq.z))) / dl));
      const float w = (((k5[dx + 2] * k5[dy + 2]) * wn) * wz) * wl;
      sw += w;
      sI = sI + v3(cq.x, cq.y, cq.z) * w;
      sv += (w * w) * cq.w;
    }
  vec3 I = v3(cp.x, cp.y, cp.z);
  float v = cp.w;
  if (sw > 0.0f) { I = sI / sw; v = sv / (sw * sw); }
  if (last) {
    const vec4 a = aux[p];
    out[p] = vec4{I.x * a.x, I.y * a.y, I.z * a.z, 1.0f};
  } else {
    col_out[p] = vec4{I.x, I.y, I.z, v};
  }
}
PT_HD void dn_iterate_pixel(const vec4* guide, const vec4* aux, const vec4* col_in, vec4* col_out, const vec4* acc, vec4* out,
                            const DenoiseParams& P, uint32_t x, uint32_t y, uint32_t s, bool last) {
  dn_iterate_pixel(guide, aux, col_in, col_out, acc, out, P, P.W, x, y, s, last);
}

}  // namespace pt
