// pt_sky.h — sun and sky: a single-scattering atmosphere as a lat-long environment map.
//
//   sky_options_error : pt_generate_sky's test of its options and size
//   sky_setup         : options and size -> SkyParams, what every texel shares (the sun's direction, alpha_eff and its chords); host
//   sky_coverage      : the 4 x 4 sub-texel coverage of the disc in sixteenths, with the early-out that changes no bit
//   sky_solid_angle   : Omega_d and the count of covered texels, in double over the rows that can hold coverage; host
//   sky_texel         : one texel's rgba
//
// Written once, as plain C++ under PT_HD: sky.hip runs sky_texel on the device, tests/emu/sky_emu.cpp on the host.  fp32,
// -ffp-contract=off, every sum in the order written here, the transcendentals pt_math.h's: the two agree bit for bit.
//
// Numerical care (|p|^2 is about 4e7 km^2; no height or chord comes from a difference of such squares):
//   height along a ray from radius r (height h) with cosine mu, at distance t:  w = t (t + 2 r mu);  h' = h + w / (sqrt(r r + w) + r)
//   radius there:                                                             sqrt(r r + w)   (relative error 1e-7: chords only)
//   impact parameter of a ray:                                                sn = sqrt((1 - mu)(1 + mu));  q = r sn
//   its clearance of a sphere R, from the height and not from q:              R - q = (R - r) + r mu mu / (1 + sn), with R - r = -h for the
//                                                                             ground and (Ra - Rg) - h for the top (q itself is rounded
//                                                                             to half a metre; a ray just under the horizon clears the
//                                                                             ground by less)
//   the ray meets the ground:                                                 mu < 0 and Rg - q > 0
//   chord to a sphere R >= r from inside:                                     -r mu + sqrt((R - q)(R + q))
//   distance to the ground from outside:                                      h (r + Rg) / (-r mu + sqrt((Rg - q)(Rg + q)))
//   the disc's test d.s >= cos(alpha) as |d - s|^2 <= (2 sin(alpha / 2))^2     (1 - d.s = |d - s|^2 / 2 for unit vectors; cos(alpha) itself
//                                                                             resolves a 0.27 degree disc to 0.3 % of its radius in fp32)
#pragma once
#include <math.h>

#include "pt_shade.h"

namespace pt {

constexpr float kSkyRg = 6360.0f, kSkyRa = 6460.0f;
constexpr float kSkyBetaR[3] = {5.802e-3f, 13.558e-3f, 33.1e-3f};
constexpr float kSkyBetaMs = 3.996e-3f, kSkyBetaMe = 8.396e-3f;
constexpr float kSkyBetaO[3] = {0.650e-3f, 1.881e-3f, 0.085e-3f};
constexpr float kSkyHR = 8.0f, kSkyHM = 1.2f, kSkyG = 0.8f;
constexpr int kSkyNV = 32, kSkyNL = 8;
constexpr float kSkyLog2e = 1.44269504088896340736f;

// what the texels of one map share
struct SkyParams {
  vec3 s;                       // towards the sun
  float r0, h0;                 // the observer's radius and height
  float air, dust, ozone, albedo, intensity;
  float chord2, chord2_near;    // (2 sin(alpha_eff / 2))^2; the same for alpha_eff + a texel's width and height: no coverage beyond
  float omega;                  // (float)Omega_d; 0: no disc is drawn
  float alpha_eff;
  uint32_t w, h;
};

PT_HD bool sky_finite(float v) { return fabsf(v) <= 3.4028234e38f; }   // false for a NaN

PT_HD const char* sky_options_error(const pt_sky_options& o, uint32_t width, uint32_t height) {
  if (!(o.sun_elevation >= -1.57079637f && o.sun_elevation <= 1.57079637f)) return "-pi/2 <= sun_elevation <= pi/2 is required";
  if (!sky_finite(o.sun_azimuth)) return "sun_azimuth must be finite";
  if (!(o.sun_angular_radius > 0.0f && o.sun_angular_radius <= 0.2f)) return "0 < sun_angular_radius <= 0.2 is required";
  if (!(o.sun_intensity >= 0.0f && sky_finite(o.sun_intensity))) return "sun_intensity must be finite and >= 0";
  if (o.sun_disc > 1u) return "sun_disc is 0 or 1";
  if (!(o.altitude_km >= 0.001f && o.altitude_km <= 60.0f)) return "0.001 <= altitude_km <= 60 is required";
  if (!(o.air_density >= 0.0f && o.air_density <= 10.0f)) return "0 <= air_density <= 10 is required";
  if (!(o.dust_density >= 0.0f && o.dust_density <= 10.0f)) return "0 <= dust_density <= 10 is required";
  if (!(o.ozone_density >= 0.0f && o.ozone_density <= 10.0f)) return "0 <= ozone_density <= 10 is required";
  if (!(o.ground_albedo >= 0.0f && o.ground_albedo <= 1.0f)) return "0 <= ground_albedo <= 1 is required";
  if (width == 0u || height == 0u || (uint64_t)width * height > (1ull << 26)) return "the image must hold 1..2^26 texels";
  return nullptr;
}

// (host) The azimuth is reduced modulo 2 pi in double before sincos_det sees it: any finite value is in its domain.
inline SkyParams sky_setup(const pt_sky_options& o, uint32_t w, uint32_t h) {
  SkyParams P;
  const float a = (float)fmod((double)o.sun_azimuth, 6.283185307179586476925);
  float sa, ca, se, ce;
  sincos_det(a, &sa, &ca);
  sincos_det(o.sun_elevation, &se, &ce);
  P.s = v3(-ca * ce, se, -sa * ce);
  P.r0 = kSkyRg + o.altitude_km;
  P.h0 = o.altitude_km;
  P.air = o.air_density; P.dust = o.dust_density; P.ozone = o.ozone_density; P.albedo = o.ground_albedo; P.intensity = o.sun_intensity;
  P.alpha_eff = fmaxf(o.sun_angular_radius, kPi / (float)h);
  float sh, chh;
  sincos_det(0.5f * P.alpha_eff, &sh, &chh);
  P.chord2 = (2.0f * sh) * (2.0f * sh);
  const float near = fminf(P.alpha_eff + (2.0f * kPi / (float)w + kPi / (float)h), kPi);
  sincos_det(0.5f * near, &sh, &chh);
  P.chord2_near = (2.0f * sh) * (2.0f * sh);
  P.omega = 0.0f;
  P.w = w; P.h = h;
  return P;
}

PT_HD vec3 sky_texel_dir(const SkyParams& P, uint32_t x, uint32_t y, float fx, float fy) {
  return uvToRayDir(vec2{((float)x + fx) / (float)P.w, ((float)y + fy) / (float)P.h});
}

// Sixteenths of the texel's 4 x 4 sub-texel directions inside the disc.  A texel whose centre lies beyond alpha_eff plus a whole texel's
// width and height holds none (its sub-texel directions lie within 3/8 of both): skipped without looking.
PT_HD uint32_t sky_coverage(const SkyParams& P, uint32_t x, uint32_t y, vec3 d) {
  if (!(length_squared(d - P.s) <= P.chord2_near)) return 0u;
  uint32_t n = 0;
  for (int j = 0; j < 4; j++)
    for (int i = 0; i < 4; i++) {
      const vec3 ds = sky_texel_dir(P, x, y, ((float)i + 0.5f) * 0.25f, ((float)j + 0.5f) * 0.25f);
      n += length_squared(ds - P.s) <= P.chord2 ? 1u : 0u;
    }
  return n;
}

// (host) Omega_d = sum of c_k omega_k with omega_k = (2 pi / w)(cos theta_top - cos theta_bottom), in double, over the rows within
// alpha_eff (and a row more) of the sun's; *texels counts the texels with coverage.
inline double sky_solid_angle(const SkyParams& P, uint32_t* texels) {
  const double pi = 3.14159265358979323846;
  const double ts = acos(fmin(fmax((double)P.s.y, -1.0), 1.0));
  const double lo = floor((ts - (double)P.alpha_eff) / pi * (double)P.h) - 1.0, hi = floor((ts + (double)P.alpha_eff) / pi * (double)P.h) + 1.0;
  const uint32_t y0 = lo < 0.0 ? 0u : (uint32_t)lo, y1 = hi >= (double)P.h ? P.h - 1u : (uint32_t)hi;
  double omega = 0.0;
  uint32_t count = 0;
  for (uint32_t y = y0; y <= y1 && y < P.h; y++) {
    const double wk = (2.0 * pi / (double)P.w) * (cos(pi * (double)y / (double)P.h) - cos(pi * (double)(y + 1u) / (double)P.h));
    uint64_t row = 0;
    for (uint32_t x = 0; x < P.w; x++) {
      const uint32_t c = sky_coverage(P, x, y, sky_texel_dir(P, x, y, 0.5f, 0.5f));
      row += c;
      count += c ? 1u : 0u;
    }
    omega += (double)row / 16.0 * wk;
  }
  *texels = count;
  return omega;
}

// exp(-x) for x >= 0 through exp2_det, 0 where the exponent leaves its domain
PT_HD float sky_exp_neg(float x) {
  const float y = x * kSkyLog2e;
  return y > 126.0f ? 0.0f : exp2_det(-y);
}

// the densities (Rayleigh, Mie, ozone) at height h >= 0
PT_HD vec3 sky_density(const SkyParams& P, float h) {
  return v3(P.air * sky_exp_neg(h / kSkyHR), P.dust * sky_exp_neg(h / kSkyHM), P.ozone * fmaxf(0.0f, 1.0f - fabsf(h - 25.0f) / 15.0f));
}

// T(tau), per channel
PT_HD vec3 sky_transmittance(vec3 tau) {
  return v3(sky_exp_neg((kSkyBetaR[0] * tau.x + kSkyBetaMe * tau.y) + kSkyBetaO[0] * tau.z),
            sky_exp_neg((kSkyBetaR[1] * tau.x + kSkyBetaMe * tau.y) + kSkyBetaO[1] * tau.z),
            sky_exp_neg((kSkyBetaR[2] * tau.x + kSkyBetaMe * tau.y) + kSkyBetaO[2] * tau.z));
}

// a point of a ray that starts at radius r, height h with cosine mu to the zenith, at distance t: its height (>= 0) and radius
PT_HD void sky_along(float r, float h, float mu, float t, float* h_out, float* r_out) {
  const float w = t * (t + (2.0f * r) * mu);
  const float rr = sqrtf(r * r + w);
  *h_out = fmaxf(h + w / (rr + r), 0.0f);
  *r_out = rr;
}

// A ray from radius r, height h, cosine mu: (Rg - q)(Rg + q) and (Ra - q)(Ra + q), the squared half-chords of the ground and of the top
// (the first is positive exactly when the ray's line passes under the ground sphere).
struct SkyChords { float ground2, top2; };
PT_HD SkyChords sky_chords(float r, float h, float mu) {
  const float sn = sqrtf((1.0f - mu) * (1.0f + mu));
  const float q = r * sn, e = r * (mu * mu) / (1.0f + sn);
  return {(e - h) * (kSkyRg + q), (((kSkyRa - kSkyRg) - h) + e) * (kSkyRa + q)};
}

// The sun's optical depth D(p) from a point at radius r, height h, with cosine mu between the zenith there and the sun; *blocked when the
// ray meets the ground sphere (D is still computed: the caller selects).
PT_HD vec3 sky_sun_depth(const SkyParams& P, float r, float h, float mu, bool* blocked) {
  const SkyChords c = sky_chords(r, h, mu);
  *blocked = mu < 0.0f && c.ground2 > 0.0f;
  const float l = -r * mu + sqrtf(fmaxf(c.top2, 0.0f));
  const float dl = l / (float)kSkyNL;
  vec3 D = v3(0.0f);
  for (int j = 0; j < kSkyNL; j++) {
    float hj, rj;
    sky_along(r, h, mu, ((float)j + 0.5f) * dl, &hj, &rj);
    D = D + sky_density(P, hj) * dl;
  }
  return D;
}

// `flags` (tests; null on the device) receives the texel's decisions: bit 0 ground, bit 1 + i blocked at view step i, bit 33 blocked at the
// ray's end.
PT_HD vec4 sky_texel(const SkyParams& P, uint32_t x, uint32_t y, uint64_t* flags = nullptr) {
  const vec3 d = sky_texel_dir(P, x, y, 0.5f, 0.5f);
  const float mu0 = d.y, mu = dot(d, P.s);
  // where the view ray ends
  const SkyChords c0 = sky_chords(P.r0, P.h0, mu0);
  const bool ground = mu0 < 0.0f && c0.ground2 > 0.0f;
  const float t_top = -P.r0 * mu0 + sqrtf(fmaxf(c0.top2, 0.0f));
  const float t_ground = P.h0 * (P.r0 + kSkyRg) / (-P.r0 * mu0 + sqrtf(fmaxf(c0.ground2, 0.0f)));
  const float t_end = ground ? t_ground : t_top;
  const float ds = t_end / (float)kSkyNV;
  vec3 tau = v3(0.0f), AR = v3(0.0f), AM = v3(0.0f);
  uint64_t seen = ground ? 1u : 0u;
  for (int i = 0; i < kSkyNV; i++) {
    const float t = ((float)i + 0.5f) * ds;
    float hi, ri;
    sky_along(P.r0, P.h0, mu0, t, &hi, &ri);
    const vec3 rho = sky_density(P, hi);
    const float mus = (P.r0 * P.s.y + t * mu) / ri;   // p.s / |p|
    bool blocked;
    const vec3 D = sky_sun_depth(P, ri, hi, fminf(fmaxf(mus, -1.0f), 1.0f), &blocked);
    const vec3 m = tau + (0.5f * rho) * ds;
    const vec3 T = sky_transmittance(m + D);
    const float lit = blocked ? 0.0f : 1.0f;
    if (flags && blocked) seen |= 2ull << i;
    AR = AR + T * ((rho.x * ds) * lit);
    AM = AM + T * ((rho.y * ds) * lit);
    tau = tau + rho * ds;
  }
  const float PR = (3.0f / (16.0f * kPi)) * (1.0f + mu * mu);
  const float gb = (1.0f + kSkyG * kSkyG) - (2.0f * kSkyG) * mu;
  const float PM = (1.0f - kSkyG * kSkyG) / ((4.0f * kPi) * (gb * sqrtf(gb)));
  const vec3 bR = v3(kSkyBetaR[0], kSkyBetaR[1], kSkyBetaR[2]);
  vec3 L = P.intensity * ((bR * PR) * AR + (kSkyBetaMs * PM) * AM);
  const vec3 Tv = sky_transmittance(tau);
  {  // the ground (selected, not branched on: every lane of a wave runs the same trip counts)
    float he, re;
    sky_along(P.r0, P.h0, mu0, t_end, &he, &re);
    const float ns = (P.r0 * P.s.y + t_end * mu) / re;
    bool blocked;
    const vec3 D = sky_sun_depth(P, re, he, fminf(fmaxf(ns, -1.0f), 1.0f), &blocked);
    const float c = (ground && !blocked) ? fmaxf(ns, 0.0f) : 0.0f;
    if (flags) *flags = seen | (blocked ? 1ull << 33 : 0ull);
    L = L + (Tv * ((P.albedo / kPi) * P.intensity)) * (sky_transmittance(D) * c);
  }
  if (P.omega > 0.0f && !ground) {   // the disc: a handful of texels, and wave-uniform away from them
    const uint32_t cov = sky_coverage(P, x, y, d);
    if (cov) L = L + (((float)cov * 0.0625f) * P.intensity) * Tv / P.omega;
  }
  const float big = 3.4028234e38f;
  return vec4{fminf(L.x, big), fminf(L.y, big), fminf(L.z, big), 1.0f};
}

}  // namespace pt
