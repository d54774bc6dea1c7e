// TEST PROGRAM (tests/test_shade_early_host.py builds and runs it; it has its own main and is never loaded into Python).
// The energy-table lookups of platinum_amd/csrc/pt_bsdf.h are split into fetch and resolve, and the shading chain of pt_shade.h issues the
// fetches of a hit together (shade_issue / shade_land).  This program holds both to what they replace, bit for bit:
//   (a) lut_resolve(lutN_fetch(...)) against a local copy of the one-piece lut1 / lut2 / lut3 formulas;
//   (b) the phased chain (BSDF(ctx, flags, luts); fetchDir(wo.z); fetchDir(wi.z); setWo(resolve); eval(wo, wi, terms); sample) against
//       the plain calls (BSDF(ctx, flags, luts, wo); eval(wo, wi); sample(wo, r, rc)), whose every lookup is fetched where it is used.
// Built with g++ -ffp-contract=off; a second build adds -fsanitize=address,undefined and must exit clean as well.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../platinum_amd/csrc/pt_shade.h"

using namespace pt;

namespace {

uint32_t hash32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
struct Rng {
  uint32_t s;
  uint32_t next() { s = s * 747796405u + 2891336453u; return hash32(s); }
  float unit() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }  // [0, 1)
  float range(float a, float b) { return a + (b - a) * unit(); }
};

// ---- the one-piece formulas the split replaces (the build's filtering definition: clamp to edge, x = c N - 0.5, i0 = floor x, taps clamped
//      to [0, N-1], a + (b - a) w; x, then y, then z) -------------------------------------------------------------------------------------
void ref_axis(float c, int n, int* i0, int* i1, float* w) {
  const float x = c * (float)n - 0.5f;
  const float fl = std::floor(x);
  *w = x - fl;
  // (every coordinate of the grid below keeps floor(x) inside int: the conversion is defined)
  const int i = (int)fl;
  *i0 = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
  const int j = i + 1;
  *i1 = j < 0 ? 0 : (j > n - 1 ? n - 1 : j);
}
float ref_lut1(const Lut& l, float cx) {
  int x0, x1; float wx;
  ref_axis(cx, l.w, &x0, &x1, &wx);
  const float a = l.d[x0], b = l.d[x1];
  return a + (b - a) * wx;
}
float ref_slice(const float* d, int W, int H, float cx, float cy) {
  int x0, x1, y0, y1; float wx, wy;
  ref_axis(cx, W, &x0, &x1, &wx);
  ref_axis(cy, H, &y0, &y1, &wy);
  const float t00 = d[y0 * W + x0], t01 = d[y0 * W + x1], t10 = d[y1 * W + x0], t11 = d[y1 * W + x1];
  const float a = t00 + (t01 - t00) * wx;
  const float b = t10 + (t11 - t10) * wx;
  return a + (b - a) * wy;
}
float ref_lut2(const Lut& l, float cx, float cy) { return ref_slice(l.d, l.w, l.h, cx, cy); }
float ref_lut3(const Lut& l, float cx, float cy, float cz) {
  int z0, z1; float wz;
  ref_axis(cz, l.depth, &z0, &z1, &wz);
  const float a = ref_slice(l.d + (size_t)z0 * l.w * l.h, l.w, l.h, cx, cy);
  const float b = ref_slice(l.d + (size_t)z1 * l.w * l.h, l.w, l.h, cx, cy);
  return a + (b - a) * wz;
}

bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// 257 coordinates for an axis of n texels: below 0, 0, every texel centre and edge the count allows, 1, above 1
std::vector<float> grid(int n) {
  std::vector<float> g = {-1.0f, -0.25f, -1e-7f, 0.0f, 1.0f, 1.0f + 1e-6f, 1.5f, 3.0f};
  for (int k = 0; g.size() < 257; k++) {
    const int t = k % n;
    if (k / n == 0) g.push_back(((float)t + 0.5f) / (float)n);   // texel centre
    else if (k / n == 1) g.push_back((float)t / (float)n);       // texel edge
    else g.push_back(((float)t + 0.5f) / (float)n + (float)(k / n) * 0.37f / (float)n);  // in between
  }
  g.resize(257);
  return g;
}

struct Tables {
  std::vector<float> E, Eavg, EMs, EavgMs, ETransIn, ETransOut;
  LutSet luts;
  Tables() {
    auto fill = [](std::vector<float>& v, size_t n, uint32_t seed) {
      v.resize(n);
      for (size_t i = 0; i < n; i++) v[i] = 0.05f + 0.9f * (float)(hash32(seed + (uint32_t)i) >> 8) * (1.0f / 16777216.0f);
    };
    fill(E, 128 * 128, 0x1000000u); fill(Eavg, 128, 0x2000000u); fill(EMs, 32 * 32 * 32, 0x3000000u); fill(EavgMs, 32 * 32, 0x4000000u);
    fill(ETransIn, 32 * 32 * 32, 0x5000000u); fill(ETransOut, 32 * 32 * 32, 0x6000000u);
    luts.E = Lut{E.data(), 128, 128, 1, 0};
    luts.Eavg = Lut{Eavg.data(), 128, 1, 1, 0};
    luts.EMs = Lut{EMs.data(), 32, 32, 32, 0};
    luts.EavgMs = Lut{EavgMs.data(), 32, 32, 1, 0};
    luts.ETransIn = Lut{ETransIn.data(), 32, 32, 32, 0};
    luts.ETransOut = Lut{ETransOut.data(), 32, 32, 32, 0};
  }
};

// ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
long check_lookup_split(const Tables& T) {
  long bad = 0, n = 0;
  const std::vector<float> g128 = grid(128), g32 = grid(32);
  for (float cx : g128) {
    const float s = lut_resolve(lut1_fetch(T.luts.Eavg, lut_axis(cx, 128)));
    bad += !same_bits(s, ref_lut1(T.luts.Eavg, cx)) + !same_bits(lut1(T.luts.Eavg, cx), s);
    n++;
  }
  for (float cy : g128) {
    const LutAxis ay = lut_axis(cy, 128);  // the shared second axis: computed once, used by every cx
    for (float cx : g128) {
      const float s = lut_resolve(lut2_fetch(T.luts.E, lut_axis(cx, 128), ay));
      bad += !same_bits(s, ref_lut2(T.luts.E, cx, cy)) + !same_bits(lut2(T.luts.E, cx, cy), s);
      n++;
    }
  }
  for (float cy : g32) {
    const LutAxis ay = lut_axis(cy, 32);
    for (float cx : g32) {
      const float s = lut_resolve(lut2_fetch(T.luts.EavgMs, lut_axis(cx, 32), ay));
      bad += !same_bits(s, ref_lut2(T.luts.EavgMs, cx, cy)) + !same_bits(lut2(T.luts.EavgMs, cx, cy), s);
      n++;
    }
  }
  for (float cz : g32) {
    const LutAxis az = lut_axis(cz, 32);
    for (float cy : g32) {
      const LutAxis ay = lut_axis(cy, 32);
      for (float cx : g32) {
        const float s = lut_resolve(lut3_fetch(T.luts.EMs, lut_axis(cx, 32), ay, az));
        bad += !same_bits(s, ref_lut3(T.luts.EMs, cx, cy, cz)) + !same_bits(lut3(T.luts.EMs, cx, cy, cz), s);
        n++;
      }
    }
  }
  // a coordinate that is no number, or beyond int: the axis stays inside the table (the one-piece formula's conversion is undefined there)
  const float odd[] = {NAN, INFINITY, -INFINITY, 3.0e38f, -3.0e38f, 1.0e10f};
  for (float c : odd) {
    const LutAxis a = lut_axis(c, 32);
    bad += !(a.i0 >= 0 && a.i0 < 32 && a.i1 >= 0 && a.i1 < 32);
    (void)lut3(T.luts.EMs, c, c, c);
    n++;
  }
  std::printf("lookup split: %ld lookups, %ld mismatches\n", n, bad);
  return bad;
}

// ---- (b) ---------------------------------------------------------------------------------------------------------------------------------
vec3 unit_dir(Rng& r, float z) {
  const float phi = r.range(0.0f, 6.2831853f);
  const float s = std::sqrt(std::fmax(0.0f, 1.0f - z * z));
  return v3(s * std::cos(phi), s * std::sin(phi), z);
}
ShadingContext make_ctx(Rng& r, int cls, uint32_t k) {
  ShadingContext c;
  c.albedo = v3(r.unit(), r.unit(), r.unit());
  c.emission = v3(0.0f);
  c.flags = 0;
  c.anisotropy = (k & 8) ? r.range(0.0f, 0.9f) : 0.0f;
  c.ior = r.range(1.05f, 2.4f);
  c.metallic = 0.0f; c.transmission = 0.0f; c.clearcoat = 0.0f; c.clearcoatRoughness = 0.0f;
  // roughness: 0 and 1 exactly on a share of the inputs, below the smooth cut (alpha < 1e-3), and anything in between
  switch (k % 6) { case 0: c.roughness = 0.0f; break; case 1: c.roughness = 1.0f; break; case 2: c.roughness = r.range(0.0f, 0.03f); break;
                   default: c.roughness = r.unit(); }
  if ((k & 16) && cls == 0) { c.flags |= PT_MATERIAL_EMISSIVE; c.emission = v3(r.range(0.0f, 20.0f), r.range(0.0f, 20.0f), r.range(0.0f, 20.0f)); }
  if (cls == 1) c.metallic = (k % 5 == 0) ? 1.0f : r.range(0.01f, 0.99f);  // (metallic 0 is class 0)
  if (cls == 2) {
    c.transmission = (k % 5 == 0) ? 1.0f : r.range(0.01f, 0.99f);
    if (k % 7 == 0) c.ior = 1.0f;
    if (k % 11 == 0) c.flags |= PT_MATERIAL_THIN_DIELECTRIC;
    if (k % 3 == 0) c.metallic = r.range(0.0f, 0.6f);
  }
  if (cls == 3) {
    c.clearcoat = r.range(0.05f, 1.0f);
    c.clearcoatRoughness = (k % 4 == 0) ? 0.0f : r.unit();
    if (k % 3 == 0) c.metallic = (k % 9 == 0) ? 1.0f : r.unit();
    if (k % 5 == 0) c.transmission = r.unit();
  }
  return c;
}

long check_phased_chain(const Tables& T) {
  long bad_total = 0;
  for (int cls = 0; cls < 4; cls++) {
    long bad = 0, evals = 0, taken[3] = {0, 0, 0};
    Rng r{0x9e3779b9u * (uint32_t)(cls + 1)};
    for (uint32_t k = 0; k < 4096; k++) {
      const ShadingContext ctx = make_ctx(r, cls, k);
      // wo: anywhere above the surface, right at the 1.5e-3 cut on both sides, and (transmission: the ray is inside) below it
      float woz = r.range(0.002f, 1.0f);
      if (k % 8 == 1) woz = 1.5e-3f * (1.0f + 1e-3f);
      if (k % 8 == 2) woz = 1.5e-3f * (1.0f - 1e-3f);
      if (k % 8 == 3) woz = 1.0f;
      if (cls >= 2 && k % 8 == 4) woz = -r.range(0.002f, 1.0f);
      const vec3 wo = unit_dir(r, woz);
      // the light direction: above, at the cut, below the horizon; 0 = the direction shade_issue fetches for when NEE does not run
      float wiz = r.range(0.002f, 1.0f);
      if (k % 16 == 5) wiz = -r.unit();
      if (k % 16 == 6) wiz = 1.5e-3f * (1.0f - 1e-3f);
      if (k % 16 == 7) wiz = 1.5e-3f * (1.0f + 1e-3f);
      const vec3 wi = (k % 16 == 8) ? v3(0.0f) : unit_dir(r, wiz);
      const vec4 rs = {r.unit(), r.unit(), r.unit(), r.unit()};
      const vec2 rc = {r.unit(), r.unit()};
      const int flags = (k & 32) ? 0 : PT_FLAG_MULTISCATTER_GGX;

      const BSDF plain(ctx, flags, T.luts, wo);
      const BsdfEval e0 = plain.eval(wo, wi);
      const BsdfSample s0 = plain.sample(wo, rs, rc);

      BSDF phased(ctx, flags, T.luts);
      NeeLight light;
      light.lit = true; light.Li = v3(1.0f); light.lwi = wi; light.lpdf = 1.0f; light.pLight = 1.0f; light.dist = 1.0f; light.dim = 0;
      ShadeGeom g;
      g.hitPos = v3(0.0f);
      g.frame = {v3(1.0f, 0.0f, 0.0f), v3(0.0f, 1.0f, 0.0f), v3(0.0f, 0.0f, 1.0f)};  // local = world: lwi is wi
      g.wo = wo;
      const ShadeFlight flight = shade_issue(g, phased, light);
      const BSDF::DirTerms lt = shade_land(phased, flight);
      const BsdfEval e1 = phased.eval(wo, g.frame.worldToLocal(light.lwi), lt);
      const BsdfSample s1 = phased.sample(wo, rs, rc);

      const bool same = same_bits(e0.f.x, e1.f.x) && same_bits(e0.f.y, e1.f.y) && same_bits(e0.f.z, e1.f.z) && same_bits(e0.pdf, e1.pdf) &&
                        same_bits(s0.wi.x, s1.wi.x) && same_bits(s0.wi.y, s1.wi.y) && same_bits(s0.wi.z, s1.wi.z) &&
                        same_bits(s0.f.x, s1.f.x) && same_bits(s0.f.y, s1.f.y) && same_bits(s0.f.z, s1.f.z) &&
                        same_bits(s0.Le.x, s1.Le.x) && same_bits(s0.Le.y, s1.Le.y) && same_bits(s0.Le.z, s1.Le.z) &&
                        same_bits(s0.pdf, s1.pdf) && s0.flags == s1.flags &&
                        same_bits(plain.cE_wo, phased.cE_wo) && same_bits(plain.cE_avg, phased.cE_avg) &&
                        same_bits(plain.cEms_wo, phased.cEms_wo) && same_bits(plain.cEms_avg, phased.cEms_avg);
      bad += !same;
      evals += length_squared(e0.f) > 0.0f;
      taken[0] += (s0.flags & Sample_Diffuse) != 0; taken[1] += (s0.flags & Sample_Glossy) != 0; taken[2] += (s0.flags & Sample_Specular) != 0;
    }
    std::printf("phased chain, class %d: 4096 inputs, %ld mismatches (%ld non-zero evals; samples: %ld diffuse, %ld glossy, %ld specular)\n",
                cls, bad, evals, taken[0], taken[1], taken[2]);
    // the inputs must exercise what they are meant to: a class whose evals are all zero, or that never takes a lobe, checks nothing
    if (evals < 1000 || taken[1] + taken[2] < 200 || (cls == 0 && taken[0] < 1000)) { std::printf("class %d: inputs do not cover the lobes\n", cls); bad++; }
    bad_total += bad;
  }
  return bad_total;
}

}  // namespace

int main() {
  const Tables T;
  const long bad = check_lookup_split(T) + check_phased_chain(T);
  std::printf("%s\n", bad == 0 ? "shade_early_check: ok" : "shade_early_check: FAILED");
  return bad == 0 ? 0 : 1;
}
