// pt_ao.h — the ambient-occlusion pass: ONE definition of the AO ray of a camera ray, of the fold of its one-bit answer and of
// the resolve.  Plain C++ under PT_HD: k_trace_ao (kernels.hip) and ao.hip run it on the device, tests/emu/ao_emu.cpp on the host.
//
//   stage_ao   : camera ray (queue entry o, d), its hit (t, the triangle's ShadeRec::ng), the path's Halton offset  ->  the AO ray
//   ao_fold    : per pixel {hits, open} += one sample's state
//   ao_value   : open / hits, 1 where no camera ray hit
//   ao_options_error : pt_set_ao_options' test
//
// Per camera ray the state is 0 (the camera ray missed), 1 (hit, AO ray occluded) or 2 (hit, AO ray unoccluded): integers, so the per-pixel
// result is exact and independent of how the samples were batched.
#pragma once
#include "pt_shade.h"

namespace pt {

#if !defined(__HIPCC__)
struct uint2 { uint32_t x, y; };   // (a host build without the HIP headers: the device side's is HIP's own)
#endif

constexpr uint32_t kAoMiss = 0u, kAoOccluded = 1u, kAoOpen = 2u;
constexpr float kAoTmin = 1e-3f;              // the shadow rays' near limit
// The AO stream is a Halton sequence of its own: index pcg4d_x(offset, PT_AO_SALT, 0, 0), dimensions 0..1 (direction) and 2 (alpha-test
// payload).  No dimension of the path's own stream moves, so every other output of a render is the bits it is without AO.
constexpr uint32_t PT_AO_SALT = 0x414f5031u;  // "AOP1"
PT_HD uint32_t ao_index(uint32_t offset) { return pcg4d_x(offset, PT_AO_SALT, 0u, 0u); }

struct AoRay {
  vec3 o, d;       // origin o + d t (shade_geometry_finish's hitPos, the same operations); cosine-weighted direction about n
  float payload;   // the alpha-test draw a shadow ray carries; 0 without cut-outs
};

// `ng`: the hit triangle's resolved world-space geometric normal (ShadeRec::ng: the reference's normalize(M * n) through the FORWARD matrix —
// under a non-uniform scale it is not the true normal, as DESIGN.md §2 says of the shading normals).  It is turned to face the viewer.
PT_HD AoRay stage_ao(const HaltonEntry* halton, bool has_alpha, vec3 o, vec3 d, float t, vec3 ng, uint32_t offset) {
  AoRay r;
  r.o = o + d * t;
  const vec3 n = dot(ng, d) > 0.0f ? v3(-ng.x, -ng.y, -ng.z) : ng;
  Halton h{halton_table(halton), ao_index(offset), 0u};
  const vec2 u = h.sample2d();
  r.payload = has_alpha ? h.sample1d() : 0.0f;
  r.d = frame_from_normal(n).localToWorld(sampleCosineHemisphere(u));
  return r;
}
// (on the scene table: what the trace kernel and the host build call)
PT_HD AoRay stage_ao(const DeviceScene& S, vec3 o, vec3 d, float t, uint32_t hit_word3, uint32_t offset) {
  const ShadeRec rec = ldg(&S.shade_recs[hit_word_tri(hit_word3)]);
  return stage_ao(S.halton, S.has_alpha != 0, o, d, t, v3(rec.ng[0], rec.ng[1], rec.ng[2]), offset);
}

// c = {hits, open}
PT_HD uint2 ao_fold(uint2 c, uint32_t state) {
  c.x += state != kAoMiss ? 1u : 0u;
  c.y += state == kAoOpen ? 1u : 0u;
  return c;
}
PT_HD float ao_value(uint32_t hits, uint32_t open) { return hits ? (float)open / (float)hits : 1.0f; }

// nullptr = accepted (distance = +inf is: an unbounded AO ray)
PT_HD const char* ao_options_error(const pt_ao_options& o) {
  if (o.enabled > 1u) return "enabled must be 0 or 1";
  if (!(o.distance > 0.0f)) return "distance must be > 0 (NaN is refused; +inf is allowed)";
  return nullptr;
}

}  // namespace pt
