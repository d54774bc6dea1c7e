// pt_shade_probe.h — one element of pt_debug_shading (include/ptamd.h): the stage between a hit record and the BSDF (pt_shade.h
// shade_geometry, pt_bsdf.h make_shading_context) called exactly as k_shade and k_aov call it.  Plain C++ under PT_HD: shade_probe.hip runs
// it on the device, tests/emu/shade_emu.cpp on the host.
#pragma once
#include <unordered_map>
#include <vector>

#include "pt_shade.h"

namespace pt {

// (instance, primitive) of triangle t = 2 * slot + half, through the definition the trace kernels' write-back uses (pt_bvh.h triangle_ids);
// (-1, -1) for the B entry of a one-triangle slot, which no hit refers to
PT_HD void shade_probe_ids(const DeviceScene& S, uint32_t t, int32_t* ids) {
  const TriRec& tr = S.tris[t >> 1];
  ids[0] = ids[1] = -1;
  if (((t & 1u) ? tr.gid_b : tr.gid_a) != kInvalidRef) triangle_ids(S, t, &ids[0], &ids[1]);
}

// Where a record keeps the triangle index the host resolved for it: the unused last word of the input record
constexpr uint32_t kShadeProbeTriWord = PT_SHADE_PROBE_IN_WORDS - 1u;

// Host: fills word kShadeProbeTriWord of each of the n records in `rec` with the triangle whose shade_probe_ids are the record's
// (instance, primitive); `ids` holds the pairs of triangles 0 .. n_tri - 1.  False when a record names no triangle of the scene.
inline bool shade_probe_resolve(const int32_t* ids, uint32_t n_tri, uint32_t* rec, uint32_t n) {
  std::unordered_map<uint64_t, uint32_t> tri_of;
  tri_of.reserve(n_tri);
  for (uint32_t t = 0; t < n_tri; t++)
    if (ids[2 * t] >= 0) tri_of[((uint64_t)(uint32_t)ids[2 * t] << 32) | (uint32_t)ids[2 * t + 1]] = t;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t* e = rec + (size_t)i * PT_SHADE_PROBE_IN_WORDS;
    const auto it = tri_of.find(((uint64_t)e[0] << 32) | e[1]);
    if (it == tri_of.end()) return false;
    e[kShadeProbeTriWord] = it->second;
  }
  return true;
}

// One record: shade_geometry for the hit (u, v, t) on triangle in[kShadeProbeTriWord] of the ray (o, d).  Only what shade_geometry reads
// of the ShadeIn is filled.  The material class is the one the hit word carries to k_shade: the low bits of the triangle's gid.
PT_HD void shade_probe_element(const DeviceScene& S, const uint32_t* in, uint32_t* out) {
  ShadeIn si{};
  si.tri = in[kShadeProbeTriWord];
  si.u = u2f(in[2]); si.v = u2f(in[3]);
  si.o = v3(u2f(in[4]), u2f(in[5]), u2f(in[6]));
  si.d = v3(u2f(in[7]), u2f(in[8]), u2f(in[9]));
  si.t = u2f(in[10]);
  ShadeGeom g;
  ShadingContext ctx;
  shade_geometry(S, si, g, ctx);
  const TriRec& tr = S.tris[si.tri >> 1];
  const uint32_t gid = (si.tri & 1u) ? ldg(&tr.gid_b) : ldg(&tr.gid_a);
  out[0] = f2u(g.hitPos.x); out[1] = f2u(g.hitPos.y); out[2] = f2u(g.hitPos.z);
  out[3] = f2u(g.frame.x.x); out[4] = f2u(g.frame.x.y); out[5] = f2u(g.frame.x.z);
  out[6] = f2u(g.frame.y.x); out[7] = f2u(g.frame.y.y); out[8] = f2u(g.frame.y.z);
  out[9] = f2u(g.frame.z.x); out[10] = f2u(g.frame.z.y); out[11] = f2u(g.frame.z.z);
  out[12] = f2u(g.wo.x); out[13] = f2u(g.wo.y); out[14] = f2u(g.wo.z);
  out[15] = f2u(ctx.albedo.x); out[16] = f2u(ctx.albedo.y); out[17] = f2u(ctx.albedo.z);
  out[18] = f2u(ctx.emission.x); out[19] = f2u(ctx.emission.y); out[20] = f2u(ctx.emission.z);
  out[21] = f2u(ctx.roughness); out[22] = f2u(ctx.metallic); out[23] = f2u(ctx.transmission); out[24] = f2u(ctx.clearcoat);
  out[25] = f2u(ctx.clearcoatRoughness); out[26] = f2u(ctx.anisotropy); out[27] = f2u(ctx.ior);
  out[28] = (uint32_t)ctx.flags;
  out[29] = gid & 3u;
  out[30] = 0u; out[31] = 0u;
}

}  // namespace pt
