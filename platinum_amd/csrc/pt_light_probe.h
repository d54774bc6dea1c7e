// pt_light_probe.h — one element of pt_debug_lights (include/ptamd.h): the light-sampling part of the shading stage (pt_shade.h) called
// exactly as k_shade calls it.  Plain C++ under PT_HD: light_probe.hip runs it on the device, tests/emu/light_emu.cpp on the host.
#pragma once
#include "pt_shade.h"

namespace pt {

PT_HD uint32_t light_probe_in_words(uint32_t fn) { return fn == PT_LIGHT_SAMPLE ? PT_LIGHT_SAMPLE_IN_WORDS : PT_LIGHT_ENV_MISS_IN_WORDS; }
PT_HD uint32_t light_probe_out_words(uint32_t fn) { return fn == PT_LIGHT_SAMPLE ? PT_LIGHT_SAMPLE_OUT_WORDS : PT_LIGHT_ENV_MISS_OUT_WORDS; }

// what is wrong with a call that the scene S cannot serve; null = it can
inline const char* light_probe_unsupported(const DeviceScene& S, uint32_t fn, const pt_light_probe_args& a, uint32_t staged_lights) {
  if (fn == PT_LIGHT_SAMPLE && a.tables == PT_LIGHT_TABLES_LDS && S.lightCount > staged_lights)
    return "pt_debug_lights: PT_LIGHT_TABLES_LDS stages at most 64 lights";
  if (fn == PT_LIGHT_ENV_MISS && S.env_texture < 0) return "pt_debug_lights: PT_LIGHT_ENV_MISS needs an environment";
  return nullptr;
}

// PT_LIGHT_SAMPLE: shade_nee_light for a hit at in[0..2] with the draws in[3..5].  Only what shade_nee_light reads of the hit is filled:
// the position, the sampler cursor and the three material terms of the gate.
PT_HD void light_probe_sample(const DeviceScene& S, const ShadeTables& T, const pt_light_probe_args& a, const float* in, uint32_t* out) {
  ShadeIn si{};
  si.dim = a.dim;
  ShadeGeom g{};
  g.hitPos = v3(in[0], in[1], in[2]);
  ShadingContext ctx{};
  ctx.roughness = a.roughness; ctx.metallic = a.metallic; ctx.transmission = a.transmission;
  NeeDraws draws;
  draws.rl = vec2{in[3], in[4]};
  draws.rz = in[5];
  const NeeLight l = shade_nee_light(S, T, si, g, ctx, draws);
  out[0] = l.lit ? 1u : 0u;
  out[1] = f2u(l.Li.x); out[2] = f2u(l.Li.y); out[3] = f2u(l.Li.z);
  out[4] = f2u(l.lwi.x); out[5] = f2u(l.lwi.y); out[6] = f2u(l.lwi.z);
  out[7] = f2u(l.lpdf); out[8] = f2u(l.pLight); out[9] = f2u(l.dist);
  out[10] = l.dim; out[11] = 0u;
}

// PT_LIGHT_ENV_MISS: stage_miss for the direction in[0..2] and lastPdf in[3], attenuation 1
PT_HD void light_probe_miss(const DeviceScene& S, const pt_light_probe_args& a, const float* in, uint32_t* out) {
  const vec3 L = stage_miss(S, v3(in[0], in[1], in[2]), v3(1.0f), a.bounce, in[3], a.lastSpecular != 0u);
  out[0] = f2u(L.x); out[1] = f2u(L.y); out[2] = f2u(L.z); out[3] = 0u;
}

}  // namespace pt
