// pt_math_probe.h — one element of pt_debug_math (include/ptamd.h): each function of the math layer called exactly as the kernels call it.
// Plain C++ under PT_HD: math_probe.hip runs it on the device, tests/emu/math_emu.cpp on the host.
#pragma once
#include "pt_denoise.h"
#include "pt_post.h"
#include "pt_sampler.h"

namespace pt {

PT_HD bool math_probe_reads_b(uint32_t fn) {
  switch (fn) {
    case PT_MATH_ATAN2: case PT_MATH_POWR: case PT_MATH_PP_POWR: case PT_MATH_DN_POWR: case PT_MATH_SAMPLE_DISK:
    case PT_MATH_SAMPLE_COSINE_HEMISPHERE: case PT_MATH_SAMPLE_TRI_UNIFORM: case PT_MATH_HALTON: case PT_MATH_HALTON_OFFSET:
    case PT_MATH_BOKEH_POWR: return true;
    default: return false;
  }
}
PT_HD bool math_probe_writes_out1(uint32_t fn) {
  return fn == PT_MATH_SINCOS || fn == PT_MATH_SAMPLE_DISK || fn == PT_MATH_SAMPLE_COSINE_HEMISPHERE || fn == PT_MATH_SAMPLE_TRI_UNIFORM;
}

// Words in, words out (floats travel as their bits).  o[0] -> out0[i], o[1] -> out1[i], o[2] -> out1[n + i] (cosine hemisphere only).
PT_HD void math_probe_eval(uint32_t fn, uint32_t a, uint32_t b, const HaltonEntry* table, uint32_t o[3]) {
  const float x = u2f(a), y = u2f(b);
  float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
  switch (fn) {
    case PT_MATH_SINCOS: sincos_det(x, &r0, &r1); break;
    case PT_MATH_COS: r0 = cos_det(x); break;
    case PT_MATH_ATAN2: r0 = atan2_det(x, y); break;
    case PT_MATH_ACOS: r0 = acos_det(x); break;
    case PT_MATH_LOG2: r0 = log2_det(x); break;
    case PT_MATH_EXP2: r0 = exp2_det(x); break;
    case PT_MATH_POWR: r0 = powr_det(x, y); break;
    case PT_MATH_PP_LOG2: r0 = pp_log2(x); break;
    case PT_MATH_PP_EXP2: r0 = pp_exp2(x); break;
    case PT_MATH_PP_EXP2S: r0 = pp_exp2s(x); break;
    case PT_MATH_PP_POWR: r0 = pp_powr(x, y); break;
    case PT_MATH_DN_EXP2: r0 = dn_exp2(x); break;
    case PT_MATH_DN_POWR: r0 = dn_powr(x, y); break;
    case PT_MATH_SAMPLE_DISK: { const vec2 p = sampleDisk({x, y}); r0 = p.x; r1 = p.y; break; }
    case PT_MATH_SAMPLE_COSINE_HEMISPHERE: { const vec3 w = sampleCosineHemisphere({x, y}); r0 = w.x; r1 = w.y; r2 = w.z; break; }
    case PT_MATH_SAMPLE_TRI_UNIFORM: { const vec2 p = sampleTriUniform({x, y}); r0 = p.x; r1 = p.y; break; }
    case PT_MATH_HALTON: r0 = halton(halton_table(table), a, b); break;
    case PT_MATH_HALTON_OFFSET: o[0] = halton_offset(a & 0xffffu, a >> 16, b); o[1] = 0u; o[2] = 0u; return;
    case PT_MATH_BOKEH_POWR: r0 = bokeh_powr(sampleDiskPolar({x, 0.0f}).x, y); break;  // pt_shade.h stage_raygen
    default: break;
  }
  o[0] = f2u(r0); o[1] = f2u(r1); o[2] = f2u(r2);
}

}  // namespace pt
