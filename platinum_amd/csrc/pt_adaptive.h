// pt_adaptive.h — the convergence criterion of tile-adaptive sampling (DESIGN.md §3b "Adaptive sampling").
//
//   adaptive_error            : relative standard error of a pixel's mean luminance after n samples
//   adaptive_pixel_converged  : err <= threshold (false for n < 2 and for a NaN err)
//
// Written once, as plain C++ under PT_HD: adaptive.hip runs it on the device, tests/emu/adaptive_emu.cpp on the host, and the two
// agree bit for bit (-ffp-contract=off, IEEE divide / sqrt).  m1, m2 are the running means of lum(L) and lum(L)^2 after the
// non-finite policy, the same bits as PT_AOV_MOMENTS .g / .b (pt_denoise.h dn_lum / aov_fold).
#pragma once
#include "pt_math.h"

namespace pt {

constexpr float kAdaptiveLumFloor = 1e-3f;

// var = max(m2 - m1^2, 0) * n / (n - 1);  err = sqrt(var / n) / max(m1, kAdaptiveLumFloor).  Both maxima keep a NaN (a NaN
// moment must not read as converged), unlike fmaxf.
PT_HD float adaptive_error(float m1, float m2, uint32_t n) {
  const float nf = (float)n;
  const float d = m2 - m1 * m1;
  const float var = (d < 0.0f ? 0.0f : d) * (nf / (nf - 1.0f));
  const float den = m1 < kAdaptiveLumFloor ? kAdaptiveLumFloor : m1;
  return sqrtf(var / nf) / den;
}

PT_HD bool adaptive_pixel_converged(float m1, float m2, uint32_t n, float threshold) {
  if (n < 2u) return false;
  return adaptive_error(m1, m2, n) <= threshold;
}

}  // namespace pt
