// pt_exposure.h — auto exposure: a luminance-histogram meter ahead of the post-process.
//
//   exposure_classify : a pixel's luminance -> one of 259 counters (256 bins, below, above, nonfinite)
//   exposure_resolve  : the counters -> the metered mean, the EV and the gain (serial: one lane on the device)
//   exposure_apply    : rgb * gain, alpha copied
//
// Written once, as plain C++ under PT_HD: exposure.hip runs it on the device, tests/emu/exposure_emu.cpp on the host.  The histogram is
// integer, so it does not depend on the order pixels arrive in; the float path is the fixed sequence below over pt_math.h's deterministic
// exp2 (-ffp-contract=off, IEEE double divide), so the two agree bit for bit.
//
// Bins: 8 per octave over the 32 octaves [2^-16, 2^16), taken from the exponent and the top three mantissa bits of Y — no logarithm.
// Bin b covers log2 Y in [-16 + b/8, -16 + (b+1)/8) up to the piecewise-linear mantissa; its centre is taken as -16 + (2b + 1) / 16.
#pragma once
#include <stddef.h>

#include "pt_denoise.h"
#include "pt_post.h"

namespace pt {

constexpr uint32_t kExpBins = 256;
constexpr uint32_t kExpBelow = 256, kExpAbove = 257, kExpNonfinite = 258;  // the outlier counters follow the bins (pt_exposure_meter)
constexpr uint32_t kExpCounters = 259;
constexpr float kExpLumMin = 1.52587890625e-05f;  // 2^-16
constexpr float kExpLumMax = 65536.0f;            // 2^16

// the meter record's first 259 words are the counters, in the order of the keys above
static_assert(offsetof(pt_exposure_meter, below) == 4 * kExpBelow && offsetof(pt_exposure_meter, above) == 4 * kExpAbove &&
              offsetof(pt_exposure_meter, nonfinite) == 4 * kExpNonfinite, "pt_exposure_meter: counters are bins, below, above, nonfinite");

PT_HD uint32_t exposure_classify(float Y) {
  if (!(fabsf(Y) <= 3.4028234663852886e38f)) return kExpNonfinite;  // NaN, +-inf
  if (Y < kExpLumMin) return kExpBelow;                               // 0, negatives, denormals
  if (Y >= kExpLumMax) return kExpAbove;
  return (f2u(Y) >> 20) - 888u;                                       // (111 << 3) = 888: the exponent of 2^-16 and a zero mantissa
}
// alpha is ignored
PT_HD uint32_t exposure_pixel_key(vec4 c) { return exposure_classify(dn_lum(v3(c.x, c.y, c.z))); }

// m->bins / below / above / nonfinite hold the counts; fills the rest of the record.  Only binned pixels are metered: of their n, the
// ranks [lo, hi) in ascending luminance are kept (the fractions cut dark and bright tails), and the mean is that of the kept bins' centres.
PT_HD void exposure_resolve(pt_exposure_meter* m, const pt_exposure_options& o, float prev_ev, uint32_t has_prev) {
  uint64_t n = 0;
  for (uint32_t b = 0; b < kExpBins; b++) n += m->bins[b];
  uint64_t lo = (uint64_t)((double)n * (double)o.low_fraction);
  uint64_t hi = (uint64_t)((double)n * (double)o.high_fraction);
  if (hi > n) hi = n;
  if (hi <= lo) { lo = 0; hi = n; }
  uint64_t S = 0, rank = 0;
  for (uint32_t b = 0; b < kExpBins; b++) {   // bin b holds the ranks [rank, rank + bins[b])
    const uint64_t r0 = rank, r1 = rank + m->bins[b];
    const uint64_t k0 = r0 > lo ? r0 : lo, k1 = r1 < hi ? r1 : hi;
    if (k1 > k0) S += (k1 - k0) * (uint64_t)(2u * b + 1u);
    rank = r1;
  }
  const uint64_t K = hi - lo;
  float mean_log2 = 0.0f, target_ev = 0.0f;
  if (n != 0) {
    mean_log2 = (float)((double)S / (double)(16u * K)) - 16.0f;
    target_ev = fminf(fmaxf(o.target_log2 - mean_log2, o.min_ev), o.max_ev);
  }
  const float ev = has_prev ? prev_ev + (1.0f - o.smoothing) * (target_ev - prev_ev) : target_ev;
  m->metered = (uint32_t)n;
  m->kept = (uint32_t)K;
  m->_pad = 0;
  m->weighted = S;
  m->mean_log2 = mean_log2;
  m->target_ev = target_ev;
  m->ev = ev;
  m->gain = pp_exp2s(ev);
}

PT_HD vec4 exposure_apply(vec4 c, float gain) { return vec4{c.x * gain, c.y * gain, c.z * gain, c.w}; }

// pt_set_exposure_options' test, shared with pt_debug_exposure; null = valid, otherwise what is wrong
PT_HD const char* exposure_options_error(const pt_exposure_options& o) {
  if (!(fabsf(o.target_log2) <= 32.0f)) return "target_log2 must be finite with |target_log2| <= 32";
  if (!(o.low_fraction >= 0.0f && o.low_fraction < o.high_fraction && o.high_fraction <= 1.0f)) return "0 <= low_fraction < high_fraction <= 1 is required";
  if (!(o.min_ev >= -32.0f && o.min_ev <= o.max_ev && o.max_ev <= 32.0f)) return "-32 <= min_ev <= max_ev <= 32 is required";
  if (!(o.smoothing >= 0.0f && o.smoothing < 1.0f)) return "0 <= smoothing < 1 is required";
  return nullptr;
}

}  // namespace pt
