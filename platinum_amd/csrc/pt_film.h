// pt_film.h — the transparent film: the foreground's radiance with a per-pixel coverage, and the backdrop a target read puts behind it
// (DESIGN.md §3i).
//
//   film_sample      : what one sample contributes: {L.rgb after the non-finite policy, 1} when its camera ray hit, {0, 0, 0, 0} (a select) when not
//   film_fold        : the accumulator's running-mean step (pt_denoise.h aov_fold) on all four channels
//   film_compose     : the display chain's source under a backdrop: base + colour * (1 - a), or base / a
//   film_alpha_byte  : the target's alpha byte in transparent mode: pp_pack_rgba8's quantiser of a
//   film_options_error : pt_set_film_options' test
//
// Written once, as plain C++ under PT_HD: film.hip runs it on the device, tests/emu/film_emu.cpp on the host.  Every operation is one IEEE
// fp32 operation (-ffp-contract=off; the divide correctly rounded), so host and device agree bit for bit.
#pragma once
#include "pt_denoise.h"
#include "pt_post.h"

namespace pt {

// x_s.  `hit`: the bounce-0 hit record's miss test (hit_word_miss), as k_film_flags wrote it: 1 hit, 0 miss.
PT_HD vec4 film_sample(vec4 l4, uint32_t hit, uint32_t nonfinite_policy) {
  vec3 L = v3(l4.x, l4.y, l4.z);
  if (not_finite(L) && nonfinite_policy == PT_NONFINITE_ZERO) L = v3(0.0f);
  return hit ? vec4{L.x, L.y, L.z, 1.0f} : vec4{0.0f, 0.0f, 0.0f, 0.0f};
}

// `f` holds the mean of n samples
PT_HD vec4 film_fold(vec4 f, vec4 x, uint32_t n) {
  const vec3 c = aov_fold(v3(f.x, f.y, f.z), v3(x.x, x.y, x.z), n);
  return vec4{c.x, c.y, c.z, aov_fold(f.w, x.w, n)};
}

// The source of the display chain under PT_BACKDROP_COLOR or PT_BACKDROP_TRANSPARENT (SCENE never gets here).  `base`: film.rgb or its
// denoised image (.w is not read); `a`: film.a.  The result's .w is what film_alpha_byte quantises: 1 under COLOR, a under TRANSPARENT.
PT_HD vec4 film_compose(vec4 base, float a, uint32_t backdrop, const float* rgb) {
  if (backdrop == PT_BACKDROP_COLOR) {
    const float k = 1.0f - a;
    return vec4{base.x + rgb[0] * k, base.y + rgb[1] * k, base.z + rgb[2] * k, 1.0f};
  }
  if (!(a > 0.0f)) return vec4{0.0f, 0.0f, 0.0f, a};   // (also NaN)
  return vec4{base.x / a, base.y / a, base.z / a, a};
}

// 0xAABBGGRR with the alpha byte replaced by the quantised a
PT_HD uint32_t film_alpha_byte(uint32_t rgba8, float a) { return (rgba8 & 0x00ffffffu) | ((pp_pack_rgba8(vec3{a, a, a}) & 255u) << 24); }

// null = valid, otherwise what is wrong
PT_HD const char* film_options_error(const pt_film_options& o) {
  if (o.backdrop > PT_BACKDROP_TRANSPARENT) return "no such backdrop";
  for (int k = 0; k < 3; k++)
    if (!(o.backdrop_rgb[k] >= 0.0f && o.backdrop_rgb[k] <= 3.4028234663852886e38f)) return "every backdrop_rgb component must be finite and >= 0";
  return nullptr;
}

}  // namespace pt
