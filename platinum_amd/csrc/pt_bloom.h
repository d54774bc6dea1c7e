// pt_bloom.h — bloom: an energy-conserving glare pyramid ahead of the post-process.
//
//   bloom_plan      : the frame's size and the level count -> each level's size and place in the pyramid
//   bloom_bright    : a frame pixel -> the light it scatters (soft threshold on luminance; a non-finite pixel scatters nothing)
//   bloom_down_sum  : one texel of level l+1 from the 4x4 taps of level l, weights (1, 3, 3, 1)^2 / 64
//   bloom_up_texel  : the bilinear 2x tap set of a coarse level at a fine texel, weights (1, 3)^2 / 16
//   bloom_combine   : U_l = D_l + scatter * up(U_{l+1});  bloom_composite: out = in + intensity * (up(U_1) / norm - bright(in))
//
// Written once, as plain C++ under PT_HD: bloom.hip runs it on the device, tests/emu/bloom_emu.cpp on the host.  fp32, -ffp-contract=off,
// every sum in the order written here, every weight product exact, no atomics: the two agree bit for bit.  The taps reach their source
// through a callable, so the tiled kernels (LDS tile, clamped at staging) and the host loops run the same per-texel code.
#pragma once
#include <stddef.h>

#include "pt_denoise.h"
#include "pt_post.h"

namespace pt {

constexpr float kBloomMaxScatter = 18446744073709551616.0f;  // 2^64: what one channel of one pixel may scatter

// Level 0 is the frame; level l+1 is ((w_l + 1) / 2) x ((h_l + 1) / 2); L = min(levels, halvings until a level is 1 x 1).
PT_HD void bloom_plan(uint32_t W, uint32_t H, uint32_t levels, pt_bloom_plan* p) {
  *p = pt_bloom_plan{};
  uint32_t w = W, h = H, L = 0, off = 0;
  p->width[0] = W; p->height[0] = H;
  while (L < levels && L < PT_BLOOM_MAX_LEVELS && (w > 1u || h > 1u)) {
    w = (w + 1u) / 2u; h = (h + 1u) / 2u; L++;
    p->width[L] = w; p->height[L] = h; p->offset[L] = off;
    off += w * h;
  }
  p->levels = L;
  p->total_texels = off;
}

// norm = sum over k < L of scatter^k: the running sum += the running power, from k = 0
PT_HD float bloom_norm(uint32_t L, float scatter) {
  float norm = 0.0f, p = 1.0f;
  for (uint32_t k = 0; k < L; k++) { norm += p; p *= scatter; }
  return norm;
}

PT_HD bool bloom_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

// alpha is ignored
PT_HD vec3 bloom_bright(vec4 c, float threshold, float knee) {
  const float Y = dn_lum(v3(c.x, c.y, c.z));
  if (!(fabsf(Y) <= 3.0e38f) || !bloom_finite(c.x) || !bloom_finite(c.y) || !bloom_finite(c.z) || Y <= 0.0f) return v3(0.0f);
  const float s = fminf(fmaxf((Y - threshold) + knee, 0.0f), 2.0f * knee);
  const float soft = (s * s) / (4.0f * knee + 1e-6f);
  const float w = fmaxf(soft, Y - threshold) / Y;
  return v3(fminf(fmaxf(c.x, 0.0f) * w, kBloomMaxScatter), fminf(fmaxf(c.y, 0.0f) * w, kBloomMaxScatter), fminf(fmaxf(c.z, 0.0f) * w, kBloomMaxScatter));
}

// index v of a level of n texels, clamped
PT_HD uint32_t bloom_clamp(int32_t v, uint32_t n) { return v < 0 ? 0u : ((uint32_t)v >= n ? n - 1u : (uint32_t)v); }

// tap(i, j): the source texel (2x - 1 + i, 2y - 1 + j), already clamped to the source level.  Rows j = 0..3, in each i = 0..3, from 0.
template <class Tap>
PT_HD vec3 bloom_down_sum(Tap&& tap) {
  const float k[4] = {0.125f, 0.375f, 0.375f, 0.125f};
  vec3 a = v3(0.0f);
  for (int j = 0; j < 4; j++)
    for (int i = 0; i < 4; i++) {
      const float w = k[j] * k[i];
      const vec3 v = tap(i, j);
      a = v3(a.x + w * v.x, a.y + w * v.y, a.z + w * v.z);
    }
  return a;
}
// the same through a source level of sw x sh texels read by src(x, y)
template <class Src>
PT_HD vec3 bloom_down_texel(Src&& src, uint32_t sw, uint32_t sh, uint32_t x, uint32_t y) {
  return bloom_down_sum([&](int i, int j) { return src(bloom_clamp(2 * (int32_t)x - 1 + i, sw), bloom_clamp(2 * (int32_t)y - 1 + j, sh)); });
}

// the two taps of one axis at fine index x over a coarse level of n texels
PT_HD void bloom_up_taps(uint32_t x, uint32_t n, uint32_t* a, uint32_t* b, float* wa, float* wb) {
  const int32_t c = (int32_t)(x >> 1);
  if ((x & 1u) == 0u) { *a = bloom_clamp(c - 1, n); *b = bloom_clamp(c, n); *wa = 0.25f; *wb = 0.75f; }
  else                { *a = bloom_clamp(c, n); *b = bloom_clamp(c + 1, n); *wa = 0.75f; *wb = 0.25f; }
}
// up(C)(x, y) over the cw x ch coarse level read by src(x, y): (ya, xa), (ya, xb), (yb, xa), (yb, xb)
template <class Src>
PT_HD vec3 bloom_up_texel(Src&& src, uint32_t cw, uint32_t ch, uint32_t x, uint32_t y) {
  uint32_t xa, xb, ya, yb;
  float wxa, wxb, wya, wyb;
  bloom_up_taps(x, cw, &xa, &xb, &wxa, &wxb);
  bloom_up_taps(y, ch, &ya, &yb, &wya, &wyb);
  const vec3 c00 = src(xa, ya), c10 = src(xb, ya), c01 = src(xa, yb), c11 = src(xb, yb);
  const float w00 = wya * wxa, w10 = wya * wxb, w01 = wyb * wxa, w11 = wyb * wxb;
  return v3(((w00 * c00.x + w10 * c10.x) + w01 * c01.x) + w11 * c11.x, ((w00 * c00.y + w10 * c10.y) + w01 * c01.y) + w11 * c11.y,
            ((w00 * c00.z + w10 * c10.z) + w01 * c01.z) + w11 * c11.z);
}

// U_l = D_l + scatter * up(U_{l+1})
PT_HD vec3 bloom_combine(vec3 d, vec3 up, float scatter) { return v3(d.x + scatter * up.x, d.y + scatter * up.y, d.z + scatter * up.z); }

// out.c = in.c + intensity * (up(U_1).c / norm - b.c); a channel that is not finite keeps its bits (its sum is that NaN or infinity
// anyway: this pins the payload), and so does alpha
PT_HD float bloom_mix(float in, float up1, float b, float norm, float intensity) {
  const float B = up1 / norm;
  return bloom_finite(in) ? in + intensity * (B - b) : in;
}
PT_HD vec4 bloom_composite(vec4 c, vec3 up1, float norm, const pt_bloom_options& o) {
  const vec3 b = bloom_bright(c, o.threshold, o.knee);
  return vec4{bloom_mix(c.x, up1.x, b.x, norm, o.intensity), bloom_mix(c.y, up1.y, b.y, norm, o.intensity),
              bloom_mix(c.z, up1.z, b.z, norm, o.intensity), c.w};
}

// pt_set_bloom_options' test, shared with pt_debug_bloom; null = valid, otherwise what is wrong
PT_HD const char* bloom_options_error(const pt_bloom_options& o) {
  if (!(o.intensity >= 0.0f && o.intensity <= 1.0f)) return "0 <= intensity <= 1 is required";
  if (!(o.threshold >= 0.0f && bloom_finite(o.threshold))) return "threshold must be finite and >= 0";
  if (!(o.knee >= 0.0f && bloom_finite(o.knee))) return "knee must be finite and >= 0";
  if (!(o.scatter > 0.0f && o.scatter <= 1.0f)) return "0 < scatter <= 1 is required";
  if (o.levels < 1u || o.levels > PT_BLOOM_MAX_LEVELS) return "1 <= levels <= 12 is required";
  return nullptr;
}

}  // namespace pt
