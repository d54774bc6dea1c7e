// pt_view.h — pass views: what the render target shows of the data a render keeps beside the accumulator.
//
//   view_depth        : a pixel's depth d = r / h and whether it is valid (n > 0, h > 0, d finite and >= 0)
//   view_range_*      : the range record of k_view_range: min and max of d as integers (the floats are non-negative, so their bits order as
//                       they do), the number of valid pixels; and z0, z1 as the view uses them
//   view_ramp         : grey, or the five-stop heat ramp; a NaN is drawn as 1
//   view_id_colour    : an id's colour from an integer hash; kMatteNone is black
//   view_pixel        : one pixel of a data view (NORMAL, DEPTH, ALPHA, MATTE, SAMPLES, NOISE) as 0xAABBGGRR, alpha byte 255
//   view_options_error, view_available, view_shown : pt_set_view_options' test and the availability rule
//
// Written once, as plain C++ under PT_HD: view.hip runs it on the device, tests/emu/view_emu.cpp on the host.  Every operation is one IEEE fp32
// operation (-ffp-contract=off; the divide and sqrt correctly rounded), so host and device agree byte for byte.  The noise view's error is
// adaptive sampling's own (pt_adaptive.h adaptive_error), the bytes are the post-process's quantiser (pt_post.h pp_pack_rgba8).
#pragma once
#include <string.h>

#include "pt_adaptive.h"
#include "pt_layout.h"
#include "pt_matte.h"
#include "pt_post.h"

namespace pt {

// what k_view_range leaves behind; cleared to 0 ahead of it.  The minimum is kept as the maximum of the inverted bits, so one memset serves,
// and inv_min != 0 says that some pixel was valid (a depth's sign bit is clear, so its inverted bits are >= 0x80000000).  `count` is kept only
// where it is asked for (pt_read_view_stats, pt_debug_view): a present needs the range alone.
struct ViewRecord { uint32_t inv_min, max, count, _pad; };
static_assert(sizeof(ViewRecord) == 16, "ViewRecord");

// what the kernels need of pt_view_options, and of the render
struct ViewParams {
  uint32_t view, ramp, auto_range;
  float z0, z1;      // auto_range = 0: the options' range
  float noise_max;
  uint32_t spp;      // SAMPLES: the render's spp
};

PT_HD ViewParams view_params(const pt_view_options& o, uint32_t spp) { return ViewParams{o.view, o.ramp, o.auto_range, o.depth_min, o.depth_max, o.noise_max, spp}; }

PT_HD uint32_t view_float_bits(float f) { uint32_t b; memcpy(&b, &f, sizeof(b)); return b; }
PT_HD float view_bits_float(uint32_t b) { float f; memcpy(&f, &b, sizeof(f)); return f; }

// N: the normal AOV's pixel (.w = the hit fraction h), r: the moments AOV's .r.  True when the pixel is valid; then *d = r / h.
PT_HD bool view_depth(float r, float h, uint32_t n, float* d) {
  if (n == 0u || !(h > 0.0f)) return false;   // (also a NaN h)
  const float q = r / h;
  if (!(q >= 0.0f && q <= 3.4028234663852886e38f)) return false;
  *d = q;
  return true;
}
// d >= 0 as the integer the range pass folds (-0 counts as 0)
PT_HD uint32_t view_depth_key(float d) { return view_float_bits(d) & 0x7fffffffu; }

PT_HD void view_range_fold(ViewRecord& rec, uint32_t key) {
  rec.inv_min = ~key > rec.inv_min ? ~key : rec.inv_min;
  rec.max = key > rec.max ? key : rec.max;
  rec.count += 1u;
}
// z0, z1 as the view uses them: the options' with auto_range = 0, else the record's, 0 and 0 when no pixel was valid
PT_HD void view_range(const ViewParams& P, const ViewRecord& rec, float* z0, float* z1) {
  if (!P.auto_range) { *z0 = P.z0; *z1 = P.z1; return; }
  *z0 = rec.inv_min ? view_bits_float(~rec.inv_min) : 0.0f;
  *z1 = rec.inv_min ? view_bits_float(rec.max) : 0.0f;
}

// the heat ramp's stops a_0 .. a_4: blue, cyan, green, yellow, red (selects: a table indexed at run time would live in scratch)
PT_HD vec3 view_heat_stop(int k) { return vec3{k >= 3 ? 1.0f : 0.0f, (k >= 1 && k <= 3) ? 1.0f : 0.0f, k <= 1 ? 1.0f : 0.0f}; }

// v in [0, 1] or NaN (drawn as 1)
PT_HD vec3 view_ramp(uint32_t ramp, float v) {
  if (v != v) v = 1.0f;
  if (ramp != PT_RAMP_HEAT) return vec3{v, v, v};
  const float s = v * 4.0f;
  const int i = (int)s, k = i < 3 ? i : 3;
  const float f = s - (float)k;
  const vec3 a = view_heat_stop(k), b = view_heat_stop(k + 1);
  return vec3{a.x + (b.x - a.x) * f, a.y + (b.y - a.y) * f, a.z + (b.z - a.z) * f};
}

PT_HD uint32_t view_hash(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
PT_HD vec3 view_id_colour(uint32_t id) {
  if (id == kMatteNone) return vec3{0.0f, 0.0f, 0.0f};
  const uint32_t x = view_hash(id);
  return vec3{(float)(x & 255u) / 255.0f * 0.75f + 0.25f, (float)((x >> 8) & 255u) / 255.0f * 0.75f + 0.25f,
              (float)((x >> 16) & 255u) / 255.0f * 0.75f + 0.25f};
}

// the slots of one layer, weighted by their share of the pixel's n samples (n > 0), summed in slot order from 0
PT_HD vec3 view_matte(const MatteSlots& m, uint32_t n) {
  vec3 c{0.0f, 0.0f, 0.0f};
  const float nf = (float)n;
#pragma unroll
  for (uint32_t k = 0; k < kMatteSlots; k++) {
    if (m.count[k] == 0u) continue;
    const float w = (float)m.count[k] / nf;
    const vec3 col = view_id_colour(m.id[k]);
    c.x = c.x + w * col.x; c.y = c.y + w * col.y; c.z = c.z + w * col.z;
  }
  return c;
}

PT_HD float view_depth_value(float d, float z0, float z1) {
  float t = z1 > z0 ? (d - z0) / (z1 - z0) : 0.0f;
  t = t < 0.0f ? 0.0f : t;
  t = t > 1.0f ? 1.0f : t;
  return 1.0f - t;
}

PT_HD float view_samples_value(uint32_t n, uint32_t spp) {
  const float v = (float)n / (float)spp;
  return v < 1.0f ? v : 1.0f;   // (n > 0, so never 0 / 0)
}

PT_HD float view_noise_value(float m1, float m2, uint32_t n, float noise_max) {
  if (n < 2u) return 1.0f;
  const float err = adaptive_error(m1, m2, n);
  if (err != err) return 1.0f;
  const float v = err / noise_max;
  return v < 1.0f ? v : 1.0f;
}

// One pixel of a data view.  `px` fetches what the view reads, and nothing else: normal() the normal AOV's pixel, moments() {r, m1, m2} of the
// moments AOV (or {0, m1, m2} of the adaptive moments), alpha() film.a, slots(m) the eight slots of the layer shown.
template <class Px>
PT_HD uint32_t view_pixel(const ViewParams& P, float z0, float z1, uint32_t n, const Px& px) {
  if (n == 0u) return 0xff000000u;
  vec3 c{0.0f, 0.0f, 0.0f};
  switch (P.view) {
    case PT_VIEW_NORMAL: {
      const vec4 N = px.normal();
      c = vec3{N.x * 0.5f + 0.5f, N.y * 0.5f + 0.5f, N.z * 0.5f + 0.5f};
    } break;
    case PT_VIEW_DEPTH: {
      float d;
      if (view_depth(px.moments().x, px.normal().w, n, &d)) c = view_ramp(P.ramp, view_depth_value(d, z0, z1));
    } break;
    case PT_VIEW_ALPHA: c = view_ramp(PT_RAMP_GREY, px.alpha()); break;
    case PT_VIEW_MATTE: {
      MatteSlots m;
      px.slots(m);
      c = view_matte(m, n);
    } break;
    case PT_VIEW_SAMPLES: c = view_ramp(P.ramp, view_samples_value(n, P.spp)); break;
    case PT_VIEW_NOISE: {
      const vec3 M = px.moments();
      c = view_ramp(P.ramp, view_noise_value(M.y, M.z, n, P.noise_max));
    } break;
    default: break;
  }
  return pp_pack_rgba8(c);
}

// pt_set_view_options' test, shared with pt_debug_view; null = valid, otherwise what is wrong
PT_HD const char* view_options_error(const pt_view_options& o) {
  const float big = 3.4028234663852886e38f;
  if (o.view >= PT_VIEW_COUNT) return "no such view";
  if (o.layer > PT_MATTE_MATERIAL) return "no such layer";
  if (o.ramp > PT_RAMP_HEAT) return "no such ramp";
  if (o.auto_range > 1u) return "auto_range must be 0 or 1";
  if (!o.auto_range && !(o.depth_min >= 0.0f && o.depth_min < o.depth_max && o.depth_max <= big))
    return "0 <= depth_min < depth_max, both finite, is required without auto_range";
  if (!(o.noise_max > 0.0f && o.noise_max <= big)) return "noise_max must be finite and > 0";
  return nullptr;
}

// Does a render that keeps this data show the view?  (merged: a device group's merged image, which shows the beauty only)
PT_HD bool view_available(uint32_t view, bool aov, bool film, bool matte, bool adaptive, bool merged) {
  if (merged) return view == PT_VIEW_BEAUTY;
  switch (view) {
    case PT_VIEW_BEAUTY: case PT_VIEW_SAMPLES: return true;
    case PT_VIEW_ALBEDO: case PT_VIEW_NORMAL: case PT_VIEW_DEPTH: return aov;
    case PT_VIEW_ALPHA: return film;
    case PT_VIEW_MATTE: return matte;
    case PT_VIEW_NOISE: return aov || adaptive;
    default: return false;
  }
}
PT_HD uint32_t view_shown(uint32_t view, bool aov, bool film, bool matte, bool adaptive, bool merged) {
  return view_available(view, aov, film, matte, adaptive, merged) ? view : (uint32_t)PT_VIEW_BEAUTY;
}
PT_HD bool view_is_data(uint32_t view) { return view >= PT_VIEW_NORMAL && view < PT_VIEW_COUNT; }

}  // namespace pt
