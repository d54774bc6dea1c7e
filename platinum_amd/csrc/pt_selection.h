// pt_selection.h — the selection overlay: an antialiased outline around, and an optional tint over, the pixels covered by a set of matte
// ids, drawn onto the RGBA8 target after the post-process.
//
//   sel_radius / sel_weight : lim = width + 0.5, R = ceil(lim) - 1, k(dx, dy) = clamp(lim - sqrt(dx^2 + dy^2), 0, 1)
//   sel_dilate              : D(p) = max over |dx|, |dy| <= R of m(p + (dx, dy)) * k(dx, dy), through a callable that gives 0 outside the image
//   sel_composite           : fill alpha m * fill.a, outline alpha (D - m) * outline.a, mixed into the target's bytes
//   sel_tile_pixel          : the block-tile map of k_selection_overlay: LDS texel of block b -> image pixel, or outside
//
// Written once, as plain C++ under PT_HD: selection.hip runs it on the device, tests/emu/selection_emu.cpp on the host.  Every operation is
// one IEEE fp32 operation (-ffp-contract=off; sqrt and divide correctly rounded), and D is a max of single products, which does not depend
// on the tap order: host and device agree byte for byte.  The colours are UI colours in the target's own encoding: nothing here goes through
// exposure, bloom or a tonemapper.
#pragma once
#include <stddef.h>

#include "pt_post.h"

namespace pt {

constexpr uint32_t kSelBlock = 16;                                  // k_selection_overlay: 16 x 16 pixels per block
constexpr int32_t kSelMaxRadius = 16;                               // R at width 16
constexpr uint32_t kSelTileMax = kSelBlock + 2u * kSelMaxRadius;    // the staged tile's side at R = 16: 48
constexpr uint32_t kSelTapsMax = 2u * kSelMaxRadius + 1u;           // the weight table's side at R = 16: 33

// what the kernel needs of pt_selection_options
struct SelParams {
  float lim;       // width + 0.5
  int32_t R;       // ceil(lim) - 1
  float outline[4], fill[4];
};

PT_HD float sel_limit(float width) { return width + 0.5f; }
PT_HD int32_t sel_radius(float width) { return (int32_t)ceilf(sel_limit(width)) - 1; }
PT_HD float sel_weight(float lim, int32_t dx, int32_t dy) { return fminf(fmaxf(lim - sqrtf((float)(dx * dx + dy * dy)), 0.0f), 1.0f); }

PT_HD SelParams sel_params(const pt_selection_options& o) {
  SelParams P;
  P.lim = sel_limit(o.width);
  P.R = sel_radius(o.width);
  for (int k = 0; k < 4; k++) { P.outline[k] = o.outline_rgba[k]; P.fill[k] = o.fill_rgba[k]; }
  return P;
}

// The staged tile of block (bx, by): (kSelBlock + 2R)^2 texels, row-major, texel (0, 0) at the block's first pixel - (R, R).  Texel t is
// image pixel (*x, *y) when the return value is true, and outside the W x H image (staged as coverage 0) when it is false.
PT_HD uint32_t sel_tile_side(int32_t R) { return kSelBlock + 2u * (uint32_t)R; }
PT_HD bool sel_tile_pixel(uint32_t bx, uint32_t by, int32_t R, uint32_t t, uint32_t W, uint32_t H, uint32_t* x, uint32_t* y) {
  const uint32_t T = sel_tile_side(R);
  const uint32_t ty = t / T, tx = t - ty * T;
  const int32_t px = (int32_t)(bx * kSelBlock + tx) - R, py = (int32_t)(by * kSelBlock + ty) - R;   // (W * H <= 2^28: no overflow)
  if (px < 0 || py < 0 || (uint32_t)px >= W || (uint32_t)py >= H) return false;
  *x = (uint32_t)px; *y = (uint32_t)py;
  return true;
}
// the tile texel of the block's own pixel (lx, ly), lx, ly < kSelBlock, displaced by (dx, dy), |dx|, |dy| <= R
PT_HD uint32_t sel_tile_texel(int32_t R, uint32_t lx, uint32_t ly, int32_t dx, int32_t dy) {
  return (uint32_t)((int32_t)ly + R + dy) * sel_tile_side(R) + (uint32_t)((int32_t)lx + R + dx);
}

// tap(dx, dy): the coverage at p + (dx, dy), 0 outside the image; weight(dx, dy): k(dx, dy)
template <class Tap, class Weight>
PT_HD float sel_dilate(int32_t R, Tap&& tap, Weight&& weight) {
  float D = 0.0f;
  for (int32_t dy = -R; dy <= R; dy++)
    for (int32_t dx = -R; dx <= R; dx++) D = fmaxf(D, tap(dx, dy) * weight(dx, dy));
  return D;
}

PT_HD float sel_mix(float c, float s, float a) { return c * (1.0f - a) + s * a; }

// One pixel of the target (0xAABBGGRR) under coverage m and dilation D.  Alpha 0 keeps a byte and alpha 1 gives exactly the packed colour;
// with both alphas 0 the pixel keeps its four bytes, and the alpha byte is never changed (a render target's is 255).
PT_HD uint32_t sel_composite(uint32_t rgba8, float m, float D, const SelParams& P) {
  const float af = m * P.fill[3], ao = (D - m) * P.outline[3];
  if (af == 0.0f && ao == 0.0f) return rgba8;
  vec3 c;
  c.x = (float)(rgba8 & 255u) / 255.0f; c.y = (float)((rgba8 >> 8) & 255u) / 255.0f; c.z = (float)((rgba8 >> 16) & 255u) / 255.0f;
  c.x = sel_mix(sel_mix(c.x, P.fill[0], af), P.outline[0], ao);
  c.y = sel_mix(sel_mix(c.y, P.fill[1], af), P.outline[1], ao);
  c.z = sel_mix(sel_mix(c.z, P.fill[2], af), P.outline[2], ao);
  return (pp_pack_rgba8(c) & 0x00ffffffu) | (rgba8 & 0xff000000u);
}

// pt_set_selection_options' test, shared with pt_debug_selection_overlay; null = valid, otherwise what is wrong
PT_HD const char* selection_options_error(const pt_selection_options& o) {
  if (o.layer > PT_MATTE_MATERIAL) return "no such layer";
  if (!(o.width >= 1.0f && o.width <= 16.0f)) return "1 <= width <= 16 is required";
  for (int k = 0; k < 4; k++) {
    if (!(o.outline_rgba[k] >= 0.0f && o.outline_rgba[k] <= 1.0f)) return "every outline_rgba component must lie in [0, 1]";
    if (!(o.fill_rgba[k] >= 0.0f && o.fill_rgba[k] <= 1.0f)) return "every fill_rgba component must lie in [0, 1]";
  }
  return nullptr;
}

}  // namespace pt
