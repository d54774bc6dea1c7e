// TEST HARNESS ONLY (tests/emu) — the host build of the selection overlay (platinum_amd/csrc/pt_selection.h), twice: the per-pixel
// definition, and the kernel's own way block by block (staging through sel_tile_pixel into an LDS-sized array, the weight table, the two
// block votes, the tap loop from the tile); for tests/test_selection_host.py and tests/test_gpu_selection.py.
// Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// A translation unit of its own: tests/selection_lib.py builds it into tests/_build/libptamd_selection.so (tests/host_build.py load).
// With -DSELECTION_EMU_MAIN it is a stand-alone program that drives both paths over the tests' sizes and widths (a sanitizer build runs it).
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../platinum_amd/csrc/pt_selection.h"

using namespace pt;

extern "C" {

int32_t sel_host_radius(float width) { return sel_radius(width); }
float sel_host_weight(float width, int32_t dx, int32_t dy) { return sel_weight(sel_limit(width), dx, dy); }
// 1 when pt_set_selection_options would accept the options
uint32_t sel_host_options_valid(const pt_selection_options* o) { return selection_options_error(*o) == nullptr; }
uint32_t sel_host_pack(const float* rgb) { return pp_pack_rgba8(vec3{rgb[0], rgb[1], rgb[2]}); }
uint32_t sel_host_block() { return kSelBlock; }
// the tile map: 1 and (x, y) in xy_out for an in-image texel, 0 otherwise
uint32_t sel_host_tile_pixel(uint32_t bx, uint32_t by, int32_t R, uint32_t t, uint32_t W, uint32_t H, uint32_t* xy_out) {
  return sel_tile_pixel(bx, by, R, t, W, H, &xy_out[0], &xy_out[1]) ? 1u : 0u;
}
uint32_t sel_host_tile_texel(int32_t R, uint32_t lx, uint32_t ly, int32_t dx, int32_t dy) { return sel_tile_texel(R, lx, ly, dx, dy); }

static float dilate_pixel(const float* cov, uint32_t W, uint32_t H, uint32_t x, uint32_t y, const SelParams& P) {
  return sel_dilate(
      P.R,
      [&](int32_t dx, int32_t dy) {
        const int64_t qx = (int64_t)x + dx, qy = (int64_t)y + dy;
        return qx < 0 || qy < 0 || qx >= (int64_t)W || qy >= (int64_t)H ? 0.0f : cov[(size_t)qy * W + (size_t)qx];
      },
      [&](int32_t dx, int32_t dy) { return sel_weight(P.lim, dx, dy); });
}

// the two alphas of every pixel, by the definition
void sel_host_alphas(const float* cov, uint32_t W, uint32_t H, const pt_selection_options* o, float* fill_alpha, float* outline_alpha) {
  const SelParams P = sel_params(*o);
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++) {
      const float m = cov[(size_t)y * W + x], D = dilate_pixel(cov, W, H, x, y, P);
      fill_alpha[(size_t)y * W + x] = m * P.fill[3];
      outline_alpha[(size_t)y * W + x] = (D - m) * P.outline[3];
    }
}

// The definition, pixel by pixel.  `enabled` is not looked at.
void sel_host_overlay(const uint32_t* rgba8, const float* cov, uint32_t W, uint32_t H, const pt_selection_options* o, uint32_t* out) {
  const SelParams P = sel_params(*o);
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++) {
      const size_t p = (size_t)y * W + x;
      out[p] = sel_composite(rgba8[p], cov[p], dilate_pixel(cov, W, H, x, y, P), P);
    }
}

// k_selection_overlay block by block.  Returns 0, or 1 when an address fell outside the tile or the table.  blocks_out (may be null):
// {blocks, blocks that returned at the first vote, blocks that skipped the tap loop at the second}.
int32_t sel_host_overlay_blocks(const uint32_t* rgba8, const float* cov, uint32_t W, uint32_t H, const pt_selection_options* o, uint32_t early_out,
                                uint32_t* out, uint32_t* blocks_out) {
  const SelParams P = sel_params(*o);
  const int32_t R = P.R;
  if (R < 0 || R > kSelMaxRadius) return 1;
  const uint32_t T = sel_tile_side(R), taps = 2u * (uint32_t)R + 1u;
  const uint32_t blocks_x = (W + kSelBlock - 1u) / kSelBlock, blocks_y = (H + kSelBlock - 1u) / kSelBlock;
  std::memcpy(out, rgba8, (size_t)W * H * 4);
  uint32_t stats[3] = {blocks_x * blocks_y, 0u, 0u};
  int32_t bad = 0;
  for (uint32_t b = 0; b < blocks_x * blocks_y; b++) {
    std::vector<float> tile((size_t)kSelTileMax * kSelTileMax), weights((size_t)kSelTapsMax * kSelTapsMax);   // the two LDS arrays, their real size
    const uint32_t by = b / blocks_x, bx = b - by * blocks_x;
    bool some = false, ones = true;
    for (uint32_t t = 0; t < T * T; t++) {
      uint32_t x, y;
      const float v = sel_tile_pixel(bx, by, R, t, W, H, &x, &y) ? cov[(size_t)y * W + x] : 0.0f;
      tile.at(t) = v;
      some = some || v != 0.0f;
      ones = ones && v == 1.0f;
    }
    for (uint32_t i = 0; i < taps * taps; i++) {
      const uint32_t j = i / taps;
      weights.at(i) = sel_weight(P.lim, (int32_t)(i - j * taps) - R, (int32_t)j - R);
    }
    if (early_out && !some) { stats[1]++; continue; }
    if (ones) stats[2]++;
    for (uint32_t l = 0; l < kSelBlock * kSelBlock; l++) {
      const uint32_t lx = l & (kSelBlock - 1u), ly = l / kSelBlock;
      const uint32_t x = bx * kSelBlock + lx, y = by * kSelBlock + ly;
      if (x >= W || y >= H) continue;
      const uint32_t centre = sel_tile_texel(R, lx, ly, 0, 0), wc = (uint32_t)R * taps + (uint32_t)R;
      const float m = tile.at(centre);
      const float D = ones ? m
                           : sel_dilate(
                                 R,
                                 [&](int32_t dx, int32_t dy) {
                                   const int64_t a = (int64_t)centre + (int64_t)dy * T + dx;
                                   if (a < 0 || a >= (int64_t)T * T || a != (int64_t)sel_tile_texel(R, lx, ly, dx, dy)) { bad = 1; return 0.0f; }
                                   return tile[(size_t)a];
                                 },
                                 [&](int32_t dx, int32_t dy) {
                                   const int64_t a = (int64_t)wc + (int64_t)dy * taps + dx;
                                   if (a < 0 || a >= (int64_t)taps * taps) { bad = 1; return 0.0f; }
                                   return weights[(size_t)a];
                                 });
      const size_t p = (size_t)y * W + x;
      out[p] = sel_composite(rgba8[p], m, D, P);
    }
  }
  if (blocks_out) std::memcpy(blocks_out, stats, sizeof(stats));
  return bad;
}

// sizeof / offsetof of the struct as this compiler lays it out, and the kernel's constants
void sel_host_layout(uint32_t out[11]) {
  uint32_t k = 0;
  out[k++] = sizeof(pt_selection_options);
  out[k++] = offsetof(pt_selection_options, enabled); out[k++] = offsetof(pt_selection_options, layer); out[k++] = offsetof(pt_selection_options, width);
  out[k++] = offsetof(pt_selection_options, _pad); out[k++] = offsetof(pt_selection_options, outline_rgba); out[k++] = offsetof(pt_selection_options, fill_rgba);
  out[k++] = kSelBlock; out[k++] = (uint32_t)kSelMaxRadius; out[k++] = kSelTileMax; out[k++] = kSelTapsMax;
}

}  // extern "C"

#ifdef SELECTION_EMU_MAIN
int main() {
  const uint32_t sizes[][2] = {{1, 1}, {2, 1}, {1, 7}, {3, 2}, {16, 16}, {17, 15}, {33, 31}, {67, 45}, {300, 3}};
  const float widths[] = {1.0f, 1.5f, 2.0f, 7.25f, 16.0f};
  uint32_t s = 12345u;
  auto next = [&]() { s = s * 1664525u + 1013904223u; return s; };
  for (const auto& wh : sizes)
    for (const float width : widths)
      for (int card = 0; card < 4; card++) {
        const uint32_t W = wh[0], H = wh[1];
        const size_t npix = (size_t)W * H;
        std::vector<uint32_t> img(npix), a(npix), b(npix);
        std::vector<float> cov(npix, 0.0f);
        for (auto& v : img) v = next();
        if (card == 1) for (auto& v : cov) v = 1.0f;
        if (card == 2) for (auto& v : cov) v = (float)(next() >> 8) * (1.0f / 16777216.0f);
        if (card == 3) cov[npix / 2] = 1.0f;
        pt_selection_options o{1u, 0u, width, 0.0f, {1.0f, 0.55f, 0.0f, 1.0f}, {0.2f, 0.4f, 1.0f, 0.5f}};
        if (selection_options_error(o)) return 1;
        uint32_t blocks[3];
        sel_host_overlay(img.data(), cov.data(), W, H, &o, a.data());
        if (sel_host_overlay_blocks(img.data(), cov.data(), W, H, &o, 1u, b.data(), blocks)) return 2;
        if (std::memcmp(a.data(), b.data(), npix * 4)) return 3;
        if (sel_host_overlay_blocks(img.data(), cov.data(), W, H, &o, 0u, b.data(), nullptr)) return 2;
        if (std::memcmp(a.data(), b.data(), npix * 4)) return 3;
        size_t changed = 0;
        for (size_t p = 0; p < npix; p++) changed += a[p] != img[p];
        printf("%u x %u, width %g (R %d), card %d: %zu pixels drawn, %u blocks (%u returned early, %u tint only)\n", W, H, width, sel_radius(width), card,
               changed, blocks[0], blocks[1], blocks[2]);
        if (card == 0 && (changed || blocks[1] != blocks[0])) return 4;
      }
  return 0;
}
#endif
