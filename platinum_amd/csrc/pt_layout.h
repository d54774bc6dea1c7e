// pt_layout.h — the three index maps that tie the wavefront together, defined ONCE: 8x8 pixel tiles, the queue segments and the
// per-sample radiance buffer Lbuf.  Every kernel, launcher, allocation, host read-back and emulator that needs one of them calls
// this header; nothing else spells the arithmetic out.  Plain integer functions (PT_HD, no HIP types): the same code for hipcc
// (host and device) and for the g++ builds under tests/emu.
#pragma once
#include "pt_math.h"

namespace pt {

// ---- tiles -----------------------------------------------------------------------------------------------------------
// The image is cut into 8x8 pixel tiles, row-major; tiles on the right and bottom edge may be partial.  `lane` is a pixel's
// place in its tile, row-major too: one wave covers a tile with one lane per pixel.
PT_HD uint32_t tiles_x(uint32_t W) { return (W + 7u) / 8u; }
PT_HD uint32_t tiles_y(uint32_t H) { return (H + 7u) / 8u; }
PT_HD uint32_t tile_count(uint32_t W, uint32_t H) { return tiles_x(W) * tiles_y(H); }
PT_HD uint32_t tile_of_pixel(uint32_t x, uint32_t y, uint32_t W) { return (y >> 3) * tiles_x(W) + (x >> 3); }
PT_HD uint32_t lane_of_pixel(uint32_t x, uint32_t y) { return (y & 7u) * 8u + (x & 7u); }
struct PixelXY { uint32_t x, y; };
// (the lanes of a partial tile that fall outside the image get x >= W or y >= H)
PT_HD PixelXY tile_pixel(uint32_t tile, uint32_t lane, uint32_t tilesX) {
  const uint32_t ty = tile / tilesX;
  return {(tile - ty * tilesX) * 8u + (lane & 7u), ty * 8u + (lane >> 3)};
}

// A pixel rectangle [x0, x1) x [y0, y1), top-left origin: what a render samples (a render region; the whole frame
// otherwise).  The kernels that place a virtual tile in the image take it as their validity test.
struct Rect { uint32_t x0, y0, x1, y1; };
PT_HD bool rect_contains(const Rect& r, uint32_t x, uint32_t y) { return x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1; }
// The image tiles a non-empty rectangle inside a W-wide image touches, ascending: rows of tiles [y0 / 8, (y1 - 1) / 8], in each the tiles
// [x0 / 8, (x1 - 1) / 8].  Writes the first `capacity` of them to `out` (may be null) and returns their number.
PT_HD uint32_t rect_tiles(const Rect& r, uint32_t W, uint32_t* out, uint32_t capacity) {
  const uint32_t tilesX = tiles_x(W), tx0 = r.x0 >> 3, tx1 = (r.x1 - 1u) >> 3, ty0 = r.y0 >> 3, ty1 = (r.y1 - 1u) >> 3;
  uint32_t n = 0;
  for (uint32_t ty = ty0; ty <= ty1; ty++)
    for (uint32_t tx = tx0; tx <= tx1; tx++, n++)
      if (out && n < capacity) out[n] = ty * tilesX + tx;
  return n;
}

// ---- the per-sample radiance buffer Lbuf -----------------------------------------------------------------------------
// One vec4 per (pixel, sample in flight), laid out TILE-major: the entries of one 8x8 tile under all samples are contiguous (128 KB at 128
// samples in flight) and a segment's rays all belong to its tile(s): the shadow kernel's read-modify-writes of a segment stay inside that
// window (a [sample][pixel] layout spread them over planes 33 MB apart: every access its own line).  `pid` in the path state IS this index.
// Inside a tile the order is [pixel][sample] (r4; r1-r3 had [sample][pixel]): the camera rays of a chunk are 64 SAMPLES OF ONE PIXEL
// (k_raygen), so a chunk's 64 entries are 1 KB contiguous here too, and k_accumulate folds a pixel's samples from consecutive words.
// Whole tiles: tile_count * 64 * nsamples entries.
PT_HD uint32_t lbuf_index(uint32_t tile, uint32_t s, uint32_t nsamples, uint32_t lane) { return (tile * 64u + lane) * nsamples + s; }
// ... of pixel p (row-major) of a W-wide image
PT_HD uint32_t lbuf_index_of_pixel(uint32_t p, uint32_t W, uint32_t s, uint32_t nsamples) {
  const uint32_t y = p / W, x = p - y * W;
  return lbuf_index(tile_of_pixel(x, y, W), s, nsamples, lane_of_pixel(x, y));
}
// the pixel (row-major) of a pid of a ONE-sample batch (the debug entry points: pt_trace_primary, pt_debug_sample): lbuf_index(tile, 0, 1,
// lane) = tile * 64 + lane, inverted, then tile_pixel.  (Spelt out: the trace kernels' hit log keeps the instruction order it had.)
PT_HD uint32_t pixel_of_pid_1spp(uint32_t pid, uint32_t W) {
  const uint32_t lane = pid & 63u, tile = pid >> 6, tilesX = tiles_x(W);
  const uint32_t ty = tile / tilesX, tx = tile - ty * tilesX;
  return (ty * 8u + (lane >> 3)) * W + tx * 8u + (lane & 7u);
}
// ... of a batch of `nsamples`: a pixel's samples are consecutive, so pid / nsamples = tile * 64 + lane, the pixel's SLOT in tile-major order
// (what the camera-ray lists are indexed by: pt_camlist.h), and that is the pid of the one-sample layout.
PT_HD uint32_t pixel_slot_of_pid(uint32_t pid, uint32_t nsamples) { return nsamples == 1u ? pid : pid / nsamples; }
PT_HD uint32_t pixel_of_pid(uint32_t pid, uint32_t nsamples, uint32_t W) { return pixel_of_pid_1spp(pixel_slot_of_pid(pid, nsamples), W); }

// ---- queue segments --------------------------------------------------------------------------------------------------
// Slot of entry r of segment s.  Segments are interleaved in GROUPS of PT_SEG_GROUP 64-entry chunks: chunks 16g .. 16g + 15 of a
// segment are contiguous (16 KB per array), group g of neighbouring segments follows — a segment's entries are a few long runs
// (the class-binned passes of k_shade gather from them; +1 % over single-chunk interleaving), while concurrently processed
// segments still start in different memory channels (a plain segment-major layout cost the closest-hit kernel 1.4x in round 1).
#ifndef PT_SEG_GROUP
#define PT_SEG_GROUP 16
#endif
constexpr uint32_t kSegGroupChunks = PT_SEG_GROUP;
PT_HD uint32_t seg_slot(uint32_t nseg, uint32_t s, uint32_t r) {
  const uint32_t k = r >> 6;
  return (((k / kSegGroupChunks) * nseg + s) * kSegGroupChunks + (k % kSegGroupChunks)) * 64u + (r & 63u);
}
// the segment a queue slot belongs to (inverse of seg_slot)
PT_HD uint32_t slot_segment(uint32_t nseg, uint32_t slot) { return ((slot >> 6) / kSegGroupChunks) % nseg; }
// slots of a queue array that holds nseg segments of seg_cap entries each: every segment's last group is allocated whole
PT_HD uint64_t seg_queue_slots(uint32_t nseg, uint32_t seg_cap) {
  const uint64_t K = seg_cap / 64u;
  return (uint64_t)nseg * ((K + kSegGroupChunks - 1) / kSegGroupChunks * kSegGroupChunks) * 64;
}
// Segment sg is the queue share of tiles [first, first + tiles_per_seg).  Consecutive segments cycle over `bands` horizontal bands
// of the image (the chunk tables list the segments in order, so the rays in flight in a trace kernel come from `bands`
// neighbourhoods instead of one); nseg is a multiple of bands.
PT_HD uint32_t segment_first_tile(uint32_t nseg, uint32_t bands, uint32_t tiles_per_seg, uint32_t sg) {
  const uint32_t per_band = nseg / bands;
  return ((sg % bands) * per_band + sg / bands) * tiles_per_seg;
}
// A segment's window of Lbuf starts at its first tile; a path's entry is that base + the relative index it carries in rayD.w.
PT_HD uint32_t segment_lbuf_base(uint32_t nseg, uint32_t bands, uint32_t tiles_per_seg, uint32_t nsamples, uint32_t sg) {
  return segment_first_tile(nseg, bands, tiles_per_seg, sg) * nsamples * 64u;
}


// ---- where a camera ray lands in its segment ---------------------------------------------------------------------------
// k_raygen walks a segment's tiles in order and each tile's 64 * nsamples rays pixel-major, sample-minor (ray r of a tile: pixel lane
// r / nsamples, sample r % nsamples), 64 rays per wave iteration, and packs the rays of the pixels inside the image by ballot: packing keeps
// the order.  The pixels of a tile inside the image form a rectangle vw x vh at the tile's origin, so a ray's place in its segment is a closed
// form: (valid pixels before its pixel in the segment) * nsamples + sample.  k_camera_primary (kernels.hip) places a run of a segment's rays
// with it, without the rays before them.
PT_HD uint32_t tile_valid_w(uint32_t tile, uint32_t tilesX, uint32_t W) {
  const uint32_t x0 = (tile % tilesX) * 8u;
  return x0 >= W ? 0u : (W - x0 < 8u ? W - x0 : 8u);
}
PT_HD uint32_t tile_valid_h(uint32_t tile, uint32_t tilesX, uint32_t H) {
  const uint32_t y0 = (tile / tilesX) * 8u;
  return y0 >= H ? 0u : (H - y0 < 8u ? H - y0 : 8u);
}
// valid pixels of a tile whose lane is below `lane` (lane <= 64)
PT_HD uint32_t tile_pixels_before(uint32_t lane, uint32_t vw, uint32_t vh) {
  const uint32_t y = lane >> 3, x = lane & 7u;
  return (y < vh ? y : vh) * vw + (y < vh ? (x < vw ? x : vw) : 0u);
}
// valid rays among rays [0, r) of a tile (r <= 64 * nsamples)
PT_HD uint32_t tile_rays_before(uint32_t r, uint32_t nsamples, uint32_t vw, uint32_t vh) {
  const uint32_t pl = r / nsamples, s = r - pl * nsamples;
  const bool in = pl < 64u && (pl & 7u) < vw && (pl >> 3) < vh;
  return tile_pixels_before(pl, vw, vh) * nsamples + (in ? s : 0u);
}
// Entry index (the r of seg_slot) of the first ray of wave iteration k of a segment whose first tile is `first_tile`: iteration k covers rays
// [(k % nsamples) * 64, + 64) of tile first_tile + k / nsamples.  With k = tiles_per_seg * nsamples: the segment's ray count.  Tiles at or past
// `tiles` (the segments behind the image's last tile) hold nothing.
PT_HD uint32_t camera_rays_before(uint32_t first_tile, uint32_t k, uint32_t nsamples, uint32_t tilesX, uint32_t tiles, uint32_t W, uint32_t H) {
  const uint32_t t_end = k / nsamples;
  uint32_t n = 0;
  for (uint32_t t = 0; t < t_end && first_tile + t < tiles; t++)
    n += tile_valid_w(first_tile + t, tilesX, W) * tile_valid_h(first_tile + t, tilesX, H) * nsamples;
  const uint32_t tile = first_tile + t_end;
  if (tile < tiles) n += tile_rays_before((k - t_end * nsamples) * 64u, nsamples, tile_valid_w(tile, tilesX, W), tile_valid_h(tile, tilesX, H));
  return n;
}

}  // namespace pt
