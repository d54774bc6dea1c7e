// TEST HARNESS ONLY (tests/emu) — the host build of the index maps of platinum_amd/csrc/pt_layout.h, of the tile folds' addressing
// (pt_tilefold.h) and of plan_queues (queue_plan.h), one table per map, for tests/test_layout_host.py.  Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// Fifth part of tests/emu/host_harness.cpp; not compiled alone.
#ifndef PTAMD_TESTS_EMU_LAYOUT_PROBE
#define PTAMD_TESTS_EMU_LAYOUT_PROBE
#include "../../platinum_amd/csrc/pt_device.h"
#include "../../platinum_amd/csrc/pt_layout.h"
#include "../../platinum_amd/csrc/pt_tilefold.h"
#include "../../platinum_amd/csrc/queue_plan.h"

using namespace pt;

extern "C" {

int lp_plan(uint32_t W, uint32_t H, uint32_t nsamples, uint32_t tiles_per_seg_override, uint32_t seg_bands, pt_queue_plan* out) {
  const char* why = "";
  return plan_queues(W, H, nsamples, nsamples, 0, tiles_per_seg_override, seg_bands, out, &why);
}
uint32_t lp_meta_pid_bits() { return 32u - kMetaPidShift; }  // the pid relative to the segment's window rides in these bits of rayD.w
uint32_t lp_tile_count(uint32_t W, uint32_t H) { return tile_count(W, H); }
uint64_t lp_seg_queue_slots(uint32_t nseg, uint32_t seg_cap) { return seg_queue_slots(nseg, seg_cap); }

// slot[sg * seg_cap + r] = seg_slot(sg, r); owner[...] = slot_segment of that slot
void lp_slots(uint32_t nseg, uint32_t seg_cap, uint32_t* slot, uint32_t* owner) {
  for (uint32_t sg = 0; sg < nseg; sg++)
    for (uint32_t r = 0; r < seg_cap; r++) {
      const size_t at = (size_t)sg * seg_cap + r;
      slot[at] = seg_slot(nseg, sg, r);
      owner[at] = slot_segment(nseg, slot[at]);
    }
}
void lp_segments(uint32_t nseg, uint32_t bands, uint32_t tiles_per_seg, uint32_t nsamples, uint32_t* first_tile, uint32_t* lbuf_base) {
  for (uint32_t sg = 0; sg < nseg; sg++) {
    first_tile[sg] = segment_first_tile(nseg, bands, tiles_per_seg, sg);
    lbuf_base[sg] = segment_lbuf_base(nseg, bands, tiles_per_seg, nsamples, sg);
  }
}
// out[(tile * 64 + lane) * nsamples + s], enumeration order (NOT the layout under test)
void lp_lbuf(uint32_t tiles, uint32_t nsamples, uint32_t* out) {
  for (uint32_t t = 0; t < tiles; t++)
    for (uint32_t l = 0; l < 64; l++)
      for (uint32_t s = 0; s < nsamples; s++) *out++ = lbuf_index(t, s, nsamples, l);
}
// per pixel (row-major): its tile, its lane, lbuf_index_of_pixel(p, W, 0, 1) and pixel_of_pid_1spp of that
void lp_pixels(uint32_t W, uint32_t H, uint32_t* tile, uint32_t* lane, uint32_t* pid1, uint32_t* back) {
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++) {
      const uint32_t p = y * W + x;
      tile[p] = tile_of_pixel(x, y, W);
      lane[p] = lane_of_pixel(x, y);
      pid1[p] = lbuf_index_of_pixel(p, W, 0, 1);
      back[p] = pixel_of_pid_1spp(pid1[p], W);
    }
}
// xy[(tile * 64 + lane) * 2] = tile_pixel(tile, lane)
void lp_tile_pixels(uint32_t W, uint32_t H, uint32_t* xy) {
  for (uint32_t t = 0; t < tile_count(W, H); t++)
    for (uint32_t l = 0; l < 64; l++) {
      const PixelXY q = tile_pixel(t, l, tiles_x(W));
      *xy++ = q.x;
      *xy++ = q.y;
    }
}

// fold_tile of every (tile < ntiles, lane): out[(tile * 64 + lane) * 5] = {itile, live, inside, q.x, q.y}.  active == null: the full-frame
// form (rect unused); else virtual tiles over the list active[0, *active_count), with rect = {x0, y0, x1, y1}.
void lp_fold_tiles(uint32_t W, uint32_t H, uint32_t ntiles, const uint32_t* active, const uint32_t* active_count, const uint32_t* rect,
                   uint32_t* out) {
  const Rect r = rect ? Rect{rect[0], rect[1], rect[2], rect[3]} : Rect{};
  for (uint32_t t = 0; t < ntiles; t++)
    for (uint32_t l = 0; l < 64; l++) {
      const FoldTile f = active ? fold_tile<true>(t, l, W, H, active, active_count, r) : fold_tile<false>(t, l, W, H, nullptr, nullptr, r);
      *out++ = f.itile; *out++ = f.live; *out++ = f.inside; *out++ = f.q.x; *out++ = f.q.y;
    }
}
// the (pid, slot) pairs of one staging round of `tile` (samples s0 .. s0 + nb - 1 of nsamples), lane by lane in fold_stage's order; returns
// their number (<= 512 pairs)
uint32_t lp_fold_stage(uint32_t tile, uint32_t s0, uint32_t nb, uint32_t nsamples, uint32_t* out) {
  uint32_t n = 0;
  for (uint32_t l = 0; l < 64; l++)
    fold_stage(tile, l, s0, nb, nsamples, [&](uint32_t pid, uint32_t slot) { out[2 * n] = pid; out[2 * n + 1] = slot; n++; });
  return n;
}
uint32_t lp_fold_row() { return kFoldRow; }

}  // extern "C"

#endif  // PTAMD_TESTS_EMU_LAYOUT_PROBE
