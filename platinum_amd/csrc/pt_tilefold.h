// pt_tilefold.h — what every per-sample side channel of a batch shares, defined ONCE (DESIGN.md §3 "Tile folds and queue walks"): how a
// fold kernel places its tile in the image, the order in which a round of eight samples goes through LDS, and the walk over a segment of the
// bounce-0 queue that fills a side channel.  kernels.hip (Lbuf), denoise.hip (Abuf), matte.hip (Mbuf), film.hip (Fbuf) and ao.hip (Obuf) call it; a new
// side channel starts here.  One that needs a trace of its own (Obuf: ambient occlusion, pt_ao.h) is filled by a consumer of the bounce-0 chunk
// table over the trace kernels' ray loop instead of the walk (k_trace_ao, kernels.hip), forms its pid as the walk does, and folds like the
// others.  The first two are plain integer functions (PT_HD) that tests/emu also compiles for the host; the walk is device code.
#pragma once
#include "pt_device.h"
#include "pt_layout.h"
#if defined(__HIPCC__)
#include "kernels.h"
#endif

namespace pt {

// ---- the tile of a fold kernel -----------------------------------------------------------------------------------------
// One wave folds one 8x8 tile, lane = pixel.  Full frame: `tile` is the image tile and a lane is inside when its pixel is in the image.
// ADAPTIVE (adaptive and region renders): `tile` is a VIRTUAL tile — the per-sample buffers are dense over those — that is live below
// *active_count and then stands for image tile active[tile]; a lane is inside when its pixel is in `rect`.  `live` says whether the wave has
// samples to stage, `inside` whether the lane has a pixel to fold: at a region's border a live tile has lanes that are not inside.
struct FoldTile {
  uint32_t tile, itile;   // as addressed in the per-sample buffers (lbuf_index) / in the image
  bool live, inside;
  PixelXY q;              // the lane's pixel (meaningful when inside)
};
template <bool ADAPTIVE>
PT_HD FoldTile fold_tile(uint32_t tile, uint32_t lane, uint32_t width, uint32_t height, const uint32_t* active, const uint32_t* active_count,
                         const Rect& rect) {
  const uint32_t tilesX = tiles_x(width), tiles = ADAPTIVE ? *active_count : tilesX * tiles_y(height);
  const bool live = tile < tiles;
  const uint32_t itile = ADAPTIVE ? (live ? active[tile] : 0u) : tile;
  const PixelXY q = tile_pixel(itile, lane, tilesX);
  const bool inside = live && (ADAPTIVE ? rect_contains(rect, q.x, q.y) : q.x < width && q.y < height);
  return {tile, itile, live, inside, q};
}
// ---- one staging round ---------------------------------------------------------------------------------------------------
// A tile's entries are [pixel][sample] (lbuf_index): samples s0 .. s0 + nb - 1 (nb <= 8) of eight pixels are 8 x 128 contiguous bytes of vec4,
// so the wave loads 64 pixels x 8 samples in eight steps, eight lanes per pixel and one per sample, fully coalesced, and turns them through
// LDS: load(pid, slot) moves entry `pid` to slot pixel * kFoldRow + (s - s0); after a barrier lane p folds slots p * kFoldRow + 0 .. nb - 1
// in order.  UNROLL: how many of the eight loads a lane keeps in flight.
constexpr uint32_t kFoldRow = 9;  // slots per pixel row in LDS (8 samples + 1 of padding against bank conflicts)
template <uint32_t UNROLL = 8, class Load>
PT_HD void fold_stage(uint32_t tile, uint32_t lane, uint32_t s0, uint32_t nb, uint32_t nsamples, Load load) {
#pragma unroll UNROLL
  for (uint32_t i = 0; i < 8u; i++) {
    const uint32_t px = i * 8u + (lane >> 3), j = lane & 7u;
    if (j < nb) load(lbuf_index(tile, s0 + j, nsamples, px), px * kFoldRow + j);
  }
}
#if defined(__HIPCC__)
// ---- the walk over the bounce-0 queue --------------------------------------------------------------------------------------
// Between the camera trace of a batch and k_shade(0) state buffer 0 holds the camera rays.  Wave w takes segments w, w + waves, ... (the
// kernel's loop: in here it changes the kernel's scalar loads); f(i, pid, hit_word) gets each ray's queue slot, Lbuf entry and hit word 3.
template <class F>
__device__ __forceinline__ void walk_bounce0(const Segments& seg, const PathState& st, const vec4* __restrict__ hit, uint32_t sg, uint32_t lane, F f) {
  const uint32_t n = seg.active[0][sg];
  const uint32_t base = segment_lbuf_base(seg, sg);
  for (uint32_t k = lane; k < n; k += 64) {
    const uint32_t i = seg_slot(seg.nseg, sg, k);
    const vec4 h4 = hit[i], d4 = st.rayD[i];
    f(i, base + (f2u(d4.w) >> kMetaPidShift), f2u(h4.w));
  }
}
#endif

}  // namespace pt
