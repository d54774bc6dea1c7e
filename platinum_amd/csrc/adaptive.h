// adaptive.h — host-visible launchers of the tile-adaptive checkpoint (adaptive.hip; the criterion is pt_adaptive.h).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_layout.h"

namespace pt {

// Bytes of device scratch the compaction needs for an image of `tiles` 8x8 tiles.
size_t adaptive_scratch_bytes(uint32_t tiles);
// The checkpoint after n samples: tests the *count_in tiles of list_in against the per-pixel (lum, lum^2) means `mom` (of a W-wide image),
// writes the still active ones in ascending order to list_out and their number to *count_out, and enqueues a copy of that number to
// host_count (pinned).  A tile's verdict is taken over its pixels inside `rect` (the whole frame, or the render region).  tiles: the length
// of the lists (>= *count_in: the render's first list); flags: one byte per tile of scratch; scratch: adaptive_scratch_bytes(tiles).
// Everything is enqueued on `s`.
hipError_t launch_adaptive_check(hipStream_t s, const uint32_t* list_in, const uint32_t* count_in, uint32_t* list_out, uint32_t* count_out,
                                 const vec2* mom, uint32_t W, const Rect& rect, uint32_t tiles, uint32_t n, float threshold, uint8_t* flags,
                                 void* scratch, size_t scratch_bytes, uint32_t* host_count);

}  // namespace pt
