// view.h — host-side launch interface of view.hip: the data views of the render target (pt_view.h holds the arithmetic).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_view.h"

namespace pt {

// The images a data view reads, all W x H and row-major; a pointer the view does not read may be null.
struct ViewImages {
  const vec4* normal;       // the normal AOV {N, h}
  const vec4* moments;      // the moments AOV {r, m1, m2, _}, or null: NOISE reads mom2
  const vec2* mom2;         // the adaptive moments {m1, m2}
  const vec4* film;         // {premultiplied foreground, a}
  const uint4* slots;       // the first slot pair of the layer shown, of pixel 0
  uint32_t slot_stride;     // uint4 between two pixels' slots: 4 for one layer alone, kMattePixelVec4 for the renderer's slot image
  // the pixel's sample count n: counts[pixel], or with counts null tile_n[its tile] inside `rect` and 0 outside it, or with both null n_uniform
  const uint32_t* counts;
  const uint32_t* tile_n;
  uint32_t n_uniform;
  Rect rect;                // the render's rectangle: what the depth range is taken over
  uint32_t width, height;
};

// The depth range of `rect` into *rec, which is cleared first: one k_view_range block per 256 pixels up to 2048 blocks, at most one integer
// atomic per field and block (none for a bound the record already holds).  `count`: also the number of valid pixels, one add per block; a
// present leaves it out.  Reads normal, moments and the counts.
hipError_t launch_view_range(hipStream_t s, const ViewImages& I, ViewRecord* rec, bool count);
// One data view onto the W x H target (0xAABBGGRR per pixel), one lane per pixel.  `rec` is read under DEPTH with auto_range only.
void launch_view_pass(hipStream_t s, const ViewImages& I, const ViewParams& P, const ViewRecord* rec, uint32_t* target);

}  // namespace pt
