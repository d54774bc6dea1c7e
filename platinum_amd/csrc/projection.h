// projection.h — host-visible launchers of the projected ray generation (projection.hip; the arithmetic in pt_projection.h).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pt_projection.h"

namespace pt {

// launch_raygen's counterpart for a render whose projection is not PT_PROJ_PERSPECTIVE: the same queue, Lbuf, segment counts and wave
// statistics, the rays of `P`.  `tiles` null: the full frame; else the active tiles and rectangle of an adaptive or region render.
void launch_raygen_projected(hipStream_t s, uint32_t grid, const DeviceScene& S, const ProjectionConstants& P, PathState st, vec4* Lbuf, Segments seg,
                             uint32_t first_sample, uint32_t nsamples, const TileSet* tiles);
// The bounce-0 queue of a ONE-sample full-frame batch scattered to pixel order (pt_debug_camera_rays): origins / directions [pixel][3], either
// may be null.
void launch_camera_rays(hipStream_t s, uint32_t grid, uint32_t width, PathState st, Segments seg, float* origins, float* directions);

}  // namespace pt
