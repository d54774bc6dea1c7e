// ao.h — host-visible launchers of the ambient-occlusion fold and scatter kernels (ao.hip; the AO ray, the fold and the resolve in pt_ao.h;
// the trace itself is k_trace_ao in kernels.hip, launch_trace_ao in kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pt_ao.h"

namespace pt {

// After the accumulate kernels: the batch's states Obuf folded into counts[pixel] = {hits, open}; over `tiles` (an adaptive or region
// render) when not null, else over the whole frame.
void launch_accumulate_ao(hipStream_t s, uint2* counts, const uint32_t* Obuf, uint32_t width, uint32_t height, uint32_t nsamples, const TileSet* tiles);
// pt_debug_ao: the states of a one-sample batch from Obuf to pixel order (pixels whose camera ray is not in the queue are left alone)
void launch_ao_scatter(hipStream_t s, uint32_t grid, uint32_t width, PathState st, const vec4* hit, Segments seg, const uint32_t* Obuf, uint32_t* state);

}  // namespace pt
