// bloom.h — host-side launch interface of bloom.hip: the glare pyramid ahead of the post-process.
#pragma once
#include <hip/hip_runtime.h>

#include "pt_bloom.h"

namespace pt {

// Blooms the plan's frame `img` into `out` (another image of the frame's size) through `pyramid` (plan.total_texels texels, which hold
// U_1..U_L afterwards): k_bloom_down0, k_bloom_down per level, k_bloom_up per level, k_bloom_composite.  plan.levels == 0 (a 1 x 1 frame)
// copies.  Returns the copy's or the launches' error.
hipError_t launch_bloom(hipStream_t s, const vec4* img, vec4* out, vec4* pyramid, const pt_bloom_plan& plan, const pt_bloom_options& o);

}  // namespace pt
