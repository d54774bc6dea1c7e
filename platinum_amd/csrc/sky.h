// sky.h — host-side launch interface of sky.hip: the sun-and-sky generator behind pt_generate_sky.
#pragma once
#include <hip/hip_runtime.h>

#include "pt_sky.h"

namespace pt {

// Fills the P.w x P.h lat-long image `out` with sky_texel: k_sky, one lane per texel, 256-thread blocks (P.w * P.h <= 2^26).
void launch_sky(hipStream_t s, const SkyParams& P, vec4* out);

}  // namespace pt
