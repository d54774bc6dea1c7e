// selection.h — host-side launch interface of selection.hip: the selection overlay on the RGBA8 target.
#pragma once
#include <hip/hip_runtime.h>

#include "pt_selection.h"

namespace pt {

// Draws the outline and the tint of `o` onto the W x H target (0xAABBGGRR per pixel, in place) from `coverage` (W x H floats, read only):
// one k_selection_overlay block per 16 x 16 pixels.
void launch_selection_overlay(hipStream_t s, uint32_t* target, const float* coverage, uint32_t width, uint32_t height, const pt_selection_options& o);

}  // namespace pt
