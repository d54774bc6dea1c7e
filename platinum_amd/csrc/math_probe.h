// math_probe.h — host-side launch interface of math_probe.hip: the kernel behind pt_debug_math (include/ptamd.h).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_device.h"

namespace pt {

// out0[i] (out1[i], out1[n + i]) = function fn of a[i] (b[i]), i < n, as pt_math_probe.h math_probe_eval defines it; b / out1 may be null
// for a function that does not touch them.  `table`: the renderer's 620 Halton entries.
void launch_math_probe(hipStream_t s, uint32_t fn, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* out0, uint32_t* out1,
                       const HaltonEntry* table);

}  // namespace pt
