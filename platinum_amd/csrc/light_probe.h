// light_probe.h — host-side launch interface of light_probe.hip: the kernel behind pt_debug_lights (include/ptamd.h).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_device.h"

namespace pt {

constexpr uint32_t kLightProbeStaged = 64;  // lights a block stages for PT_LIGHT_TABLES_LDS: k_shade's kShadeLights (kernels.hip)

// out[i] = function fn of in[i], i < n, as pt_light_probe.h defines the records; S_device: the device copy of the started render's scene table
void launch_light_probe(hipStream_t s, const DeviceScene* S_device, uint32_t fn, uint32_t n, pt_light_probe_args args, const float* in, uint32_t* out);

}  // namespace pt
