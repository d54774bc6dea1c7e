// shade_probe.h — host-side launch interface of shade_probe.hip: the kernels behind pt_debug_shading (include/ptamd.h).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_device.h"

namespace pt {

// ids[2 t], ids[2 t + 1] = (instance, primitive) of triangle t, t < 2 * slot_count (pt_shade_probe.h shade_probe_ids)
void launch_shade_probe_ids(hipStream_t s, const DeviceScene* S_device, uint32_t n_tri, int32_t* ids);
// out[i] = the probe's record of in[i], i < n, as pt_shade_probe.h defines the records (every in[i] resolved: its triangle word is filled);
// S_device: the device copy of the started render's scene table
void launch_shade_probe(hipStream_t s, const DeviceScene* S_device, uint32_t n, const uint32_t* in, uint32_t* out);

}  // namespace pt
