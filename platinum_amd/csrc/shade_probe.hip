// shade_probe.hip — pt_debug_shading's kernels: the stage between a hit record and the BSDF (pt_shade.h shade_geometry over pt_bsdf.h
// make_shading_context and tex_sample) evaluated elementwise on the device against a started render's scene.  A parity surface for the
// tests; no render path launches it.
#include "shade_probe.h"

#include "pt_shade_probe.h"

namespace pt {

constexpr uint32_t kShadeProbeBlock = 256, kShadeProbeMaxBlocks = 2048;

__global__ __launch_bounds__(kShadeProbeBlock) void k_shade_probe_ids(const DeviceScene* __restrict__ Sp, uint32_t n_tri, int32_t* __restrict__ ids) {
  const DeviceScene& S = *Sp;
  for (uint32_t t = blockIdx.x * kShadeProbeBlock + threadIdx.x; t < n_tri; t += gridDim.x * kShadeProbeBlock) shade_probe_ids(S, t, &ids[2 * (size_t)t]);
}

__global__ __launch_bounds__(kShadeProbeBlock) void k_shade_probe(const DeviceScene* __restrict__ Sp, uint32_t n, const uint32_t* __restrict__ in,
                                                                  uint32_t* __restrict__ out) {
  const DeviceScene& S = *Sp;  // the table k_shade reads, through the same pointer
  for (uint32_t i = blockIdx.x * kShadeProbeBlock + threadIdx.x; i < n; i += gridDim.x * kShadeProbeBlock) {  // n <= 2^24: 32 * i never wraps
    uint32_t a[PT_SHADE_PROBE_IN_WORDS], o[PT_SHADE_PROBE_OUT_WORDS];
    for (uint32_t k = 0; k < PT_SHADE_PROBE_IN_WORDS; k++) a[k] = in[i * PT_SHADE_PROBE_IN_WORDS + k];
    shade_probe_element(S, a, o);
    for (uint32_t k = 0; k < PT_SHADE_PROBE_OUT_WORDS; k++) out[i * PT_SHADE_PROBE_OUT_WORDS + k] = o[k];
  }
}

static uint32_t shade_probe_blocks(uint32_t n) {
  const uint32_t blocks = (n + kShadeProbeBlock - 1) / kShadeProbeBlock;
  return blocks < kShadeProbeMaxBlocks ? blocks : kShadeProbeMaxBlocks;
}

void launch_shade_probe_ids(hipStream_t s, const DeviceScene* S_device, uint32_t n_tri, int32_t* ids) {
  k_shade_probe_ids<<<shade_probe_blocks(n_tri), kShadeProbeBlock, 0, s>>>(S_device, n_tri, ids);
}

void launch_shade_probe(hipStream_t s, const DeviceScene* S_device, uint32_t n, const uint32_t* in, uint32_t* out) {
  k_shade_probe<<<shade_probe_blocks(n), kShadeProbeBlock, 0, s>>>(S_device, n, in, out);
}

}  // namespace pt
