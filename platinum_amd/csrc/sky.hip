// sky.hip — the sun-and-sky generator on the device (pt_sky.h holds the arithmetic).
//
//   k_sky   one lane per texel of the lat-long map, 256-thread blocks numbered row-major over the texels.  Every lane runs the same
//           32 x 8 steps: the ground and blocked cases are selects, so a wave diverges only at the disc's coverage, which a wave-uniform
//           distance test skips everywhere but beside the sun.  ALU-bound (about 700 exponentials per texel against one 16-byte store): no
//           LDS, no atomics, nothing read but the parameters.
//
// Compiled with -ffp-contract=off (deterministic fp32 contract, pt_math.h).
#include <hip/hip_runtime.h>

#include "sky.h"

namespace pt {

constexpr uint32_t kSkyBlock = 256;

__global__ void __launch_bounds__(kSkyBlock) k_sky(SkyParams P, vec4* __restrict__ out) {
  const uint32_t i = blockIdx.x * kSkyBlock + threadIdx.x;   // < 2^26 + 256: never wraps
  if (i >= P.w * P.h) return;
  const uint32_t y = i / P.w, x = i - y * P.w;
  out[i] = sky_texel(P, x, y);
}

void launch_sky(hipStream_t s, const SkyParams& P, vec4* out) {
  const uint32_t n = P.w * P.h;
  hipLaunchKernelGGL(k_sky, dim3((n + kSkyBlock - 1u) / kSkyBlock), dim3(kSkyBlock), 0, s, P, out);
}

}  // namespace pt
