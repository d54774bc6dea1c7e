// math_probe.hip — pt_debug_math's kernel: the math layer (pt_math.h, pt_sampler.h, the guards of pt_post.h and pt_denoise.h) evaluated
// elementwise on the device, outside any render.  A parity surface for the tests; no render path launches it.
#include "math_probe.h"

#include "pt_math_probe.h"

namespace pt {

constexpr uint32_t kProbeBlock = 256, kProbeMaxBlocks = 2048;

__global__ __launch_bounds__(kProbeBlock) void k_math_probe(uint32_t fn, uint32_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                            uint32_t* __restrict__ out0, uint32_t* __restrict__ out1, const HaltonEntry* __restrict__ table) {
  const bool reads_b = math_probe_reads_b(fn), writes_1 = math_probe_writes_out1(fn);
  for (uint32_t i = blockIdx.x * kProbeBlock + threadIdx.x; i < n; i += gridDim.x * kProbeBlock) {  // n <= 2^24: i never wraps
    uint32_t o[3];
    math_probe_eval(fn, a[i], reads_b ? b[i] : 0u, table, o);
    out0[i] = o[0];
    if (writes_1) out1[i] = o[1];
    if (fn == PT_MATH_SAMPLE_COSINE_HEMISPHERE) out1[n + i] = o[2];
  }
}

void launch_math_probe(hipStream_t s, uint32_t fn, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* out0, uint32_t* out1,
                       const HaltonEntry* table) {
  const uint32_t blocks = (n + kProbeBlock - 1) / kProbeBlock;
  k_math_probe<<<blocks < kProbeMaxBlocks ? blocks : kProbeMaxBlocks, kProbeBlock, 0, s>>>(fn, n, a, b, out0, out1, table);
}

}  // namespace pt
