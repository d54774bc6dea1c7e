// light_probe.hip — pt_debug_lights' kernel: the light-sampling part of the shading stage (pt_shade.h: shade_nee_light with sampleLightPower
// and sample_environment under it, stage_miss) evaluated elementwise on the device against a started render's scene.  A parity surface for
// the tests; no render path launches it.
#include "light_probe.h"

#include "pt_light_probe.h"

namespace pt {

constexpr uint32_t kLightProbeBlock = 256, kLightProbeMaxBlocks = 2048;

__global__ __launch_bounds__(kLightProbeBlock) void k_light_probe(const DeviceScene* __restrict__ Sp, uint32_t fn, uint32_t n, pt_light_probe_args args,
                                                                  const float* __restrict__ in, uint32_t* __restrict__ out) {
  const DeviceScene& S = *Sp;  // the table k_shade reads, through the same pointer
  __shared__ LightRec lds_lights[kLightProbeStaged];
  // the launch refuses the staged form for more lights than fit, so the copy below stays inside lds_lights
  const bool lights_in_lds = fn == PT_LIGHT_SAMPLE && args.tables == PT_LIGHT_TABLES_LDS && S.lightCount <= kLightProbeStaged;
  if (lights_in_lds) {  // k_shade's copy loop
    const uint4* ls = reinterpret_cast<const uint4*>(S.light_recs);
    uint4* ld = reinterpret_cast<uint4*>(lds_lights);
    for (uint32_t i = threadIdx.x; i < S.lightCount * (uint32_t)(sizeof(LightRec) / 16); i += kLightProbeBlock) ld[i] = ldg(&ls[i]);
  }
  __syncthreads();
  ShadeTables T = shade_tables(S);
  if (lights_in_lds) { T.lights = lds_lights; T.lights_lds = 1; }
  for (uint32_t i = blockIdx.x * kLightProbeBlock + threadIdx.x; i < n; i += gridDim.x * kLightProbeBlock) {  // n <= 2^24: 12 * i never wraps
    if (fn == PT_LIGHT_SAMPLE) {
      float a[PT_LIGHT_SAMPLE_IN_WORDS];
      uint32_t o[PT_LIGHT_SAMPLE_OUT_WORDS];
      for (uint32_t k = 0; k < PT_LIGHT_SAMPLE_IN_WORDS; k++) a[k] = in[i * PT_LIGHT_SAMPLE_IN_WORDS + k];
      light_probe_sample(S, T, args, a, o);
      for (uint32_t k = 0; k < PT_LIGHT_SAMPLE_OUT_WORDS; k++) out[i * PT_LIGHT_SAMPLE_OUT_WORDS + k] = o[k];
    } else {
      float a[PT_LIGHT_ENV_MISS_IN_WORDS];
      uint32_t o[PT_LIGHT_ENV_MISS_OUT_WORDS];
      for (uint32_t k = 0; k < PT_LIGHT_ENV_MISS_IN_WORDS; k++) a[k] = in[i * PT_LIGHT_ENV_MISS_IN_WORDS + k];
      light_probe_miss(S, args, a, o);
      for (uint32_t k = 0; k < PT_LIGHT_ENV_MISS_OUT_WORDS; k++) out[i * PT_LIGHT_ENV_MISS_OUT_WORDS + k] = o[k];
    }
  }
}

void launch_light_probe(hipStream_t s, const DeviceScene* S_device, uint32_t fn, uint32_t n, pt_light_probe_args args, const float* in, uint32_t* out) {
  const uint32_t blocks = (n + kLightProbeBlock - 1) / kLightProbeBlock;
  k_light_probe<<<blocks < kLightProbeMaxBlocks ? blocks : kLightProbeMaxBlocks, kLightProbeBlock, 0, s>>>(S_device, fn, n, args, in, out);
}

}  // namespace pt
