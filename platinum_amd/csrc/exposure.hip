// exposure.hip — auto exposure on the device (pt_exposure.h holds the arithmetic).
//
//   k_exposure_histogram  the rectangle's pixels -> 259 counters: per block in LDS, then one global integer atomic per non-zero counter
//   k_exposure_resolve    one wave; lane 0 turns the counters into the mean, the ev and the gain, and advances the smoothing state
//   k_exposure_apply      frame * gain -> the renderer's scratch image, which k_postprocess then reads
// All three are enqueued on the renderer's stream ahead of k_postprocess; the gain travels through device memory, never through the host.
// Only integer atomics are used, so the counters do not depend on the order pixels arrive in.
//
// Compiled with -ffp-contract=off (deterministic fp32 contract, pt_math.h).
#include <hip/hip_runtime.h>

#include "exposure.h"

namespace pt {

// One pixel per lane and step: a pixel is one 16-byte load.  The rectangle's pixels are numbered row by row, so a region costs its area and
// a wave reads whole row segments.  A converged flat wall puts all 64 lanes of a wave into one bin: lanes that share a key are counted with
// a ballot and added once by their first lane, for up to kPeel distinct keys per wave and step; what is left after that (a noisy wave) adds
// lane by lane.
__global__ void __launch_bounds__(256) k_exposure_histogram(const vec4* __restrict__ img, uint32_t pitch, Rect rect, uint32_t* __restrict__ counters) {
  constexpr int kPeel = 4;
  __shared__ uint32_t h[kExpCounters];
  for (uint32_t c = threadIdx.x; c < kExpCounters; c += 256u) h[c] = 0u;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rw = rect.x1 - rect.x0, n = rw * (rect.y1 - rect.y0);
  for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {   // uniform over the block: every lane reaches the ballots
    const uint32_t i = base + threadIdx.x;
    const bool valid = i < n;
    uint32_t key = 0u;
    if (valid) {
      const uint32_t y = i / rw, x = i - y * rw;
      key = exposure_pixel_key(img[(size_t)(rect.y0 + y) * pitch + (rect.x0 + x)]);
    }
    unsigned long long rem = __ballot(valid);
    for (int round = 0; round < kPeel && rem != 0ull; round++) {
      const uint32_t first = (uint32_t)__ffsll((long long)rem) - 1u;
      const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)first);
      const unsigned long long same = __ballot(valid && key == k) & rem;
      if (lane == first) atomicAdd(&h[k], (uint32_t)__popcll(same));
      rem &= ~same;
    }
    if ((rem >> lane) & 1ull) atomicAdd(&h[key], 1u);
  }
  __syncthreads();
  for (uint32_t c = threadIdx.x; c < kExpCounters; c += 256u) {
    const uint32_t v = h[c];
    if (v) atomicAdd(&counters[c], v);
  }
}

// The wave stages the counters in LDS (a lane reading 2 x 256 words of global memory one after the other would cost more than the histogram);
// lane 0 runs the serial resolve on that copy and writes the rest of the record.
__global__ void __launch_bounds__(64) k_exposure_resolve(ExposureRecord* __restrict__ rec, pt_exposure_options o, uint32_t for_target) {
  __shared__ pt_exposure_meter m;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&rec->meter);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&m);
  for (uint32_t c = threadIdx.x; c < kExpCounters; c += 64u) dst[c] = src[c];
  __syncthreads();
  if (threadIdx.x != 0u) return;
  exposure_resolve(&m, o, rec->prev_ev, rec->has_prev);
  rec->meter.metered = m.metered; rec->meter.kept = m.kept; rec->meter._pad = 0u; rec->meter.weighted = m.weighted;
  rec->meter.mean_log2 = m.mean_log2; rec->meter.target_ev = m.target_ev; rec->meter.ev = m.ev; rec->meter.gain = m.gain;
  if (for_target) { rec->prev_ev = m.ev; rec->has_prev = 1u; }
}

__global__ void __launch_bounds__(256) k_exposure_apply(const vec4* __restrict__ img, vec4* __restrict__ out, uint32_t npix,
                                                        const ExposureRecord* __restrict__ rec) {
  const float gain = rec->meter.gain;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < npix; i += gridDim.x * 256u) out[i] = exposure_apply(img[i], gain);
}

// enough blocks to fill the chip (256 CUs x 8 blocks), grid-stride beyond that
static uint32_t exposure_grid(uint32_t n) {
  const uint32_t blocks = (n + 255u) / 256u;
  return blocks < 2048u ? (blocks ? blocks : 1u) : 2048u;
}

hipError_t launch_exposure_meter(hipStream_t s, const vec4* img, uint32_t W, const Rect& rect, const pt_exposure_options& o, ExposureRecord* rec,
                                 bool for_target) {
  const hipError_t e = hipMemsetAsync(rec, 0, sizeof(uint32_t) * kExpCounters, s);
  if (e != hipSuccess) return e;
  const uint32_t n = (rect.x1 - rect.x0) * (rect.y1 - rect.y0);
  hipLaunchKernelGGL(k_exposure_histogram, dim3(exposure_grid(n)), dim3(256), 0, s, img, W, rect, reinterpret_cast<uint32_t*>(rec));
  hipLaunchKernelGGL(k_exposure_resolve, dim3(1), dim3(64), 0, s, rec, o, for_target ? 1u : 0u);
  return hipGetLastError();
}

void launch_exposure_apply(hipStream_t s, const vec4* img, vec4* out, uint32_t npix, const ExposureRecord* rec) {
  hipLaunchKernelGGL(k_exposure_apply, dim3(exposure_grid(npix)), dim3(256), 0, s, img, out, npix, rec);
}

}  // namespace pt
