// adaptive.hip — the checkpoint of tile-adaptive sampling (pt_adaptive.h holds the criterion; DESIGN.md §3b "Adaptive sampling").
//
//   k_adaptive_check  one wave per virtual tile, one lane per pixel: a tile stays active unless every pixel inside `rect` passes
//                     adaptive_pixel_converged (a __ballot, no float reduction); writes flags[virtual tile]
//   compaction        hipcub::DeviceSelect::Flagged (stable): the still active tiles -> the next list, ascending, and its count
//   count copy        the new count -> pinned host memory, so the host learns without blocking when no tile is left
// Only a batch that ends at a checkpoint launches any of it (renderer.hip enqueue_batch).
//
// Compiled with -ffp-contract=off (deterministic fp32 contract, pt_math.h).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "adaptive.h"
#include "pt_adaptive.h"
#include "pt_layout.h"

namespace pt {

// flags[v] for every v < tiles: 1 = tile list_in[v] stays active, 0 = it converged at n samples (or v is past the active count)
__global__ void __launch_bounds__(256) k_adaptive_check(const uint32_t* __restrict__ list_in, const uint32_t* __restrict__ count_in,
                                                        const vec2* __restrict__ mom, uint32_t W, Rect rect, uint32_t tiles, uint32_t n,
                                                        float threshold, uint8_t* __restrict__ flags) {
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const uint32_t v = blockIdx.x * 4u + (threadIdx.x >> 6);   // wave-uniform
  if (v >= tiles) return;
  if (v >= *count_in) {
    if (lane == 0) flags[v] = 0;
    return;
  }
  const PixelXY q = tile_pixel(list_in[v], lane, tiles_x(W));
  const uint32_t x = q.x, y = q.y;
  bool converged = true;   // pixels outside the rectangle (the whole frame, or the render region) take no part
  if (rect_contains(rect, x, y)) {
    const vec2 m = mom[(size_t)y * W + x];
    converged = adaptive_pixel_converged(m.x, m.y, n, threshold);
  }
  const unsigned long long open = __ballot(!converged);
  if (lane == 0) flags[v] = open != 0ull ? 1 : 0;
}

size_t adaptive_scratch_bytes(uint32_t tiles) {
  size_t bytes = 0;
  (void)hipcub::DeviceSelect::Flagged(nullptr, bytes, (const uint32_t*)nullptr, (const uint8_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                      (int)tiles, (hipStream_t)0);
  return bytes;
}

hipError_t launch_adaptive_check(hipStream_t s, const uint32_t* list_in, const uint32_t* count_in, uint32_t* list_out, uint32_t* count_out,
                                 const vec2* mom, uint32_t W, const Rect& rect, uint32_t tiles, uint32_t n, float threshold, uint8_t* flags,
                                 void* scratch, size_t scratch_bytes, uint32_t* host_count) {
  hipLaunchKernelGGL(k_adaptive_check, dim3((tiles + 3u) / 4u), dim3(256), 0, s, list_in, count_in, mom, W, rect, tiles, n, threshold, flags);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = hipcub::DeviceSelect::Flagged(scratch, scratch_bytes, list_in, flags, list_out, count_out, (int)tiles, s);
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(host_count, count_out, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
}

}  // namespace pt
