// selection.hip — the selection overlay on the device (pt_selection.h holds the arithmetic and the tile map).
//
//   k_selection_overlay          after k_postprocess, on the RGBA8 target in place: one block per 16 x 16 pixels stages its pixels' coverage and
//                                a halo of R into LDS (0 outside the image) beside the (2R + 1)^2 tap weights, votes, and every lane then runs the
//                                tap loop from LDS and does one read-modify-write of its pixel's four bytes
// Two block votes, both exact shortcuts of the definition: a tile that is 0 everywhere leaves m = D = 0 at each of the block's pixels, so the
// block returns without touching the target (most blocks of most frames); a tile that is 1 everywhere gives D = m = 1 (every product is
// 1 * k <= 1 and the centre's is 1), so the block skips the tap loop and tints only.
// No atomics, no scratch; 13 572 B of LDS (48^2 + 33^2 floats, the tile and the table at R = 16).
//
// Compiled with -ffp-contract=off (deterministic fp32 contract, pt_math.h).
#include <hip/hip_runtime.h>

#include "selection.h"

namespace pt {

__global__ void __launch_bounds__(256) k_selection_overlay(uint32_t* __restrict__ target, const float* __restrict__ coverage, uint32_t width,
                                                           uint32_t height, uint32_t blocks_x, SelParams P) {
  __shared__ float tile[kSelTileMax * kSelTileMax];
  __shared__ float weights[kSelTapsMax * kSelTapsMax];
  const uint32_t by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
  const int32_t R = P.R;
  const uint32_t T = sel_tile_side(R), taps = 2u * (uint32_t)R + 1u;
  bool some = false, ones = true;
  for (uint32_t t = threadIdx.x; t < T * T; t += 256u) {
    uint32_t x, y;
    const float v = sel_tile_pixel(bx, by, R, t, width, height, &x, &y) ? coverage[(size_t)y * width + x] : 0.0f;
    tile[t] = v;
    some = some || v != 0.0f;
    ones = ones && v == 1.0f;
  }
  for (uint32_t i = threadIdx.x; i < taps * taps; i += 256u) {
    const uint32_t j = i / taps;
    weights[i] = sel_weight(P.lim, (int32_t)(i - j * taps) - R, (int32_t)j - R);
  }
  if (__syncthreads_or(some) == 0) return;
  const bool full = __syncthreads_and(ones) != 0;
  const uint32_t lx = threadIdx.x & (kSelBlock - 1u), ly = threadIdx.x / kSelBlock;
  const uint32_t x = bx * kSelBlock + lx, y = by * kSelBlock + ly;
  if (x >= width || y >= height) return;
  const float* __restrict__ centre = tile + sel_tile_texel(R, lx, ly, 0, 0);
  const float* __restrict__ wc = weights + (uint32_t)R * taps + (uint32_t)R;
  const float m = centre[0];
  const float D = full ? m
                       : sel_dilate(R, [&](int32_t dx, int32_t dy) { return centre[dy * (int32_t)T + dx]; },
                                    [&](int32_t dx, int32_t dy) { return wc[dy * (int32_t)taps + dx]; });
  uint32_t* px = target + (size_t)y * width + x;
  const uint32_t before = *px, after = sel_composite(before, m, D, P);
  if (after != before) *px = after;
}

void launch_selection_overlay(hipStream_t s, uint32_t* target, const float* coverage, uint32_t width, uint32_t height, const pt_selection_options& o) {
  const uint32_t blocks_x = (width + kSelBlock - 1u) / kSelBlock, blocks_y = (height + kSelBlock - 1u) / kSelBlock;
  hipLaunchKernelGGL(k_selection_overlay, dim3(blocks_x * blocks_y), dim3(256), 0, s, target, coverage, width, height, blocks_x, sel_params(o));
}

}  // namespace pt
