// bloom.hip — bloom on the device (pt_bloom.h holds the arithmetic).
//
//   k_bloom_down0      frame -> level 1 with the bright pass: 16 x 16 texels per block from a 34 x 34 source tile staged in LDS once, so
//                      the bright pass (and its division) is paid once per source pixel, not once per tap
//   k_bloom_down       level l -> level l+1, the same tiling without the bright pass
//   k_bloom_up         U_l = D_l + scatter * up(U_{l+1}), in place (a texel reads only its own D_l and the other level)
//   k_bloom_composite  the frame: the last up, the division by norm and the mix in one pass; U_1 is never expanded in memory
// All are enqueued on the renderer's stream ahead of k_postprocess.  No atomics: the result does not depend on scheduling.
//
// Compiled with -ffp-contract=off (deterministic fp32 contract, pt_math.h).
#include <hip/hip_runtime.h>

#include "bloom.h"

namespace pt {

constexpr uint32_t kTile = 16, kSrcTile = 2 * kTile + 2;   // 34: the taps of 16 texels reach one source texel past both ends

// Blocks are numbered row by row over the destination's tiles (a one-dimensional grid: a tall image has more tile rows than a grid's y
// may count).  Index clamping happens at staging, so the taps index the tile directly.
template <bool kBright>
__device__ __forceinline__ void bloom_down_block(const vec4* __restrict__ src, uint32_t sw, uint32_t sh, vec4* __restrict__ dst, uint32_t dw,
                                                 uint32_t dh, uint32_t tiles_x, float threshold, float knee) {
  __shared__ float tile[3][kSrcTile * kSrcTile];
  const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
  const int32_t ox = (int32_t)(2u * kTile * bx) - 1, oy = (int32_t)(2u * kTile * by) - 1;
  for (uint32_t e = threadIdx.x; e < kSrcTile * kSrcTile; e += kTile * kTile) {
    const uint32_t ly = e / kSrcTile, lx = e - ly * kSrcTile;
    const uint32_t sx = bloom_clamp(ox + (int32_t)lx, sw), sy = bloom_clamp(oy + (int32_t)ly, sh);
    const vec4 c = src[(size_t)sy * sw + sx];
    const vec3 v = kBright ? bloom_bright(c, threshold, knee) : v3(c.x, c.y, c.z);
    tile[0][e] = v.x; tile[1][e] = v.y; tile[2][e] = v.z;
  }
  __syncthreads();
  const uint32_t ty = threadIdx.x / kTile, tx = threadIdx.x - ty * kTile;
  const uint32_t x = bx * kTile + tx, y = by * kTile + ty;
  if (x >= dw || y >= dh) return;
  const vec3 a = bloom_down_sum([&](int i, int j) {
    const uint32_t e = (2u * ty + (uint32_t)j) * kSrcTile + 2u * tx + (uint32_t)i;
    return v3(tile[0][e], tile[1][e], tile[2][e]);
  });
  dst[(size_t)y * dw + x] = vec4{a.x, a.y, a.z, 0.0f};
}

__global__ void __launch_bounds__(256) k_bloom_down0(const vec4* __restrict__ img, uint32_t W, uint32_t H, vec4* __restrict__ dst, uint32_t dw,
                                                     uint32_t dh, uint32_t tiles_x, float threshold, float knee) {
  bloom_down_block<true>(img, W, H, dst, dw, dh, tiles_x, threshold, knee);
}

__global__ void __launch_bounds__(256) k_bloom_down(const vec4* __restrict__ src, uint32_t sw, uint32_t sh, vec4* __restrict__ dst, uint32_t dw,
                                                    uint32_t dh, uint32_t tiles_x) {
  bloom_down_block<false>(src, sw, sh, dst, dw, dh, tiles_x, 0.0f, 0.0f);
}

// one texel per lane, 16 x 16 per block
__global__ void __launch_bounds__(256) k_bloom_up(vec4* __restrict__ fine, uint32_t fw, uint32_t fh, const vec4* __restrict__ coarse, uint32_t cw,
                                                  uint32_t ch, uint32_t tiles_x, float scatter) {
  const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
  const uint32_t ty = threadIdx.x / kTile, tx = threadIdx.x - ty * kTile;
  const uint32_t x = bx * kTile + tx, y = by * kTile + ty;
  if (x >= fw || y >= fh) return;
  const vec3 up = bloom_up_texel([&](uint32_t ux, uint32_t uy) { const vec4 c = coarse[(size_t)uy * cw + ux]; return v3(c.x, c.y, c.z); }, cw, ch, x, y);
  const size_t p = (size_t)y * fw + x;
  const vec4 d = fine[p];
  const vec3 u = bloom_combine(v3(d.x, d.y, d.z), up, scatter);
  fine[p] = vec4{u.x, u.y, u.z, 0.0f};
}

__global__ void __launch_bounds__(256) k_bloom_composite(const vec4* __restrict__ img, vec4* __restrict__ out, uint32_t W, uint32_t H,
                                                         const vec4* __restrict__ u1, uint32_t cw, uint32_t ch, uint32_t tiles_x, float norm,
                                                         pt_bloom_options o) {
  const uint32_t by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
  const uint32_t ty = threadIdx.x / kTile, tx = threadIdx.x - ty * kTile;
  const uint32_t x = bx * kTile + tx, y = by * kTile + ty;
  if (x >= W || y >= H) return;
  const vec3 up = bloom_up_texel([&](uint32_t ux, uint32_t uy) { const vec4 c = u1[(size_t)uy * cw + ux]; return v3(c.x, c.y, c.z); }, cw, ch, x, y);
  const size_t p = (size_t)y * W + x;
  out[p] = bloom_composite(img[p], up, norm, o);
}

static uint32_t tiles(uint32_t n) { return (n + kTile - 1u) / kTile; }

hipError_t launch_bloom(hipStream_t s, const vec4* img, vec4* out, vec4* pyramid, const pt_bloom_plan& plan, const pt_bloom_options& o) {
  const uint32_t L = plan.levels, W = plan.width[0], H = plan.height[0];
  if (L == 0u) return hipMemcpyAsync(out, img, sizeof(vec4) * (size_t)W * H, hipMemcpyDeviceToDevice, s);
  const dim3 block(kTile * kTile);
  auto level = [&](uint32_t l) { return pyramid + plan.offset[l]; };
  hipLaunchKernelGGL(k_bloom_down0, dim3(tiles(plan.width[1]) * tiles(plan.height[1])), block, 0, s, img, W, H, level(1), plan.width[1], plan.height[1],
                     tiles(plan.width[1]), o.threshold, o.knee);
  for (uint32_t l = 1; l < L; l++)
    hipLaunchKernelGGL(k_bloom_down, dim3(tiles(plan.width[l + 1]) * tiles(plan.height[l + 1])), block, 0, s, (const vec4*)level(l), plan.width[l],
                       plan.height[l], level(l + 1), plan.width[l + 1], plan.height[l + 1], tiles(plan.width[l + 1]));
  for (uint32_t l = L; l-- > 1u;)   // U_L = D_L as the last down left it: up for l = L-1..1
    hipLaunchKernelGGL(k_bloom_up, dim3(tiles(plan.width[l]) * tiles(plan.height[l])), block, 0, s, level(l), plan.width[l], plan.height[l],
                       (const vec4*)level(l + 1), plan.width[l + 1], plan.height[l + 1], tiles(plan.width[l]), o.scatter);
  hipLaunchKernelGGL(k_bloom_composite, dim3(tiles(W) * tiles(H)), block, 0, s, img, out, W, H, (const vec4*)level(1), plan.width[1], plan.height[1],
                     tiles(W), bloom_norm(L, o.scatter), o);
  return hipGetLastError();
}

}  // namespace pt
