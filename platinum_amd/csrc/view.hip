// view.hip — the data views of the render target on the device (pt_view.h holds the arithmetic).
//
//   k_view_range   DEPTH with auto_range, ahead of k_view_pass on the same stream: the rectangle's pixels, row by row and grid-strided, -> the
//                  min and max of the valid depths and their number.  Each lane folds its pixels in registers, a wave reduces with shuffles,
//                  the block's four waves meet in 48 B of LDS, and one lane issues the block's integer atomics: a max for a bound only
//                  where it would move the record (every block's atomics land on one 16-byte record and are served one after the other;
//                  a max that cannot move it is a no-op, so leaving it out is exact), and the count's add only where the count is read.
//                  The depths are non-negative floats, whose bits order as integers: the result does not depend on the order of arrival.
//   k_view_pass    in place of source, exposure, bloom, k_postprocess and the film's alpha byte: one lane per pixel reads what its view needs
//                  with 16-byte loads and writes the pixel's four bytes.  A streaming kernel: no LDS, no atomics.
//
// Compiled with -ffp-contract=off (deterministic fp32 contract, pt_math.h).
#include <hip/hip_runtime.h>

#include "view.h"

namespace pt {

namespace {

__device__ __forceinline__ uint32_t view_count(const ViewImages& I, uint32_t p, uint32_t x, uint32_t y) {
  if (I.counts) return I.counts[p];
  if (I.tile_n) return rect_contains(I.rect, x, y) ? I.tile_n[tile_of_pixel(x, y, I.width)] : 0u;
  return I.n_uniform;
}

// what view_pixel fetches of pixel p
struct DevicePx {
  const ViewImages& I;
  uint32_t p;
  __device__ __forceinline__ vec4 normal() const { return I.normal[p]; }
  __device__ __forceinline__ vec3 moments() const {
    if (I.moments) { const vec4 m = I.moments[p]; return vec3{m.x, m.y, m.z}; }
    const vec2 m = I.mom2[p];
    return vec3{0.0f, m.x, m.y};
  }
  __device__ __forceinline__ float alpha() const { const vec4 f = I.film[p]; return f.w; }
  __device__ __forceinline__ void slots(MatteSlots& m) const {
    const uint4* __restrict__ px = I.slots + (size_t)p * I.slot_stride;
#pragma unroll
    for (uint32_t q = 0; q < kMatteSlots / 2u; q++) {
      const uint4 v = px[q];
      m.id[2u * q] = v.x; m.count[2u * q] = v.y; m.id[2u * q + 1u] = v.z; m.count[2u * q + 1u] = v.w;
    }
  }
};

}  // namespace

__global__ void __launch_bounds__(256) k_view_range(ViewImages I, ViewRecord* __restrict__ rec, uint32_t with_count) {
  __shared__ uint32_t part[3 * 4];
  ViewRecord mine{0u, 0u, 0u, 0u};
  const uint32_t rw = I.rect.x1 - I.rect.x0, n = rw * (I.rect.y1 - I.rect.y0);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const uint32_t ry = i / rw, x = I.rect.x0 + (i - ry * rw), y = I.rect.y0 + ry;
    const uint32_t p = y * I.width + x;
    const uint32_t cnt = view_count(I, p, x, y);
    float d;
    if (cnt != 0u && view_depth(I.moments[p].x, I.normal[p].w, cnt, &d)) view_range_fold(mine, view_depth_key(d));
  }
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t a = __shfl_xor(mine.inv_min, off, 64), b = __shfl_xor(mine.max, off, 64), c = __shfl_xor(mine.count, off, 64);
    mine.inv_min = a > mine.inv_min ? a : mine.inv_min;
    mine.max = b > mine.max ? b : mine.max;
    mine.count += c;
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) { part[3u * wave] = mine.inv_min; part[3u * wave + 1u] = mine.max; part[3u * wave + 2u] = mine.count; }
  __syncthreads();
  if (threadIdx.x != 0u) return;
  for (uint32_t w = 1; w < 4u; w++) {
    mine.inv_min = part[3u * w] > mine.inv_min ? part[3u * w] : mine.inv_min;
    mine.max = part[3u * w + 1u] > mine.max ? part[3u * w + 1u] : mine.max;
    mine.count += part[3u * w + 2u];
  }
  if (mine.count == 0u) return;   // (nothing valid in this block: the record keeps its bits)
  if (mine.inv_min > __hip_atomic_load(&rec->inv_min, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&rec->inv_min, mine.inv_min);
  if (mine.max > __hip_atomic_load(&rec->max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&rec->max, mine.max);
  if (with_count) atomicAdd(&rec->count, mine.count);
}

__global__ void __launch_bounds__(256) k_view_pass(ViewImages I, ViewParams P, const ViewRecord* __restrict__ rec, uint32_t* __restrict__ target) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= I.width * I.height) return;
  const uint32_t y = p / I.width, x = p - y * I.width;
  float z0 = 0.0f, z1 = 0.0f;
  if (P.view == PT_VIEW_DEPTH) view_range(P, P.auto_range ? *rec : ViewRecord{0u, 0u, 0u, 0u}, &z0, &z1);
  target[p] = view_pixel(P, z0, z1, view_count(I, p, x, y), DevicePx{I, p});
}

// enough blocks to fill the chip (256 CUs x 8 blocks), grid-stride beyond that
hipError_t launch_view_range(hipStream_t s, const ViewImages& I, ViewRecord* rec, bool count) {
  const hipError_t e = hipMemsetAsync(rec, 0, sizeof(ViewRecord), s);
  if (e != hipSuccess) return e;
  const uint32_t n = (I.rect.x1 - I.rect.x0) * (I.rect.y1 - I.rect.y0), blocks = (n + 255u) / 256u;
  hipLaunchKernelGGL(k_view_range, dim3(blocks < 2048u ? (blocks ? blocks : 1u) : 2048u), dim3(256), 0, s, I, rec, count ? 1u : 0u);
  return hipGetLastError();
}

void launch_view_pass(hipStream_t s, const ViewImages& I, const ViewParams& P, const ViewRecord* rec, uint32_t* target) {
  const uint32_t npix = I.width * I.height;
  hipLaunchKernelGGL(k_view_pass, dim3((npix + 255u) / 256u), dim3(256), 0, s, I, P, rec, target);
}

}  // namespace pt
