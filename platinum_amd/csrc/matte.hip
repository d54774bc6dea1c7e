// matte.hip — ID mattes on the device (pt_matte.h holds the fold and the resolve arithmetic).
//
//   k_matte_ids                  after the camera trace of a batch, before k_shade(0): per camera ray, {instance, material} -> Mbuf[pid] (8 B)
//   k_accumulate_matte           after the accumulate kernels: folds Mbuf into both layers' slots, per pixel in sample order
//                                (k_accumulate_matte_adaptive: the same over the active tiles of an adaptive or region render)
//   k_matte_resolve              a read: the slots of one layer against a sorted id set -> coverage per pixel
//   k_matte_clear                every slot := {kMatteNone, 0}
// Only a render started with mattes enabled launches any of them (renderer.hip enqueue_batch).
//
// Compiled with -ffp-contract=off (deterministic fp32 contract, pt_math.h).
#include <hip/hip_runtime.h>

#include "matte.h"
#include "pt_tilefold.h"

namespace pt {

namespace {

// a pixel's slots of one layer <-> its four uint4 {id, count, id, count} of the slot image
__device__ __forceinline__ void load_slots(const uint4* __restrict__ px, MatteSlots& m) {
#pragma unroll
  for (uint32_t q = 0; q < kMatteSlots / 2u; q++) {
    const uint4 v = px[q];
    m.id[2u * q] = v.x; m.count[2u * q] = v.y; m.id[2u * q + 1u] = v.z; m.count[2u * q + 1u] = v.w;
  }
}
__device__ __forceinline__ void store_slots(uint4* __restrict__ px, const MatteSlots& m) {
#pragma unroll
  for (uint32_t q = 0; q < kMatteSlots / 2u; q++) px[q] = uint4{m.id[2u * q], m.count[2u * q], m.id[2u * q + 1u], m.count[2u * q + 1u]};
}

}  // namespace

__global__ void __launch_bounds__(256) k_matte_clear(uint4* __restrict__ slots, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) slots[i] = uint4{kMatteNone, 0u, kMatteNone, 0u};
}

// ---- k_matte_ids: the bounce-0 queue (pt_tilefold.h walk_bounce0) -> Mbuf.  Reads the queue only: word 3 of the hit record and of rayD. ----
__global__ void __launch_bounds__(256) k_matte_ids(const DeviceScene* __restrict__ Sp, PathState st, const vec4* __restrict__ hit, Segments seg,
                                                   MatteIds* __restrict__ Mbuf) {
  const ShadeRec* __restrict__ recs = Sp->shade_recs;
  const uint32_t lane = wave_lane(), wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t sg = wave; sg < seg.nseg; sg += nwaves)
    walk_bounce0(seg, st, hit, sg, lane, [&](uint32_t, uint32_t pid, uint32_t hw) {
      MatteIds m{kMatteNone, kMatteNone};
      if (!hit_word_miss(hw)) {
        const uint32_t tri = hit_word_tri(hw);
        m.inst = ldg(&recs[tri].inst);
        m.material = ldg(&recs[tri].material);
      }
      Mbuf[pid] = m;
    });
}

// ---- k_accumulate_matte: one wave per 8x8 tile (pt_tilefold.h fold_tile / fold_stage) ------------------------------------------------------
// A round stages 8-B entries of Mbuf (4.6 KB of LDS); every lane then folds the samples of its pixel in sample order into the 16 slots it
// holds in registers across the batch, and stores them once.  ADAPTIVE: k_accumulate_matte_adaptive.
template <bool ADAPTIVE>
__device__ __forceinline__ void accumulate_matte_body(uint4* __restrict__ slots, const MatteIds* __restrict__ Mbuf, uint32_t width, uint32_t height,
                                                      uint32_t nsamples, const uint32_t* __restrict__ active,
                                                      const uint32_t* __restrict__ active_count, Rect rect) {
  __shared__ MatteIds stage[64 * kFoldRow];
  const uint32_t lane = wave_lane();
  const FoldTile t = fold_tile<ADAPTIVE>(blockIdx.x, lane, width, height, active, active_count, rect);
  const bool live = t.live, inside = t.inside;
  uint4* __restrict__ px = slots + ((size_t)t.q.y * width + t.q.x) * kMattePixelVec4;
  MatteSlots I, M;
  matte_clear(I); matte_clear(M);
  if (inside) { load_slots(px, I); load_slots(px + kMatteSlots / 2u, M); }
  for (uint32_t s0 = 0; s0 < nsamples; s0 += 8u) {
    const uint32_t nb = nsamples - s0 < 8u ? nsamples - s0 : 8u;
    __syncthreads();
    // (four loads in flight per lane: all eight cost 8 more VGPRs than the 64 of 8 waves per SIMD)
    if (live) fold_stage<4>(t.tile, lane, s0, nb, nsamples, [&](uint32_t pid, uint32_t slot) { stage[slot] = Mbuf[pid]; });
    __syncthreads();
    if (inside) {
      for (uint32_t j = 0; j < nb; j++) {
        const MatteIds m = stage[lane * kFoldRow + j];
        matte_fold(I, m.inst);
        matte_fold(M, m.material);
      }
    }
  }
  if (inside) { store_slots(px, I); store_slots(px + kMatteSlots / 2u, M); }
}

__global__ void __launch_bounds__(64) k_accumulate_matte(uint4* __restrict__ slots, const MatteIds* __restrict__ Mbuf, uint32_t width,
                                                          uint32_t height, uint32_t nsamples) {
  accumulate_matte_body<false>(slots, Mbuf, width, height, nsamples, nullptr, nullptr, Rect{});
}

__global__ void __launch_bounds__(64) k_accumulate_matte_adaptive(uint4* __restrict__ slots, const MatteIds* __restrict__ Mbuf, uint32_t width,
                                                                   uint32_t height, uint32_t nsamples, const uint32_t* __restrict__ active,
                                                                   const uint32_t* __restrict__ active_count, Rect rect) {
  accumulate_matte_body<true>(slots, Mbuf, width, height, nsamples, active, active_count, rect);
}

// ---- k_matte_resolve: one lane per pixel; a lane binary-searches its 8 slot ids in the caller's sorted id set ---------------------------------
__global__ void __launch_bounds__(256) k_matte_resolve(const uint4* __restrict__ slots, uint32_t layer, const uint32_t* __restrict__ ids,
                                                       uint32_t id_count, const uint32_t* __restrict__ tile_n, uint32_t n_uniform, Rect rect,
                                                       uint32_t width, uint32_t height, float* __restrict__ coverage_out) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= width * height) return;
  const uint32_t y = p / width, x = p - y * width;
  const uint32_t n = tile_n ? (rect_contains(rect, x, y) ? tile_n[tile_of_pixel(x, y, width)] : 0u) : n_uniform;
  MatteSlots m;
  load_slots(slots + (size_t)p * kMattePixelVec4 + layer * (kMatteSlots / 2u), m);
  coverage_out[p] = matte_coverage(m, ids, id_count, n);
}

void launch_matte_clear(hipStream_t s, uint4* slots, size_t npix) {
  const size_t n = npix * kMattePixelVec4;
  if (n) hipLaunchKernelGGL(k_matte_clear, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, s, slots, n);
}

void launch_matte_ids(hipStream_t s, uint32_t grid, const DeviceScene* S_device, PathState st, const vec4* hit, Segments seg, MatteIds* Mbuf) {
  hipLaunchKernelGGL(k_matte_ids, dim3(grid), dim3(256), 0, s, S_device, st, hit, seg, Mbuf);
}

void launch_accumulate_matte(hipStream_t s, uint4* slots, const MatteIds* Mbuf, uint32_t width, uint32_t height, uint32_t nsamples,
                             const TileSet* tiles) {
  // one block per tile of the image, or per tile that may still be active
  if (tiles)
    hipLaunchKernelGGL(k_accumulate_matte_adaptive, dim3(tiles->max_active), dim3(64), 0, s, slots, Mbuf, width, height, nsamples, tiles->active,
                       tiles->active_count, tiles->rect);
  else
    hipLaunchKernelGGL(k_accumulate_matte, dim3(tile_count(width, height)), dim3(64), 0, s, slots, Mbuf, width, height, nsamples);
}

void launch_matte_resolve(hipStream_t s, const uint4* slots, uint32_t layer, const uint32_t* ids, uint32_t id_count, const uint32_t* tile_n,
                          uint32_t n_uniform, const Rect& rect, uint32_t width, uint32_t height, float* coverage_out) {
  const uint32_t npix = width * height;
  hipLaunchKernelGGL(k_matte_resolve, dim3((npix + 255u) / 256u), dim3(256), 0, s, slots, layer, ids, id_count, tile_n, n_uniform, rect, width, height,
                     coverage_out);
}

}  // namespace pt
