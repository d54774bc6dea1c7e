// ao.hip — the ambient-occlusion pass on the device beside its trace (pt_ao.h holds the AO ray, the fold and the resolve).
//
//   k_trace_ao (kernels.hip)     after the camera trace of a batch, before k_shade(0): one any-hit ray per camera ray -> Obuf[pid] (4 B):
//                                0 the camera ray missed, 1 occluded, 2 open
//   k_accumulate_ao              after the accumulate kernels: folds Obuf into the per-pixel counts {hits, open}
//                                (k_accumulate_ao_adaptive: the same over the active tiles of an adaptive or region render)
//   k_ao_scatter                 pt_debug_ao: Obuf of a one-sample batch -> pixel order
// Only a render started with AO enabled launches any of them (renderer.hip enqueue_batch).
#include <hip/hip_runtime.h>

#include "ao.h"
#include "pt_tilefold.h"

namespace pt {

// ---- k_accumulate_ao: one wave per 8x8 tile (pt_tilefold.h fold_tile / fold_stage) ---------------------------------------------------------
// A round stages 4-B entries of Obuf (64 * 9 * 4 B of LDS); every lane then folds the samples of its pixel into the uint2 it holds in
// registers across the batch, and stores it once.  Integer sums: the order does not matter, and there are no atomics.
template <bool ADAPTIVE>
__device__ __forceinline__ void accumulate_ao_body(uint2* __restrict__ counts, const uint32_t* __restrict__ Obuf, uint32_t width, uint32_t height,
                                                   uint32_t nsamples, const uint32_t* __restrict__ active, const uint32_t* __restrict__ active_count,
                                                   Rect rect) {
  __shared__ uint32_t stage[64 * kFoldRow];
  const uint32_t lane = wave_lane();
  const FoldTile t = fold_tile<ADAPTIVE>(blockIdx.x, lane, width, height, active, active_count, rect);
  const bool live = t.live, inside = t.inside;
  const size_t p = (size_t)t.q.y * width + t.q.x;
  uint2 c = inside ? counts[p] : uint2{0u, 0u};
  for (uint32_t s0 = 0; s0 < nsamples; s0 += 8u) {
    const uint32_t nb = nsamples - s0 < 8u ? nsamples - s0 : 8u;
    __syncthreads();
    if (live) fold_stage(t.tile, lane, s0, nb, nsamples, [&](uint32_t pid, uint32_t slot) { stage[slot] = Obuf[pid]; });
    __syncthreads();
    if (inside) {
      for (uint32_t j = 0; j < nb; j++) c = ao_fold(c, stage[lane * kFoldRow + j]);
    }
  }
  if (inside) counts[p] = c;
}

__global__ void __launch_bounds__(64) k_accumulate_ao(uint2* __restrict__ counts, const uint32_t* __restrict__ Obuf, uint32_t width, uint32_t height,
                                                       uint32_t nsamples) {
  accumulate_ao_body<false>(counts, Obuf, width, height, nsamples, nullptr, nullptr, Rect{});
}

__global__ void __launch_bounds__(64) k_accumulate_ao_adaptive(uint2* __restrict__ counts, const uint32_t* __restrict__ Obuf, uint32_t width,
                                                                uint32_t height, uint32_t nsamples, const uint32_t* __restrict__ active,
                                                                const uint32_t* __restrict__ active_count, Rect rect) {
  accumulate_ao_body<true>(counts, Obuf, width, height, nsamples, active, active_count, rect);
}

// ---- k_ao_scatter: the bounce-0 queue of a one-sample batch (pt_tilefold.h walk_bounce0) names the pids that hold a state ----
__global__ void __launch_bounds__(256) k_ao_scatter(uint32_t width, PathState st, const vec4* __restrict__ hit, Segments seg,
                                                    const uint32_t* __restrict__ Obuf, uint32_t* __restrict__ state) {
  const uint32_t lane = wave_lane();
  for (uint32_t sg = wave_index(); sg < seg.nseg; sg += wave_count())
    walk_bounce0(seg, st, hit, sg, lane, [&](uint32_t, uint32_t pid, uint32_t) { state[pixel_of_pid_1spp(pid, width)] = Obuf[pid]; });
}

void launch_accumulate_ao(hipStream_t s, uint2* counts, const uint32_t* Obuf, uint32_t width, uint32_t height, uint32_t nsamples, const TileSet* tiles) {
  // one block per tile of the image, or per tile that may still be active
  if (tiles)
    hipLaunchKernelGGL(k_accumulate_ao_adaptive, dim3(tiles->max_active), dim3(64), 0, s, counts, Obuf, width, height, nsamples, tiles->active,
                       tiles->active_count, tiles->rect);
  else
    hipLaunchKernelGGL(k_accumulate_ao, dim3(tile_count(width, height)), dim3(64), 0, s, counts, Obuf, width, height, nsamples);
}

void launch_ao_scatter(hipStream_t s, uint32_t grid, uint32_t width, PathState st, const vec4* hit, Segments seg, const uint32_t* Obuf, uint32_t* state) {
  hipLaunchKernelGGL(k_ao_scatter, dim3(grid), dim3(256), 0, s, width, st, hit, seg, Obuf, state);
}

}  // namespace pt
