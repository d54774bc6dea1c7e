// film.hip — the transparent film on the device (pt_film.h holds the fold and the compose arithmetic).
//
//   k_film_flags                 after the camera trace of a batch, before k_shade(0): per camera ray, hit ? 1 : 0 -> Fbuf[pid] (4 B)
//   k_accumulate_film            after the accumulate kernels: folds Lbuf masked by Fbuf into the film, per pixel in sample order
//                                (k_accumulate_film_adaptive: the same over the active tiles of an adaptive or region render)
//   k_film_compose               a target read under a backdrop: the film (or its denoised image) over the backdrop -> the chain's source
//   k_film_alpha                 transparent mode, after k_postprocess: the target's alpha byte
// Only a render started with the film enabled launches any of them (renderer.hip enqueue_batch, display.hip display_source).
//
// Compiled with -ffp-contract=off (deterministic fp32 contract, pt_math.h).
#include <hip/hip_runtime.h>

#include "film.h"
#include "pt_tilefold.h"

namespace pt {

// ---- k_film_flags: the bounce-0 queue (pt_tilefold.h walk_bounce0) -> Fbuf.  Reads the queue only: word 3 of the hit record and of rayD. ----
__global__ void __launch_bounds__(256) k_film_flags(PathState st, const vec4* __restrict__ hit, Segments seg, uint32_t* __restrict__ Fbuf) {
  const uint32_t lane = wave_lane(), wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t sg = wave; sg < seg.nseg; sg += nwaves)
    walk_bounce0(seg, st, hit, sg, lane, [&](uint32_t, uint32_t pid, uint32_t hw) { Fbuf[pid] = hit_word_miss(hw) ? 0u : 1u; });
}

// ---- k_accumulate_film: one wave per 8x8 tile (pt_tilefold.h fold_tile / fold_stage) -------------------------------------------------------
// A round stages 16-B entries of Lbuf and 4-B entries of Fbuf (11.5 KB of LDS); every lane then folds the samples of its pixel in sample
// order into the vec4 it holds in registers across the batch, and stores it once.  No atomics: k_accumulate has counted the non-finite
// samples.  ADAPTIVE: k_accumulate_film_adaptive.
template <bool ADAPTIVE>
__device__ __forceinline__ void accumulate_film_body(vec4* __restrict__ film, const vec4* __restrict__ Lbuf, const uint32_t* __restrict__ Fbuf,
                                                     uint32_t width, uint32_t height, uint32_t nsamples, uint32_t n0, uint32_t nonfinite_policy,
                                                     const uint32_t* __restrict__ active, const uint32_t* __restrict__ active_count, Rect rect) {
  __shared__ vec4 stageL[64 * kFoldRow];
  __shared__ uint32_t stageF[64 * kFoldRow];
  const uint32_t lane = wave_lane();
  const FoldTile t = fold_tile<ADAPTIVE>(blockIdx.x, lane, width, height, active, active_count, rect);
  const bool live = t.live, inside = t.inside;
  const size_t p = (size_t)t.q.y * width + t.q.x;
  vec4 f = inside ? film[p] : vec4{0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t s0 = 0; s0 < nsamples; s0 += 8u) {
    const uint32_t nb = nsamples - s0 < 8u ? nsamples - s0 : 8u;
    __syncthreads();
    if (live)
      fold_stage(t.tile, lane, s0, nb, nsamples, [&](uint32_t pid, uint32_t slot) {
        stageL[slot] = Lbuf[pid];
        stageF[slot] = Fbuf[pid];
      });
    __syncthreads();
    if (inside) {
      for (uint32_t j = 0; j < nb; j++)
        f = film_fold(f, film_sample(stageL[lane * kFoldRow + j], stageF[lane * kFoldRow + j], nonfinite_policy), n0 + s0 + j);
    }
  }
  if (inside) film[p] = f;
}

__global__ void __launch_bounds__(64) k_accumulate_film(vec4* __restrict__ film, const vec4* __restrict__ Lbuf, const uint32_t* __restrict__ Fbuf,
                                                         uint32_t width, uint32_t height, uint32_t nsamples, uint32_t n0, uint32_t nonfinite_policy) {
  accumulate_film_body<false>(film, Lbuf, Fbuf, width, height, nsamples, n0, nonfinite_policy, nullptr, nullptr, Rect{});
}

__global__ void __launch_bounds__(64) k_accumulate_film_adaptive(vec4* __restrict__ film, const vec4* __restrict__ Lbuf,
                                                                  const uint32_t* __restrict__ Fbuf, uint32_t width, uint32_t height,
                                                                  uint32_t nsamples, uint32_t n0, uint32_t nonfinite_policy,
                                                                  const uint32_t* __restrict__ active, const uint32_t* __restrict__ active_count,
                                                                  Rect rect) {
  accumulate_film_body<true>(film, Lbuf, Fbuf, width, height, nsamples, n0, nonfinite_policy, active, active_count, rect);
}

// ---- the display chain's two kernels: one lane per pixel -------------------------------------------------------------------------------------
struct FilmBackdrop { uint32_t backdrop; float rgb[3]; };

__global__ void __launch_bounds__(256) k_film_compose(const vec4* __restrict__ base, const vec4* __restrict__ film, vec4* __restrict__ out,
                                                      uint32_t width, uint32_t height, Rect rect, FilmBackdrop b) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= width * height) return;
  const uint32_t y = p / width, x = p - y * width;
  out[p] = rect_contains(rect, x, y) ? film_compose(base[p], film[p].w, b.backdrop, b.rgb) : vec4{0.0f, 0.0f, 0.0f, 0.0f};
}

__global__ void __launch_bounds__(256) k_film_alpha(uint32_t* __restrict__ target, const vec4* __restrict__ composed, uint32_t npix) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p < npix) target[p] = film_alpha_byte(target[p], composed[p].w);
}

void launch_film_flags(hipStream_t s, uint32_t grid, PathState st, const vec4* hit, Segments seg, uint32_t* Fbuf) {
  hipLaunchKernelGGL(k_film_flags, dim3(grid), dim3(256), 0, s, st, hit, seg, Fbuf);
}

void launch_accumulate_film(hipStream_t s, vec4* film, const vec4* Lbuf, const uint32_t* Fbuf, uint32_t width, uint32_t height, uint32_t nsamples,
                            uint32_t n0, uint32_t nonfinite_policy, const TileSet* tiles) {
  // one block per tile of the image, or per tile that may still be active
  if (tiles)
    hipLaunchKernelGGL(k_accumulate_film_adaptive, dim3(tiles->max_active), dim3(64), 0, s, film, Lbuf, Fbuf, width, height, nsamples, n0,
                       nonfinite_policy, tiles->active, tiles->active_count, tiles->rect);
  else
    hipLaunchKernelGGL(k_accumulate_film, dim3(tile_count(width, height)), dim3(64), 0, s, film, Lbuf, Fbuf, width, height, nsamples, n0,
                       nonfinite_policy);
}

void launch_film_compose(hipStream_t s, const vec4* base, const vec4* film, vec4* out, uint32_t width, uint32_t height, const Rect& rect,
                         const pt_film_options& o) {
  const uint32_t npix = width * height;
  const FilmBackdrop b{o.backdrop, {o.backdrop_rgb[0], o.backdrop_rgb[1], o.backdrop_rgb[2]}};
  hipLaunchKernelGGL(k_film_compose, dim3((npix + 255u) / 256u), dim3(256), 0, s, base, film, out, width, height, rect, b);
}

void launch_film_alpha(hipStream_t s, uint32_t* target, const vec4* composed, uint32_t npix) {
  hipLaunchKernelGGL(k_film_alpha, dim3((npix + 255u) / 256u), dim3(256), 0, s, target, composed, npix);
}

}  // namespace pt
