// denoise.hip — first-hit AOVs and the a-trous denoiser on the device (pt_denoise.h holds the arithmetic; DESIGN.md §3 "Denoiser").
//
//   k_aov             after k_trace_closest(bounce 0), before k_shade(0): per camera ray, stage_aov -> Abuf[pid] (32 B)
//   k_accumulate_aov  after k_accumulate / k_gmon: folds Abuf and Lbuf into the three AOV images, per pixel in sample order
//                     (k_accumulate_aov_adaptive: the same over the active tiles of an adaptive render)
//   k_dn_prep         demodulation, variance, depth gradient (k_dn_prep_counts: with per-pixel sample counts, adaptive renders)
//   k_dn_despeckle    the optional firefly clamp between the prep and the first a-trous step (col0 -> col1)
//   k_atrous          one 5x5 step per launch (ping-pong); the last one remodulates
// The filter runs over a rectangle of the frame as if it were the whole image (a render region): its kernels take W x H of
// the rectangle, the frame's width as the row pitch, and pointers to the rectangle's first pixel.
// Only a render started with AOVs enabled launches any of them (renderer.hip enqueue_batch).
//
// Compiled with -ffp-contract=off (deterministic fp32 contract, pt_math.h).
#include <hip/hip_runtime.h>

#include "denoise.h"
#include "pt_denoise.h"
#include "pt_tilefold.h"

namespace pt {

// ---- k_aov: the bounce-0 queue (pt_tilefold.h walk_bounce0) -> Abuf.  Reads the queue only. ----------------------------------------
// Abuf[2 * pid] = {albedo, t}, Abuf[2 * pid + 1] = {normal, 1} for a hit; {1, 1, 1, 0}, {0, 0, 0, 0} for a miss.
__global__ void __launch_bounds__(256) k_aov(const DeviceScene* __restrict__ Sp, PathState st, const vec4* __restrict__ hit, Segments seg,
                                             vec4* __restrict__ Abuf) {
  const DeviceScene& S = *Sp;
  const uint32_t lane = wave_lane(), wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwaves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t sg = wave; sg < seg.nseg; sg += nwaves)
    walk_bounce0(seg, st, hit, sg, lane, [&](uint32_t i, uint32_t pid, uint32_t hw) {
      const vec4 h4 = hit[i], d4 = st.rayD[i];
      AovSample a = aov_miss();
      float hf = 0.0f;
      if (!hit_word_miss(hw)) {
        const vec4 o4 = st.rayO[i];
        ShadeIn in;
        in.o = v3(o4.x, o4.y, o4.z);
        in.d = v3(d4.x, d4.y, d4.z);
        in.att = v3(1.0f);
        in.rayO = &st.rayO[i];
        in.rayD = &st.rayD[i];
        in.lastSpecular = false;
        in.offset = 0; in.dim = 0; in.bounce = 0;
        in.t = h4.x; in.u = h4.y; in.v = h4.z;
        in.tri = hit_word_tri(hw);
        a = stage_aov(S, in);
        hf = 1.0f;
      }
      Abuf[2u * pid] = vec4{a.albedo.x, a.albedo.y, a.albedo.z, a.t};
      Abuf[2u * pid + 1u] = vec4{a.normal.x, a.normal.y, a.normal.z, hf};
    });
}

// ---- k_accumulate_aov: one wave per 8x8 tile (pt_tilefold.h fold_tile / fold_stage) -----------------------------------------------
// A round stages three streams (Lbuf and the two halves of Abuf); every lane then folds the samples of its pixel in sample order.  One
// wave per block: the three staging areas take 27 KB.  ADAPTIVE: k_accumulate_aov_adaptive.
template <bool ADAPTIVE>
__device__ __forceinline__ void accumulate_aov_body(vec4* __restrict__ albedo, vec4* __restrict__ normal, vec4* __restrict__ moments,
                                                    const vec4* __restrict__ Abuf, const vec4* __restrict__ Lbuf, uint32_t width,
                                                    uint32_t height, uint32_t nsamples, uint32_t n0, uint32_t nonfinite_policy,
                                                    const uint32_t* __restrict__ active, const uint32_t* __restrict__ active_count, Rect rect) {
  __shared__ vec4 stage[3][64 * kFoldRow];
  const uint32_t lane = wave_lane();
  const FoldTile t = fold_tile<ADAPTIVE>(blockIdx.x, lane, width, height, active, active_count, rect);
  const bool live = t.live, inside = t.inside;
  const size_t p = (size_t)t.q.y * width + t.q.x;
  vec4 A = inside ? albedo[p] : vec4{0, 0, 0, 0}, N = inside ? normal[p] : vec4{0, 0, 0, 0}, M = inside ? moments[p] : vec4{0, 0, 0, 0};
  for (uint32_t s0 = 0; s0 < nsamples; s0 += 8u) {
    const uint32_t nb = nsamples - s0 < 8u ? nsamples - s0 : 8u;
    __syncthreads();
    if (live)
      fold_stage(t.tile, lane, s0, nb, nsamples, [&](uint32_t pid, uint32_t slot) {
        stage[0][slot] = Lbuf[pid];
        stage[1][slot] = Abuf[2u * pid];
        stage[2][slot] = Abuf[2u * pid + 1u];
      });
    __syncthreads();
    if (inside) {
      for (uint32_t j = 0; j < nb; j++) {
        const vec4 l4 = stage[0][lane * kFoldRow + j], a4 = stage[1][lane * kFoldRow + j], n4 = stage[2][lane * kFoldRow + j];
        vec3 L = v3(l4.x, l4.y, l4.z);
        // (not_finite(L), pt_shade.h, written out: behind the call the test compiles branch-free here, a kernel 44 bytes shorter and not the parent's)
        if (!(fabsf(L.x) <= 3.0e38f && fabsf(L.y) <= 3.0e38f && fabsf(L.z) <= 3.0e38f) && nonfinite_policy == PT_NONFINITE_ZERO) L = v3(0.0f);
        const float lum = dn_lum(L);
        const uint32_t n = n0 + s0 + j;
        const vec3 a = aov_fold(v3(A.x, A.y, A.z), v3(a4.x, a4.y, a4.z), n);
        const vec3 nn = aov_fold(v3(N.x, N.y, N.z), v3(n4.x, n4.y, n4.z), n);
        const vec3 m = aov_fold(v3(M.x, M.y, M.z), v3(a4.w, lum, lum * lum), n);
        A = vec4{a.x, a.y, a.z, 1.0f};
        N = vec4{nn.x, nn.y, nn.z, aov_fold(N.w, n4.w, n)};
        M = vec4{m.x, m.y, m.z, 0.0f};
      }
    }
  }
  if (inside) { albedo[p] = A; normal[p] = N; moments[p] = M; }
}

__global__ void __launch_bounds__(64) k_accumulate_aov(vec4* __restrict__ albedo, vec4* __restrict__ normal, vec4* __restrict__ moments,
                                                        const vec4* __restrict__ Abuf, const vec4* __restrict__ Lbuf, uint32_t width,
                                                        uint32_t height, uint32_t nsamples, uint32_t n0, uint32_t nonfinite_policy) {
  accumulate_aov_body<false>(albedo, normal, moments, Abuf, Lbuf, width, height, nsamples, n0, nonfinite_policy, nullptr, nullptr, Rect{});
}

__global__ void __launch_bounds__(64) k_accumulate_aov_adaptive(vec4* __restrict__ albedo, vec4* __restrict__ normal, vec4* __restrict__ moments,
                                                                 const vec4* __restrict__ Abuf, const vec4* __restrict__ Lbuf, uint32_t width,
                                                                 uint32_t height, uint32_t nsamples, uint32_t n0, uint32_t nonfinite_policy,
                                                                 const uint32_t* __restrict__ active, const uint32_t* __restrict__ active_count,
                                                                 Rect rect) {
  accumulate_aov_body<true>(albedo, normal, moments, Abuf, Lbuf, width, height, nsamples, n0, nonfinite_policy, active, active_count, rect);
}

// ---- the filter: 16x16 pixel blocks -----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_dn_prep(const vec4* __restrict__ acc, const vec4* __restrict__ albedo, const vec4* __restrict__ normal,
                                                 const vec4* __restrict__ moments, uint32_t W, uint32_t H, uint32_t pitch, float N,
                                                 vec4* __restrict__ guide, vec4* __restrict__ col, vec4* __restrict__ aux) {
  const uint32_t x = blockIdx.x * 16u + threadIdx.x, y = blockIdx.y * 16u + threadIdx.y;
  if (x < W && y < H) dn_prep_pixel(acc, albedo, normal, moments, W, H, pitch, x, y, N, guide, col, aux);
}

// the prep of an adaptive render: N = the pixel's own sample count, its tile's (dn_prep_pixel_counts); the tile is that of the pixel
// in the frame, (x0 + x, y0 + y)
__global__ void __launch_bounds__(256) k_dn_prep_counts(const vec4* __restrict__ acc, const vec4* __restrict__ albedo, const vec4* __restrict__ normal,
                                                        const vec4* __restrict__ moments, uint32_t W, uint32_t H, uint32_t pitch, uint32_t x0,
                                                        uint32_t y0, const uint32_t* __restrict__ tile_n, vec4* __restrict__ guide,
                                                        vec4* __restrict__ col, vec4* __restrict__ aux) {
  const uint32_t x = blockIdx.x * 16u + threadIdx.x, y = blockIdx.y * 16u + threadIdx.y;
  if (x < W && y < H) dn_prep_pixel_counts(acc, albedo, normal, moments, W, H, pitch, x0, y0, x, y, tile_n, guide, col, aux);
}

// the firefly clamp (dn_despeckle_pixel): 9 loads of col, up to 9 of guide.w, one divide
__global__ void __launch_bounds__(256) k_dn_despeckle(const vec4* __restrict__ guide, const vec4* __restrict__ col_in, vec4* __restrict__ col_out,
                                                      DenoiseParams P, uint32_t pitch, float threshold) {
  const uint32_t x = blockIdx.x * 16u + threadIdx.x, y = blockIdx.y * 16u + threadIdx.y;
  if (x < P.W && y < P.H) dn_despeckle_pixel(guide, col_in, col_out, P, pitch, x, y, threshold);
}

__global__ void __launch_bounds__(256) k_atrous(const vec4* __restrict__ guide, const vec4* __restrict__ aux, const vec4* __restrict__ col_in,
                                                vec4* __restrict__ col_out, const vec4* __restrict__ acc, vec4* __restrict__ out, DenoiseParams P,
                                                uint32_t pitch, uint32_t step, uint32_t last) {
  const uint32_t x = blockIdx.x * 16u + threadIdx.x, y = blockIdx.y * 16u + threadIdx.y;
  if (x < P.W && y < P.H) dn_iterate_pixel(guide, aux, col_in, col_out, acc, out, P, pitch, x, y, step, last != 0);
}

// iterations 0: demodulation and remodulation only, which is the identity: the accumulator itself (alpha 1)
__global__ void __launch_bounds__(256) k_dn_copy(const vec4* __restrict__ acc, vec4* __restrict__ out, uint32_t W, uint32_t H, uint32_t pitch) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < W * H) {
    const uint32_t y = i / W;
    const size_t p = (size_t)y * pitch + (i - y * W);
    const vec4 c = acc[p];
    out[p] = vec4{c.x, c.y, c.z, 1.0f};
  }
}

void launch_aov(hipStream_t s, uint32_t grid, const DeviceScene* S_device, PathState st, const vec4* hit, Segments seg, vec4* Abuf) {
  hipLaunchKernelGGL(k_aov, dim3(grid), dim3(256), 0, s, S_device, st, hit, seg, Abuf);
}

void launch_accumulate_aov(hipStream_t s, vec4* albedo, vec4* normal, vec4* moments, const vec4* Abuf, const vec4* Lbuf, uint32_t width,
                           uint32_t height, uint32_t nsamples, uint32_t n0, uint32_t nonfinite_policy, const TileSet* tiles) {
  // one block per tile of the image, or per tile that may still be active
  if (tiles)
    hipLaunchKernelGGL(k_accumulate_aov_adaptive, dim3(tiles->max_active), dim3(64), 0, s, albedo, normal, moments, Abuf, Lbuf, width, height, nsamples,
                       n0, nonfinite_policy, tiles->active, tiles->active_count, tiles->rect);
  else
    hipLaunchKernelGGL(k_accumulate_aov, dim3(tile_count(width, height)), dim3(64), 0, s, albedo, normal, moments, Abuf, Lbuf, width, height, nsamples,
                       n0, nonfinite_policy);
}

void launch_denoise(hipStream_t s, const vec4* acc, const vec4* albedo, const vec4* normal, const vec4* moments, uint32_t W, uint32_t H,
                    uint32_t nsamples, const DenoiseParams& Pf, uint32_t iterations, vec4* guide, vec4* aux, vec4* col0, vec4* col1, vec4* out,
                    const uint32_t* tile_n, const Rect& rect, const pt_despeckle_options& despeckle) {
  // the rectangle as an image of its own: its size, the frame's width as the pitch, every image from the rectangle's first pixel on
  const uint32_t pitch = W, x0 = rect.x0, y0 = rect.y0;
  const size_t org = (size_t)y0 * pitch + x0;
  W = rect.x1 - rect.x0; H = rect.y1 - rect.y0;
  DenoiseParams P = Pf;
  P.W = W; P.H = H;
  acc += org; albedo += org; normal += org; moments += org; out += org;
  if (iterations == 0) {
    hipLaunchKernelGGL(k_dn_copy, dim3((W * H + 255u) / 256u), dim3(256), 0, s, acc, out, W, H, pitch);
    return;
  }
  guide += org; aux += org; col0 += org; col1 += org;
  const dim3 grid((W + 15u) / 16u, (H + 15u) / 16u), block(16, 16);
  if (tile_n) hipLaunchKernelGGL(k_dn_prep_counts, grid, block, 0, s, acc, albedo, normal, moments, W, H, pitch, x0, y0, tile_n, guide, col0, aux);
  else hipLaunchKernelGGL(k_dn_prep, grid, block, 0, s, acc, albedo, normal, moments, W, H, pitch, (float)nsamples, guide, col0, aux);
  vec4* cin = col0;
  vec4* cout = col1;
  if (despeckle.enabled) {
    hipLaunchKernelGGL(k_dn_despeckle, grid, block, 0, s, guide, cin, cout, P, pitch, despeckle.threshold);
    vec4* t = cin; cin = cout; cout = t;
  }
  for (uint32_t i = 0; i < iterations; i++) {
    hipLaunchKernelGGL(k_atrous, grid, block, 0, s, guide, aux, cin, cout, acc, out, P, pitch, 1u << i, i + 1 == iterations ? 1u : 0u);
    vec4* t = cin; cin = cout; cout = t;
  }
}

}  // namespace pt
