// projection.hip — ray generation under the projections of pt_projection.h.
//
//   k_raygen_projected<false>    k_raygen's counterpart: the camera rays of a full-frame batch under an orthographic, equirectangular or
//                                fisheye camera
//   k_raygen_projected<true>     k_raygen_adaptive's: the same over the active tiles and the rectangle of an adaptive or region render
//   k_camera_rays                pt_debug_camera_rays: the bounce-0 queue of a one-sample batch, scattered to pixel order
// Only a render started under a projection other than PT_PROJ_PERSPECTIVE launches the first two (renderer.hip launch_camera_raygen); a
// perspective render launches k_raygen / k_raygen_adaptive as ever.  Everything but the stage function mirrors kernels.hip: the segment
// walk, the pixel-major / sample-minor order, the ballot compaction, seg_slot, lbuf_index, the Lbuf reset, the segment's count and poison
// word, and the wave statistics — so every kernel behind it finds the queue k_raygen would have left for the same rays.
//
// Compiled with -ffp-contract=off (deterministic fp32 contract, pt_math.h).
#include <hip/hip_runtime.h>

#include "projection.h"
#include "pt_tilefold.h"

namespace pt {

__device__ __forceinline__ uint32_t pj_wave_prefix(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// TILES = false: `tiles` = the image's tile count, a pixel is valid inside the image.  TILES = true: virtual tile t < *active_count is image
// tile active[t], a pixel is valid inside `rect`.  KIND: the projection, chosen once per wave by the kernel below.
template <bool TILES, uint32_t KIND>
__device__ __forceinline__ void raygen_projected_body(const DeviceScene& S, const ProjectionConstants& P, const PathState& st, vec4* __restrict__ Lbuf,
                                                      const Segments& seg, uint32_t first_sample, uint32_t nsamples, uint32_t tilesX, uint32_t tiles,
                                                      const Rect& rect, const uint32_t* __restrict__ active) {
  const uint32_t lane = wave_lane();
  uint32_t started = 0;
  for (uint32_t sg = wave_index(); sg < seg.nseg; sg += wave_count()) {
    uint32_t n_out = 0;
    const uint32_t first_tile = segment_first_tile(seg, sg);
    for (uint32_t k = 0; k < seg.tiles_per_seg * nsamples; k++) {
      const uint32_t tile = first_tile + k / nsamples;
      if (tile >= tiles) break;  // wave-uniform
      const uint32_t r = (k % nsamples) * 64u + lane;   // ray r of the tile's 64 * nsamples, pixel-major
      const uint32_t pl = r / nsamples, s = r - pl * nsamples;
      const PixelXY q = tile_pixel(TILES ? active[tile] : tile, pl, tilesX);
      const bool valid = TILES ? rect_contains(rect, q.x, q.y) : (q.x < S.width && q.y < S.height);
      RayGenOut rg;
      if (valid) rg = stage_raygen_kind<KIND>(S, P, q.x, q.y, first_sample + s);
      const unsigned long long m = __ballot(valid);
      if (valid) {
        const uint32_t j = seg_slot(seg.nseg, sg, n_out + pj_wave_prefix(m));
        const uint32_t pid = lbuf_index(tile, s, nsamples, pl);
        const uint32_t rel = pid - first_tile * nsamples * 64u;  // relative to the segment's window (segment_lbuf_base)
        st.rayO[j] = vec4{rg.o.x, rg.o.y, rg.o.z, 0.0f};
        st.rayD[j] = vec4{rg.d.x, rg.d.y, rg.d.z, u2f((rg.dim & kMetaDimMask) | (rel << kMetaPidShift))};
        st.att[j] = vec4{1.0f, 1.0f, 1.0f, u2f(rg.offset)};
        Lbuf[pid] = vec4{0.0f, 0.0f, 0.0f, 1.0f};
      }
      n_out += (uint32_t)__popcll(m);
    }
    if (lane == 0) { seg.active[0][sg] = n_out; seg.poison[sg] = 0u; }
    started += n_out;
  }
  if (lane == 0) {
    WaveStats& ws = seg.stats[wave_index()];
    ws.paths += started;
    ws.closest += started;
  }
}

// P.kind is a kernel argument: the switch is wave-uniform, taken once, outside the loops.  amdgpu_waves_per_eu(8): the vector registers fit
// eight waves per SIMD with room to spare (k_raygen's budget), but with two structs of scene and projection constants in the argument list
// the compiler otherwise keeps 106 scalar registers live, which it counts as seven waves; told the minimum it stays at 78 and parks the rest in VGPR lanes (no scratch).
template <bool TILES>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8))) k_raygen_projected(DeviceScene S, ProjectionConstants P, PathState st, vec4* __restrict__ Lbuf, Segments seg,
                                                              uint32_t first_sample, uint32_t nsamples, uint32_t tilesX, uint32_t tilesY, Rect rect,
                                                              const uint32_t* __restrict__ active, const uint32_t* __restrict__ active_count) {
  const uint32_t tiles = TILES ? *active_count : tilesX * tilesY;
  if (P.kind == PT_PROJ_ORTHOGRAPHIC)
    raygen_projected_body<TILES, PT_PROJ_ORTHOGRAPHIC>(S, P, st, Lbuf, seg, first_sample, nsamples, tilesX, tiles, rect, active);
  else if (P.kind == PT_PROJ_EQUIRECT)
    raygen_projected_body<TILES, PT_PROJ_EQUIRECT>(S, P, st, Lbuf, seg, first_sample, nsamples, tilesX, tiles, rect, active);
  else
    raygen_projected_body<TILES, PT_PROJ_FISHEYE>(S, P, st, Lbuf, seg, first_sample, nsamples, tilesX, tiles, rect, active);
}

// One lane per queue entry of a one-sample batch (k_hit_records' walk): the ray's pixel through the pid in rayD.w.
__global__ void __launch_bounds__(kBlock) k_camera_rays(uint32_t width, PathState st, Segments seg, float* __restrict__ origins,
                                                         float* __restrict__ directions) {
  const uint32_t lane = wave_lane();
  for (uint32_t sg = wave_index(); sg < seg.nseg; sg += wave_count()) {
    const uint32_t n = seg.active[0][sg];
    for (uint32_t k = lane; k < n; k += 64) {
      const uint32_t i = seg_slot(seg.nseg, sg, k);
      const vec4 o = st.rayO[i], d = st.rayD[i];
      const size_t p = 3 * (size_t)pixel_of_pid_1spp(segment_lbuf_base(seg, sg) + (f2u(d.w) >> kMetaPidShift), width);
      if (origins) { origins[p] = o.x; origins[p + 1] = o.y; origins[p + 2] = o.z; }
      if (directions) { directions[p] = d.x; directions[p + 1] = d.y; directions[p + 2] = d.z; }
    }
  }
}

void launch_raygen_projected(hipStream_t s, uint32_t grid, const DeviceScene& S, const ProjectionConstants& P, PathState st, vec4* Lbuf, Segments seg,
                             uint32_t first_sample, uint32_t nsamples, const TileSet* tiles) {
  if (tiles)
    hipLaunchKernelGGL(k_raygen_projected<true>, dim3(grid), dim3(kBlock), 0, s, S, P, st, Lbuf, seg, first_sample, nsamples, tiles_x(S.width),
                       tiles_y(S.height), tiles->rect, tiles->active, tiles->active_count);
  else
    hipLaunchKernelGGL(k_raygen_projected<false>, dim3(grid), dim3(kBlock), 0, s, S, P, st, Lbuf, seg, first_sample, nsamples, tiles_x(S.width),
                       tiles_y(S.height), Rect{}, nullptr, nullptr);
}

void launch_camera_rays(hipStream_t s, uint32_t grid, uint32_t width, PathState st, Segments seg, float* origins, float* directions) {
  hipLaunchKernelGGL(k_camera_rays, dim3(grid), dim3(kBlock), 0, s, width, st, seg, origins, directions);
}

}  // namespace pt
