// trace_kernels.hip — k_trace_closest and k_trace_shadow, the two trace kernels of every bounce, and their launchers.
//
// A translation unit of their own because they are compiled WITHOUT LLVM's SLP vectoriser (Makefile: -fno-slp-vectorize).  Under plain -O3
// the pass packs the vec3 arithmetic of the slab and triangle tests into v_pk_mul_f32 / v_pk_add_f32; those want even-aligned register
// pairs, which cost these kernels 6 to 9 VGPRs each, and a packed f32 instruction issues no faster than its two scalar halves
// (MI355X_MICROARCH.md).  Packed and scalar forms are the same IEEE operation per lane and contraction stays off: not a bit of a result
// depends on the flag.  Without it the closest-hit kernel fits the 72 registers of a seventh wave per SIMD (Walk::kClosestTraceBlocksPerCu)
// with no spill.  The loop itself is trace_loop.h; the other kernels over that loop (k_trace_closest_unlisted, k_trace_ao) stay in kernels.hip,
// built as they were.  What the build holds these kernels to: tests/test_trace_unit_resources.py.
//
// Compiled with -ffp-contract=off (deterministic fp32 contract, pt_math.h).
#include <hip/hip_runtime.h>

#include "trace_loop.h"

namespace pt {

// ---- closest hit (trace_closest_body, trace_loop.h) ---------------------------------------------------------------------------------
// (The counting instantiation — pt_measure_traversal's, never a render's — keeps kClosestBlocksPerCu and is launched on that grid: with its
//  counters it needs 75 registers, and held to 72 it would spill one of them.)
template <class W, bool COUNT>
__global__ void __launch_bounds__(W::kThreads, COUNT ? W::kClosestBlocksPerCu : W::kClosestTraceBlocksPerCu)
k_trace_closest(DeviceScene S, PathState st, vec4* __restrict__ hit, Segments seg, uint32_t cur, BatchCounters* __restrict__ ctr, uint32_t bounce,
                uint32_t* __restrict__ spill, int32_t* __restrict__ hitlog, uint32_t log_stride) {
  trace_closest_body<W, COUNT, false>(S, st, hit, seg, cur, ctr, bounce, &ctr->work_closest[bounce], spill, hitlog, log_stride, CameraLists{});
}

// ---- shadow (any hit) --------------------------------------------------------------------------------------------------
template <class W, bool COUNT>
__global__ void __launch_bounds__(W::kThreads, W::kShadowBlocksPerCu)
k_trace_shadow(DeviceScene S, ShadowQueue sq, vec4* __restrict__ Lbuf, Segments seg, BatchCounters* __restrict__ ctr, uint32_t bounce,
               uint32_t* __restrict__ spill) {
  uint32_t pid = 0;
  auto begin = [&](uint32_t& ray, TravState& ts, const TraversalStack& stack, TraversalCount* tc) {
    const vec4 o4 = sq.o[ray];
    const vec4 d4 = sq.d[ray];
    pid = f2u(d4.w);
    const float ir = S.has_alpha ? sq.contrib[ray].w : 0.0f;  // kernel.metal:625
    return trav_init(S, ts, v3(o4.x, o4.y, o4.z), v3(d4.x, d4.y, d4.z), 1e-3f, o4.w, ir, stack, true, tc);
  };
  auto finish = [&](uint32_t& ray, TravState& ts) {
    if (ts.best.tri == kInvalidRef) {  // unoccluded: L += attenuation * Ld (kernel.metal:631-637)
      const vec4 c = sq.contrib[ray];
      vec4 L = Lbuf[pid];
      L.x += c.x; L.y += c.y; L.z += c.z;
      Lbuf[pid] = L;
    }
    ray = kInvalidRef;
  };
  trace_rays<W, true, COUNT, 2>(S, seg, seg.table_shadow, ctr->chunks_shadow[bounce], &ctr->work_shadow[bounce], spill, ctr, bounce, &ctr->nodes_shadow,
                                &ctr->tris_shadow, begin, finish);
}

// ---- launchers (host) ---------------------------------------------------------------------------------------------------
template <class W> static TraceWalk trace_walk_of() {
  return {(uint32_t)W::kThreads, (uint32_t)W::kClosestBlocksPerCu, (uint32_t)W::kClosestTraceBlocksPerCu, (uint32_t)W::kShadowBlocksPerCu, !W::kTwoLevel,
          W::kPushesPerLevel, W::kExitEntries};
}
TraceWalk trace_walk(bool two_level, bool wide6) { return two_level ? trace_walk_of<WalkTwoLevel>() : wide6 ? trace_walk_of<Walk6>() : trace_walk_of<Walk4>(); }
void launch_trace_closest(hipStream_t s, uint32_t grid, const DeviceScene& S, PathState st, vec4* hit, Segments seg, uint32_t cur,
                          BatchCounters* ctr, uint32_t bounce, uint32_t* spill, int32_t* hitlog, uint32_t log_stride, bool count) {
  launch_walk(S, count, [&](auto walk, auto counted) {
    using W = decltype(walk);
    hipLaunchKernelGGL((k_trace_closest<W, decltype(counted)::value>), dim3(grid), dim3(W::kThreads), 0, s, S, st, hit, seg, cur, ctr, bounce, spill, hitlog, log_stride);
  });
}
void launch_trace_shadow(hipStream_t s, uint32_t grid, const DeviceScene& S, ShadowQueue sq, vec4* Lbuf, Segments seg,
                         BatchCounters* ctr, uint32_t bounce, uint32_t* spill, bool count) {
  launch_walk(S, count, [&](auto walk, auto counted) {
    using W = decltype(walk);
    hipLaunchKernelGGL((k_trace_shadow<W, decltype(counted)::value>), dim3(grid), dim3(W::kThreads), 0, s, S, sq, Lbuf, seg, ctr, bounce, spill);
  });
}

}  // namespace pt
