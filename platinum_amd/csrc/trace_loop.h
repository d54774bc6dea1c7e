// trace_loop.h — what the trace kernels share: the wave helpers, the chunk claims, the wave-cooperative traversal step, the persistent ray loop
// and the closest-hit body.  DEVICE CODE ONLY (hipcc): it is included by the translation units that hold a trace kernel — trace_kernels.hip
// (k_trace_closest, k_trace_shadow) and kernels.hip (k_trace_closest_unlisted, k_trace_ao; k_shade and k_camera_primary use the wave helpers and
// the PT_TAIL_* marks) — and is not one of the PT_HD pt_*.h headers that the host harness compiles.  Each unit compiles it under its own flags
// (Makefile).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.h"
#include "pt_bvh.h"
#include "pt_camlist.h"
#include "queue_plan.h"

namespace pt {

// ---- wave helpers (wave64; wave_lane, wave_index and wave_count are in kernels.h) ------------------------------------
__device__ __forceinline__ uint32_t wave_prefix(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
#ifdef PT_TAIL_PROBE
#define PT_TAIL_BEGIN const unsigned long long tail_t0 = wall_clock64(); unsigned long long tail_take = 0, tail_setup = 0, tail_ta = 0;
#define PT_TAIL_T(acc) { const unsigned long long tb_ = wall_clock64(); acc += tb_ - tail_ta; tail_ta = tb_; }
#define PT_TAIL_MARK tail_ta = wall_clock64();
#define PT_TAIL_END(kind)                                                                                         \
  if (wave_lane() == 0 && bounce < 16u) {                                                                           \
    const unsigned long long t1 = wall_clock64();                                                                   \
    atomicMax(&ctr->tail_end_max[kind][bounce], t1); atomicAdd(&ctr->tail_end_sum[kind][bounce], t1);              \
    atomicMax(&ctr->tail_start_inv[kind][bounce], ~tail_t0); atomicAdd(&ctr->tail_waves[kind][bounce], 1ull);     \
    atomicAdd(&ctr->tail_take[kind][bounce], tail_take); atomicAdd(&ctr->tail_setup[kind][bounce], tail_setup);     \
    atomicAdd(&ctr->tail_busy[kind][bounce], t1 - tail_t0);                                                         \
  }
#else
#define PT_TAIL_BEGIN
#define PT_TAIL_END(kind)
#define PT_TAIL_T(acc)
#define PT_TAIL_MARK
#endif

// ---- chunk claims for the trace kernels ------------------------------------------------------------------------------
// 64-ray chunks claimed per cursor atomic.  ONE L2 address sustains ~88 returning atomics per microsecond
// (MI355X_MICROARCH.md "dequeue"); at 2 chunks per claim the C2 closest-hit kernel (10.6 Grays/s = 166 chunks/us) ran AT that
// limit and C3 at two thirds of it — 73 % of the C2 kernel's wave time was s_waitcnt.  Claims are therefore "guided": 8 chunks
// while plenty of work is left, then 4, 2, 1 towards the end of the list so that the last waves finish together
// (a fixed 8 costs C3 3 % in the tail; guided, C2 closest-hit went from 36.2 to 23.0 ms per step, shadow from 26.0 to 15.4).
constexpr uint32_t kClaimMax = 8;

// A chunk-table entry: segment (16 bits: nseg <= 32768), chunk within the segment (10 bits: seg_cap <= 65536), rays in the chunk - 1 (6 bits).
__device__ __forceinline__ uint32_t chunk_entry(uint32_t sg, uint32_t k, uint32_t rays) { return ((rays - 1u) << 26) | (k << 16) | sg; }
static_assert(kMaxSegments <= 65536 && kMaxSegmentSlots / 64 <= 1024, "chunk_entry packs 16 + 10 + 6 bits");

struct ChunkClaims {
  const uint32_t* __restrict__ table;   // [total + 8] chunk_entry(segment, chunk, rays) for every non-empty chunk, segment-major
  uint32_t* cursor;
  uint32_t nseg, total, lane;
  uint32_t next_c, end_c, run_c = 0;
  uint32_t e0 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0, e5 = 0, e6 = 0, e7 = 0;   // the entries of the run being consumed (wave-uniform: scalar registers)
  uint32_t claim_k = kClaimMax, nwaves_grid = 1;
  __device__ __forceinline__ void init(const uint32_t* tab, uint32_t total_, uint32_t* cur, const Segments& seg, uint32_t lane_) {
    table = tab; total = total_; cursor = cur; nseg = seg.nseg; lane = lane_;
    next_c = end_c = 0;
    nwaves_grid = gridDim.x * (blockDim.x >> 6);
    claim_k = guided(total);
  }
  __device__ __forceinline__ uint32_t guided(uint32_t remaining) const {
    return remaining > 32u * nwaves_grid ? kClaimMax : remaining > 8u * nwaves_grid ? 4u : remaining > 2u * nwaves_grid ? 2u : 1u;
  }
  // ---- per-lane ray replacement ----
  // The wave keeps a pool = the not yet started rays [pool_next, pool_end) of its current chunk.  Lanes whose ray has
  // finished (need == true) take the next pool entries in lane order; an empty pool is refilled from the claim list.
  // Wave-uniform call. Returns kInvalidRef for lanes that got nothing; `exhausted` = no chunk left anywhere.
  uint32_t pool_next = 0, pool_end = 0;
  bool exhausted = false;
  __device__ __forceinline__ uint32_t take(bool need) {
    uint32_t got = kInvalidRef;
    for (;;) {
      const unsigned long long m = __ballot(need && got == kInvalidRef);
      if (m == 0) return got;
      if (pool_next == pool_end) {
        if (exhausted) return got;
        if (next_c == end_c) {
          uint32_t base = 0;
          if (lane == 0) base = atomicAdd(cursor, claim_k);
          base = __builtin_amdgcn_readfirstlane(base);
          if (base >= total) { exhausted = true; return got; }
          next_c = run_c = base;
          end_c = base + claim_k < total ? base + claim_k : total;
          claim_k = guided(total - end_c);
          // the entries of the whole run in ONE load (lanes 0..7; the table is padded by kClaimMax entries): the wave waits for
          // the claim and for this once per run of up to 8 chunks — with one entry + one segment count fetched per chunk it spent 5 % (C3) to
          // 15 % (C2) of its time here (r6, -DPT_TAIL_PROBE)
          const int ev = (int)table[base + (lane & 7u)];   // (one register; lanes 0..7 hold the run)
          e0 = (uint32_t)__builtin_amdgcn_readlane(ev, 0); e1 = (uint32_t)__builtin_amdgcn_readlane(ev, 1); e2 = (uint32_t)__builtin_amdgcn_readlane(ev, 2);
          e3 = (uint32_t)__builtin_amdgcn_readlane(ev, 3); e4 = (uint32_t)__builtin_amdgcn_readlane(ev, 4); e5 = (uint32_t)__builtin_amdgcn_readlane(ev, 5);
          e6 = (uint32_t)__builtin_amdgcn_readlane(ev, 6); e7 = (uint32_t)__builtin_amdgcn_readlane(ev, 7);
        }
        const uint32_t at = next_c++ - run_c;
        const uint32_t e = at == 0u ? e0 : at == 1u ? e1 : at == 2u ? e2 : at == 3u ? e3 : at == 4u ? e4 : at == 5u ? e5 : at == 6u ? e6 : e7;
        pool_next = seg_slot(nseg, e & 0xffffu, ((e >> 16) & 0x3ffu) * 64u);
        pool_end = pool_next + (e >> 26) + 1u;
      }
      if (need && got == kInvalidRef) {
        const uint32_t idx = pool_next + wave_prefix(m);
        if (idx < pool_end) got = idx;
      }
      const uint32_t avail = pool_end - pool_next, want = (uint32_t)__popcll(m);
      pool_next += want < avail ? want : avail;
    }
  }
};

// ---- wave-cooperative traversal step ---------------------------------------------------------------------------------
// One iteration for the lanes of a wave that still hold a ray: (1) lanes with a node to visit and room in their leaf
// queue visit it (trav_node: slab tests, candidate leaves queued, next node chosen); (2) the wave votes — when at least
// half of these lanes have a queued leaf, or a lane cannot go on without emptying its queue (queue full, or node stack
// exhausted with nobody else able to advance), every lane with a queued leaf runs ONE triangle test.  The triangle code
// therefore executes with most lanes busy instead of whenever a single lane met a leaf.  A ray is finished when its node
// stack is exhausted and its queue is empty (any-hit: on the first accepted hit).
#ifndef PT_TRI_VOTE
#define PT_TRI_VOTE 2
#endif
template <class W, bool ANY, bool COUNT>
__device__ __forceinline__ void wave_traverse(const DeviceScene& S, const BvhNode* lds_nodes, TravState& ts, TraversalCount* tc) {
  constexpr int kFull = W::kPendRows - W::kRoom;   // a lane with more leaves queued has no room for a node step's
  if (ts.cur != kInvalidRef && ts.st.npend <= kFull) {
    if (W::kTwoLevel) {
      // Exit markers are handled at once; ENTERING an instance (two dependent loads, three divides) is voted on like the
      // triangle tests: it runs when half of the lanes that can advance are waiting at an instance, or nobody has a node.
      trav_leave(ts);
      const bool at_inst = ts.cur != kInvalidRef && (ts.cur & kInstBit) != 0;
      const bool at_node = ts.cur != kInvalidRef && !at_inst;
      const unsigned long long mi = __ballot(at_inst), mn = __ballot(at_node);
      if (mi != 0 && (2 * __popcll(mi) >= __popcll(mn) || mn == 0)) {
        if (at_inst) trav_resolve(S, ts);
      } else if (at_node) {
        if (lds_nodes) W::template node<COUNT>(lds_nodes, ts, tc); else W::template node<COUNT>(S.nodes, ts, tc);
      }
    } else {
      W::template node<COUNT>(S.nodes, ts, tc);
    }
  }
  const bool pending = ts.st.npend > 0;
  const bool stuck = pending && (ts.cur == kInvalidRef || ts.st.npend > kFull);
  const bool advancing = ts.cur != kInvalidRef && !stuck;
  const unsigned long long mp = __ballot(pending);
  if (mp == 0) return;
  // triangle round when half of the lanes holding a ray have a queued leaf, a lane's queue is full, or nobody can advance
  const bool go = PT_TRI_VOTE * __popcll(mp) >= __popcll(__ballot(1)) || __ballot(ts.st.npend > kFull) != 0 || __ballot(advancing) == 0;
  if (go && pending) {
    if (W::template leaf<ANY, COUNT>(S, ts, tc)) { ts.cur = kInvalidRef; ts.st.npend = 0; ts.st.sp = 0; }
  }
}

// the two-level structure's nodes -> LDS (when they fit); returns the pointer the traversal should use (nullptr: HBM)
__device__ __forceinline__ const BvhNode* stage_nodes(const DeviceScene& S, BvhNode* lds_nodes, uint32_t room) {
  if (S.node_count > room) return nullptr;
  const uint4* src = reinterpret_cast<const uint4*>(S.nodes);
  uint4* dst = reinterpret_cast<uint4*>(lds_nodes);
  for (uint32_t i = threadIdx.x; i < S.node_count * 4; i += blockDim.x) dst[i] = src[i];
  __syncthreads();
  return lds_nodes;
}

// ---- the persistent ray loop of the trace kernels ---------------------------------------------------------------------
// What k_trace_closest, k_trace_closest_unlisted and k_trace_shadow share: the LDS stack and leaf queue (and the staged nodes), the chunk
// claims from `table` / `total` / `cursor`, the take / traverse / refill-vote loop over the wave's 64 rays, the COUNT fold into *nodes / *tris
// and the PT_TAIL_* marks of kind TAIL.  The kernel owns the ray (`ts`, `ray`) and says what differs: begin(stack, tc) loads ray `ray` and
// runs trav_init on it (or drops it: ray = kInvalidRef), true = finished at once; finish() writes the ray's result and sets ray = kInvalidRef.
template <class W, bool ANY, bool COUNT, int TAIL, class Begin, class Finish>
__device__ __forceinline__ void trace_rays(const DeviceScene& S, const Segments& seg, const uint32_t* __restrict__ table, uint32_t total,
                                           uint32_t* __restrict__ cursor, uint32_t* __restrict__ spill, BatchCounters* __restrict__ ctr, uint32_t bounce,
                                           unsigned long long* nodes, unsigned long long* tris, Begin begin, Finish finish) {
  PT_TAIL_BEGIN
  constexpr uint32_t kTB = W::kThreads;
  __shared__ uint32_t lds_stack[W::kStackRows + 1][kTB];
  __shared__ uint32_t lds_pend[W::kPendRows + 1][kTB];
  __shared__ BvhNode lds_nodes_buf[W::kLdsNodes ? W::kLdsNodes : 1];
  const BvhNode* lds_nodes = W::kLdsNodes ? stage_nodes(S, lds_nodes_buf, W::kLdsNodes) : nullptr;
  const uint32_t lane = wave_lane();
  ChunkClaims src;
  src.init(table, total, cursor, seg, lane);
  TraversalStack stack;
  stack.lds = &lds_stack[0][threadIdx.x];
  stack.pend = &lds_pend[0][threadIdx.x];
  stack.lds_stride = kTB;
  stack.spill = spill + ((size_t)blockIdx.x * kTB + threadIdx.x);
  stack.spill_stride = gridDim.x * kTB;
  TraversalCount tc;

  // (written as an explicit init / step loop: with the whole traversal behind one call the compiler produced a kernel
  //  1.5x slower on secondary rays)
  TravState ts;
  uint32_t ray = kInvalidRef;
  const uint32_t refill = seg.refill_threshold;
  for (;;) {
    PT_TAIL_MARK
    const uint32_t fresh = src.take(ray == kInvalidRef);
    PT_TAIL_T(tail_take)
    if (fresh != kInvalidRef) {
      ray = fresh;
      if (begin(ray, ts, stack, COUNT ? &tc : nullptr)) finish(ray, ts);
    }
    PT_TAIL_T(tail_setup)
    if (__ballot(ray != kInvalidRef) == 0) {
      if (src.exhausted && src.pool_next == src.pool_end) break;
      continue;
    }
    while (ray != kInvalidRef) {
      wave_traverse<W, ANY, COUNT>(S, lds_nodes, ts, &tc);
      if (ts.cur == kInvalidRef && ts.st.npend == 0) finish(ray, ts);
      // lanes still in this loop vote: leave for a refill once the wave has emptied below the threshold
      if (refill && !src.exhausted && (uint32_t)__popcll(__ballot(ray != kInvalidRef)) < refill) break;
    }
  }
  if (COUNT) {
    const uint32_t nn = wave_sum(tc.nodes), t = wave_sum(tc.tris);
    if (lane == 0) {
      atomicAdd(nodes, (unsigned long long)nn);
      atomicAdd(tris, (unsigned long long)t);
    }
  }
  PT_TAIL_END(TAIL)
}

// ---- closest hit ---------------------------------------------------------------------------------------------------
// (the body of k_trace_closest.  UNLISTED: the instantiation behind k_trace_closest_unlisted, which walks the tree for the camera rays of the
//  pixels whose list did not fit and drops every other ray of the queue: k_camera_primary has traced those.  `cursor`: the launch's claim cursor.)
template <class W, bool COUNT, bool UNLISTED>
__device__ __forceinline__ void trace_closest_body(const DeviceScene& S, PathState st, vec4* __restrict__ hit, const Segments& seg, uint32_t cur,
                                                   BatchCounters* __restrict__ ctr, uint32_t bounce, uint32_t* __restrict__ cursor,
                                                   uint32_t* __restrict__ spill, int32_t* __restrict__ hitlog, uint32_t log_stride, const CameraLists& cl) {
  auto begin = [&](uint32_t& ray, TravState& ts, const TraversalStack& stack, TraversalCount* tc) {
    const vec4 o4 = st.rayO[ray];
    const vec4 d4 = st.rayD[ray];
    float ir = 0.0f;  // alpha-test payload: the sample drawn before `intersect` (kernel.metal:510), only needed with cut-outs
    if (S.has_alpha) ir = Halton{halton_table(S.halton), f2u(st.att[ray].w), f2u(d4.w) & kMetaDimMask}.sample1d();
#ifdef PT_DEBUG_PID
    ts.dbg = ctr->_pad[1] == bounce + 1u && segment_lbuf_base(seg, slot_segment(seg.nseg, ray)) + (f2u(d4.w) >> kMetaPidShift) == ctr->_pad[0];
    if (ts.dbg) printf("dbg ray slot %u lane %u wave %u o %.9g %.9g %.9g d %.9g %.9g %.9g\n", ray, wave_lane(), wave_index(), o4.x, o4.y, o4.z, d4.x, d4.y, d4.z);
#endif
    if (UNLISTED && cl.count[pixel_slot_of_pid(segment_lbuf_base(seg, slot_segment(seg.nseg, ray)) + (f2u(d4.w) >> kMetaPidShift), seg.nsamples)] != kCamWalk) {
      ray = kInvalidRef;   // a listed pixel's ray: hit[ray] holds k_camera_primary's answer
      return false;
    }
    return trav_init(S, ts, v3(o4.x, o4.y, o4.z), v3(d4.x, d4.y, d4.z), 1e-3f, kInf, ir, stack, false, tc);
  };
  auto finish = [&](uint32_t& ray, TravState& ts) {
    const RayHit& h = ts.best;
#ifdef PT_DEBUG_PID
    if (ts.dbg) printf("dbg finish: t %.9g u %.9g v %.9g tri %u gid %u\n", h.t, h.u, h.v, h.tri, h.gid >> 2);
    ts.dbg = false;
#endif
    hit[ray] = vec4{h.t, h.u, h.v, u2f(hit_word(h))};
    if (hitlog) {
      // (the hit log is only kept for one-sample batches)
      const uint32_t pixel = pixel_of_pid_1spp(segment_lbuf_base(seg, slot_segment(seg.nseg, ray)) + (f2u(st.rayD[ray].w) >> kMetaPidShift), S.width);
      int32_t* hl = &hitlog[((size_t)bounce * log_stride + pixel) * 2];
      hl[0] = hl[1] = -1;
      if (h.tri != kInvalidRef) triangle_ids(S, h.tri, &hl[0], &hl[1]);
    }
    ray = kInvalidRef;
  };
  trace_rays<W, false, COUNT, 0>(S, seg, seg.table_closest, ctr->chunks_closest[bounce], cursor, spill, ctr, bounce, &ctr->nodes_closest, &ctr->tris_closest,
                                 begin, finish);
}

// ---- host: the structure S holds and `count` -> (its description, COUNT) as types ------------------------------------------------------
// launch(Walk{}, std::bool_constant<COUNT>{}) launches that instantiation.
template <class F> static void launch_walk(const DeviceScene& S, bool count, F launch) {
  auto counted = [&](auto walk) { if (count) launch(walk, std::true_type{}); else launch(walk, std::false_type{}); };
  if (S.two_level) counted(WalkTwoLevel{}); else if (S.wide6) counted(Walk6{}); else counted(Walk4{});
}

}  // namespace pt
