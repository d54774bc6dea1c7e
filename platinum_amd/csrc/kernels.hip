// kernels.hip — the gfx950 wavefront path-tracing kernels (all but k_trace_closest and k_trace_shadow: trace_kernels.hip, over the ray loop of
// trace_loop.h, which the closest-hit walks kept here share).
//
// One batch = `nsamples` samples of every pixel traced together.  Per bounce b:
//     k_trace_closest(b)  ->  k_shade(b)  ->  k_trace_shadow(b)
// preceded by k_raygen and followed by k_accumulate.  All kernels are stream-ordered; queue sizes never visit the host.
//
// Queues are SEGMENTS.  A segment is the queue share of a few 8x8 pixel tiles (Segments::tiles_per_seg, 1 unless the image
// has more than 32768 tiles) under all samples of the batch: segment s owns the slots {seg_slot(s, r) : r < seg_cap} of
// every queue array (interleaved in groups of 16 chunks, pt_layout.h seg_slot) and one count per queue.  A segment is always processed by ONE wave
// at a time, front to back: k_raygen fills it, k_shade shades it and compacts the survivors (ballot + mbcnt prefix) into
// the same segment of the other state buffer and its NEE rays into the same segment of the shadow queue.  Survivors <=
// inputs, so a segment never overflows and NO atomic sits on the producer side.  (Round-1 measurement: with one global
// append counter per queue, raygen and shade were pinned at the ~88 returning atomics/us one L2 address sustains —
// MI355X_MICROARCH.md "dequeue"; raygen got 6.7x faster without it.)  The producers are persistent grids: there are ~8x
// more segments than resident waves, so the grid can be sized for whatever occupancy a kernel's registers allow and the
// tile count never has to divide it.  k_raygen's waves take segments round-robin; k_shade's waves claim them LONGEST FIRST
// from a list k_chunk_tables sorts after every producer (r6: in plain order the chip idled 10-14 % of every k_shade launch
// waiting for the waves that had drawn a long segment last).
// The trace kernels consume DENSE CHUNK TABLES: after every producer, k_chunk_tables lists the non-empty 64-entry
// chunks of all segments, segment-major (= image tiles in raster order, each under its samples; an entry names its
// segment, chunk and ray count), and the trace waves claim runs of that list from one cursor (8 chunks per atomic, fewer
// towards the end of the list; a run's entries arrive in one load): the rays in flight at any moment come from a
// small neighbourhood of the image, there are no empty chunks to sweep, and a chunk of survivors still comes from one
// tile.  Results are written in place (hit[i], Lbuf[pid]), so it does not matter which wave traces a ray.  Statistics
// are kept per physical wave (no atomics) and reduced by k_fold_counters.
//
// Compiled with -ffp-contract=off (deterministic fp32 contract, pt_math.h).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.h"
#include "pt_ao.h"
#include "pt_camlist.h"
#include "pt_denoise.h"
#include "pt_post.h"
#include "pt_shade.h"
#include "pt_tilefold.h"
#include "queue_plan.h"
#include "trace_loop.h"

namespace pt {

// Queue entries are written once and read once.  k_shade moves them with non-temporal loads / stores so that they do not push the
// tables, vertices and LUT texels it gathers out of the caches (k_shade -2.4 % on C3 and C2; the same on the ray loads and hit stores
// of the trace kernels changed nothing on C3 and cost 2 % on C2).
__device__ __forceinline__ vec4 ld_stream(const vec4* p) {
  using f4 = __attribute__((ext_vector_type(4))) float;
  const f4 v = __builtin_nontemporal_load((const f4*)p);
  return vec4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ uint32_t ld_stream(const uint32_t* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st_stream(vec4* p, vec4 v) {
  using f4 = __attribute__((ext_vector_type(4))) float;
  __builtin_nontemporal_store(f4{v.x, v.y, v.z, v.w}, (f4*)p);
}
__device__ __forceinline__ void st_stream(uint32_t* p, uint32_t v) { __builtin_nontemporal_store(v, p); }

// Lists the non-empty chunks of every segment, segment-major.  blockIdx.y = 0: the closest-hit queue (state buffer `cur`);
// 1: the shadow queue.  kTableBlocks blocks per list, each owning a contiguous slice of the segments: a block first sums
// the chunk counts of all segments before its slice (its base offset), scans its own slice in LDS, then all of its threads write
// the slice's entries cooperatively (entry -> segment by binary search in the LDS prefix), so the stores are coalesced.  (One block
// per list took 0.18 ms per call at 64 samples in flight — 2.5 % of a C2 step.)
constexpr uint32_t kTableBlocks = 32;
__global__ void __launch_bounds__(1024) k_chunk_tables(Segments seg, uint32_t cur, BatchCounters* __restrict__ ctr,
                                                        uint32_t bounce_closest, uint32_t bounce_shadow, uint32_t do_shadow) {
  if (blockIdx.y == 2) {
    // ---- the order in which k_shade's waves take the segments of the closest-hit queue: LONGEST FIRST.  A segment is one wave's sequential work
    //      there; with the plain segment order the chip waited 10 % (C3) to 14 % (C2) of every k_shade launch — 15-29 % from bounce 3 on, where the
    //      segments differ by an order of magnitude — for the waves that had drawn a long segment last (r6, -DPT_TAIL_PROBE).  Key: the time k_shade
    //      measured for this segment at this bounce in the PREVIOUS batch of the render (same camera, same scene: the same work), else the
    //      segment's size.  A counting sort over 240 logarithmic classes (5 bits of exponent, 3 of mantissa); the order inside a class is whatever
    //      the atomics make it — no result depends on the order in which segments are shaded.
    if (blockIdx.x != 0) return;
    const uint32_t* __restrict__ cnt = seg.active[cur];
    const uint32_t* __restrict__ cost = seg.shade_cost + (size_t)bounce_closest * seg.nseg;
    __shared__ uint32_t hist[256];
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    auto size_class = [&](uint32_t w) {
      const uint32_t c = cost[w], v = c ? c : cnt[w];
      const uint32_t e = 31u - (uint32_t)__builtin_clz(v | 8u);
      return 255u - (v < 8u ? v : (e - 2u) * 8u + ((v >> (e - 3u)) & 7u));
    };
    for (uint32_t w = threadIdx.x; w < seg.nseg; w += 1024) atomicAdd(&hist[size_class(w)], 1u);
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t run = 0; for (int b = 0; b < 256; b++) { const uint32_t h = hist[b]; hist[b] = run; run += h; } }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < seg.nseg; w += 1024) seg.shade_order[atomicAdd(&hist[size_class(w)], 1u)] = w;
    return;
  }
  const bool sh = blockIdx.y == 1;
  if (sh && !do_shadow) return;
  const uint32_t* __restrict__ counts = sh ? seg.shadow : seg.active[cur];
  uint32_t* __restrict__ table = sh ? seg.table_shadow : seg.table_closest;
  __shared__ uint32_t part[1024];
  __shared__ uint32_t base_sh;
  const uint32_t slice = (seg.nseg + kTableBlocks - 1) / kTableBlocks;  // segments per block (<= 1024 for nseg <= 32768)
  const uint32_t w_begin = blockIdx.x * slice;
  const uint32_t w_end = w_begin + slice < seg.nseg ? w_begin + slice : seg.nseg;
  // base = chunks of all segments before this slice; the last block also learns the grand total
  uint32_t before = 0, total = 0;
  for (uint32_t w = threadIdx.x; w < seg.nseg; w += 1024) {
    const uint32_t nc = (counts[w] + 63u) / 64u;
    total += nc;
    if (w < w_begin) before += nc;
  }
  part[threadIdx.x] = before;
  __syncthreads();
  for (uint32_t off = 512; off > 0; off >>= 1) { if (threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off]; __syncthreads(); }
  if (threadIdx.x == 0) base_sh = part[0];
  __syncthreads();
  if (blockIdx.x == kTableBlocks - 1) {
    part[threadIdx.x] = total;
    __syncthreads();
    for (uint32_t off = 512; off > 0; off >>= 1) { if (threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off]; __syncthreads(); }
    if (threadIdx.x == 0) {
      if (sh) ctr->chunks_shadow[bounce_shadow] = part[0];
      else ctr->chunks_closest[bounce_closest] = part[0];
    }
    __syncthreads();
  }
  // inclusive scan of this slice's per-segment chunk counts (thread t <-> segment w_begin + t)
  __shared__ uint32_t rays_of[1024];   // rays of segment w_begin + t: an entry carries its chunk's ray count, so that the trace waves need no second look-up
  const uint32_t mine_n = (w_begin + threadIdx.x < w_end) ? counts[w_begin + threadIdx.x] : 0u;
  rays_of[threadIdx.x] = mine_n;
  const uint32_t mine = (mine_n + 63u) / 64u;
  part[threadIdx.x] = mine;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {  // Hillis-Steele
    const uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  const uint32_t n_entries = part[1023];
  const uint32_t base = base_sh;
  for (uint32_t e = threadIdx.x; e < n_entries; e += 1024) {
    // first t with inclusive prefix part[t] > e
    uint32_t lo = 0, hi = 1023;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (part[mid] > e) hi = mid; else lo = mid + 1; }
    const uint32_t k = e - (lo ? part[lo - 1] : 0u);
    const uint32_t left = rays_of[lo] - k * 64u;   // >= 1: only non-empty chunks are listed
    table[base + e] = chunk_entry(w_begin + lo, k, left < 64u ? left : 64u);
  }
}

// ---- raygen ------------------------------------------------------------------------------------------------------
// Segment s = T consecutive tiles under all samples of the batch.  One wave iteration emits 64 camera rays; lanes outside the image (partial
// edge tiles) are squeezed out.  r4: the 64 rays of an iteration are consecutive SAMPLES OF ONE PIXEL (pixel-major, sample-minor through
// the tile) where r1-r3 emitted one sample of the tile's 64 pixels.  The samples of a pixel differ by a sub-pixel
// jitter, so the lanes of a bounce-0 chunk walk the same nodes and test the same triangles: their loads fall on the same addresses (one
// L1 look-up instead of 64), they finish together, and their hits shade one triangle of one material.  Nothing else knows the order of a
// segment's entries: a path finds its radiance entry through `pid`, which is computed here from (tile, pixel, sample).
__global__ void __launch_bounds__(kBlock) k_raygen(DeviceScene S, PathState st, vec4* __restrict__ Lbuf, Segments seg,
                                                    BatchCounters* __restrict__ ctr, uint32_t first_sample,
                                                    uint32_t nsamples, uint32_t tilesX, uint32_t tilesY) {
  const uint32_t lane = wave_lane();
  const uint32_t tiles = tilesX * tilesY;
  uint32_t started = 0;
  for (uint32_t sg = wave_index(); sg < seg.nseg; sg += wave_count()) {
    uint32_t n_out = 0;
    const uint32_t first_tile = segment_first_tile(seg, sg);
    for (uint32_t k = 0; k < seg.tiles_per_seg * nsamples; k++) {
      const uint32_t tile = first_tile + k / nsamples;
      if (tile >= tiles) break;  // wave-uniform
      const uint32_t r = (k % nsamples) * 64u + lane;   // ray r of the tile's 64 * nsamples, pixel-major
      const uint32_t pl = r / nsamples, s = r - pl * nsamples;
      const PixelXY q = tile_pixel(tile, pl, tilesX);
      const bool valid = q.x < S.width && q.y < S.height;
      RayGenOut rg;
      if (valid) rg = stage_raygen(S, q.x, q.y, first_sample + s);
      const unsigned long long m = __ballot(valid);
      if (valid) {
        const uint32_t j = seg_slot(seg.nseg, sg, n_out + wave_prefix(m));
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

// Tile-adaptive sampling: k_raygen over the VIRTUAL tiles 0 .. *active_count - 1, the still active tiles of the render; virtual tile v
// is image tile active[v] (an ascending list).  Lbuf, the segments and the pids are dense over virtual tiles: only the pixel position
// of a ray looks the list up, and segments past the active count emit nothing.  (A kernel of its own: as one template with k_raygen,
// the merged k_raygen missed the speed margin set for it: profiles/HISTORY.md §10.)  A pixel starts a path when it lies in `rect`: the
// whole frame, or the render region, whose border tiles leave the Lbuf entries of their pixels outside it unwritten.
__global__ void __launch_bounds__(kBlock) k_raygen_adaptive(DeviceScene S, PathState st, vec4* __restrict__ Lbuf, Segments seg,
                                                             uint32_t first_sample, uint32_t nsamples, uint32_t tilesX, Rect rect,
                                                             const uint32_t* __restrict__ active, const uint32_t* __restrict__ active_count) {
  const uint32_t lane = wave_lane();
  const uint32_t tiles = *active_count;   // virtual tiles
  uint32_t started = 0;
  for (uint32_t sg = wave_index(); sg < seg.nseg; sg += wave_count()) {
    uint32_t n_out = 0;
    const uint32_t first_tile = segment_first_tile(seg, sg);
    for (uint32_t k = 0; k < seg.tiles_per_seg * nsamples; k++) {
      const uint32_t tile = first_tile + k / nsamples;
      if (tile >= tiles) break;  // wave-uniform
      const uint32_t r = (k % nsamples) * 64u + lane;
      const uint32_t pl = r / nsamples, s = r - pl * nsamples;
      const PixelXY q = tile_pixel(active[tile], pl, tilesX);   // of the image tile
      const bool valid = rect_contains(rect, q.x, q.y);
      RayGenOut rg;
      if (valid) rg = stage_raygen(S, q.x, q.y, first_sample + s);
      const unsigned long long m = __ballot(valid);
      if (valid) {
        const uint32_t j = seg_slot(seg.nseg, sg, n_out + wave_prefix(m));
        const uint32_t pid = lbuf_index(tile, s, nsamples, pl);
        const uint32_t rel = pid - first_tile * nsamples * 64u;
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

// ---- camera rays from per-pixel leaf lists (pt_camlist.h; built once per render by camera_lists.hip) --------------------------------------
// Bounce 0 of a full-frame render batch of a pinhole camera over the 6-wide one-BVH structure.  A camera ray's candidates are known before it
// exists: its pixel's list names every node with a leaf child the pixel's cone can touch, nearest first.  A ray runs ITS OWN slab test
// (node6_slabs: the walk's arithmetic) against the leaf children each entry names and trav_leaf on those that pass, until an entry lies beyond
// best.t * kCamCullSlack.  So a triangle is tested iff its leaf child passes this ray's slab test, as in the walk; what differs is the order
// in which candidates lower best.t, against which the list trace culls with a wider margin than the walk (kCamCullSlack, pt_camlist.h).  No
// node stack, no leaf queue, no LDS; the next entry's node is fetched while the current one's triangles are tested.  The hit[] record is
// k_trace_closest's.  Pixels flagged kCamWalk are left to k_trace_closest_unlisted.

// the ordinary traversal for the camera rays of the pixels flagged kCamWalk (launched only when the build flagged any), from the chunk table
// k_chunk_tables makes of the queue k_camera_primary filled.  Its claims run on a cursor of its own (work_closest[63]: bounces stop at 50):
// k_camera_primary has used up bounce 0's for its work units
constexpr uint32_t kUnlistedCursor = 63;
__global__ void __launch_bounds__(Walk6::kThreads, Walk6::kClosestBlocksPerCu)
k_trace_closest_unlisted(DeviceScene S, PathState st, vec4* __restrict__ hit, Segments seg, BatchCounters* __restrict__ ctr, uint32_t* __restrict__ spill,
                         CameraLists cl) {
  trace_closest_body<Walk6, false, true>(S, st, hit, seg, 0u, ctr, 0u, &ctr->work_closest[kUnlistedCursor], spill, nullptr, 0u, cl);
}

// ---- bounce 0 in one kernel: camera rays generated and traced from their pixels' lists -----------------------------------------------------
// The list trace needs no stack, no leaf queue and no LDS, and the wave that generates 64 samples of a pixel knows the pixel: it goes
// straight to that pixel's list with the ray in registers.  What k_raygen would leave in memory (rayO, rayD, att, Lbuf, the segment's count
// and poison flag, paths / closest of WaveStats) is written word for word, to the same slots, and hit[] beside it: the ray is never read
// back, and the state stores drain while the trace waits for its nodes.  k_chunk_tables still runs behind it (shade_order, and the table
// k_trace_closest_unlisted claims from).
//
// Work units: a segment costs k_raygen the same everywhere, here its cost follows the list lengths.  A unit is PT_PRIMARY_UNIT consecutive wave
// iterations of a segment, claimed from bounce 0's cursor (work_closest[0]: nothing else uses it in this path); where a unit's first ray lands
// in the segment is a closed form (pt_layout.h camera_rays_before), so units need nothing from one another.  The unit that starts a segment
// writes its count.
//
// One pixel per iteration: when the 64 rays of an iteration are samples of ONE pixel (always when the batch's sample count is a multiple of
// 64), the list, its entries and their nodes are the same for all lanes; only best.t, the cull decision and the leaf masks are per lane.  The
// wave then walks the list with a wave-uniform index (cam_trace_wave: entry, node and triangle records are fetched once per wave, from
// addresses the compiler can prove uniform) and leaves when no lane's cull test passes.  Per lane the entries, the children and the
// triangles come in cam_trace_list's order, so the bits are those of the per-lane loop, which iterations that straddle two pixels still take.
#ifndef PT_PRIMARY_WAVES
#define PT_PRIMARY_WAVES 6
#endif
#ifndef PT_PRIMARY_UNIT
#define PT_PRIMARY_UNIT 16
#endif
constexpr uint32_t kPrimaryUnit = PT_PRIMARY_UNIT;

// (`on`: this lane holds a ray.  len, list and nodes are wave-uniform.)
__device__ __forceinline__ void cam_trace_wave(const DeviceScene& S, TravState& ts, bool on, const BvhNode6* __restrict__ nodes,
                                               const CamListEntry* __restrict__ list, uint32_t len) {
  const CamListEntry none{0u, kInf};
  // two entries ahead, one node ahead: entry i + 1 has arrived when entry i's slab tests free the node registers
  CamListEntry e = len ? list[0] : none, e1 = len > 1u ? list[1] : none;
  BvhNode6 n = nodes[e.ref >> 6];
  for (uint32_t i = 0; i < len; i++) {
    const CamListEntry e2 = i + 2u < len ? list[i + 2u] : none;
    const float lim = ts.best.t * kCamCullSlack;
    on = on && !(e.dist > lim);   // (dist rises and best.t falls along the list: a lane that has left stays out, as after cam_trace_list's break)
    if (__ballot(on) == 0) break;
    uint32_t m = 0;
    if (on) m = node6_leaf_hits(n, ts, lim) & e.ref & 63u;
    const uint32_t base_leaf = n.base_leaf;
    n = nodes[e1.ref >> 6];
    uint32_t any = 0;   // the children some lane still has to test: a wave-uniform mask
#pragma unroll
    for (uint32_t r = 0; r < 6u; r++) any |= __ballot((m >> r) & 1u) != 0 ? 1u << r : 0u;
    while (any) {   // children in rising order for every lane, one wave-uniform leaf at a time
      const uint32_t r = (uint32_t)__builtin_ctz(any);
      any &= any - 1u;
      bool fin = false;
      if ((m >> r) & 1u) trav_leaf(S, ts, kLeafBit | (base_leaf + r), false, &fin, nullptr);
    }
    e = e1; e1 = e2;
  }
}

// ONE_PIXEL: the batch's sample count is a multiple of 64, every iteration is one pixel and the wave walks its list together; otherwise every
// ray walks its own pixel's list (cam_trace_ray, pt_camlist.h).  Two instantiations, chosen per batch by launch_camera_primary: with both
// walks in one kernel the allocator spilled 46 registers into the entry and triangle loops, apart the wave walk needs no scratch at all.
template <bool ONE_PIXEL>
__global__ void __launch_bounds__(kBlock, PT_PRIMARY_WAVES)
k_camera_primary(DeviceScene S, PathState st, vec4* __restrict__ Lbuf, vec4* __restrict__ hit, Segments seg, BatchCounters* __restrict__ ctr,
                 uint32_t first_sample, uint32_t nsamples, uint32_t tilesX, uint32_t tilesY, const CamListEntry* __restrict__ cl_entries,
                 const uint32_t* __restrict__ cl_count, uint32_t cl_cap, const BvhNode6* __restrict__ nodes) {
  PT_TAIL_BEGIN
  const uint32_t bounce = 0;
  (void)bounce;
  const uint32_t lane = wave_lane();
  const uint32_t tiles = tilesX * tilesY;
  const uint32_t seg_iters = seg.tiles_per_seg * nsamples;                     // wave iterations of a segment (k_raygen's k)
  const uint32_t seg_units = (seg_iters + kPrimaryUnit - 1u) / kPrimaryUnit;
  const uint32_t units = seg.nseg * seg_units;
  uint32_t started = 0;
  for (;;) {
    PT_TAIL_MARK
    uint32_t u = 0;
    if (lane == 0) u = atomicAdd(&ctr->work_closest[0], 1u);
    u = __builtin_amdgcn_readfirstlane(u);
    PT_TAIL_T(tail_take)
    if (u >= units) break;
    const uint32_t sg = u / seg_units, k0 = (u - sg * seg_units) * kPrimaryUnit;
    const uint32_t k1 = k0 + kPrimaryUnit < seg_iters ? k0 + kPrimaryUnit : seg_iters;
    const uint32_t first_tile = segment_first_tile(seg, sg);
    if (k0 == 0u && lane == 0) {
      seg.active[0][sg] = camera_rays_before(first_tile, seg_iters, nsamples, tilesX, tiles, S.width, S.height);
      seg.poison[sg] = 0u;
    }
    const uint32_t n_first = camera_rays_before(first_tile, k0, nsamples, tilesX, tiles, S.width, S.height);
    uint32_t n_out = n_first;
    for (uint32_t k = k0; k < k1; k++) {
      const uint32_t tile = first_tile + k / nsamples;
      if (tile >= tiles) break;  // wave-uniform
      const uint32_t r0 = (k % nsamples) * 64u, r = r0 + lane;   // ray r of the tile's 64 * nsamples, pixel-major
      const uint32_t pl = r / nsamples, s = r - pl * nsamples;
      const PixelXY q = tile_pixel(tile, pl, tilesX);
      const bool valid = q.x < S.width && q.y < S.height;
      RayGenOut rg;
      if (valid) rg = stage_raygen(S, q.x, q.y, first_sample + s);
      const unsigned long long m = __ballot(valid);
      uint32_t j = 0;
      if (valid) {
        j = seg_slot(seg.nseg, sg, n_out + wave_prefix(m));
        const uint32_t pid = lbuf_index(tile, s, nsamples, pl);
        const uint32_t rel = pid - first_tile * nsamples * 64u;  // relative to the segment's window (segment_lbuf_base)
        st.rayO[j] = vec4{rg.o.x, rg.o.y, rg.o.z, 0.0f};
        st.rayD[j] = vec4{rg.d.x, rg.d.y, rg.d.z, u2f((rg.dim & kMetaDimMask) | (rel << kMetaPidShift))};
        st.att[j] = vec4{1.0f, 1.0f, 1.0f, u2f(rg.offset)};
        Lbuf[pid] = vec4{0.0f, 0.0f, 0.0f, 1.0f};
      }
      n_out += (uint32_t)__popcll(m);
      if (m == 0) continue;
      // ---- the list trace of these rays ----
      // a ray's list: that of its pixel's slot (pixel_slot_of_pid of its pid); a count of kCamWalk leaves the pixel to k_trace_closest_unlisted
      if constexpr (ONE_PIXEL) {
        const uint32_t qs = tile * 64u + r0 / nsamples;
        const uint32_t len = __builtin_amdgcn_readfirstlane(cl_count[qs]);
        if (len == kCamWalk) continue;
        TravState ts;
        if (valid) {
          float ir = 0.0f;  // alpha-test payload, as in k_trace_closest
          if (S.has_alpha) ir = Halton{halton_table(S.halton), rg.offset, rg.dim & kMetaDimMask}.sample1d();
          (void)trav_init(S, ts, rg.o, rg.d, 1e-3f, kInf, ir, TraversalStack{}, false, nullptr);   // (lists exist only over a tree whose root is a node)
        }
        cam_trace_wave(S, ts, valid, nodes, cl_entries + (size_t)qs * cl_cap, len);
        if (valid) {
          const RayHit& h = ts.best;
          hit[j] = vec4{h.t, h.u, h.v, u2f(hit_word(h))};
        }
      } else if (valid) {
        const uint32_t qs = tile * 64u + pl;
        const uint32_t len = cl_count[qs];
        if (len != kCamWalk) {
          float ir = 0.0f;
          if (S.has_alpha) ir = Halton{halton_table(S.halton), rg.offset, rg.dim & kMetaDimMask}.sample1d();
          TravState ts;
          (void)trav_init(S, ts, rg.o, rg.d, 1e-3f, kInf, ir, TraversalStack{}, false, nullptr);
          cam_trace_ray(S, ts, nodes, cl_entries + (size_t)qs * cl_cap, len);
          const RayHit& h = ts.best;
          hit[j] = vec4{h.t, h.u, h.v, u2f(hit_word(h))};
        }
      }
    }
    started += n_out - n_first;
  }
  if (lane == 0) {
    WaveStats& ws = seg.stats[wave_index()];
    ws.paths += started;
    ws.closest += started;
  }
  PT_TAIL_END(0)
}

// ---- shade -----------------------------------------------------------------------------------------------------------
// Persistent grid sized for the kernel's occupancy (launch_shade); wave w shades segments w, w + P, ...
// Per block, once: the read-mostly tables every hit touches are staged in LDS — the Halton entries of the dimensions
// this bounce can reach (5 + 7b .. 15 + 12b: raygen consumes 4, every bounce 7 to 12), the area-light table (binary
// search + one record per NEE sample) and the E_avg / E_ms_avg energy tables.
// Per hit: geometry + material (NEE's draws run under their gathers), the light sample, then the BSDF set-up and the NEE
// eval on energy-table taps that were all issued together (wo's and the light direction's: one round trip instead of four),
// the shadow record compacted into the shadow queue right away, then the BSDF sample / throughput / roulette and the
// compaction of the survivor.  NEE before the sample (each random number is addressed by its dimension, so the order does
// not matter) means the shadow record is not held in registers across the sampling code.
#ifndef PT_SHADE_WAVES
#define PT_SHADE_WAVES 4   // waves per SIMD the kernel is compiled for (128 VGPRs at most; its row in tests/test_kernel_resources.py)
#endif
#ifndef PT_SHADE_BLOCK
#define PT_SHADE_BLOCK 256
#endif
constexpr uint32_t kShadeBlock = PT_SHADE_BLOCK;
constexpr uint32_t kShadeHalton = 128;  // staged Halton window (entries); dimensions beyond it are read from HBM
constexpr uint32_t kShadeLights = 64;   // staged area lights; a bigger table is read from HBM
constexpr int kLutE = 128, kLutEavg = 128, kLutEavgMs = 32, kLut3 = 32;  // table shapes (checked by load_luts); kLut3: EMs, ETransIn, ETransOut
constexpr uint32_t kBinCap = 128;       // a bin is emptied as soon as it holds 64 entries, and a scan step adds at most 64

__global__ void __launch_bounds__(PT_SHADE_BLOCK, (PT_SHADE_WAVES * 4 * 64) / PT_SHADE_BLOCK)
k_shade(const DeviceScene* __restrict__ Sp, PathState sin, PathState sout, const vec4* __restrict__ hit, ShadowQueue sq,
        vec4* __restrict__ Lbuf, Segments seg, uint32_t cur, BatchCounters* __restrict__ ctr, uint32_t bounce) {
  PT_TAIL_BEGIN
  const DeviceScene& S = *Sp;  // scene table read through the scalar cache: by value it cost 100 spilled SGPRs here
  __shared__ HaltonEntry lds_halton[kShadeHalton];
  __shared__ LightRec lds_lights[kShadeLights];
  __shared__ float lds_Eavg[kLutEavg];
  __shared__ float lds_EavgMs[kLutEavgMs * kLutEavgMs];
  static_assert(kMaxSegmentSlots <= 65536, "slot numbers inside a segment are binned as uint16_t (queue_plan.h bounds seg_cap)");
  __shared__ uint16_t lds_bins[kShadeBlock / 64][5][kBinCap];  // per wave: slot numbers by material class (+ misses), 1.25 KB
  __shared__ uint32_t lds_bin_tri[kShadeBlock / 64][5][kBinCap]; // ... and the triangle hit there: the pass starts its ShadeRec load with the state gather
  const uint32_t halton_base = 5u + 7u * bounce;
  uint32_t halton_count = 11u + 5u * bounce;
  if (halton_base >= (uint32_t)kHaltonDims) halton_count = 0;
  else if (halton_base + halton_count > (uint32_t)kHaltonDims) halton_count = (uint32_t)kHaltonDims - halton_base;
  if (halton_count > kShadeHalton) halton_count = kShadeHalton;
  const bool lights_in_lds = S.lightCount <= kShadeLights;
  {
    const uint4* src = reinterpret_cast<const uint4*>(S.halton + halton_base);
    uint4* dst = reinterpret_cast<uint4*>(lds_halton);
    for (uint32_t i = threadIdx.x; i < halton_count * 2; i += kShadeBlock) dst[i] = ldg(&src[i]);
    if (lights_in_lds) {
      const uint4* ls = reinterpret_cast<const uint4*>(S.light_recs);
      uint4* ld = reinterpret_cast<uint4*>(lds_lights);
      for (uint32_t i = threadIdx.x; i < S.lightCount * (uint32_t)(sizeof(LightRec) / 16); i += kShadeBlock) ld[i] = ldg(&ls[i]);
    }
    for (uint32_t i = threadIdx.x; i < (uint32_t)kLutEavg; i += kShadeBlock) lds_Eavg[i] = ldg(&S.luts.Eavg.d[i]);
    for (uint32_t i = threadIdx.x; i < (uint32_t)(kLutEavgMs * kLutEavgMs); i += kShadeBlock) lds_EavgMs[i] = ldg(&S.luts.EavgMs.d[i]);
  }
  __syncthreads();
  ShadeTables T;
  T.luts.E = Lut{S.luts.E.d, kLutE, kLutE, 1, 0};
  T.luts.Eavg = Lut{lds_Eavg, kLutEavg, 1, 1, 1};
  T.luts.EMs = Lut{S.luts.EMs.d, kLut3, kLut3, kLut3, 0};
  T.luts.EavgMs = Lut{lds_EavgMs, kLutEavgMs, kLutEavgMs, 1, 1};
  T.luts.ETransIn = Lut{S.luts.ETransIn.d, kLut3, kLut3, kLut3, 0};
  T.luts.ETransOut = Lut{S.luts.ETransOut.d, kLut3, kLut3, kLut3, 0};
  T.halton = HaltonTab{S.halton, lds_halton, halton_base, halton_count};
  T.lights = lights_in_lds ? lds_lights : S.light_recs;
  T.light_cdf = S.light_cdf;
  T.lights_lds = lights_in_lds ? 1 : 0;

  const uint32_t lane = wave_lane();
  uint32_t shaded = 0, total_out = 0, total_shadow = 0;
  // first claim = the wave's index; further ones come from a per-launch cursor (segments differ in size by the time the
  // later bounces are reached, so a static deal would leave waves idle at the end of every launch)
  uint32_t claim = wave_index();   // position in seg.shade_order: the segments, longest first (k_chunk_tables)
  uint16_t* bin = &lds_bins[threadIdx.x >> 6][0][0];  // this wave's bins: [class][kBinCap] slot numbers within the segment
  uint32_t* bin_tri = &lds_bin_tri[threadIdx.x >> 6][0][0];
  while (claim < seg.nseg) {
    const uint32_t sg = __builtin_amdgcn_readfirstlane(seg.shade_order[claim]);
    const unsigned long long seg_t0 = wall_clock64();
    const uint32_t lbuf_base = segment_lbuf_base(seg, sg);  // this segment's window of the per-sample radiance buffer
    const uint32_t n = __builtin_amdgcn_readfirstlane(seg.active[cur][sg]);  // (a scalar for the compiler too: the scan loop and the bin counters stay in SGPRs)
    uint32_t n_out = 0, n_shadow = 0;
    // != 0: a path of this segment (paths never leave their segment) carries a throughput with an infinity or a NaN in it
    const uint32_t seg_poisoned = S.env_texture < 0 ? __builtin_amdgcn_readfirstlane(seg.poison[sg]) : 0u;
    unsigned long long poisoned_now = 0;
    // ---- hits are shaded one MATERIAL CLASS per wave pass.  The segment is scanned 64 slots at a time; every slot number goes
    //      to the LDS bin of its hit's class (4 lobe classes + misses); as soon as a bin holds 64 entries they are shaded
    //      together; what is left at the end of the segment is shaded in mixed passes.  (Measured on C3: the same kernel costs
    //      0.092 ns per hit when every sphere is diffuse and 0.126 with the per-instance material mix.)
    uint32_t cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0, cnt4 = 0;  // wave-uniform bin fill levels
    uint32_t k0 = 0;
    for (;;) {
      while (k0 < n && cnt0 < 64 && cnt1 < 64 && cnt2 < 64 && cnt3 < 64 && cnt4 < 64) {
        const uint32_t k = k0 + lane;
        uint32_t cls = 5;  // no entry
        uint32_t w = 0;
        if (k < n) {
          w = f2u(hit[seg_slot(seg.nseg, sg, k)].w);
          cls = hit_word_miss(w) ? 4u : hit_word_class(w);
          // a miss without an environment adds attenuation * backgroundColor = attenuation * 0 (kernel.metal:311 / :541, defs.metal:21):
          // nothing — unless the BSDF has driven the throughput to an infinity or a NaN (a zero pdf), when the reference's sum turns NaN
          // (one in ~1e8 paths: the segment's flag says whether the throughputs of its misses have to be looked at at all)
          if (hit_word_miss(w) && S.env_texture < 0) {
            if (!seg_poisoned) cls = 5u;
            else {
              const vec4 a4 = sin.att[seg_slot(seg.nseg, sg, k)];
              if (!not_finite(v3(a4.x, a4.y, a4.z))) cls = 5u;
            }
          }
        }
        const unsigned long long m0 = __ballot(cls == 0), m1 = __ballot(cls == 1), m2 = __ballot(cls == 2), m3 = __ballot(cls == 3),
                                 m4 = __ballot(cls == 4);
        if (cls < 5) {
          const uint32_t at = cls == 0 ? cnt0 + wave_prefix(m0) : cls == 1 ? cnt1 + wave_prefix(m1) : cls == 2 ? cnt2 + wave_prefix(m2)
                            : cls == 3 ? cnt3 + wave_prefix(m3) : cnt4 + wave_prefix(m4);
          bin[cls * kBinCap + at] = (uint16_t)k;
          bin_tri[cls * kBinCap + at] = hit_word_tri(w);
        }
        cnt0 += (uint32_t)__popcll(m0); cnt1 += (uint32_t)__popcll(m1); cnt2 += (uint32_t)__popcll(m2);
        cnt3 += (uint32_t)__popcll(m3); cnt4 += (uint32_t)__popcll(m4);
        k0 += 64;
      }
      // one pass: a full bin if there is one, else (segment scanned) whatever is left, class by class
      // (the fill levels are only ever named by constant: they stay in scalar registers)
      uint32_t k = kInvalidRef, tri = 0;
      bool is_miss = false;
      const uint32_t full = cnt0 >= 64 ? 0u : cnt1 >= 64 ? 1u : cnt2 >= 64 ? 2u : cnt3 >= 64 ? 3u : cnt4 >= 64 ? 4u : 5u;
      if (full < 5) {
        uint32_t c = 0;
        if (full == 0) c = cnt0 -= 64; else if (full == 1) c = cnt1 -= 64; else if (full == 2) c = cnt2 -= 64;
        else if (full == 3) c = cnt3 -= 64; else c = cnt4 -= 64;
        k = bin[full * kBinCap + c + lane];
        tri = bin_tri[full * kBinCap + c + lane];
        is_miss = full == 4;
      } else {
        if (cnt0 + cnt1 + cnt2 + cnt3 + cnt4 == 0) break;
        // (k0 >= n here) fill the pass from the bins in class order
        uint32_t taken = 0;
#define PT_TAKE_FROM(c, cnt)                                                                                                   \
        {                                                                                                                      \
          const uint32_t take = cnt < 64 - taken ? cnt : 64 - taken;                                                           \
          if (lane >= taken && lane < taken + take) { k = bin[c * kBinCap + cnt - take + (lane - taken)]; tri = bin_tri[c * kBinCap + cnt - take + (lane - taken)]; is_miss = c == 4; }  \
          cnt -= take;                                                                                                         \
          taken += take;                                                                                                       \
        }
        PT_TAKE_FROM(0, cnt0) PT_TAKE_FROM(1, cnt1) PT_TAKE_FROM(2, cnt2) PT_TAKE_FROM(3, cnt3) PT_TAKE_FROM(4, cnt4)
#undef PT_TAKE_FROM
      }
      const bool has = k != kInvalidRef && !is_miss;
      const uint32_t i = seg_slot(seg.nseg, sg, k != kInvalidRef ? k : 0u);
      if (k != kInvalidRef && is_miss) {
        // a miss ends the path; it adds the environment's radiance (kernel.metal:517-539)
        const vec4 o4 = sin.rayO[i];
        const vec4 d4 = sin.rayD[i];
        const vec4 a4 = sin.att[i];
        const vec3 att = v3(a4.x, a4.y, a4.z);
        const uint32_t mpid = lbuf_base + (f2u(d4.w) >> kMetaPidShift);
        vec4 L = Lbuf[mpid];
        if (S.env_texture >= 0) {
          const vec3 Le = stage_miss(S, v3(d4.x, d4.y, d4.z), att, bounce, o4.w, (f2u(d4.w) & kMetaSpecular) != 0);
          L.x += Le.x; L.y += Le.y; L.z += Le.z;
        }
        // L += attenuation * backgroundColor (kernel.metal:311 / :541; backgroundColor = 0): + 0 for a finite throughput, NaN otherwise
        L.x += att.x * 0.0f; L.y += att.y * 0.0f; L.z += att.z * 0.0f;
        Lbuf[mpid] = L;
      }
      uint32_t c_shadow = 0, c_alive = 0;  // written by the lanes inside the divergent region, made wave-uniform after it
      if (has) {
        const vec4 h4 = ld_stream(&hit[i]);
        const vec4 o4 = ld_stream(&sin.rayO[i]);
        const vec4 d4 = ld_stream(&sin.rayD[i]);
        const vec4 a4 = ld_stream(&sin.att[i]);
        const uint32_t meta = f2u(d4.w);
        const uint32_t pid = lbuf_base + (meta >> kMetaPidShift);
        ShadeIn in;
        in.o = v3(o4.x, o4.y, o4.z);
        in.d = v3(d4.x, d4.y, d4.z);
        in.att = v3(a4.x, a4.y, a4.z);
        in.rayO = &sin.rayO[i];
        in.rayD = &sin.rayD[i];
        in.lastSpecular = (meta & kMetaSpecular) != 0;
        in.offset = f2u(a4.w);
        in.dim = (meta & kMetaDimMask) + 1;  // +1: the alpha-test payload `ir` drawn before intersect (kernel.metal:510)
        in.bounce = bounce;
        in.t = h4.x; in.u = h4.y; in.v = h4.z;
        in.tri = tri;
        ShadeGeom g;
        ShadingContext sc;
        // ---- the gathers behind the ShadeRec are started, NEE's three draws (VALU + LDS only) run under them ----
        const ShadeGeomRaw raw = shade_geometry_fetch(S, in);
        const NeeDraws draws = shade_nee_draws(T, in);
        shade_geometry_finish(S, in, raw, g, sc);
        // ---- the light sample first (it needs no table), then the energy-table taps of wo and of the light direction are issued
        //      together and waited for once (pt_shade.h shade_issue / shade_land) ----
        const NeeLight light = shade_nee_light(S, T, in, g, sc, draws);
        BSDF bsdf(sc, S.flags, T.luts);
        const ShadeFlight flight = shade_issue(g, bsdf, light);
        const BSDF::DirTerms light_terms = shade_land(bsdf, flight);
        // ---- NEE; its shadow ray goes to this segment of the shadow queue now (ballot over the lanes in here) ----
        uint32_t dim_rr;
        {
          const NeeOut nee = shade_nee_eval(S, T, in, g, bsdf, light, light_terms);
          dim_rr = nee.dim;
          const unsigned long long m = __ballot(nee.shadow);
          if (nee.shadow) {
            const uint32_t j = seg_slot(seg.nseg, sg, n_shadow + wave_prefix(m));
            st_stream(&sq.o[j], vec4{g.hitPos.x, g.hitPos.y, g.hitPos.z, nee.tmax});
            st_stream(&sq.d[j], vec4{nee.d.x, nee.d.y, nee.d.z, u2f(pid)});
            st_stream(&sq.contrib[j], vec4{nee.contrib.x, nee.contrib.y, nee.contrib.z, nee.payload});
          }
          c_shadow = (uint32_t)__popcll(m);
        }
        // ---- BSDF sample, emission, throughput, roulette; survivors -> this segment of the next bounce's queue ----
        const BounceOut bo = shade_bounce(S, T, in, g, sc, bsdf, dim_rr);
        if (bo.has_emitted) {
          vec4 L = Lbuf[pid];
          L.x += bo.emitted.x; L.y += bo.emitted.y; L.z += bo.emitted.z;
          Lbuf[pid] = L;
        }
        const unsigned long long m = __ballot(bo.alive);
        poisoned_now |= __ballot(bo.alive && not_finite(bo.next_att));
        if (bo.alive) {
          const uint32_t j = seg_slot(seg.nseg, sg, n_out + wave_prefix(m));
          st_stream(&sout.rayO[j], vec4{g.hitPos.x, g.hitPos.y, g.hitPos.z, bo.next_pdf});
          st_stream(&sout.rayD[j], vec4{bo.next_d.x, bo.next_d.y, bo.next_d.z, u2f((bo.dim & kMetaDimMask) | (bo.next_specular ? kMetaSpecular : 0u) | (meta & ~(kMetaDimMask | kMetaSpecular)))});
          st_stream(&sout.att[j], vec4{bo.next_att.x, bo.next_att.y, bo.next_att.z, u2f(in.offset)});
        }
        c_alive = (uint32_t)__popcll(m);
      }
      // the counts of the lanes that were in the region, for every lane (the queue cursors are wave-uniform)
      const unsigned long long mh = __ballot(has);
      if (mh) {
        const int src = __builtin_ctzll(mh);
        n_shadow += (uint32_t)__builtin_amdgcn_readlane((int)c_shadow, src);
        n_out += (uint32_t)__builtin_amdgcn_readlane((int)c_alive, src);
        shaded += (uint32_t)__popcll(mh);
      }
    }
    if (lane == 0) {
      seg.active[cur ^ 1][sg] = n_out;
      seg.shadow[sg] = n_shadow;
      if (poisoned_now) seg.poison[sg] = 1u;
      seg.shade_cost[(size_t)bounce * seg.nseg + sg] = (uint32_t)(wall_clock64() - seg_t0) + 1u;   // the next batch's sort key (k_chunk_tables)
    }
    total_out += n_out;
    total_shadow += n_shadow;
    uint32_t next = 0;
    if (lane == 0) next = wave_count() + atomicAdd(&ctr->work_shade[bounce], 1u);
    claim = __builtin_amdgcn_readfirstlane(next);
  }
  if (lane == 0) {
    WaveStats& ws = seg.stats[wave_index()];
    ws.closest += total_out;
    ws.shadow += total_shadow;
    ws.shaded += shaded;
  }
  PT_TAIL_END(1)
}

// ---- ambient occlusion (any hit; pt_ao.h) ---------------------------------------------------------------------------------
// One AO ray per camera ray, between the camera trace of a render batch and k_shade(0): a consumer of the bounce-0 queue over the shared ray
// loop.  It claims the chunks of bounce 0's closest-hit table (which every branch of the camera trace leaves behind) on a cursor of its own:
// bounces stop at 50 and kUnlistedCursor is 63.  begin reads the queue entry and its hit record: a camera miss writes state 0 and drops
// the ray, a hit becomes stage_ao's ray; finish writes 1 (occluded) or 2 (open).  Reads the queue only, writes Obuf[pid] only (pid as
// walk_bounce0 forms it).  `raylog` (pt_debug_ao, one-sample batches): the AO rays in pixel order, origins then directions log_stride
// pixels apart.  Built and launched at the closest-hit kernel's occupancy: with stage_ao fused into begin it needs that kernel's 80 VGPRs (at the
// shadow kernel's 72 it spilled 10 of them; tests/test_ao_kernel_resources.py holds the bound and the report to each other).
constexpr uint32_t kAoCursor = 62;
template <class W>
__global__ void __launch_bounds__(W::kThreads, W::kClosestBlocksPerCu)
k_trace_ao(DeviceScene S, PathState st, const vec4* __restrict__ hit, Segments seg, BatchCounters* __restrict__ ctr, uint32_t* __restrict__ spill,
           uint32_t* __restrict__ Obuf, float tmax, float* __restrict__ raylog, uint32_t log_stride) {
  uint32_t pid = 0;
  auto begin = [&](uint32_t& ray, TravState& ts, const TraversalStack& stack, TraversalCount* tc) {
    const vec4 d4 = st.rayD[ray];
    const vec4 h4 = hit[ray];
    pid = segment_lbuf_base(seg, slot_segment(seg.nseg, ray)) + (f2u(d4.w) >> kMetaPidShift);
    if (hit_word_miss(f2u(h4.w))) {
      Obuf[pid] = kAoMiss;
      ray = kInvalidRef;
      return false;
    }
    const vec4 o4 = st.rayO[ray];
    const AoRay a = stage_ao(S, v3(o4.x, o4.y, o4.z), v3(d4.x, d4.y, d4.z), h4.x, f2u(h4.w), f2u(st.att[ray].w));
    if (raylog) {
      const size_t p = 3 * (size_t)pixel_of_pid_1spp(pid, S.width);
      float* o = raylog + p;
      float* d = raylog + 3 * (size_t)log_stride + p;
      o[0] = a.o.x; o[1] = a.o.y; o[2] = a.o.z;
      d[0] = a.d.x; d[1] = a.d.y; d[2] = a.d.z;
    }
    return trav_init(S, ts, a.o, a.d, kAoTmin, tmax, a.payload, stack, true, tc);
  };
  auto finish = [&](uint32_t& ray, TravState& ts) {
    Obuf[pid] = ts.best.tri == kInvalidRef ? kAoOpen : kAoOccluded;
    ray = kInvalidRef;
  };
  // (`bounce` only names the tail probe's row: there is none for this launch)
  trace_rays<W, true, false, 2>(S, seg, seg.table_closest, ctr->chunks_closest[0], &ctr->work_closest[kAoCursor], spill, ctr, kAoCursor, nullptr, nullptr,
                                begin, finish);
}

// ---- accumulate (kernel.metal:672-684): running mean, one sample at a time, in sample order --------------------------
// One wave per 8x8 tile (pt_tilefold.h: fold_tile places it, fold_stage turns eight samples of its 64 pixels through LDS per round); every
// lane then folds the samples of ITS pixel in sample order — the running mean is a sequential recurrence per pixel (kernel.metal:672-684).
// ADAPTIVE (k_accumulate_adaptive) also folds the running means of (lum, lum^2) into `mom` with aov_fold / dn_lum (the bits of
// PT_AOV_MOMENTS .g / .b) and sets the tile's sample count; `mom` is null when no checkpoint will read it.
template <bool ADAPTIVE>
__device__ __forceinline__ void accumulate_body(vec4* __restrict__ acc, const vec4* __restrict__ Lbuf, uint32_t npixels, uint32_t width,
                                                uint32_t nsamples, uint32_t n0, uint32_t nonfinite_policy, BatchCounters* __restrict__ ctr,
                                                const uint32_t* __restrict__ active, const uint32_t* __restrict__ active_count,
                                                vec2* __restrict__ mom, uint32_t* __restrict__ tile_n, Rect rect) {
  __shared__ vec4 stage[kBlock / 64][64 * kFoldRow];
  const uint32_t lane = wave_lane(), w = threadIdx.x >> 6;   // (every wave of the block runs the same number of rounds: uniform barriers)
  const FoldTile t = fold_tile<ADAPTIVE>(blockIdx.x * (kBlock / 64) + w, lane, width, npixels / width, active, active_count, rect);
  const bool live = t.live, inside = t.inside;
  const uint32_t p = t.q.y * width + t.q.x;
  vec4 a = inside ? acc[p] : vec4{0.0f, 0.0f, 0.0f, 0.0f};
  vec2 m = ADAPTIVE && inside && mom ? mom[p] : vec2{0.0f, 0.0f};
  for (uint32_t s0 = 0; s0 < nsamples; s0 += 8u) {
    const uint32_t nb = nsamples - s0 < 8u ? nsamples - s0 : 8u;
    __syncthreads();
    if (live) {
#pragma unroll
      for (uint32_t i = 0; i < 8u; i++) {   // fold_stage, written out: through the call this kernel takes 6 more VGPRs (one LDS address per step)
        const uint32_t px = i * 8u + (lane >> 3), j = lane & 7u;
        if (j < nb) stage[w][px * kFoldRow + j] = ld_stream(&Lbuf[lbuf_index(t.tile, s0 + j, nsamples, px)]);
      }
    }
    __syncthreads();
    if (inside) {
      for (uint32_t j = 0; j < nb; j++) {
        const vec4 v = stage[w][lane * kFoldRow + j];
        vec3 L = v3(v.x, v.y, v.z);
        if (not_finite(L)) {
          atomicAdd(&ctr->nonfinite, 1u);
          if (nonfinite_policy == PT_NONFINITE_ZERO) L = v3(0.0f);
        }
        const uint32_t localFrameIdx = n0 + s0 + j;
        if (ADAPTIVE) {
          const float lum = dn_lum(L);
          m = vec2{aov_fold(m.x, lum, localFrameIdx), aov_fold(m.y, lum * lum, localFrameIdx)};
        }
        if (localFrameIdx > 0) {
          L = L + v3(a.x, a.y, a.z) * (float)localFrameIdx;
          L = L / (float)(localFrameIdx + 1);
        }
        a = vec4{L.x, L.y, L.z, 1.0f};
      }
    }
  }
  if (inside) acc[p] = a;
  if (ADAPTIVE) {
    if (inside && mom) mom[p] = m;
    if (live && lane == 0) tile_n[t.itile] = n0 + nsamples;
  }
}

__global__ void __launch_bounds__(kBlock) k_accumulate(vec4* __restrict__ acc, const vec4* __restrict__ Lbuf,
                                                        uint32_t npixels, uint32_t width, uint32_t nsamples, uint32_t n0,
                                                        uint32_t nonfinite_policy, BatchCounters* __restrict__ ctr) {
  accumulate_body<false>(acc, Lbuf, npixels, width, nsamples, n0, nonfinite_policy, ctr, nullptr, nullptr, nullptr, nullptr, Rect{});
}

__global__ void __launch_bounds__(kBlock) k_accumulate_adaptive(vec4* __restrict__ acc, const vec4* __restrict__ Lbuf,
                                                                 uint32_t npixels, uint32_t width, uint32_t nsamples, uint32_t n0,
                                                                 uint32_t nonfinite_policy, BatchCounters* __restrict__ ctr,
                                                                 const uint32_t* __restrict__ active, const uint32_t* __restrict__ active_count,
                                                                 vec2* __restrict__ mom, uint32_t* __restrict__ tile_n, Rect rect) {
  accumulate_body<true>(acc, Lbuf, npixels, width, nsamples, n0, nonfinite_policy, ctr, active, active_count, mom, tile_n, rect);
}

// ---- GMoN ---------------------------------------------------------------------------------------------
// Accumulate into the bucket images exactly as the reference does with RendererFlags_GMoN: sample f goes to bucket
// f / ceil(spp / buckets) (renderer_pt.cpp:124-139) with the running-mean weight n = f / gmonBuckets
// (kernel.metal:675-681 — note: NOT the sample's index inside its bucket; reproduced as is).
__global__ void __launch_bounds__(kBlock) k_accumulate_gmon(vec4* __restrict__ buckets, const vec4* __restrict__ Lbuf,
                                                             uint32_t npixels, uint32_t width, uint32_t nsamples, uint32_t n0,
                                                             uint32_t samples_per_bucket, uint32_t gmon_buckets, uint32_t bucket_base,
                                                             uint32_t nonfinite_policy, BatchCounters* __restrict__ ctr) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= npixels) return;
  const uint32_t l0 = lbuf_index_of_pixel(p, width, 0, nsamples);
  constexpr uint32_t kGroup = 8u;  // (as k_accumulate: one 128-byte line of samples per round of loads)
  vec4 v[kGroup];
  for (uint32_t s = 0; s < nsamples; s++) {
    if (s % kGroup == 0) {
#pragma unroll
      for (uint32_t j = 0; j < kGroup; j++)
        if (s + j < nsamples) v[j] = ld_stream(&Lbuf[l0 + (s + j)]);   // (a pixel's samples are consecutive: lbuf_index)
    }
    vec4 L4 = v[0];
#pragma unroll
    for (uint32_t j = 1; j < kGroup; j++) if (s % kGroup == j) L4 = v[j];
    vec3 L = v3(L4.x, L4.y, L4.z);
    if (not_finite(L)) {
      atomicAdd(&ctr->nonfinite, 1u);
      if (nonfinite_policy == PT_NONFINITE_ZERO) L = v3(0.0f);
    }
    const uint32_t f = n0 + s;
    vec4* acc = buckets + (size_t)(f / samples_per_bucket - bucket_base) * npixels;  // (bucket_base: the buckets[] of a device-group member starts there)
    const uint32_t localFrameIdx = f / gmon_buckets;
    if (localFrameIdx > 0) {
      const vec4 a = acc[p];
      L = L + v3(a.x, a.y, a.z) * (float)localFrameIdx;
      L = L / (float)(localFrameIdx + 1);
    }
    acc[p] = vec4{L.x, L.y, L.z, 1.0f};
  }
}

// shaders/gmon.metal:14-55: per pixel, sort the bucket means by luma (stable bubble sort), Gini coefficient of the
// sorted lumas, drop c = int(min(G, cap) * (n / 2)) values from both ends, average the rest.
__global__ void __launch_bounds__(kBlock) k_gmon(vec4* __restrict__ acc, const vec4* __restrict__ buckets, uint32_t npixels,
                                                  uint32_t nBuckets, float cap) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= npixels) return;
  const vec3 lw = v3(0.2126f, 0.7152f, 0.0722f);  // gmon.metal:10
  vec3 values[32];                                // maxBuckets (gmon.metal:12)
  for (uint32_t i = 0; i < nBuckets; i++) {
    const vec4 b = buckets[(size_t)i * npixels + p];
    values[i] = v3(b.x, b.y, b.z);
  }
  for (uint32_t i = nBuckets; i > 1; i--)
    for (uint32_t j = 1; j < i; j++)
      if (dot(values[j], lw) < dot(values[j - 1], lw)) {
        const vec3 temp = values[j - 1];
        values[j - 1] = values[j];
        values[j] = temp;
      }
  vec3 sum = v3(0.0f), weightedSum = v3(0.0f);
  for (uint32_t i = 0; i < nBuckets; i++) {
    sum = sum + values[i];
    weightedSum = weightedSum + (float)(i + 1) * values[i];
  }
  float G = (2.0f * dot(weightedSum, lw)) / ((float)nBuckets * dot(sum, lw)) - (float)(nBuckets + 1) / (float)nBuckets;
  G = fminf(G, cap);
  // int(G * float(n / 2)); a NaN/negative G (all-black pixel with cap <= 0) keeps every bucket
  const float cf = G * (float)(nBuckets / 2);
  const int c = cf > 0.0f ? (int)cf : 0;
  sum = v3(0.0f);
  for (int i = c; i < (int)nBuckets - c; i++) sum = sum + values[i];
  const vec3 color = sum / (float)((int)nBuckets - 2 * c);
  acc[p] = vec4{color.x, color.y, color.z, 1.0f};
}

// ---- device-group merge (multi_device.hip): weighted sum of the members' running means ------------------------------------
__global__ void __launch_bounds__(kBlock) k_weighted_add(vec4* __restrict__ out, const vec4* __restrict__ in, float w, uint32_t npixels,
                                                          uint32_t first, uint32_t last) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= npixels) return;
  const vec4 a = in[p];
  vec4 o = first ? vec4{0.0f, 0.0f, 0.0f, 0.0f} : out[p];
  o.x += w * a.x; o.y += w * a.y; o.z += w * a.z;
  o.w = last ? 1.0f : 0.0f;
  out[p] = o;
}

// ---- post-process + tonemap -> RGBA8 (pt_post.h) ------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_postprocess(const vec4* __restrict__ acc, uint32_t* __restrict__ rgba8, uint32_t W,
                                                         uint32_t H, PostConstants pc) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= W * H) return;
  const uint32_t py = p / W, px = p - py * W;
  rgba8[p] = pp_pack_rgba8(postprocess_pixel(acc, W, H, px, py, pc));
}

// ---- bookkeeping --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_fold_counters(const BatchCounters* __restrict__ ctr, Totals* __restrict__ tot,
                                                           Segments seg, uint32_t counted) {
  // one block: reduce the per-wave statistics, then clear them for the next batch
  __shared__ unsigned long long red[4][kBlock];
  unsigned long long a[4] = {0, 0, 0, 0};
  for (uint32_t w = threadIdx.x; w < seg.nstats; w += kBlock) {
    WaveStats& ws = seg.stats[w];
    a[0] += ws.closest; a[1] += ws.shadow; a[2] += ws.shaded; a[3] += ws.paths;
    ws.closest = 0; ws.shadow = 0; ws.shaded = 0; ws.paths = 0;
  }
  for (int k = 0; k < 4; k++) red[k][threadIdx.x] = a[k];
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned long long t[4] = {0, 0, 0, 0};
  for (int k = 0; k < 4; k++)
    for (int i = 0; i < kBlock; i++) t[k] += red[k][i];
  if (!counted) {
    tot->closest_rays += t[0];
    tot->shadow_rays += t[1];
    tot->shaded_hits += t[2];
    tot->paths += t[3];
    tot->nonfinite += ctr->nonfinite;
  } else {  // instrumented sample (pt_measure_traversal): only feeds the per-ray fetch averages
    tot->nodes_closest += ctr->nodes_closest; tot->tris_closest += ctr->tris_closest;
    tot->nodes_shadow += ctr->nodes_shadow; tot->tris_shadow += ctr->tris_shadow;
    tot->counted_closest += t[0]; tot->counted_shadow += t[1];
  }
}

// one LightRec per area light (once per render)
__global__ void __launch_bounds__(kBlock) k_light_records(DeviceScene S, LightRec* __restrict__ out, float* __restrict__ cdf) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < S.lightCount) { out[i] = make_light_rec(S, S.lights[i]); cdf[i] = S.lights[i].cumulativePower; }
}

// one ShadeRec per triangle of every leaf slot: entry 2 * slot + half (once per render, after the BVH build)
__global__ void __launch_bounds__(kBlock) k_shade_records(DeviceScene S, ShadeRec* __restrict__ out) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= 2u * S.slot_count) return;
  const TriRec& tr = S.tris[t >> 1];
  const uint32_t gid = (t & 1u) ? tr.gid_b : tr.gid_a;
  if (gid == kInvalidRef) { out[t] = ShadeRec{}; return; }  // the B entry of a one-triangle slot: never referred to
  const uint32_t inst = tr.inst_code & kSlotInstMask;
  out[t] = make_shade_rec(S, inst, (gid >> 2) - S.instances[inst].tri_global_base);
}

// primary-ray records for pt_trace_primary: segment order -> pixel order
__global__ void __launch_bounds__(kBlock) k_hit_records(DeviceScene S, PathState st, const vec4* __restrict__ hit, Segments seg,
                                                         pt_hit_record* __restrict__ out) {
  const uint32_t lane = wave_lane();
  for (uint32_t sg = wave_index(); sg < seg.nseg; sg += wave_count()) {
    const uint32_t n = seg.active[0][sg];
    for (uint32_t k = lane; k < n; k += 64) {
      const uint32_t i = seg_slot(seg.nseg, sg, k);
      const vec4 h = hit[i];
      pt_hit_record r;
      if (!hit_word_miss(f2u(h.w))) {
        r.t = h.x; r.u = h.y; r.v = h.z;
        triangle_ids(S, hit_word_tri(f2u(h.w)), &r.instance, &r.primitive);
      } else {
        r.t = 0.0f; r.u = 0.0f; r.v = 0.0f; r.instance = -1; r.primitive = -1;
      }
      out[pixel_of_pid_1spp(segment_lbuf_base(seg, sg) + (f2u(st.rayD[i].w) >> kMetaPidShift), S.width)] = r;
    }
  }
}

// ---- launchers (host) ---------------------------------------------------------------------------------------------------
void launch_raygen(hipStream_t s, uint32_t grid, const DeviceScene& S, PathState st, vec4* Lbuf, Segments seg, BatchCounters* ctr,
                   uint32_t first_sample, uint32_t nsamples, const TileSet* tiles) {
  if (tiles)
    hipLaunchKernelGGL(k_raygen_adaptive, dim3(grid), dim3(kBlock), 0, s, S, st, Lbuf, seg, first_sample, nsamples, tiles_x(S.width), tiles->rect,
                       tiles->active, tiles->active_count);
  else
    hipLaunchKernelGGL(k_raygen, dim3(grid), dim3(kBlock), 0, s, S, st, Lbuf, seg, ctr, first_sample, nsamples, tiles_x(S.width), tiles_y(S.height));
}
void launch_chunk_tables(hipStream_t s, Segments seg, uint32_t cur, BatchCounters* ctr, uint32_t bounce_closest,
                         uint32_t bounce_shadow, bool do_shadow) {
  hipLaunchKernelGGL(k_chunk_tables, dim3(kTableBlocks, 3), dim3(1024), 0, s, seg, cur, ctr, bounce_closest, bounce_shadow, do_shadow ? 1u : 0u);
}
void launch_camera_primary(hipStream_t s, uint32_t grid, uint32_t grid_unlisted, const DeviceScene& S, PathState st, vec4* Lbuf, vec4* hit, Segments seg,
                           BatchCounters* ctr, uint32_t first_sample, uint32_t nsamples, uint32_t* spill, const CameraLists& cl, bool any_unlisted) {
  const BvhNode6* nodes = reinterpret_cast<const BvhNode6*>(S.nodes);
  if (nsamples % 64u == 0u)
    hipLaunchKernelGGL(k_camera_primary<true>, dim3(grid), dim3(kBlock), 0, s, S, st, Lbuf, hit, seg, ctr, first_sample, nsamples, tiles_x(S.width),
                       tiles_y(S.height), cl.entries, cl.count, cl.cap, nodes);
  else
    hipLaunchKernelGGL(k_camera_primary<false>, dim3(grid), dim3(kBlock), 0, s, S, st, Lbuf, hit, seg, ctr, first_sample, nsamples, tiles_x(S.width),
                       tiles_y(S.height), cl.entries, cl.count, cl.cap, nodes);
  if (any_unlisted) {   // the walk claims from bounce 0's chunk table: the table pass comes first (the caller runs it otherwise)
    launch_chunk_tables(s, seg, 0, ctr, 0, 0, false);
    hipLaunchKernelGGL(k_trace_closest_unlisted, dim3(grid_unlisted), dim3(kBlock), 0, s, S, st, hit, seg, ctr, spill, cl);
  }
}
uint32_t primary_blocks_per_cu() { return PT_PRIMARY_WAVES; }
uint32_t shade_block_threads() { return kShadeBlock; }
uint32_t shade_blocks_per_cu() { return (PT_SHADE_WAVES * 4 * 64) / PT_SHADE_BLOCK; }
void launch_shade(hipStream_t s, uint32_t grid, const DeviceScene* S, PathState sin, PathState sout, const vec4* hit,
                  ShadowQueue sq, vec4* Lbuf, Segments seg, uint32_t cur, BatchCounters* ctr, uint32_t bounce) {
  hipLaunchKernelGGL(k_shade, dim3(grid), dim3(kShadeBlock), 0, s, S, sin, sout, hit, sq, Lbuf, seg, cur, ctr, bounce);
}
void launch_trace_ao(hipStream_t s, uint32_t grid_closest, const DeviceScene& S, PathState st, const vec4* hit, Segments seg, BatchCounters* ctr,
                     uint32_t* spill, uint32_t* Obuf, float distance, float* raylog, uint32_t log_stride) {
  launch_walk(S, false, [&](auto walk, auto) {
    using W = decltype(walk);
    hipLaunchKernelGGL((k_trace_ao<W>), dim3(grid_closest), dim3(W::kThreads), 0, s, S, st, hit, seg, ctr, spill, Obuf, distance, raylog, log_stride);
  });
}
void launch_accumulate(hipStream_t s, vec4* acc, const vec4* Lbuf, uint32_t npixels, uint32_t width, uint32_t nsamples, uint32_t n0,
                       uint32_t nonfinite_policy, BatchCounters* ctr, const TileSet* tiles, vec2* mom, uint32_t* tile_n) {
  // one wave per 8x8 tile of the image, or per tile that may still be active
  const dim3 grid(((tiles ? tiles->max_active : tile_count(width, npixels / width)) + kBlock / 64 - 1) / (kBlock / 64));
  if (tiles)
    hipLaunchKernelGGL(k_accumulate_adaptive, grid, dim3(kBlock), 0, s, acc, Lbuf, npixels, width, nsamples, n0, nonfinite_policy, ctr, tiles->active,
                       tiles->active_count, mom, tile_n, tiles->rect);
  else
    hipLaunchKernelGGL(k_accumulate, grid, dim3(kBlock), 0, s, acc, Lbuf, npixels, width, nsamples, n0, nonfinite_policy, ctr);
}
void launch_accumulate_gmon(hipStream_t s, vec4* buckets, const vec4* Lbuf, uint32_t npixels, uint32_t width, uint32_t nsamples, uint32_t n0,
                            uint32_t samples_per_bucket, uint32_t gmon_buckets, uint32_t bucket_base, uint32_t nonfinite_policy, BatchCounters* ctr) {
  hipLaunchKernelGGL(k_accumulate_gmon, dim3((npixels + kBlock - 1) / kBlock), dim3(kBlock), 0, s, buckets, Lbuf, npixels, width, nsamples, n0,
                     samples_per_bucket, gmon_buckets, bucket_base, nonfinite_policy, ctr);
}
void launch_weighted_add(hipStream_t s, vec4* out, const vec4* in, float w, uint32_t npixels, bool first, bool last) {
  hipLaunchKernelGGL(k_weighted_add, dim3((npixels + kBlock - 1) / kBlock), dim3(kBlock), 0, s, out, in, w, npixels, first ? 1u : 0u, last ? 1u : 0u);
}
void launch_gmon(hipStream_t s, vec4* acc, const vec4* buckets, uint32_t npixels, uint32_t nBuckets, float cap) {
  hipLaunchKernelGGL(k_gmon, dim3((npixels + kBlock - 1) / kBlock), dim3(kBlock), 0, s, acc, buckets, npixels, nBuckets, cap);
}
void launch_postprocess(hipStream_t s, const vec4* acc, uint32_t* rgba8, uint32_t W, uint32_t H, const PostConstants& pc) {
  hipLaunchKernelGGL(k_postprocess, dim3((W * H + kBlock - 1) / kBlock), dim3(kBlock), 0, s, acc, rgba8, W, H, pc);
}
void launch_fold_counters(hipStream_t s, const BatchCounters* ctr, Totals* tot, Segments seg, bool counted) {
  hipLaunchKernelGGL(k_fold_counters, dim3(1), dim3(kBlock), 0, s, ctr, tot, seg, counted ? 1u : 0u);
}
void launch_shade_records(hipStream_t s, const DeviceScene& S, ShadeRec* out) {
  if (S.slot_count) hipLaunchKernelGGL(k_shade_records, dim3((2u * S.slot_count + kBlock - 1) / kBlock), dim3(kBlock), 0, s, S, out);
}
void launch_light_records(hipStream_t s, const DeviceScene& S, LightRec* out, float* cdf) {
  if (S.lightCount) hipLaunchKernelGGL(k_light_records, dim3((S.lightCount + kBlock - 1) / kBlock), dim3(kBlock), 0, s, S, out, cdf);
}
void launch_hit_records(hipStream_t s, uint32_t grid, const DeviceScene& S, PathState st, const vec4* hit, Segments seg,
                        pt_hit_record* out) {
  hipLaunchKernelGGL(k_hit_records, dim3(grid), dim3(kBlock), 0, s, S, st, hit, seg, out);
}

}  // namespace pt
