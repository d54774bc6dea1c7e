// kernels.h — host-visible launchers of the wavefront kernels (kernels.hip, trace_kernels.hip) and the LBVH builder (lbvh.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_camlist.h"
#include "pt_device.h"
#include "pt_layout.h"
#include "pt_post.h"

namespace pt {

struct WaveStats { unsigned long long closest, shadow, shaded, paths; };  // per physical wave, owner-updated, reduced by k_fold_counters

// Queue segments (kernels.hip): segment s = the queue share of `tiles_per_seg` consecutive tiles (pt_layout.h segment_first_tile) under
// all samples of a batch; it owns `seg_cap` slots of every queue array (pt_layout.h seg_slot) and one count per queue.
struct Segments {
  uint32_t* active[2];  // [state buffer][segment] live paths in the segment
  uint32_t* shadow;     // [segment] shadow rays in the segment
  uint32_t* poison;     // [segment] != 0: a path of the segment carries a throughput that is not finite (k_shade's scan of the misses)
  WaveStats* stats;     // [nstats] per physical wave of the producer kernels
  uint32_t* table_closest;  // dense lists of non-empty chunks, chunk_entry(segment, k, rays) (kernels.hip: 16 bits of segment, 10 of k, 6 of rays - 1), rebuilt by k_chunk_tables;
                            // 8 entries of padding behind capacity / 64: a trace wave loads a whole run of up to 8 chunks wherever the list ends
  uint32_t* table_shadow;
  uint32_t* shade_order;    // [nseg] the segments by falling size of the closest-hit queue: the order in which k_shade's waves claim them (k_chunk_tables)
  uint32_t* shade_cost;     // [bounce][nseg] 100 MHz ticks k_shade spent on the segment at that bounce in the PREVIOUS batch of this render (0: none yet)
  uint32_t seg_cap;     // slots per segment (a multiple of 64) = tiles_per_seg * samples_in_flight * 64
  uint32_t nseg;        // segments (<= 32768: k_chunk_tables packs the id into 16 bits and scans <= 1024 per block)
  uint32_t tiles_per_seg;
  uint32_t nsamples;      // samples of the current batch (the per-sample radiance buffer holds nsamples * 64 entries per tile)
  uint32_t bands;         // consecutive segments cycle over this many horizontal bands of the image (nseg % bands == 0)
  uint32_t nstats;      // WaveStats slots (>= waves of the largest producer grid)
  uint32_t refill_threshold; // trace kernels: refill a wave's idle lanes when fewer than this many still hold a ray (0 = only when all idle)
};
PT_HD uint32_t segment_first_tile(const Segments& seg, uint32_t sg) { return segment_first_tile(seg.nseg, seg.bands, seg.tiles_per_seg, sg); }
PT_HD uint32_t segment_lbuf_base(const Segments& seg, uint32_t sg) { return segment_lbuf_base(seg.nseg, seg.bands, seg.tiles_per_seg, seg.nsamples, sg); }
// lane of the wave (wave64); physical wave id / count of the launch (blockDim.x is a multiple of 64)
__device__ __forceinline__ uint32_t wave_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ uint32_t wave_index() { return blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); }
__device__ __forceinline__ uint32_t wave_count() { return gridDim.x * (blockDim.x >> 6); }

// The tiles a batch of an adaptive or region render covers (pt_renderer::tile_set): virtual tile v < *active_count is image tile active[v],
// only the pixels inside `rect` are sampled and folded; max_active >= *active_count (the first list's length) sizes a fold kernel's grid.
// A launcher that takes a `const TileSet*` runs the full-frame kernel when it is null, else the _adaptive one (pt_tilefold.h fold_tile<true>).
struct TileSet { const uint32_t* active; const uint32_t* active_count; uint32_t max_active; Rect rect; };

void launch_raygen(hipStream_t s, uint32_t grid, const DeviceScene& S, PathState st, vec4* Lbuf, Segments seg, BatchCounters* ctr,
                   uint32_t first_sample, uint32_t nsamples, const TileSet* tiles);
// After a producer: list the non-empty chunks of the closest-hit queue (state buffer `cur`, consumed at bounce
// `bounce_closest`) and, if do_shadow, of the shadow queue consumed at `bounce_shadow`.
void launch_chunk_tables(hipStream_t s, Segments seg, uint32_t cur, BatchCounters* ctr, uint32_t bounce_closest,
                         uint32_t bounce_shadow, bool do_shadow);
// What the host has to know of the structure the trace kernels walk (pt_bvh.h Walk4 / Walk6 / WalkTwoLevel, as the kernels were compiled)
struct TraceWalk {
  uint32_t block_threads;
  uint32_t closest_blocks_per_cu;         // k_trace_closest_unlisted and k_trace_ao (kernels.hip)
  uint32_t closest_trace_blocks_per_cu;   // k_trace_closest (trace_kernels.hip: built without SLP packing, one wave per SIMD more)
  uint32_t shadow_blocks_per_cu;
  bool blocks_tunable;         // $PTAMD_CLOSEST_BLOCKS_PER_CU / $PTAMD_SHADOW_BLOCKS_PER_CU apply (not where one block fills a CU's LDS)
  uint32_t pushes_per_level, exit_entries;   // stack entries a tree of L levels needs: L * pushes_per_level + exit_entries
};
TraceWalk trace_walk(bool two_level, bool wide6);
void launch_trace_closest(hipStream_t s, uint32_t grid, const DeviceScene& S, PathState st, vec4* hit, Segments seg, uint32_t cur,
                          BatchCounters* ctr, uint32_t bounce, uint32_t* spill, int32_t* hitlog, uint32_t log_stride, bool count);
// Bounce 0 of a full-frame render batch from the per-pixel leaf lists `cl` (camera_lists.hip) instead of launch_raygen + launch_trace_closest, as
// ONE kernel (k_camera_primary, `grid` blocks, primary_blocks_per_cu() per CU): the camera rays are generated and traced in registers, and every
// word launch_raygen leaves in memory is written as it writes it, with hit[] beside it.  One-BVH 6-wide structure only.  The caller runs the table
// pass behind it — unless the build flagged pixels (any_unlisted): then the table pass and the ordinary traversal for those pixels' rays
// (k_trace_closest_unlisted, `grid_unlisted` blocks as launch_trace_closest takes them), which claims from that table, follow here.
void launch_camera_primary(hipStream_t s, uint32_t grid, uint32_t grid_unlisted, const DeviceScene& S, PathState st, vec4* Lbuf, vec4* hit, Segments seg,
                           BatchCounters* ctr, uint32_t first_sample, uint32_t nsamples, uint32_t* spill, const CameraLists& cl, bool any_unlisted);
uint32_t primary_blocks_per_cu();
// `grid` blocks of shade_block_threads() threads (a persistent grid: shade_blocks_per_cu() per CU keeps it resident)
uint32_t shade_block_threads();
uint32_t shade_blocks_per_cu();
void launch_shade(hipStream_t s, uint32_t grid, const DeviceScene* S_device, PathState sin, PathState sout, const vec4* hit,
                  ShadowQueue sq, vec4* Lbuf, Segments seg, uint32_t cur, BatchCounters* ctr, uint32_t bounce);
void launch_trace_shadow(hipStream_t s, uint32_t grid, const DeviceScene& S, ShadowQueue sq, vec4* Lbuf, Segments seg,
                         BatchCounters* ctr, uint32_t bounce, uint32_t* spill, bool count);
// The AO trace of a render batch (k_trace_ao, pt_ao.h): one any-hit ray of at most `distance` per camera ray of the bounce-0 queue, between the
// camera trace (and its table pass) and k_shade(0); Obuf[pid] = 0 camera miss, 1 occluded, 2 open.  `grid_closest`: the closest-hit
// kernel's persistent grid, whose occupancy the kernel is built for.  raylog (may be null; one-sample batches): 2 * 3 * log_stride floats, the AO rays'
// origins then directions in pixel order.
void launch_trace_ao(hipStream_t s, uint32_t grid_closest, const DeviceScene& S, PathState st, const vec4* hit, Segments seg, BatchCounters* ctr,
                     uint32_t* spill, uint32_t* Obuf, float distance, float* raylog, uint32_t log_stride);
// Over a tile set it also folds the per-pixel running means of (lum, lum^2) into `mom` (unless null) and writes n0 + nsamples to
// tile_n[image tile]; a full-frame batch reads neither.
void launch_accumulate(hipStream_t s, vec4* acc, const vec4* Lbuf, uint32_t npixels, uint32_t width, uint32_t nsamples, uint32_t n0,
                       uint32_t nonfinite_policy, BatchCounters* ctr, const TileSet* tiles, vec2* mom, uint32_t* tile_n);
void launch_accumulate_gmon(hipStream_t s, vec4* buckets, const vec4* Lbuf, uint32_t npixels, uint32_t width, uint32_t nsamples, uint32_t n0,
                            uint32_t samples_per_bucket, uint32_t gmon_buckets, uint32_t bucket_base, uint32_t nonfinite_policy, BatchCounters* ctr);
// out[p] = (first ? 0 : out[p]) + w * in[p]  — merging the accumulators of a device group's members (alpha is set to 1 by the last call)
void launch_weighted_add(hipStream_t s, vec4* out, const vec4* in, float w, uint32_t npixels, bool first, bool last);
void launch_gmon(hipStream_t s, vec4* acc, const vec4* buckets, uint32_t npixels, uint32_t nBuckets, float cap);
void launch_postprocess(hipStream_t s, const vec4* acc, uint32_t* rgba8, uint32_t W, uint32_t H, const PostConstants& pc);
void launch_fold_counters(hipStream_t s, const BatchCounters* ctr, Totals* tot, Segments seg, bool counted);
void launch_shade_records(hipStream_t s, const DeviceScene& S, ShadeRec* out);
void launch_light_records(hipStream_t s, const DeviceScene& S, LightRec* out, float* cdf);
void launch_hit_records(hipStream_t s, uint32_t grid, const DeviceScene& S, PathState st, const vec4* hit, Segments seg,
                        pt_hit_record* out);

// ---- LBVH (lbvh.hip) ----
struct LbvhResult {
  BvhNode* nodes = nullptr;   // node_count records, the root first
  TriRec* tris = nullptr;     // slot_count leaf slots: in leaf order (one BVH: one or two triangles each), in flattening order (two-level: one each)
  uint32_t slot_count = 0;
  MeshTrav* mesh_trav = nullptr;  // two-level only: one record per mesh
  uint32_t root_ref = kInvalidRef;
  uint32_t node_count = 0;    // 4-wide nodes emitted
  uint32_t max_depth = 0;     // of the binary tree
  uint32_t depth4 = 0;        // levels of the tree (the traversal stack needs <= 3 entries per level; 5 when wide6)
  bool wide6 = false;         // nodes[] holds BvhNode6 records (pt_device.h)
};
// The builder's temporaries: ONE device allocation that is kept between builds and only ever grows (a hipFree is a device synchronisation
// and took ~0.2 ms of a 2.2 ms build; C3 needs ~0.4 GB).  Owned by the renderer and given back with it; release() may be called any number of times.
struct LbvhScratch {
  char* base = nullptr;
  size_t cap = 0;
  LbvhScratch() = default;
  LbvhScratch(const LbvhScratch&) = delete;
  LbvhScratch& operator=(const LbvhScratch&) = delete;
  ~LbvhScratch() { release(); }
  hipError_t ensure(size_t bytes);
  void release();
};
// How the flattened triangles are grouped into leaf slots (host_scene.h build_primitives; device copies).  prim_tri == nullptr: one triangle
// per slot, slot = flattened triangle index.
struct PrimTables { const uint32_t* prim_tri = nullptr; const uint32_t* mesh_prim_base = nullptr; const uint32_t* inst_prim_base = nullptr; uint32_t slot_count = 0; };
// Flattens the instanced scene to world-space triangles and builds the BVH entirely on the device.
// `S` needs positions / indices / meshes / instances filled in. Returns hipSuccess or the failing HIP error.
hipError_t build_lbvh(hipStream_t s, const DeviceScene& S, const PrimTables& prims, uint32_t instance_count, uint32_t stack_capacity,
                      LbvhScratch* scratch, LbvhResult* out);
// The two-level structure: a TLAS over the instances' world boxes + one object-space BLAS per mesh, in one node array
// (depth4 = TLAS levels + deepest BLAS levels; the traversal stack also holds one exit marker).  `meshes` is the host copy
// of S.meshes (mesh_count entries).
hipError_t build_two_level(hipStream_t s, const DeviceScene& S, const MeshInfo* meshes, uint32_t mesh_count, uint32_t instance_count,
                           uint32_t tri_count, uint32_t stack_capacity, LbvhScratch* scratch, LbvhResult* out);

}  // namespace pt
