// renderer_state.h — private state of one `pt_renderer`, shared by renderer.hip (the single-device driver of the path tracer),
// display.hip (everything between an HDR image and the RGBA8 render target) and multi_device.hip (the C ABI, and the device group that
// shards samples over several renderers).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "host_scene.h"
#include "adaptive.h"
#include "ao.h"
#include "bloom.h"
#include "camera_lists.h"
#include "denoise.h"
#include "exposure.h"
#include "math_probe.h"
#include "film.h"
#include "matte.h"
#include "projection.h"
#include "pt_math_probe.h"
#include "selection.h"
#include "sky.h"
#include "view.h"
#include "kernels.h"
#include "pt_bvh.h"

using namespace pt;

int pt_fail(int code, const std::string& msg);          // records the message for pt_last_error() (thread-local), returns code
const std::string& pt_last_error_string();
inline int fail(int code, const std::string& msg) { return pt_fail(code, msg); }

namespace {

#define PT_HIP(call)                                                                                       \
  do {                                                                                                     \
    hipError_t e_ = (call);                                                                                \
    if (e_ != hipSuccess) {                                                                                \
      char buf_[512];                                                                                      \
      snprintf(buf_, sizeof(buf_), "%s:%d: %s failed: %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
      return fail(e_ == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_HIP, buf_);                     \
    }                                                                                                      \
  } while (0)

// A device array that KEEPS its allocation across pt_start_render calls: the frontend restarts the render on every camera or scene
// edit (renderer_pt.cpp:199-217 makes startRender cheap), and releasing + re-allocating the ~53 GB of path queues took 1.3-1.5 s per
// restart on MI355X (hipFree of multi-GB buffers unmaps them; measured r03) against 12 ms for everything else.  alloc() only goes back
// to the driver when the array has to GROW; the memory is returned in pt_destroy.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;    // elements in use
  size_t cap = 0;  // elements allocated
  hipError_t alloc(size_t count) {
    if (count <= cap) { n = count; return hipSuccess; }
    release();
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * count);
    if (e != hipSuccess) { p = nullptr; return e; }
    n = cap = count;
    return hipSuccess;
  }
  size_t bytes_held() const { return cap * sizeof(T); }
  hipError_t upload(const std::vector<T>& v) {
    hipError_t e = alloc(v.size());
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = cap = 0;
  }
  ~DevBuf() { release(); }
};

// (K_AO_TRACE, K_AO_FOLD: the ambient-occlusion pass, reported by pt_get_ao_stats alone; the five classes of pt_stats keep their meaning)
enum KernelClass { K_RAYGEN = 0, K_CLOSEST, K_SHADE, K_SHADOW, K_ACCUM, K_AO_TRACE, K_AO_FOLD, K_CLASSES };

struct TimedLaunch { int cls; hipEvent_t start, stop; };

}  // namespace

struct pt_renderer {
  int device = 0;
  int num_cu = 256;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;

  // create-time tables
  DevBuf<float> lut_data;
  LutSet luts{};
  uint32_t lut_w_E = 0, lut_w_Eavg = 0;
  DevBuf<HaltonEntry> halton;

  // scene (valid after pt_start_render)
  bool started = false;
  DevBuf<pt_float3> positions;
  DevBuf<pt_vertex_data> vdata;
  DevBuf<uint32_t> indices, slots;
  DevBuf<MeshInfo> meshes;
  DevBuf<InstanceInfo> instances;
  DevBuf<pt_material_gpu> materials;
  DevBuf<pt_area_light> lights_d;
  std::vector<pt_area_light> lights;
  DevBuf<DeviceScene> scene_d;
  DevBuf<ShadeRec> shade_recs;
  DevBuf<LightRec> light_recs;
  DevBuf<float> light_cdf;
  DevBuf<uint32_t> prim_tri_d, mesh_prim_base_d, inst_prim_base_d;  // leaf-slot grouping of the one-BVH structure (host_scene.h build_primitives)
  DevBuf<InstanceTrav> inst_trav;   // two-level structure only
  bool two_level = false;
  int two_level_override = -1;      // $PTAMD_TWO_LEVEL: 0 / 1 force the choice, -1 = by instancing factor
  DevBuf<uint8_t> tex_data;           // all textures in their own formats (host_scene.h decode_textures)
  DevBuf<float> tex_decode;           // the 8-bit decode tables
  DevBuf<TexInfo> textures;
  DevBuf<pt_alias_entry> env_alias_d;
  std::vector<pt_alias_entry> env_alias;
  LbvhResult bvh{};
  LbvhScratch bvh_scratch{};  // the builder's temporaries, kept between builds
  DeviceScene S{};
  pt_render_params params{};
  pt_constants constants{};
  uint32_t instance_count = 0, tri_count = 0, slot_count = 0;

  // wavefront buffers
  uint32_t samples_in_flight = 0;
  size_t capacity = 0;  // path slots
  DevBuf<vec4> st_rayO[2], st_rayD[2], st_att[2], hit, sq_o, sq_d, sq_c, Lbuf, acc_own;
  DevBuf<uint32_t> spill, seg_active[2], seg_shadow, seg_poison;
  DevBuf<WaveStats> wave_stats;
  DevBuf<uint32_t> chunk_table[2];
  DevBuf<uint32_t> shade_order, shade_cost;
  DevBuf<vec4> gmon_buckets_d;  // [bucket][pixel] with PT_FLAG_GMON (renderer_pt.cpp:824-830)
  float gmon_cap = 1.0f;        // GmonOptions.cap (pt_shader_defs.hpp:164-166)
  pt_post_options post{};
  pt_tonemap_options tonemap{};
  DevBuf<uint32_t> render_target;  // RGBA8 (renderer_pt.cpp:832-835)
  // first-hit AOVs + denoiser (denoise.hip): only a render started with denoise.enabled allocates or launches any of it
  pt_denoise_options denoise{};
  pt_despeckle_options despeckle{};  // the firefly clamp ahead of the filter, read by every enqueue_denoise
  bool aov = false;                 // this render accumulates AOVs
  DevBuf<vec4> Abuf;                // 2 vec4 per Lbuf entry: {albedo, t}, {normal, hit}
  DevBuf<vec4> aov_img;             // [PT_AOV_*][pixel] running means
  DevBuf<vec4> dn_guide, dn_aux, dn_col[2], denoised;  // the filter's per-pixel buffers and its output
  // ID mattes (matte.hip): only a render started with matte_opts.enabled allocates or launches any of it
  pt_matte_options matte_opts{};
  bool matte = false;               // this render keeps mattes
  DevBuf<MatteIds> Mbuf;            // {instance, material} of the first hit per Lbuf entry
  DevBuf<uint4> matte_slots;        // [pixel][layer][slot] {id, count}: kMattePixelVec4 uint4 per pixel
  DevBuf<uint32_t> matte_ids;       // pt_read_matte: the caller's id set, sorted
  DevBuf<float> matte_cov;          // pt_read_matte: the coverage image
  std::vector<uint32_t> material_base;  // [instance] index of its first material in the flattened table (pt_pick decodes with it)
  // selection overlay (selection.hip): nothing is allocated or launched until a target of a render that keeps mattes is read
  // with selection.enabled and a set that is not empty.  The set and both arrays outlive pt_start_render; the arrays are the overlay's own
  // (not matte_ids / matte_cov), so a pt_read_matte between a present and its consumption cannot disturb what the present draws.
  pt_selection_options selection{};
  std::vector<uint32_t> sel_set;    // pt_set_selection: the ids, sorted and without duplicates
  DevBuf<uint32_t> sel_ids;         // sel_set on the device
  DevBuf<float> sel_cov;            // the set's coverage image: what k_selection_overlay reads
  // transparent film (film.hip): only a render started with film_opts.enabled allocates or launches any of it; the composed
  // source only once a target of such a render is read under a backdrop other than PT_BACKDROP_SCENE
  pt_film_options film_opts{};
  bool film = false;                // this render keeps a film
  DevBuf<uint32_t> Fbuf;            // 1: the camera ray hit, 0: it missed, per Lbuf entry
  DevBuf<vec4> film_img;            // [pixel] {premultiplied foreground, coverage} running means
  DevBuf<vec4> film_src;            // the film over the backdrop: what the display chain starts from
  // ambient occlusion (k_trace_ao in kernels.hip, ao.hip): only a render started with ao_opts.enabled allocates or launches any of it
  pt_ao_options ao_opts{};
  bool ao = false;                  // this render keeps AO counts
  float ao_distance = 1.0f;         // of this render (ao_opts is what the NEXT start reads)
  DevBuf<uint32_t> Obuf;            // 0: the camera ray missed, 1: hit and AO ray occluded, 2: hit and AO ray open, per Lbuf entry
  DevBuf<uint2> ao_counts;          // [pixel] {hits, open}
  // camera projection (projection.hip): proj_opts is what pt_set_camera_projection holds for the NEXT start; proj and the constants
  // derived from it and the snapshot's camera belong to the current render.  Under PT_PROJ_PERSPECTIVE nothing of projection.hip is launched.
  pt_camera_projection proj_opts{};
  pt_camera_projection proj{};
  ProjectionConstants proj_constants{};
  // pass views (view.hip): nothing is allocated or launched under PT_VIEW_BEAUTY.  The record (the depth view's range) is
  // allocated by the first target read under DEPTH with auto_range, or the first pt_read_view_stats, and outlives pt_start_render like exp_rec.
  pt_view_options view_opts{};
  DevBuf<ViewRecord> view_rec;      // [1] what k_view_range found: read by k_view_pass on the device, never through the host
  // auto exposure (exposure.hip): nothing is allocated or launched until a target is read with exposure.enabled, or the
  // meter is read.  The record holds the previous ev, so it outlives pt_start_render like the other arrays.
  pt_exposure_options exposure{};
  DevBuf<ExposureRecord> exp_rec;   // [1] the meter record and the smoothing state
  DevBuf<vec4> exp_img;             // the frame * gain: what k_postprocess reads with exposure.enabled
  // bloom (bloom.hip): nothing is allocated or launched until a target is read with bloom.enabled.  Both arrays are sized
  // for the frame on use and outlive pt_start_render like the other arrays.
  pt_bloom_options bloom{};
  DevBuf<vec4> bloom_pyr;           // the levels 1..L of the pyramid, back to back (pt_plan_bloom)
  DevBuf<vec4> bloom_img;           // the bloomed frame: what k_postprocess reads with bloom.enabled
  // tile-adaptive sampling (adaptive.hip): only a render started with adaptive_opts.enabled allocates or launches any of it
  pt_adaptive_options adaptive_opts{};
  bool adaptive = false;            // this render samples adaptively
  DevBuf<uint32_t> ad_list[2];      // the active tiles, ascending; [ad_cur] is the current list, the other one the next checkpoint's
  DevBuf<uint32_t> ad_count;        // [2] the lists' lengths (device-side: batches read the current one)
  DevBuf<uint32_t> ad_tile_n;       // [tile] samples folded into the tile's pixels
  DevBuf<vec2> ad_mom;              // [pixel] running means of (lum, lum^2)
  DevBuf<uint8_t> ad_flags, ad_scratch;  // the checkpoint's per-tile verdicts, the compaction's scratch
  uint32_t* ad_host_count = nullptr;     // pinned: the active count after the newest checkpoint enqueued
  hipEvent_t ad_event = nullptr;         // recorded behind the copy to ad_host_count
  bool ad_event_valid = false;
  int ad_cur = 0;
  uint32_t ad_next = 0;                  // the next checkpoint's sample count (>= total: none left)
  // render region: a render started with region_opts.enabled samples the pixels of `rect` only.  It runs through the
  // virtual-tile path of adaptive sampling (`vtiles`): the first active list holds the tiles the rectangle touches, and without adaptive
  // sampling it never changes.  ad_list / ad_count / ad_tile_n serve both; ad_mom / ad_flags / ad_scratch only an adaptive render.
  pt_render_region region_opts{};
  bool region = false;              // this render samples a region
  bool vtiles = false;              // adaptive || region: batches address virtual tiles through ad_list
  Rect rect{};                      // what this render samples: the region, or the whole frame
  uint32_t ad_tiles0 = 0;           // length of the first active list: the lists' capacity, the most tiles a batch can cover
  // per-pixel leaf lists of the camera rays (camera_lists.hip): built at pt_start_render for a pinhole camera over the 6-wide one-BVH
  // structure of a full-frame, non-adaptive render (host_scene.h camera_lists_wanted); every other render releases them and traces bounce 0 with
  // k_raygen + k_trace_closest
  DevBuf<CamListEntry> cam_entries;    // [pixel slot][cam_cap]
  DevBuf<uint32_t> cam_count;          // [pixel slot] entries, or kCamWalk
  DevBuf<CamListCounters> cam_counters;
  bool cam_lists = false;              // this render traces bounce 0 of its batches from the lists
  bool no_camera_lists = false;        // $PTAMD_NO_CAMERA_LISTS: never build them (the A/B switch)
  uint32_t cam_cap = 0, cam_cap_override = 0;   // entries per pixel; $PTAMD_TEST_CAMLIST_CAP (tests only: a tiny capacity exercises the kCamWalk path)
  pt_camera_list_stats cam_stats{};
  uint32_t primary_grid = 0;
  TraceWalk walk{};   // of the structure in use (kernels.h trace_walk; set with the build)
  uint32_t closest_grid = 0, closest_trace_grid = 0, shadow_grid = 0, closest_blocks_asked = 0, shadow_blocks_asked = 0;  // persistent trace grids, each sized for its kernel's occupancy (asked: $PTAMD_*_BLOCKS_PER_CU, 0 = unset)
  uint32_t last_batch_ns = 0, last_batch_first = 0;  // the batch Lbuf holds ($PTAMD_DEBUG_PIXEL)
  uint32_t nseg = 0, tiles_per_seg = 1, seg_bands = 4, tiles_per_seg_override = 0, nstats = 0, seg_cap = 0, blocks_per_cu = 6, shade_grid = 0, refill_threshold = 48;
  DevBuf<BatchCounters> ctr;
  DevBuf<Totals> totals;
  vec4* acc = nullptr;
  uint32_t grid = 0;

  // ---- member of a device group (multi_device.hip): where this renderer's samples sit in the whole render ----
  uint32_t gmon_sample_base = 0;   // index of its first sample relative to the render's first sample (GMoN bucket + weight use the global index)
  uint32_t gmon_total_spp = 0;     // spp of the whole render (bucket size = ceil(spp / buckets)); 0 = params.spp
  uint32_t gmon_bucket_base = 0;   // first bucket it owns; its bucket array starts there
  uint32_t gmon_own_buckets = 0;   // buckets it owns; 0 = params.gmon_buckets
  struct DeviceGroup* group = nullptr;  // non-null on the front object of a device group

  // progress (renderer_pt.hpp:168-171).  `accumulated` counts the samples pt_render_step has ACCEPTED (what the reference's
  // m_accumulatedFrames counts: encoded, not finished); `launched` of them are enqueued on the stream, the rest are pending:
  // render() calls that arrive while the GPU is still busy are merged into one batch (renderer.hip flush_pending).
  uint64_t accumulated = 0, total = 0, launched = 0;
  uint32_t batches = 0;                 // batches enqueued since pt_start_render
  hipEvent_t batch_done = nullptr;      // recorded behind the newest batch
  bool batch_done_valid = false;
  std::chrono::steady_clock::time_point render_start;
  uint64_t timer_ms = 0;

  // measurement
  bool profiling = false;
  std::vector<TimedLaunch> timed;
  double ms_class[K_CLASSES] = {};
  uint64_t launches[K_CLASSES] = {};
  double upload_ms = 0, bvh_ms = 0;

  TileSet tile_set() { return TileSet{ad_list[ad_cur].p, ad_count.p + ad_cur, ad_tiles0, rect}; }   // of a render with `vtiles`: the current list
  PathState path_state(int k) { return PathState{st_rayO[k].p, st_rayD[k].p, st_att[k].p}; }
  ShadowQueue shadow_queue() { return ShadowQueue{sq_o.p, sq_d.p, sq_c.p}; }
  Segments segments() { return Segments{{seg_active[0].p, seg_active[1].p}, seg_shadow.p, seg_poison.p, wave_stats.p, chunk_table[0].p, chunk_table[1].p, shade_order.p, shade_cost.p, seg_cap, nseg, tiles_per_seg, /*nsamples: set per batch*/ 0u, seg_bands, nstats, refill_threshold}; }

  // A restart keeps every device array (they are re-filled, and only re-allocated when they must grow); what it drops is the
  // acceleration structure of the previous scene and the "started" state.  The arrays' destructors return the memory (pt_destroy).
  void free_scene() {
    if (bvh.nodes) (void)hipFree(bvh.nodes);
    if (bvh.tris) (void)hipFree(bvh.tris);
    if (bvh.mesh_trav) (void)hipFree(bvh.mesh_trav);
    bvh = LbvhResult{};
    acc = nullptr;
    started = false;
    aov = false;
    matte = false;
    film = false;
    ao = false;
    cam_lists = false;
    adaptive = false;
    region = false;
    vtiles = false;
    ad_event_valid = false;
    last_batch_ns = 0;
  }
  // bytes of path-queue memory this renderer already holds (reused by the next render: they count as free when the batch is sized)
  size_t queue_bytes_held() const {
    size_t b = hit.bytes_held() + sq_o.bytes_held() + sq_d.bytes_held() + sq_c.bytes_held() + Lbuf.bytes_held() + chunk_table[0].bytes_held() + chunk_table[1].bytes_held();
    for (int k = 0; k < 2; k++) b += st_rayO[k].bytes_held() + st_rayD[k].bytes_held() + st_att[k].bytes_held();
    return b;
  }
  void release_camera_lists() { cam_entries.release(); cam_count.release(); cam_lists = false; }
  void release_adaptive() {
    release_checkpoints();
    ad_list[0].release(); ad_list[1].release(); ad_count.release(); ad_tile_n.release();
  }
  // what only the checkpoints of adaptive sampling use (a region render without adaptive sampling holds the lists and counts alone)
  void release_checkpoints() { ad_mom.release(); ad_flags.release(); ad_scratch.release(); }
  void drop_timed() {
    for (auto& t : timed) { (void)hipEventDestroy(t.start); (void)hipEventDestroy(t.stop); }
    timed.clear();
  }
};




// The extern "C" entry points (multi_device.hip) dispatch to the functions below or to the group.

// ---- the driver (renderer.hip): start, batches, waits, and the reads of what the render itself produces ----
int dev_create(const pt_create_info* info, int device_ordinal, pt_renderer** out);
void dev_destroy(pt_renderer* r);
int dev_start_render(pt_renderer* r, const pt_scene_snapshot* scene, const pt_render_params* p);
// what a start refuses for its parameters alone, a device group's (own_streams: a caller stream cannot drive it) and a single device's alike
int validate_start_params(const pt_scene_snapshot* scene, const pt_render_params* p, bool own_streams);
int dev_render_step(pt_renderer* r, uint32_t max_spp);
// enqueues the samples accepted but pending; `all`: every one of them now; `sync_checkpoints`: wait for each adaptive checkpoint enqueued
int flush_pending(pt_renderer* r, bool all, bool sync_checkpoints = false);
int dev_wait(pt_renderer* r);
int dev_status(const pt_renderer* r);
int dev_progress(const pt_renderer* r, uint64_t* accumulated, uint64_t* total);
uint64_t dev_render_time_ms(const pt_renderer* r);
int dev_read_accumulator(pt_renderer* r, float* rgba_out);
int dev_set_gmon_options(pt_renderer* r, const pt_gmon_options* o);
int dev_read_gmon_bucket(pt_renderer* r, uint32_t bucket, float* rgba_out);
void* dev_accumulator_device_ptr(pt_renderer* r);
int dev_get_constants(const pt_renderer* r, pt_constants* out);
int dev_get_lights(const pt_renderer* r, pt_area_light* out, uint32_t capacity, uint32_t* count);
int dev_get_env_alias(const pt_renderer* r, pt_alias_entry* out, uint64_t capacity, uint64_t* count);
int dev_trace_primary(pt_renderer* r, uint32_t sample_idx, pt_hit_record* out);
int dev_debug_sample(pt_renderer* r, uint32_t sample_idx, float* radiance_out, int32_t* hits_out);
int dev_measure_traversal(pt_renderer* r, uint32_t sample_idx);
int dev_set_profiling(pt_renderer* r, int enabled);
int dev_get_stats(pt_renderer* r, pt_stats* out);
int dev_read_aov(pt_renderer* r, uint32_t aov, float* rgba_out);
int dev_debug_math(pt_renderer* r, uint32_t fn, uint32_t n, const void* a, const void* b, void* out0, void* out1);
int dev_generate_sky(pt_renderer* r, const pt_sky_options* o, uint32_t width, uint32_t height, float* rgba_out, pt_sky_stats* stats_out);
int dev_debug_lights(pt_renderer* r, uint32_t fn, uint32_t n, const pt_light_probe_args* args, const void* in, void* out);
int dev_debug_shading(pt_renderer* r, uint32_t n, const void* in, void* out);
int dev_set_adaptive_options(pt_renderer* r, const pt_adaptive_options* o);
int dev_read_sample_counts(pt_renderer* r, uint32_t* out);
int dev_set_render_region(pt_renderer* r, const pt_render_region* o);
int dev_get_camera_list_stats(pt_renderer* r, pt_camera_list_stats* out);
int dev_set_matte_options(pt_renderer* r, const pt_matte_options* o);
int dev_read_matte_slots(pt_renderer* r, uint32_t layer, pt_matte_slot* out);
int dev_read_matte(pt_renderer* r, uint32_t layer, const uint32_t* ids, uint32_t id_count, float* coverage_out);
int dev_pick(pt_renderer* r, uint32_t x, uint32_t y, pt_pick_result* out);
int dev_read_film(pt_renderer* r, float* rgba_out);
int dev_set_ao_options(pt_renderer* r, const pt_ao_options* o);
int dev_read_ao(pt_renderer* r, float* out);
int dev_read_ao_counts(pt_renderer* r, uint32_t* out);
int dev_debug_ao(pt_renderer* r, uint32_t sample_idx, float* origins, float* directions, uint32_t* state);
int dev_get_ao_stats(pt_renderer* r, pt_ao_stats* out);
int dev_set_camera_projection(pt_renderer* r, const pt_camera_projection* p);
int dev_get_camera_projection(pt_renderer* r, pt_camera_projection* out);
int dev_debug_camera_rays(pt_renderer* r, uint32_t sample_idx, float* origins, float* directions);

// ---- display (display.hip): the stages' options, and the chain from an HDR image to the RGBA8 target.  `merged`: a device group's merged
//      image on this renderer's device, which the group has waited for; NULL = the renderer's own image ----
int dev_set_post_options(pt_renderer* r, const pt_post_options* o);
int dev_set_tonemap_options(pt_renderer* r, const pt_tonemap_options* o);
int dev_set_denoise_options(pt_renderer* r, const pt_denoise_options* o);
int dev_set_despeckle_options(pt_renderer* r, const pt_despeckle_options* o);
int dev_set_exposure_options(pt_renderer* r, const pt_exposure_options* o);
int dev_reset_exposure(pt_renderer* r);
int dev_set_bloom_options(pt_renderer* r, const pt_bloom_options* o);
int dev_set_film_options(pt_renderer* r, const pt_film_options* o);
int dev_read_denoised(pt_renderer* r, float* rgba_out);
int dev_read_render_target(pt_renderer* r, const vec4* merged, uint8_t* rgba8_out);                // blocks
int dev_present(pt_renderer* r, const vec4* merged, void** device_rgba8_out, void** stream_out);  // enqueues only
int dev_read_exposure_meter(pt_renderer* r, const vec4* merged, pt_exposure_meter* out);           // blocks; what a target read would meter now
int dev_debug_exposure(pt_renderer* r, const float* rgba, uint32_t width, uint32_t height, const uint32_t* rect, const pt_exposure_options* options,
                       pt_exposure_meter* out, float* scaled_out);
int dev_debug_bloom(pt_renderer* r, const float* rgba, uint32_t width, uint32_t height, const pt_bloom_options* options, float* out, float* pyramid_out);
int dev_set_selection_options(pt_renderer* r, const pt_selection_options* o);
int dev_set_selection(pt_renderer* r, const uint32_t* ids, uint32_t id_count);
int dev_get_selection(const pt_renderer* r, uint32_t* ids_out, uint32_t capacity, uint32_t* count);
int dev_debug_selection_overlay(pt_renderer* r, const uint8_t* rgba8_in, const float* coverage, uint32_t width, uint32_t height,
                                const pt_selection_options* options, uint8_t* rgba8_out);
int dev_set_view_options(pt_renderer* r, const pt_view_options* o);
int dev_read_view_stats(pt_renderer* r, const vec4* merged, pt_view_stats* out);                   // blocks; draws nothing
int dev_debug_view(pt_renderer* r, const pt_view_inputs* in, uint32_t width, uint32_t height, const uint32_t* rect, const pt_view_options* options,
                   uint8_t* rgba8_out, pt_view_stats* stats_out);
