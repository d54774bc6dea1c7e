// renderer.hip — host driver behind the C ABI (include/ptamd.h): the MI355X counterpart of
// `pt::renderer_pt::Renderer` (src/renderer_pt/renderer_pt.{hpp,cpp}).
//
//   pt_create          Renderer::Renderer + loadGgxLutTextures            renderer_pt.cpp:18-60, 385-446
//   pt_start_render    startRender + the rebuild* half of render()         :72-111, 199-217, 448-651, 838-1021
//   pt_render_step     render() steady state                               :113-197
//   pt_status/...      status / renderProgress / renderTime                :1023-1037
//   pt_read_accumulator  (the reference only reads back RGBA8, :1039-1059; the float mean is the parity surface)
//
// This file is the path tracer's driver: start, batches, waits, and the reads of what a render itself produces (accumulator, AOVs, mattes,
// sample counts, statistics).  What turns an HDR image into the RGBA8 render target is display.hip.
//
// No CPU path exists in this library: without a HIP device pt_create fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "queue_plan.h"
#include "runtime_identity.h"
#include "renderer_state.h"
#include "light_probe.h"
#include "pt_light_probe.h"
#include "shade_probe.h"
#include "pt_shade_probe.h"

using namespace pt;

namespace {
thread_local std::string g_last_error;
}
int pt_fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
const std::string& pt_last_error_string() { return g_last_error; }

namespace {

struct ScopedTimer {  // records a pair of events around one launch when profiling is on
  pt_renderer* r;
  int cls;
  hipEvent_t start = nullptr, stop = nullptr;
  ScopedTimer(pt_renderer* r_, int cls_) : r(r_), cls(cls_) {
    if (!r->profiling) return;
    if (hipEventCreate(&start) != hipSuccess || hipEventCreate(&stop) != hipSuccess) { start = stop = nullptr; return; }
    (void)hipEventRecord(start, r->stream);
  }
  ~ScopedTimer() {
    if (!start) return;
    (void)hipEventRecord(stop, r->stream);
    r->timed.push_back({cls, start, stop});
  }
};

// Times a stretch of one stream with a pair of events: the first is recorded on construction (`started` tells whether that worked); stop() records
// the second, waits for it and gives the milliseconds between.  The events go with the object, on every path out of its scope.
struct EventStopwatch {
  hipStream_t s;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t started;
  explicit EventStopwatch(hipStream_t s_) : s(s_) {
    started = hipEventCreate(&e0);
    if (started == hipSuccess) started = hipEventCreate(&e1);
    if (started == hipSuccess) started = hipEventRecord(e0, s);
  }
  hipError_t stop(float* ms) {
    hipError_t e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) (void)hipEventElapsedTime(ms, e0, e1);
    return e;
  }
  ~EventStopwatch() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

// Free device memory now; 0 when the runtime cannot tell.  Every budget of pt_start_render reads 0 as "unknown" and then credits nothing
// (host_scene.h choose_accel_structure, camera_lists_fit, queue_budget).
size_t free_device_bytes() {
  size_t free_b = 0, total_b = 0;
  return hipMemGetInfo(&free_b, &total_b) == hipSuccess ? free_b : 0;
}

enum BatchMode { BATCH_RENDER, BATCH_DEBUG, BATCH_MEASURE };

// The camera rays of a batch into state buffer 0: k_raygen / k_raygen_adaptive under PT_PROJ_PERSPECTIVE, exactly as before the projections;
// under any other kind of this render their counterpart in projection.hip.  Render, debug and measuring batches all come through here.
void launch_camera_raygen(pt_renderer* r, Segments seg, uint32_t first, uint32_t ns, const TileSet* tiles) {
  if (r->proj.kind == PT_PROJ_PERSPECTIVE)
    launch_raygen(r->stream, r->grid, r->S, r->path_state(0), r->Lbuf.p, seg, r->ctr.p, first, ns, tiles);
  else
    launch_raygen_projected(r->stream, r->grid, r->S, r->proj_constants, r->path_state(0), r->Lbuf.p, seg, first, ns, tiles);
}

// One batch: `ns` samples of every pixel, first sample index `first`, `n0` samples already in the accumulator.
int enqueue_batch(pt_renderer* r, uint32_t first, uint32_t ns, uint32_t n0, BatchMode mode, int32_t* hitlog) {
  const DeviceScene& S = r->S;
  hipStream_t s = r->stream;
  BatchCounters* ctr = r->ctr.p;
  // the per-bounce hit log is indexed by pixel through pixel_of_pid_1spp (pt_layout.h): it only exists for one-sample batches
  if (hitlog && ns != 1) return fail(PT_ERR_INVALID_ARGUMENT, "the hit log is kept for one-sample batches only");
  if (ns == 0 || ns > r->samples_in_flight) return fail(PT_ERR_INVALID_ARGUMENT, "batch larger than the queues");
  PT_HIP(hipMemsetAsync(ctr, 0, sizeof(BatchCounters), s));
  const bool count = mode == BATCH_MEASURE;
  Segments seg = r->segments();
  seg.nsamples = ns;
#ifdef PT_DEBUG_PID
  if (const char* e = getenv("PTAMD_DEBUG_RAY")) {  // debug build only: "x,y,sample,bounce" -> the closest-hit kernel prints that ray's traversal
    uint32_t x = 0, y = 0, sm = 0, b = 0;
    if (sscanf(e, "%u,%u,%u,%u", &x, &y, &sm, &b) == 4 && sm >= first && sm < first + ns) {
      const uint32_t v[2] = {lbuf_index(tile_of_pixel(x, y, S.width), sm - first, ns, lane_of_pixel(x, y)), b + 1u};
      PT_HIP(hipMemcpyAsync(&ctr->_pad[0], v, 8, hipMemcpyHostToDevice, s));
    }
  }
#endif
  // an adaptive or region render's batch covers the active tiles only: the kernels that place a tile in the image read the current list,
  // and take the render's rectangle as their validity test (null: the full-frame kernels)
  const bool ad = mode == BATCH_RENDER && r->vtiles;
  const TileSet tile_set = r->tile_set();
  const TileSet* tiles = ad ? &tile_set : nullptr;
  // Bounce 0, the camera rays.  A render batch with lists generates and traces them in one kernel (k_camera_primary), timed as bounce 0's
  // closest-hit launch together with the walk for flagged pixels; the table pass alone is left in the raygen class.  Lists imply a full-frame
  // render (camera_lists_wanted, host_scene.h: no adaptive sampling, no region), so `tiles` is null here.  Every other batch generates them,
  // lists the queue's chunks and walks the tree; the debug and measuring batches always do (the hit log and nodes_per_ray stay what they are).
  if (mode == BATCH_RENDER && r->cam_lists) {
    const bool any_unlisted = r->cam_stats.pixels_walk != 0;
    {
      ScopedTimer t(r, K_CLOSEST);
      launch_camera_primary(s, r->primary_grid, r->closest_grid, S, r->path_state(0), r->Lbuf.p, r->hit.p, seg, ctr, first, ns, r->spill.p,
                            CameraLists{r->cam_entries.p, r->cam_count.p, r->cam_cap}, any_unlisted);
    }
    if (!any_unlisted) {
      ScopedTimer t(r, K_RAYGEN);
      launch_chunk_tables(s, seg, 0, ctr, 0, 0, false);
    }
  } else {
    {
      ScopedTimer t(r, K_RAYGEN);
      launch_camera_raygen(r, seg, first, ns, tiles);
      launch_chunk_tables(s, seg, 0, ctr, 0, 0, false);
    }
    ScopedTimer t(r, K_CLOSEST);
    launch_trace_closest(s, count ? r->closest_grid : r->closest_trace_grid, S, r->path_state(0), r->hit.p, seg, 0u, ctr, 0u, r->spill.p, hitlog, S.width * S.height, count);
  }
  // The first-hit passes of a render batch: the camera rays' hits, read from the queue before k_shade consumes it.
  if (mode == BATCH_RENDER) {
    // first-hit AOVs of a render that keeps them (denoise.hip)
    if (r->aov) launch_aov(s, r->grid, r->scene_d.p, r->path_state(0), r->hit.p, seg, r->Abuf.p);
    // ID mattes of a render that keeps them (matte.hip): the same hits' instance and material, independent of the AOVs (timed with the
    // accumulate class, where its other kernel is: pt_stats.ms_accumulate with mattes on minus off is what mattes cost)
    if (r->matte) {
      ScopedTimer t(r, K_ACCUM);
      launch_matte_ids(s, r->grid, r->scene_d.p, r->path_state(0), r->hit.p, seg, r->Mbuf.p);
    }
    // the film of a render that keeps one (film.hip): which of the same camera rays hit anything (timed with the accumulate class, as the mattes)
    if (r->film) {
      ScopedTimer t(r, K_ACCUM);
      launch_film_flags(s, r->grid, r->path_state(0), r->hit.p, seg, r->Fbuf.p);
    }
    // ambient occlusion of a render that keeps it (k_trace_ao): one any-hit ray from each of the same hits, in a timer class of its own
    if (r->ao) {
      ScopedTimer t(r, K_AO_TRACE);
      launch_trace_ao(s, r->closest_grid, S, r->path_state(0), r->hit.p, seg, ctr, r->spill.p, r->Obuf.p, r->ao_distance, nullptr, 0u);
    }
  }
  // The bounces: bounce b's closest hits (bounce 0's are in hit[] already), k_shade, and the shadow rays it queued.
  int cur = 0;
  const bool mis = S.integrator == PT_INTEGRATOR_MIS;
  for (uint32_t b = 0; b < S.max_bounces; b++) {
    if (b != 0) {
      ScopedTimer t(r, K_CLOSEST);
      launch_trace_closest(s, count ? r->closest_grid : r->closest_trace_grid, S, r->path_state(cur), r->hit.p, seg, (uint32_t)cur, ctr, b, r->spill.p, hitlog, S.width * S.height, count);
    }
    {
      ScopedTimer t(r, K_SHADE);
      launch_shade(s, r->shade_grid, r->scene_d.p, r->path_state(cur), r->path_state(cur ^ 1), r->hit.p, r->shadow_queue(), r->Lbuf.p, seg, (uint32_t)cur, ctr, b);
      // closest-hit list of bounce b + 1 (written to chunks_closest[b + 1]) and shadow list of bounce b
      launch_chunk_tables(s, seg, (uint32_t)(cur ^ 1), ctr, b + 1, b, mis);
    }
    if (mis) {
      ScopedTimer t(r, K_SHADOW);
      launch_trace_shadow(s, r->shadow_grid, S, r->shadow_queue(), r->Lbuf.p, seg, ctr, b, r->spill.p, count);
    }
    cur ^= 1;
  }
  if (mode == BATCH_RENDER) {
    ScopedTimer t(r, K_ACCUM);
    const uint32_t npix = S.width * S.height;
    if (r->params.flags & PT_FLAG_GMON) {
      const uint32_t buckets = r->params.gmon_buckets;
      const uint32_t total_spp = r->gmon_total_spp ? r->gmon_total_spp : r->params.spp;
      const uint32_t spb = (total_spp + buckets - 1) / buckets;  // renderer_pt.cpp:124-125
      const uint32_t f0 = n0 + r->gmon_sample_base;              // (a member of a device group: index within the whole render)
      launch_accumulate_gmon(s, r->gmon_buckets_d.p, r->Lbuf.p, npix, S.width, ns, f0, spb, buckets, r->gmon_bucket_base, r->params.nonfinite_policy, ctr);
      // the reference resolves after every frame with fullBuckets = gmonIdx + 1 (renderer_pt.cpp:164-179); only the last
      // resolve of a batch is observable
      launch_gmon(s, r->acc, r->gmon_buckets_d.p, npix, (f0 + ns - 1) / spb + 1 - r->gmon_bucket_base, r->gmon_cap);
    } else {
      launch_accumulate(s, r->acc, r->Lbuf.p, npix, S.width, ns, n0, r->params.nonfinite_policy, ctr, tiles, r->adaptive ? r->ad_mom.p : nullptr,
                        r->ad_tile_n.p);
    }
    if (r->aov)
      launch_accumulate_aov(s, r->aov_img.p, r->aov_img.p + npix, r->aov_img.p + 2 * (size_t)npix, r->Abuf.p, r->Lbuf.p, S.width, S.height, ns, n0,
                            r->params.nonfinite_policy, tiles);
    if (r->matte) launch_accumulate_matte(s, r->matte_slots.p, r->Mbuf.p, S.width, S.height, ns, tiles);
    if (r->film) launch_accumulate_film(s, r->film_img.p, r->Lbuf.p, r->Fbuf.p, S.width, S.height, ns, n0, r->params.nonfinite_policy, tiles);
  }
  if (mode == BATCH_RENDER && r->ao) {
    ScopedTimer t(r, K_AO_FOLD);
    launch_accumulate_ao(s, r->ao_counts.p, r->Obuf.p, S.width, S.height, ns, tiles);
  }
  // a batch that ends at a checkpoint (flush_pending never lets one straddle it): test the active tiles, compact the list into the other
  // buffer, and send the new count to pinned host memory
  if (ad && r->adaptive && r->ad_next < r->total && n0 + ns == r->ad_next) {
    {
      ScopedTimer t(r, K_ACCUM);
      PT_HIP(launch_adaptive_check(s, tiles->active, tiles->active_count, r->ad_list[r->ad_cur ^ 1].p, r->ad_count.p + (r->ad_cur ^ 1), r->ad_mom.p, S.width, r->rect,
                                   r->ad_tiles0, r->ad_next, r->adaptive_opts.threshold, r->ad_flags.p, r->ad_scratch.p, r->ad_scratch.n,
                                   r->ad_host_count));
    }
    PT_HIP(hipEventRecord(r->ad_event, s));
    r->ad_event_valid = true;
    r->ad_cur ^= 1;
    r->ad_next += r->adaptive_opts.interval;
  }
  // BATCH_DEBUG still folds (to clear the per-wave statistics) but into a scratch Totals slot
  launch_fold_counters(s, ctr, mode == BATCH_DEBUG ? r->totals.p + 1 : r->totals.p, seg, count);
  PT_HIP(hipGetLastError());
  r->last_batch_ns = ns; r->last_batch_first = first;
  return PT_OK;
}

void collect_timings(pt_renderer* r) {
  for (auto& t : r->timed) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) {
      r->ms_class[t.cls] += ms;
      r->launches[t.cls]++;
    }
  }
  r->drop_timed();
}

int load_luts(pt_renderer* r, const uint8_t* b, size_t size) {
  if (size < 12 + 16 * 8 || memcmp(b, "PTLUT01\0", 8) != 0) return fail(PT_ERR_BAD_LUT, "LUT blob: bad magic (expected PTLUT01)");
  uint32_t count;
  memcpy(&count, b + 8, 4);
  if (count != 8) return fail(PT_ERR_BAD_LUT, "LUT blob: expected 8 tables (renderer_pt.hpp:154-165)");
  uint32_t hdr[32];
  memcpy(hdr, b + 12, sizeof(hdr));
  const size_t data_off = 12 + 16 * 8;
  const size_t nfloats = (size - data_off) / 4;
  // expected shapes (renderer_pt.hpp:154-165 + resource/lut): E 128x128, Eavg 128, 3-D 32^3, 2-D avg 32^2
  const uint32_t expect[8][3] = {{128, 128, 1}, {128, 1, 1}, {32, 32, 32}, {32, 32, 1}, {32, 32, 32}, {32, 32, 32}, {32, 32, 1}, {32, 32, 1}};
  for (int i = 0; i < 8; i++) {
    const uint32_t w = hdr[4 * i], h = hdr[4 * i + 1], d = hdr[4 * i + 2], off = hdr[4 * i + 3];
    if (w != expect[i][0] || h != expect[i][1] || d != expect[i][2] || (size_t)off + (size_t)w * h * d > nfloats)
      return fail(PT_ERR_BAD_LUT, "LUT blob: unexpected table shape");
  }
  std::vector<float> data(nfloats);
  memcpy(data.data(), b + data_off, nfloats * 4);
  PT_HIP(r->lut_data.upload(data));
  Lut* ls[6] = {&r->luts.E, &r->luts.Eavg, &r->luts.EMs, &r->luts.EavgMs, &r->luts.ETransIn, &r->luts.ETransOut};
  for (int i = 0; i < 6; i++) {
    ls[i]->w = (int)hdr[4 * i]; ls[i]->h = (int)hdr[4 * i + 1]; ls[i]->depth = (int)hdr[4 * i + 2];
    ls[i]->d = r->lut_data.p + hdr[4 * i + 3];
  }
  r->lut_w_E = hdr[0];
  r->lut_w_Eavg = hdr[4];
  return PT_OK;
}

int build_halton_table(pt_renderer* r) {
  std::vector<HaltonEntry> tab;
  tab.reserve(kHaltonDims);
  for (uint32_t c = 2; (int)tab.size() < kHaltonDims; c++) {  // defs.metal:115-194: the first 620 primes
    bool prime = true;
    for (uint32_t d = 2; d * d <= c; d++)
      if (c % d == 0) { prime = false; break; }
    if (!prime) continue;
    tab.push_back(make_halton_entry(c));
  }
  PT_HIP(r->halton.upload(tab));
  return PT_OK;
}

}  // namespace

extern "C" const char* pt_last_error(void) { return g_last_error.c_str(); }

extern "C" int pt_plan_queues(uint32_t width, uint32_t height, uint32_t spp, uint32_t samples_in_flight, uint64_t free_hbm_bytes,
                              uint32_t tiles_per_seg_override, uint32_t seg_bands, pt_queue_plan* out) {
  if (!out) return fail(PT_ERR_INVALID_ARGUMENT, "pt_plan_queues: null argument");
  const char* why = "";
  const int rc = plan_queues(width, height, spp, samples_in_flight, free_hbm_bytes, tiles_per_seg_override, seg_bands, out, &why);
  return rc == PT_OK ? PT_OK : fail(rc, std::string("pt_plan_queues: ") + why);
}

std::string pt_rccl_bound_path();  // multi_device.hip: "" until RCCL has been loaded

extern "C" int pt_get_runtime_info(pt_runtime_info* out) {
  if (!out) return fail(PT_ERR_INVALID_ARGUMENT, "pt_get_runtime_info: null argument");
  memset(out, 0, sizeof(*out));
  const RuntimeObjects o = mapped_runtime_objects();
  auto put = [](char* dst, size_t cap, const std::string& s) { snprintf(dst, cap, "%s", s.c_str()); };
  put(out->hip_runtime_path, sizeof(out->hip_runtime_path), object_of((const void*)&hipRuntimeGetVersion));
  put(out->hsa_runtime_path, sizeof(out->hsa_runtime_path), o.hsa.empty() ? std::string() : o.hsa[0]);
  put(out->rccl_path, sizeof(out->rccl_path), pt_rccl_bound_path());
  out->hip_runtimes_mapped = (uint32_t)o.hip.size();
  out->hsa_runtimes_mapped = (uint32_t)o.hsa.size();
  out->rccl_mapped = (uint32_t)o.rccl.size();
  int v = 0;
  out->hip_runtime_version = hipRuntimeGetVersion(&v) == hipSuccess ? v : 0;
  put(out->all_mapped, sizeof(out->all_mapped), join_paths(o.hip) + " | " + join_paths(o.hsa) + " | " + join_paths(o.rccl));
  return PT_OK;
}

int dev_create(const pt_create_info* info, int device_ordinal, pt_renderer** out) {
  if (!info || !out) return fail(PT_ERR_INVALID_ARGUMENT, "pt_create: null argument");
  *out = nullptr;
  if (info->abi_version != PT_ABI_VERSION && info->abi_version != 4u) return fail(PT_ERR_INVALID_ARGUMENT, "pt_create: ABI version mismatch");
  {  // one HIP runtime over one HSA runtime per process, or whoever initialises second sees no GPU (runtime_identity.h)
    const std::string conflict = runtime_conflict();
    if (!conflict.empty()) return fail(PT_ERR_RUNTIME_CONFLICT, "pt_create: " + conflict);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(PT_ERR_NO_DEVICE, "pt_create: no HIP device available (this library has no CPU fallback)");
  if (device_ordinal < 0 || device_ordinal >= ndev) return fail(PT_ERR_INVALID_ARGUMENT, "pt_create: bad device ordinal");
  PT_HIP(hipSetDevice(device_ordinal));
  auto* r = new pt_renderer();
  pt_default_post_options(&r->post);
  pt_default_tonemap_options(&r->tonemap);
  pt_default_denoise_options(&r->denoise);
  pt_default_despeckle_options(&r->despeckle);
  pt_default_exposure_options(&r->exposure);
  pt_default_bloom_options(&r->bloom);
  pt_default_adaptive_options(&r->adaptive_opts);
  pt_default_render_region(&r->region_opts);
  pt_default_matte_options(&r->matte_opts);
  pt_default_selection_options(&r->selection);
  pt_default_film_options(&r->film_opts);
  pt_default_ao_options(&r->ao_opts);
  pt_default_camera_projection(&r->proj_opts);
  r->proj = r->proj_opts;
  pt_default_view_options(&r->view_opts);
  r->device = device_ordinal;
  if (const char* e = getenv("PTAMD_REFILL")) r->refill_threshold = (uint32_t)atoi(e);
  if (const char* e = getenv("PTAMD_TILES_PER_SEG")) r->tiles_per_seg_override = (uint32_t)std::max(0, atoi(e));  // tuning knobs
  if (const char* e = getenv("PTAMD_SEG_BANDS")) r->seg_bands = (uint32_t)std::max(1, std::min(64, atoi(e)));
  if (const char* e = getenv("PTAMD_TWO_LEVEL")) r->two_level_override = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("PTAMD_BLOCKS_PER_CU")) r->blocks_per_cu = (uint32_t)std::max(1, std::min(8, atoi(e)));
  if (const char* e = getenv("PTAMD_CLOSEST_BLOCKS_PER_CU")) r->closest_blocks_asked = (uint32_t)std::max(1, std::min(8, atoi(e)));
  if (const char* e = getenv("PTAMD_NO_CAMERA_LISTS")) r->no_camera_lists = atoi(e) != 0;
  if (const char* e = getenv("PTAMD_TEST_CAMLIST_CAP")) r->cam_cap_override = (uint32_t)std::max(1, std::min((int)kCamListMaxCapacity, atoi(e)));
  if (const char* e = getenv("PTAMD_SHADOW_BLOCKS_PER_CU")) r->shadow_blocks_asked = (uint32_t)std::max(1, std::min(8, atoi(e)));
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, r->device) == hipSuccess) r->num_cu = prop.multiProcessorCount;
  int rc = PT_OK;
  do {
    if (hipStreamCreateWithFlags(&r->own_stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(PT_ERR_HIP, "hipStreamCreate failed"); break; }
    r->stream = r->own_stream;
    if (hipEventCreateWithFlags(&r->batch_done, hipEventDisableTiming) != hipSuccess) { rc = fail(PT_ERR_HIP, "hipEventCreate failed"); break; }
    std::vector<uint8_t> file;
    const uint8_t* blob = (const uint8_t*)info->lut_blob;
    size_t size = (size_t)info->lut_blob_size;
    if (!blob) {
      const char* path = info->lut_path ? info->lut_path : getenv("PTAMD_LUT_PATH");
      if (!path) { rc = fail(PT_ERR_BAD_LUT, "pt_create: no LUT blob, lut_path or $PTAMD_LUT_PATH"); break; }
      FILE* f = fopen(path, "rb");
      if (!f) { rc = fail(PT_ERR_BAD_LUT, std::string("pt_create: cannot open LUT file ") + path); break; }
      fseek(f, 0, SEEK_END);
      long n = ftell(f);
      fseek(f, 0, SEEK_SET);
      file.resize((size_t)n);
      if (fread(file.data(), 1, (size_t)n, f) != (size_t)n) { fclose(f); rc = fail(PT_ERR_BAD_LUT, "pt_create: short read on LUT file"); break; }
      fclose(f);
      blob = file.data();
      size = file.size();
    }
    if ((rc = load_luts(r, blob, size)) != PT_OK) break;
    if ((rc = build_halton_table(r)) != PT_OK) break;
    if (r->ctr.alloc(1) != hipSuccess || r->totals.alloc(2) != hipSuccess) { rc = fail(PT_ERR_OUT_OF_MEMORY, "counter allocation failed"); break; }
  } while (0);
  if (rc != PT_OK) { dev_destroy(r); return rc; }
  *out = r;
  return PT_OK;
}

void dev_destroy(pt_renderer* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->stream) (void)hipStreamSynchronize(r->stream);
  r->drop_timed();
  r->free_scene();  // the acceleration structure is raw pointers; every device array and the BVH builder's kept scratch go with `delete r`
  if (r->batch_done) (void)hipEventDestroy(r->batch_done);
  if (r->ad_event) (void)hipEventDestroy(r->ad_event);
  if (r->ad_host_count) (void)hipHostFree(r->ad_host_count);
  if (r->own_stream) (void)hipStreamDestroy(r->own_stream);
  delete r;
}

int validate_start_params(const pt_scene_snapshot* scene, const pt_render_params* p, bool own_streams) {
  if (!scene || !p) return fail(PT_ERR_INVALID_ARGUMENT, "pt_start_render: null argument");
  if (p->width == 0 || p->height == 0 || p->spp == 0) return fail(PT_ERR_INVALID_ARGUMENT, "pt_start_render: empty size or spp");
  if (own_streams && p->stream)
    return fail(PT_ERR_INVALID_ARGUMENT, "pt_start_render: a caller stream cannot drive a device group (every member owns its stream)");
  if (p->max_bounces < 1 || p->max_bounces > 50)
    return fail(PT_ERR_INVALID_ARGUMENT, "pt_start_render: max_bounces must be 1..50 (620 Halton dimensions, kernel.metal:5)");
  if ((uint64_t)p->width * p->height > (1ull << 28)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_start_render: image too large");
  if (p->integrator != PT_INTEGRATOR_SIMPLE && p->integrator != PT_INTEGRATOR_MIS) return fail(PT_ERR_INVALID_ARGUMENT, "bad integrator");
  if (p->nonfinite_policy > PT_NONFINITE_ZERO) return fail(PT_ERR_INVALID_ARGUMENT, "bad nonfinite_policy");
  if (p->accel_structure > PT_ACCEL_TWO_LEVEL) return fail(PT_ERR_INVALID_ARGUMENT, "bad accel_structure");
  if ((p->flags & PT_FLAG_GMON) && (p->gmon_buckets < 1 || p->gmon_buckets > 32))
    return fail(PT_ERR_INVALID_ARGUMENT, "gmon_buckets must be 1..32 (gmon.metal:12 maxBuckets)");
  if (scene->instance_count && (!scene->instances || !scene->instance_materials || !scene->meshes))
    return fail(PT_ERR_INVALID_ARGUMENT, "pt_start_render: null scene arrays");
  return PT_OK;
}

// ---- pt_start_render, phase by phase (dev_start_render below runs them in this order).  r->S, the HostScene and r->bvh carry the scene from
//      one phase to the next; what a phase needs of the renderer's options (denoise, adaptive, region) it reads there. ----
namespace {

Rect render_rect(const pt_renderer* r, const pt_render_params* p) {
  const pt_render_region& g = r->region_opts;
  return g.enabled ? Rect{g.x0, g.y0, g.x1, g.y1} : Rect{0u, 0u, p->width, p->height};
}

// 1. the parameters, then what this renderer's options rule out
int validate_start(const pt_renderer* r, const pt_scene_snapshot* scene, const pt_render_params* p) {
  if (const int rc = validate_start_params(scene, p, /*own_streams=*/false)) return rc;
  if (r->adaptive_opts.enabled && (p->flags & PT_FLAG_GMON))
    return fail(PT_ERR_UNSUPPORTED, "pt_start_render: adaptive sampling does not support PT_FLAG_GMON (a bucket would have to be resolved per tile count)");
  if (r->region_opts.enabled) {
    const pt_render_region& g = r->region_opts;
    if (g.x1 > p->width || g.y1 > p->height)
      return fail(PT_ERR_INVALID_ARGUMENT, "pt_start_render: the render region [" + std::to_string(g.x0) + ", " + std::to_string(g.x1) + ") x [" +
                                               std::to_string(g.y0) + ", " + std::to_string(g.y1) + ") does not fit the " +
                                               std::to_string(p->width) + " x " + std::to_string(p->height) + " image");
    if (p->flags & PT_FLAG_GMON)
      return fail(PT_ERR_UNSUPPORTED, "pt_start_render: a render region does not support PT_FLAG_GMON (the GMoN kernels index the radiance buffer by image pixel)");
  }
  return PT_OK;
}

// 2a. flatten the snapshot, derive constants and the light table (host_scene.h)
int flatten_scene(pt_renderer* r, const pt_scene_snapshot* scene, const pt_render_params* p, HostScene* hs) {
  std::string err;
  const int rc = build_host_scene(scene, p, r->lut_w_E, r->lut_w_Eavg, hs, &err);
  if (rc != PT_OK) return fail(rc, err);
  if (hs->tri_count >= (1u << 27)) return fail(PT_ERR_UNSUPPORTED, "more than 2^27 flattened triangles (the hit record keeps 28 bits for 2 * leaf slot + half)");
  if (hs->instances.size() >= (1u << kSlotInstBits)) return fail(PT_ERR_UNSUPPORTED, "more than 2^26 instances (a leaf slot keeps 26 bits for the instance)");
  return PT_OK;
}

// 2b. upload it and fill r->S with everything but the acceleration structure and the records
int upload_scene(pt_renderer* r, const pt_render_params* p, HostScene* hs) {
  r->instance_count = (uint32_t)hs->instances.size();
  r->tri_count = hs->tri_count;
  r->constants = hs->constants;
  r->lights = hs->lights;
  const pt_constants& C = r->constants;
  PT_HIP(r->positions.upload(hs->positions));
  PT_HIP(r->vdata.upload(hs->vdata));
  PT_HIP(r->indices.upload(hs->indices));
  PT_HIP(r->slots.upload(hs->slots));
  PT_HIP(r->meshes.upload(hs->meshes));
  PT_HIP(r->instances.upload(hs->instances));
  PT_HIP(r->materials.upload(hs->materials));
  PT_HIP(r->lights_d.upload(r->lights));
  PT_HIP(r->tex_data.upload(hs->tex_data));
  PT_HIP(r->tex_decode.upload(hs->tex_decode));
  PT_HIP(r->textures.upload(hs->textures));
  PT_HIP(r->env_alias_d.upload(hs->env_alias));
  r->env_alias = std::move(hs->env_alias);

  DeviceScene& S = r->S;
  memset(&S, 0, sizeof(S));
  S.positions = r->positions.p; S.vdata = r->vdata.p; S.indices = r->indices.p; S.slots = r->slots.p;
  S.meshes = r->meshes.p; S.instances = r->instances.p; S.materials = r->materials.p; S.lights = r->lights_d.p;
  S.halton = r->halton.p;
  S.luts = r->luts;
  S.camera = C.camera;
  S.idt = hs->idt;
  S.width = p->width; S.height = p->height;
  S.tex_data = r->tex_data.p; S.tex_decode = r->tex_decode.p; S.textures = r->textures.p; S.tex_native = hs->tex_native; S.env_alias = r->env_alias_d.p;
  S.env_texture = hs->env_texture;
  S.envLightCount = C.envLightCount;
  S.has_alpha = hs->has_alpha ? 1u : 0u;
  S.lightCount = C.lightCount;
  S.totalLightPower = C.totalLightPower;
  S.flags = p->flags;
  S.integrator = p->integrator;
  S.max_bounces = p->max_bounces;
  S.tri_count = r->tri_count;
  S.root_ref = kInvalidRef;
  return PT_OK;
}

// 3. the acceleration structure (replaces rebuildAccelerationStructures, renderer_pt.cpp:653-749): which one (host_scene.h
// choose_accel_structure), its build, and its place in r->S
int build_accel(pt_renderer* r, const pt_render_params* p, HostScene* hs) {
  DeviceScene& S = r->S;
  EventStopwatch watch(r->stream);
  PT_HIP(watch.started);
  uint64_t unique_tris = 0;
  for (const MeshInfo& m : hs->meshes) unique_tris += m.tri_count;
  std::vector<InstanceTrav> itrav;
  const bool invertible = instance_trav_records(hs->instances, &itrav);
  const size_t free_b = free_device_bytes();
  const AccelChoice choice = choose_accel_structure(invertible, r->tri_count, unique_tris, free_b, p->accel_structure, r->two_level_override);
  r->two_level = choice.two_level;
  // The switch is not silent: the two structures agree bit for bit except where fp32 Moeller-Trumbore reports a FALSE hit that
  // lies outside an instance's tighter object-space boxes (fuzz seed 310601: one pixel-sample in ~1 500 scenes).
  if (choice.automatic && !getenv("PTAMD_QUIET"))
    fprintf(stderr, "ptamd: PT_ACCEL_AUTO chose the TWO-LEVEL structure (flattening %u triangles would take %.1f GB of the %.1f GB free): 1.75x the "
                    "traversal time of one BVH, and closest hits can differ from it where fp32 Moeller-Trumbore accepts a triangle the ray passes "
                    "outside of (the seed-310601 class: ~1 pixel-sample per 1 500 scenes); PT_ACCEL_ONE_BVH / PT_ACCEL_TWO_LEVEL pin the choice\n",
            r->tri_count, (double)(r->tri_count * kFlatBytesPerTri) / 1e9, (double)free_b / 1e9);
  hipError_t be;
  if (r->two_level) {
    PT_HIP(r->inst_trav.upload(itrav));
    be = build_two_level(r->stream, S, hs->meshes.data(), (uint32_t)hs->meshes.size(), r->instance_count, r->tri_count,
                         (uint32_t)(kLdsStack + kSpillStack), &r->bvh_scratch, &r->bvh);
  } else {
    // leaf slots: two consecutive triangles of a mesh that share an edge go into ONE slot ($PTAMD_NO_PAIRS: one triangle per slot, as r3 had it)
    build_primitives(hs, getenv("PTAMD_NO_PAIRS") == nullptr);
    PT_HIP(r->prim_tri_d.upload(hs->prim_tri));
    PT_HIP(r->mesh_prim_base_d.upload(hs->mesh_prim_base));
    PT_HIP(r->inst_prim_base_d.upload(hs->inst_prim_base));
    PrimTables prims;
    prims.prim_tri = r->prim_tri_d.p; prims.mesh_prim_base = r->mesh_prim_base_d.p; prims.inst_prim_base = r->inst_prim_base_d.p;
    prims.slot_count = hs->prim_count;
    be = build_lbvh(r->stream, S, prims, r->instance_count, (uint32_t)(kLdsStack + kSpillStack), &r->bvh_scratch, &r->bvh);
  }
  if (be != hipSuccess)
    return fail(be == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_HIP, std::string("LBVH build failed: ") + hipGetErrorString(be));
  float ms = 0;
  PT_HIP(watch.stop(&ms));
  r->bvh_ms = ms;
  // traversal stack: <= 3 pushes per 4-wide level (5 per 6-wide one); 4-wide depth = ceil(binary depth / 2)
  r->walk = trace_walk(r->two_level, r->bvh.wide6);
  if (r->bvh.depth4 * r->walk.pushes_per_level + r->walk.exit_entries > (uint32_t)kStackTotal)
    return fail(PT_ERR_UNSUPPORTED, "BVH too deep for the traversal stack (degenerate geometry: thousands of coincident triangles?)");
  S.nodes = r->bvh.nodes;
  S.tris = r->bvh.tris;
  S.slot_count = r->slot_count = r->bvh.slot_count;
  S.root_ref = r->bvh.root_ref;
  S.node_count = r->bvh.node_count;
  S.two_level = r->two_level ? 1u : 0u;
  S.wide6 = r->bvh.wide6 ? 1u : 0u;
  S.inst_trav = r->inst_trav.p;
  S.mesh_trav = r->bvh.mesh_trav;
  return PT_OK;
}

// 4. the shade and light records, then the device copy of r->S, which is complete with them
int build_records(pt_renderer* r) {
  DeviceScene& S = r->S;
  PT_HIP(r->shade_recs.alloc(std::max<size_t>(1, 2 * (size_t)r->slot_count)));  // entry 2 * slot + half
  S.shade_recs = r->shade_recs.p;
  launch_shade_records(r->stream, S, r->shade_recs.p);
  PT_HIP(r->light_recs.alloc(std::max<size_t>(1, r->lights.size())));
  PT_HIP(r->light_cdf.alloc(std::max<size_t>(1, r->lights.size())));
  S.light_recs = r->light_recs.p;
  S.light_cdf = r->light_cdf.p;
  launch_light_records(r->stream, S, r->light_recs.p, r->light_cdf.p);
  PT_HIP(r->scene_d.upload(std::vector<DeviceScene>(1, S)));  // k_shade reads the table from memory (scalar loads)
  return PT_OK;
}

// 5. the per-pixel leaf lists of the camera rays (camera_lists.hip): taken BEFORE the queues are planned, and bounded (host_scene.h
// camera_lists_fit); a render that does not get them gives back those of the previous one
int build_camera_lists(pt_renderer* r, const pt_render_params* p) {
  const DeviceScene& S = r->S;
  r->cam_stats = pt_camera_list_stats{};
  const bool want = camera_lists_projection(r->proj_opts.kind) &&
                    camera_lists_wanted(r->no_camera_lists, r->two_level, r->bvh.wide6, S.root_ref, S.camera.apertureRadius,
                                        r->adaptive_opts.enabled != 0, r->region_opts.enabled != 0);
  const uint32_t cap = r->cam_cap_override ? r->cam_cap_override : kCamListCapacity;
  const size_t slots = (size_t)tile_count(p->width, p->height) * 64;
  const size_t free_b = free_device_bytes();
  if (!want || !camera_lists_fit(camera_list_bytes(p->width, p->height, cap), free_b, r->cam_entries.bytes_held() + r->cam_count.bytes_held())) {
    r->release_camera_lists();
    return PT_OK;
  }
  PT_HIP(r->cam_entries.alloc(slots * cap));
  PT_HIP(r->cam_count.alloc(slots));
  PT_HIP(r->cam_counters.alloc(1));
  PT_HIP(hipMemsetAsync(r->cam_counters.p, 0, sizeof(CamListCounters), r->stream));
  EventStopwatch watch(r->stream);
  PT_HIP(watch.started);
  launch_camera_lists(r->stream, S, r->cam_entries.p, r->cam_count.p, cap, r->cam_counters.p);
  float ms = 0;
  PT_HIP(watch.stop(&ms));
  PT_HIP(hipGetLastError());
  CamListCounters c{};
  PT_HIP(hipMemcpy(&c, r->cam_counters.p, sizeof(c), hipMemcpyDeviceToHost));
  r->cam_cap = cap;
  r->cam_lists = true;
  r->cam_stats.built = 1u;
  r->cam_stats.capacity = cap;
  r->cam_stats.pixels_listed = c.listed;
  r->cam_stats.pixels_walk = c.walk;
  r->cam_stats.entries = c.entries;
  r->cam_stats.build_ms = ms;
  for (uint32_t k = 0; k < kCamHistBins; k++) r->cam_stats.length_histogram[k] = c.hist[k];
  return PT_OK;
}

// 6. the wavefront buffers: the queue plan for the memory at hand (host_scene.h queue_budget, queue_plan.h), the grids, and every array a batch
// of this render touches
int allocate_buffers(pt_renderer* r, const pt_render_params* p) {
  const uint64_t npix = (uint64_t)p->width * p->height;
  const bool aov = r->denoise.enabled != 0;
  if (!aov) { r->Abuf.release(); r->aov_img.release(); }  // (an AOV-off render holds nothing more than before)
  const bool matte = r->matte_opts.enabled != 0;
  if (!matte) { r->Mbuf.release(); r->matte_slots.release(); r->matte_ids.release(); r->matte_cov.release(); }   // (nor does a matte-off render)
  const bool film = r->film_opts.enabled != 0;
  if (!film) { r->Fbuf.release(); r->film_img.release(); r->film_src.release(); }   // (nor a film-off render)
  const bool ao = r->ao_opts.enabled != 0;
  if (!ao) { r->Obuf.release(); r->ao_counts.release(); }   // (nor an AO-off render)
  const bool adaptive = r->adaptive_opts.enabled != 0;
  const bool region = r->region_opts.enabled != 0;
  if (!adaptive) r->release_checkpoints();                  // (nor does an adaptive-off render;
  if (!adaptive && !region) r->release_adaptive();          //  a region render keeps the tile lists and counts, which both use)
  // Queue segments (kernels.hip): one per 8x8 tile (a few tiles each once the image has more than 32640 of them), each with
  // room for its tiles under all samples in flight; queue_plan.h holds the sizing and every index-width limit.  The producers
  // (raygen, shade) are persistent grids whose waves take segments round-robin; the trace kernels claim chunks from a table,
  // so every grid is sized for its own kernel's occupancy.
  {
    const uint64_t budget = queue_budget(free_device_bytes(), r->queue_bytes_held(), r->cam_entries.bytes_held() + r->cam_count.bytes_held(), aov,
                                         r->Abuf.bytes_held(), matte, r->Mbuf.bytes_held(), film, r->Fbuf.bytes_held(), ao, r->Obuf.bytes_held());
    pt_queue_plan plan{};
    const char* why = "";
    const int rc = plan_queues(p->width, p->height, p->spp, p->samples_in_flight, budget, r->tiles_per_seg_override, r->seg_bands, &plan, &why);
    if (rc != PT_OK) return fail(rc, std::string("pt_start_render: ") + why);
    r->samples_in_flight = plan.samples_in_flight;
    r->tiles_per_seg = plan.tiles_per_seg;
    r->nseg = plan.nseg;
    r->seg_cap = plan.seg_cap;
    r->capacity = (size_t)plan.capacity;
  }
  const uint32_t sif = r->samples_in_flight;
  r->grid = (uint32_t)r->num_cu * r->blocks_per_cu;                 // raygen, hit records: 256-thread blocks
  r->shade_grid = (uint32_t)r->num_cu * shade_blocks_per_cu();     // as many blocks as k_shade's registers / LDS keep resident
  r->primary_grid = (uint32_t)r->num_cu * primary_blocks_per_cu();
  r->closest_grid = (uint32_t)r->num_cu * (r->walk.blocks_tunable && r->closest_blocks_asked ? r->closest_blocks_asked : r->walk.closest_blocks_per_cu);
  // (k_trace_closest's own grid: it is built for one block per CU more than the closest-hit walks of kernels.hip, which keep closest_grid)
  r->closest_trace_grid = (uint32_t)r->num_cu * (r->walk.blocks_tunable && r->closest_blocks_asked ? r->closest_blocks_asked : r->walk.closest_trace_blocks_per_cu);
  r->shadow_grid = (uint32_t)r->num_cu * (r->walk.blocks_tunable && r->shadow_blocks_asked ? r->shadow_blocks_asked : r->walk.shadow_blocks_per_cu);
  r->nstats = std::max(std::max(r->grid, r->primary_grid) * (kBlock / 64), r->shade_grid * (shade_block_threads() / 64));
  for (int k = 0; k < 2; k++) {
    PT_HIP(r->st_rayO[k].alloc(r->capacity)); PT_HIP(r->st_rayD[k].alloc(r->capacity));
    PT_HIP(r->st_att[k].alloc(r->capacity));
  }
  PT_HIP(r->hit.alloc(r->capacity));
  PT_HIP(r->sq_o.alloc(r->capacity)); PT_HIP(r->sq_d.alloc(r->capacity)); PT_HIP(r->sq_c.alloc(r->capacity));
  PT_HIP(r->Lbuf.alloc((size_t)tile_count(p->width, p->height) * 64 * sif));  // tile-major, whole tiles (pt_layout.h lbuf_index)
  for (int k = 0; k < 2; k++) PT_HIP(r->seg_active[k].alloc(r->nseg));
  PT_HIP(r->seg_shadow.alloc(r->nseg));
  PT_HIP(r->seg_poison.alloc(r->nseg));
  PT_HIP(r->wave_stats.alloc(r->nstats));
  for (int k = 0; k < 2; k++) PT_HIP(r->chunk_table[k].alloc(r->capacity / 64 + 8));   // + 8: a trace wave loads the entries of a whole run of up to 8 chunks, wherever the list ends
  PT_HIP(r->shade_order.alloc(r->nseg));
  // (max_bounces + 1 rows: the table pass after the LAST bounce's k_shade still sorts for a bounce nobody runs, and reads that row)
  PT_HIP(r->shade_cost.alloc((size_t)r->nseg * (r->S.max_bounces + 1u)));
  PT_HIP(hipMemsetAsync(r->shade_cost.p, 0, sizeof(uint32_t) * r->shade_cost.n, r->stream));   // no batch of this render has been shaded yet
  PT_HIP(r->spill.alloc((size_t)std::max(std::max(r->closest_grid, r->closest_trace_grid), r->shadow_grid) * r->walk.block_threads * kSpillStack));  // per-thread HBM stack slab behind the LDS stack
  PT_HIP(hipMemsetAsync(r->wave_stats.p, 0, sizeof(WaveStats) * r->nstats, r->stream));
  if (p->external_accumulator) {
    r->acc = (vec4*)p->external_accumulator;
  } else {
    PT_HIP(r->acc_own.alloc(npix));
    r->acc = r->acc_own.p;
  }
  if (p->flags & PT_FLAG_GMON) {
    const uint32_t own = r->gmon_own_buckets ? r->gmon_own_buckets : p->gmon_buckets;
    PT_HIP(r->gmon_buckets_d.alloc((size_t)npix * own));
    PT_HIP(hipMemsetAsync(r->gmon_buckets_d.p, 0, sizeof(vec4) * npix * own, r->stream));
  }
  PT_HIP(hipMemsetAsync(r->acc, 0, sizeof(vec4) * npix, r->stream));
  if (aov) {
    PT_HIP(r->Abuf.alloc(2 * r->Lbuf.n));
    PT_HIP(r->aov_img.alloc(3 * npix));
    PT_HIP(hipMemsetAsync(r->aov_img.p, 0, sizeof(vec4) * 3 * npix, r->stream));
  }
  if (matte) {
    PT_HIP(r->Mbuf.alloc(r->Lbuf.n));
    PT_HIP(r->matte_slots.alloc((size_t)npix * kMattePixelVec4));
    launch_matte_clear(r->stream, r->matte_slots.p, (size_t)npix);   // every slot {PT_MATTE_NONE, 0}
    PT_HIP(hipGetLastError());
  }
  if (film) {
    PT_HIP(r->Fbuf.alloc(r->Lbuf.n));
    PT_HIP(r->film_img.alloc(npix));
    PT_HIP(hipMemsetAsync(r->film_img.p, 0, sizeof(vec4) * npix, r->stream));
  }
  if (ao) {
    PT_HIP(r->Obuf.alloc(r->Lbuf.n));
    PT_HIP(r->ao_counts.alloc(npix));
    PT_HIP(hipMemsetAsync(r->ao_counts.p, 0, sizeof(uint2) * npix, r->stream));
  }
  if (adaptive || region) {  // every tile the rectangle touches starts active (the whole frame: [0, tiles)), ascending (adaptive.hip)
    const Rect rect = render_rect(r, p);
    const uint32_t tiles = tile_count(p->width, p->height);
    std::vector<uint32_t> first(rect_tiles(rect, p->width, nullptr, 0));
    (void)rect_tiles(rect, p->width, first.data(), (uint32_t)first.size());
    const uint32_t active = (uint32_t)first.size();
    r->ad_tiles0 = active;
    PT_HIP(r->ad_list[0].upload(first));
    PT_HIP(r->ad_list[1].upload(first));
    PT_HIP(r->ad_count.upload(std::vector<uint32_t>{active, active}));
    PT_HIP(r->ad_tile_n.alloc(tiles));
    PT_HIP(hipMemsetAsync(r->ad_tile_n.p, 0, sizeof(uint32_t) * tiles, r->stream));
    if (adaptive) {
      PT_HIP(r->ad_mom.alloc(npix));
      PT_HIP(hipMemsetAsync(r->ad_mom.p, 0, sizeof(vec2) * npix, r->stream));
      PT_HIP(r->ad_flags.alloc(active));
      PT_HIP(r->ad_scratch.alloc(std::max<size_t>(1, adaptive_scratch_bytes(active))));
      if (!r->ad_host_count) PT_HIP(hipHostMalloc((void**)&r->ad_host_count, sizeof(uint32_t), hipHostMallocDefault));
      if (!r->ad_event) PT_HIP(hipEventCreateWithFlags(&r->ad_event, hipEventDisableTiming));
      *r->ad_host_count = active;
    }
  }
  PT_HIP(hipMemsetAsync(r->totals.p, 0, sizeof(Totals), r->stream));
  PT_HIP(hipStreamSynchronize(r->stream));
  return PT_OK;
}

// 7. nothing can fail any more: the render exists from here on
void reset_progress(pt_renderer* r, const pt_render_params* p) {
  for (int k = 0; k < K_CLASSES; k++) { r->ms_class[k] = 0; r->launches[k] = 0; }
  r->accumulated = 0;
  r->launched = 0;
  r->batches = 0;
  r->last_batch_ns = 0;   // Lbuf holds nothing of THIS render yet
  r->batch_done_valid = false;
  r->total = p->spp;
  r->aov = r->denoise.enabled != 0;
  r->matte = r->matte_opts.enabled != 0;
  r->film = r->film_opts.enabled != 0;
  r->ao = r->ao_opts.enabled != 0;
  r->ao_distance = r->ao_opts.distance;
  r->adaptive = r->adaptive_opts.enabled != 0;
  r->region = r->region_opts.enabled != 0;
  r->vtiles = r->adaptive || r->region;
  r->rect = render_rect(r, p);
  r->proj = r->proj_opts;   // (proj_constants: dev_start_render, from the snapshot's camera)
  r->ad_cur = 0;
  r->ad_event_valid = false;
  r->ad_next = r->adaptive_opts.min_spp;   // the first checkpoint (none when min_spp >= spp)
  r->started = true;
  r->render_start = std::chrono::steady_clock::now();
  r->timer_ms = 0;
}

}  // namespace

int dev_start_render(pt_renderer* r, const pt_scene_snapshot* scene, const pt_render_params* p) {
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_start_render: null argument");
  int rc = validate_start(r, scene, p);
  if (rc != PT_OK) return rc;
  PT_HIP(hipSetDevice(r->device));
  if (r->stream) PT_HIP(hipStreamSynchronize(r->stream));
  r->drop_timed();
  r->free_scene();
  r->params = *p;
  r->stream = p->stream ? (hipStream_t)p->stream : r->own_stream;
  const auto t_up0 = std::chrono::steady_clock::now();
  const bool phase_log = getenv("PTAMD_START_PHASES") != nullptr;   // analysis aid: where a (re)start spends its wall time
  auto phase = [&, t_last = std::chrono::steady_clock::now()](const char* what) mutable {
    if (!phase_log) return;
    (void)hipDeviceSynchronize();
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "ptamd start: %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  };
  HostScene hs;
  if ((rc = flatten_scene(r, scene, p, &hs)) != PT_OK) return rc;
  const ProjectionConstants proj_constants = derive_projection(scene->camera, p->width, p->height, r->proj_opts);
  r->material_base.resize(hs.instances.size());
  for (size_t i = 0; i < hs.instances.size(); i++) r->material_base[i] = hs.instances[i].material_base;
  phase("host flatten + light table");
  if ((rc = upload_scene(r, p, &hs)) != PT_OK) return rc;
  phase("upload");
  PT_HIP(hipDeviceSynchronize());
  r->upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up0).count();
  if ((rc = build_accel(r, p, &hs)) != PT_OK) return rc;
  phase("acceleration structure");
  if ((rc = build_records(r)) != PT_OK) return rc;
  phase("shade / light records");
  if ((rc = build_camera_lists(r, p)) != PT_OK) return rc;
  phase("camera lists");
  if ((rc = allocate_buffers(r, p)) != PT_OK) return rc;
  phase("queues + accumulator");
  reset_progress(r, p);
  r->proj_constants = proj_constants;
  return PT_OK;
}

// Tile-adaptive sampling: has the newest checkpoint enqueued completed with no tile left?  Never blocks: the count is read from pinned host
// memory once the event behind its copy has completed.  Then the render is complete: what is accepted but not yet enqueued is dropped,
// and pt_progress / pt_status report the whole render (batches already enqueued carry no tile).
int adaptive_observe(pt_renderer* r) {
  if (!r->ad_event_valid) return PT_OK;
  const hipError_t q = hipEventQuery(r->ad_event);
  if (q == hipErrorNotReady) { (void)hipGetLastError(); return PT_OK; }
  if (q != hipSuccess) {
    (void)hipGetLastError();
    return fail(PT_ERR_HIP, std::string("adaptive sampling: a checkpoint failed: ") + hipGetErrorString(q));
  }
  if (*(volatile uint32_t*)r->ad_host_count == 0) r->accumulated = r->launched = r->total;
  return PT_OK;
}

// Enqueues accepted-but-pending samples.  The reference's frontend calls render() once per UI frame for exactly ONE sample
// (renderer_pt.cpp:131-153, frontend.cpp:209-210); a one-sample batch leaves the deep bounces of the wavefront too narrow for the
// chip (C3: 1 in flight runs at about a third of the 64-in-flight rate).  So a step that arrives while the previous batch is
// still executing is not enqueued on its own: it waits until the GPU has drained (then everything pending goes out as ONE batch)
// or until a full batch of `samples_in_flight` has gathered (enqueued behind the running one, so the GPU never idles).  A caller
// slower than the GPU gets exactly the old behaviour (one batch per call); a tight render() loop converges to full batches.
// The image does not depend on the batching: k_accumulate folds samples in index order.  `all`: enqueue everything now.
// An adaptive render also cuts a batch at the next checkpoint and stops once it has observed that no tile is active (adaptive_observe);
// `sync_checkpoints` (pt_wait and the blocking reads) waits for each checkpoint it enqueues, so that no batch follows the last active tile.
int flush_pending(pt_renderer* r, bool all, bool sync_checkpoints) {
  if (r->adaptive) { const int rc = adaptive_observe(r); if (rc != PT_OK) return rc; }
  while (r->launched < r->accumulated) {
    const uint64_t pending = r->accumulated - r->launched;
    bool idle = true;
    if (r->batch_done_valid) {
      const hipError_t q = hipEventQuery(r->batch_done);
      if (q == hipErrorNotReady) {
        idle = false;
        (void)hipGetLastError();  // hipErrorNotReady is an answer, not a failure: do not leave it for the next hipGetLastError() check
      } else if (q != hipSuccess) {  // a fault or a lost context is NOT "still busy": report it now, not at some later wait
        (void)hipGetLastError();
        return fail(PT_ERR_HIP, std::string("pt_render_step: the previous batch failed: ") + hipGetErrorString(q));
      }
    }
    if (!all && !idle && pending < r->samples_in_flight) break;
    uint32_t ns = (uint32_t)std::min<uint64_t>(pending, r->samples_in_flight);
    const bool cut = r->adaptive && r->ad_next < r->total && r->launched + ns >= r->ad_next;   // batches never straddle a checkpoint
    if (cut) ns = (uint32_t)(r->ad_next - r->launched);
    const int rc = enqueue_batch(r, r->params.first_sample + (uint32_t)r->launched, ns, (uint32_t)r->launched, BATCH_RENDER, nullptr);
    if (rc != PT_OK) return rc;
    r->launched += ns;
    r->batches++;
    if (r->batch_done && hipEventRecord(r->batch_done, r->stream) == hipSuccess) r->batch_done_valid = true;
    if (cut && sync_checkpoints) {
      PT_HIP(hipEventSynchronize(r->ad_event));
      const int orc = adaptive_observe(r);
      if (orc != PT_OK) return orc;
    }
  }
  return PT_OK;
}

int dev_render_step(pt_renderer* r, uint32_t max_spp) {
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "null renderer");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "pt_render_step before pt_start_render");
  PT_HIP(hipSetDevice(r->device));
  const uint64_t remaining = r->total - r->accumulated;
  r->accumulated += max_spp == 0 ? remaining : std::min<uint64_t>(max_spp, remaining);
  // the last samples of the render go out at once: nothing is ever pending while status() reports Done
  const int rc = flush_pending(r, r->accumulated == r->total);
  r->timer_ms = (uint64_t)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r->render_start).count();
  return rc;
}

int dev_wait(pt_renderer* r) {
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "null renderer");
  PT_HIP(hipSetDevice(r->device));
  if (r->started) { const int rc = flush_pending(r, true, true); if (rc != PT_OK) return rc; }
  PT_HIP(hipStreamSynchronize(r->stream));
  if (r->started && r->adaptive) { const int rc = adaptive_observe(r); if (rc != PT_OK) return rc; }
  collect_timings(r);
  if (r->started && getenv("PTAMD_DUMP_CHUNKS")) {  // analysis aid: 64-ray chunks per bounce of the LAST batch (the counters are per batch)
    BatchCounters h{};
    if (hipMemcpy(&h, r->ctr.p, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess) {
      fprintf(stderr, "ptamd chunks closest:");
      for (uint32_t b = 0; b < r->S.max_bounces; b++) fprintf(stderr, " %u", h.chunks_closest[b]);
      fprintf(stderr, "\nptamd chunks shadow:");
      for (uint32_t b = 0; b < r->S.max_bounces; b++) fprintf(stderr, " %u", h.chunks_shadow[b]);
      fprintf(stderr, "\n");
    }
  }
#ifdef PT_TAIL_PROBE   // analysis build only: per launch of the LAST batch, how long the chip waited for its last wave after the average wave had run out of work
  if (r->started) {
    BatchCounters h{};
    if (hipMemcpy(&h, r->ctr.p, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess) {
      const char* names[3] = {"closest", "shade", "shadow"};
      for (int k = 0; k < 3; k++) {
        double tot = 0, tail = 0;
        fprintf(stderr, "ptamd tail %s:", names[k]);
        for (uint32_t b = 0; b < r->S.max_bounces && b < 16; b++) {
          if (!h.tail_waves[k][b]) continue;
          const double t0 = (double)(~h.tail_start_inv[k][b]), t1 = (double)h.tail_end_max[k][b], mean = (double)h.tail_end_sum[k][b] / (double)h.tail_waves[k][b];
          fprintf(stderr, " b%u %.2f ms, idle tail %.1f %%;", b, (t1 - t0) / 1e5, 100.0 * (t1 - mean) / (t1 - t0));
          tot += t1 - t0; tail += t1 - mean;
        }
        fprintf(stderr, "  all: %.2f ms, %.1f %% idle tail", tot / 1e5, tot > 0 ? 100.0 * tail / tot : 0.0);
        if (k != 1) {
          double take = 0, setup = 0, busy = 0;
          for (uint32_t b = 0; b < r->S.max_bounces && b < 16; b++) { take += (double)h.tail_take[k][b]; setup += (double)h.tail_setup[k][b]; busy += (double)h.tail_busy[k][b]; }
          if (busy > 0) fprintf(stderr, "; wave time: %.1f %% taking chunks, %.1f %% loading rays + set-up", 100.0 * take / busy, 100.0 * setup / busy);
        }
        fprintf(stderr, "\n");
      }
    } else (void)hipGetLastError();
  }
#endif
#ifdef PT_DEBUG_PID   // debug build only (tools/build_variant.sh dbg -DPT_DEBUG_PID), like $PTAMD_DEBUG_RAY: nothing of it ships in libptamd.so
  if (r->started && r->last_batch_ns) {
    if (const char* e = getenv("PTAMD_DEBUG_PIXEL")) {  // analysis aid: "x,y" -> the per-sample radiance of that pixel in the LAST batch
      uint32_t x = 0, y = 0;
      if (sscanf(e, "%u,%u", &x, &y) == 2 && x < r->S.width && y < r->S.height) {
        const uint32_t ns = r->last_batch_ns;
        const size_t at0 = lbuf_index(tile_of_pixel(x, y, r->S.width), 0, ns, lane_of_pixel(x, y));   // the pixel's ns samples are consecutive
        std::vector<vec4> v(ns);
        bool ok = at0 + ns <= r->Lbuf.n;   // (a restart with another size / batch before any new batch: last_batch_ns is reset then, this is the belt)
        if (ok) ok = hipMemcpy(v.data(), r->Lbuf.p + at0, sizeof(vec4) * ns, hipMemcpyDeviceToHost) == hipSuccess;
        if (!ok) (void)hipGetLastError();   // an analysis aid must not leave an error for the next batch's hipGetLastError()
        for (uint32_t k = 0; ok && k < ns; k++) {
          uint32_t b[3]; memcpy(b, &v[k], 12);
          fprintf(stderr, "ptamd pixel %u,%u sample %u: %08x %08x %08x  %.9g %.9g %.9g\n", x, y, r->last_batch_first + k, b[0], b[1], b[2], v[k].x, v[k].y, v[k].z);
        }
      }
    }
  }
#endif
  if (r->started)
    r->timer_ms = (uint64_t)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r->render_start).count();
  return PT_OK;
}

int dev_status(const pt_renderer* r) {  // renderer_pt.cpp:1023-1031
  if (!r) return PT_STATUS_BLOCKED;
  if (r->started && r->accumulated < r->total) return PT_STATUS_BUSY;
  int st = PT_STATUS_READY;
  if (r->started) st |= PT_STATUS_DONE;
  return st;
}

int dev_progress(const pt_renderer* r, uint64_t* accumulated, uint64_t* total) {
  if (!r || !accumulated || !total) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  *accumulated = r->accumulated;
  *total = r->total;
  return PT_OK;
}

uint64_t dev_render_time_ms(const pt_renderer* r) { return r ? r->timer_ms : 0; }

int dev_read_accumulator(pt_renderer* r, float* rgba_out) {
  if (!r || !rgba_out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "pt_read_accumulator before pt_start_render");
  int rc = dev_wait(r);
  if (rc != PT_OK) return rc;
  PT_HIP(hipMemcpy(rgba_out, r->acc, sizeof(vec4) * (size_t)r->S.width * r->S.height, hipMemcpyDeviceToHost));
  return PT_OK;
}

int dev_read_aov(pt_renderer* r, uint32_t aov, float* rgba_out) {
  if (!r || !rgba_out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started || !r->aov) return fail(PT_ERR_BAD_STATE, "pt_read_aov: the render was not started with AOVs enabled");
  if (aov > PT_AOV_MOMENTS) return fail(PT_ERR_INVALID_ARGUMENT, "pt_read_aov: no such AOV");
  int rc = dev_wait(r);
  if (rc != PT_OK) return rc;
  const size_t npix = (size_t)r->S.width * r->S.height;
  PT_HIP(hipMemcpy(rgba_out, r->aov_img.p + aov * npix, sizeof(vec4) * npix, hipMemcpyDeviceToHost));
  return PT_OK;
}

// ---- the film (film.hip, pt_film.h; its options and its place in the display chain: display.hip) ------------------------------------------
int dev_read_film(pt_renderer* r, float* rgba_out) {
  if (!r || !rgba_out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started || !r->film) return fail(PT_ERR_BAD_STATE, "pt_read_film: the render was not started with the film enabled");
  int rc = dev_wait(r);
  if (rc != PT_OK) return rc;
  PT_HIP(hipMemcpy(rgba_out, r->film_img.p, sizeof(vec4) * (size_t)r->S.width * r->S.height, hipMemcpyDeviceToHost));
  return PT_OK;
}

// ---- ambient occlusion (pt_ao.h, k_trace_ao in kernels.hip, ao.hip) --------------------------------------------------------------------------
extern "C" void pt_default_ao_options(pt_ao_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->distance = 1.0f;
}

// (the options are checked before the renderer, as dev_set_film_options)
int dev_set_ao_options(pt_renderer* r, const pt_ao_options* o) {
  if (!o) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_ao_options: null options");
  if (const char* why = ao_options_error(*o)) return fail(PT_ERR_INVALID_ARGUMENT, std::string("pt_set_ao_options: ") + why);
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_ao_options: null renderer");
  r->ao_opts = *o;
  return PT_OK;
}

namespace {

// what every AO read checks first, in this order: the arguments, then the render's state; then it waits for the render
int ao_read_counts(pt_renderer* r, const void* out, const char* who, std::vector<uint2>* counts) {
  if (!r || !out) return fail(PT_ERR_INVALID_ARGUMENT, std::string(who) + ": null argument");
  if (!r->started || !r->ao) return fail(PT_ERR_BAD_STATE, std::string(who) + ": the render was not started with ambient occlusion enabled");
  const int rc = dev_wait(r);
  if (rc != PT_OK) return rc;
  counts->resize((size_t)r->S.width * r->S.height);
  PT_HIP(hipMemcpy(counts->data(), r->ao_counts.p, sizeof(uint2) * counts->size(), hipMemcpyDeviceToHost));
  return PT_OK;
}

}  // namespace

int dev_read_ao_counts(pt_renderer* r, uint32_t* out) {
  std::vector<uint2> c;
  const int rc = ao_read_counts(r, out, "pt_read_ao_counts", &c);
  if (rc != PT_OK) return rc;
  for (size_t p = 0; p < c.size(); p++) { out[2 * p] = c[p].x; out[2 * p + 1] = c[p].y; }
  return PT_OK;
}

int dev_read_ao(pt_renderer* r, float* out) {
  std::vector<uint2> c;
  const int rc = ao_read_counts(r, out, "pt_read_ao", &c);
  if (rc != PT_OK) return rc;
  for (size_t p = 0; p < c.size(); p++) out[p] = ao_value(c[p].x, c[p].y);
  return PT_OK;
}

int dev_get_ao_stats(pt_renderer* r, pt_ao_stats* out) {
  std::vector<uint2> c;
  const int rc = ao_read_counts(r, out, "pt_get_ao_stats", &c);
  if (rc != PT_OK) return rc;
  memset(out, 0, sizeof(*out));
  for (const uint2& v : c) out->rays += v.x;   // one AO ray per camera ray that hit
  out->ms_trace = (float)r->ms_class[K_AO_TRACE];
  out->ms_fold = (float)r->ms_class[K_AO_FOLD];
  return PT_OK;
}

// One sample of every pixel: pt_trace_primary's batch (camera rays, table pass, tree walk), then the AO trace of a render batch with its ray log,
// and the states scattered to pixel order.  Obuf is the render's own (each batch rewrites it before its fold); the counts are not touched.
int dev_debug_ao(pt_renderer* r, uint32_t sample_idx, float* origins, float* directions, uint32_t* state) {
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_ao: null renderer");
  if (!r->started || !r->ao) return fail(PT_ERR_BAD_STATE, "pt_debug_ao: the render was not started with ambient occlusion enabled");
  PT_HIP(hipSetDevice(r->device));
  { const int rc = flush_pending(r, true); if (rc != PT_OK) return rc; }
  const uint32_t npix = r->S.width * r->S.height;
  DevBuf<float> log;
  DevBuf<uint32_t> st;
  PT_HIP(log.alloc(6 * (size_t)npix));
  PT_HIP(st.alloc(npix));
  hipStream_t s = r->stream;
  PT_HIP(hipMemsetAsync(log.p, 0, sizeof(float) * log.n, s));      // a pixel whose camera ray missed: zero origin and direction, state 0
  PT_HIP(hipMemsetAsync(st.p, 0, sizeof(uint32_t) * st.n, s));
  PT_HIP(hipMemsetAsync(r->ctr.p, 0, sizeof(BatchCounters), s));
  Segments seg = r->segments();
  seg.nsamples = 1;
  launch_camera_raygen(r, seg, sample_idx, 1, nullptr);
  launch_chunk_tables(s, seg, 0, r->ctr.p, 0, 0, false);
  launch_trace_closest(s, r->closest_trace_grid, r->S, r->path_state(0), r->hit.p, seg, 0, r->ctr.p, 0, r->spill.p, nullptr, npix, false);
  launch_trace_ao(s, r->closest_grid, r->S, r->path_state(0), r->hit.p, seg, r->ctr.p, r->spill.p, r->Obuf.p, r->ao_distance, log.p, npix);
  launch_ao_scatter(s, r->grid, r->S.width, r->path_state(0), r->hit.p, seg, r->Obuf.p, st.p);
  launch_fold_counters(s, r->ctr.p, r->totals.p + 1, seg, false);  // clears the per-wave statistics (scratch slot), as pt_trace_primary
  PT_HIP(hipGetLastError());
  PT_HIP(hipStreamSynchronize(s));
  if (origins) PT_HIP(hipMemcpy(origins, log.p, sizeof(float) * 3 * (size_t)npix, hipMemcpyDeviceToHost));
  if (directions) PT_HIP(hipMemcpy(directions, log.p + 3 * (size_t)npix, sizeof(float) * 3 * (size_t)npix, hipMemcpyDeviceToHost));
  if (state) PT_HIP(hipMemcpy(state, st.p, sizeof(uint32_t) * npix, hipMemcpyDeviceToHost));
  return PT_OK;
}

// one elementwise launch of math_probe.hip on uploaded arguments; the renderer's own state is untouched (the Halton table is read)
int dev_debug_math(pt_renderer* r, uint32_t fn, uint32_t n, const void* a, const void* b, void* out0, void* out1) {
  if (fn >= PT_MATH_COUNT) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_math: unknown function");
  if (n == 0 || n > (1u << 24)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_math: n must be 1..2^24");
  const bool reads_b = math_probe_reads_b(fn), writes_1 = math_probe_writes_out1(fn);
  if (!a || !out0 || (reads_b && !b) || (writes_1 && !out1)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_math: null argument");
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_math: null renderer");
  PT_HIP(hipSetDevice(r->device));
  const size_t n1 = fn == PT_MATH_SAMPLE_COSINE_HEMISPHERE ? 2 * (size_t)n : n;  // words of out1
  DevBuf<uint32_t> da, db, d0, d1;
  PT_HIP(da.alloc(n)); PT_HIP(d0.alloc(n));
  if (reads_b) PT_HIP(db.alloc(n));
  if (writes_1) PT_HIP(d1.alloc(n1));
  PT_HIP(hipMemcpyAsync(da.p, a, sizeof(uint32_t) * n, hipMemcpyHostToDevice, r->stream));
  if (reads_b) PT_HIP(hipMemcpyAsync(db.p, b, sizeof(uint32_t) * n, hipMemcpyHostToDevice, r->stream));
  launch_math_probe(r->stream, fn, n, da.p, db.p, d0.p, d1.p, r->halton.p);
  PT_HIP(hipGetLastError());
  PT_HIP(hipStreamSynchronize(r->stream));
  PT_HIP(hipMemcpy(out0, d0.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
  if (writes_1) PT_HIP(hipMemcpy(out1, d1.p, sizeof(uint32_t) * n1, hipMemcpyDeviceToHost));
  return PT_OK;
}

// ---- sun and sky (sky.hip) ----
extern "C" void pt_default_sky_options(pt_sky_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->sun_elevation = 0.5f;
  o->sun_angular_radius = 0.004712f;
  o->sun_intensity = 1.0f;
  o->sun_disc = 1u;
  o->altitude_km = 0.001f;
  o->air_density = o->dust_density = o->ozone_density = 1.0f;
  o->ground_albedo = 0.3f;
}

// One launch of k_sky into a buffer of its own, timed by events; Omega_d and the covered texels are counted on the host (pt_sky.h) and the
// renderer's own state is untouched.  (The options and the size are checked before the renderer, as dev_debug_bloom.)
int dev_generate_sky(pt_renderer* r, const pt_sky_options* o, uint32_t width, uint32_t height, float* rgba_out, pt_sky_stats* stats_out) {
  if (!o || !rgba_out) return fail(PT_ERR_INVALID_ARGUMENT, "pt_generate_sky: null argument");
  if (const char* why = sky_options_error(*o, width, height)) return fail(PT_ERR_INVALID_ARGUMENT, std::string("pt_generate_sky: ") + why);
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_generate_sky: null renderer");
  PT_HIP(hipSetDevice(r->device));
  SkyParams P = sky_setup(*o, width, height);
  uint32_t texels = 0;
  const double omega = sky_solid_angle(P, &texels);
  P.omega = o->sun_disc ? (float)omega : 0.0f;
  const size_t n = (size_t)width * height;
  DevBuf<vec4> img;
  PT_HIP(img.alloc(n));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  PT_HIP(hipEventCreate(&e0));
  hipError_t e = hipEventCreate(&e1);
  if (e == hipSuccess) e = hipEventRecord(e0, r->stream);
  if (e == hipSuccess) { launch_sky(r->stream, P, img.p); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipEventRecord(e1, r->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
  float ms = 0.0f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  PT_HIP(e);
  PT_HIP(hipMemcpy(rgba_out, img.p, sizeof(vec4) * n, hipMemcpyDeviceToHost));
  if (stats_out) {
    stats_out->sun_direction[0] = P.s.x; stats_out->sun_direction[1] = P.s.y; stats_out->sun_direction[2] = P.s.z;
    stats_out->sun_radius_used = P.alpha_eff;
    stats_out->sun_solid_angle = omega;
    stats_out->sun_texels = texels;
    stats_out->kernel_ms = ms;
  }
  return PT_OK;
}

// one elementwise launch of light_probe.hip on uploaded records against the started render's scene table; the render's state is untouched.
// The draws and directions are checked on the host first: shade_nee_light and stage_miss index tables with them, and a draw outside [0, 1)
// (a NaN too) would walk the light search or the alias table out of bounds.
int dev_debug_lights(pt_renderer* r, uint32_t fn, uint32_t n, const pt_light_probe_args* args, const void* in, void* out) {
  if (fn >= PT_LIGHT_COUNT) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_lights: unknown function");
  if (n == 0 || n > (1u << 24)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_lights: n must be 1..2^24");
  if (!args || !in || !out) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_lights: null argument");
  if (fn == PT_LIGHT_SAMPLE && args->tables != PT_LIGHT_TABLES_HBM && args->tables != PT_LIGHT_TABLES_LDS)
    return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_lights: tables must be PT_LIGHT_TABLES_HBM or PT_LIGHT_TABLES_LDS");
  if (fn == PT_LIGHT_SAMPLE && args->dim > kMetaDimMask) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_lights: dim must fit a path's cursor (0..1023)");
  const uint32_t wi = light_probe_in_words(fn), wo = light_probe_out_words(fn);
  const float* f = (const float*)in;
  for (size_t i = 0; i < n; i++) {
    const float* e = f + i * wi;
    if (fn == PT_LIGHT_SAMPLE) {
      for (int k = 3; k < 6; k++)
        if (!(e[k] >= 0.0f && e[k] < 1.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_lights: a draw lies outside [0, 1)");
    } else {
      for (int k = 0; k < 3; k++)
        if (!(e[k] >= -1.0f && e[k] <= 1.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_lights: a direction component lies outside [-1, 1]");
    }
  }
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_lights: null renderer");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "pt_debug_lights before pt_start_render");
  if (const char* why = light_probe_unsupported(r->S, fn, *args, kLightProbeStaged)) return fail(PT_ERR_UNSUPPORTED, why);
  PT_HIP(hipSetDevice(r->device));
  DevBuf<float> din;
  DevBuf<uint32_t> dout;
  PT_HIP(din.alloc((size_t)n * wi)); PT_HIP(dout.alloc((size_t)n * wo));
  PT_HIP(hipMemcpyAsync(din.p, in, sizeof(float) * (size_t)n * wi, hipMemcpyHostToDevice, r->stream));
  launch_light_probe(r->stream, r->scene_d.p, fn, n, *args, din.p, dout.p);
  PT_HIP(hipGetLastError());
  PT_HIP(hipStreamSynchronize(r->stream));
  PT_HIP(hipMemcpy(out, dout.p, sizeof(uint32_t) * (size_t)n * wo, hipMemcpyDeviceToHost));
  return PT_OK;
}

// pt_debug_shading: the (instance, primitive) pairs of every triangle come back from the device first (one launch over the leaf slots), the
// host resolves each record's triangle against them and refuses the batch if one names none; then one elementwise launch of
// shade_probe.hip on the resolved records against the started render's scene table.  The render's state is untouched.
int dev_debug_shading(pt_renderer* r, uint32_t n, const void* in, void* out) {
  if (n == 0 || n > (1u << 24)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_shading: n must be 1..2^24");
  if (!in || !out) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_shading: null argument");
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_shading: null renderer");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "pt_debug_shading before pt_start_render");
  PT_HIP(hipSetDevice(r->device));
  const uint32_t n_tri = 2u * r->slot_count;
  std::vector<int32_t> ids(2 * (size_t)n_tri);
  if (n_tri) {
    DevBuf<int32_t> dids;
    PT_HIP(dids.alloc(ids.size()));
    launch_shade_probe_ids(r->stream, r->scene_d.p, n_tri, dids.p);
    PT_HIP(hipGetLastError());
    PT_HIP(hipStreamSynchronize(r->stream));
    PT_HIP(hipMemcpy(ids.data(), dids.p, sizeof(int32_t) * ids.size(), hipMemcpyDeviceToHost));
  }
  std::vector<uint32_t> rec((size_t)n * PT_SHADE_PROBE_IN_WORDS);
  memcpy(rec.data(), in, sizeof(uint32_t) * rec.size());
  if (!shade_probe_resolve(ids.data(), n_tri, rec.data(), n))
    return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_shading: a record's (instance, primitive) names no triangle of the scene");
  DevBuf<uint32_t> din, dout;
  PT_HIP(din.alloc(rec.size())); PT_HIP(dout.alloc((size_t)n * PT_SHADE_PROBE_OUT_WORDS));
  PT_HIP(hipMemcpyAsync(din.p, rec.data(), sizeof(uint32_t) * rec.size(), hipMemcpyHostToDevice, r->stream));
  launch_shade_probe(r->stream, r->scene_d.p, n, din.p, dout.p);
  PT_HIP(hipGetLastError());
  PT_HIP(hipStreamSynchronize(r->stream));
  PT_HIP(hipMemcpy(out, dout.p, sizeof(uint32_t) * (size_t)n * PT_SHADE_PROBE_OUT_WORDS, hipMemcpyDeviceToHost));
  return PT_OK;
}

extern "C" void pt_default_adaptive_options(pt_adaptive_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->threshold = 0.02f;
  o->min_spp = 32;
  o->interval = 32;
}

// (the options are checked before the renderer: a host without a device can exercise the validation)
int dev_set_adaptive_options(pt_renderer* r, const pt_adaptive_options* o) {
  if (!o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!(o->threshold > 0.0f && o->threshold <= 3.4028234663852886e38f))
    return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_adaptive_options: threshold must be finite and > 0");
  if (o->min_spp < 2) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_adaptive_options: min_spp must be >= 2");
  if (o->interval < 1) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_adaptive_options: interval must be >= 1");
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_adaptive_options: null renderer");
  r->adaptive_opts = *o;
  return PT_OK;
}

int dev_read_sample_counts(pt_renderer* r, uint32_t* out) {
  if (!r || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "pt_read_sample_counts before pt_start_render");
  int rc = dev_wait(r);
  if (rc != PT_OK) return rc;
  const uint32_t W = r->S.width, H = r->S.height;
  if (!r->vtiles) {
    std::fill(out, out + (size_t)W * H, (uint32_t)r->launched);
    return PT_OK;
  }
  // per tile; a region render without adaptive sampling folds every batch into every tile of its list: the same numbers.  Pixels outside the
  // render's rectangle hold no sample.
  std::vector<uint32_t> tn(r->ad_tile_n.n);
  PT_HIP(hipMemcpy(tn.data(), r->ad_tile_n.p, sizeof(uint32_t) * tn.size(), hipMemcpyDeviceToHost));
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++) out[(size_t)y * W + x] = rect_contains(r->rect, x, y) ? tn[tile_of_pixel(x, y, W)] : 0u;
  return PT_OK;
}

extern "C" void pt_default_render_region(pt_render_region* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
}

int dev_get_camera_list_stats(pt_renderer* r, pt_camera_list_stats* out) {
  if (!r || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "pt_get_camera_list_stats before pt_start_render");
  *out = r->cam_stats;
  return PT_OK;
}

// (the options are checked before the renderer, as dev_set_adaptive_options)
int dev_set_render_region(pt_renderer* r, const pt_render_region* o) {
  if (!o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (o->enabled && (o->x0 >= o->x1 || o->y0 >= o->y1))
    return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_render_region: the region is empty (x0 < x1 and y0 < y1 are required)");
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_render_region: null renderer");
  r->region_opts = *o;
  return PT_OK;
}

// ---- ID mattes (matte.hip, pt_matte.h) ----------------------------------------------------------------------------------------------------
extern "C" void pt_default_matte_options(pt_matte_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
}

int dev_set_matte_options(pt_renderer* r, const pt_matte_options* o) {
  if (!r || !o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  r->matte_opts = *o;
  return PT_OK;
}

namespace {

// what every matte read checks first, in this order: the arguments, then the render's state
int matte_read_check(const pt_renderer* r, const void* out, uint32_t layer, const char* who) {
  if (!r || !out) return fail(PT_ERR_INVALID_ARGUMENT, std::string(who) + ": null argument");
  if (layer >= kMatteLayers) return fail(PT_ERR_INVALID_ARGUMENT, std::string(who) + ": no such layer");
  if (!r->started || !r->matte) return fail(PT_ERR_BAD_STATE, std::string(who) + ": the render was not started with mattes enabled");
  return PT_OK;
}

}  // namespace

int dev_read_matte_slots(pt_renderer* r, uint32_t layer, pt_matte_slot* out) {
  int rc = matte_read_check(r, out, layer, "pt_read_matte_slots");
  if (rc != PT_OK) return rc;
  if ((rc = dev_wait(r)) != PT_OK) return rc;
  // one layer out of the [pixel][layer][slot] image: rows of 64 B, 128 B apart
  const size_t npix = (size_t)r->S.width * r->S.height, row = kMattePixelBytes / kMatteLayers;
  PT_HIP(hipMemcpy2D(out, row, (const uint8_t*)r->matte_slots.p + layer * row, kMattePixelBytes, row, npix, hipMemcpyDeviceToHost));
  return PT_OK;
}

int dev_read_matte(pt_renderer* r, uint32_t layer, const uint32_t* ids, uint32_t id_count, float* coverage_out) {
  int rc = matte_read_check(r, coverage_out, layer, "pt_read_matte");
  if (rc == PT_ERR_INVALID_ARGUMENT) return rc;
  if (id_count && !ids) return fail(PT_ERR_INVALID_ARGUMENT, "pt_read_matte: null id set");
  if (rc != PT_OK) return rc;
  if ((rc = dev_wait(r)) != PT_OK) return rc;
  const std::vector<uint32_t> set = matte_id_set(ids, id_count);
  const size_t npix = (size_t)r->S.width * r->S.height;
  PT_HIP(r->matte_ids.alloc(std::max<size_t>(1, set.size())));
  if (!set.empty()) PT_HIP(hipMemcpyAsync(r->matte_ids.p, set.data(), sizeof(uint32_t) * set.size(), hipMemcpyHostToDevice, r->stream));
  PT_HIP(r->matte_cov.alloc(npix));
  launch_matte_resolve(r->stream, r->matte_slots.p, layer, r->matte_ids.p, (uint32_t)set.size(), r->vtiles ? r->ad_tile_n.p : nullptr,
                       (uint32_t)r->launched, r->rect, r->S.width, r->S.height, r->matte_cov.p);
  PT_HIP(hipGetLastError());
  PT_HIP(hipStreamSynchronize(r->stream));   // (`set` is read by the copy until here)
  PT_HIP(hipMemcpy(coverage_out, r->matte_cov.p, sizeof(float) * npix, hipMemcpyDeviceToHost));
  return PT_OK;
}

int dev_pick(pt_renderer* r, uint32_t x, uint32_t y, pt_pick_result* out) {
  if (!r || !out) return fail(PT_ERR_INVALID_ARGUMENT, "pt_pick: null argument");
  if (!r->started || !r->matte) return fail(PT_ERR_BAD_STATE, "pt_pick: the render was not started with mattes enabled");
  if (x >= r->S.width || y >= r->S.height) return fail(PT_ERR_INVALID_ARGUMENT, "pt_pick: the pixel is outside the frame");
  int rc = dev_wait(r);
  if (rc != PT_OK) return rc;
  pt_matte_slot px[kMatteLayers][kMatteSlots];
  static_assert(sizeof(px) == kMattePixelBytes, "pt_pick reads one pixel of the slot image");
  PT_HIP(hipMemcpy(px, (const uint8_t*)r->matte_slots.p + ((size_t)y * r->S.width + x) * kMattePixelBytes, sizeof(px), hipMemcpyDeviceToHost));
  uint32_t n = rect_contains(r->rect, x, y) ? (uint32_t)r->launched : 0u;
  if (n && r->adaptive)   // the tile's own count
    PT_HIP(hipMemcpy(&n, r->ad_tile_n.p + tile_of_pixel(x, y, r->S.width), sizeof(n), hipMemcpyDeviceToHost));
  uint32_t win[kMatteLayers][2];
  for (uint32_t l = 0; l < kMatteLayers; l++) {
    MatteSlots m;
    for (uint32_t k = 0; k < kMatteSlots; k++) { m.id[k] = px[l][k].id; m.count[k] = px[l][k].count; }
    const uint32_t b = matte_pick(m);
    win[l][0] = m.id[b]; win[l][1] = m.count[b];
  }
  *out = pt_pick_result{};
  out->instance = win[PT_MATTE_INSTANCE][0]; out->instance_count = win[PT_MATTE_INSTANCE][1];
  out->material = win[PT_MATTE_MATERIAL][0]; out->material_count = win[PT_MATTE_MATERIAL][1];
  out->material_instance = out->material_slot = PT_MATTE_NONE;
  if (out->material != PT_MATTE_NONE && !r->material_base.empty()) {
    // the last instance whose first material is at or before it (instances without materials share their successor's base)
    const auto it = std::upper_bound(r->material_base.begin(), r->material_base.end(), out->material);
    const size_t i = (size_t)(it - r->material_base.begin()) - (it == r->material_base.begin() ? 0u : 1u);
    out->material_instance = (uint32_t)i;
    out->material_slot = out->material - r->material_base[i];
  }
  out->samples = n;
  return PT_OK;
}

extern "C" int pt_region_tiles(uint32_t width, uint32_t height, const pt_render_region* o, uint32_t* tiles_out, uint32_t capacity, uint32_t* count) {
  if (!o || !count || (capacity && !tiles_out)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_region_tiles: null argument");
  if (width == 0 || height == 0) return fail(PT_ERR_INVALID_ARGUMENT, "pt_region_tiles: empty image");
  Rect rect{0u, 0u, width, height};
  if (o->enabled) {
    if (o->x0 >= o->x1 || o->y0 >= o->y1) return fail(PT_ERR_INVALID_ARGUMENT, "pt_region_tiles: the region is empty");
    if (o->x1 > width || o->y1 > height) return fail(PT_ERR_INVALID_ARGUMENT, "pt_region_tiles: the region does not fit the image");
    rect = Rect{o->x0, o->y0, o->x1, o->y1};
  }
  *count = rect_tiles(rect, width, tiles_out, capacity);
  return PT_OK;
}

int dev_set_gmon_options(pt_renderer* r, const pt_gmon_options* o) {
  if (!r || !o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  // G never exceeds 1, so a larger cap only acts on the NaN of an all-black pixel: min(NaN, cap) = cap, and int(cap * (n / 2)) of a
  // huge or infinite cap is undefined in k_gmon (a trim count past the bucket array in the oracle).  NaN is refused by the same test.
  if (!(o->cap >= 0.0f && o->cap <= 1.0f)) return fail(PT_ERR_INVALID_ARGUMENT, "gmon cap must lie in [0, 1]");
  r->gmon_cap = o->cap;
  return PT_OK;
}

int dev_read_gmon_bucket(pt_renderer* r, uint32_t bucket, float* rgba_out) {
  if (!r || !rgba_out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  const uint32_t own = r->gmon_own_buckets ? r->gmon_own_buckets : r->params.gmon_buckets;
  if (!r->started || !(r->params.flags & PT_FLAG_GMON) || bucket < r->gmon_bucket_base || bucket - r->gmon_bucket_base >= own)
    return fail(PT_ERR_BAD_STATE, "no such GMoN bucket");
  bucket -= r->gmon_bucket_base;
  int rc = dev_wait(r);
  if (rc != PT_OK) return rc;
  const size_t npix = (size_t)r->S.width * r->S.height;
  PT_HIP(hipMemcpy(rgba_out, r->gmon_buckets_d.p + npix * bucket, sizeof(vec4) * npix, hipMemcpyDeviceToHost));
  return PT_OK;
}

void* dev_accumulator_device_ptr(pt_renderer* r) { return (r && r->started) ? (void*)r->acc : nullptr; }

int dev_get_constants(const pt_renderer* r, pt_constants* out) {
  if (!r || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "no render started");
  *out = r->constants;
  return PT_OK;
}

int dev_get_lights(const pt_renderer* r, pt_area_light* out, uint32_t capacity, uint32_t* count) {
  if (!r || !count) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "no render started");
  *count = (uint32_t)r->lights.size();
  if (out)
    for (uint32_t i = 0; i < std::min<uint32_t>(capacity, *count); i++) out[i] = r->lights[i];
  return PT_OK;
}

int dev_get_env_alias(const pt_renderer* r, pt_alias_entry* out, uint64_t capacity, uint64_t* count) {
  if (!r || !count) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "no render started");
  *count = r->env_alias.size();
  if (out)
    for (uint64_t i = 0; i < std::min<uint64_t>(capacity, *count); i++) out[i] = r->env_alias[i];
  return PT_OK;
}

int dev_trace_primary(pt_renderer* r, uint32_t sample_idx, pt_hit_record* out) {
  if (!r || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "no render started");
  PT_HIP(hipSetDevice(r->device));
  { const int rc = flush_pending(r, true); if (rc != PT_OK) return rc; }
  const uint32_t npix = r->S.width * r->S.height;
  DevBuf<pt_hit_record> rec;
  PT_HIP(rec.alloc(npix));
  hipStream_t s = r->stream;
  PT_HIP(hipMemsetAsync(r->ctr.p, 0, sizeof(BatchCounters), s));
  Segments seg = r->segments();
  seg.nsamples = 1;
  launch_camera_raygen(r, seg, sample_idx, 1, nullptr);
  launch_chunk_tables(s, seg, 0, r->ctr.p, 0, 0, false);
  launch_trace_closest(s, r->closest_trace_grid, r->S, r->path_state(0), r->hit.p, seg, 0, r->ctr.p, 0, r->spill.p, nullptr, npix, false);
  launch_hit_records(s, r->grid, r->S, r->path_state(0), r->hit.p, seg, rec.p);
  launch_fold_counters(s, r->ctr.p, r->totals.p + 1, seg, false);  // clears the per-wave statistics (scratch slot)
  PT_HIP(hipGetLastError());
  PT_HIP(hipStreamSynchronize(s));
  PT_HIP(hipMemcpy(out, rec.p, sizeof(pt_hit_record) * npix, hipMemcpyDeviceToHost));
  return PT_OK;
}

extern "C" void pt_default_camera_projection(pt_camera_projection* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->kind = PT_PROJ_PERSPECTIVE;
  p->ortho_height = 1.0f;
  p->fov_x = 2.0f * kPi; p->fov_y = kPi;
  p->fisheye_fov = kPi;
}

// (the options are checked before the renderer, as dev_set_despeckle_options)
int dev_set_camera_projection(pt_renderer* r, const pt_camera_projection* p) {
  if (!p) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_camera_projection: null options");
  if (const char* why = projection_error(*p)) return fail(PT_ERR_INVALID_ARGUMENT, std::string("pt_set_camera_projection: ") + why);
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_camera_projection: null renderer");
  r->proj_opts = *p;
  return PT_OK;
}

int dev_get_camera_projection(pt_renderer* r, pt_camera_projection* out) {
  if (!r || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "pt_get_camera_projection before pt_start_render");
  *out = r->proj;
  return PT_OK;
}

int dev_debug_camera_rays(pt_renderer* r, uint32_t sample_idx, float* origins, float* directions) {
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "pt_debug_camera_rays before pt_start_render");
  PT_HIP(hipSetDevice(r->device));
  { const int rc = flush_pending(r, true); if (rc != PT_OK) return rc; }
  const size_t n = 3 * (size_t)r->S.width * r->S.height;
  DevBuf<float> o, d;
  if (origins) PT_HIP(o.alloc(n));
  if (directions) PT_HIP(d.alloc(n));
  hipStream_t s = r->stream;
  PT_HIP(hipMemsetAsync(r->ctr.p, 0, sizeof(BatchCounters), s));
  Segments seg = r->segments();
  seg.nsamples = 1;
  launch_camera_raygen(r, seg, sample_idx, 1, nullptr);
  launch_camera_rays(s, r->grid, r->S.width, r->path_state(0), seg, o.p, d.p);
  launch_fold_counters(s, r->ctr.p, r->totals.p + 1, seg, false);  // clears the per-wave statistics (scratch slot), as pt_trace_primary
  PT_HIP(hipGetLastError());
  PT_HIP(hipStreamSynchronize(s));
  if (origins) PT_HIP(hipMemcpy(origins, o.p, sizeof(float) * n, hipMemcpyDeviceToHost));
  if (directions) PT_HIP(hipMemcpy(directions, d.p, sizeof(float) * n, hipMemcpyDeviceToHost));
  return PT_OK;
}

int dev_debug_sample(pt_renderer* r, uint32_t sample_idx, float* radiance_out, int32_t* hits_out) {
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "no render started");
  PT_HIP(hipSetDevice(r->device));
  { const int rc = flush_pending(r, true); if (rc != PT_OK) return rc; }
  const size_t npix = (size_t)r->S.width * r->S.height;
  DevBuf<int32_t> log;
  if (hits_out) {
    PT_HIP(log.alloc(npix * 2 * r->S.max_bounces));
    PT_HIP(hipMemsetAsync(log.p, 0xff, sizeof(int32_t) * log.n, r->stream));
  }
  int rc = enqueue_batch(r, sample_idx, 1, 0, BATCH_DEBUG, log.p);
  if (rc != PT_OK) return rc;
  PT_HIP(hipStreamSynchronize(r->stream));
  r->drop_timed();
  if (radiance_out) {  // Lbuf of a one-sample batch is [tile][lane]: bring it back and put it in image order
    const uint32_t W = r->S.width, H = r->S.height;
    std::vector<vec4> tiled((size_t)tile_count(W, H) * 64);
    PT_HIP(hipMemcpy(tiled.data(), r->Lbuf.p, sizeof(vec4) * tiled.size(), hipMemcpyDeviceToHost));
    for (uint32_t y = 0; y < H; y++)
      for (uint32_t x = 0; x < W; x++) {
        const vec4& v = tiled[lbuf_index(tile_of_pixel(x, y, W), 0, 1, lane_of_pixel(x, y))];
        float* o = radiance_out + ((size_t)y * W + x) * 4;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
      }
  }
  if (hits_out) PT_HIP(hipMemcpy(hits_out, log.p, sizeof(int32_t) * log.n, hipMemcpyDeviceToHost));
  return PT_OK;
}

int dev_measure_traversal(pt_renderer* r, uint32_t sample_idx) {
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "no render started");
  PT_HIP(hipSetDevice(r->device));
  { const int rc = flush_pending(r, true); if (rc != PT_OK) return rc; }
  const bool prof = r->profiling;
  r->profiling = false;
  int rc = enqueue_batch(r, sample_idx, 1, 0, BATCH_MEASURE, nullptr);
  r->profiling = prof;
  if (rc != PT_OK) return rc;
  PT_HIP(hipStreamSynchronize(r->stream));
  return PT_OK;
}

int dev_set_profiling(pt_renderer* r, int enabled) {
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  r->profiling = enabled != 0;
  return PT_OK;
}

int dev_get_stats(pt_renderer* r, pt_stats* out) {
  if (!r || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "no render started");
  int rc = dev_wait(r);
  if (rc != PT_OK) return rc;
  Totals t{};
  PT_HIP(hipMemcpy(&t, r->totals.p, sizeof(Totals), hipMemcpyDeviceToHost));
  memset(out, 0, sizeof(*out));
  out->triangles = r->tri_count;
  out->leaf_slots = r->slot_count;
  out->bvh_nodes = r->bvh.node_count;
  out->bvh_max_depth = r->bvh.depth4;
  out->samples_in_flight = r->samples_in_flight;
  out->upload_ms = r->upload_ms;
  out->bvh_build_ms = r->bvh_ms;
  out->closest_rays = t.closest_rays;
  out->shadow_rays = t.shadow_rays;
  out->shaded_hits = t.shaded_hits;
  out->paths = t.paths;
  out->nonfinite_samples = t.nonfinite;
  out->ms_raygen = r->ms_class[K_RAYGEN]; out->ms_closest = r->ms_class[K_CLOSEST]; out->ms_shade = r->ms_class[K_SHADE];
  out->ms_shadow = r->ms_class[K_SHADOW]; out->ms_accumulate = r->ms_class[K_ACCUM];
  out->accel_two_level = r->two_level ? 1u : 0u;
  out->batches = r->batches;
  out->launches_closest = r->launches[K_CLOSEST];
  out->launches_shadow = r->launches[K_SHADOW];
  if (t.counted_closest) {
    out->nodes_per_closest_ray = (double)t.nodes_closest / (double)t.counted_closest;
    out->tris_per_closest_ray = (double)t.tris_closest / (double)t.counted_closest;
  }
  if (t.counted_shadow) {
    out->nodes_per_shadow_ray = (double)t.nodes_shadow / (double)t.counted_shadow;
    out->tris_per_shadow_ray = (double)t.tris_shadow / (double)t.counted_shadow;
  }
  return PT_OK;
}

