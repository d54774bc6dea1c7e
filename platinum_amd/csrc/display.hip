// display.hip — everything between an HDR image and the RGBA8 render target: the options of the post-process, the tonemapper, the denoiser,
// the firefly clamp, auto exposure, bloom and the selection overlay, and the display chain that runs them (enqueue_display at the end of this
// file): source (merged | film over a backdrop | denoised | accumulator), auto exposure, bloom, k_postprocess, the film's alpha
// byte, selection overlay; or, under a pass view, the albedo AOV as the source, or a data view in place of everything up to
// the overlay.  No kernel lives here:
// the launches are those of kernels.hip, denoise.hip, exposure.hip, bloom.hip, matte.hip, selection.hip, film.hip and view.hip, and the path tracer's driver
// (renderer.hip) is reached through flush_pending and dev_wait.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "renderer_state.h"

using namespace pt;

extern "C" void pt_default_post_options(pt_post_options* o) {  // core/postprocessing.hpp:168-198
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->ca_green_shift = 70.0f;
  o->vig_feather = 50.0f; o->vig_power = 20.0f; o->vig_roundness = 100.0f;
}

extern "C" void pt_default_tonemap_options(pt_tonemap_options* o) {  // postprocessing.hpp:29-160, 209-226
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->tonemapper = PT_TONEMAP_AGX;
  for (int k = 0; k < 3; k++) { o->agx_slope[k] = 1.0f; o->agx_power[k] = 1.0f; }
  o->agx_saturation = 1.0f;
  o->khr_compression_start = 0.8f; o->khr_desaturation = 0.15f;
  o->flim_pre_exposure = 4.3f;
  for (int k = 0; k < 3; k++) { o->flim_pre_formation_filter[k] = 1.0f; o->flim_extended_gamut_mul[k] = 1.0f; o->flim_print_backlight[k] = 1.0f; o->flim_post_formation_filter[k] = 1.0f; }
  o->flim_extended_gamut_scale[0] = 1.05f; o->flim_extended_gamut_scale[1] = 1.12f; o->flim_extended_gamut_scale[2] = 1.045f;
  o->flim_extended_gamut_rotation[0] = 0.5f; o->flim_extended_gamut_rotation[1] = 2.0f; o->flim_extended_gamut_rotation[2] = 0.1f;
  o->flim_sigmoid_log2_min = -10.0f; o->flim_sigmoid_log2_max = 22.0f;
  o->flim_sigmoid_toe[0] = 0.440f; o->flim_sigmoid_toe[1] = 0.280f;
  o->flim_sigmoid_shoulder[0] = 0.591f; o->flim_sigmoid_shoulder[1] = 0.779f;
  o->flim_negative_exposure = 6.0f; o->flim_negative_density = 5.0f;
  o->flim_print_exposure = 6.0f; o->flim_print_density = 27.5f;
  o->flim_black_point = 0.0f; o->flim_auto_black_point = 1;
  o->flim_midtone_saturation = 1.02f;
  for (int k = 0; k < 3; k++) { o->shadow_color[k] = 0.5f; o->midtone_color[k] = 0.5f; o->highlight_color[k] = 0.5f; }
  const float p3[4][2] = {{0.680f, 0.320f}, {0.265f, 0.690f}, {0.150f, 0.060f}, {0.3127f, 0.3290f}};  // colorspace.cpp:6
  for (int k = 0; k < 2; k++) { o->output_space.r[k] = p3[0][k]; o->output_space.g[k] = p3[1][k]; o->output_space.b[k] = p3[2][k]; o->output_space.w[k] = p3[3][k]; }
}

int dev_set_post_options(pt_renderer* r, const pt_post_options* o) {
  if (!r || !o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  r->post = *o;
  return PT_OK;
}

int dev_set_tonemap_options(pt_renderer* r, const pt_tonemap_options* o) {
  if (!r || !o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (o->tonemapper > PT_TONEMAP_FLIM) return fail(PT_ERR_INVALID_ARGUMENT, "bad tonemapper");
  r->tonemap = *o;
  return PT_OK;
}

// ---- the denoiser and the firefly clamp ahead of it (denoise.hip) ----
extern "C" void pt_default_denoise_options(pt_denoise_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->iterations = 5;
  o->sigma_luminance = 4.0f; o->sigma_normal = 128.0f; o->sigma_depth = 1.0f;
}

int dev_set_denoise_options(pt_renderer* r, const pt_denoise_options* o) {
  if (!r || !o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (o->iterations > 8) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_denoise_options: iterations must be 0..8");
  const float sg[3] = {o->sigma_luminance, o->sigma_normal, o->sigma_depth};
  for (float v : sg)
    if (!(v > 0.0f && v <= 3.4028234663852886e38f)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_denoise_options: every sigma must be finite and > 0");
  r->denoise = *o;
  return PT_OK;
}

extern "C" void pt_default_despeckle_options(pt_despeckle_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->threshold = 2.0f;
}

// (the options are checked before the renderer, as dev_set_adaptive_options)
int dev_set_despeckle_options(pt_renderer* r, const pt_despeckle_options* o) {
  if (!o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!(o->threshold >= 1.0f && o->threshold <= 3.4028234663852886e38f))
    return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_despeckle_options: threshold must be finite and >= 1");
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_despeckle_options: null renderer");
  r->despeckle = *o;
  return PT_OK;
}

// The filter over `colour` (the accumulator, or the film in its place: the guides, counts, region, options and firefly clamp are the same)
// into r->denoised, enqueued on the renderer's stream (denoise.hip).  Samples pending are enqueued first.
static int enqueue_denoise(pt_renderer* r, const vec4* colour) {
  { const int rc = flush_pending(r, true); if (rc != PT_OK) return rc; }
  const size_t npix = (size_t)r->S.width * r->S.height;
  PT_HIP(r->denoised.alloc(npix));
  if (r->region) PT_HIP(hipMemsetAsync(r->denoised.p, 0, sizeof(vec4) * npix, r->stream));   // the filter writes the region only
  if (r->denoise.iterations) {
    PT_HIP(r->dn_guide.alloc(npix)); PT_HIP(r->dn_aux.alloc(npix));
    PT_HIP(r->dn_col[0].alloc(npix)); PT_HIP(r->dn_col[1].alloc(npix));
  }
  DenoiseParams P;
  P.W = r->S.width; P.H = r->S.height;
  P.sigma_l = r->denoise.sigma_luminance; P.sigma_n = fminf(r->denoise.sigma_normal, kDnSigmaNormalMax); P.sigma_z = r->denoise.sigma_depth;
  launch_denoise(r->stream, colour, r->aov_img.p, r->aov_img.p + npix, r->aov_img.p + 2 * npix, P.W, P.H, (uint32_t)r->launched, P,
                 r->denoise.iterations, r->dn_guide.p, r->dn_aux.p, r->dn_col[0].p, r->dn_col[1].p, r->denoised.p,
                 r->adaptive ? r->ad_tile_n.p : nullptr,   // an adaptive render: each pixel's own sample count
                 r->rect,                                    // a region render: the region as an image of its own
                 r->despeckle);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

// (whatever denoise.apply_to_target says: the render keeps AOVs, so the filter can run)
int dev_read_denoised(pt_renderer* r, float* rgba_out) {
  if (!r || !rgba_out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started || !r->aov) return fail(PT_ERR_BAD_STATE, "pt_read_denoised: the render was not started with AOVs enabled");
  int rc = dev_wait(r);
  if (rc != PT_OK) return rc;
  if ((rc = enqueue_denoise(r, r->acc)) != PT_OK) return rc;
  PT_HIP(hipStreamSynchronize(r->stream));
  PT_HIP(hipMemcpy(rgba_out, r->denoised.p, sizeof(vec4) * (size_t)r->S.width * r->S.height, hipMemcpyDeviceToHost));
  return PT_OK;
}

// ---- auto exposure (exposure.hip) ----
extern "C" void pt_default_exposure_options(pt_exposure_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->target_log2 = -2.4739313f;   // log2 0.18
  o->low_fraction = 0.10f; o->high_fraction = 0.95f;
  o->min_ev = -16.0f; o->max_ev = 16.0f;
}

// (the options are checked before the renderer, as dev_set_adaptive_options)
int dev_set_exposure_options(pt_renderer* r, const pt_exposure_options* o) {
  if (!o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (const char* why = exposure_options_error(*o)) return fail(PT_ERR_INVALID_ARGUMENT, std::string("pt_set_exposure_options: ") + why);
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_exposure_options: null renderer");
  r->exposure = *o;
  return PT_OK;
}

// the record, allocated and cleared (no previous ev) on first use
static int exposure_record(pt_renderer* r) {
  if (r->exp_rec.p) return PT_OK;
  PT_HIP(r->exp_rec.alloc(1));
  PT_HIP(hipMemsetAsync(r->exp_rec.p, 0, sizeof(ExposureRecord), r->stream));
  return PT_OK;
}

int dev_reset_exposure(pt_renderer* r) {
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->exp_rec.p) return PT_OK;   // nothing metered yet: nothing to forget
  PT_HIP(hipSetDevice(r->device));
  PT_HIP(hipMemsetAsync(&r->exp_rec.p->has_prev, 0, sizeof(uint32_t), r->stream));
  return PT_OK;
}

// The meter ahead of the post-process, enqueued on the renderer's stream: meters *src over the render's rectangle, advances the smoothing
// state, writes *src * gain into the scratch image and points *src at it.
static int enqueue_exposure(pt_renderer* r, const vec4** src) {
  const size_t npix = (size_t)r->S.width * r->S.height;
  { const int rc = exposure_record(r); if (rc != PT_OK) return rc; }
  PT_HIP(r->exp_img.alloc(npix));
  PT_HIP(launch_exposure_meter(r->stream, *src, r->S.width, r->rect, r->exposure, r->exp_rec.p, true));
  launch_exposure_apply(r->stream, *src, r->exp_img.p, (uint32_t)npix, r->exp_rec.p);
  PT_HIP(hipGetLastError());
  *src = r->exp_img.p;
  return PT_OK;
}

// the three kernels on an uploaded image, with a record of its own (no smoothing state); the renderer's own state is untouched
int dev_debug_exposure(pt_renderer* r, const float* rgba, uint32_t width, uint32_t height, const uint32_t* rect, const pt_exposure_options* options,
                       pt_exposure_meter* out, float* scaled_out) {
  if (!options || !rgba || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (const char* why = exposure_options_error(*options)) return fail(PT_ERR_INVALID_ARGUMENT, std::string("pt_debug_exposure: ") + why);
  if (width == 0 || height == 0 || (uint64_t)width * height > (1ull << 28)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_exposure: the image must hold 1..2^28 pixels");
  Rect rc{0u, 0u, width, height};
  if (rect) {
    rc = Rect{rect[0], rect[1], rect[2], rect[3]};
    if (rc.x0 >= rc.x1 || rc.y0 >= rc.y1 || rc.x1 > width || rc.y1 > height) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_exposure: the rectangle is empty or does not fit the image");
  }
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_exposure: null renderer");
  PT_HIP(hipSetDevice(r->device));
  const size_t npix = (size_t)width * height;
  DevBuf<vec4> img, scaled;
  DevBuf<ExposureRecord> rec;
  PT_HIP(img.alloc(npix)); PT_HIP(scaled.alloc(npix)); PT_HIP(rec.alloc(1));
  PT_HIP(hipMemcpyAsync(img.p, rgba, sizeof(vec4) * npix, hipMemcpyHostToDevice, r->stream));
  PT_HIP(hipMemsetAsync(rec.p, 0, sizeof(ExposureRecord), r->stream));
  PT_HIP(launch_exposure_meter(r->stream, img.p, width, rc, *options, rec.p, false));
  launch_exposure_apply(r->stream, img.p, scaled.p, (uint32_t)npix, rec.p);
  PT_HIP(hipGetLastError());
  PT_HIP(hipStreamSynchronize(r->stream));
  PT_HIP(hipMemcpy(out, &rec.p->meter, sizeof(*out), hipMemcpyDeviceToHost));
  if (scaled_out) PT_HIP(hipMemcpy(scaled_out, scaled.p, sizeof(vec4) * npix, hipMemcpyDeviceToHost));
  return PT_OK;
}

// ---- bloom (bloom.hip) ----
extern "C" void pt_default_bloom_options(pt_bloom_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->intensity = 0.05f;
  o->scatter = 1.0f;
  o->levels = 6u;
}

// (the options are checked before the renderer, as dev_set_exposure_options)
int dev_set_bloom_options(pt_renderer* r, const pt_bloom_options* o) {
  if (!o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (const char* why = bloom_options_error(*o)) return fail(PT_ERR_INVALID_ARGUMENT, std::string("pt_set_bloom_options: ") + why);
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_bloom_options: null renderer");
  r->bloom = *o;
  return PT_OK;
}

extern "C" int pt_plan_bloom(uint32_t width, uint32_t height, uint32_t levels, pt_bloom_plan* out) {
  if (!out) return fail(PT_ERR_INVALID_ARGUMENT, "pt_plan_bloom: null argument");
  if (width == 0 || height == 0 || (uint64_t)width * height > (1ull << 28)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_plan_bloom: the image must hold 1..2^28 pixels");
  if (levels < 1u || levels > PT_BLOOM_MAX_LEVELS) return fail(PT_ERR_INVALID_ARGUMENT, "pt_plan_bloom: 1 <= levels <= 12 is required");
  bloom_plan(width, height, levels, out);
  return PT_OK;
}

// Bloom ahead of the post-process, enqueued on the renderer's stream: blooms the full frame *src into the scratch image and points *src
// at it.  (*src is the accumulator, the denoised image, a group's merged image or the auto-exposed image, never bloom_img itself.)
static int enqueue_bloom(pt_renderer* r, const vec4** src) {
  pt_bloom_plan plan;
  bloom_plan(r->S.width, r->S.height, r->bloom.levels, &plan);
  PT_HIP(r->bloom_img.alloc((size_t)r->S.width * r->S.height));
  PT_HIP(r->bloom_pyr.alloc(plan.total_texels ? plan.total_texels : 1u));
  PT_HIP(launch_bloom(r->stream, *src, r->bloom_img.p, r->bloom_pyr.p, plan, r->bloom));
  *src = r->bloom_img.p;
  return PT_OK;
}

// the same launches on an uploaded image, with buffers of its own; the renderer's own state is untouched
int dev_debug_bloom(pt_renderer* r, const float* rgba, uint32_t width, uint32_t height, const pt_bloom_options* options, float* out, float* pyramid_out) {
  if (!options || !rgba || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (const char* why = bloom_options_error(*options)) return fail(PT_ERR_INVALID_ARGUMENT, std::string("pt_debug_bloom: ") + why);
  if (width == 0 || height == 0 || (uint64_t)width * height > (1ull << 28)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_bloom: the image must hold 1..2^28 pixels");
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_bloom: null renderer");
  PT_HIP(hipSetDevice(r->device));
  const size_t npix = (size_t)width * height;
  pt_bloom_plan plan;
  bloom_plan(width, height, options->levels, &plan);
  DevBuf<vec4> img, bloomed, pyr;
  PT_HIP(img.alloc(npix)); PT_HIP(bloomed.alloc(npix)); PT_HIP(pyr.alloc(plan.total_texels ? plan.total_texels : 1u));
  PT_HIP(hipMemcpyAsync(img.p, rgba, sizeof(vec4) * npix, hipMemcpyHostToDevice, r->stream));
  PT_HIP(launch_bloom(r->stream, img.p, bloomed.p, pyr.p, plan, *options));
  PT_HIP(hipStreamSynchronize(r->stream));
  PT_HIP(hipMemcpy(out, bloomed.p, sizeof(vec4) * npix, hipMemcpyDeviceToHost));
  if (pyramid_out && plan.total_texels) PT_HIP(hipMemcpy(pyramid_out, pyr.p, sizeof(vec4) * plan.total_texels, hipMemcpyDeviceToHost));
  return PT_OK;
}

// ---- the selection overlay (selection.hip) ----
extern "C" void pt_default_selection_options(pt_selection_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->layer = PT_MATTE_INSTANCE;
  o->width = 2.0f;
  o->outline_rgba[0] = 1.0f; o->outline_rgba[1] = 0.55f; o->outline_rgba[2] = 0.0f; o->outline_rgba[3] = 1.0f;
  o->fill_rgba[0] = 1.0f; o->fill_rgba[1] = 0.55f; o->fill_rgba[2] = 0.0f; o->fill_rgba[3] = 0.0f;
}

// (the options are checked before the renderer, as dev_set_bloom_options)
int dev_set_selection_options(pt_renderer* r, const pt_selection_options* o) {
  if (!o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (const char* why = selection_options_error(*o)) return fail(PT_ERR_INVALID_ARGUMENT, std::string("pt_set_selection_options: ") + why);
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_selection_options: null renderer");
  r->selection = *o;
  return PT_OK;
}

// The set goes to the overlay's own device array behind everything enqueued so far (a present enqueued earlier draws the earlier set) and
// the copy is waited for, as dev_read_matte waits for its own: the host array it reads is the renderer's.
int dev_set_selection(pt_renderer* r, const uint32_t* ids, uint32_t id_count) {
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_selection: null renderer");
  if (id_count && !ids) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_selection: null id set");
  std::vector<uint32_t> set = matte_id_set(ids, id_count);
  if (!set.empty()) {
    PT_HIP(hipSetDevice(r->device));
    if (set.size() > r->sel_ids.cap) PT_HIP(hipStreamSynchronize(r->stream));   // (the array is replaced: nothing enqueued may still read it)
    PT_HIP(r->sel_ids.alloc(set.size()));
    PT_HIP(hipMemcpyAsync(r->sel_ids.p, set.data(), sizeof(uint32_t) * set.size(), hipMemcpyHostToDevice, r->stream));
    PT_HIP(hipStreamSynchronize(r->stream));
  }
  r->sel_set.swap(set);
  return PT_OK;
}

int dev_get_selection(const pt_renderer* r, uint32_t* ids_out, uint32_t capacity, uint32_t* count) {
  if (!r || !count || (capacity && !ids_out)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_get_selection: null argument");
  *count = (uint32_t)r->sel_set.size();
  const size_t n = std::min<size_t>(capacity, r->sel_set.size());
  if (n) memcpy(ids_out, r->sel_set.data(), sizeof(uint32_t) * n);
  return PT_OK;
}

// Is there an overlay to draw on this render's target?
static bool selection_drawn(const pt_renderer* r) { return r->selection.enabled && r->matte && !r->sel_set.empty(); }

// The overlay after the post-process, enqueued on the renderer's stream: the set's coverage resolved as dev_read_matte resolves it, into
// the overlay's own image, then drawn onto r->render_target in place.
static int enqueue_selection(pt_renderer* r) {
  PT_HIP(r->sel_cov.alloc((size_t)r->S.width * r->S.height));
  launch_matte_resolve(r->stream, r->matte_slots.p, r->selection.layer, r->sel_ids.p, (uint32_t)r->sel_set.size(), r->vtiles ? r->ad_tile_n.p : nullptr,
                       (uint32_t)r->launched, r->rect, r->S.width, r->S.height, r->sel_cov.p);
  launch_selection_overlay(r->stream, r->render_target.p, r->sel_cov.p, r->S.width, r->S.height, r->selection);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

// the overlay kernel on an uploaded target and coverage image, with buffers of its own; the renderer's own state is untouched
int dev_debug_selection_overlay(pt_renderer* r, const uint8_t* rgba8_in, const float* coverage, uint32_t width, uint32_t height,
                                const pt_selection_options* options, uint8_t* rgba8_out) {
  if (!options || !rgba8_in || !coverage || !rgba8_out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (const char* why = selection_options_error(*options)) return fail(PT_ERR_INVALID_ARGUMENT, std::string("pt_debug_selection_overlay: ") + why);
  if (width == 0 || height == 0 || (uint64_t)width * height > (1ull << 28))
    return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_selection_overlay: the image must hold 1..2^28 pixels");
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_selection_overlay: null renderer");
  PT_HIP(hipSetDevice(r->device));
  const size_t npix = (size_t)width * height;
  DevBuf<uint32_t> target;
  DevBuf<float> cov;
  PT_HIP(target.alloc(npix)); PT_HIP(cov.alloc(npix));
  PT_HIP(hipMemcpyAsync(target.p, rgba8_in, 4 * npix, hipMemcpyHostToDevice, r->stream));
  PT_HIP(hipMemcpyAsync(cov.p, coverage, sizeof(float) * npix, hipMemcpyHostToDevice, r->stream));
  launch_selection_overlay(r->stream, target.p, cov.p, width, height, *options);
  PT_HIP(hipGetLastError());
  PT_HIP(hipStreamSynchronize(r->stream));
  PT_HIP(hipMemcpy(rgba8_out, target.p, 4 * npix, hipMemcpyDeviceToHost));
  return PT_OK;
}

// ---- the film's options (film.hip; the film itself is the driver's, renderer.hip) ----
extern "C" void pt_default_film_options(pt_film_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->backdrop = PT_BACKDROP_SCENE;
}

// (the options are checked before the renderer, as dev_set_selection_options)
int dev_set_film_options(pt_renderer* r, const pt_film_options* o) {
  if (!o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (const char* why = film_options_error(*o)) return fail(PT_ERR_INVALID_ARGUMENT, std::string("pt_set_film_options: ") + why);
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_film_options: null renderer");
  r->film_opts = *o;
  return PT_OK;
}

// ---- pass views (view.hip) ----
extern "C" void pt_default_view_options(pt_view_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->view = PT_VIEW_BEAUTY; o->layer = PT_MATTE_INSTANCE; o->ramp = PT_RAMP_GREY;
  o->auto_range = 1u;
  o->depth_min = 0.0f; o->depth_max = 1.0f;
  o->noise_max = 0.1f;
}

// (the options are checked before the renderer, as dev_set_film_options)
int dev_set_view_options(pt_renderer* r, const pt_view_options* o) {
  if (!o) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (const char* why = view_options_error(*o)) return fail(PT_ERR_INVALID_ARGUMENT, std::string("pt_set_view_options: ") + why);
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_set_view_options: null renderer");
  r->view_opts = *o;
  return PT_OK;
}

// The view this render's target shows now: the one asked for when the render keeps its data, else the beauty (a group's merged image always).
static uint32_t view_now(const pt_renderer* r, const vec4* merged) {
  return view_shown(r->view_opts.view, r->aov, r->film, r->matte, r->adaptive, merged != nullptr);
}

// what the render keeps, as the view kernels read it: the pixel's n as dev_read_sample_counts gives it
static ViewImages view_images(const pt_renderer* r) {
  const size_t npix = (size_t)r->S.width * r->S.height;
  ViewImages I{};
  if (r->aov) { I.normal = r->aov_img.p + PT_AOV_NORMAL * npix; I.moments = r->aov_img.p + PT_AOV_MOMENTS * npix; }
  if (r->adaptive) I.mom2 = r->ad_mom.p;
  if (r->film) I.film = r->film_img.p;
  if (r->matte) { I.slots = r->matte_slots.p + r->view_opts.layer * (kMatteSlots / 2u); I.slot_stride = kMattePixelVec4; }
  I.tile_n = r->vtiles ? r->ad_tile_n.p : nullptr;
  I.n_uniform = (uint32_t)r->launched;
  I.rect = r->rect;
  I.width = r->S.width; I.height = r->S.height;
  return I;
}

// the record, allocated on first use
static int view_record(pt_renderer* r) {
  if (r->view_rec.p) return PT_OK;
  PT_HIP(r->view_rec.alloc(1));
  return PT_OK;
}

// A data view in place of source, exposure, bloom, post-process and the film's alpha byte, enqueued on the renderer's stream: the depth
// range first when the view asks for the frame's own (the record stays on the device: present does not block), then k_view_pass into
// r->render_target.
static int enqueue_view(pt_renderer* r, uint32_t view) {
  const size_t npix = (size_t)r->S.width * r->S.height;
  if (r->render_target.n != npix) PT_HIP(r->render_target.alloc(npix));
  const ViewImages I = view_images(r);
  ViewParams P = view_params(r->view_opts, r->params.spp);
  P.view = view;
  if (view == PT_VIEW_DEPTH && P.auto_range) {
    if (const int rc = view_record(r)) return rc;
    PT_HIP(launch_view_range(r->stream, I, r->view_rec.p, false));
  }
  launch_view_pass(r->stream, I, P, r->view_rec.p, r->render_target.p);
  PT_HIP(hipGetLastError());
  return PT_OK;
}

// What a target read would show now, and under DEPTH the range it would use: the range pass alone, waited for.  Nothing is drawn.
int dev_read_view_stats(pt_renderer* r, const vec4* merged, pt_view_stats* out) {
  if (!r || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "pt_read_view_stats before pt_start_render");
  if (merged) PT_HIP(hipSetDevice(r->device));
  else if (const int rc = dev_wait(r)) return rc;
  memset(out, 0, sizeof(*out));
  out->shown = view_now(r, merged);
  if (out->shown != PT_VIEW_DEPTH) return PT_OK;
  if (const int rc = view_record(r)) return rc;
  PT_HIP(launch_view_range(r->stream, view_images(r), r->view_rec.p, true));
  PT_HIP(hipStreamSynchronize(r->stream));
  ViewRecord rec;
  PT_HIP(hipMemcpy(&rec, r->view_rec.p, sizeof(rec), hipMemcpyDeviceToHost));
  out->depth_pixels = rec.count;
  view_range(view_params(r->view_opts, r->params.spp), rec, &out->depth_min, &out->depth_max);
  return PT_OK;
}

// the two kernels on uploaded inputs, with buffers and a record of their own; the renderer's own state is untouched
int dev_debug_view(pt_renderer* r, const pt_view_inputs* in, uint32_t width, uint32_t height, const uint32_t* rect, const pt_view_options* options,
                   uint8_t* rgba8_out, pt_view_stats* stats_out) {
  if (!options || !in || !rgba8_out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (const char* why = view_options_error(*options)) return fail(PT_ERR_INVALID_ARGUMENT, std::string("pt_debug_view: ") + why);
  const uint32_t view = options->view;
  if (!view_is_data(view)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_view: BEAUTY and ALBEDO go through the post-process, not through a view kernel");
  if (width == 0 || height == 0 || (uint64_t)width * height > (1ull << 28)) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_view: the image must hold 1..2^28 pixels");
  Rect rc{0u, 0u, width, height};
  if (rect) {
    rc = Rect{rect[0], rect[1], rect[2], rect[3]};
    if (rc.x0 >= rc.x1 || rc.y0 >= rc.y1 || rc.x1 > width || rc.y1 > height) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_view: the rectangle is empty or does not fit the image");
  }
  const bool reads_normal = view == PT_VIEW_NORMAL || view == PT_VIEW_DEPTH, reads_moments = view == PT_VIEW_DEPTH || view == PT_VIEW_NOISE;
  if (!in->counts || (reads_normal && !in->normal) || (reads_moments && !in->moments) || (view == PT_VIEW_ALPHA && !in->film) ||
      (view == PT_VIEW_MATTE && !in->slots))
    return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_view: a null input that the view reads");
  if (view == PT_VIEW_SAMPLES && in->spp == 0u) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_view: SAMPLES needs spp >= 1");
  if (!r) return fail(PT_ERR_INVALID_ARGUMENT, "pt_debug_view: null renderer");
  PT_HIP(hipSetDevice(r->device));
  const size_t npix = (size_t)width * height;
  DevBuf<vec4> normal, moments, film;
  DevBuf<uint4> slots;
  DevBuf<uint32_t> counts, target;
  DevBuf<ViewRecord> rec;
  ViewImages I{};
  PT_HIP(counts.alloc(npix)); PT_HIP(target.alloc(npix)); PT_HIP(rec.alloc(1));
  PT_HIP(hipMemcpyAsync(counts.p, in->counts, sizeof(uint32_t) * npix, hipMemcpyHostToDevice, r->stream));
  const auto upload = [&](DevBuf<vec4>& b, const float* src, const vec4** dst) -> int {
    PT_HIP(b.alloc(npix));
    PT_HIP(hipMemcpyAsync(b.p, src, sizeof(vec4) * npix, hipMemcpyHostToDevice, r->stream));
    *dst = b.p;
    return PT_OK;
  };
  if (reads_normal) { if (const int e = upload(normal, in->normal, &I.normal)) return e; }
  if (reads_moments) { if (const int e = upload(moments, in->moments, &I.moments)) return e; }
  if (view == PT_VIEW_ALPHA) { if (const int e = upload(film, in->film, &I.film)) return e; }
  if (view == PT_VIEW_MATTE) {
    PT_HIP(slots.alloc(npix * (kMatteSlots / 2u)));
    PT_HIP(hipMemcpyAsync(slots.p, in->slots, sizeof(pt_matte_slot) * kMatteSlots * npix, hipMemcpyHostToDevice, r->stream));
    I.slots = slots.p; I.slot_stride = kMatteSlots / 2u;
  }
  I.counts = counts.p;
  I.rect = rc;
  I.width = width; I.height = height;
  const ViewParams P = view_params(*options, in->spp);
  if (view == PT_VIEW_DEPTH) PT_HIP(launch_view_range(r->stream, I, rec.p, true));
  else PT_HIP(hipMemsetAsync(rec.p, 0, sizeof(ViewRecord), r->stream));
  launch_view_pass(r->stream, I, P, rec.p, target.p);
  PT_HIP(hipGetLastError());
  PT_HIP(hipStreamSynchronize(r->stream));
  PT_HIP(hipMemcpy(rgba8_out, target.p, 4 * npix, hipMemcpyDeviceToHost));
  if (stats_out) {
    ViewRecord h;
    PT_HIP(hipMemcpy(&h, rec.p, sizeof(h), hipMemcpyDeviceToHost));
    memset(stats_out, 0, sizeof(*stats_out));
    stats_out->shown = view;
    if (view == PT_VIEW_DEPTH) { stats_out->depth_pixels = h.count; view_range(P, h, &stats_out->depth_min, &stats_out->depth_max); }
  }
  return PT_OK;
}

// ---- the display chain.  Everything is enqueued on r->stream; the callers below decide what is waited for. ----

// The image the chain starts from: a group's merged image when one is given, else the denoised image (its filter enqueued here) of a
// render that keeps AOVs and applies it to the target, else the accumulator.
// Under a backdrop other than PT_BACKDROP_SCENE a render that keeps a film (never a group's merged image) starts from the film composed
// over the backdrop instead (k_film_compose into r->film_src): base = film.rgb, or the same filter run over the film.
static bool backdrop_shown(const pt_renderer* r, const vec4* merged) { return !merged && r->film && r->film_opts.backdrop != PT_BACKDROP_SCENE; }

static int display_source(pt_renderer* r, const vec4* merged, const vec4** src) {
  *src = merged ? merged : r->acc;
  const bool backdrop = backdrop_shown(r, merged);
  const vec4* base = backdrop ? r->film_img.p : r->acc;
  if (!merged && r->aov && r->denoise.apply_to_target) {
    if (const int rc = enqueue_denoise(r, base)) return rc;
    *src = base = r->denoised.p;
  }
  if (!backdrop) return PT_OK;
  PT_HIP(r->film_src.alloc((size_t)r->S.width * r->S.height));
  launch_film_compose(r->stream, base, r->film_img.p, r->film_src.p, r->S.width, r->S.height, r->rect, r->film_opts);
  PT_HIP(hipGetLastError());
  *src = r->film_src.p;
  return PT_OK;
}

// Source, auto exposure, bloom, post-process into r->render_target, the film's alpha byte and the selection overlay onto it: one step of the exposure smoothing state
// per call, and nothing allocated or launched for a stage that is disabled.  (A group's merged image gets no overlay: a group keeps no mattes.)
// Pass views.  BEAUTY: the chain as above.  A data view: k_view_pass writes the target in place of everything up to the
// overlay, which still draws on top; the exposure smoothing state does not advance.  ALBEDO: the albedo AOV is the source, auto exposure and
// bloom are skipped (the state does not advance either) and no alpha byte is written: the composed film is not made.
static int enqueue_display(pt_renderer* r, const vec4* merged) {
  const uint32_t view = view_now(r, merged);
  const size_t npix = (size_t)r->S.width * r->S.height;
  if (view_is_data(view)) {
    if (const int rc = enqueue_view(r, view)) return rc;
    if (selection_drawn(r)) { const int rc = enqueue_selection(r); if (rc != PT_OK) return rc; }
    return PT_OK;
  }
  const vec4* src;
  if (view == PT_VIEW_ALBEDO) src = r->aov_img.p + PT_AOV_ALBEDO * npix;
  else {
    if (const int rc = display_source(r, merged, &src)) return rc;
    if (r->exposure.enabled) { const int rc = enqueue_exposure(r, &src); if (rc != PT_OK) return rc; }
    if (r->bloom.enabled) { const int rc = enqueue_bloom(r, &src); if (rc != PT_OK) return rc; }
  }
  if (r->render_target.n != npix) PT_HIP(r->render_target.alloc(npix));
  PostConstants pc;
  pc.post = r->post;
  pc.tm = r->tonemap;
  const Mat3 odt = compute_transform(r->params.working_space, r->tonemap.output_space);  // renderer_pt.cpp:190-191
  pc.odt = PPMat3{odt.c0, odt.c1, odt.c2};
  launch_postprocess(r->stream, src, r->render_target.p, r->S.width, r->S.height, pc);
  PT_HIP(hipGetLastError());
  // transparent film: the alpha byte from the composed source, before the overlay (which leaves alpha alone)
  if (view == PT_VIEW_BEAUTY && backdrop_shown(r, merged) && r->film_opts.backdrop == PT_BACKDROP_TRANSPARENT) {
    launch_film_alpha(r->stream, r->render_target.p, r->film_src.p, (uint32_t)npix);
    PT_HIP(hipGetLastError());
  }
  if (!merged && selection_drawn(r)) { const int rc = enqueue_selection(r); if (rc != PT_OK) return rc; }
  return PT_OK;
}

// Enqueue only: the image shows every sample accepted so far, and the caller orders its reads behind *stream_out.  Present never blocks,
// so unlike the reads below it does not wait for an adaptive render's checkpoints (flush_pending without sync_checkpoints, not dev_wait).
int dev_present(pt_renderer* r, const vec4* merged, void** device_rgba8_out, void** stream_out) {
  if (!r || !device_rgba8_out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "pt_present_render_target before pt_start_render");
  PT_HIP(hipSetDevice(r->device));
  { const int rc = flush_pending(r, true); if (rc != PT_OK) return rc; }
  if (const int rc = enqueue_display(r, merged)) return rc;
  *device_rgba8_out = r->render_target.p;
  if (stream_out) *stream_out = (void*)r->stream;
  return PT_OK;
}

// The blocking read.  A single device waits for its render (dev_wait: every checkpoint included); a group has waited for its members and
// hands in their merged image.
int dev_read_render_target(pt_renderer* r, const vec4* merged, uint8_t* rgba8_out) {
  if (!r || !rgba8_out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "pt_read_render_target before pt_start_render");
  if (merged) PT_HIP(hipSetDevice(r->device));
  else if (const int rc = dev_wait(r)) return rc;
  if (const int rc = enqueue_display(r, merged)) return rc;
  PT_HIP(hipStreamSynchronize(r->stream));
  PT_HIP(hipMemcpy(rgba8_out, r->render_target.p, (size_t)r->S.width * r->S.height * 4, hipMemcpyDeviceToHost));
  return PT_OK;
}

// What enqueue_display would meter now: the same source, the histogram with for_target = false (the smoothing state stays as it is),
// and nothing after it: no scaling, no bloom.
int dev_read_exposure_meter(pt_renderer* r, const vec4* merged, pt_exposure_meter* out) {
  if (!r || !out) return fail(PT_ERR_INVALID_ARGUMENT, "null argument");
  if (!r->started) return fail(PT_ERR_BAD_STATE, "pt_read_exposure_meter before pt_start_render");
  PT_HIP(hipSetDevice(r->device));
  int rc = dev_wait(r);
  if (rc != PT_OK) return rc;
  const vec4* src;
  if ((rc = display_source(r, merged, &src)) != PT_OK) return rc;
  if ((rc = exposure_record(r)) != PT_OK) return rc;
  PT_HIP(launch_exposure_meter(r->stream, src, r->S.width, r->rect, r->exposure, r->exp_rec.p, false));
  PT_HIP(hipStreamSynchronize(r->stream));
  PT_HIP(hipMemcpy(out, &r->exp_rec.p->meter, sizeof(*out), hipMemcpyDeviceToHost));
  return PT_OK;
}
