/* ptamd_renderer.hpp — the C++ face of libptamd.so: a header-only class with the public members of the reference's
 * pt::renderer_pt::Renderer (/root/reference/src/renderer_pt/renderer_pt.hpp:14-73), implemented over the C ABI of
 * ptamd.h.  It is what a Linux/ROCm build of the reference's frontend would compile instead of renderer_pt.cpp
 * (INTEGRATION.md shows the Store-walking half of that file); here it is also the C++ host side the parity tests drive
 * (tests/cpp/shim_render.cpp).
 *
 *   reference member (renderer_pt.hpp)                          here
 *   Renderer(MTL::Device*, MTL::CommandQueue*, Store&) noexcept  Renderer(int device) / Renderer(std::vector<int> devices) noexcept
 *   ~Renderer()                                            :34   ~Renderer()
 *   void render()                                          :36   void render()                 one sample per call (merged into batches by the
 *                                                                                               library while the GPU is busy), returns at once
 *   void startRender(cameraNodeId, viewportSize, sampleCount,
 *                    gmonBuckets, workingSpace, flags = 0) :38   void startRender(scene, viewportSize, sampleCount, gmonBuckets,
 *                                                                                 workingSpace, flags = 0)
 *        (the Store& of the constructor and the camera node become the flat pt_scene_snapshot, which names its camera)
 *   selectedKernel() / selectKernel(uint32_t)              :47   the same; enum class Integrators { Simple, MIS }   :16-19
 *   const MTL::Texture* presentRenderTarget() const        :55   const void* presentRenderTarget() const   RGBA8 in device memory
 *   NS::SharedPtr<MTL::Buffer> readbackRenderTarget(uint2*) :57  std::vector<uint8_t> readbackRenderTarget(uint2*) const   blocks
 *   int status() const                                     :59   the same bits: Status_Blocked/Ready/Busy/Done      :21-26
 *   std::pair<size_t, size_t> renderProgress() const       :61   the same
 *   size_t renderTime() const                              :63   the same (milliseconds)
 *   std::vector<postprocess::PostProcessPass::Options>
 *     postProcessOptions()                              :65      the same: one tagged pointer per pass (Exposure, ChromaticAberration,
 *                                                                ContrastSaturation, ToneCurve, Vignette — the order of renderer_pt.cpp:343-352)
 *                                                                into option structs this object owns (ptamd_postprocess.hpp)
 *   postprocess::Tonemap::Options* tonemapOptions()     :67      the same: TonemapOptions with agxOptions.look / khrOptions / flimOptions / postTonemap
 *   shaders_pt::GmonOptions& gmonOptions()              :71      pt_gmon_options& (the one member, `cap`)
 *   color::Colorspace& outputColorspace()               :73      pt_colorspace& (the four chromaticity pairs a color::Colorspace is built from)
 *        the caller edits them in place; they are flattened and handed to the library whenever an image is asked for (the reference's
 *        passes read theirs when they are encoded)
 *   (no counterpart)                                             pt_denoise_options& denoiseOptions() / setDenoiseOptions(...), readbackAov(kind),
 *                                                                readbackDenoised(): first-hit AOVs and the a-trous denoiser (ptamd.h, ABI 5);
 *                                                                `enabled` is handed over at startRender, the rest whenever an image is asked for
 *   (no counterpart)                                             pt_despeckle_options& despeckleOptions() / setDespeckleOptions(...): the firefly
 *                                                                clamp ahead of the filter (ptamd.h, ABI 5 extension); handed over whenever an
 *                                                                image is asked for
 *   (no counterpart)                                             pt_exposure_options& exposureOptions(), resetExposure(), readExposureMeter(): auto
 *                                                                exposure, a luminance-histogram meter ahead of the post-process (ptamd.h, ABI 5
 *                                                                extension); handed over whenever a target is asked for
 *   (no counterpart)                                             pt_bloom_options& bloomOptions(): bloom, an energy-conserving glare pyramid ahead of
 *                                                                the post-process (ptamd.h, ABI 5 extension); handed over whenever a target is
 *                                                                asked for
 *   (no counterpart)                                             pt_adaptive_options& adaptiveOptions() / setAdaptiveOptions(...),
 *                                                                readbackSampleCounts(): tile-adaptive sampling (ptamd.h, ABI 5 extension);
 *                                                                handed over at startRender
 *   (no counterpart)                                             pt_render_region& renderRegion() / setRenderRegion(...): sample only a pixel
 *                                                                rectangle of the frame (ptamd.h, ABI 5 extension); handed over at startRender
 *   (no counterpart; the raster viewport's selection only)       pt_matte_options& matteOptions(), readbackMatteSlots(), readbackMatte(), pick():
 *                                                                ID mattes, per-pixel instance and material coverage of the camera rays' first
 *                                                                hits (ptamd.h, ABI 5 extension); handed over at startRender
 *   (no counterpart; the raster viewport's selection outline)    pt_selection_options& selectionOptions(), setSelection(ids), selection(): an outline
 *                                                                around and a tint over the selected ids, drawn onto the target after the
 *                                                                post-process (ptamd.h, ABI 5 extension); the options are handed over whenever a
 *                                                                target is asked for, the ids at once
 *   (no counterpart; "film transparent" of other path tracers)   pt_film_options& filmOptions() / setFilmOptions(...), readbackFilm(): the foreground
 *                                                                with alpha, and the backdrop a target shows behind it (ptamd.h, ABI 5 extension);
 *                                                                `enabled` is handed over at startRender, the backdrop whenever a target is asked for
 *   (no counterpart; the "ambient occlusion" pass of a compositor) pt_ao_options& ambientOcclusionOptions() / setAmbientOcclusionOptions(...),
 *                                                                readbackAmbientOcclusion(), readbackAmbientOcclusionCounts(), debugAmbientOcclusion():
 *                                                                one occlusion ray from every camera ray's first hit (ptamd.h, ABI 5 extension);
 *                                                                handed over at startRender
 *   (no counterpart; the camera type of a scene editor)           pt_camera_projection& projection() / setProjection(...), renderProjection(): orthographic,
 *                                                                panoramic and fisheye cameras beside the perspective one (ptamd.h, ABI 5 extension);
 *                                                                handed over at startRender
 *   (no counterpart; the "sun and sky" light of a scene editor)   generateSky(options, width, height): a single-scattering atmosphere as a lat-long
 *                                                                environment image, generated on the device (ptamd.h, ABI 5 extension)
 *   (no counterpart; the "render pass" drop-down of a viewport)    pt_view_options& viewOptions(), viewStats(): what the target shows of the AOVs, the
 *                                                                mattes, the film's alpha and the sampling (ptamd.h, ABI 5 extension); handed
 *                                                                over whenever a target is asked for
 * Error behaviour as the reference's: nothing throws; a failing call prints "renderer_pt: <message>" to stderr (the
 * reference prints and asserts, renderer_pt.cpp:402, 1044) and leaves the object in Status_Blocked; lastError() keeps the text.
 * Threading as the reference's: one caller thread per Renderer.
 */
#ifndef PTAMD_RENDERER_HPP
#define PTAMD_RENDERER_HPP

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "ptamd.h"
#include "ptamd_postprocess.hpp"

namespace ptamd::renderer_pt {

struct float2 { float x, y; };
struct uint2 { uint32_t x, y; };

class Renderer {
public:
  enum class Integrators { Simple = 0, MIS };  // renderer_pt.hpp:16-19
  enum Status {                                // renderer_pt.hpp:21-26
    Status_Blocked = 0,
    Status_Ready = 1 << 0,
    Status_Busy = 1 << 2,
    Status_Done = 1 << 3,
  };

  // `device`: HIP ordinal (the reference takes the window's MTL::Device).  lutPath: the GGX energy tables
  // (loadGgxLutTextures, renderer_pt.cpp:385-446); nullptr = $PTAMD_LUT_PATH.
  explicit Renderer(int device = 0, const char* lutPath = nullptr) noexcept { create(&device, 0, device, lutPath); }
  // A device group: every render is shared by these devices (sample ranges, one RCCL reduce; ptamd.h pt_create_info).
  explicit Renderer(const std::vector<int>& devices, const char* lutPath = nullptr) noexcept {
    create(devices.data(), (uint32_t)devices.size(), devices.empty() ? 0 : devices[0], lutPath);
  }
  Renderer(const Renderer&) = delete;
  Renderer& operator=(const Renderer&) = delete;
  ~Renderer() { if (m_pt) pt_destroy(m_pt); }

  // renderer_pt.cpp:113-197 steady state: one more sample of every pixel is accepted (on EVERY device of a group: N samples);
  // does not wait.  Calls that arrive while the GPU is busy are merged into batches by the library (ptamd.h pt_render_step), so
  // a tight `while (status() & Status_Busy) render();` loop runs at the full batch rate.  A frontend that calls render() once per
  // vsync is limited to refresh-rate samples per second by that loop itself (the reference's structural ceiling, BASELINE.md §1:
  // 60 spp/s where an MI355X traces ~950 on C3); setSamplesPerRender(n) lets such a loop accept n samples per call.
  void render() {
    if (!m_pt || !m_started) return;
    check(pt_render_step(m_pt, m_samplesPerRender));
  }

  // renderer_pt.cpp:199-217 + the rebuild half of the first render() (:72-111): the scene is copied to the device, light table,
  // constants and acceleration structure are built; progress restarts at 0.  `scene` is only read during the call.
  void startRender(const pt_scene_snapshot& scene, float2 viewportSize, uint32_t sampleCount, uint32_t gmonBuckets,
                   const pt_colorspace& workingSpace, int flags = 0) {
    m_started = false;
    if (!m_pt) return;
    pt_render_params p{};
    p.width = (uint32_t)viewportSize.x;
    p.height = (uint32_t)viewportSize.y;
    p.spp = sampleCount;
    p.gmon_buckets = gmonBuckets;
    p.flags = flags;
    p.integrator = m_selectedPipeline;
    p.working_space = workingSpace;
    p.max_bounces = m_maxBounces;
    p.first_sample = m_firstSample;
    p.samples_in_flight = m_samplesInFlight;
    p.nonfinite_policy = m_nonfinitePolicy;
    p.accel_structure = m_accelStructure;
    if (!check(pt_set_denoise_options(m_pt, &m_denoise))) return;   // (`enabled` is read here)
    if (!check(pt_set_adaptive_options(m_pt, &m_adaptive))) return;  // (read here)
    if (!check(pt_set_render_region(m_pt, &m_region))) return;       // (read here)
    if (!check(pt_set_matte_options(m_pt, &m_matte))) return;        // (read here)
    if (!check(pt_set_film_options(m_pt, &m_film))) return;          // (`enabled` is read here)
    if (!check(pt_set_camera_projection(m_pt, &m_projection))) return;   // (read here)
    if (!check(pt_set_ao_options(m_pt, &m_ao))) return;              // (read here)
    if (!check(pt_start_render(m_pt, &scene, &p))) return;
    m_size = uint2{p.width, p.height};
    m_started = true;
  }

  [[nodiscard]] constexpr uint32_t selectedKernel() const { return m_selectedPipeline; }
  constexpr void selectKernel(uint32_t kernel) { m_selectedPipeline = kernel; }

  // The post-processed RGBA8 image in DEVICE memory (W*H*4 bytes; valid until the next startRender); the work is enqueued on
  // presentStream() (a hipStream_t) — order a blit after it.  nullptr on failure.
  [[nodiscard]] const void* presentRenderTarget() const {
    if (!m_pt || !m_started || !pushOptions()) return nullptr;
    void* img = nullptr;
    if (!check(pt_present_render_target(m_pt, &img, &m_presentStream))) return nullptr;
    return img;
  }
  [[nodiscard]] void* presentStream() const { return m_presentStream; }

  // renderer_pt.cpp:1039-1059: blocks until the enqueued samples are done, returns W*H*4 bytes (row-major, top-left origin).
  [[nodiscard]] std::vector<uint8_t> readbackRenderTarget(uint2* size) const {
    std::vector<uint8_t> out;
    if (size) *size = m_size;
    if (!m_pt || !m_started || !pushOptions()) return out;
    out.resize((size_t)m_size.x * m_size.y * 4);
    if (!check(pt_read_render_target(m_pt, out.data()))) out.clear();
    return out;
  }

  [[nodiscard]] int status() const { return m_pt && m_started ? pt_status(m_pt) : (int)Status_Blocked; }  // renderer_pt.cpp:1023-1031
  [[nodiscard]] std::pair<size_t, size_t> renderProgress() const {                                        // :1033-1035
    uint64_t done = 0, total = 0;
    if (m_pt && m_started) pt_progress(m_pt, &done, &total);
    return {(size_t)done, (size_t)total};
  }
  [[nodiscard]] size_t renderTime() const { return m_pt && m_started ? (size_t)pt_render_time_ms(m_pt) : 0; }  // :1037

  // Option structs the UI edits every frame (renderer_pt.hpp:65-73; types: ptamd_postprocess.hpp = core/postprocessing.hpp's shapes).
  // One entry per post-process pass, in the order the reference runs them (renderer_pt.cpp:343-352); the UI switches on `type` and edits
  // through the pointer (pt_viewport.cpp:259-335).
  [[nodiscard]] std::vector<postprocess::PostProcessPass::Options> postProcessOptions() {
    using P = postprocess::PostProcessPass;
    std::vector<P::Options> options(5);
    options[0].type = P::Type::Exposure; options[0].exposure = &m_exposure;
    options[1].type = P::Type::ChromaticAberration; options[1].chromaticAberration = &m_chromaticAberration;
    options[2].type = P::Type::ContrastSaturation; options[2].contrastSaturation = &m_contrastSaturation;
    options[3].type = P::Type::ToneCurve; options[3].toneCurve = &m_toneCurve;
    options[4].type = P::Type::Vignette; options[4].vignette = &m_vignette;
    return options;
  }
  [[nodiscard]] constexpr postprocess::Tonemap::Options* tonemapOptions() { return &m_tonemap; }
  [[nodiscard]] constexpr pt_gmon_options& gmonOptions() { return m_gmonOptions; }
  pt_colorspace& outputColorspace() { return m_outputSpace; }

  // ---- what the reference fixes at compile time or does not have (ptamd.h "NEW") ----
  // Camera projections (ptamd.h pt_camera_projection, no counterpart in the reference): how the next startRender makes its camera rays —
  // PT_PROJ_PERSPECTIVE (the reference's camera, the default), _ORTHOGRAPHIC (ortho_height), _EQUIRECT (fov_x, fov_y) or _FISHEYE
  // (fisheye_fov).  Edited in place like filmOptions(); read at startRender, which fails on options outside their ranges.
  [[nodiscard]] constexpr pt_camera_projection& projection() { return m_projection; }
  void setProjection(const pt_camera_projection& p) { m_projection = p; }
  // The projection the current render was started with; the default one when no render is.
  [[nodiscard]] pt_camera_projection renderProjection() const {
    pt_camera_projection out;
    pt_default_camera_projection(&out);
    if (m_pt && m_started) (void)check(pt_get_camera_projection(m_pt, &out));
    return out;
  }
  void setMaxBounces(uint32_t b) { m_maxBounces = b; }              // kernel.metal:5 MAX_BOUNCES = 50 (the default here too)
  void setFirstSample(uint32_t s) { m_firstSample = s; }            // frameIdx of the first sample: sample-range shards
  void setSamplesInFlight(uint32_t s) { m_samplesInFlight = s; }    // 0 = automatic
  void setSamplesPerRender(uint32_t n) { m_samplesPerRender = n ? n : 1; }  // samples one render() call accepts; 1 = the reference
  void setNonfinitePolicy(uint32_t p) { m_nonfinitePolicy = p; }    // PT_NONFINITE_*
  void setAccelStructure(uint32_t a) { m_accelStructure = a; }      // PT_ACCEL_*
  // The float accumulator (renderer_pt.cpp:812-821): W*H RGBA32F running mean, alpha 1 — the parity surface.  Blocks.
  [[nodiscard]] std::vector<float> readbackAccumulator() const {
    std::vector<float> out;
    if (!m_pt || !m_started || !check(pt_set_gmon_options(m_pt, &m_gmonOptions))) return out;  // (the resolve reads GmonOptions.cap)
    out.resize((size_t)m_size.x * m_size.y * 4);
    if (!check(pt_read_accumulator(m_pt, out.data()))) out.clear();
    return out;
  }
  // First-hit AOVs and the denoiser (ptamd.h, ABI 5).  Edited in place like gmonOptions().
  [[nodiscard]] constexpr pt_denoise_options& denoiseOptions() { return m_denoise; }
  void setDenoiseOptions(const pt_denoise_options& o) { m_denoise = o; }
  // One AOV image (PT_AOV_*), W*H RGBA32F; empty for a render started without AOVs.  Blocks.
  [[nodiscard]] std::vector<float> readbackAov(uint32_t kind) const {
    std::vector<float> out;
    if (!m_pt || !m_started || !check(pt_set_denoise_options(m_pt, &m_denoise))) return out;
    out.resize((size_t)m_size.x * m_size.y * 4);
    if (!check(pt_read_aov(m_pt, kind, out.data()))) out.clear();
    return out;
  }
  // The denoised image, W*H RGBA32F; empty for a render started without AOVs.  Blocks.
  [[nodiscard]] std::vector<float> readbackDenoised() const {
    std::vector<float> out;
    if (!m_pt || !m_started || !check(pt_set_gmon_options(m_pt, &m_gmonOptions)) || !check(pt_set_denoise_options(m_pt, &m_denoise)) ||
        !check(pt_set_despeckle_options(m_pt, &m_despeckle)))
      return out;
    out.resize((size_t)m_size.x * m_size.y * 4);
    if (!check(pt_read_denoised(m_pt, out.data()))) out.clear();
    return out;
  }
  // The firefly clamp ahead of the a-trous filter (ptamd.h, an additive extension of ABI 5).  Edited in place like denoiseOptions(); read
  // whenever a denoised image is asked for, no restart needed.
  [[nodiscard]] constexpr pt_despeckle_options& despeckleOptions() { return m_despeckle; }
  void setDespeckleOptions(const pt_despeckle_options& o) { m_despeckle = o; }
  // Auto exposure (ptamd.h, an additive extension of ABI 5): with enabled set, presentRenderTarget / readbackRenderTarget meter the image's
  // luminance histogram and scale the image to the target ahead of the post-process; the Exposure pass's stops act on top as compensation.
  // Edited in place like denoiseOptions(); read whenever a target is asked for, no restart needed.
  [[nodiscard]] constexpr pt_exposure_options& exposureOptions() { return m_autoExposure; }
  // Forgets the previously applied ev (a cut to another scene): the next target starts from its own target_ev.
  void resetExposure() { if (m_pt) check(pt_reset_exposure(m_pt)); }
  // The histogram and the ev a target asked for now would apply (a UI histogram; works with enabled = 0).  Blocks; false on failure.
  [[nodiscard]] bool readExposureMeter(pt_exposure_meter* out) const {
    return m_pt && m_started && out && check(pt_set_denoise_options(m_pt, &m_denoise)) && check(pt_set_despeckle_options(m_pt, &m_despeckle)) &&
           check(pt_set_exposure_options(m_pt, &m_autoExposure)) && check(pt_read_exposure_meter(m_pt, out));
  }
  // Bloom (ptamd.h, an additive extension of ABI 5): with enabled set, presentRenderTarget / readbackRenderTarget scatter `intensity` of the
  // light above `threshold` through a down/up image pyramid, after auto exposure and ahead of the post-process.  Edited in place like
  // denoiseOptions(); read whenever a target is asked for, no restart needed.
  [[nodiscard]] constexpr pt_bloom_options& bloomOptions() { return m_bloom; }
  // Tile-adaptive sampling (ptamd.h, an additive extension of ABI 5).  Edited in place like denoiseOptions(); read at startRender.
  [[nodiscard]] constexpr pt_adaptive_options& adaptiveOptions() { return m_adaptive; }
  void setAdaptiveOptions(const pt_adaptive_options& o) { m_adaptive = o; }
  // The samples folded into each pixel, W*H (its 8x8 tile's count; uniform for a non-adaptive render).  Blocks.
  [[nodiscard]] std::vector<uint32_t> readbackSampleCounts() const {
    std::vector<uint32_t> out;
    if (!m_pt || !m_started) return out;
    out.resize((size_t)m_size.x * m_size.y);
    if (!check(pt_read_sample_counts(m_pt, out.data()))) out.clear();
    return out;
  }
  // Render regions (ptamd.h, an additive extension of ABI 5): the next startRender samples only the pixels [x0, x1) x [y0, y1); everything
  // outside stays zero, alpha included.  Edited in place like adaptiveOptions(); enabled = 0 (the default) is the whole frame.
  [[nodiscard]] constexpr pt_render_region& renderRegion() { return m_region; }
  void setRenderRegion(const pt_render_region& o) { m_region = o; }
  void setRenderRegion(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) { m_region = pt_render_region{1u, x0, y0, x1, y1}; }
  // ID mattes (ptamd.h, an additive extension of ABI 5): a render started with enabled set keeps, per pixel, which instances and materials
  // its camera rays hit first.  Edited in place like adaptiveOptions(); read at startRender.
  [[nodiscard]] constexpr pt_matte_options& matteOptions() { return m_matte; }
  void setMatteOptions(const pt_matte_options& o) { m_matte = o; }
  // The slots of one layer (PT_MATTE_INSTANCE / PT_MATTE_MATERIAL), W*H*PT_MATTE_SLOTS; empty for a render started without mattes.  Blocks.
  [[nodiscard]] std::vector<pt_matte_slot> readbackMatteSlots(uint32_t layer) const {
    std::vector<pt_matte_slot> out;
    if (!m_pt || !m_started) return out;
    out.resize((size_t)m_size.x * m_size.y * PT_MATTE_SLOTS);
    if (!check(pt_read_matte_slots(m_pt, layer, out.data()))) out.clear();
    return out;
  }
  // Coverage of a set of ids of one layer, W*H floats in [0, 1]: a selection mask (PT_MATTE_NONE selects the background).  Blocks.
  [[nodiscard]] std::vector<float> readbackMatte(uint32_t layer, const std::vector<uint32_t>& ids) const {
    std::vector<float> out;
    if (!m_pt || !m_started) return out;
    out.resize((size_t)m_size.x * m_size.y);
    if (!check(pt_read_matte(m_pt, layer, ids.empty() ? nullptr : ids.data(), (uint32_t)ids.size(), out.data()))) out.clear();
    return out;
  }
  // What is under pixel (x, y), top-left origin ("click to select"); false on failure.  Blocks until the enqueued samples are done.
  [[nodiscard]] bool pick(uint32_t x, uint32_t y, pt_pick_result* out) const { return m_pt && m_started && out && check(pt_pick(m_pt, x, y, out)); }
  // Selection overlay (ptamd.h, an additive extension of ABI 5): with enabled set, presentRenderTarget / readbackRenderTarget of a render
  // that keeps mattes draw an outline around the pixels covered by the selected ids of `layer`, and a tint over them, after the post-process
  // (UI colours in the target's encoding).  A render without mattes and a device group silently show no overlay.  Edited in place like
  // bloomOptions(); read whenever a target is asked for, no restart needed.
  [[nodiscard]] constexpr pt_selection_options& selectionOptions() { return m_selection; }
  // The selected ids (any order, duplicates allowed, PT_MATTE_NONE = the background; empty clears); kept across startRender.  false on failure.
  bool setSelection(const std::vector<uint32_t>& ids) { return m_pt && check(pt_set_selection(m_pt, ids.empty() ? nullptr : ids.data(), (uint32_t)ids.size())); }
  // The stored selection: ascending, without duplicates.
  [[nodiscard]] std::vector<uint32_t> selection() const {
    std::vector<uint32_t> out;
    uint32_t n = 0;
    if (!m_pt || !check(pt_get_selection(m_pt, nullptr, 0, &n))) return out;
    out.resize(n);
    if (n && !check(pt_get_selection(m_pt, out.data(), n, &n))) out.clear();
    return out;
  }
  // Transparent film (ptamd.h, an additive extension of ABI 5): a render started with enabled set keeps the foreground's premultiplied
  // radiance and its coverage beside the accumulator; `backdrop` chooses what presentRenderTarget / readbackRenderTarget of such a render
  // show behind it (PT_BACKDROP_SCENE: the accumulator as ever, _COLOR: backdrop_rgb, _TRANSPARENT: nothing, with a straight-alpha target).
  // Edited in place like bloomOptions(); `enabled` is read at startRender, the backdrop whenever a target is asked for.
  [[nodiscard]] constexpr pt_film_options& filmOptions() { return m_film; }
  void setFilmOptions(const pt_film_options& o) { m_film = o; }
  // The film, W*H*4 floats {premultiplied foreground rgb, coverage}; empty for a render started without it.  Blocks.
  [[nodiscard]] std::vector<float> readbackFilm() const {
    std::vector<float> out;
    if (!m_pt || !m_started) return out;
    out.resize((size_t)m_size.x * m_size.y * 4);
    if (!check(pt_read_film(m_pt, out.data()))) out.clear();
    return out;
  }
  // Ambient occlusion (ptamd.h, an additive extension of ABI 5): a render started with enabled set traces one cosine-weighted occlusion ray of
  // at most `distance` from every camera ray's first hit and keeps per pixel how many camera rays hit and how many of their AO rays were open.
  // Edited in place like filmOptions(); read at startRender.
  [[nodiscard]] constexpr pt_ao_options& ambientOcclusionOptions() { return m_ao; }
  void setAmbientOcclusionOptions(const pt_ao_options& o) { m_ao = o; }
  // open / hits per pixel, W*H floats (1 where no camera ray hit); empty for a render started without AO.  Blocks.
  [[nodiscard]] std::vector<float> readbackAmbientOcclusion() const {
    std::vector<float> out;
    if (!m_pt || !m_started) return out;
    out.resize((size_t)m_size.x * m_size.y);
    if (!check(pt_read_ao(m_pt, out.data()))) out.clear();
    return out;
  }
  // {hits, open} per pixel, W*H*2 words; empty for a render started without AO.  Blocks.
  [[nodiscard]] std::vector<uint32_t> readbackAmbientOcclusionCounts() const {
    std::vector<uint32_t> out;
    if (!m_pt || !m_started) return out;
    out.resize((size_t)m_size.x * m_size.y * 2);
    if (!check(pt_read_ao_counts(m_pt, out.data()))) out.clear();
    return out;
  }
  // The AO rays of one sample of every pixel, in pixel order: origins and directions (W*H*3 floats each) and the state per camera ray
  // (0 missed, 1 occluded, 2 open).  false, with the vectors empty, for a render started without AO.  Blocks.
  bool debugAmbientOcclusion(uint32_t sampleIdx, std::vector<float>& origins, std::vector<float>& directions, std::vector<uint32_t>& state) const {
    origins.clear(); directions.clear(); state.clear();
    if (!m_pt || !m_started) return false;
    const size_t n = (size_t)m_size.x * m_size.y;
    origins.resize(3 * n); directions.resize(3 * n); state.resize(n);
    if (check(pt_debug_ao(m_pt, sampleIdx, origins.data(), directions.data(), state.data()))) return true;
    origins.clear(); directions.clear(); state.clear();
    return false;
  }
  // Sun and sky (ptamd.h, an additive extension of ABI 5): the width x height lat-long RGBA32F image of a single-scattering atmosphere under
  // `o`, in the environment map's layout (hand it to the scene as its environment texture); empty on failure.  Needs no started render.  Blocks.
  [[nodiscard]] std::vector<float> generateSky(const pt_sky_options& o, uint32_t width, uint32_t height, pt_sky_stats* stats = nullptr) const {
    std::vector<float> out;
    if (!m_pt || width == 0 || height == 0 || (uint64_t)width * height > (1ull << 26)) return out;
    out.resize((size_t)width * height * 4);
    if (!check(pt_generate_sky(m_pt, &o, width, height, out.data(), stats))) out.clear();
    return out;
  }
  // Pass views (ptamd.h, an additive extension of ABI 5): `view` chooses what presentRenderTarget / readbackRenderTarget show: the beauty,
  // or the albedo, the normals, the depth, the film's alpha, the ID mattes, the sample counts or the noise estimate the render keeps.  A view
  // whose data the render does not keep silently shows the beauty.  Edited in place like bloomOptions(); read whenever a target is asked for.
  [[nodiscard]] constexpr pt_view_options& viewOptions() { return m_view; }
  // The view the target shows now and, under PT_VIEW_DEPTH, the range in use.  Blocks; draws nothing.  shown = PT_VIEW_BEAUTY on failure.
  [[nodiscard]] pt_view_stats viewStats() const {
    pt_view_stats s{};
    if (!m_pt || !m_started || !pushOptions()) return s;
    if (!check(pt_read_view_stats(m_pt, &s))) s = pt_view_stats{};
    return s;
  }
  void wait() const { if (m_pt && m_started) check(pt_wait(m_pt)); }
  [[nodiscard]] bool ok() const { return m_pt != nullptr && m_lastError.empty(); }
  [[nodiscard]] const std::string& lastError() const { return m_lastError; }
  [[nodiscard]] pt_renderer* handle() const { return m_pt; }

private:
  void create(const int* devices, uint32_t count, int first, const char* lutPath) noexcept {
    pt_tonemap_options defaults;
    pt_default_tonemap_options(&defaults);
    m_outputSpace = defaults.output_space;   // Display P3 (renderer_pt.hpp:182)
    pt_default_denoise_options(&m_denoise);
    pt_default_despeckle_options(&m_despeckle);
    pt_default_exposure_options(&m_autoExposure);
    pt_default_bloom_options(&m_bloom);
    pt_default_adaptive_options(&m_adaptive);
    pt_default_render_region(&m_region);
    pt_default_matte_options(&m_matte);
    pt_default_selection_options(&m_selection);
    pt_default_film_options(&m_film);
    pt_default_ao_options(&m_ao);
    pt_default_view_options(&m_view);
    pt_default_camera_projection(&m_projection);
    std::vector<int32_t> ord(devices, devices + count);
    pt_create_info ci{};
    ci.abi_version = PT_ABI_VERSION;
    ci.device_ordinal = first;
    ci.lut_path = lutPath;
    ci.device_ordinals = count ? ord.data() : nullptr;
    ci.device_count = count;
    if (!check(pt_create(&ci, &m_pt))) m_pt = nullptr;
  }
  bool check(int rc) const {
    if (rc == PT_OK) { m_lastError.clear(); return true; }
    m_lastError = pt_last_error();
    std::fprintf(stderr, "renderer_pt: %s\n", m_lastError.c_str());
    return false;
  }
  // the option structs are pushed when an image is asked for (the reference's passes read them when they are encoded)
  bool pushOptions() const {
    pt_post_options post;
    pt_tonemap_options tonemap;
    postprocess::flatten(m_exposure, m_chromaticAberration, m_contrastSaturation, m_toneCurve, m_vignette, &post);
    postprocess::flatten(m_tonemap, m_outputSpace, &tonemap);
    return check(pt_set_gmon_options(m_pt, &m_gmonOptions)) && check(pt_set_post_options(m_pt, &post)) && check(pt_set_tonemap_options(m_pt, &tonemap)) &&
           check(pt_set_denoise_options(m_pt, &m_denoise)) && check(pt_set_despeckle_options(m_pt, &m_despeckle)) &&
           check(pt_set_exposure_options(m_pt, &m_autoExposure)) && check(pt_set_bloom_options(m_pt, &m_bloom)) &&
           check(pt_set_selection_options(m_pt, &m_selection)) && check(pt_set_film_options(m_pt, &m_film)) &&
           check(pt_set_view_options(m_pt, &m_view));
  }

  pt_renderer* m_pt = nullptr;
  bool m_started = false;
  uint2 m_size{1, 1};
  uint32_t m_selectedPipeline = uint32_t(Integrators::MIS);  // renderer_pt.hpp:98
  uint32_t m_maxBounces = 50, m_firstSample = 0, m_samplesInFlight = 0, m_nonfinitePolicy = 0, m_accelStructure = PT_ACCEL_AUTO;
  uint32_t m_samplesPerRender = 1;
  postprocess::ExposureOptions m_exposure;                        // the passes' option structs (BasicPostProcessPass::m_options, postprocessing.hpp:304)
  postprocess::ChromaticAberrationOptions m_chromaticAberration;
  postprocess::ContrastSaturationOptions m_contrastSaturation;
  postprocess::ToneCurveOptions m_toneCurve;
  postprocess::VignetteOptions m_vignette;
  postprocess::TonemapOptions m_tonemap;
  pt_colorspace m_outputSpace{};
  pt_gmon_options m_gmonOptions{1.0f};
  pt_denoise_options m_denoise{};
  pt_despeckle_options m_despeckle{};
  pt_exposure_options m_autoExposure{};
  pt_bloom_options m_bloom{};
  pt_adaptive_options m_adaptive{};
  pt_render_region m_region{};
  pt_matte_options m_matte{};
  pt_selection_options m_selection{};
  pt_film_options m_film{};
  pt_ao_options m_ao{};
  pt_view_options m_view{};
  pt_camera_projection m_projection{};
  mutable void* m_presentStream = nullptr;
  mutable std::string m_lastError;
};

}  // namespace ptamd::renderer_pt

#endif
