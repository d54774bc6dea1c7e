/*
 * ptamd.h — C ABI of libptamd.so, the MI355X (gfx950) wavefront path tracer that sits behind the
 * `pt::renderer_pt::Renderer` operator surface of teofum/platinum.
 *
 * The reference has no FFI layer: `Renderer` (src/renderer_pt/renderer_pt.hpp:28-73) is a concrete C++ class
 * that the SDL2/ImGui frontend calls directly and that pulls the scene out of `Store&`.  This header is what a
 * binding for that class would bind: one entry point per public `Renderer` member, Metal handles replaced by
 * plain memory, the scene passed as a flat snapshot whose records keep the reference's exact byte layouts
 * (src/renderer_pt/pt_shader_defs.hpp, src/core/mesh.hpp) so the frontend's buffers can be handed over as-is.
 *
 * Plain C: pointers and sizes only, no C++/torch/HIP types in any signature.
 * Threading: one renderer = one caller thread (the reference is single-threaded, frontend.cpp:188-270).
 * Errors: every call returns PT_OK (0) or a negative pt_error; pt_last_error() returns the message of the last
 * failure on the calling thread (the reference prints to stderr and asserts: metal_utils.mm:172-214).
 * There is NO CPU fallback: pt_create fails with PT_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef PTAMD_H
#define PTAMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 5u /* 4: pt_get_runtime_info, PT_ERR_RUNTIME_CONFLICT, pt_stats::leaf_slots; 5: AOVs + denoiser (pt_create accepts 4 and 5), then tile-adaptive sampling as an additive extension */

/* ---------------------------------------------------------------------------------------------------------- */
/* Enums (same numeric values as the reference)                                                                 */

/* renderer_pt.hpp:21-26  enum Status */
enum { PT_STATUS_BLOCKED = 0, PT_STATUS_READY = 1, PT_STATUS_BUSY = 4, PT_STATUS_DONE = 8 };
/* renderer_pt.hpp:16-19  enum Integrators (kernel.metal:256 pathtracingKernel, :473 misKernel) */
enum { PT_INTEGRATOR_SIMPLE = 0, PT_INTEGRATOR_MIS = 1 };
/* pt_shader_defs.hpp:75-79  enum RendererFlags */
enum { PT_FLAG_NONE = 0, PT_FLAG_MULTISCATTER_GGX = 1 << 0, PT_FLAG_GMON = 1 << 1 };
/* A path whose radiance is NaN/inf (the reference's BSDF can produce one: e.g. a NaN pdf in the rough-glass eval,
 * about 1 path in 5e8 on C2) poisons its pixel's running mean for good in the reference (kernel.metal:672-684).
 * PROPAGATE keeps that behaviour (parity default); ZERO counts the sample as black and reports it in pt_stats. */
enum { PT_NONFINITE_PROPAGATE = 0, PT_NONFINITE_ZERO = 1 };
/* pt_shader_defs.hpp:85-90  MaterialGPU::MaterialFlags */
enum {
  PT_MATERIAL_THIN_DIELECTRIC = 1 << 0,
  PT_MATERIAL_USE_ALPHA = 1 << 1,
  PT_MATERIAL_EMISSIVE = 1 << 2,
  PT_MATERIAL_ANISOTROPIC = 1 << 3
};

typedef enum pt_error {
  PT_OK = 0,
  PT_ERR_INVALID_ARGUMENT = -1,
  PT_ERR_NO_DEVICE = -2,     /* no usable HIP device: the library never falls back to the CPU */
  PT_ERR_HIP = -3,           /* a HIP runtime call failed; message has file:line and hipGetErrorString */
  PT_ERR_OUT_OF_MEMORY = -4,
  PT_ERR_BAD_STATE = -5,     /* e.g. pt_render_step before pt_start_render */
  PT_ERR_UNSUPPORTED = -6,   /* a scene feature that is not implemented */
  PT_ERR_BAD_LUT = -7,
  PT_ERR_RUNTIME_CONFLICT = -8 /* more than one HIP runtime mapped into the process (pt_get_runtime_info says which) */
} pt_error;

/* ---------------------------------------------------------------------------------------------------------- */
/* Scene snapshot: what crosses the ABI instead of `Store&`.  Byte layouts are the reference's.                */

/* simd float3: 16-byte stride (renderer_pt.cpp:231, core/mesh.cpp:67-69) */
typedef struct pt_float3 { float x, y, z, _pad; } pt_float3;

/* core/mesh.hpp:17-21  VertexData, 48 B: normal @0, tangent(xyzw) @16, texCoords @32 */
typedef struct pt_vertex_data {
  pt_float3 normal;
  float tangent[4];
  float texCoords[2];
  float _pad[2];
} pt_vertex_data;

/* pt_shader_defs.hpp:84-103  MaterialGPU, 96 B */
typedef struct pt_material_gpu {
  float baseColor[4];          /* @0  */
  pt_float3 emission;          /* @16 */
  float emissionStrength;      /* @32 */
  float roughness;             /* @36 */
  float metallic;              /* @40 */
  float transmission;          /* @44 */
  float ior;                   /* @48 */
  float anisotropy;            /* @52 */
  float anisotropyRotation;    /* @56 */
  float clearcoat;             /* @60 */
  float clearcoatRoughness;    /* @64 */
  int32_t flags;               /* @68 */
  int32_t baseTextureId;       /* @72 */
  int32_t rmTextureId;         /* @76 */
  int32_t transmissionTextureId; /* @80 */
  int32_t clearcoatTextureId;  /* @84 */
  int32_t emissionTextureId;   /* @88 */
  int32_t normalTextureId;     /* @92 */
} pt_material_gpu;

/* One mesh = the four shared buffers of core/mesh.hpp:23-60.  `indices` doubles as PrimitiveData[]
 * (pt_shader_defs.hpp:48-50, renderer_pt.cpp:237-239). */
typedef struct pt_mesh {
  const pt_float3* positions;        /* vertex_count x 16 B */
  const pt_vertex_data* vertex_data; /* vertex_count x 48 B */
  const uint32_t* indices;           /* 3 * triangle_count */
  const uint32_t* material_slots;    /* triangle_count (core/mesh.hpp:32,55) */
  uint32_t vertex_count;
  uint32_t triangle_count;
} pt_mesh;

/* MTLAccelerationStructureInstanceDescriptor, 64 B packed (filled at renderer_pt.cpp:706-739):
 * 4 columns x packed float3 @0, options @48, mask @52, intersectionFunctionTableOffset @56,
 * accelerationStructureIndex (= mesh index) @60 */
typedef struct pt_instance {
  float transform[4][3];
  uint32_t options;
  uint32_t mask;
  uint32_t intersectionFunctionTableOffset;
  uint32_t accelerationStructureIndex;
} pt_instance;

/* InstanceResource (pt_shader_defs.hpp:126-128): the per-INSTANCE material array, indexed by the
 * triangle's material slot (renderer_pt.cpp:560-640 duplicates materials per instance). */
typedef struct pt_instance_materials {
  const pt_material_gpu* materials;
  uint32_t material_count;
  uint32_t _pad;
} pt_instance_materials;

/* Camera node: world matrix (scene.cpp:515-534, column-major float4x4) + core/camera.hpp:10-18.
 * The library derives CameraData exactly as Renderer::updateConstants (renderer_pt.cpp:965-1021). */
typedef struct pt_camera {
  float world[4][4];        /* columns */
  float sensor_size[2];     /* mm, default {36,24} */
  float focal_length;       /* mm */
  float aperture;           /* f-number, 0 = pinhole */
  uint32_t aperture_blades; /* sides of the aperture polygon (used when roundness < 1); fewer than 3 count as 3 */
  float roundness;
  float bokeh_power;        /* any float: the lens radius sqrt(u)^(2^bokeh_power) is 0 / 1 at the extremes, a NaN counts as 0 */
  float focus_distance;
} pt_camera;

/* core/colorspace.hpp:22-42: CIE xy chromaticities of the primaries and the white point */
typedef struct pt_colorspace { float r[2], g[2], b[2], w[2]; } pt_colorspace;

/* Scene textures. The reference uploads these pixel formats (loaders/texture.cpp:30-48) and samples
 * them with address::repeat + filter::linear (bsdf.metal:24, kernel.metal:167, intersections.metal:33). */
enum {
  PT_TEX_RGBA8_SRGB = 0, /* MTL::PixelFormatRGBA8Unorm_sRGB: base colour / emission (decoded to linear before filtering) */
  PT_TEX_RGBA8 = 1,      /* RGBA8Unorm: linear RGB (normal maps) */
  PT_TEX_RG8 = 2,        /* RG8Unorm: roughness, metallic */
  PT_TEX_R8 = 3,         /* R8Unorm: transmission / clearcoat */
  PT_TEX_RGBA32F = 4     /* RGBA32Float: HDR environment maps */
};
typedef struct pt_texture {
  const void* pixels;    /* row-major, top row first, tightly packed */
  uint32_t width, height;
  uint32_t format;       /* PT_TEX_* */
  uint32_t _pad;
} pt_texture;

/* core/environment.hpp:15-19 AliasEntry, 12 B */
typedef struct pt_alias_entry { float pdf, p; uint32_t aliasIdx; } pt_alias_entry;

typedef struct pt_scene_snapshot {
  const pt_mesh* meshes;
  uint32_t mesh_count;
  uint32_t instance_count;
  const pt_instance* instances;                    /* instance_count */
  const pt_instance_materials* instance_materials; /* instance_count */
  pt_camera camera;
  const pt_texture* textures;                      /* texture_count; MaterialGPU::*TextureId index this array */
  uint32_t texture_count;
  int32_t env_texture;                             /* Environment::textureId (scene envmap), -1 = none */
  const pt_alias_entry* env_alias;                 /* width*height entries, or NULL: built by the library exactly as
                                                      Environment::rebuildAliasTable (core/environment.cpp:5-91) */
} pt_scene_snapshot;

/* ---------------------------------------------------------------------------------------------------------- */
/* Derived device constants, exported for parity checks (pt_get_constants)                                     */

/* pt_shader_defs.hpp:52-61 CameraData, 80 B */
typedef struct pt_camera_data {
  pt_float3 position, topLeft, pixelDeltaU, pixelDeltaV;
  float apertureRadius;
  uint32_t apertureBlades;
  float apertureRoundness;
  float bokehPower;
} pt_camera_data;

/* pt_shader_defs.hpp:105-115 Constants, 176 B */
typedef struct pt_constants {
  uint32_t frameIdx, spp, gmonBuckets;
  uint32_t lightCount;
  uint32_t envLightCount;
  uint32_t lutSizeE, lutSizeEavg;
  int32_t flags;
  float totalLightPower;
  uint32_t _pad0;
  uint32_t size[2];
  pt_float3 idt[3];  /* float3x3 columns */
  pt_camera_data camera;
} pt_constants;

/* pt_shader_defs.hpp:63-68 AreaLight, 48 B (built by the library as renderer_pt.cpp:838-917) */
typedef struct pt_area_light {
  uint32_t instanceIdx;
  uint32_t indices[3];
  float area, power, cumulativePower;
  float _pad;
  pt_float3 emission;
} pt_area_light;

/* ---------------------------------------------------------------------------------------------------------- */
/* Renderer                                                                                                      */

typedef struct pt_renderer pt_renderer;

/* Renderer::Renderer(device, queue, store) (renderer_pt.hpp:28-32, renderer_pt.cpp:18-60): builds the
 * pipelines and loads the 8 GGX energy LUTs (renderer_pt.cpp:385-446). */
typedef struct pt_create_info {
  uint32_t abi_version;   /* PT_ABI_VERSION */
  int32_t device_ordinal; /* HIP device; the reference takes the MTL::Device of the window */
  const void* lut_blob;   /* the LUT blob (tools/make_lut_blob.py) in host memory, or NULL ... */
  uint64_t lut_blob_size;
  const char* lut_path;   /* ... to read it from this file (NULL: $PTAMD_LUT_PATH) */
  /* NEW (ABI 3): a DEVICE GROUP.  device_count >= 2 devices share every render: the samples [first_sample, first_sample + spp)
   * are dealt to them in contiguous ranges (whole GMoN buckets with PT_FLAG_GMON), each device renders its range on its own
   * host thread and stream, and the running means are merged when the image is asked for (pt_wait / pt_read_*): ONE RCCL
   * all-reduce of the float accumulator over xGMI (bucket means gathered to the first device and resolved there with GMoN).
   * The merged image lives on device_ordinals[0] (in external_accumulator when given).  A device may be listed more than
   * once (logical shards on one GPU).  device_count == 0: the single device `device_ordinal`. */
  const int32_t* device_ordinals;
  uint32_t device_count;
} pt_create_info;

int pt_create(const pt_create_info* info, pt_renderer** out);
/* Which GPU runtime objects this process holds and which of them serves this library.  No counterpart in the reference (Metal is a
 * system framework); needed here because PyTorch's ROCm wheel bundles private copies of libamdhip64 / libhsa-runtime64 / librccl
 * that can end up mapped BESIDE the system's, and then only the runtime that initialises first sees the GPU.
 * pt_create returns PT_ERR_RUNTIME_CONFLICT when hip_runtimes_mapped exceeds 1 (a second libhsa-runtime64 under one HIP runtime is what
 * rocprofv3's tool library maps: reported, not refused).  Touches no GPU. */
typedef struct pt_runtime_info {
  char hip_runtime_path[512]; /* the libamdhip64 this library's hip* calls resolve to */
  char hsa_runtime_path[512]; /* the (first) libhsa-runtime64 mapped */
  char rccl_path[512];        /* the librccl bound by a device group / pt_rccl_probe; "" until one of them has loaded it */
  uint32_t hip_runtimes_mapped, hsa_runtimes_mapped, rccl_mapped; /* distinct shared objects of each kind in the process */
  int32_t hip_runtime_version; /* hipRuntimeGetVersion of the serving runtime, 0 if the call failed */
  char all_mapped[2048];      /* every matching object, " + " separated: hip | hsa | rccl */
} pt_runtime_info;
int pt_get_runtime_info(pt_runtime_info* out);
/* How a device group deals the samples [0, spp) of a render to its `members` (pure host arithmetic, exported for tests):
 * contiguous ranges, equal up to one sample; with PT_FLAG_GMON whole buckets per member (bucket b = samples
 * [b * ceil(spp / buckets), ...), renderer_pt.cpp:124-126), bucket0/bucket1 = each member's bucket range (may be NULL). */
int pt_group_partition(uint32_t spp, uint32_t members, int32_t flags, uint32_t gmon_buckets, uint64_t* first, uint64_t* count,
                       uint32_t* bucket0, uint32_t* bucket1);
/* Loads librccl.so the way a device group over >= 2 distinct GPUs does (dlopen) and binds the entry points the merge uses
 * (ncclCommInitAll, ncclCommDestroy, ncclAllReduce, ncclGroupStart, ncclGroupEnd, ncclGetErrorString).  No GPU is touched:
 * a build-box check that the multi-GPU path can find its collective library.  PT_OK or PT_ERR_UNSUPPORTED (pt_last_error). */
int pt_rccl_probe(void);
/* The same on a GPU, one step further: a communicator of ONE rank on `device_ordinal`, the merge's grouped in-place
 * ncclAllReduce(sum, float32) on a known pattern, result checked, communicator destroyed — every RCCL call the distinct-device merge
 * makes, with its argument types and stream ordering, as far as a one-GPU box can run them. */
int pt_rccl_selftest(int32_t device_ordinal);
/* Renderer::~Renderer (renderer_pt.hpp:34) */
void pt_destroy(pt_renderer* r);

/* Parameters of Renderer::startRender(camera, size, spp, gmonBuckets, workingSpace, flags)
 * (renderer_pt.hpp:38-45) + selectKernel (:47-53) + what the reference fixes at compile time or lacks. */
typedef struct pt_render_params {
  uint32_t width, height;      /* viewport size */
  uint32_t spp;                /* samples this renderer accumulates (m_accumulationFrames) */
  uint32_t gmon_buckets;       /* used only with PT_FLAG_GMON (1..32, gmon.metal:12); constants.gmonBuckets is 1 otherwise */
  int32_t flags;               /* PT_FLAG_* */
  uint32_t integrator;         /* PT_INTEGRATOR_* (default MIS, renderer_pt.hpp:98) */
  pt_colorspace working_space; /* default BT2020 (pt_viewport.hpp:95) */
  uint32_t max_bounces;        /* NEW: kernel.metal:5 hard-codes 50; 1..50 */
  uint32_t first_sample;       /* NEW: frameIdx of this renderer's first sample (multi-GPU shards) */
  uint32_t samples_in_flight;  /* NEW: samples traced concurrently per batch; 0 = auto */
  uint32_t nonfinite_policy;   /* NEW: PT_NONFINITE_*: what a NaN/inf sample does to the running mean */
  void* external_accumulator;  /* optional DEVICE pointer to W*H float4; NULL = library-owned */
  void* stream;                /* optional hipStream_t to enqueue on; NULL = library-owned stream */
  uint32_t accel_structure;    /* NEW (ABI 3): PT_ACCEL_*.  The reference always builds BLAS per mesh + TLAS over instances
                                  (renderer_pt.cpp:653-749); closest hits are identical whichever structure is walked */
  uint32_t _reserved;
} pt_render_params;
/* PT_ACCEL_AUTO: one BVH over the flattened world-space triangles (fastest: C3 7.4 vs 4.2 Grays/s) unless that would not fit
 * beside the path queues; PT_ACCEL_TWO_LEVEL: TLAS over instances + one object-space BLAS per mesh (C3: 65 KB instead of 82 MB
 * of nodes, staged in LDS by the trace kernels); needs invertible instance transforms, else one BVH is built. */
enum { PT_ACCEL_AUTO = 0, PT_ACCEL_ONE_BVH = 1, PT_ACCEL_TWO_LEVEL = 2 };

/* How pt_start_render sizes the wavefront queues for an image (pure host arithmetic, exported for tests): the samples traced
 * concurrently per batch after every index-width limit has been applied (an explicit samples_in_flight is HALVED until the
 * 16-bit segment slots, the 32-bit queue indices and the chunk tables can address the batch; the image does not change),
 * and the segment geometry.  free_hbm_bytes only matters for samples_in_flight = 0 (auto); tiles_per_seg_override /
 * seg_bands are the $PTAMD_TILES_PER_SEG / $PTAMD_SEG_BANDS tuning knobs (0 / 4 by default). */
typedef struct pt_queue_plan {
  uint32_t samples_in_flight;  /* what a batch will carry */
  uint32_t tiles_per_seg;      /* 8x8 pixel tiles per queue segment */
  uint32_t nseg;               /* segments (<= 32768) */
  uint32_t seg_cap;            /* path slots per segment = tiles_per_seg * samples_in_flight * 64 (<= 65536) */
  uint64_t capacity;           /* path slots per queue array */
  uint64_t lbuf_entries;       /* entries of the per-sample radiance buffer */
} pt_queue_plan;
int pt_plan_queues(uint32_t width, uint32_t height, uint32_t spp, uint32_t samples_in_flight, uint64_t free_hbm_bytes,
                   uint32_t tiles_per_seg_override, uint32_t seg_bands, pt_queue_plan* out);

/* Renderer::startRender + the rebuild* half of the first Renderer::render() (renderer_pt.cpp:72-111,
 * 199-217): copies the snapshot to HBM, builds light table, constants and the LBVH.  The caller owns the
 * snapshot memory only until this returns. Resets progress to 0. */
int pt_start_render(pt_renderer* r, const pt_scene_snapshot* scene, const pt_render_params* params);

/* Renderer::render() steady state (renderer_pt.cpp:113-197): accept up to `max_spp_this_call` further samples (the reference
 * encodes exactly 1) and return without waiting. 0 = all remaining samples.  Progress counts accepted samples, as the reference's
 * m_accumulatedFrames counts encoded ones.  Calls that arrive while the GPU is still executing the previous batch are merged into
 * one batch of up to samples_in_flight samples (a one-sample batch cannot fill the chip); pt_wait, the pt_read_* / present entry
 * points and the call that accepts the render's last sample enqueue whatever is pending.  The image is the same either way. */
int pt_render_step(pt_renderer* r, uint32_t max_spp_this_call);
/* Block until everything enqueued so far has completed (the reference only blocks in readback). */
int pt_wait(pt_renderer* r);

/* Renderer::status() (renderer_pt.cpp:1023-1031), renderProgress() (:1033-1035), renderTime() (:1037) */
int pt_status(const pt_renderer* r);
int pt_progress(const pt_renderer* r, uint64_t* accumulated, uint64_t* total);
uint64_t pt_render_time_ms(const pt_renderer* r);

/* Renderer::gmonOptions() (renderer_pt.hpp:71; pt_shader_defs.hpp:164-166 GmonOptions). With PT_FLAG_GMON the samples
 * are accumulated into `gmon_buckets` bucket images (bucket = sample / ceil(spp / buckets), renderer_pt.cpp:124-139)
 * and the accumulator holds their Gini-weighted median-of-means (shaders/gmon.metal), recomputed after every batch. */
typedef struct pt_gmon_options { float cap; } pt_gmon_options; /* default 1.0; 0 <= cap <= 1, else PT_ERR_INVALID_ARGUMENT */
int pt_set_gmon_options(pt_renderer* r, const pt_gmon_options* options);
/* One bucket image (W*H*4 floats), for parity checks. */
int pt_read_gmon_bucket(pt_renderer* r, uint32_t bucket, float* rgba_out);

/* ---- post-process chain + tonemap -> RGBA8 ---------------------------------------------------------
 * Renderer::postProcessOptions() / tonemapOptions() / outputColorspace() (renderer_pt.hpp:65-73) edit option structs the
 * UI writes every frame (core/postprocessing.hpp:168-218); pass order exposure, chromaticAberration, contrastSaturation,
 * toneCurve, vignette, tonemap (renderer_pt.cpp:343-353).  Field names follow the reference's structs. */
typedef struct pt_post_options {
  float exposure;                                          /* ExposureOptions */
  float ca_amount, ca_green_shift;                         /* ChromaticAberrationOptions (0, 70) */
  float contrast, saturation;                              /* ContrastSaturationOptions */
  float blacks, shadows, highlights, whites;               /* ToneCurveOptions */
  float vig_amount, vig_midpoint, vig_feather, vig_power, vig_roundness; /* VignetteOptions (0, 0, 50, 20, 100) */
} pt_post_options;

enum { PT_TONEMAP_NONE = 0, PT_TONEMAP_AGX = 1, PT_TONEMAP_KHRONOS_PBR = 2, PT_TONEMAP_FLIM = 3 }; /* postprocess::Tonemapper */

typedef struct pt_tonemap_options {
  uint32_t tonemapper;                                     /* default AgX (postprocessing.hpp:219) */
  float agx_offset[3], agx_slope[3], agx_power[3], agx_saturation;      /* agx::Look (looks::none) */
  float khr_compression_start, khr_desaturation;           /* khronos_pbr::Options (0.8, 0.15) */
  float flim_pre_exposure, flim_pre_formation_filter[3], flim_pre_formation_filter_strength; /* flim::Options */
  float flim_extended_gamut_scale[3], flim_extended_gamut_rotation[3], flim_extended_gamut_mul[3];
  float flim_sigmoid_log2_min, flim_sigmoid_log2_max, flim_sigmoid_toe[2], flim_sigmoid_shoulder[2];
  float flim_negative_exposure, flim_negative_density, flim_print_backlight[3], flim_print_exposure, flim_print_density;
  float flim_black_point;
  uint32_t flim_auto_black_point;
  float flim_post_formation_filter[3], flim_post_formation_filter_strength, flim_midtone_saturation;
  float shadow_color[3], midtone_color[3], highlight_color[3];          /* LiftGammaGain (0.5 each) */
  float shadow_offset, midtone_offset, highlight_offset;
  pt_colorspace output_space;                              /* outputColorspace(), default Display P3 (renderer_pt.hpp:182) */
} pt_tonemap_options;

/* Fill with the reference's defaults (postprocessing.hpp:168-226, flim::presets::flim). */
void pt_default_post_options(pt_post_options* o);
void pt_default_tonemap_options(pt_tonemap_options* o);
int pt_set_post_options(pt_renderer* r, const pt_post_options* o);
int pt_set_tonemap_options(pt_renderer* r, const pt_tonemap_options* o);
/* readbackRenderTarget() (renderer_pt.hpp:57, renderer_pt.cpp:1039-1059): the post-processed, tonemapped RGBA8 image
 * (W*H*4 bytes, row-major, top-left origin). Blocks. */
int pt_read_render_target(pt_renderer* r, uint8_t* rgba8_out);
/* presentRenderTarget() (renderer_pt.hpp:55, used by pt_viewport.cpp:711 to blit): post-processes the current accumulator into
 * the library's RGBA8 render target ON THE DEVICE and returns its device address (W*H*4 bytes, valid until the next
 * pt_start_render / pt_destroy) without a host copy.  The work is enqueued on the renderer's stream; *stream_out (may be NULL)
 * receives that hipStream_t so the caller can order its blit after it.  A device group presents on device_ordinals[0]. */
int pt_present_render_target(pt_renderer* r, void** device_rgba8_out, void** stream_out);

/* The float accumulator: W*H RGBA32F, row-major, top-left origin, running mean, alpha 1
 * (renderer_pt.cpp:812-821, kernel.metal:672-684).  Blocks like readbackRenderTarget (:1039-1059). */
int pt_read_accumulator(pt_renderer* r, float* rgba_out);
/* Device address of the accumulator (for an RCCL reduce by the caller); NULL before pt_start_render. */
void* pt_accumulator_device_ptr(pt_renderer* r);


/* ---- first-hit AOVs and the denoiser (NEW, ABI 5; no reference counterpart) -----------------------------------------------
 * A render started while `enabled` is set keeps three W*H RGBA32F images beside the accumulator, running means over its samples
 * folded per pixel in sample order like the accumulator (the same bits however the samples are batched):
 *   PT_AOV_ALBEDO   rgb: linear base colour at the camera ray's first hit (base texture included); a miss contributes (1,1,1).  a: 1
 *   PT_AOV_NORMAL   rgb: world-space shading normal at the first hit (normal map included); a miss contributes 0.  a: hit fraction h
 *   PT_AOV_MOMENTS  r: first-hit distance (a miss contributes 0; mean depth = r / h); g, b: means of lum(L) and lum(L)^2 of the
 *                   sample radiance after the non-finite policy, lum = (0.2126, 0.7152, 0.0722).  a: 0
 * The accumulator and every other result are the same bits with AOVs on or off.  AOVs cost 32 bytes per path slot: with
 * samples_in_flight = 0 the renderer counts them when it sizes its batches (pt_plan_queues describes AOV-off renders).
 * The denoiser is an edge-avoiding a-trous filter (SVGF's spatial filter: Dammertz et al. 2010, Schied et al. 2017, no temporal
 * part) guided by the AOVs, run on demand over the current image (DESIGN.md section 3 states its arithmetic).
 * A device group (device_count >= 2) refuses enabled = 1 with PT_ERR_UNSUPPORTED: merging the AOVs would take one more all-reduce. */
typedef struct pt_denoise_options {
  uint32_t enabled;          /* accumulate AOVs for renders started from now on (read at pt_start_render) */
  uint32_t iterations;       /* 0..8, default 5; 0 = demodulate + remodulate only (the accumulator itself) */
  float sigma_luminance, sigma_normal, sigma_depth;   /* 4, 128, 1: finite and > 0; a sigma_normal above 2^24 counts as 2^24 */
  uint32_t apply_to_target;  /* pt_read_render_target / pt_present_render_target post-process the denoised image (of a render
                                started with AOVs; a render without them shows its accumulator as before) */
} pt_denoise_options;
enum { PT_AOV_ALBEDO = 0, PT_AOV_NORMAL = 1, PT_AOV_MOMENTS = 2 };
void pt_default_denoise_options(pt_denoise_options* o);
/* The filter fields take effect at the next read or present, `enabled` at the next pt_start_render. */
int pt_set_denoise_options(pt_renderer* r, const pt_denoise_options* o);
/* One AOV image (W*H*4 floats).  Blocks like pt_read_accumulator.  PT_ERR_BAD_STATE for a render started without AOVs. */
int pt_read_aov(pt_renderer* r, uint32_t aov, float* rgba_out);
/* The denoised image (W*H*4 floats, alpha 1).  Blocks.  PT_ERR_BAD_STATE for a render started without AOVs. */
int pt_read_denoised(pt_renderer* r, float* rgba_out);

/* ---- firefly clamp ahead of the denoiser (NEW, an additive extension of ABI 5: new entry points and one new struct, no existing struct changed) ----
 * At 1-4 spp a single sample 10-1000x brighter than its neighbours passes the luminance edge-stop of its own pixel and is smeared over the
 * filter's footprint.  With `enabled` set the denoiser clamps such pixels between its prep and its first a-trous step: a valid pixel whose
 * demodulated luminance L exceeds lim = threshold * M, M the largest luminance among its up to 8 neighbours in the 3x3 window (valid, of its
 * own class geometry / background, inside the image or the render region), becomes I * (lim / L); its variance is kept.  A pixel with no such
 * neighbour is left alone.  The clamp needs iterations >= 1: iterations = 0 returns the accumulator either way.
 * The options take effect at the next pt_read_denoised, or read / present with apply_to_target; no restart is needed.  enabled = 0 gives
 * the bits of a library without the clamp.  A device group refuses enabled = 1 with PT_ERR_UNSUPPORTED, like the denoiser. */
typedef struct pt_despeckle_options {
  uint32_t enabled;   /* default 0 */
  float threshold;    /* finite and >= 1; default 2 */
} pt_despeckle_options;
void pt_default_despeckle_options(pt_despeckle_options* o);
/* PT_ERR_INVALID_ARGUMENT for a threshold that is not finite or < 1 (checked before the renderer) */
int pt_set_despeckle_options(pt_renderer* r, const pt_despeckle_options* o);

/* ---- auto exposure: a luminance-histogram meter ahead of the post-process (NEW, an additive extension of ABI 5: new entry points and two
 * new structs, no existing struct changed) ----
 * With `enabled` set, pt_read_render_target / pt_present_render_target meter the image the post-process is about to read (the accumulator;
 * the denoised image with apply_to_target; a device group's merged image) over the render's rectangle (the frame, or the render region),
 * scale its rgb by `gain` into a scratch image and post-process that: target = post-process(image * gain).  pt_post_options.exposure acts on
 * top as compensation.  Everything is enqueued on the renderer's stream; there is no host round trip.
 * Per pixel Y = (0.2126 r + 0.7152 g) + 0.0722 b (alpha ignored) is counted, in this order, as `nonfinite` (NaN, +-inf), `below` (Y < 2^-16:
 * 0, negatives, denormals), `above` (Y >= 2^16), or in bin (bits(Y) >> 20) - 888: 8 bins per octave over [2^-16, 2^16).  Only binned pixels
 * are metered.  With n their number, lo = (uint64)(n * low_fraction), hi = min(n, (uint64)(n * high_fraction)) in double (lo = 0, hi = n
 * when hi <= lo), the pixels of ascending rank [lo, hi) are kept: K = hi - lo of them, S = sum over them of (2 * bin + 1).  Then
 *   mean_log2 = (float)((double)S / (double)(16 K)) - 16     target_ev = min(max(target_log2 - mean_log2, min_ev), max_ev)
 *   ev = previous ev + (1 - smoothing) * (target_ev - previous ev), or target_ev when there is no previous one     gain = 2^ev
 * and mean_log2 = target_ev = 0 when n = 0.  The previous ev is kept on the device; pt_start_render keeps it, so the
 * exposure eases across camera restarts.  enabled = 0 allocates and launches nothing and gives the bits of a library without the meter.
 * pt_read_accumulator, pt_read_denoised and the AOVs are never scaled. */
typedef struct pt_exposure_options {
  uint32_t enabled;        /* default 0; read at every pt_read_render_target / pt_present_render_target, no restart */
  float target_log2;       /* log2 luminance the metered mean is brought to; default -2.4739313f (log2 0.18); finite, |x| <= 32 */
  float low_fraction;      /* default 0.10 */
  float high_fraction;     /* default 0.95; 0 <= low < high <= 1 */
  float min_ev, max_ev;    /* defaults -16, 16; finite, -32 <= min_ev <= max_ev <= 32 (gain stays finite and non-zero) */
  float smoothing;         /* default 0; 0 <= s < 1: weight of the previously applied ev */
} pt_exposure_options;
void pt_default_exposure_options(pt_exposure_options* o);
/* PT_ERR_INVALID_ARGUMENT for options outside the ranges above (checked before the renderer) */
int pt_set_exposure_options(pt_renderer* r, const pt_exposure_options* o);
/* Forgets the previous ev: the next metered target starts from its own target_ev. */
int pt_reset_exposure(pt_renderer* r);

typedef struct pt_exposure_meter {
  uint32_t bins[256];
  uint32_t below, above, nonfinite, metered;   /* metered = sum of bins */
  uint32_t kept;  uint32_t _pad;  uint64_t weighted;   /* K and S */
  float mean_log2, target_ev, ev, gain;
} pt_exposure_meter;
/* Meters the image a target read would show now.  Blocks.  Works with enabled = 0 (a UI histogram).  Does NOT advance the smoothing
 * state: ev is what a target read made at this moment would apply.  PT_ERR_BAD_STATE before pt_start_render. */
int pt_read_exposure_meter(pt_renderer* r, pt_exposure_meter* out);
/* Parity surface: upload a host W*H RGBA32F image, run the same three kernels over `rect` ({x0, y0, x1, y1}, or NULL for the whole image)
 * with `options` and no smoothing state, and return the record and (scaled_out may be NULL) the scaled image.  Needs only pt_create. */
int pt_debug_exposure(pt_renderer* r, const float* rgba, uint32_t width, uint32_t height, const uint32_t* rect,
                      const pt_exposure_options* options, pt_exposure_meter* out, float* scaled_out);

/* ---- bloom: an energy-conserving glare pyramid ahead of the post-process (NEW, an additive extension of ABI 5: new entry points and two
 * new structs, no existing struct changed) ----
 * With `enabled` set, pt_read_render_target / pt_present_render_target scatter a fraction `intensity` of the light above `threshold` with a
 * wide point-spread function and leave the rest in place:  out = in - intensity * bright(in) + intensity * (PSF * bright(in)).  It runs over
 * the full frame on the renderer's stream, after the denoised-image selection and after auto exposure (so `threshold` is in the units of
 * the auto-exposed image) and ahead of the post-process (pt_post_options.exposure acts after it).  fp32, no contraction, every sum in the
 * order written here.
 * Plan: level 0 is the frame; level l+1 is ((w_l + 1) / 2) x ((h_l + 1) / 2); L = min(levels, halvings until a level is 1 x 1).  A 1 x 1
 * frame has L = 0 and keeps its bits.  The pyramid holds levels 1..L back to back, 16 bytes per texel.
 * Bright pass b of a pixel rgb (alpha ignored): Y = (0.2126 r + 0.7152 g) + 0.0722 b.  b = 0 when !(|Y| <= 3e38), a channel is not finite
 * or Y <= 0; otherwise s = min(max((Y - threshold) + knee, 0), 2 knee), soft = (s s) / (4 knee + 1e-6), w = max(soft, Y - threshold) / Y,
 * b.c = min(max(rgb.c, 0) w, 2^64).  A NaN or infinite pixel scatters nothing.
 * Down: D_0 = b; D_{l+1}(x, y) = sum over j = 0..3, then i = 0..3, from 0, of (k[j] k[i]) D_l(clamp(2x - 1 + i), clamp(2y - 1 + j)),
 * k = (1, 3, 3, 1) / 8.
 * Up: up(C)(x, y) with cx = x >> 1 takes (cx - 1, 1/4), (cx, 3/4) for even x and (cx, 3/4), (cx + 1, 1/4) for odd x, the same in y, indices
 * clamped to the coarse level, summed as ((ya,xa) + (ya,xb)) + (yb,xa)) + (yb,xb) with weights wy wx.
 * Combine: U_L = D_L; U_l = D_l + scatter * up(U_{l+1}) for l = L-1..1; norm = sum over k < L of scatter^k (fp32, running sum += running
 * power from k = 0); B = up(U_1) / norm; out.c = in.c + intensity * (B.c - b.c); a channel that is not finite and alpha keep their bits.
 * enabled = 0 allocates and launches nothing and gives the bits of a library without bloom.  pt_read_accumulator, pt_read_denoised, the
 * AOVs and pt_read_exposure_meter never see it.  With a render region the zeros outside it receive scattered light; their alpha stays 0. */
#define PT_BLOOM_MAX_LEVELS 12u
typedef struct pt_bloom_options {
  uint32_t enabled;     /* default 0; read at every pt_read_render_target / pt_present_render_target, no restart */
  float intensity;      /* default 0.05; the scattered fraction, in [0, 1] */
  float threshold;      /* default 0; luminance above which light scatters; finite, >= 0 */
  float knee;           /* default 0; half-width of the soft transition around the threshold; finite, >= 0 */
  float scatter;        /* default 1; weight of each coarser octave relative to the one below it, in (0, 1] */
  uint32_t levels;      /* default 6; 1..PT_BLOOM_MAX_LEVELS */
} pt_bloom_options;
void pt_default_bloom_options(pt_bloom_options* o);
/* PT_ERR_INVALID_ARGUMENT for options outside the ranges above (checked before the renderer) */
int pt_set_bloom_options(pt_renderer* r, const pt_bloom_options* o);

typedef struct pt_bloom_plan {
  uint32_t levels;         /* L */
  uint32_t total_texels;   /* texels of the levels 1..L */
  uint32_t width[PT_BLOOM_MAX_LEVELS + 1], height[PT_BLOOM_MAX_LEVELS + 1];   /* [0] is the frame; entries past L are 0 */
  uint32_t offset[PT_BLOOM_MAX_LEVELS + 1];                                    /* first texel of level l in the pyramid; [0] is 0 */
} pt_bloom_plan;
/* Pure host arithmetic (exported for tests, like pt_plan_queues).  PT_ERR_INVALID_ARGUMENT for an image outside 1..2^28 pixels or levels
 * outside 1..PT_BLOOM_MAX_LEVELS. */
int pt_plan_bloom(uint32_t width, uint32_t height, uint32_t levels, pt_bloom_plan* out);
/* Parity surface: upload a host W*H RGBA32F image, run the same launches with `options` (whatever `enabled` says) and return the bloomed
 * image and (pyramid_out may be NULL) U_1..U_L as pt_plan_bloom lays them out, total_texels x 4 floats (.w is 0).  Needs only pt_create.
 * The image must hold 1..2^28 pixels. */
int pt_debug_bloom(pt_renderer* r, const float* rgba, uint32_t width, uint32_t height, const pt_bloom_options* options, float* out,
                   float* pyramid_out);

/* ---- sun and sky: a single-scattering atmosphere as environment map (NEW, an additive extension of ABI 5: two entry points and two
 * structs) ----
 * pt_generate_sky fills a width x height lat-long RGBA32F image in the environment map's own layout (texel (x, y) looks along
 * uvToRayDir((x + 1/2) / w, (y + 1/2) / h), the direction whose miss lookup lands on its centre); the caller hands it to the renderer as
 * the snapshot's env_texture like any other RGBA32F environment.  One kernel launch on the renderer's stream, one lane per texel; the
 * model, its constants and the order of every sum are DESIGN.md section 3m.  Lengths in km; the three channels are the render's
 * working-space rgb as given.  The sun stands at s = (-cos a cos e, sin e, -sin a cos e): column a / 2pi * w, row (pi/2 - e) / pi * h.
 * The disc has the radius alpha_eff = max(sun_angular_radius, pi / height) and is drawn by 4 x 4 coverage per texel, its radiance
 * sun_intensity * T / Omega_d with Omega_d the DISCRETE solid angle of the covered texels: the disc's irradiance is sun_intensity times
 * the coverage-weighted mean transmittance at every map size.  Every output is finite and >= 0, alpha is 1.
 * Needs only pt_create.  PT_ERR_INVALID_ARGUMENT, before the renderer is looked at: options outside the ranges below, a NaN anywhere, an
 * image outside 1..2^26 texels, a null options or rgba_out; then a null renderer. */
typedef struct pt_sky_options {
  float sun_elevation, sun_azimuth;   /* radians; elevation in [-pi/2, pi/2], azimuth any finite value (reduced modulo 2 pi in double) */
  float sun_angular_radius;           /* default 0.004712 (0.27 deg); in (0, 0.2] */
  float sun_intensity;                /* irradiance of the sun above the atmosphere, per channel; default 1; finite, >= 0 */
  uint32_t sun_disc;                  /* default 1: draw the disc; 0: sky and ground only */
  float altitude_km;                  /* default 0.001; in [0.001, 60] */
  float air_density, dust_density, ozone_density;   /* defaults 1; in [0, 10] */
  float ground_albedo;                /* default 0.3; in [0, 1] */
} pt_sky_options;
typedef struct pt_sky_stats {
  float sun_direction[3]; float sun_radius_used;   /* s; alpha_eff */
  double sun_solid_angle;                          /* Omega_d */
  uint32_t sun_texels; float kernel_ms;            /* texels with coverage > 0; the kernel's time by events */
} pt_sky_stats;
void pt_default_sky_options(pt_sky_options* o);   /* elevation 0.5, azimuth 0, the defaults above */
int pt_generate_sky(pt_renderer* r, const pt_sky_options* options, uint32_t width, uint32_t height, float* rgba_out,
                    pt_sky_stats* stats_out /* may be NULL */);

/* ---- math probe (NEW, an additive extension of ABI 5: one entry point and one enum) ----
 * Parity surface: the deterministic fp32 math, the sample warps and the Halton sequence of the kernels, evaluated on the device on their own.
 * One elementwise launch on the renderer's stream computes function `fn` on n elements: a[i] (and b[i] for a function of two arguments) in,
 * out0[i] (and out1[i] for a function of two results) out, upload and read-back inside the call.  Every array holds n 4-byte elements, float
 * unless stated.  Needs only pt_create.
 *   PT_MATH_SINCOS          sincos(a): out0 = sin, out1 = cos          PT_MATH_COS    cos(a)
 *   PT_MATH_ATAN2           atan2(y = a, x = b)                         PT_MATH_ACOS   acos(a)
 *   PT_MATH_LOG2 / EXP2     log2(a), exp2(a)                            PT_MATH_POWR   powr(x = a, y = b)
 *   PT_MATH_PP_LOG2 / PP_EXP2 / PP_EXP2S / PP_POWR, PT_MATH_DN_EXP2 / DN_POWR: the range-guarded forms of the post-process and the denoiser
 *   PT_MATH_SAMPLE_DISK, PT_MATH_SAMPLE_TRI_UNIFORM: u = (a, b) -> (out0, out1)
 *   PT_MATH_SAMPLE_COSINE_HEMISPHERE: u = (a, b) -> x = out0[i], y = out1[i], z = out1[n + i]: out1 holds 2n floats for this function alone
 *   PT_MATH_HALTON          halton(index = a, dimension = b), both uint32, b < 620, from the renderer's own table
 *   PT_MATH_HALTON_OFFSET   the sample-stream offset of pixel (x = a & 0xffff, y = a >> 16) and sample b (a, b, out0: uint32)
 *   PT_MATH_BOKEH_POWR      the thin-lens radius: lens sample u = a, bokehPower = b -> sqrt(u)^(2^b), defined for every float b
 * The unguarded functions are evaluated as they stand: outside their domains the result is unspecified.
 * PT_ERR_INVALID_ARGUMENT, before the renderer is looked at: fn >= PT_MATH_COUNT, n = 0 or n > 2^24, a null a or out0, a null b / out1 for a
 * function that reads / writes it; then a null renderer. */
enum {
  PT_MATH_SINCOS = 0, PT_MATH_COS = 1, PT_MATH_ATAN2 = 2, PT_MATH_ACOS = 3, PT_MATH_LOG2 = 4, PT_MATH_EXP2 = 5, PT_MATH_POWR = 6,
  PT_MATH_PP_LOG2 = 7, PT_MATH_PP_EXP2 = 8, PT_MATH_PP_EXP2S = 9, PT_MATH_PP_POWR = 10, PT_MATH_DN_EXP2 = 11, PT_MATH_DN_POWR = 12,
  PT_MATH_SAMPLE_DISK = 13, PT_MATH_SAMPLE_COSINE_HEMISPHERE = 14, PT_MATH_SAMPLE_TRI_UNIFORM = 15,
  PT_MATH_HALTON = 16, PT_MATH_HALTON_OFFSET = 17, PT_MATH_BOKEH_POWR = 18, PT_MATH_COUNT = 19
};
int pt_debug_math(pt_renderer* r, uint32_t fn, uint32_t n, const void* a, const void* b, void* out0, void* out1);

/* ---- light probe (NEW, an additive extension of ABI 5: one entry point, one struct and two enums) ----
 * Parity surface: the light-sampling part of the shading stage, evaluated on the device on its own against the scene of the STARTED render
 * (its light records, cumulative table, environment texture and alias table).  One elementwise launch on the renderer's stream; upload and
 * read-back inside the call; the render's state is left alone.  `in` holds n records of 4-byte words, `out` receives n records:
 *   PT_LIGHT_SAMPLE    in:  8 floats  hit position x y z, the three NEE draws rl.x rl.y rz, 2 unused
 *                      out: 12 words  lit (uint32), Li r g b, lwi x y z, lpdf, pLight, dist, dim (uint32), 0
 *                      = shade_nee_light for a hit at that position of a material with args->roughness / metallic / transmission, whose sampler
 *                      cursor is args->dim, with the render's integrator.  args->tables picks the light table the search and the record load
 *                      read: PT_LIGHT_TABLES_HBM the scene's own, PT_LIGHT_TABLES_LDS a copy staged per block as the shade kernel stages it
 *                      (at most 64 lights).  Both give the same bits.
 *   PT_LIGHT_ENV_MISS  in:  4 floats  direction x y z, lastPdf
 *                      out: 4 floats  the radiance a miss in that direction adds for attenuation 1 at bounce args->bounce after a sample
 *                      that was specular or not (args->lastSpecular), 0
 * PT_ERR_INVALID_ARGUMENT, before the renderer is looked at: fn >= PT_LIGHT_COUNT, n = 0 or n > 2^24, a null args / in / out, args->tables
 * not one of the two; then a null renderer.  PT_ERR_BAD_STATE before pt_start_render.  PT_ERR_UNSUPPORTED: PT_LIGHT_TABLES_LDS with more than
 * 64 lights, PT_LIGHT_ENV_MISS on a render without an environment. */
enum { PT_LIGHT_SAMPLE = 0, PT_LIGHT_ENV_MISS = 1, PT_LIGHT_COUNT = 2 };
enum { PT_LIGHT_TABLES_HBM = 0, PT_LIGHT_TABLES_LDS = 1 };
#define PT_LIGHT_SAMPLE_IN_WORDS 8u
#define PT_LIGHT_SAMPLE_OUT_WORDS 12u
#define PT_LIGHT_ENV_MISS_IN_WORDS 4u
#define PT_LIGHT_ENV_MISS_OUT_WORDS 4u
typedef struct pt_light_probe_args {
  float roughness, metallic, transmission;   /* PT_LIGHT_SAMPLE: the material terms that gate NEE */
  uint32_t dim;                              /* PT_LIGHT_SAMPLE: the sampler cursor at the hit */
  uint32_t tables;                           /* PT_LIGHT_SAMPLE: PT_LIGHT_TABLES_* */
  uint32_t bounce, lastSpecular;             /* PT_LIGHT_ENV_MISS */
} pt_light_probe_args;
int pt_debug_lights(pt_renderer* r, uint32_t fn, uint32_t n, const pt_light_probe_args* args, const void* in, void* out);

/* ---- shading-frame probe (NEW, an additive extension of ABI 5: one entry point) ----
 * Parity surface: the stage between a hit record and the BSDF — the interpolation of normals, tangents and UVs, the instance transform, the
 * tangent frame with and without a normal map, wo, and the shading context with its texture taps — evaluated on the device on its own
 * against the scene of the STARTED render, exactly as the shade and AOV kernels evaluate it.  One elementwise launch on the renderer's
 * stream; upload and read-back inside the call; the render's state is left alone.  `in` holds n records of PT_SHADE_PROBE_IN_WORDS 4-byte
 * words, `out` receives n records of PT_SHADE_PROBE_OUT_WORDS:
 *   in:  instance (uint32), primitive (uint32: the triangle inside the instance's mesh), u, v, ray origin x y z, ray direction x y z, t, 0
 *   out: hitPos x y z, frame.x x y z, frame.y x y z, frame.z x y z, wo x y z, albedo r g b, emission r g b, roughness, metallic,
 *        transmission, clearcoat, clearcoatRoughness, anisotropy, ior, flags (int32), material class (uint32, 0..3), 0, 0
 * u, v, the ray and t are taken as they come: any float is answered (the stage indexes nothing with them but the textures, whose
 * addressing wraps).
 * PT_ERR_INVALID_ARGUMENT, before the renderer is looked at: n = 0 or n > 2^24, a null in / out; then a null renderer.  PT_ERR_BAD_STATE
 * before pt_start_render.  PT_ERR_INVALID_ARGUMENT for a record whose (instance, primitive) names no triangle of the scene: such a batch
 * is refused on the host and nothing is launched. */
#define PT_SHADE_PROBE_IN_WORDS 12u
#define PT_SHADE_PROBE_OUT_WORDS 32u
int pt_debug_shading(pt_renderer* r, uint32_t n, const void* in, void* out);

/* ---- tile-adaptive sampling (NEW, an additive extension of ABI 5: new entry points and one new struct, no existing struct changed) ----
 * A render started while `enabled` is set stops sampling an 8x8 tile of the accumulator once it has converged; pt_render_params.spp
 * becomes the per-pixel maximum.  Checkpoints are at the sample counts c_k = min_spp + k * interval with c_k < spp.  At each, every
 * still-active tile is tested with the luminance moments of its pixels after c_k samples (m1, m2: the running means of lum(L) and
 * lum(L)^2 after the non-finite policy, the same bits as PT_AOV_MOMENTS .g / .b):
 *     var = max(m2 - m1^2, 0) * n / (n - 1),   err = sqrt(var / n) / max(m1, 1e-3)
 * The tile converges when err <= threshold for every one of its pixels inside the image (a NaN err keeps it active).  A converged tile
 * receives no further samples: its accumulator and AOV pixels stay as they were at c_k.  Batches never straddle a checkpoint, so an
 * adaptive render is the same bits for any samples_in_flight and any sequence of pt_render_step calls, and a tile that stopped after n
 * samples equals a uniform render with spp = n on that tile.  A render with spp <= min_spp has no checkpoint.
 * The render ends at spp, or once the host has observed that no tile is active: pt_progress then reports accumulated = total and
 * pt_status Done.  pt_render_step never blocks to find out (the count arrives through pinned memory); pt_wait may synchronise at
 * checkpoints.  pt_trace_primary, pt_debug_sample and pt_measure_traversal stay full-frame.
 * Refused with PT_ERR_UNSUPPORTED: PT_FLAG_GMON together with enabled (at pt_start_render), and enabled = 1 on a device group. */
typedef struct pt_adaptive_options {
  uint32_t enabled;    /* read at pt_start_render; default 0 */
  float threshold;     /* finite and > 0; default 0.02 */
  uint32_t min_spp;    /* >= 2; default 32: the first checkpoint */
  uint32_t interval;   /* >= 1; default 32: samples between checkpoints */
} pt_adaptive_options;
void pt_default_adaptive_options(pt_adaptive_options* o);
/* PT_ERR_INVALID_ARGUMENT for threshold not finite or <= 0, min_spp < 2, interval < 1 */
int pt_set_adaptive_options(pt_renderer* r, const pt_adaptive_options* o);
/* The samples folded into each pixel (W*H values, its tile's count); on a non-adaptive render the uniform count.  Blocks like
 * pt_read_accumulator. */
int pt_read_sample_counts(pt_renderer* r, uint32_t* out);

/* ---- render regions (NEW, an additive extension of ABI 5: new entry points and one new struct, no existing struct changed) ----
 * A render started while `enabled` is set samples only the pixels [x0, x1) x [y0, y1) of the frame (top-left origin): the region R.
 * The sampler is a function of (pixel, sample index), so the render is a restriction of the full-frame one: every accumulator and AOV
 * pixel inside R holds the bits it holds without a region, for any samples_in_flight and any sequence of pt_render_step calls;
 * outside R the accumulator, the AOVs and the denoised image are all-zero bits, alpha included, and pt_read_sample_counts returns 0.
 * pt_stats.paths counts the paths of R only (area(R) * spp for a uniform render).  spp, progress, status and batching are unchanged;
 * enabled = 1 with R equal to the whole frame gives the bits of a render without a region in every output.
 * The denoiser filters R as if it were the whole image: taps outside R are skipped like taps outside the image, the depth gradient is
 * one-sided at R's border and the variance blur sees R only.  Post-processing and present run over the full frame, on R plus zeros.
 * With adaptive sampling the first active tiles are those R touches, and a tile's verdict is taken over its pixels inside R only (a
 * border tile may stop earlier than in a full-frame adaptive render); everything else is as stated above for adaptive sampling.
 * pt_trace_primary, pt_debug_sample and pt_measure_traversal stay full-frame.  The queues are sized for the frame (pt_plan_queues).
 * Refused with PT_ERR_UNSUPPORTED: PT_FLAG_GMON together with enabled (at pt_start_render), and enabled = 1 on a device group.
 * pt_start_render returns PT_ERR_INVALID_ARGUMENT when x1 > width or y1 > height. */
typedef struct pt_render_region {
  uint32_t enabled;         /* read at pt_start_render; default 0: the whole frame */
  uint32_t x0, y0, x1, y1;  /* pixels [x0, x1) x [y0, y1) */
} pt_render_region;
void pt_default_render_region(pt_render_region* o);
/* PT_ERR_INVALID_ARGUMENT for enabled with x0 >= x1 or y0 >= y1 */
int pt_set_render_region(pt_renderer* r, const pt_render_region* o);
/* Pure host arithmetic (exported for tests, like pt_plan_queues): the 8x8 image tiles (row-major, (W + 7) / 8 per row) a region
 * activates, ascending; every tile when enabled = 0.  Writes up to `capacity` of them and their total number to *count. */
int pt_region_tiles(uint32_t width, uint32_t height, const pt_render_region* o, uint32_t* tiles_out, uint32_t capacity, uint32_t* count);

/* ---- camera-ray leaf lists (NEW, an additive extension of ABI 5: one new entry point and one new struct, no existing struct changed) ----
 * At pt_start_render, for a pinhole camera (apertureRadius <= 0) over the one-BVH structure in its 6-wide form, a full-frame non-adaptive
 * render builds for every pixel the list of tree nodes whose leaf children the pixel's camera rays can reach, and traces bounce 0 of every
 * batch from it instead of walking the tree from the root once per sample.  Every output is the bits of a render without the lists
 * ($PTAMD_NO_CAMERA_LISTS=1 keeps them off).  A pixel whose list does not fit `capacity` entries is traced by the ordinary traversal.
 * Not built (built = 0, everything else 0) for: a thin-lens camera, the two-level structure, 4-wide nodes, adaptive sampling, a render
 * region, $PTAMD_NO_CAMERA_LISTS, or when the lists would take more than 1/16 of the free device memory. */
#define PT_CAMLIST_HIST_BINS 65
typedef struct pt_camera_list_stats {
  uint32_t built;           /* 1: this render traces its camera rays from the lists */
  uint32_t capacity;        /* entries per pixel */
  uint64_t pixels_listed;   /* pixels with a list (an empty one included) */
  uint64_t pixels_walk;     /* pixels whose list did not fit: traced by the ordinary traversal */
  uint64_t entries;         /* entries of all lists */
  double build_ms;          /* device time of the build (HIP events) */
  uint32_t length_histogram[PT_CAMLIST_HIST_BINS];  /* pixels by list length before the capacity is applied: 0 .. 63, 64 or more */
  uint32_t _pad;
} pt_camera_list_stats;
/* PT_ERR_BAD_STATE before pt_start_render.  Does not block. */
int pt_get_camera_list_stats(pt_renderer* r, pt_camera_list_stats* out);

/* ---- ID mattes (NEW, an additive extension of ABI 5: new entry points and three new structs, no existing struct changed) ----
 * A render started while `enabled` is set keeps, beside the accumulator, what each pixel's camera rays hit first: two layers of
 * PT_MATTE_SLOTS slots {id, count} per pixel.
 *   PT_MATTE_INSTANCE  id = the index of the hit instance in pt_scene_snapshot.instances
 *   PT_MATTE_MATERIAL  id = the index of the hit triangle's material in the flattened material table:
 *                      (sum of instance_materials[j].material_count over the instances j before the hit one) + the triangle's material slot
 * A camera ray that hits nothing has the id PT_MATTE_NONE on both layers, and takes a slot like any other id.
 * The fold: a pixel's samples are folded in sample order 0, 1, 2, ...  The slots are scanned 0 .. PT_MATTE_SLOTS - 1: the first slot with
 * count != 0 and the sample's id gets count + 1; otherwise the first slot with count == 0 becomes {id, 1}; otherwise the sample goes to
 * nothing.  Slots are first come, with no eviction; an empty slot is {PT_MATTE_NONE, 0}.  With n the pixel's sample count
 * (pt_read_sample_counts), other = n - (the sum of the counts) is the number of samples that found no slot: 0 wherever at most
 * PT_MATTE_SLOTS distinct ids were seen.  The slots are a function of the ordered sample sequence: the same bits for any samples_in_flight
 * and any sequence of pt_render_step calls, for every acceleration structure and with or without the camera-ray leaf lists.
 * Mattes work with GMoN, render regions (pixels outside the region keep empty slots), adaptive sampling (a tile's slots stop with the
 * tile), thin-lens cameras and every acceleration structure; they are independent of the AOVs and the denoiser, and every other output of
 * the render is the bits it is without them.  pt_trace_primary, pt_debug_sample and pt_measure_traversal never touch the slots.
 * Memory: 8 B per path slot and 128 B per pixel, held only by a render that enabled mattes.  pt_plan_queues describes matte-off renders.
 * Refused with PT_ERR_UNSUPPORTED: enabled = 1 on a device group (slot lists do not merge by a sum). */
#define PT_MATTE_SLOTS 8
#define PT_MATTE_NONE 0xFFFFFFFFu
enum { PT_MATTE_INSTANCE = 0, PT_MATTE_MATERIAL = 1 };
typedef struct pt_matte_options {
  uint32_t enabled;         /* read at pt_start_render; default 0 */
} pt_matte_options;
typedef struct pt_matte_slot {
  uint32_t id, count;
} pt_matte_slot;
void pt_default_matte_options(pt_matte_options* o);
int pt_set_matte_options(pt_renderer* r, const pt_matte_options* o);
/* The slots of one layer, W*H*PT_MATTE_SLOTS of them: pixel-major (row-major pixels), each pixel's slots in first-seen order.  Blocks like
 * pt_read_accumulator.  PT_ERR_INVALID_ARGUMENT for a layer that does not exist; PT_ERR_BAD_STATE before pt_start_render and for a render
 * started without mattes (pt_read_matte and pt_pick alike). */
int pt_read_matte_slots(pt_renderer* r, uint32_t layer, pt_matte_slot* out);
/* Coverage of the id set ids[0, id_count) (any order, duplicates allowed; PT_MATTE_NONE selects the background) per pixel, W*H floats:
 * (float)(the sum of the counts of the pixel's slots whose id is in the set) / (float)n, one IEEE division; 0 where n = 0 and for the empty
 * set.  One kernel over the slots; blocks.  PT_ERR_INVALID_ARGUMENT for a bad layer, or ids NULL with id_count > 0. */
int pt_read_matte(pt_renderer* r, uint32_t layer, const uint32_t* ids, uint32_t id_count, float* coverage_out);
typedef struct pt_pick_result {
  uint32_t instance, instance_count;          /* the instance-layer slot with the largest count, ties to the lowest slot; PT_MATTE_NONE = background */
  uint32_t material, material_count;          /* the same on the material layer */
  uint32_t material_instance, material_slot;  /* `material` decoded into the caller's (instance, material slot); PT_MATTE_NONE for background */
  uint32_t samples, _pad;                     /* the pixel's n */
} pt_pick_result;
/* What is under pixel (x, y), top-left origin: one 128-byte read-back after a stream sync, no kernel (an adaptive render reads its tile's
 * sample count too).  PT_ERR_INVALID_ARGUMENT for x >= width or y >= height. */
int pt_pick(pt_renderer* r, uint32_t x, uint32_t y, pt_pick_result* out);

/* ---- selection overlay (NEW, an additive extension of ABI 5: new entry points and one new struct, no existing struct changed) ----
 * With `enabled` set, every pt_read_render_target and pt_present_render_target of a render that keeps ID mattes draws, as the last step of
 * the display chain (after the post-process, on the RGBA8 target, on the device), an antialiased outline around the pixels covered by the
 * ids of pt_set_selection on `layer`, and a tint over them.  The colours are UI colours in the target's own encoding: they do not go
 * through auto exposure, bloom, the post-process or the tonemapper.
 * Per pixel p, with m(p) the coverage pt_read_matte gives for the set (0 outside a render region and where no sample was taken) and c a
 * channel's byte / 255:
 *   lim = width + 0.5, R = ceil(lim) - 1, k(dx, dy) = min(max(lim - sqrt(dx^2 + dy^2), 0), 1)
 *   D(p) = max over |dx|, |dy| <= R with p + (dx, dy) inside the frame of m(p + (dx, dy)) * k(dx, dy)          (>= m(p): k(0, 0) = 1)
 *   af = m * fill_rgba[3], ao = (D - m) * outline_rgba[3]
 *   c1 = c * (1 - af) + fill * af, c2 = c1 * (1 - ao) + outline * ao, byte = c2 clamped to [0, 1], * 255 + 0.5, truncated
 * in fp32, one IEEE operation each.  The band lies outside the silhouette, `width` pixels wide and soft where the coverage is fractional;
 * alpha 0 keeps a byte, alpha 1 gives exactly the colour's byte, a pixel with af = ao = 0 keeps its four bytes and the alpha byte is never
 * changed.  The options and the set are read by every target read and present: no restart is needed.
 * Nothing is drawn, allocated or launched, silently, when enabled = 0, when the set is empty, when the render was started without mattes,
 * and on a device group (which keeps no mattes).  The accumulator, the AOVs, the slots, the exposure meter and pt_read_exposure_meter are
 * unaffected either way.
 * PT_ERR_INVALID_ARGUMENT (checked before the renderer): a layer that does not exist, width not in [1, 16], a colour component not in
 * [0, 1] (NaN included).  PT_ERR_UNSUPPORTED: enabled = 1 on a device group. */
typedef struct pt_selection_options {
  uint32_t enabled;         /* default 0 */
  uint32_t layer;           /* PT_MATTE_INSTANCE (default) or PT_MATTE_MATERIAL: what the ids of pt_set_selection are */
  float width;              /* outline width in pixels, 1 .. 16; default 2 */
  float _pad;
  float outline_rgba[4];    /* default (1, 0.55, 0, 1) */
  float fill_rgba[4];       /* default (1, 0.55, 0, 0): no tint */
} pt_selection_options;
void pt_default_selection_options(pt_selection_options* o);
int pt_set_selection_options(pt_renderer* r, const pt_selection_options* o);
/* The selected ids: any order, duplicates allowed, PT_MATTE_NONE selects the background; id_count = 0 clears the selection.  The set is kept
 * sorted and without duplicates, and survives pt_start_render.  Its upload is ordered on the renderer's stream (a present enqueued before the
 * call draws the earlier set) and waited for.  PT_ERR_INVALID_ARGUMENT for ids NULL with id_count > 0. */
int pt_set_selection(pt_renderer* r, const uint32_t* ids, uint32_t id_count);
/* Copies up to `capacity` ids of the stored set (ascending); returns their number in *count.  ids_out may be NULL with capacity 0. */
int pt_get_selection(const pt_renderer* r, uint32_t* ids_out, uint32_t capacity, uint32_t* count);
/* The overlay kernel on an uploaded target (width*height RGBA8 pixels) and coverage image (width*height floats) with buffers of its own:
 * needs no render and leaves the renderer's state alone; `enabled` is not looked at.  1 .. 2^28 pixels. */
int pt_debug_selection_overlay(pt_renderer* r, const uint8_t* rgba8_in, const float* coverage, uint32_t width, uint32_t height,
                               const pt_selection_options* options, uint8_t* rgba8_out);

/* ---- transparent film (NEW, an additive extension of ABI 5: new entry points and one new struct, no existing struct changed) ----
 * A render started while `enabled` is set keeps, beside the accumulator, one more W*H RGBA32F image, the FILM: per pixel the running mean
 * (the accumulator's recurrence, in sample order, one IEEE fp32 operation each) of
 *   x_s = the camera ray of sample s hit geometry ? {L_s.r, L_s.g, L_s.b, 1} : {0, 0, 0, 0}
 * with L_s the sample's radiance after the non-finite policy (what the accumulator folds).  A ray that passes a stochastic alpha cut-out
 * and then leaves the scene is a miss.  The miss case is a select: a NaN sample that missed contributes 0.  So film.rgb is the
 * premultiplied foreground and film.a the coverage; at a pixel every sample of which hit, film.rgb is the accumulator's rgb bit for bit
 * (without GMoN; under PT_FLAG_GMON the film is a plain running mean, as the AOVs are).  The bits do not depend on samples_in_flight or on
 * the sequence of pt_render_step calls.  A region render leaves the film {0, 0, 0, 0} outside the rectangle; an adaptive render's tile
 * holds the film of its own sample count.  Every other output of the render is the bits it is without the film.
 * `backdrop` and `backdrop_rgb` are read by every pt_read_render_target / pt_present_render_target / pt_read_exposure_meter of a render
 * that keeps a film (no restart is needed); they choose the image the display chain starts from, with a = film.a and base = film.rgb (with
 * denoise.apply_to_target on a render that also keeps AOVs: the a-trous filter run over film.rgb in place of the accumulator; the
 * luminance moments that drive it still describe the full radiance):
 *   PT_BACKDROP_SCENE        the accumulator (or its denoised image): the chain of a render without a film, bit for bit
 *   PT_BACKDROP_COLOR        base.c + backdrop_rgb.c * (1 - a) per channel; the target's alpha byte stays 255
 *   PT_BACKDROP_TRANSPARENT  a > 0 ? base.c / a : 0, the unpremultiplied foreground; after the post-process the target's alpha byte is
 *                            a quantised as the colour bytes are (<= 0 or NaN: 0, >= 1: 255, else (uint32)(a * 255 + 0.5)): straight alpha
 * Outside a render region the composed source is 0 (alpha byte 0 when transparent).  Auto exposure, bloom and the exposure meter take the
 * composed source.  The selection overlay draws after the alpha byte is written and never changes it.  backdrop_rgb is scene-linear, in
 * the render's working space.  A backdrop other than SCENE on a render without a film, and on a device group, silently shows the accumulator.
 * Memory: 4 B per path slot and 16 B per pixel, held only by a render that enabled the film (plus 16 B per pixel once a backdrop is shown).
 * PT_ERR_INVALID_ARGUMENT (checked before the renderer): an unknown backdrop, a colour component that is negative or not finite.
 * PT_ERR_UNSUPPORTED: enabled = 1 on a device group. */
enum { PT_BACKDROP_SCENE = 0, PT_BACKDROP_COLOR = 1, PT_BACKDROP_TRANSPARENT = 2 };
typedef struct pt_film_options {
  uint32_t enabled;        /* keep the film for renders started from now on (read at pt_start_render); default 0 */
  uint32_t backdrop;       /* default PT_BACKDROP_SCENE; read by every target read / present */
  float backdrop_rgb[3];   /* finite and >= 0; default 0 */
} pt_film_options;
void pt_default_film_options(pt_film_options* o);
int pt_set_film_options(pt_renderer* r, const pt_film_options* o);
/* The film, W*H*4 floats {premultiplied foreground rgb, coverage}.  Blocks like pt_read_aov.  PT_ERR_BAD_STATE before pt_start_render and
 * for a render started without the film. */
int pt_read_film(pt_renderer* r, float* rgba_out);

/* ---- pass views (NEW, an additive extension of ABI 5: new entry points and new structs, no existing struct changed) ----
 * A view selector for the render target: what pt_read_render_target / pt_present_render_target show of the data the render keeps beside the
 * accumulator.  The options are read by every target read and present (no restart); under the default, PT_VIEW_BEAUTY, nothing is allocated
 * or launched and every output keeps its bits.
 *   PT_VIEW_BEAUTY   the display chain as it is
 *   PT_VIEW_ALBEDO   the albedo AOV (a scene-linear colour in the working space) in place of the chain's source; auto exposure and bloom are
 *                    skipped (the exposure smoothing state does not advance), the post-process and the tonemapper run as ever
 * Every other view is a DATA view: one kernel writes the target directly with alpha byte 255, in place of source, exposure, bloom,
 * post-process and the film's alpha byte; nothing of the colour pipeline touches data.  With n the pixel's sample count as
 * pt_read_sample_counts gives it, a pixel with n = 0 is (0, 0, 0, 255); every step is one IEEE fp32 operation and the bytes are quantised as
 * the post-process quantises them (<= 0 or NaN: 0, >= 1: 255, else (uint32)(c * 255 + 0.5)):
 *   PT_VIEW_NORMAL   c = N.c * 0.5 + 0.5 of the normal AOV's rgb (a miss-only pixel is mid grey)
 *   PT_VIEW_DEPTH    with h the normal AOV's alpha and r the moments AOV's .r, a pixel is valid when n > 0, h > 0 and d = r / h is finite and
 *                    >= 0.  auto_range: z0, z1 = the min and max of d over the valid pixels of the render's rectangle, found on the device
 *                    (0, 0 when there is none); else z0, z1 = depth_min, depth_max.  t = z1 > z0 ? (d - z0) / (z1 - z0) : 0 clamped to [0, 1],
 *                    v = 1 - t (near is bright), colour = ramp(v); an invalid pixel is black
 *   PT_VIEW_ALPHA    v = film.a, grey
 *   PT_VIEW_MATTE    colour = the sum over the slots k = 0 .. 7 of `layer`, in order from 0, of w_k * col(id_k), w_k = (float)count_k / (float)n
 *                    (a slot with count 0 is skipped); col(PT_MATTE_NONE) = 0, else with x = id hashed by x ^= x >> 16, x *= 0x7feb352d,
 *                    x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16: col.c = (float)byte_c(x) / 255 * 0.75 + 0.25 for bytes 0, 1, 2 = r, g, b.
 *                    Samples that found no slot darken the pixel.
 *   PT_VIEW_SAMPLES  v = min((float)n / (float)spp, 1), colour = ramp(v): the heat map of an adaptive or region render
 *   PT_VIEW_NOISE    err = the relative standard error of adaptive sampling's criterion from the luminance moments m1, m2 (PT_AOV_MOMENTS .g, .b,
 *                    the same bits as the adaptive moments); v = 1 when n < 2 or err is NaN, else min(err / noise_max, 1); colour = ramp(v)
 *   ramp             PT_RAMP_GREY: (v, v, v).  PT_RAMP_HEAT: s = v * 4, k = min((int)s, 3), f = s - k, c = a_k + (a_(k+1) - a_k) * f over the
 *                    stops blue (0,0,1), cyan (0,1,1), green (0,1,0), yellow (1,1,0), red (1,0,0).  A NaN v is drawn as v = 1.
 * Availability: ALBEDO, NORMAL and DEPTH need a render that keeps AOVs, ALPHA the film, MATTE the ID mattes, NOISE AOVs or adaptive sampling;
 * SAMPLES is always available.  A view whose data the render does not keep, and any view on a device group's merged image, silently shows
 * BEAUTY (as a film backdrop does on a render without a film); pt_view_stats.shown says which view the target shows.
 * The selection overlay still draws on top of every view.  Present never blocks: the depth range lives in a 16-byte device record the view
 * kernel reads.  pt_read_exposure_meter ignores the view.
 * PT_ERR_INVALID_ARGUMENT (checked before the renderer): view >= PT_VIEW_COUNT, a layer or ramp that does not exist, auto_range > 1, with
 * auto_range = 0 a depth_min or depth_max that is not finite, depth_min < 0 or depth_min >= depth_max, a noise_max that is not finite or <= 0.
 * Never refused on a device group: the options go to every member. */
enum { PT_VIEW_BEAUTY = 0, PT_VIEW_ALBEDO = 1, PT_VIEW_NORMAL = 2, PT_VIEW_DEPTH = 3,
       PT_VIEW_ALPHA = 4, PT_VIEW_MATTE = 5, PT_VIEW_SAMPLES = 6, PT_VIEW_NOISE = 7, PT_VIEW_COUNT = 8 };
enum { PT_RAMP_GREY = 0, PT_RAMP_HEAT = 1 };
typedef struct pt_view_options {
  uint32_t view;        /* default PT_VIEW_BEAUTY; read by every target read / present, no restart */
  uint32_t layer;       /* PT_VIEW_MATTE: PT_MATTE_INSTANCE (default) or PT_MATTE_MATERIAL */
  uint32_t ramp;        /* DEPTH, SAMPLES, NOISE: PT_RAMP_GREY (default) or PT_RAMP_HEAT */
  uint32_t auto_range;  /* DEPTH: 1 (default) = range from the frame's own nearest / farthest hit, found on the device */
  float depth_min, depth_max;   /* DEPTH with auto_range = 0; defaults 0, 1 */
  float noise_max;      /* NOISE: the relative error drawn as full scale; default 0.1 */
  uint32_t _pad;
} pt_view_options;
void pt_default_view_options(pt_view_options* o);
int pt_set_view_options(pt_renderer* r, const pt_view_options* o);

typedef struct pt_view_stats {
  uint32_t shown;          /* the view the target shows now (BEAUTY when the asked one is not available) */
  uint32_t depth_pixels;   /* DEPTH: pixels that entered the range */
  float depth_min, depth_max;   /* DEPTH: z0, z1 as used */
} pt_view_stats;
/* Blocks; runs the range pass when DEPTH is shown (0, 0, 0 under any other view) and draws nothing.  PT_ERR_BAD_STATE before pt_start_render. */
int pt_read_view_stats(pt_renderer* r, pt_view_stats* out);

typedef struct pt_view_inputs {   /* any pointer the view does not read may be NULL */
  const float *albedo, *normal, *moments, *film;   /* W*H*4 floats each, as pt_read_aov / pt_read_film give them */
  const pt_matte_slot* slots;                        /* W*H*PT_MATTE_SLOTS of one layer, as pt_read_matte_slots */
  const uint32_t* counts;                            /* W*H, as pt_read_sample_counts */
  uint32_t spp;                                      /* SAMPLES: the render's spp */
} pt_view_inputs;
/* The data-view kernels on uploaded inputs with buffers of their own: needs no render and leaves the renderer's state alone.  `rect`
 * {x0, y0, x1, y1} (NULL = the whole image) is the rectangle the depth range is taken over.  1 .. 2^28 pixels.  PT_ERR_INVALID_ARGUMENT also
 * for BEAUTY and ALBEDO (they go through the post-process), for a NULL input the view reads (counts always), and for SAMPLES with spp = 0.
 * stats_out may be NULL. */
int pt_debug_view(pt_renderer* r, const pt_view_inputs* in, uint32_t width, uint32_t height, const uint32_t* rect,
                  const pt_view_options* options, uint8_t* rgba8_out, pt_view_stats* stats_out);

/* ---- camera projections (NEW, an additive extension of ABI 5: new entry points and one new struct, no existing struct changed) ----
 * How the camera rays of a render are made.  The projection is read at pt_start_render; under the default, PT_PROJ_PERSPECTIVE, every
 * output and every launch is what it is without this block, bit for bit.  pt_camera, pt_camera_data and pt_constants do not change, and
 * pt_get_constants returns under every projection what it returns under PERSPECTIVE.
 * With u, v, w the normalised columns 0..2 of pt_camera.world (its scale removed, as for the perspective camera; the camera looks down -w),
 * pos its column 3, and (fx, fy) = (px + jitter.x, py + jitter.y) the sample position in pixels (Halton dimensions 0-1, formed in fp32):
 *   PT_PROJ_ORTHOGRAPHIC  the view volume is ortho_height high and ortho_height * W / H wide, centred on pos: o = pos + (fx / W - 1/2) * width * u
 *                         - (fy / H - 1/2) * ortho_height * v, d = -w.  No near or far plane: the ray starts on the camera's plane.
 *   PT_PROJ_EQUIRECT      phi = (fx / W - 1/2) * fov_x, theta = pi/2 + (fy / H - 1/2) * fov_y,
 *                         d = sin(theta) sin(phi) u + cos(theta) v - sin(theta) cos(phi) w, o = pos.  With the defaults and a camera with
 *                         u = +z, v = +y, w = -x (looking along +x, y up) the image has the layout of an environment map, pixel for texel.
 *   PT_PROJ_FISHEYE       equidistant: half = min(W, H) / 2, x = (fx - W/2) / half, y = (H/2 - fy) / half, r = |(x, y)|,
 *                         theta = min(r * fisheye_fov / 2, pi), d = sin(theta) (x/r) u + sin(theta) (y/r) v - cos(theta) w (r = 0: d = -w),
 *                         o = pos.  Every pixel gets a ray: the corners continue the mapping beyond the image circle.
 * The image centre looks down -w, x grows to the right and y grows down, as under PERSPECTIVE.  Every kind other than PERSPECTIVE is a
 * pinhole: pt_camera.aperture (and sensor_size, focal_length, focus_distance) is IGNORED, Halton dimensions 2-3 are consumed and not
 * evaluated, so a path draws from bounce 1 on what it draws under a perspective pinhole.  A render under such a kind builds no camera-ray
 * leaf lists (pt_camera_list_stats.built = 0) and walks the tree at bounce 0; AOVs, mattes, the film, adaptive sampling, regions and pass
 * views work as ever, and pt_trace_primary, pt_debug_sample and pt_measure_traversal follow the projection.
 * PT_ERR_INVALID_ARGUMENT (checked before the renderer): an unknown kind; of the fields of the chosen kind (the others are ignored) one that
 * is not finite, ortho_height <= 0, fov_x outside (0, 2 pi], fov_y outside (0, pi], fisheye_fov outside (0, 2 pi] (the bounds are the
 * fp32 values of 2 pi and pi).  PT_ERR_UNSUPPORTED: a kind other than PERSPECTIVE on a device group. */
enum { PT_PROJ_PERSPECTIVE = 0, PT_PROJ_ORTHOGRAPHIC = 1, PT_PROJ_EQUIRECT = 2, PT_PROJ_FISHEYE = 3 };
typedef struct pt_camera_projection {
  uint32_t kind;        /* PT_PROJ_*; default PERSPECTIVE */
  float ortho_height;   /* ORTHOGRAPHIC: height of the view volume in world units, > 0; the width follows the image's aspect; default 1 */
  float fov_x, fov_y;   /* EQUIRECT: radians covered horizontally (0, 2 pi] and vertically (0, pi]; defaults 2 pi, pi */
  float fisheye_fov;    /* FISHEYE (equidistant): full angle reached at the shorter side's edge, (0, 2 pi]; default pi */
  uint32_t _pad[3];
} pt_camera_projection;
void pt_default_camera_projection(pt_camera_projection* p);
int pt_set_camera_projection(pt_renderer* r, const pt_camera_projection* p);   /* read at the next pt_start_render */
/* What the current render was started with.  PT_ERR_BAD_STATE before pt_start_render. */
int pt_get_camera_projection(pt_renderer* r, pt_camera_projection* out);
/* The camera rays of sample `sample_idx` of every pixel, W*H*3 floats each, row-major: the ray-generation kernel a full-frame render batch
 * of one sample launches under the current render's projection (PERSPECTIVE: k_raygen), its queue scattered back to pixel order.  Either
 * pointer may be NULL.  Full-frame like pt_trace_primary; blocks.  PT_ERR_BAD_STATE before pt_start_render. */
int pt_debug_camera_rays(pt_renderer* r, uint32_t sample_idx, float* origins /* W*H*3 */, float* directions /* W*H*3 */);

/* ---- ambient occlusion (NEW, an additive extension of ABI 5: new entry points and new structs, no existing struct changed) ----
 * A render started while `enabled` is set traces, for every camera ray that hit geometry, ONE more ray from the hit and keeps per pixel two
 * integers: `hits`, the camera rays of the pixel's samples that hit, and `open`, those of them whose AO ray met nothing.  The AO ray:
 *   origin     o + d * t of the camera ray and its first hit, in fp32 (the point shading starts from)
 *   normal     the hit triangle's world-space GEOMETRIC normal normalize(M * n) through the instance's forward matrix (the reference's
 *              definition: under a non-uniform scale it is not the true normal), turned to face the viewer: -n when dot(n, d) > 0
 *   direction  cosine-weighted about that normal, from a Halton stream of AO's own: index pcg4d(offset, salt, 0, 0).x of the path's
 *              offset, dimensions 0-1 (dimension 2: the alpha-test draw of a scene with cut-outs).  No draw of the path itself moves.
 *   range      [1e-3, distance], any hit; cut-outs are tested as for shadow rays.  distance = +inf is allowed.
 * pt_read_ao gives open / hits per pixel (1 where hits = 0).  The counts are integers: they do not depend on samples_in_flight, on the
 * sequence of pt_render_step calls or on the queue layout.  A region render leaves {0, 0} (AO 1) outside the rectangle; an adaptive
 * render's tile holds the counts of its own samples.  Thin-lens and projected cameras work as ever (the origin is the queue's).  Every other
 * output of the render, pt_stats' ray counters included, is the bits it is without AO; the AO trace and fold are timed on their own
 * (pt_ao_stats), not in pt_stats' classes.  There is no AO pass view.
 * Memory: 4 B per path slot and 8 B per pixel, held only by a render that enabled AO.
 * PT_ERR_INVALID_ARGUMENT (checked before the renderer): enabled > 1, a distance that is NaN or <= 0.  PT_ERR_UNSUPPORTED: enabled = 1, the
 * reads and pt_debug_ao on a device group. */
typedef struct pt_ao_options {
  uint32_t enabled;    /* keep AO for renders started from now on (read at pt_start_render); default 0 */
  float distance;      /* the AO rays' far limit in world units, > 0, +inf allowed; default 1 */
  uint32_t _pad[2];
} pt_ao_options;
void pt_default_ao_options(pt_ao_options* o);
int pt_set_ao_options(pt_renderer* r, const pt_ao_options* o);
/* open / hits per pixel, W*H floats.  Blocks like pt_read_aov.  PT_ERR_BAD_STATE before pt_start_render and for a render started without AO. */
int pt_read_ao(pt_renderer* r, float* out /* W*H */);
/* {hits, open} per pixel, W*H*2 words.  Blocks; errors as pt_read_ao. */
int pt_read_ao_counts(pt_renderer* r, uint32_t* out /* W*H*2 */);
/* One sample of every pixel in pixel order: the batch pt_trace_primary runs, then the AO trace of a render batch, which also logs its rays.
 * state: 0 the camera ray missed (origin and direction 0), 1 hit and AO ray occluded, 2 hit and AO ray unoccluded.  Any pointer may be
 * NULL.  Full-frame; blocks; leaves the render's accumulated state alone.  Errors as pt_read_ao. */
int pt_debug_ao(pt_renderer* r, uint32_t sample_idx, float* origins /* W*H*3 */, float* directions /* W*H*3 */, uint32_t* state /* W*H */);
typedef struct pt_ao_stats {
  uint64_t rays;             /* AO rays traced since pt_start_render (= the sum of hits over the frame) */
  float ms_trace, ms_fold;   /* device time of the AO trace / the AO fold since pt_start_render, under pt_set_profiling */
} pt_ao_stats;
/* Blocks (it sums the counts).  Errors as pt_read_ao. */
int pt_get_ao_stats(pt_renderer* r, pt_ao_stats* out);

const char* pt_last_error(void);

/* ---------------------------------------------------------------------------------------------------------- */
/* Parity / measurement surface (no reference counterpart; used by tests and bench.py)                          */

int pt_get_constants(const pt_renderer* r, pt_constants* out);
/* The environment alias table in use (given or built): copies up to `capacity` entries; *count = width*height or 0. */
int pt_get_env_alias(const pt_renderer* r, pt_alias_entry* out, uint64_t capacity, uint64_t* count);
/* Copies up to `capacity` lights; returns the light count in *count. */
int pt_get_lights(const pt_renderer* r, pt_area_light* out, uint32_t capacity, uint32_t* count);

/* Closest-hit record of the camera ray of every pixel for sample `sample_idx` (raygen + traversal only). */
typedef struct pt_hit_record {
  float t, u, v;
  int32_t instance; /* -1 = miss */
  int32_t primitive;
} pt_hit_record;
int pt_trace_primary(pt_renderer* r, uint32_t sample_idx, pt_hit_record* out /* W*H */);

/* Trace ONE sample without touching the accumulator; returns its radiance and the (instance, primitive)
 * hit at every bounce of every pixel's path (-1,-1 where the path was already dead or missed).
 *   radiance_out : W*H*4 floats (rgb, 1)               or NULL
 *   hits_out     : max_bounces * W*H * 2 int32          or NULL */
int pt_debug_sample(pt_renderer* r, uint32_t sample_idx, float* radiance_out, int32_t* hits_out);

typedef struct pt_stats {
  uint64_t triangles;          /* flattened world-space triangles */
  uint64_t bvh_nodes;
  uint32_t bvh_max_depth;      /* levels of the tree (two-level: TLAS + deepest BLAS); the traversal stack holds <= 5 entries per level of the
                                  6-wide form the one-BVH structure is built in by default, <= 3 of the 4-wide form ($PTAMD_BVH4, the radix tree, a tree too deep for the 6-wide form) */
  uint32_t samples_in_flight;
  double upload_ms;            /* snapshot -> HBM */
  double bvh_build_ms;         /* LBVH build (device time) */
  uint64_t closest_rays;       /* rays traced since pt_start_render */
  uint64_t shadow_rays;
  uint64_t shaded_hits;
  uint64_t paths;              /* pixel*samples started */
  uint64_t nonfinite_samples;  /* samples whose radiance was NaN/inf (zeroed under PT_NONFINITE_ZERO) */
  /* device time per kernel class since pt_start_render, HIP events on the launch stream */
  double ms_raygen, ms_closest, ms_shade, ms_shadow, ms_accumulate;
  uint64_t launches_closest, launches_shadow;
  /* instrumented traversal (pt_measure_traversal): mean BVH nodes / triangles fetched per ray */
  double nodes_per_closest_ray, tris_per_closest_ray;
  double nodes_per_shadow_ray, tris_per_shadow_ray;
  uint32_t accel_two_level;    /* 1: the two-level structure is in use */
  uint32_t batches;            /* batches enqueued since pt_start_render (pt_render_step calls that arrive while the GPU is busy are merged) */
  uint64_t leaf_slots;         /* 64-byte leaf slots of the acceleration structure: a slot holds one triangle, or two of one instance that share an
                                  edge (one-BVH structure); tris_per_*_ray count triangle TESTS, a slot fetch serves one or two of them */
} pt_stats;
int pt_get_stats(pt_renderer* r, pt_stats* out);
/* Enable per-kernel HIP-event timing (adds two event records per launch). */
int pt_set_profiling(pt_renderer* r, int enabled);
/* Run one instrumented sample (outside any timed region) to count node/triangle fetches per ray. */
int pt_measure_traversal(pt_renderer* r, uint32_t sample_idx);

#ifdef __cplusplus
}
#endif
#endif /* PTAMD_H */
