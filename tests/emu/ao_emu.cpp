// TEST HARNESS ONLY (tests/emu) — the host build of the ambient-occlusion pass (platinum_amd/csrc/pt_ao.h: stage_ao, ao_fold, ao_value,
// ao_options_error) on top of the host harness's scene and traversal, for tests/ao_lib.py.  A library of its own (tests/host_build.py
// load(src, lib)): host_harness.cpp stays as it is.  Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
#include "wavefront_emu.cpp"  // emu_*: host scene + BVH (Emu), traverse<>
#include "../../platinum_amd/csrc/pt_ao.h"
#include "../../platinum_amd/csrc/pt_projection.h"

namespace {

// What k_trace_ao does for one camera ray: the state, and the AO ray when the camera ray hit.  `proj` null or PERSPECTIVE: stage_raygen.
uint32_t ao_one(const Emu* e, const ProjectionConstants* P, uint32_t x, uint32_t y, uint32_t sample, float distance, TravScratch& scratch, AoRay* ray) {
  const DeviceScene& S = e->S;
  const RayGenOut rg = P ? stage_raygen_projected(S, *P, x, y, sample) : stage_raygen(S, x, y, sample);
  TraversalStack st = scratch.stack();
  TraversalCount tc;
  const float ir = S.has_alpha ? Halton{halton_table(S.halton), rg.offset, rg.dim}.sample1d() : 0.0f;
  const RayHit hit = traverse<false, false>(S, rg.o, rg.d, 1e-3f, kInf, ir, st, &tc);
  if (hit.tri == kInvalidRef) return kAoMiss;
  const AoRay a = stage_ao(S, rg.o, rg.d, hit.t, hit_word(hit), rg.offset);
  if (ray) *ray = a;
  const RayHit sh = traverse<true, false>(S, a.o, a.d, kAoTmin, distance, a.payload, st, &tc);
  return sh.tri == kInvalidRef ? kAoOpen : kAoOccluded;
}

struct MaybeProjection {
  ProjectionConstants P;
  bool on;
  MaybeProjection(const Emu* e, const pt_camera* cam, const pt_camera_projection* p) : on(cam && p && p->kind != PT_PROJ_PERSPECTIVE) {
    if (on) P = derive_projection(*cam, e->S.width, e->S.height, *p);
  }
  const ProjectionConstants* get() const { return on ? &P : nullptr; }
};

}  // namespace

extern "C" {

// 0 = the options are accepted, 1 = refused (pt_set_ao_options' test)
int ao_refused(const pt_ao_options* o) { return ao_options_error(*o) != nullptr; }
// {sizeof, offsets of enabled and distance} of pt_ao_options, {sizeof, offsets of rays, ms_trace, ms_fold} of pt_ao_stats
void ao_layout(uint32_t* out /*7*/) {
  const uint32_t v[7] = {sizeof(pt_ao_options), offsetof(pt_ao_options, enabled), offsetof(pt_ao_options, distance), sizeof(pt_ao_stats),
                         offsetof(pt_ao_stats, rays), offsetof(pt_ao_stats, ms_trace), offsetof(pt_ao_stats, ms_fold)};
  for (int i = 0; i < 7; i++) out[i] = v[i];
}
// host_scene.h queue_budget of a render without AOVs, mattes or a film, with AO on or off
uint64_t ao_queue_budget(uint64_t free_bytes, uint64_t queues_held, int ao, uint64_t obuf_held) {
  return queue_budget(free_bytes, queues_held, 0, false, 0, false, 0, false, 0, ao != 0, obuf_held);
}
uint32_t ao_salt() { return PT_AO_SALT; }
uint32_t ao_index_of(uint32_t offset) { return ao_index(offset); }
float ao_value_of(uint32_t hits, uint32_t open) { return ao_value(hits, open); }
// counts[2 * i .. + 2) = ao_fold(counts[...], states[i]) for n independent pixels
void ao_fold_states(uint32_t n, const uint32_t* states, uint32_t* counts) {
  for (uint32_t i = 0; i < n; i++) {
    const uint2 c = ao_fold(uint2{counts[2 * i], counts[2 * i + 1]}, states[i]);
    counts[2 * i] = c.x; counts[2 * i + 1] = c.y;
  }
}

// One sample of every pixel, row-major: what pt_debug_ao returns.  cam / proj: null for the emu's own perspective camera.
void ao_debug(void* h, const pt_camera* cam, const pt_camera_projection* proj, uint32_t sample, float distance, float* origins, float* directions,
              uint32_t* state) {
  const Emu* e = (const Emu*)h;
  const MaybeProjection mp(e, cam, proj);
  TravScratch scratch;
  for (uint32_t y = 0; y < e->S.height; y++)
    for (uint32_t x = 0; x < e->S.width; x++) {
      const size_t i = (size_t)y * e->S.width + x;
      AoRay a{v3(0.0f), v3(0.0f), 0.0f};
      state[i] = ao_one(e, mp.get(), x, y, sample, distance, scratch, &a);
      origins[3 * i] = a.o.x; origins[3 * i + 1] = a.o.y; origins[3 * i + 2] = a.o.z;
      directions[3 * i] = a.d.x; directions[3 * i + 1] = a.d.y; directions[3 * i + 2] = a.d.z;
    }
}

// Samples [first, first + ns) of every pixel folded into counts[pixel] = {hits, open} with ao_fold (the caller zeroes them before the first call)
void ao_counts(void* h, const pt_camera* cam, const pt_camera_projection* proj, uint32_t first, uint32_t ns, float distance, uint32_t* counts) {
  const Emu* e = (const Emu*)h;
  const MaybeProjection mp(e, cam, proj);
  TravScratch scratch;
  for (uint32_t y = 0; y < e->S.height; y++)
    for (uint32_t x = 0; x < e->S.width; x++) {
      const size_t i = (size_t)y * e->S.width + x;
      uint2 c{counts[2 * i], counts[2 * i + 1]};
      for (uint32_t s = 0; s < ns; s++) c = ao_fold(c, ao_one(e, mp.get(), x, y, first + s, distance, scratch, nullptr));
      counts[2 * i] = c.x; counts[2 * i + 1] = c.y;
    }
}

// The camera rays of one sample as the queue holds them, row-major: origins / directions [pixel][3] and the path's Halton offset (att.w)
void ao_camera_rays(void* h, const pt_camera* cam, const pt_camera_projection* proj, uint32_t sample, float* origins, float* directions,
                    uint32_t* offset) {
  const Emu* e = (const Emu*)h;
  const MaybeProjection mp(e, cam, proj);
  for (uint32_t y = 0; y < e->S.height; y++)
    for (uint32_t x = 0; x < e->S.width; x++) {
      const RayGenOut rg = mp.get() ? stage_raygen_projected(e->S, *mp.get(), x, y, sample) : stage_raygen(e->S, x, y, sample);
      const size_t i = (size_t)y * e->S.width + x;
      origins[3 * i] = rg.o.x; origins[3 * i + 1] = rg.o.y; origins[3 * i + 2] = rg.o.z;
      directions[3 * i] = rg.d.x; directions[3 * i + 1] = rg.d.y; directions[3 * i + 2] = rg.d.z;
      offset[i] = rg.offset;
    }
}

}  // extern "C"
