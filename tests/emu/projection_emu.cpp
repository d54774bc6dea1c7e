// TEST HARNESS ONLY (tests/emu) — the host build of the camera projections (platinum_amd/csrc/pt_projection.h: projection_error,
// derive_projection, stage_raygen_projected) on top of the host harness's scene and traversal, for tests/projection_lib.py.  A library of its
// own (tests/host_build.py load(src, lib)): host_harness.cpp stays as it is.  Not part of libptamd.so, never loaded by platinum_amd, not a
// fallback.
#include "wavefront_emu.cpp"  // emu_*: host scene + BVH (Emu), traverse<>
#include "../../platinum_amd/csrc/pt_projection.h"

extern "C" {

// 0 = the options are accepted, 1 = refused (pt_set_camera_projection's test)
int pj_refused(const pt_camera_projection* p) { return projection_error(*p) != nullptr; }

// the derived constants as floats: {topLeft, dU, dV, dir, pos, u, v, w} x 3
void pj_constants(const pt_camera* cam, uint32_t W, uint32_t H, const pt_camera_projection* p, float* out /*24*/) {
  const ProjectionConstants P = derive_projection(*cam, W, H, *p);
  const float* src[8] = {P.topLeft, P.dU, P.dV, P.dir, P.pos, P.u, P.v, P.w};
  for (int k = 0; k < 8; k++) for (int c = 0; c < 3; c++) out[3 * k + c] = src[k][c];
}

// The camera rays of one sample, row-major: origins / directions [pixel][3], offset / dim [pixel] as ray generation leaves them.
// PERSPECTIVE: stage_raygen on the emu's own camera constants; else stage_raygen_projected on `cam`.
void pj_rays(void* h, const pt_camera* cam, const pt_camera_projection* p, uint32_t sample, float* origins, float* directions, uint32_t* offset,
             uint32_t* dim) {
  const Emu* e = (const Emu*)h;
  const DeviceScene& S = e->S;
  const ProjectionConstants P = derive_projection(*cam, S.width, S.height, *p);
  for (uint32_t y = 0; y < S.height; y++)
    for (uint32_t x = 0; x < S.width; x++) {
      const RayGenOut rg = p->kind == PT_PROJ_PERSPECTIVE ? stage_raygen(S, x, y, sample) : stage_raygen_projected(S, P, x, y, sample);
      const size_t i = (size_t)y * S.width + x;
      origins[3 * i] = rg.o.x; origins[3 * i + 1] = rg.o.y; origins[3 * i + 2] = rg.o.z;
      directions[3 * i] = rg.d.x; directions[3 * i + 1] = rg.d.y; directions[3 * i + 2] = rg.d.z;
      offset[i] = rg.offset; dim[i] = rg.dim;
    }
}

// emu_trace_primary under a projection
void pj_trace_primary(void* h, const pt_camera* cam, const pt_camera_projection* p, uint32_t sample, pt_hit_record* out) {
  Emu* e = (Emu*)h;
  const DeviceScene& S = e->S;
  const ProjectionConstants P = derive_projection(*cam, S.width, S.height, *p);
  TravScratch scratch;
  for (uint32_t y = 0; y < S.height; y++)
    for (uint32_t x = 0; x < S.width; x++) {
      const RayGenOut rg = p->kind == PT_PROJ_PERSPECTIVE ? stage_raygen(S, x, y, sample) : stage_raygen_projected(S, P, x, y, sample);
      TraversalStack st = scratch.stack();
      TraversalCount tc;
      const float ir = S.has_alpha ? Halton{halton_table(S.halton), rg.offset, rg.dim}.sample1d() : 0.0f;
      const RayHit hit = traverse<false, false>(S, rg.o, rg.d, 1e-3f, kInf, ir, st, &tc);
      pt_hit_record& r = out[y * S.width + x];
      if (hit.tri != kInvalidRef) { r.t = hit.t; r.u = hit.u; r.v = hit.v; triangle_ids(S, hit.tri, &r.instance, &r.primitive); }
      else { r.t = r.u = r.v = 0; r.instance = r.primitive = -1; }
    }
}

// the product's rayDirToUv (pt_shade.h) on n directions
void pj_ray_dir_to_uv(uint32_t n, const float* d, float* uv) {
  for (uint32_t i = 0; i < n; i++) {
    const vec2 r = rayDirToUv(v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]));
    uv[2 * i] = r.x; uv[2 * i + 1] = r.y;
  }
}

// the radiance of camera rays that leave the scene at bounce 0: stage_miss (pt_shade.h) with the throughput a camera ray carries
void pj_miss_radiance(void* h, uint32_t n, const float* d, float* rgb) {
  const DeviceScene& S = ((const Emu*)h)->S;
  for (uint32_t i = 0; i < n; i++) {
    const vec3 L = stage_miss(S, v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), v3(1.0f), 0u, 0.0f, false);
    rgb[3 * i] = L.x; rgb[3 * i + 1] = L.y; rgb[3 * i + 2] = L.z;
  }
}

}  // extern "C"
