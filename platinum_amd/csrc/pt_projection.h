// pt_projection.h — the camera projections beside the reference's perspective camera (include/ptamd.h pt_camera_projection):
// orthographic, equirectangular (panoramic) and equidistant fisheye.  No reference counterpart.
//
//   projection_error          : pt_set_camera_projection's test
//   derive_projection         : pt_camera + image size + options -> the fp32 constants a render's ray generation reads (host, once per start)
//   stage_raygen_projected    : HaltonSampler ctor + one camera ray, the counterpart of pt_shade.h stage_raygen
// stage_raygen and DeviceScene are left as they are: the constants below reach k_raygen_projected (projection.hip) as a kernel argument of
// their own.  Plain C++ under PT_HD with pt_math.h's deterministic functions only, so that tests/emu builds the same arithmetic for the
// host and the device agrees with it bit for bit; every expression is the operation sequence it spells (-ffp-contract=off).
#pragma once
#include "pt_device.h"
#include "pt_sampler.h"
#include "pt_shade.h"

namespace pt {

constexpr float kHalfPi = 1.5707963267948966f;

// The derived fp32 constants of one render's projection.  Plain floats (no vec3 members): the struct is a kernel argument.
struct ProjectionConstants {
  uint32_t kind;       // PT_PROJ_*
  float W, H;          // (float)width, (float)height
  float pos[3];        // column 3 of pt_camera.world
  float u[3], v[3], w[3];   // columns 0..2, each divided by its length (host_scene.h build_host_scene: the same three divisions)
  // ORTHOGRAPHIC
  float topLeft[3], dU[3], dV[3], dir[3];
  // EQUIRECT
  float fov_x, fov_y;
  // FISHEYE
  float half;          // min(W, H) * 0.5f
  float half_fov;      // fisheye_fov * 0.5f
};

PT_HD const char* projection_error(const pt_camera_projection& p) {
  auto inside = [](float x, float hi) { return x == x && x > 0.0f && x <= hi; };   // (a NaN fails x == x, +inf fails x <= hi)
  switch (p.kind) {
    case PT_PROJ_PERSPECTIVE: return nullptr;
    case PT_PROJ_ORTHOGRAPHIC: return inside(p.ortho_height, 3.402823466e38f) ? nullptr : "ortho_height must be finite and > 0";
    case PT_PROJ_EQUIRECT:
      if (!inside(p.fov_x, 2.0f * kPi)) return "fov_x must lie in (0, 2 pi]";
      return inside(p.fov_y, kPi) ? nullptr : "fov_y must lie in (0, pi]";
    case PT_PROJ_FISHEYE: return inside(p.fisheye_fov, 2.0f * kPi) ? nullptr : "fisheye_fov must lie in (0, 2 pi]";
    default: return "unknown projection kind";
  }
}

PT_HD void st3(float* o, vec3 a) { o[0] = a.x; o[1] = a.y; o[2] = a.z; }
PT_HD vec3 ldf3(const float* a) { return v3(a[0], a[1], a[2]); }

// u, v, w, pos as build_host_scene derives them for the perspective camera; the orthographic frame in its operation order with
// vh = ortho_height in place of focus_distance * cropped / focal_length and no focus distance along w.
inline ProjectionConstants derive_projection(const pt_camera& cam, uint32_t width, uint32_t height, const pt_camera_projection& p) {
  ProjectionConstants P{};
  vec3 col[4];
  for (int i = 0; i < 4; i++) col[i] = v3(cam.world[i][0], cam.world[i][1], cam.world[i][2]);
  const vec3 u = col[0] / length(col[0]);
  const vec3 v = col[1] / length(col[1]);
  const vec3 w = col[2] / length(col[2]);
  const vec3 pos = col[3];
  const float sx = (float)width, sy = (float)height;
  P.kind = p.kind;
  P.W = sx; P.H = sy;
  st3(P.pos, pos); st3(P.u, u); st3(P.v, v); st3(P.w, w);
  {
    const float vh = p.kind == PT_PROJ_ORTHOGRAPHIC ? p.ortho_height : 1.0f;
    const float vw = vh * (sx / sy);
    const vec3 vu = u * vw;
    const vec3 vv = -v * vh;
    st3(P.topLeft, pos - (vu + vv) * 0.5f);
    st3(P.dU, vu / sx);
    st3(P.dV, vv / sy);
    st3(P.dir, normalize(-w));
  }
  P.fov_x = p.fov_x; P.fov_y = p.fov_y;
  P.half = (float)(width < height ? width : height) * 0.5f;
  P.half_fov = p.fisheye_fov * 0.5f;
  return P;
}

// One camera ray under KIND != PT_PROJ_PERSPECTIVE.  Every kind is a pinhole in the sampler's sense: dimensions 0-1 place the sample in
// the pixel, dimensions 2-3 are consumed and not evaluated, so offset / dim leave with the values stage_raygen gives a pinhole camera.
// KIND is a template argument so that a caller that has branched on P.kind once (k_raygen_projected: outside its loops) holds only the
// constants of that kind in registers.
template <uint32_t KIND>
PT_HD RayGenOut stage_raygen_kind(const DeviceScene& S, const ProjectionConstants& P, uint32_t px, uint32_t py, uint32_t sample) {
  Halton h{halton_table(S.halton), halton_offset(px, py, sample), 0};
  const vec2 pixelSample = h.sample2d();  // dims 0-1
  h.dim += 2;                             // dims 2-3: the lens sample no projection here has
  const float fx = (float)px + pixelSample.x;
  const float fy = (float)py + pixelSample.y;
  RayGenOut out;
  out.offset = h.offset;
  out.dim = h.dim;
  if (KIND == PT_PROJ_ORTHOGRAPHIC) {
    // o = (topLeft + fx * dU) + fy * dV;  d = dir
    out.o = (ldf3(P.topLeft) + fx * ldf3(P.dU)) + fy * ldf3(P.dV);
    out.d = ldf3(P.dir);
  } else if (KIND == PT_PROJ_EQUIRECT) {
    // phi = (fx / W - 0.5) * fov_x;  theta = pi/2 + (fy / H - 0.5) * fov_y
    // d = normalize(((sin(theta) * sin(phi)) * u + cos(theta) * v) - (sin(theta) * cos(phi)) * w)
    const float phi = (fx / P.W - 0.5f) * P.fov_x;
    const float theta = kHalfPi + (fy / P.H - 0.5f) * P.fov_y;
    float sp, cp, st, ct;
    sincos_det(phi, &sp, &cp);
    sincos_det(theta, &st, &ct);
    out.o = ldf3(P.pos);
    out.d = normalize(((st * sp) * ldf3(P.u) + ct * ldf3(P.v)) - (st * cp) * ldf3(P.w));
  } else {  // PT_PROJ_FISHEYE
    // x = (fx - W * 0.5) / half;  y = (H * 0.5 - fy) / half;  r = sqrt(x * x + y * y);  theta = min(r * half_fov, pi)
    // d = normalize(((sin(theta) * (x / r)) * u + (sin(theta) * (y / r)) * v) - cos(theta) * w);  r == 0: d = -w, by a select
    const float x = (fx - P.W * 0.5f) / P.half;
    const float y = (P.H * 0.5f - fy) / P.half;
    const float r = sqrtf(x * x + y * y);
    const float theta = fminf(r * P.half_fov, kPi);
    float s, c;
    sincos_det(theta, &s, &c);
    const float rs = r > 0.0f ? r : 1.0f;
    const vec3 d = normalize(((s * (x / rs)) * ldf3(P.u) + (s * (y / rs)) * ldf3(P.v)) - c * ldf3(P.w));
    out.o = ldf3(P.pos);
    out.d = r > 0.0f ? d : -ldf3(P.w);
  }
  return out;
}
// ... under P.kind (not PT_PROJ_PERSPECTIVE): the same three functions behind one switch
PT_HD RayGenOut stage_raygen_projected(const DeviceScene& S, const ProjectionConstants& P, uint32_t px, uint32_t py, uint32_t sample) {
  if (P.kind == PT_PROJ_ORTHOGRAPHIC) return stage_raygen_kind<PT_PROJ_ORTHOGRAPHIC>(S, P, px, py, sample);
  if (P.kind == PT_PROJ_EQUIRECT) return stage_raygen_kind<PT_PROJ_EQUIRECT>(S, P, px, py, sample);
  return stage_raygen_kind<PT_PROJ_FISHEYE>(S, P, px, py, sample);
}

// Camera-ray leaf lists are built from pinhole pixel cones: a render under any other projection walks the tree at bounce 0
// (beside host_scene.h camera_lists_wanted, whose signature tests/emu pins).
inline bool camera_lists_projection(uint32_t kind) { return kind == PT_PROJ_PERSPECTIVE; }

}  // namespace pt
