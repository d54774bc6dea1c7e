// TEST PROGRAM (tests/): the camera projections through include/ptamd_renderer.hpp and the C ABI without a GPU — the defaults, the struct
// layout, the accessors' types, every refusal of the options, and the order of the entry points' checks (the options before the renderer).
// tests/test_projection_cpp.py compiles and runs it; it returns 0 when everything holds.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <type_traits>

#include "ptamd_renderer.hpp"
#include "ptamd_scene.h"

using ptamd::renderer_pt::Renderer;

static_assert(sizeof(pt_camera_projection) == 32 && offsetof(pt_camera_projection, kind) == 0 && offsetof(pt_camera_projection, ortho_height) == 4 &&
                  offsetof(pt_camera_projection, fov_x) == 8 && offsetof(pt_camera_projection, fov_y) == 12 &&
                  offsetof(pt_camera_projection, fisheye_fov) == 16 && offsetof(pt_camera_projection, _pad) == 20,
              "pt_camera_projection");
static_assert(PT_PROJ_PERSPECTIVE == 0 && PT_PROJ_ORTHOGRAPHIC == 1 && PT_PROJ_EQUIRECT == 2 && PT_PROJ_FISHEYE == 3, "the kinds");
static_assert(sizeof(pt_camera) == 96 && sizeof(pt_camera_data) == 80 && sizeof(pt_constants) == 176, "the camera structs keep their sizes");
static_assert(PT_ABI_VERSION == 5u, "an additive extension");
static_assert(PT_GLTF_ORTHOGRAPHIC_CAMERAS == 4 && PT_GLTF_SKIP_EMPTY_NODES == 1 && PT_GLTF_CREATE_SCENE_NODES == 2, "the glTF option bits");
static_assert(std::is_same<decltype(std::declval<Renderer&>().projection()), pt_camera_projection&>::value, "projection() hands out the struct itself");
static_assert(std::is_same<decltype(std::declval<const Renderer&>().renderProjection()), pt_camera_projection>::value, "renderProjection() returns a copy");

static int refused(const pt_camera_projection& p) { return pt_set_camera_projection(nullptr, &p) == PT_ERR_INVALID_ARGUMENT &&
                                                           std::string(pt_last_error()).find("null renderer") == std::string::npos; }
static int accepted(const pt_camera_projection& p) { return pt_set_camera_projection(nullptr, &p) == PT_ERR_INVALID_ARGUMENT &&
                                                            std::string(pt_last_error()).find("null renderer") != std::string::npos; }

int main() {
  const float two_pi = 2.0f * 3.14159265358979323846f, pi = 3.14159265358979323846f;
  pt_camera_projection d;
  d.kind = 7u; d.ortho_height = d.fov_x = d.fov_y = d.fisheye_fov = 7.0f; d._pad[0] = d._pad[1] = d._pad[2] = 7u;
  pt_default_camera_projection(&d);
  if (d.kind != PT_PROJ_PERSPECTIVE || d.ortho_height != 1.0f || d.fov_x != two_pi || d.fov_y != pi || d.fisheye_fov != pi) return 2;
  if (d._pad[0] || d._pad[1] || d._pad[2]) return 3;
  pt_default_camera_projection(nullptr);
  Renderer* r = nullptr;
  if (r) {   // (compiled, not run: no GPU here)
    pt_camera_projection& p = r->projection();
    p.kind = PT_PROJ_FISHEYE;
    p.fisheye_fov = two_pi;
    r->setProjection(p);
    if (r->renderProjection().kind != PT_PROJ_FISHEYE) return 4;
  }
  if (!accepted(d)) return 5;                                   // valid options, no renderer: the options are looked at first
  if (pt_set_camera_projection(nullptr, nullptr) != PT_ERR_INVALID_ARGUMENT) return 6;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float bad[] = {0.0f, -1.0f, nan, inf, -inf};
  pt_camera_projection p = d;
  p.kind = 4u; if (!refused(p)) return 7;
  p.kind = 0xffffffffu; if (!refused(p)) return 7;
  for (float b : bad) {
    p = d; p.kind = PT_PROJ_ORTHOGRAPHIC; p.ortho_height = b; if (!refused(p)) return 8;
    p = d; p.kind = PT_PROJ_EQUIRECT; p.fov_x = b; if (!refused(p)) return 9;
    p = d; p.kind = PT_PROJ_EQUIRECT; p.fov_y = b; if (!refused(p)) return 10;
    p = d; p.kind = PT_PROJ_FISHEYE; p.fisheye_fov = b; if (!refused(p)) return 11;
    // the fields of the other kinds are not looked at
    p = d; p.ortho_height = p.fov_x = p.fov_y = p.fisheye_fov = b; if (!accepted(p)) return 12;
    p = d; p.kind = PT_PROJ_ORTHOGRAPHIC; p.fov_x = p.fov_y = p.fisheye_fov = b; if (!accepted(p)) return 13;
    p = d; p.kind = PT_PROJ_EQUIRECT; p.ortho_height = p.fisheye_fov = b; if (!accepted(p)) return 14;
    p = d; p.kind = PT_PROJ_FISHEYE; p.ortho_height = p.fov_x = p.fov_y = b; if (!accepted(p)) return 15;
  }
  // closed above at the fp32 values of 2 pi and pi
  p = d; p.kind = PT_PROJ_EQUIRECT; if (!accepted(p)) return 16;
  p.fov_x = std::nextafter(two_pi, inf); if (!refused(p)) return 17;
  p = d; p.kind = PT_PROJ_EQUIRECT; p.fov_y = std::nextafter(pi, inf); if (!refused(p)) return 18;
  p = d; p.kind = PT_PROJ_FISHEYE; p.fisheye_fov = two_pi; if (!accepted(p)) return 19;
  p.fisheye_fov = std::nextafter(two_pi, inf); if (!refused(p)) return 20;
  float rays[3];
  if (pt_get_camera_projection(nullptr, &p) != PT_ERR_INVALID_ARGUMENT) return 21;
  if (pt_debug_camera_rays(nullptr, 0u, rays, rays) != PT_ERR_INVALID_ARGUMENT) return 22;
  if (pt_scene_get_camera_projection(nullptr, 0u, &p) != PT_ERR_INVALID_ARGUMENT) return 23;
  return 0;
}
