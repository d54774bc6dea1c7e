// TEST PROGRAM (tests/): a stand-alone walk of pt_projection.h — projection_error, derive_projection and stage_raygen_projected — over the
// option edges of the formula test, built by tests/test_projection_sanitize.py with -fsanitize=address,undefined and run on the host.  It
// links nothing of the product: the header is plain C++.  Returns 0 when every ray is finite and of unit length and the sanitizers stay silent.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../platinum_amd/csrc/pt_projection.h"

using namespace pt;

int main() {
  std::vector<HaltonEntry> halton;
  for (uint32_t c = 2; (int)halton.size() < kHaltonDims; c++) {
    bool prime = true;
    for (uint32_t d = 2; d * d <= c; d++) if (c % d == 0) { prime = false; break; }
    if (prime) halton.push_back(make_halton_entry(c));
  }
  DeviceScene S{};
  S.halton = halton.data();
  const float two_pi = 2.0f * kPi, tiny = 1e-3f;
  // a rotated camera and one whose matrix also scales its axes
  const float cams[2][4][4] = {
      {{0.4536f, 0.0f, 0.8912f, 0.0f}, {-0.3470f, 0.9211f, 0.1766f, 0.0f}, {-0.8209f, -0.3894f, 0.4178f, 0.0f}, {1.25f, -0.5f, 3.0f, 1.0f}},
      {{1.1340f, 0.0f, 2.2280f, 0.0f}, {-0.1041f, 0.2763f, 0.0530f, 0.0f}, {-5.7463f, -2.7258f, 2.9246f, 0.0f}, {1.25f, -0.5f, 3.0f, 1.0f}}};
  std::vector<pt_camera_projection> projs;
  pt_camera_projection d{};
  d.kind = PT_PROJ_PERSPECTIVE; d.ortho_height = 1.0f; d.fov_x = two_pi; d.fov_y = kPi; d.fisheye_fov = kPi;
  { pt_camera_projection p = d; p.kind = PT_PROJ_ORTHOGRAPHIC; p.ortho_height = 2.5f; projs.push_back(p); }
  for (float fx : {tiny, kPi, two_pi}) for (float fy : {tiny, kPi}) { pt_camera_projection p = d; p.kind = PT_PROJ_EQUIRECT; p.fov_x = fx; p.fov_y = fy; projs.push_back(p); }
  for (float f : {tiny, kPi, two_pi}) { pt_camera_projection p = d; p.kind = PT_PROJ_FISHEYE; p.fisheye_fov = f; projs.push_back(p); }
  const uint32_t sizes[3][2] = {{1, 1}, {5, 3}, {50, 35}};
  const uint32_t samples[3] = {0, 1, 977};
  unsigned long rays = 0;
  for (const auto& cw : cams) {
    pt_camera cam{};
    for (int c = 0; c < 4; c++) for (int r = 0; r < 4; r++) cam.world[c][r] = cw[c][r];
    cam.sensor_size[0] = 36.0f; cam.sensor_size[1] = 24.0f; cam.focal_length = 28.0f; cam.focus_distance = 1.0f; cam.aperture = 2.8f;
    for (const pt_camera_projection& p : projs) {
      if (projection_error(p)) { std::fprintf(stderr, "refused: %s\n", projection_error(p)); return 2; }
      for (const auto& sz : sizes) {
        S.width = sz[0]; S.height = sz[1];
        const ProjectionConstants P = derive_projection(cam, sz[0], sz[1], p);
        for (uint32_t s : samples)
          for (uint32_t y = 0; y < sz[1]; y++)
            for (uint32_t x = 0; x < sz[0]; x++) {
              const RayGenOut rg = stage_raygen_projected(S, P, x, y, s);
              const float len = sqrtf(dot(rg.d, rg.d));
              if (!(std::isfinite(rg.o.x) && std::isfinite(rg.o.y) && std::isfinite(rg.o.z)) || !(fabsf(len - 1.0f) <= 1e-6f) || rg.dim != 4u) {
                std::fprintf(stderr, "kind %u %ux%u sample %u pixel %u,%u: |d| = %.9g dim %u\n", p.kind, sz[0], sz[1], s, x, y, len, rg.dim);
                return 3;
              }
              rays++;
            }
      }
    }
  }
  // what the validation refuses must be refused without reading anything else
  pt_camera_projection bad = d;
  bad.kind = 99u;
  if (!projection_error(bad)) return 4;
  bad = d; bad.kind = PT_PROJ_FISHEYE; bad.fisheye_fov = NAN;
  if (!projection_error(bad)) return 4;
  std::printf("%lu rays\n", rays);
  return 0;
}
