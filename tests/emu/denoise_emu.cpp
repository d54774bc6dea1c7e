// TEST HARNESS ONLY (tests/emu) — the host build of the denoiser's arithmetic and of the first-hit AOV stage
// (platinum_amd/csrc/pt_denoise.h), for tests/test_denoise_host.py and tests/test_gpu_denoise.py.  It reuses the host scene (Emu) and
// the per-path function (emu_path) of wavefront_emu.cpp.  Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// Second part of tests/emu/host_harness.cpp, which includes wavefront_emu.cpp before it; not compiled alone.
#ifndef PTAMD_TESTS_EMU_DENOISE_EMU
#define PTAMD_TESTS_EMU_DENOISE_EMU
#include "../../platinum_amd/csrc/pt_denoise.h"

extern "C" {

// The filter as denoise.hip runs it (launch_denoise): prep, `iterations` a-trous steps, remodulation fused into the last one.
// Every image is W*H*4 floats, row-major.  N = samples folded into the AOVs.
void dn_host_filter(const float* acc, const float* albedo, const float* normal, const float* moments, uint32_t W, uint32_t H, uint32_t N,
                    uint32_t iterations, float sigma_l, float sigma_n, float sigma_z, float* out) {
  const size_t npix = (size_t)W * H;
  const vec4* a = (const vec4*)acc;
  vec4* o = (vec4*)out;
  if (iterations == 0) {
    for (size_t p = 0; p < npix; p++) o[p] = vec4{a[p].x, a[p].y, a[p].z, 1.0f};
    return;
  }
  std::vector<vec4> guide(npix), aux(npix), col0(npix), col1(npix);
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++)
      dn_prep_pixel(a, (const vec4*)albedo, (const vec4*)normal, (const vec4*)moments, W, H, x, y, (float)N, guide.data(), col0.data(), aux.data());
  DenoiseParams P;
  P.W = W; P.H = H; P.sigma_l = sigma_l; P.sigma_n = sigma_n; P.sigma_z = sigma_z;
  vec4* cin = col0.data();
  vec4* cout = col1.data();
  for (uint32_t i = 0; i < iterations; i++) {
    for (uint32_t y = 0; y < H; y++)
      for (uint32_t x = 0; x < W; x++) dn_iterate_pixel(guide.data(), aux.data(), cin, cout, a, o, P, x, y, 1u << i, i + 1 == iterations);
    std::swap(cin, cout);
  }
}

// stage_aov on given camera-ray hits (e.g. the device's pt_trace_primary records of sample `sample`): albedo_out / normal_out get
// {albedo, t} / {normal, hit} per pixel, as k_aov writes them for a one-sample batch.  The ray is this host's stage_raygen.
void dn_host_stage_aov(void* h, uint32_t sample, const pt_hit_record* hits, float* albedo_out, float* normal_out) {
  Emu* e = (Emu*)h;
  const uint32_t W = e->S.width, H = e->S.height;
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++) {
      const size_t p = (size_t)y * W + x;
      const pt_hit_record& r = hits[p];
      AovSample a = aov_miss();
      float hf = 0.0f;
      if (r.instance >= 0) {
        // the hit's shading record, built for this (instance, primitive) as k_shade_records does for a leaf slot
        DeviceScene S = e->S;
        const ShadeRec rec = make_shade_rec(S, (uint32_t)r.instance, (uint32_t)r.primitive);
        S.shade_recs = &rec;
        const RayGenOut rg = stage_raygen(S, x, y, sample);
        const vec4 qO{rg.o.x, rg.o.y, rg.o.z, 0.0f}, qD{rg.d.x, rg.d.y, rg.d.z, 0.0f};
        ShadeIn in;
        in.o = rg.o; in.d = rg.d; in.att = v3(1.0f); in.rayO = &qO; in.rayD = &qD; in.lastSpecular = false;
        in.offset = 0; in.dim = 0; in.bounce = 0;
        in.t = r.t; in.u = r.u; in.v = r.v; in.tri = 0;
        a = stage_aov(S, in);
        hf = 1.0f;
      }
      float* ao = albedo_out + 4 * p;
      float* no = normal_out + 4 * p;
      ao[0] = a.albedo.x; ao[1] = a.albedo.y; ao[2] = a.albedo.z; ao[3] = a.t;
      no[0] = a.normal.x; no[1] = a.normal.y; no[2] = a.normal.z; no[3] = hf;
    }
}

// lum and lum^2 of n RGBA radiance values (pt_denoise.h dn_lum, the function k_accumulate_aov uses)
void dn_host_lum(const float* rgba, size_t n, float* lum, float* lum2) {
  for (size_t i = 0; i < n; i++) {
    const float l = dn_lum(v3(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2]));
    lum[i] = l;
    lum2[i] = l * l;
  }
}

// Samples [first, first + ns) of every pixel: the accumulator and the three AOV images, folded as k_accumulate / k_accumulate_aov do
// (n0 samples already in them).  A sample that is not finite (the kernels' own test) is counted, and under PT_NONFINITE_ZERO (the policy of
// the render params the scene was created with) replaced by black before the accumulator's fold (kernels.hip accumulate_body) and before
// dn_lum (denoise.hip accumulate_aov_body).  Returns the number of such samples; `nonfinite_px` (W*H, may be null) is incremented at their
// pixels.  Single-threaded; for small images.
uint64_t dn_host_render(void* h, uint32_t first, uint32_t ns, uint32_t n0, float* acc, float* albedo, float* normal, float* moments,
                        uint32_t* nonfinite_px) {
  Emu* e = (Emu*)h;
  const DeviceScene& S = e->S;
  const uint32_t W = S.width, H = S.height;
  std::vector<pt_hit_record> hits((size_t)W * H);
  std::vector<float> ab((size_t)W * H * 4), nb((size_t)W * H * 4);
  TravScratch scratch;
  const bool zero = e->params.nonfinite_policy == PT_NONFINITE_ZERO;
  uint64_t nonfinite = 0;
  for (uint32_t s = 0; s < ns; s++) {
    emu_trace_primary(h, first + s, hits.data());
    dn_host_stage_aov(h, first + s, hits.data(), ab.data(), nb.data());
    const uint32_t n = n0 + s;
    for (uint32_t y = 0; y < H; y++)
      for (uint32_t x = 0; x < W; x++) {
        const size_t p = (size_t)y * W + x;
        vec3 L = emu_path<false>(e, x, y, first + s, scratch);
        if (not_finite(L)) {
          nonfinite++;
          if (nonfinite_px) nonfinite_px[p]++;
          if (zero) L = v3(0.0f);
        }
        float* c = acc + 4 * p;
        const vec3 cm = aov_fold(v3(c[0], c[1], c[2]), L, n);
        c[0] = cm.x; c[1] = cm.y; c[2] = cm.z; c[3] = 1.0f;
        const float l = dn_lum(L);
        float* A = albedo + 4 * p;
        float* Nn = normal + 4 * p;
        float* M = moments + 4 * p;
        const vec3 a = aov_fold(v3(A[0], A[1], A[2]), v3(ab[4 * p], ab[4 * p + 1], ab[4 * p + 2]), n);
        const vec3 nn = aov_fold(v3(Nn[0], Nn[1], Nn[2]), v3(nb[4 * p], nb[4 * p + 1], nb[4 * p + 2]), n);
        const vec3 m = aov_fold(v3(M[0], M[1], M[2]), v3(ab[4 * p + 3], l, l * l), n);
        A[0] = a.x; A[1] = a.y; A[2] = a.z; A[3] = 1.0f;
        Nn[0] = nn.x; Nn[1] = nn.y; Nn[2] = nn.z; Nn[3] = aov_fold(Nn[3], nb[4 * p + 3], n);
        M[0] = m.x; M[1] = m.y; M[2] = m.z; M[3] = 0.0f;
      }
  }
  return nonfinite;
}

// sizeof / offsetof of pt_denoise_options as this compiler lays it out, and the library's defaults as the header states them
void dn_host_options_layout(uint32_t out[7]) {
  out[0] = sizeof(pt_denoise_options);
  out[1] = offsetof(pt_denoise_options, enabled);
  out[2] = offsetof(pt_denoise_options, iterations);
  out[3] = offsetof(pt_denoise_options, sigma_luminance);
  out[4] = offsetof(pt_denoise_options, sigma_normal);
  out[5] = offsetof(pt_denoise_options, sigma_depth);
  out[6] = offsetof(pt_denoise_options, apply_to_target);
}

}  // extern "C"

#endif  // PTAMD_TESTS_EMU_DENOISE_EMU
