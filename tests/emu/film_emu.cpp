// TEST HARNESS ONLY (tests/emu) — the host build of the transparent film (platinum_amd/csrc/pt_film.h): the per-sample fold, the two compose
// modes, the alpha byte and the queue budget with the flag buffer; for tests/test_film_host.py and tests/test_gpu_film.py.
// Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// A translation unit of its own: tests/film_lib.py builds it into tests/_build/libptamd_film.so (tests/host_build.py load).
// With -DFILM_EMU_MAIN it is a stand-alone program that drives the fold and the compose over edge values (a sanitizer build runs it).
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../platinum_amd/csrc/host_scene.h"
#include "../../platinum_amd/csrc/pt_film.h"

using namespace pt;

extern "C" {

// film[p] (the mean of n0 samples) folded with samples 0 .. ns - 1 of pixel p, in order: L is [npix][ns][4], flags [npix][ns]
void film_host_fold(float* film, const float* L, const uint32_t* flags, uint32_t npix, uint32_t ns, uint32_t n0, uint32_t nonfinite_policy) {
  for (uint32_t p = 0; p < npix; p++) {
    vec4 f{film[4 * p], film[4 * p + 1], film[4 * p + 2], film[4 * p + 3]};
    for (uint32_t s = 0; s < ns; s++) {
      const float* l = L + ((size_t)p * ns + s) * 4;
      f = film_fold(f, film_sample(vec4{l[0], l[1], l[2], l[3]}, flags[(size_t)p * ns + s], nonfinite_policy), n0 + s);
    }
    film[4 * p] = f.x; film[4 * p + 1] = f.y; film[4 * p + 2] = f.z; film[4 * p + 3] = f.w;
  }
}

// k_film_compose over a W x H frame: base and film are [H][W][4]; rect = {x0, y0, x1, y1}; 0 outside it
void film_host_compose(const float* base, const float* film, uint32_t W, uint32_t H, const uint32_t* rect, const pt_film_options* o, float* out) {
  const Rect rc{rect[0], rect[1], rect[2], rect[3]};
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++) {
      const size_t p = (size_t)y * W + x;
      vec4 c{0.0f, 0.0f, 0.0f, 0.0f};
      if (rect_contains(rc, x, y)) c = film_compose(vec4{base[4 * p], base[4 * p + 1], base[4 * p + 2], base[4 * p + 3]}, film[4 * p + 3], o->backdrop, o->backdrop_rgb);
      out[4 * p] = c.x; out[4 * p + 1] = c.y; out[4 * p + 2] = c.z; out[4 * p + 3] = c.w;
    }
}

// k_film_alpha: the target's alpha bytes from the composed source's .w
void film_host_alpha(const uint32_t* rgba8, const float* composed, uint32_t npix, uint32_t* out) {
  for (uint32_t p = 0; p < npix; p++) out[p] = film_alpha_byte(rgba8[p], composed[4 * (size_t)p + 3]);
}

// 1 when pt_set_film_options would accept the options
uint32_t film_host_options_valid(const pt_film_options* o) { return film_options_error(*o) == nullptr; }

// what pt_start_render lets the queue plan count on (host_scene.h)
uint64_t film_host_queue_budget(uint64_t free_bytes, uint64_t queues_held, uint64_t lists_held, int aov, uint64_t abuf_held, int matte,
                                uint64_t mbuf_held, int film, uint64_t fbuf_held) {
  return queue_budget(free_bytes, queues_held, lists_held, aov != 0, abuf_held, matte != 0, mbuf_held, film != 0, fbuf_held);
}

// sizeof / offsetof of the struct as this compiler lays it out
void film_host_layout(uint32_t out[4]) {
  out[0] = sizeof(pt_film_options);
  out[1] = offsetof(pt_film_options, enabled); out[2] = offsetof(pt_film_options, backdrop); out[3] = offsetof(pt_film_options, backdrop_rgb);
}

}  // extern "C"

#ifdef FILM_EMU_MAIN
int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity(), den = std::numeric_limits<float>::denorm_min();
  // the fold: every batch split of 16 samples gives the same bits, for each policy, with non-finite samples on hits and on misses
  const uint32_t npix = 5, ns = 16;
  std::vector<float> L((size_t)npix * ns * 4);
  std::vector<uint32_t> F((size_t)npix * ns);
  uint32_t s = 2463534242u;
  auto next = [&]() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; };
  for (uint32_t p = 0; p < npix; p++)
    for (uint32_t k = 0; k < ns; k++) {
      float* l = &L[((size_t)p * ns + k) * 4];
      for (int c = 0; c < 3; c++) l[c] = (float)(next() >> 8) * (4.0f / 16777216.0f);
      l[3] = 1.0f;
      F[(size_t)p * ns + k] = p == 0 ? 1u : p == 1 ? 0u : next() & 1u;
    }
  L[(3 * ns + 2) * 4 + 1] = nan; F[3 * ns + 2] = 1u;
  L[(3 * ns + 5) * 4 + 0] = inf; F[3 * ns + 5] = 0u;
  L[(4 * ns + 7) * 4 + 2] = -inf; F[4 * ns + 7] = 1u;
  L[(4 * ns + 9) * 4 + 2] = nan; F[4 * ns + 9] = 0u;
  for (uint32_t policy = 0; policy < 2; policy++) {
    std::vector<float> whole((size_t)npix * 4, 0.0f);
    film_host_fold(whole.data(), L.data(), F.data(), npix, ns, 0, policy);
    const uint32_t splits[][4] = {{16, 0, 0, 0}, {7, 7, 2, 0}, {1, 8, 7, 0}, {5, 5, 5, 1}};
    for (const auto& sp : splits) {
      std::vector<float> part((size_t)npix * 4, 0.0f);
      uint32_t n0 = 0;
      for (uint32_t b = 0; b < 4 && sp[b]; b++) {
        std::vector<float> Lb((size_t)npix * sp[b] * 4);
        std::vector<uint32_t> Fb((size_t)npix * sp[b]);
        for (uint32_t p = 0; p < npix; p++)
          for (uint32_t k = 0; k < sp[b]; k++) {
            std::memcpy(&Lb[((size_t)p * sp[b] + k) * 4], &L[((size_t)p * ns + n0 + k) * 4], 16);
            Fb[(size_t)p * sp[b] + k] = F[(size_t)p * ns + n0 + k];
          }
        film_host_fold(part.data(), Lb.data(), Fb.data(), npix, sp[b], n0, policy);
        n0 += sp[b];
      }
      if (n0 != ns || std::memcmp(whole.data(), part.data(), whole.size() * 4)) return 2;
    }
    if (whole[3] != 1.0f || whole[4] != 0.0f || whole[5] != 0.0f || whole[6] != 0.0f || whole[7] != 0.0f) return 3;   // all hit, all miss
    if (policy == 1 && !(std::isfinite(whole[12]) && std::isfinite(whole[13]) && std::isfinite(whole[18]))) return 4;   // ZERO: nothing non-finite survives
    if (policy == 0 && !(std::isnan(whole[13]) && std::isfinite(whole[12]))) return 5;                                  // KEEP: the hit's NaN does, the miss's infinity does not
    printf("policy %u: film of pixel 2 = %g %g %g %g\n", policy, whole[8], whole[9], whole[10], whole[11]);
  }
  // the compose over alphas and backdrops, inside and outside a rectangle
  const float alphas[] = {0.0f, 1.0f, 1.0f / 3.0f, den, nan, 0.5f};
  const uint32_t W = 6, H = 2, rect[4] = {1, 0, 6, 2};
  std::vector<float> base((size_t)W * H * 4), film((size_t)W * H * 4), out((size_t)W * H * 4);
  for (uint32_t p = 0; p < W * H; p++) {
    const float a = alphas[p % 6];
    for (int c = 0; c < 3; c++) base[4 * p + c] = film[4 * p + c] = a * (0.25f + (float)c);
    base[4 * p + 3] = 1.0f; film[4 * p + 3] = a;
  }
  std::vector<uint32_t> target((size_t)W * H, 0xff102030u), withAlpha((size_t)W * H);
  const float backs[][3] = {{0.0f, 0.0f, 0.0f}, {1.0e30f, 2.0f, 0.5f}};
  for (uint32_t mode = PT_BACKDROP_COLOR; mode <= PT_BACKDROP_TRANSPARENT; mode++)
    for (const auto& b : backs) {
      pt_film_options o{1u, mode, {b[0], b[1], b[2]}};
      if (film_options_error(o)) return 6;
      film_host_compose(base.data(), film.data(), W, H, rect, &o, out.data());
      film_host_alpha(target.data(), out.data(), W * H, withAlpha.data());
      if (out[0] != 0.0f || out[3] != 0.0f || (withAlpha[0] >> 24) != 0u) return 7;                    // outside the rectangle
      if ((withAlpha[1] >> 24) != 255u) return 8;                                                       // alpha 1, in either mode
      if (mode == PT_BACKDROP_TRANSPARENT && ((withAlpha[2] >> 24) != 85u || (withAlpha[3] >> 24) != 0u || (withAlpha[4] >> 24) != 0u)) return 9;
      for (uint32_t p = 0; p < W * H; p++)
        if ((withAlpha[p] & 0x00ffffffu) != 0x00102030u) return 10;
      printf("backdrop %u (%g %g %g): alpha 1/3 -> %g %g %g %g\n", mode, b[0], b[1], b[2], out[8], out[9], out[10], out[11]);
    }
  pt_film_options bad{0u, 3u, {0.0f, 0.0f, 0.0f}};
  if (!film_options_error(bad)) return 11;
  bad.backdrop = 0u; bad.backdrop_rgb[1] = nan;
  if (!film_options_error(bad)) return 11;
  return 0;
}
#endif
