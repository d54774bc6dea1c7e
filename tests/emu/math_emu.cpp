// TEST HARNESS ONLY (tests/emu) — the host build of the math layer as pt_debug_math runs it (platinum_amd/csrc/pt_math_probe.h over pt_math.h,
// pt_sampler.h and the guards of pt_post.h / pt_denoise.h), for tests/test_math_host.py and tests/test_gpu_math.py.
// Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// With -DMATH_EMU_MAIN it is a stand-alone program that feeds in-domain sweeps through every function (a sanitizer build runs it:
// -fsanitize=address,undefined,float-cast-overflow proves that the stated domains keep the float -> int casts defined).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../platinum_amd/csrc/pt_math_probe.h"

namespace {
const std::vector<pt::HaltonEntry>& math_emu_table() {
  static const std::vector<pt::HaltonEntry> tab = [] {
    std::vector<pt::HaltonEntry> t;
    for (uint32_t c = 2; (int)t.size() < pt::kHaltonDims; c++) {
      bool prime = true;
      for (uint32_t d = 2; d * d <= c; d++) if (c % d == 0) { prime = false; break; }
      if (prime) t.push_back(pt::make_halton_entry(c));
    }
    return t;
  }();
  return tab;
}
}  // namespace

extern "C" {

// pt_debug_math's signature without the renderer; the same fn ids, arguments and results
void emu_math_batch(uint32_t fn, uint32_t n, const void* a_, const void* b_, void* out0_, void* out1_) {
  const uint32_t* a = (const uint32_t*)a_; const uint32_t* b = (const uint32_t*)b_;
  uint32_t* out0 = (uint32_t*)out0_; uint32_t* out1 = (uint32_t*)out1_;
  const pt::HaltonEntry* table = math_emu_table().data();
  const bool reads_b = pt::math_probe_reads_b(fn), writes_1 = pt::math_probe_writes_out1(fn);
  for (uint32_t i = 0; i < n; i++) {
    uint32_t o[3];
    pt::math_probe_eval(fn, a[i], reads_b ? b[i] : 0u, table, o);
    out0[i] = o[0];
    if (writes_1) out1[i] = o[1];
    if (fn == PT_MATH_SAMPLE_COSINE_HEMISPHERE) out1[n + i] = o[2];
  }
}

}  // extern "C"

#ifdef MATH_EMU_MAIN
// In-domain sweeps of every function: a strided walk over the float bit patterns inside each raw function's domain (both signs), every
// float for the guarded forms, the unit square for the warps, strided indices in every dimension for Halton.
int main() {
  using namespace pt;
  std::vector<uint32_t> a, b;
  auto run = [&](uint32_t fn) {
    std::vector<uint32_t> o0(a.size()), o1(2 * a.size());
    emu_math_batch(fn, (uint32_t)a.size(), a.data(), b.data(), o0.data(), o1.data());
    uint32_t h = 0;
    for (uint32_t v : o0) h = h * 31u + v;
    printf("fn %2u: %zu elements, out0 hash %08x\n", fn, a.size(), h);
    fflush(stdout);
  };
  auto floats_upto = [&](float lim, uint32_t step) {  // +-0 .. +-lim, denormals included
    a.clear();
    for (uint32_t u = 0; u <= f2u(lim); u += step) { a.push_back(u); a.push_back(u | 0x80000000u); }
    a.push_back(f2u(lim)); a.push_back(f2u(-lim));
    b.assign(a.size(), f2u(1.0f));
  };
  floats_upto(8192.0f, 997u); run(PT_MATH_SINCOS); run(PT_MATH_COS);
  floats_upto(3.0e38f, 1009u); b = a; for (size_t i = 0; i < b.size(); i++) b[i] = a[(i * 7919u + 13u) % a.size()];
  run(PT_MATH_ATAN2); run(PT_MATH_ACOS);
  a.clear(); for (uint32_t u = 0x00800000u; u < 0x7f800000u; u += 1013u) a.push_back(u);
  b.assign(a.size(), f2u(1.0f)); run(PT_MATH_LOG2);
  // exp2_det: [-126.5, 127.5)
  a.clear(); for (uint32_t u = 0; u < f2u(127.5f); u += 499u) a.push_back(u);
  for (uint32_t u = 0x80000000u; u <= f2u(-126.5f); u += 499u) a.push_back(u);
  a.push_back(f2u(-126.5f)); a.push_back(f2u(127.5f) - 1u);
  b.assign(a.size(), 0u); run(PT_MATH_EXP2);
  // powr_det over the thin lens' range: x in [2^-16, 1), y in [1/2, 2]
  a.clear(); b.clear();
  for (uint32_t u = f2u(1.52587890625e-05f), k = 0; u < f2u(1.0f); u += 4093u, k++) { a.push_back(u); b.push_back(f2u(0.5f + 1.5f * (float)(k % 1024u) / 1023.0f)); }
  run(PT_MATH_POWR);
  // the guarded forms: every class of float, NaN and the infinities included
  a.clear(); for (uint64_t u = 0; u < (1ull << 32); u += 65521u) a.push_back((uint32_t)u);
  a.push_back(0x7f800000u); a.push_back(0xff800000u); a.push_back(0x7fc00000u);
  b = a; for (size_t i = 0; i < b.size(); i++) b[i] = a[(i * 7919u + 13u) % a.size()];
  run(PT_MATH_PP_LOG2); run(PT_MATH_BOKEH_POWR);
  // dn_exp2 guards the lower side only (a filter weight's exponent is never positive): NaN and everything below 127.5
  { const std::vector<uint32_t> all = a; a.clear(); for (uint32_t u : all) if (!(u2f(u) >= 127.5f)) a.push_back(u); b = a; run(PT_MATH_DN_EXP2); a = all; b = all; }
  // pp_exp2 / pp_exp2s: every class but NaN, which passes both comparisons and reaches exp2_det's cast (outside their domain)
  { std::vector<uint32_t> nn; for (uint32_t u : a) if (u2f(u) == u2f(u)) nn.push_back(u); a = nn; b = nn; }
  run(PT_MATH_PP_EXP2S); run(PT_MATH_PP_EXP2);
  // the guarded powers: finite bases and exponents whose product is a number (a NaN product is outside pp_powr's and dn_powr's domain)
  a.clear(); b.clear();
  for (uint32_t u = 0, k = 0; u < 0x7f800000u; u += 65521u, k++) { a.push_back(u); b.push_back(f2u(-40.0f + 80.0f * (float)(k % 257u) / 256.0f)); }
  run(PT_MATH_PP_POWR);
  // dn_powr as the filter calls it: x in [0, 1] and a rounding above (1 + 2^-20), sigma_n up to kDnSigmaNormalMax
  a.clear(); b.clear();
  for (uint32_t u = 0, k = 0; u <= f2u(1.0f); u += 65521u, k++) { a.push_back(u); b.push_back(f2u(1024.0f * (float)(k % 257u) / 256.0f)); }
  for (uint32_t k = 0; k <= 8u; k++) { a.push_back(f2u(1.0f) + k); b.push_back(f2u(kDnSigmaNormalMax)); }
  for (uint32_t u = 0; u <= f2u(1.0f); u += 65521u) { a.push_back(u); b.push_back(f2u(kDnSigmaNormalMax)); }
  run(PT_MATH_DN_POWR);
  // the warps over [0, 1)^2, the edges included
  a.clear(); b.clear();
  for (uint32_t i = 0; i <= 256; i++)
    for (uint32_t j = 0; j <= 256; j++) {
      a.push_back(f2u(i == 256 ? kOneMinusEpsilon : (float)i / 256.0f));
      b.push_back(f2u(j == 256 ? kOneMinusEpsilon : (float)j / 256.0f));
    }
  run(PT_MATH_SAMPLE_DISK); run(PT_MATH_SAMPLE_COSINE_HEMISPHERE); run(PT_MATH_SAMPLE_TRI_UNIFORM);
  // Halton: every dimension, strided indices and the ends of the range
  a.clear(); b.clear();
  for (uint32_t d = 0; d < (uint32_t)kHaltonDims; d++) {
    for (uint64_t i = 0; i < (1ull << 32); i += 16777213u + d) { a.push_back((uint32_t)i); b.push_back(d); }
    a.push_back(0xffffffffu); b.push_back(d);
  }
  run(PT_MATH_HALTON); run(PT_MATH_HALTON_OFFSET);
  return 0;
}
#endif
