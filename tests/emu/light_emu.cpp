// TEST HARNESS ONLY (tests/emu) — the host build of the light-sampling part of the shading stage as pt_debug_lights runs it
// (platinum_amd/csrc/pt_light_probe.h over pt_shade.h), on the scene an Emu holds, for tests/test_light_witness_host.py and
// tests/test_gpu_light_witness.py.  Part of tests/emu/host_harness.cpp (after wavefront_emu.cpp, which defines Emu); not compiled alone.
// Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
#include "../../platinum_amd/csrc/pt_light_probe.h"

extern "C" {

// pt_debug_lights' signature on an emu_create handle: the same fn ids, arguments and records; -1 where the device refuses the call.
// PT_LIGHT_TABLES_LDS copies the records into a table of the staged size with the kernel's copy loop and sets lights_lds, as a block does.
int emu_light_probe(void* h, uint32_t fn, uint32_t n, const pt_light_probe_args* args, const void* in_, void* out_) {
  const Emu* e = (const Emu*)h;
  const DeviceScene& S = e->S;
  constexpr uint32_t kStaged = 64;  // light_probe.h kLightProbeStaged = kernels.hip kShadeLights
  if (fn >= PT_LIGHT_COUNT || !args || !in_ || !out_ || light_probe_unsupported(S, fn, *args, kStaged)) return -1;
  const float* in = (const float*)in_;
  uint32_t* out = (uint32_t*)out_;
  ShadeTables T = shade_tables(S);
  std::vector<LightRec> staged(kStaged);
  if (fn == PT_LIGHT_SAMPLE && args->tables == PT_LIGHT_TABLES_LDS) {
    struct Q { uint32_t w[4]; };
    const Q* ls = reinterpret_cast<const Q*>(S.light_recs);
    Q* ld = reinterpret_cast<Q*>(staged.data());
    for (uint32_t i = 0; i < S.lightCount * (uint32_t)(sizeof(LightRec) / 16); i++) memcpy(&ld[i], &ls[i], sizeof(Q));
    T.lights = staged.data();
    T.lights_lds = 1;
  }
  const uint32_t wi = light_probe_in_words(fn), wo = light_probe_out_words(fn);
  for (uint32_t i = 0; i < n; i++) {
    if (fn == PT_LIGHT_SAMPLE) light_probe_sample(S, T, *args, in + (size_t)i * wi, out + (size_t)i * wo);
    else light_probe_miss(S, *args, in + (size_t)i * wi, out + (size_t)i * wo);
  }
  return 0;
}

uint64_t emu_get_env_alias(void* h, pt_alias_entry* out, uint64_t cap) {
  const Emu* e = (const Emu*)h;
  for (uint64_t i = 0; i < std::min<uint64_t>(cap, e->hs.env_alias.size()); i++) out[i] = e->hs.env_alias[i];
  return e->hs.env_alias.size();
}

}  // extern "C"
