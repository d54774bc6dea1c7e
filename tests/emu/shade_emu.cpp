// TEST HARNESS ONLY (tests/emu) — the host build of the stage between a hit record and the BSDF as pt_debug_shading runs it
// (platinum_amd/csrc/pt_shade_probe.h over pt_shade.h and pt_bsdf.h), on the scene an Emu holds, for tests/test_shading_witness_host.py and
// tests/test_gpu_shading_witness.py.  Part of tests/emu/host_harness.cpp (after wavefront_emu.cpp, which defines Emu); not compiled alone.
// Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
#include "../../platinum_amd/csrc/pt_shade_probe.h"

extern "C" {

// pt_debug_shading's signature on an emu_create handle: the same records; -1 where the device refuses the call
int emu_shade_probe(void* h, uint32_t n, const void* in_, void* out_) {
  const Emu* e = (const Emu*)h;
  const DeviceScene& S = e->S;
  if (n == 0 || n > (1u << 24) || !in_ || !out_) return -1;
  const uint32_t n_tri = 2u * (uint32_t)e->tris.size();
  std::vector<int32_t> ids(2 * (size_t)n_tri);
  for (uint32_t t = 0; t < n_tri; t++) shade_probe_ids(S, t, &ids[2 * (size_t)t]);
  std::vector<uint32_t> rec((size_t)n * PT_SHADE_PROBE_IN_WORDS);
  memcpy(rec.data(), in_, sizeof(uint32_t) * rec.size());
  if (!shade_probe_resolve(ids.data(), n_tri, rec.data(), n)) return -1;
  uint32_t* out = (uint32_t*)out_;
  for (uint32_t i = 0; i < n; i++) shade_probe_element(S, &rec[(size_t)i * PT_SHADE_PROBE_IN_WORDS], out + (size_t)i * PT_SHADE_PROBE_OUT_WORDS);
  return 0;
}

}  // extern "C"
