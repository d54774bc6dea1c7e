// TEST HARNESS ONLY (tests/emu) — the host build of the ID-matte arithmetic (platinum_amd/csrc/pt_matte.h: matte_fold, matte_id_set,
// matte_coverage, matte_pick) and the layout of the three matte structs of include/ptamd.h as the C compiler sees them, for
// tests/test_matte_host.py and tests/test_gpu_matte.py.  Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// A translation unit of its own: tests/matte_lib.py builds it into tests/_build/libptamd_matte.so (tests/host_build.py load).
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/ptamd.h"
#include "../../platinum_amd/csrc/pt_matte.h"

using namespace pt;

static_assert(PT_MATTE_SLOTS == kMatteSlots && PT_MATTE_NONE == kMatteNone, "ptamd.h and pt_matte.h name the same constants");

namespace {

MatteSlots load(const pt_matte_slot* s) {
  MatteSlots m;
  for (uint32_t k = 0; k < kMatteSlots; k++) { m.id[k] = s[k].id; m.count[k] = s[k].count; }
  return m;
}
void store(const MatteSlots& m, pt_matte_slot* s) {
  for (uint32_t k = 0; k < kMatteSlots; k++) { s[k].id = m.id[k]; s[k].count = m.count[k]; }
}

}  // namespace

extern "C" {

// slots[PT_MATTE_SLOTS] := every slot empty
void mt_host_clear(pt_matte_slot* slots) {
  MatteSlots m;
  matte_clear(m);
  store(m, slots);
}

// ids[0, n) folded in order into slots[PT_MATTE_SLOTS], which hold the state before and after
void mt_host_fold(const uint32_t* ids, uint32_t n, pt_matte_slot* slots) {
  MatteSlots m = load(slots);
  for (uint32_t i = 0; i < n; i++) matte_fold(m, ids[i]);
  store(m, slots);
}

// out[p] = the coverage of the id set ids[0, id_count) (any order, duplicates allowed: sorted as pt_read_matte sorts it) in pixel p of
// slots[npix][PT_MATTE_SLOTS] with n[p] samples
void mt_host_coverage(const pt_matte_slot* slots, uint32_t npix, const uint32_t* ids, uint32_t id_count, const uint32_t* n, float* out) {
  const std::vector<uint32_t> set = matte_id_set(ids, id_count);
  for (uint32_t p = 0; p < npix; p++) out[p] = matte_coverage(load(slots + (size_t)p * kMatteSlots), set.data(), (uint32_t)set.size(), n[p]);
}

uint32_t mt_host_pick(const pt_matte_slot* slots) { return matte_pick(load(slots)); }

// sizeof, then the offset of every field: pt_matte_options (2 words), pt_matte_slot (3), pt_pick_result (9); then PT_MATTE_SLOTS, PT_MATTE_NONE,
// PT_MATTE_INSTANCE, PT_MATTE_MATERIAL
void mt_host_layout(uint32_t out[18]) {
  const size_t v[18] = {sizeof(pt_matte_options), offsetof(pt_matte_options, enabled),
                        sizeof(pt_matte_slot), offsetof(pt_matte_slot, id), offsetof(pt_matte_slot, count),
                        sizeof(pt_pick_result), offsetof(pt_pick_result, instance), offsetof(pt_pick_result, instance_count),
                        offsetof(pt_pick_result, material), offsetof(pt_pick_result, material_count), offsetof(pt_pick_result, material_instance),
                        offsetof(pt_pick_result, material_slot), offsetof(pt_pick_result, samples), offsetof(pt_pick_result, _pad),
                        PT_MATTE_SLOTS, PT_MATTE_NONE, PT_MATTE_INSTANCE, PT_MATTE_MATERIAL};
  for (int i = 0; i < 18; i++) out[i] = (uint32_t)v[i];
}

}  // extern "C"
