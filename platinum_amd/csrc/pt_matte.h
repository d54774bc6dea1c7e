// pt_matte.h — ID mattes: per-pixel coverage of the camera rays' first hits by instance and by material.
//
//   matte_fold      : one sample's id folded into a pixel's eight slots {id, count}
//   matte_coverage  : the slots resolved against a sorted id set: (float)(sum of the counts of the slots whose id is in the set) / (float)n
//   matte_pick      : the slot with the largest count, ties to the lowest slot
// Plain integer functions (PT_HD, no HIP types): the same code for hipcc (matte.hip, renderer.hip) and for the g++ build under tests/emu.
//
// The fold.  A pixel's samples are folded in sample order 0, 1, 2, ... (n0 + s, as k_accumulate folds radiance).  A sample's id is its camera
// ray's first hit's id — the instance index, or ShadeRec::material, the index of the hit triangle's material in the flattened material table:
// (sum of material_count of the instances before its own) + the triangle's material slot (host_scene.h flatten_scene) — and kMatteNone for a
// miss, which takes a slot like any other id.  The slots are scanned 0..7: the first with count != 0 and the sample's id gets count + 1;
// otherwise the first with count == 0 becomes {id, 1}; otherwise the sample goes to nothing.  First come, no eviction: the slots are a
// function of the ordered sample sequence alone, and what did not fit is other = n - sum of the counts, derived and never stored.
#pragma once
#include <algorithm>
#include <vector>

#include "pt_math.h"

namespace pt {

constexpr uint32_t kMatteSlots = 8;             // PT_MATTE_SLOTS
constexpr uint32_t kMatteNone = 0xffffffffu;    // PT_MATTE_NONE: the id of a miss, and of an empty slot {kMatteNone, 0}
constexpr uint32_t kMatteLayers = 2;            // PT_MATTE_INSTANCE, PT_MATTE_MATERIAL

// what k_matte_ids keeps of one camera ray: 8 B per path slot, indexed like Lbuf
struct alignas(8) MatteIds { uint32_t inst, material; };
static_assert(sizeof(MatteIds) == 8, "MatteIds");

// a pixel's slots of one layer, as registers: every index below is a compile-time constant once the loops are unrolled
struct MatteSlots { uint32_t id[kMatteSlots], count[kMatteSlots]; };

PT_HD void matte_clear(MatteSlots& m) {
#pragma unroll
  for (uint32_t k = 0; k < kMatteSlots; k++) { m.id[k] = kMatteNone; m.count[k] = 0u; }
}

// Compare-selects only, fully unrolled (a runtime-indexed register array would live in scratch).
PT_HD void matte_fold(MatteSlots& m, uint32_t x) {
  bool done = false;
#pragma unroll
  for (uint32_t k = 0; k < kMatteSlots; k++) {
    const bool hit = !done && m.count[k] != 0u && m.id[k] == x;
    m.count[k] += hit ? 1u : 0u;
    done = done || hit;
  }
#pragma unroll
  for (uint32_t k = 0; k < kMatteSlots; k++) {
    const bool take = !done && m.count[k] == 0u;
    m.id[k] = take ? x : m.id[k];
    m.count[k] = take ? 1u : m.count[k];
    done = done || take;
  }
}

// is x in ids[0, n), ascending and without duplicates?
PT_HD bool matte_in_set(const uint32_t* ids, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint32_t v = ids[mid];
    if (v < x) lo = mid + 1u; else hi = mid;
  }
  return lo < n && ids[lo] == x;
}

// the caller's id set as matte_in_set wants it: ascending, without duplicates (host only: pt_read_matte uploads this)
inline std::vector<uint32_t> matte_id_set(const uint32_t* ids, uint32_t n) {
  std::vector<uint32_t> set(ids, ids + n);
  std::sort(set.begin(), set.end());
  set.erase(std::unique(set.begin(), set.end()), set.end());
  return set;
}

// coverage of the id set in a pixel of n samples: one IEEE division; n = 0 gives 0
PT_HD float matte_coverage(const MatteSlots& m, const uint32_t* ids, uint32_t id_count, uint32_t n) {
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < kMatteSlots; k++) sum += matte_in_set(ids, id_count, m.id[k]) ? m.count[k] : 0u;
  return n == 0u ? 0.0f : (float)sum / (float)n;
}

// the slot with the largest count, ties to the lowest slot (a pixel without samples: slot 0, {kMatteNone, 0})
PT_HD uint32_t matte_pick(const MatteSlots& m) {
  uint32_t best = 0;
  for (uint32_t k = 1; k < kMatteSlots; k++)
    if (m.count[k] > m.count[best]) best = k;
  return best;
}

}  // namespace pt
