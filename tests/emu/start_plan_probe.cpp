// TEST HARNESS ONLY (tests/emu) — the host build of the decisions pt_start_render takes (platinum_amd/csrc/host_scene.h: the instance
// records of the two-level structure, the choice of structure, the camera-list bound, the queue budget), one export per function, for
// tests/test_start_plan_host.py.  Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
// Sixth part of tests/emu/host_harness.cpp; not compiled alone.
#ifndef PTAMD_TESTS_EMU_START_PLAN_PROBE
#define PTAMD_TESTS_EMU_START_PLAN_PROBE
#include "../../platinum_amd/csrc/host_scene.h"

using namespace pt;

extern "C" {

// in: n InstanceInfo records; out: n InstanceTrav records (pre-filled by the caller: a record the function does not reach keeps its fill)
int sp_instance_trav(const InstanceInfo* in, uint32_t n, InstanceTrav* out) {
  std::vector<InstanceTrav> trav;
  const bool invertible = instance_trav_records(std::vector<InstanceInfo>(in, in + n), &trav);
  if (invertible) memcpy(out, trav.data(), sizeof(InstanceTrav) * n);
  return invertible ? 1 : 0;
}
int sp_choose_accel(int invertible, uint32_t tri_count, uint64_t unique_tris, uint64_t free_bytes, uint32_t accel_structure, int override,
                    int* automatic) {
  const AccelChoice c = choose_accel_structure(invertible != 0, tri_count, unique_tris, free_bytes, accel_structure, override);
  *automatic = c.automatic ? 1 : 0;
  return c.two_level ? 1 : 0;
}
uint64_t sp_flat_bytes_per_tri() { return kFlatBytesPerTri; }
int sp_camera_lists_wanted(int disabled, int two_level, int wide6, uint32_t root_ref, float aperture_radius, int adaptive, int region) {
  return camera_lists_wanted(disabled != 0, two_level != 0, wide6 != 0, root_ref, aperture_radius, adaptive != 0, region != 0) ? 1 : 0;
}
uint64_t sp_cam_entry_size() { return sizeof(CamListEntry); }
uint32_t sp_cam_default_capacity() { return kCamListCapacity; }
uint64_t sp_camera_list_bytes(uint32_t W, uint32_t H, uint32_t cap) { return camera_list_bytes(W, H, cap); }
int sp_camera_lists_fit(uint64_t bytes, uint64_t free_bytes, uint64_t lists_held) { return camera_lists_fit(bytes, free_bytes, lists_held) ? 1 : 0; }
uint64_t sp_queue_budget(uint64_t free_bytes, uint64_t queues_held, uint64_t lists_held, int aov, uint64_t abuf_held) {
  return queue_budget(free_bytes, queues_held, lists_held, aov != 0, abuf_held);
}

}  // extern "C"

#endif  // PTAMD_TESTS_EMU_START_PLAN_PROBE
