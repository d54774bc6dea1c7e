// camera_lists.h — host-visible launcher of the per-pixel leaf lists of a pinhole camera (camera_lists.hip; geometry in pt_camlist.h).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_camlist.h"

namespace pt {

// what the build reports (device-side counters, read back once per pt_start_render)
struct CamListCounters {
  unsigned long long listed;    // pixels of the image with a list that fits (an empty one included)
  unsigned long long walk;      // pixels flagged kCamWalk
  unsigned long long entries;   // entries of the lists that fit
  uint32_t hist[kCamHistBins];  // pixels by list length BEFORE the capacity is applied: 0 .. 63, 64 or more
  uint32_t _pad;
};

// Builds the lists of every pixel of the W x H image over the 6-wide one-BVH structure in S (S.wide6, S.root_ref a node): `entries` holds
// tile_count * 64 * cap records, `count` tile_count * 64 words (pixel slot = tile * 64 + lane); *counters must be zero.
void launch_camera_lists(hipStream_t s, const DeviceScene& S, CamListEntry* entries, uint32_t* count, uint32_t cap, CamListCounters* counters);

}  // namespace pt
