// exposure.h — host-side launch interface of exposure.hip: the auto-exposure meter ahead of the post-process.
#pragma once
#include <hip/hip_runtime.h>

#include "pt_exposure.h"

namespace pt {

// What the meter keeps on the device: the record pt_read_exposure_meter returns (its first 259 words are the histogram's counters) and
// the smoothing state, the ev the newest target applied.
struct ExposureRecord {
  pt_exposure_meter meter;
  float prev_ev;
  uint32_t has_prev;
};

// Meters the rectangle `rect` of the W-wide image `img` into rec->meter: clears the counters, k_exposure_histogram, k_exposure_resolve.
// for_target: the launch is made for a target, and rec's smoothing state advances to the ev it resolved.  Returns the memset's or the
// launches' error.
hipError_t launch_exposure_meter(hipStream_t s, const vec4* img, uint32_t W, const Rect& rect, const pt_exposure_options& o, ExposureRecord* rec,
                                 bool for_target);
// out = img.rgb * rec->meter.gain, alpha copied, over all npix pixels of the frame
void launch_exposure_apply(hipStream_t s, const vec4* img, vec4* out, uint32_t npix, const ExposureRecord* rec);

}  // namespace pt
