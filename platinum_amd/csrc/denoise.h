// denoise.h — host-visible launchers of the AOV and denoiser kernels (denoise.hip; arithmetic in pt_denoise.h).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pt_denoise.h"

namespace pt {

// After k_trace_closest(bounce 0) of a batch: the first-hit AOVs of every camera ray -> Abuf (2 vec4 per pid, pid = the Lbuf index).
void launch_aov(hipStream_t s, uint32_t grid, const DeviceScene* S_device, PathState st, const vec4* hit, Segments seg, vec4* Abuf);
// After k_accumulate / k_gmon: Abuf and Lbuf of the batch folded into the three AOV images (n0 samples already in them); over `tiles`
// (kernels.h TileSet: Abuf and Lbuf dense over virtual tiles) or, when null, over the whole frame.
void launch_accumulate_aov(hipStream_t s, vec4* albedo, vec4* normal, vec4* moments, const vec4* Abuf, const vec4* Lbuf, uint32_t width,
                           uint32_t height, uint32_t nsamples, uint32_t n0, uint32_t nonfinite_policy, const TileSet* tiles);
// The filter over the rectangle `rect` of the current W x H image, as if the rectangle were the whole image (the whole frame: {0, 0, W, H}):
// prep, `iterations` a-trous steps, the last one remodulated into `out` (W*H vec4; pixels outside rect are left as they are).
// guide / aux / col0 / col1 are W*H vec4 of scratch each; nsamples = samples folded into the AOVs, or, with tile_n (an adaptive render),
// tile_n[8x8 tile of the frame] = the samples folded into each pixel of that tile.  With despeckle.enabled (and iterations >= 1) the firefly
// clamp runs between the prep and the first a-trous step, col0 -> col1, and the ping-pong starts from col1.
void launch_denoise(hipStream_t s, const vec4* acc, const vec4* albedo, const vec4* normal, const vec4* moments, uint32_t W, uint32_t H,
                    uint32_t nsamples, const DenoiseParams& P, uint32_t iterations, vec4* guide, vec4* aux, vec4* col0, vec4* col1, vec4* out,
                    const uint32_t* tile_n, const Rect& rect, const pt_despeckle_options& despeckle);

}  // namespace pt
