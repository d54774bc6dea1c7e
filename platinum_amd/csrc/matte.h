// matte.h — host-visible launchers of the ID-matte kernels (matte.hip; the fold and the resolve arithmetic in pt_matte.h).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pt_matte.h"

namespace pt {

// The slot image: [pixel][layer][slot] {id, count}, 128 B per pixel, addressed as 8 uint4 {id, count, id, count} per pixel.
constexpr uint32_t kMattePixelVec4 = kMatteLayers * kMatteSlots / 2u;
constexpr size_t kMattePixelBytes = (size_t)kMattePixelVec4 * sizeof(uint4);

// every slot of `npix` pixels := {kMatteNone, 0}
void launch_matte_clear(hipStream_t s, uint4* slots, size_t npix);
// After the camera trace of a batch, before k_shade(0): the first hit's {instance, material} of every camera ray -> Mbuf (pid = the Lbuf index).
void launch_matte_ids(hipStream_t s, uint32_t grid, const DeviceScene* S_device, PathState st, const vec4* hit, Segments seg, MatteIds* Mbuf);
// After the accumulate kernels: Mbuf of the batch folded into both layers' slots, per pixel in sample order; over `tiles` (kernels.h
// TileSet: Mbuf dense over virtual tiles) or, when null, over the whole frame.
void launch_accumulate_matte(hipStream_t s, uint4* slots, const MatteIds* Mbuf, uint32_t width, uint32_t height, uint32_t nsamples,
                             const TileSet* tiles);
// coverage_out[pixel] = matte_coverage of the pixel's `layer` slots against ids[0, id_count) (device, ascending, no duplicates).  The pixel's
// sample count is tile_n[its tile] inside `rect` and 0 outside it, or n_uniform everywhere when tile_n is null.
void launch_matte_resolve(hipStream_t s, const uint4* slots, uint32_t layer, const uint32_t* ids, uint32_t id_count, const uint32_t* tile_n,
                          uint32_t n_uniform, const Rect& rect, uint32_t width, uint32_t height, float* coverage_out);

}  // namespace pt
