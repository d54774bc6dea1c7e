// film.h — host-visible launchers of the film kernels (film.hip; the fold and the compose arithmetic in pt_film.h).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "pt_film.h"

namespace pt {

// After the camera trace of a batch, before k_shade(0): 1 for a camera ray that hit, 0 for one that missed -> Fbuf (pid = the Lbuf index).
void launch_film_flags(hipStream_t s, uint32_t grid, PathState st, const vec4* hit, Segments seg, uint32_t* Fbuf);
// After the accumulate kernels: Lbuf masked by Fbuf folded into the film, per pixel in sample order (n0 samples already in it); over `tiles`
// (kernels.h TileSet: the per-sample buffers dense over virtual tiles) or, when null, over the whole frame.
void launch_accumulate_film(hipStream_t s, vec4* film, const vec4* Lbuf, const uint32_t* Fbuf, uint32_t width, uint32_t height, uint32_t nsamples,
                            uint32_t n0, uint32_t nonfinite_policy, const TileSet* tiles);
// out[pixel] = film_compose(base, film.a) inside `rect`, 0 outside it; over the whole frame.  backdrop: PT_BACKDROP_COLOR or _TRANSPARENT.
void launch_film_compose(hipStream_t s, const vec4* base, const vec4* film, vec4* out, uint32_t width, uint32_t height, const Rect& rect,
                         const pt_film_options& o);
// After k_postprocess (transparent mode): the target's alpha byte := the quantised .w of the composed source.
void launch_film_alpha(hipStream_t s, uint32_t* target, const vec4* composed, uint32_t npix);

}  // namespace pt
