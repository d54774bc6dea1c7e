// TEST PROGRAM (tests/): the transparent film through include/ptamd_renderer.hpp and the C ABI without a GPU — the defaults, the struct
// layout, the accessors' types, and the order of the entry points' checks (the options before the renderer).  tests/test_film_cpp.py
// compiles and runs it; it returns 0 when everything holds.
#include <cstddef>
#include <cstdint>
#include <limits>
#include <type_traits>
#include <vector>

#include "ptamd_renderer.hpp"

using ptamd::renderer_pt::Renderer;

static_assert(sizeof(pt_film_options) == 20 && offsetof(pt_film_options, enabled) == 0 && offsetof(pt_film_options, backdrop) == 4 &&
                  offsetof(pt_film_options, backdrop_rgb) == 8,
              "pt_film_options");
static_assert(PT_BACKDROP_SCENE == 0 && PT_BACKDROP_COLOR == 1 && PT_BACKDROP_TRANSPARENT == 2, "the backdrops");
static_assert(std::is_same<decltype(std::declval<Renderer&>().filmOptions()), pt_film_options&>::value, "filmOptions() hands out the struct itself");
static_assert(std::is_same<decltype(std::declval<const Renderer&>().readbackFilm()), std::vector<float>>::value, "readbackFilm() returns W*H*4 floats");

int main() {
  pt_film_options o;
  o.enabled = 7u; o.backdrop = 7u; o.backdrop_rgb[0] = o.backdrop_rgb[1] = o.backdrop_rgb[2] = 7.0f;
  pt_default_film_options(&o);
  if (o.enabled != 0u || o.backdrop != PT_BACKDROP_SCENE) return 2;
  for (int k = 0; k < 3; k++)
    if (o.backdrop_rgb[k] != 0.0f) return 3;
  pt_default_film_options(nullptr);
  Renderer* r = nullptr;
  if (r) {   // (compiled, not run: no GPU here)
    pt_film_options& f = r->filmOptions();
    f = o;
    f.enabled = 1u;
    f.backdrop = PT_BACKDROP_TRANSPARENT;
    r->setFilmOptions(f);
    if (!r->readbackFilm().empty()) return 4;
  }
  if (pt_set_film_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 5;   // valid options, no renderer
  if (pt_set_film_options(nullptr, nullptr) != PT_ERR_INVALID_ARGUMENT) return 6;
  o.backdrop = 3u;
  if (pt_set_film_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 7;
  o.backdrop = PT_BACKDROP_COLOR;
  o.backdrop_rgb[2] = -1.0f;
  if (pt_set_film_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 8;
  o.backdrop_rgb[2] = std::numeric_limits<float>::infinity();
  if (pt_set_film_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 8;
  float px[4];
  if (pt_read_film(nullptr, px) != PT_ERR_INVALID_ARGUMENT) return 9;
  return 0;
}
