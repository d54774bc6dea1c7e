// TEST PROGRAM (tests/): the selection overlay through include/ptamd_renderer.hpp and the C ABI without a GPU — the defaults, the struct
// layout, the accessors' types, and the order of the entry points' checks (the options before the renderer).  tests/test_selection_cpp.py
// compiles and runs it; it returns 0 when everything holds.
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <vector>

#include "ptamd_renderer.hpp"

using ptamd::renderer_pt::Renderer;

static_assert(sizeof(pt_selection_options) == 48 && offsetof(pt_selection_options, width) == 8 && offsetof(pt_selection_options, outline_rgba) == 16 &&
                  offsetof(pt_selection_options, fill_rgba) == 32,
              "pt_selection_options");
static_assert(std::is_same<decltype(std::declval<Renderer&>().selectionOptions()), pt_selection_options&>::value,
              "selectionOptions() hands out the struct itself");
static_assert(std::is_same<decltype(std::declval<const Renderer&>().selection()), std::vector<uint32_t>>::value, "selection() returns the ids");
static_assert(std::is_same<decltype(std::declval<Renderer&>().setSelection(std::declval<const std::vector<uint32_t>&>())), bool>::value, "setSelection(ids)");

int main() {
  pt_selection_options o;
  pt_default_selection_options(&o);
  if (o.enabled != 0u || o.layer != PT_MATTE_INSTANCE || o.width != 2.0f || o._pad != 0.0f) return 2;
  const float outline[4] = {1.0f, 0.55f, 0.0f, 1.0f}, fill[4] = {1.0f, 0.55f, 0.0f, 0.0f};
  for (int k = 0; k < 4; k++)
    if (o.outline_rgba[k] != outline[k] || o.fill_rgba[k] != fill[k]) return 3;
  pt_default_selection_options(nullptr);
  Renderer* r = nullptr;
  if (r) {   // (compiled, not run: no GPU here)
    pt_selection_options& s = r->selectionOptions();
    s = o;
    s.enabled = 1u;
    if (!r->setSelection({3u, 1u, 3u}) || r->selection().size() != 2u) return 4;
  }
  if (pt_set_selection_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 5;   // valid options, no renderer
  if (pt_set_selection_options(nullptr, nullptr) != PT_ERR_INVALID_ARGUMENT) return 6;
  o.width = 0.5f;
  if (pt_set_selection_options(nullptr, &o) != PT_ERR_INVALID_ARGUMENT) return 7;
  const uint32_t ids[2] = {1u, 2u};
  uint32_t n = 0;
  if (pt_set_selection(nullptr, ids, 2u) != PT_ERR_INVALID_ARGUMENT) return 8;
  if (pt_get_selection(nullptr, nullptr, 0u, &n) != PT_ERR_INVALID_ARGUMENT) return 9;
  return 0;
}
