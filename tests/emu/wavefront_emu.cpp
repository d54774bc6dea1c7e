// TEST HARNESS ONLY (tests/emu) — runs the product's per-path stage functions (platinum_amd/csrc/pt_*.h, which are
// plain C++ under PT_HD) on the HOST, so that stage logic can be compared with the oracle in the GPU-less
// authoring container.  It is not part of libptamd.so, is never loaded by platinum_amd, and is not a fallback:
// it exists to debug bit-exactness before spending GPU time.  Queues, compaction and the LBVH build (the
// __global__ kernels) are NOT covered here — only `-m gpu` tests exercise those.
//
// The BVH used here is a throw-away host builder that emits the product's BvhNode / BvhNode6 / TriRec layout: median split collapsed to
// 4-wide nodes, or under $EMU_MORTON (with $EMU_PLOC=<radius>), $EMU_WIDE6 and $EMU_PAIRS the product's own tree form.
//
// First part of tests/emu/host_harness.cpp, the one translation unit of tests/_build/libptamd_host.so (tests/host_build.py); not
// compiled alone.  It holds what a test, bench.py's cpu_baseline or a kept tool reaches and nothing else: the probes of closed
// experiments that only need an Emu and traverse<> live in tools/archive/emu_probes.cpp.
#ifndef PTAMD_TESTS_EMU_WAVEFRONT_EMU
#define PTAMD_TESTS_EMU_WAVEFRONT_EMU
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

// $EMU_RCP_ULP = -1 / +1 (every component) / 2 (+-1 alternating by axis and sign; any even value: +- half of it): the ray's reciprocal direction moved by one ulp before the slab tests, as
// the device's v_rcp_f32 may: hits and radiance must not change (tests/test_stage_functions_host.py)
#include "../../platinum_amd/csrc/pt_math.h"
static int g_emu_rcp_ulp = 0;
static inline void emu_perturb_rcp(pt::vec3& inv) {
  if (!g_emu_rcp_ulp) return;
  float* c[3] = {&inv.x, &inv.y, &inv.z};
  for (int a = 0; a < 3; a++) {
    uint32_t b = pt::f2u(*c[a]);
    if ((b & 0x7f800000u) == 0x7f800000u || (b & 0x7fffffffu) == 0) continue;
    const int dir = (g_emu_rcp_ulp & 1) ? g_emu_rcp_ulp : (((a + (b >> 31)) & 1) ? g_emu_rcp_ulp / 2 : -g_emu_rcp_ulp / 2);   // odd: uniform; even: alternating +- half
    b += (uint32_t)dir;   // magnitude +- 1 ulp
    *c[a] = pt::u2f(b);
  }
}
#define PT_TEST_PERTURB_RCP(v) emu_perturb_rcp(v)
#include "../../platinum_amd/csrc/host_scene.h"
#include "../../platinum_amd/csrc/pt_layout.h"
#include "../../platinum_amd/csrc/pt_shade.h"

using namespace pt;

namespace {

struct Emu {
  HostScene hs;
  std::vector<float> lut;
  std::vector<HaltonEntry> halton;
  std::vector<TriRec> tris;
  std::vector<ShadeRec> shade_recs;
  std::vector<LightRec> light_recs;
  std::vector<float> light_cdf;
  std::vector<BvhNode> nodes;
  DeviceScene S{};
  pt_render_params params{};
};

Box3 tri_box(const TriRec& t, const vec3& v1, const vec3& v2) {
  Box3 b;
  const float* a = t.q0; const float* p1 = &v1.x; const float* p2 = &v2.x;
  for (int k = 0; k < 3; k++) { b.lo[k] = std::min(a[k], std::min(p1[k], p2[k])); b.hi[k] = std::max(a[k], std::max(p1[k], p2[k])); }
  return b;
}

// Binary median-split tree first (host only), then the same even-depth collapse + quantize_node4 the GPU builder uses.
struct BinNode { uint32_t left, right; Box3 box; };

uint32_t build_bin(std::vector<BinNode>& bin, std::vector<uint32_t>& order, const std::vector<Box3>& boxes, uint32_t first, uint32_t count) {
  if (count == 1) return kLeafBit | first;
  Box3 bb; for (int k = 0; k < 3; k++) { bb.lo[k] = 1e30f; bb.hi[k] = -1e30f; }
  for (uint32_t i = first; i < first + count; i++)
    for (int k = 0; k < 3; k++) { bb.lo[k] = std::min(bb.lo[k], boxes[order[i]].lo[k]); bb.hi[k] = std::max(bb.hi[k], boxes[order[i]].hi[k]); }
  int axis = 0; float ext = -1;
  for (int k = 0; k < 3; k++) if (bb.hi[k] - bb.lo[k] > ext) { ext = bb.hi[k] - bb.lo[k]; axis = k; }
  uint32_t mid = first + count / 2;
  std::nth_element(order.begin() + first, order.begin() + mid, order.begin() + first + count, [&](uint32_t a, uint32_t b) {
    return boxes[a].lo[axis] + boxes[a].hi[axis] < boxes[b].lo[axis] + boxes[b].hi[axis]; });
  uint32_t idx = (uint32_t)bin.size();
  bin.push_back({});
  uint32_t l = build_bin(bin, order, boxes, first, mid - first);
  uint32_t r = build_bin(bin, order, boxes, mid, first + count - mid);
  bin[idx] = {l, r, bb};
  return idx;
}

static float half_area(const Box3& b) { const float x = b.hi[0] - b.lo[0], y = b.hi[1] - b.lo[1], z = b.hi[2] - b.lo[2]; return x * y + y * z + z * x; }

// LBVH-like topology (experiments: EMU_MORTON=1): sort by 63-bit Morton code of the box centre, split ranges at the highest
// differing bit (what the Karras tree of lbvh.hip encodes).
static uint64_t expand21(uint64_t v) { v &= 0x1fffff; v = (v | v << 32) & 0x1f00000000ffffull; v = (v | v << 16) & 0x1f0000ff0000ffull;
  v = (v | v << 8) & 0x100f00f00f00f00full; v = (v | v << 4) & 0x10c30c30c30c30c3ull; v = (v | v << 2) & 0x1249249249249249ull; return v; }
uint32_t build_morton(std::vector<BinNode>& bin, const std::vector<uint32_t>& order, const std::vector<uint64_t>& keys, const std::vector<Box3>& boxes,
                      uint32_t first, uint32_t count) {
  if (count == 1) return kLeafBit | first;
  uint32_t split = first + count / 2;
  const uint64_t a = keys[first], b = keys[first + count - 1];
  if (a != b) {
    const int bit = 63 - __builtin_clzll(a ^ b);
    uint32_t lo = first, hi = first + count - 1;  // first index whose `bit` is set
    while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if ((keys[mid] >> bit) & 1) hi = mid; else lo = mid + 1; }
    split = lo;
  }
  const uint32_t idx = (uint32_t)bin.size();
  bin.push_back({});
  const uint32_t l = build_morton(bin, order, keys, boxes, first, split - first);
  const uint32_t r = build_morton(bin, order, keys, boxes, split, first + count - split);
  Box3 bb;
  auto box_of = [&](uint32_t ref) { return (ref & kLeafBit) ? boxes[order[ref & ~kLeafBit]] : bin[ref].box; };
  const Box3 bl = box_of(l), br = box_of(r);
  for (int k = 0; k < 3; k++) { bb.lo[k] = std::min(bl.lo[k], br.lo[k]); bb.hi[k] = std::max(bl.hi[k], br.hi[k]); }
  bin[idx] = {l, r, bb};
  return idx;
}

// EMU_WIDE6=1: the product's 6-wide form (BvhNode6, lbvh.hip emit_sah_node6): open the child with the largest surface area until six slots
// are used, internal children first; a node's internal children get consecutive records and its leaf children consecutive triangle slots
// (tri_perm[slot] = position in `order`).  Depth-first here (the GPU numbers level by level): the traversal only needs the two properties.
void collapse6(Emu& e, const std::vector<BinNode>& bin, const std::vector<uint32_t>& order, const std::vector<Box3>& boxes, uint32_t i, uint32_t dense,
               std::vector<uint32_t>& tri_perm) {
  uint32_t refs[6] = {bin[i].left, bin[i].right, 0, 0, 0, 0}; int count = 2;
  auto box_of = [&](uint32_t ref) { return (ref & kLeafBit) ? boxes[order[ref & ~kLeafBit]] : bin[ref].box; };
  while (count < 6) {
    int best = -1; float ba = -1.0f;
    for (int k = 0; k < count; k++) if (!(refs[k] & kLeafBit)) { const float a = half_area(box_of(refs[k])); if (a > ba) { ba = a; best = k; } }
    if (best < 0) break;
    const uint32_t r = refs[best];
    refs[best] = bin[r].left; refs[count++] = bin[r].right;
  }
  uint32_t ints[6], n_int = 0, n_leaf = 0;
  Box3 bi[6], bl[6], bx[6];
  const uint32_t base_leaf = (uint32_t)tri_perm.size();
  for (int k = 0; k < count; k++) {
    if (refs[k] & kLeafBit) { bl[n_leaf++] = inflate_box(box_of(refs[k])); tri_perm.push_back(refs[k] & ~kLeafBit); }
    else { bi[n_int] = inflate_box(box_of(refs[k])); ints[n_int++] = refs[k]; }
  }
  for (uint32_t k = 0; k < n_int; k++) bx[k] = bi[k];
  for (uint32_t k = 0; k < n_leaf; k++) bx[n_int + k] = bl[k];
  const uint32_t base_node = (uint32_t)e.nodes.size();
  e.nodes.resize(e.nodes.size() + n_int);
  const BvhNode6 n6 = quantize_node6(bx, (int)n_int, (int)n_leaf, base_node, base_leaf);
  memcpy(&e.nodes[dense], &n6, sizeof(n6));
  for (uint32_t k = 0; k < n_int; k++) collapse6(e, bin, order, boxes, ints[k], base_node + k, tri_perm);
}

// EMU_PLOC=<radius>: parallel locally-ordered clustering (Meister & Bittner 2018) on the Morton order — prototype of a GPU
// builder that approaches SAH quality: every cluster finds its nearest neighbour (smallest merged surface area) within
// +-radius positions, mutual nearest neighbours merge, the array is compacted, repeat.
uint32_t build_ploc(std::vector<BinNode>& bin, const std::vector<uint32_t>& order, const std::vector<Box3>& boxes, int radius) {
  struct Cl { uint32_t ref; Box3 box; };
  std::vector<Cl> c(order.size()), next;
  for (size_t i = 0; i < order.size(); i++) c[i] = {kLeafBit | (uint32_t)i, boxes[order[i]]};
  auto merged_area = [](const Box3& a, const Box3& b) {
    Box3 m; for (int k = 0; k < 3; k++) { m.lo[k] = std::min(a.lo[k], b.lo[k]); m.hi[k] = std::max(a.hi[k], b.hi[k]); }
    return half_area(m);
  };
  std::vector<int> nn;
  while (c.size() > 1) {
    const int n = (int)c.size();
    nn.assign(n, -1);
    for (int i = 0; i < n; i++) {
      float best = 1e30f;
      for (int j = std::max(0, i - radius); j <= std::min(n - 1, i + radius); j++) {
        if (j == i) continue;
        const float a = merged_area(c[i].box, c[j].box);
        if (a < best) { best = a; nn[i] = j; }
      }
    }
    next.clear();
    for (int i = 0; i < n; i++) {
      const int j = nn[i];
      if (nn[j] == i) {
        if (i < j) {
          BinNode b; b.left = c[i].ref; b.right = c[j].ref;
          for (int k = 0; k < 3; k++) { b.box.lo[k] = std::min(c[i].box.lo[k], c[j].box.lo[k]); b.box.hi[k] = std::max(c[i].box.hi[k], c[j].box.hi[k]); }
          bin.push_back(b);
          next.push_back({(uint32_t)bin.size() - 1, b.box});
        }
      } else next.push_back(c[i]);
    }
    c.swap(next);
  }
  return c[0].ref;
}

void collapse(Emu& e, const std::vector<BinNode>& bin, const std::vector<uint32_t>& order, const std::vector<Box3>& boxes, uint32_t i) {
  uint32_t refs[4]; Box3 bx[4]; int count = 0;
  auto add = [&](uint32_t ref) {
    bx[count] = inflate_box((ref & kLeafBit) ? boxes[order[ref & ~kLeafBit]] : bin[ref].box);
    refs[count++] = ref;
  };
  const uint32_t c[2] = {bin[i].left, bin[i].right};
  for (int k = 0; k < 2; k++) {
    if (c[k] & kLeafBit) add(c[k]);
    else { add(bin[c[k]].left); add(bin[c[k]].right); }
  }
  e.nodes[i] = quantize_node4(bx, refs, count);
  for (int k = 0; k < count; k++) if (!(refs[k] & kLeafBit)) collapse(e, bin, order, boxes, refs[k]);
}

// One host thread's traversal scratch: what a lane of the trace kernels keeps in LDS (stack rows, pending leaves) and in its spill rows.
struct TravScratch {
  std::vector<uint32_t> lds, spill, pend;
  TravScratch() : lds(std::max(kLdsStack, kLdsStack6) + 1), spill(kSpillStack), pend(std::max(kPendLeaves, kPendLeaves6) + 1) {}
  TraversalStack stack() {
    TraversalStack st; st.lds = lds.data(); st.pend = pend.data(); st.lds_stride = 1; st.spill = spill.data(); st.spill_stride = 1;
    return st;
  }
};

// One path, following the kernel sequence of kernels.hip: raygen -> closest hit -> miss | shade -> shadow -> next bounce.  Every entry
// point that needs a sample's radiance calls this.  LOG_HITS (emu_debug_sample): hits[bounce * hit_stride .. + 2) receives the
// (instance, primitive) each bounce hits, and the closest-hit ray walks the counting instantiation of traverse<>, which is thereby held
// to the oracle's hits as well.
template <bool LOG_HITS>
vec3 emu_path(const Emu* e, uint32_t x, uint32_t y, uint32_t sample, TravScratch& scratch, int32_t* hits = nullptr, size_t hit_stride = 0) {
  const DeviceScene& S = e->S;
  const uint32_t B = S.max_bounces;
  RayGenOut rg = stage_raygen(S, x, y, sample);
  vec3 o = rg.o, d = rg.d, att = v3(1.0f), L = v3(0.0f);
  float lastPdf = 0.0f; bool lastSpec = false; uint32_t dim = rg.dim;
  for (uint32_t b = 0; b < B; b++) {
    TraversalStack st = scratch.stack();
    TraversalCount tc;
    const float ir = S.has_alpha ? Halton{halton_table(S.halton), rg.offset, dim}.sample1d() : 0.0f;
    const RayHit hit = traverse<false, LOG_HITS>(S, o, d, 1e-3f, kInf, ir, st, &tc);
    if (LOG_HITS && hits && hit.tri != kInvalidRef) triangle_ids(S, hit.tri, &hits[b * hit_stride], &hits[b * hit_stride + 1]);
    if (hit.tri == kInvalidRef) {
      if (S.env_texture >= 0) L = L + stage_miss(S, d, att, b, lastPdf, lastSpec);
      L = L + att * 0.0f;  // attenuation * backgroundColor (kernel.metal:311 / :541): NaN for a throughput that is not finite
      break;
    }
    const vec4 qO{o.x, o.y, o.z, lastPdf}, qD{d.x, d.y, d.z, 0.0f};  // the queue entry the stage may re-read
    ShadeIn in; in.o = o; in.d = d; in.att = att; in.rayO = &qO; in.rayD = &qD; in.lastSpecular = lastSpec; in.offset = rg.offset;
    in.dim = dim + 1; in.bounce = b; in.t = hit.t; in.u = hit.u; in.v = hit.v; in.tri = hit.tri;
    const ShadeOut out = stage_shade(S, in);
    if (out.has_emitted) L = L + out.emitted;
    if (out.shadow) {
      const RayHit sh = traverse<true, false>(S, out.shadow_o, out.shadow_d, 1e-3f, out.shadow_tmax, out.shadow_payload, st, &tc);
      if (sh.tri == kInvalidRef) L = L + out.shadow_contrib;
    }
    if (!out.alive) break;
    o = out.next_o; d = out.next_d; att = out.next_att; lastPdf = out.next_pdf; lastSpec = out.next_specular;
    dim = out.dim & kMetaDimMask;
  }
  return L;
}

}  // namespace

extern "C" {

void* emu_create(const pt_scene_snapshot* snap, const pt_render_params* p, const void* lut_blob, uint64_t lut_size) {
  // switches of closed experiments whose code is gone: refused, so that nothing builds another tree in their name
  for (const char* gone : {"EMU_SAH_BUILD", "EMU_SAH_COLLAPSE", "EMU_WIDE_PROBE", "EMU_CULL_PROBE"})
    if (getenv(gone)) { fprintf(stderr, "emu: $%s is no longer supported (its experiment is closed and its code removed)\n", gone); return nullptr; }
  auto* e = new Emu();
  e->params = *p;
  g_emu_rcp_ulp = getenv("EMU_RCP_ULP") ? atoi(getenv("EMU_RCP_ULP")) : 0;
  const uint8_t* b = (const uint8_t*)lut_blob;
  uint32_t hdr[32]; memcpy(hdr, b + 12, sizeof(hdr));
  size_t off = 12 + 16 * 8, nf = (lut_size - off) / 4;
  e->lut.resize(nf); memcpy(e->lut.data(), b + off, nf * 4);
  std::string err;
  if (build_host_scene(snap, p, hdr[0], hdr[4], &e->hs, &err) != PT_OK) { fprintf(stderr, "emu: %s\n", err.c_str()); delete e; return nullptr; }
  for (uint32_t c = 2; (int)e->halton.size() < kHaltonDims; c++) {
    bool prime = true;
    for (uint32_t d = 2; d * d <= c; d++) if (c % d == 0) { prime = false; break; }
    if (!prime) continue;
    e->halton.push_back(make_halton_entry(c));
  }
  // flatten to world space (same sequence as lbvh.hip k_flatten): one record per leaf slot = one triangle, or with EMU_PAIRS=1 (what the
  // device build does by default) two consecutive triangles of a mesh that share an edge
  build_primitives(&e->hs, getenv("EMU_PAIRS") != nullptr);
  std::vector<TriRec> tmp; std::vector<Box3> boxes;
  for (uint32_t i = 0; i < e->hs.instances.size(); i++) {
    const InstanceInfo& in = e->hs.instances[i];
    const MeshInfo& m = e->hs.meshes[in.mesh];
    const Xform X = load_xform(in);
    for (uint32_t k = e->hs.mesh_prim_base[in.mesh]; k < e->hs.mesh_prim_base[in.mesh + 1]; k++) {
      const uint32_t t = e->hs.prim_tri[k] & ~kPrimPairBit;
      const bool pair = (e->hs.prim_tri[k] & kPrimPairBit) != 0;
      const uint32_t* idx = &e->hs.indices[3 * (size_t)(m.tri_base + t)];
      const vec3 v0 = transformPoint(ld3(e->hs.positions[m.vertex_base + idx[0]]), X);
      const vec3 v1 = transformPoint(ld3(e->hs.positions[m.vertex_base + idx[1]]), X);
      const vec3 v2 = transformPoint(ld3(e->hs.positions[m.vertex_base + idx[2]]), X);
      vec3 v3_ = v0;
      TriRec r;
      uint32_t bcode = 0;
      r._pad = 0; r.gid_b = kInvalidRef;
      r.gid_a = ((in.tri_global_base + t) << 2) | material_class(e->hs.materials[in.material_base + e->hs.slots[m.tri_base + t]]);
      if (pair) {
        for (int c = 0; c < 3; c++) {
          const uint32_t ib = idx[3 + c];
          uint32_t code = 3u;
          if (ib == idx[0]) code = 0u; else if (ib == idx[1]) code = 1u; else if (ib == idx[2]) code = 2u;
          else v3_ = transformPoint(ld3(e->hs.positions[m.vertex_base + ib]), X);
          bcode |= code << (2 * c);
        }
        r.gid_b = ((in.tri_global_base + t + 1) << 2) | material_class(e->hs.materials[in.material_base + e->hs.slots[m.tri_base + t + 1]]);
      }
      r.inst_code = i | (bcode << kSlotInstBits);
      r.q0[0] = v0.x; r.q0[1] = v0.y; r.q0[2] = v0.z; r.q1[0] = v1.x; r.q1[1] = v1.y; r.q1[2] = v1.z;
      r.q2[0] = v2.x; r.q2[1] = v2.y; r.q2[2] = v2.z; r.q3[0] = v3_.x; r.q3[1] = v3_.y; r.q3[2] = v3_.z;
      Box3 b = tri_box(r, v1, v2);
      const float* p3 = &v3_.x;
      for (int c = 0; c < 3; c++) { b.lo[c] = std::min(b.lo[c], p3[c]); b.hi[c] = std::max(b.hi[c], p3[c]); }
      tmp.push_back(r); boxes.push_back(b);
    }
  }
  std::vector<uint32_t> order(tmp.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
  uint32_t root = kInvalidRef;
  bool wide6 = false;
  std::vector<uint32_t> tri_perm;
  if (!tmp.empty()) {
    std::vector<BinNode> bin;
    if (getenv("EMU_MORTON")) {
      Box3 sb; for (int k = 0; k < 3; k++) { sb.lo[k] = 1e30f; sb.hi[k] = -1e30f; }
      for (auto& b : boxes) for (int k = 0; k < 3; k++) { sb.lo[k] = std::min(sb.lo[k], b.lo[k]); sb.hi[k] = std::max(sb.hi[k], b.hi[k]); }
      const float ext = std::max(sb.hi[0] - sb.lo[0], std::max(sb.hi[1] - sb.lo[1], sb.hi[2] - sb.lo[2]));
      const float scale = ext > 0 ? 2097152.0f / ext : 0.0f;
      std::vector<uint64_t> code(boxes.size());
      for (size_t i = 0; i < boxes.size(); i++) {
        uint64_t c = 0;
        for (int k = 0; k < 3; k++) { float q = (0.5f * (boxes[i].lo[k] + boxes[i].hi[k]) - sb.lo[k]) * scale; q = std::min(std::max(q, 0.0f), 2097151.0f); c |= expand21((uint64_t)q) << (2 - k); }
        code[i] = c;
      }
      std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return code[a] < code[b]; });
      std::vector<uint64_t> keys(order.size());
      for (size_t i = 0; i < order.size(); i++) keys[i] = code[order[i]];
      if (getenv("EMU_PLOC")) root = build_ploc(bin, order, boxes, atoi(getenv("EMU_PLOC")));
      else root = build_morton(bin, order, keys, boxes, 0, (uint32_t)tmp.size());
    } else root = build_bin(bin, order, boxes, 0, (uint32_t)tmp.size());
    if (!(root & kLeafBit) && getenv("EMU_WIDE6")) {
      e->nodes.assign(1, BvhNode{});
      e->nodes.reserve(bin.size());
      collapse6(*e, bin, order, boxes, root, 0u, tri_perm);
      root = 0u;
      wide6 = true;
    } else if (!(root & kLeafBit)) {
      e->nodes.assign(bin.size(), BvhNode{});
      collapse(*e, bin, order, boxes, root);
    }
  }
  e->tris.resize(tmp.size());
  for (size_t i = 0; i < order.size(); i++) e->tris[i] = tmp[order[wide6 ? tri_perm[i] : i]];

  DeviceScene& S = e->S;
  memset(&S, 0, sizeof(S));
  S.positions = e->hs.positions.data(); S.vdata = e->hs.vdata.data(); S.indices = e->hs.indices.data(); S.slots = e->hs.slots.data();
  S.meshes = e->hs.meshes.data(); S.instances = e->hs.instances.data(); S.materials = e->hs.materials.data();
  S.lights = e->hs.lights.data(); S.nodes = e->nodes.data(); S.tris = e->tris.data(); S.tri_count = e->hs.tri_count; S.slot_count = (uint32_t)e->tris.size();
  S.root_ref = root; S.wide6 = wide6 ? 1u : 0u; S.halton = e->halton.data();
  e->shade_recs.assign(2 * e->tris.size(), ShadeRec{});   // entry 2 * slot + half
  for (size_t i = 0; i < 2 * e->tris.size(); i++) {
    const TriRec& tr = e->tris[i >> 1];
    const uint32_t gid = (i & 1) ? tr.gid_b : tr.gid_a;
    if (gid != kInvalidRef) e->shade_recs[i] = make_shade_rec(S, tr.inst_code & kSlotInstMask, (gid >> 2) - e->hs.instances[tr.inst_code & kSlotInstMask].tri_global_base);
  }
  S.shade_recs = e->shade_recs.data();
  e->light_recs.resize(e->hs.lights.size());
  for (size_t i = 0; i < e->hs.lights.size(); i++) e->light_recs[i] = make_light_rec(S, e->hs.lights[i]);
  S.light_recs = e->light_recs.data();
  for (auto& l : e->hs.lights) e->light_cdf.push_back(l.cumulativePower);
  S.light_cdf = e->light_cdf.data();
  Lut* ls[6] = {&S.luts.E, &S.luts.Eavg, &S.luts.EMs, &S.luts.EavgMs, &S.luts.ETransIn, &S.luts.ETransOut};
  for (int i = 0; i < 6; i++) { ls[i]->w = hdr[4 * i]; ls[i]->h = hdr[4 * i + 1]; ls[i]->depth = hdr[4 * i + 2]; ls[i]->d = e->lut.data() + hdr[4 * i + 3]; }
  S.camera = e->hs.constants.camera; S.idt = e->hs.idt; S.width = p->width; S.height = p->height;
  S.lightCount = e->hs.constants.lightCount; S.totalLightPower = e->hs.constants.totalLightPower;
  S.flags = p->flags; S.integrator = p->integrator; S.max_bounces = p->max_bounces;
  S.tex_data = e->hs.tex_data.data(); S.tex_decode = e->hs.tex_decode.data(); S.textures = e->hs.textures.data(); S.tex_native = e->hs.tex_native; S.env_alias = e->hs.env_alias.data();
  S.env_texture = e->hs.env_texture; S.envLightCount = e->hs.constants.envLightCount; S.has_alpha = e->hs.has_alpha ? 1u : 0u;
  return e;
}
void emu_destroy(void* h) { delete (Emu*)h; }
void emu_get_constants(void* h, pt_constants* out) { *out = ((Emu*)h)->hs.constants; }
uint32_t emu_get_lights(void* h, pt_area_light* out, uint32_t cap) {
  Emu* e = (Emu*)h;
  for (uint32_t i = 0; i < std::min<uint32_t>(cap, (uint32_t)e->hs.lights.size()); i++) out[i] = e->hs.lights[i];
  return (uint32_t)e->hs.lights.size();
}

// One sample of every pixel; hits[(bounce * W * H + pixel) * 2 .. + 2) = the (instance, primitive) the path hits at that bounce, -1 where it has ended.
void emu_debug_sample(void* h, uint32_t sample, float* radiance /*W*H*4*/, int32_t* hits /*B*W*H*2 or null*/) {
  const Emu* e = (const Emu*)h;
  const uint32_t W = e->S.width, H = e->S.height, B = e->S.max_bounces, NP = W * H;
  if (hits) for (size_t i = 0; i < (size_t)B * NP * 2; i++) hits[i] = -1;
  TravScratch scratch;
  for (uint32_t y = 0; y < H; y++)
    for (uint32_t x = 0; x < W; x++) {
      const uint32_t pid = y * W + x;
      const vec3 L = emu_path<true>(e, x, y, sample, scratch, hits ? hits + 2 * (size_t)pid : nullptr, 2 * (size_t)NP);
      radiance[4 * pid] = L.x; radiance[4 * pid + 1] = L.y; radiance[4 * pid + 2] = L.z; radiance[4 * pid + 3] = 1.0f;
    }
}

// ---- the CPU leg of the benchmark: "the same __host__ __device__ kernels built for the host, all host cores" ----
// Renders samples [first, first + ns) of every pixel with the product's own stage functions (stage_raygen, traverse<> over the product's
// 6-wide node form, stage_shade, stage_miss: platinum_amd/csrc/pt_*.h compiled by g++ with -ffp-contract=off), std::thread workers taking
// 16x16 pixel tiles from one atomic cursor, and folds them into `acc` as k_accumulate does (running mean in sample order, n0 samples
// already there).  Per path it is the kernel sequence of kernels.hip (emu_path); what the host has no use for (queues, compaction, chunk
// claims) is the scheduler, not the arithmetic.  bench.py times this call only (the scene / BVH set-up is emu_create).
void emu_render(void* h, uint32_t first, uint32_t ns, float* acc /*W*H*4, running mean*/, uint32_t n0, uint32_t threads) {
  const Emu* e = (const Emu*)h;
  const uint32_t W = e->S.width, H = e->S.height, tx = (W + 15) / 16, ty = (H + 15) / 16;
  std::atomic<uint32_t> cursor{0};
  auto worker = [&]() {
    TravScratch scratch;
    for (;;) {
      const uint32_t t = cursor.fetch_add(1);
      if (t >= tx * ty) return;
      const uint32_t x0 = (t % tx) * 16, y0 = (t / tx) * 16;
      for (uint32_t y = y0; y < std::min(y0 + 16, H); y++)
        for (uint32_t x = x0; x < std::min(x0 + 16, W); x++) {
          float* a = acc + 4 * ((size_t)y * W + x);
          for (uint32_t s = 0; s < ns; s++) {
            vec3 L = emu_path<false>(e, x, y, first + s, scratch);
            const uint32_t n = n0 + s;                 // k_accumulate (kernel.metal:672-684)
            if (n > 0) { L = L + v3(a[0], a[1], a[2]) * (float)n; L = L / (float)(n + 1); }
            a[0] = L.x; a[1] = L.y; a[2] = L.z; a[3] = 1.0f;
          }
        }
    }
  };
  std::vector<std::thread> pool;
  for (uint32_t i = 1; i < std::max(1u, threads); i++) pool.emplace_back(worker);
  worker();
  for (auto& th : pool) th.join();
}

void emu_trace_primary(void* h, uint32_t sample, pt_hit_record* out) {
  Emu* e = (Emu*)h;
  const DeviceScene& S = e->S;
  TravScratch scratch;
  for (uint32_t y = 0; y < S.height; y++)
    for (uint32_t x = 0; x < S.width; x++) {
      RayGenOut rg = stage_raygen(S, x, y, sample);
      TraversalStack st = scratch.stack();
      TraversalCount tc;
      const float ir = S.has_alpha ? Halton{halton_table(S.halton), rg.offset, rg.dim}.sample1d() : 0.0f;
      RayHit hit = traverse<false, false>(S, rg.o, rg.d, 1e-3f, kInf, ir, st, &tc);
      pt_hit_record& r = out[y * S.width + x];
      if (hit.tri != kInvalidRef) { r.t = hit.t; r.u = hit.u; r.v = hit.v; triangle_ids(S, hit.tri, &r.instance, &r.primitive); }
      else { r.t = r.u = r.v = 0; r.instance = r.primitive = -1; }
    }
}
float emu_halton(void* h, uint32_t i, uint32_t d) { return halton(halton_table(((Emu*)h)->halton.data()), i, d); }

}  // extern "C"

#endif  // PTAMD_TESTS_EMU_WAVEFRONT_EMU
