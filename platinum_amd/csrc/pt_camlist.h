// pt_camlist.h — the geometry behind the per-pixel leaf lists of a pinhole camera (camera_lists.hip builds them once per render, k_camera_primary
// in kernels.hip traces bounce 0 from them).  Plain functions (PT_HD, no HIP types): the same code for hipcc and for the g++ build
// under tests/emu, which proves the conservative part by test (tests/test_camera_lists_host.py).
//
// All camera rays of a pixel leave one point (camera.position) and pass through that pixel's square on the image plane: they lie in a four-sided
// cone.  A list names every 6-wide node that has a leaf child whose dequantised box that cone can touch, with the mask of those children and a
// lower bound of the distance at which any ray of the pixel can enter them.  Nothing is decided per ray here: at bounce 0 every ray still runs
// its own slab test (node6_slabs, pt_bvh.h) and its own triangle tests against the children the list names.
#pragma once
#include "pt_bvh.h"

namespace pt {

// A pixel's cone reaches `m` pixels beyond its square on every side.  stage_raygen forms fx = (float)px + jitter with jitter in [0, 1), which can
// round up to px + 1 exactly, and its direction carries a few ulp (1e-7) of rounding; the per-ray slab test admits rays that pass a box at a
// distance of up to kSlabSlack - 1 = 1e-6 of t.  Seen from the apex both are angles of ~1e-6 rad; 1/16 pixel of a 1920-wide 60-degree view is 3e-5 rad
// and grows as the image shrinks: five orders of magnitude above the rounding, 30x above the slab slack.
constexpr double kCamConeMargin = 1.0 / 16.0;
constexpr uint32_t kCamWalk = 0xffffffffu;    // a pixel's count when its list did not fit: its camera rays are traced by the ordinary traversal
constexpr uint32_t kCamListCapacity = 128;    // entries per pixel (8 bytes each; only the entries in use are ever touched): DESIGN.md §4 has the length histograms behind it
constexpr uint32_t kCamListMaxCapacity = 128;
// How far beyond the best hit so far the list trace still tests a listed leaf child.  The lists are sorted by distance, so a ray finds a near hit
// at once and meets every later candidate with a tight far limit — the order in which the kCullSlack margin (pt_bvh.h) is most exposed: at
// grazing incidence on a shared edge fp32 Moeller-Trumbore reports a t up to ~1e-3 t before the ray enters that triangle's box (measured: one
// camera ray of 4e8 on C5, 89 degrees on a column, two hits 1.3e-6 t apart; the walk had met the nearer one first, the list trace culled it
// behind the other).  The list trace has no subtree to save by culling, only the candidates between 1.0001 and 1.01 best.t: it culls at 1 %.
constexpr float kCamCullSlack = 1.01f;
constexpr uint32_t kCamStack = 160;           // node stack of the build's tile walk (per wave); a tile that overflows it is flagged kCamWalk
constexpr uint32_t kCamHistBins = PT_CAMLIST_HIST_BINS;   // list lengths 0 .. 63, and "64 or more" (pt_camera_list_stats)

struct CamListEntry { uint32_t ref; float dist; };   // ref = node << 6 | mask of its leaf children inside the pixel's cone; dist = entry_dist of their union
static_assert(sizeof(CamListEntry) == 8, "CamListEntry");

// What the trace kernel reads: per pixel slot q = tile * 64 + lane (pt_layout.h pixel_slot_of_pid) a count and `cap` entries sorted by rising dist.
struct CameraLists { const CamListEntry* entries; const uint32_t* count; uint32_t cap; };

struct CamCone { double apex[3]; double n[4][3]; };   // four planes through the apex, normals pointing INTO the cone
struct DBox { double lo[3], hi[3]; };

// the cone of the image-plane rectangle [x0, x1] x [y0, y1] (pixel units, top-left origin)
PT_HD CamCone cam_cone(const pt_camera_data& cam, double x0, double y0, double x1, double y1) {
  CamCone c;
  const double p[3] = {cam.position.x, cam.position.y, cam.position.z}, tl[3] = {cam.topLeft.x, cam.topLeft.y, cam.topLeft.z};
  const double du[3] = {cam.pixelDeltaU.x, cam.pixelDeltaU.y, cam.pixelDeltaU.z}, dv[3] = {cam.pixelDeltaV.x, cam.pixelDeltaV.y, cam.pixelDeltaV.z};
  const double xs[4] = {x0, x1, x1, x0}, ys[4] = {y0, y0, y1, y1};
  double d[4][3], mid[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < 4; i++)
    for (int a = 0; a < 3; a++) { d[i][a] = (tl[a] + xs[i] * du[a] + ys[i] * dv[a]) - p[a]; mid[a] += d[i][a]; }
  for (int a = 0; a < 3; a++) c.apex[a] = p[a];
  for (int i = 0; i < 4; i++) {
    const double* u = d[i]; const double* v = d[(i + 1) & 3];
    double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const double s = n[0] * mid[0] + n[1] * mid[1] + n[2] * mid[2];   // whichever way the image plane is wound, the middle direction is inside
    for (int a = 0; a < 3; a++) c.n[i][a] = s < 0.0 ? -n[a] : n[a];
  }
  return c;
}
PT_HD CamCone cam_pixel_cone(const pt_camera_data& cam, uint32_t px, uint32_t py) {
  return cam_cone(cam, (double)px - kCamConeMargin, (double)py - kCamConeMargin, (double)px + 1.0 + kCamConeMargin, (double)py + 1.0 + kCamConeMargin);
}
// the cone of the 8x8 tile whose first pixel is (tx * 8, ty * 8): it contains the cones of its 64 pixels
PT_HD CamCone cam_tile_cone(const pt_camera_data& cam, uint32_t tx, uint32_t ty) {
  return cam_cone(cam, (double)(tx * 8u) - kCamConeMargin, (double)(ty * 8u) - kCamConeMargin, (double)(tx * 8u) + 8.0 + kCamConeMargin,
                  (double)(ty * 8u) + 8.0 + kCamConeMargin);
}

// The ONLY rejection: a box is outside iff for some plane its corner furthest along the inward normal is still outside.  (A box behind the
// apex is outside every plane; one that holds the apex is outside none.)
PT_HD bool cam_box_outside(const CamCone& c, const DBox& b) {
  for (int i = 0; i < 4; i++) {
    double s = 0.0;
    for (int a = 0; a < 3; a++) {
      const double l = c.n[i][a] * (b.lo[a] - c.apex[a]), h = c.n[i][a] * (b.hi[a] - c.apex[a]);
      s += l > h ? l : h;
    }
    if (s < 0.0) return true;
  }
  return false;
}

// child k's box as the builder quantised it: origin + q * scale in fp32 (quantize_node6 checks this very expression against the exact box)
PT_HD DBox cam_child_box(const BvhNode6& n, uint32_t k) {
  DBox b;
  for (int a = 0; a < 3; a++) {
    const uint32_t ql = k < 4u ? (n.q[a][0] >> (8u * k)) & 0xffu : (n.q[a][2] >> (8u * (k - 4u))) & 0xffu;
    const uint32_t qh = k < 4u ? (n.q[a][1] >> (8u * k)) & 0xffu : (n.q[a][2] >> (8u * (k - 4u) + 16u)) & 0xffu;
    const float s = node_scale(n.exp[a]);
    b.lo[a] = (double)(n.origin[a] + (float)ql * s);
    b.hi[a] = (double)(n.origin[a] + (float)qh * s);
  }
  return b;
}
PT_HD void cam_box_union(DBox& u, const DBox& b) {
  for (int a = 0; a < 3; a++) { u.lo[a] = b.lo[a] < u.lo[a] ? b.lo[a] : u.lo[a]; u.hi[a] = b.hi[a] > u.hi[a] ? b.hi[a] : u.hi[a]; }
}
// Euclidean distance from the apex to the box, times (1 - 1e-6): the rays are normalised, so no ray of the cone enters the box at a smaller t
PT_HD float cam_entry_dist(const CamCone& c, const DBox& b) {
  double s = 0.0;
  for (int a = 0; a < 3; a++) {
    const double d = c.apex[a] < b.lo[a] ? b.lo[a] - c.apex[a] : (c.apex[a] > b.hi[a] ? c.apex[a] - b.hi[a] : 0.0);
    s += d * d;
  }
  return (float)(sqrt(s) * (1.0 - 1e-6));
}

// The leaf children of node `n` (bit r = leaf child r, i.e. child n_int + r) among `candidates` that the cone can touch, and the entry
// distance of their union.  Returns the mask; 0: the node is not on this cone's list.
PT_HD uint32_t cam_node_leaves(const BvhNode6& n, const CamCone& c, uint32_t candidates, float* dist) {
  const uint32_t n_int = n.counts & 7u;
  uint32_t mask = 0;
  DBox u;
  for (int a = 0; a < 3; a++) { u.lo[a] = 1e300; u.hi[a] = -1e300; }
  for (uint32_t r = 0; r < 6u; r++) {
    if (!((candidates >> r) & 1u)) continue;
    const DBox b = cam_child_box(n, n_int + r);
    if (cam_box_outside(c, b)) continue;
    mask |= 1u << r;
    cam_box_union(u, b);
  }
  if (mask) *dist = cam_entry_dist(c, u);
  return mask;
}

// Keeps a pixel's list sorted by rising dist: puts (ref, dist) into the `len` entries of `list` (room for one more).  Entries of equal distance
// keep the order they arrived in; the answer does not depend on it.
PT_HD void cam_list_insert(CamListEntry* list, uint32_t len, uint32_t ref, float dist) {
  uint32_t j = len;
  while (j > 0u && list[j - 1u].dist > dist) { list[j] = list[j - 1u]; j--; }
  list[j] = CamListEntry{ref, dist};
}

// Bounce 0 of one ray from its pixel's list: what k_camera_primary runs per lane, and what tests/emu compares with the walk.  ts comes from
// trav_init.  For each entry in order: stop when its dist lies beyond best.t * kCamCullSlack (its slab test and every later one's would fail); else
// slab-test the node's leaf children with the walk's own arithmetic and run trav_leaf on those that pass and that the list names.
PT_HD void cam_trace_list(const DeviceScene& S, TravState& ts, const CamListEntry* list, uint32_t len) {
  const BvhNode6* nodes = reinterpret_cast<const BvhNode6*>(S.nodes);
  for (uint32_t i = 0; i < len; i++) {
    const CamListEntry e = list[i];
    if (e.dist > ts.best.t * kCamCullSlack) break;
    const BvhNode6 n = nodes[e.ref >> 6];
    uint32_t m = node6_leaf_hits(n, ts, ts.best.t * kCamCullSlack) & e.ref & 63u;
    while (m) {
      const uint32_t r = (uint32_t)__builtin_ctz(m);
      m &= m - 1u;
      bool fin = false;
      trav_leaf(S, ts, kLeafBit | (n.base_leaf + r), false, &fin, nullptr);
    }
  }
}


// cam_trace_list as the kernel runs it per lane (k_camera_primary where the lanes of a wave iteration belong to more than
// one pixel): the same entries, children and triangles in the same order, as ONE loop whose step is either "next entry" or "next triangle".
// The addresses do not depend on the traversal: entry i + 1 is loaded one step ahead, and its node is fetched as soon as entry i's slab
// tests are done with the node registers — it arrives while entry i's triangles are tested.  (Holding two whole nodes cost 62 spilled
// registers at 8 waves per SIMD.)  tests/emu holds it to cam_trace_list ray by ray.
PT_HD void cam_trace_ray(const DeviceScene& S, TravState& ts, const BvhNode6* __restrict__ nodes, const CamListEntry* __restrict__ list, uint32_t len) {
  const CamListEntry none{0u, kInf};
  CamListEntry e = len ? list[0] : none;
  uint32_t i = 0, m = 0, base_leaf = 0;   // m: the leaf children of the current entry still to be tested
  for (;;) {
    if (m == 0u) {
      if (i >= len || e.dist > ts.best.t * kCamCullSlack) break;
      const BvhNode6 n = nodes[e.ref >> 6];
      m = node6_leaf_hits(n, ts, ts.best.t * kCamCullSlack) & e.ref & 63u;
      base_leaf = n.base_leaf;
      i++;
      e = i < len ? list[i] : none;
    } else {
      const uint32_t r = (uint32_t)__builtin_ctz(m);
      m &= m - 1u;
      bool fin = false;
      trav_leaf(S, ts, kLeafBit | (base_leaf + r), false, &fin, nullptr);
    }
  }
}

}  // namespace pt
