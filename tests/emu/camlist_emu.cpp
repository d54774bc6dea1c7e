// TEST HARNESS ONLY (tests/emu) — the host side of the camera-ray leaf lists (platinum_amd/csrc/pt_camlist.h) for tests/test_camera_lists_host.py:
// builds the lists of every pixel as camera_lists.hip does (a tile's cone walks the tree, each pixel's cone filters the leaf children), then
// holds them to the scalar walk ray by ray.  Its own library (tests/_build/libptamd_camlist.so, host_build.load(src, lib)); it includes the
// first part of the harness for the host scene and tree.  Not part of libptamd.so, never loaded by platinum_amd, not a fallback.
#include "wavefront_emu.cpp"

#include "../../platinum_amd/csrc/pt_camlist.h"

namespace {

struct HostLists {
  uint32_t cap = 0, W = 0, H = 0;
  std::vector<CamListEntry> entries;   // [pixel slot][cap]
  std::vector<uint32_t> count;         // [pixel slot]
  std::vector<uint32_t> length;        // [pixel slot] before the capacity is applied
};

// camera_lists.hip k_camera_lists, one tile at a time
void build_lists(const DeviceScene& S, uint32_t cap, HostLists* L) {
  const uint32_t tilesX = tiles_x(S.width), tiles = tile_count(S.width, S.height);
  L->cap = cap; L->W = S.width; L->H = S.height;
  L->entries.assign((size_t)tiles * 64 * cap, CamListEntry{0u, 0.0f});
  L->count.assign((size_t)tiles * 64, 0u);
  L->length.assign((size_t)tiles * 64, 0u);
  const BvhNode6* nodes = reinterpret_cast<const BvhNode6*>(S.nodes);
  std::vector<uint32_t> stack;
  for (uint32_t tile = 0; tile < tiles; tile++) {
    const uint32_t ty = tile / tilesX, tx = tile - ty * tilesX;
    const CamCone tile_cone = cam_tile_cone(S.camera, tx, ty);
    CamCone pix[64];
    bool valid[64];
    for (uint32_t lane = 0; lane < 64; lane++) {
      const PixelXY q = tile_pixel(tile, lane, tilesX);
      valid[lane] = q.x < S.width && q.y < S.height;
      pix[lane] = cam_pixel_cone(S.camera, q.x, q.y);
    }
    stack.assign(1, S.root_ref);
    while (!stack.empty()) {
      const uint32_t cur = stack.back();
      stack.pop_back();
      const BvhNode6& n = nodes[cur];
      const uint32_t n_int = n.counts & 7u, n_all = n_int + ((n.counts >> 3) & 7u);
      uint32_t mask = 0;
      for (uint32_t k = 0; k < n_all; k++) if (!cam_box_outside(tile_cone, cam_child_box(n, k))) mask |= 1u << k;
      const uint32_t leaves = mask >> n_int;
      if (leaves)
        for (uint32_t lane = 0; lane < 64; lane++) {
          if (!valid[lane]) continue;
          float dist = 0.0f;
          const uint32_t mine = cam_node_leaves(n, pix[lane], leaves, &dist);
          if (!mine) continue;
          const size_t slot = (size_t)tile * 64 + lane;
          if (L->length[slot] < cap) cam_list_insert(&L->entries[slot * cap], L->length[slot], cur << 6 | mine, dist);
          L->length[slot]++;
        }
      for (uint32_t k = 0; k < n_int; k++) if ((mask >> k) & 1u) stack.push_back(n.base_node + k);
    }
    for (uint32_t lane = 0; lane < 64; lane++) {
      const size_t slot = (size_t)tile * 64 + lane;
      L->count[slot] = !valid[lane] ? 0u : L->length[slot] <= cap ? L->length[slot] : kCamWalk;
    }
  }
}

// stage_raygen's pinhole ray through (px + jx, py + jy)
void camera_ray(const DeviceScene& S, uint32_t px, uint32_t py, float jx, float jy, vec3* o, vec3* d) {
  const pt_camera_data& cam = S.camera;
  const float fx = (float)px + jx, fy = (float)py + jy;
  *o = ld3(cam.position);
  *d = normalize(((ld3(cam.topLeft) + fx * ld3(cam.pixelDeltaU)) + fy * ld3(cam.pixelDeltaV)) - *o);
}

}  // namespace

extern "C" {

// Builds the lists with `cap` entries per pixel and, for every pixel and every jitter (jit[2 * j], jit[2 * j + 1]), holds the list to the walk:
//   out[0] pixels, out[1] pixels flagged kCamWalk, out[2] entries of all lists, out[3] longest list (before the capacity),
//   out[4] rays traced, out[5] leaf-queue entries the walks made, out[6] of them NOT contained in the pixel's list (node and mask bits),
//   out[7] rays whose list trace differs from the walk in a bit of (tri, t, u, v), out[8] rays that hit something,
//   out[9] pixels whose slot is not tile_of_pixel * 64 + lane_of_pixel or whose pixel_of_pid does not lead back to them (at 1, 46 and 64 samples)
// Rays of flagged pixels are skipped (counted in out[1] only).  Returns 0, or -1 when the scene is not a 6-wide tree with a pinhole camera.
int cl_check(void* h, uint32_t cap, const float* jit, uint32_t njit, uint64_t* out) {
  const Emu* e = (const Emu*)h;
  const DeviceScene& S = e->S;
  for (int k = 0; k < 10; k++) out[k] = 0;
  if (!S.wide6 || S.root_ref == kInvalidRef || (S.root_ref & kLeafBit) || S.camera.apertureRadius > 0.0f) return -1;
  HostLists L;
  build_lists(S, cap, &L);
  TravScratch scratch;
  for (uint32_t y = 0; y < S.height; y++)
    for (uint32_t x = 0; x < S.width; x++) {
      const uint32_t slot = tile_of_pixel(x, y, S.width) * 64u + lane_of_pixel(x, y);
      out[0]++;
      for (uint32_t ns : {1u, 46u, 64u})
        for (uint32_t s : {0u, ns - 1u}) {
          const uint32_t pid = lbuf_index(tile_of_pixel(x, y, S.width), s, ns, lane_of_pixel(x, y));
          if (pixel_slot_of_pid(pid, ns) != slot || pixel_of_pid(pid, ns, S.width) != y * S.width + x) { out[9]++; break; }
        }
      out[3] = std::max<uint64_t>(out[3], L.length[slot]);
      if (L.count[slot] == kCamWalk) { out[1]++; continue; }
      const CamListEntry* list = &L.entries[(size_t)slot * cap];
      const uint32_t len = L.count[slot];
      out[2] += len;
      for (uint32_t j = 0; j < njit; j++) {
        vec3 o, d;
        camera_ray(S, x, y, jit[2 * j], jit[2 * j + 1], &o, &d);
        out[4]++;
        // the scalar walk (pt_bvh.h trav_step), with every leaf-queue entry it makes looked up in the list
        TravState ts;
        RayHit walk;
        if (trav_init(S, ts, o, d, 1e-3f, kInf, 0.0f, scratch.stack(), false, nullptr)) return -1;
        while (ts.cur != kInvalidRef) {
          const uint32_t node = ts.cur;
          trav_node6<false>(S.nodes, ts, nullptr);
          if (ts.st.npend > 0) {
            const uint32_t mask = ts.st.pend[0] & 63u;
            out[5]++;
            bool found = false;
            for (uint32_t i = 0; i < len; i++) if ((list[i].ref >> 6) == node) found = (mask & ~(list[i].ref & 63u)) == 0u;
            if (!found) out[6]++;
          }
          while (ts.st.npend > 0) (void)trav_pending_leaf6<false, false>(S, ts, nullptr);
        }
        walk = ts.best;
        // the list trace
        TravState tl;
        if (trav_init(S, tl, o, d, 1e-3f, kInf, 0.0f, scratch.stack(), false, nullptr)) return -1;
        cam_trace_list(S, tl, list, len);
        const RayHit& a = tl.best;
        if (a.tri != walk.tri || f2u(a.t) != f2u(walk.t) || f2u(a.u) != f2u(walk.u) || f2u(a.v) != f2u(walk.v)) out[7]++;
        if (walk.tri != kInvalidRef) out[8]++;
      }
    }
  return 0;
}

// ---- the cone test on its own: a box against the cone of pixel (px, py) / of the tile that holds it --------------------------------------------
int cl_pixel_box_outside(const pt_camera_data* cam, uint32_t px, uint32_t py, const double* lo, const double* hi) {
  DBox b;
  for (int a = 0; a < 3; a++) { b.lo[a] = lo[a]; b.hi[a] = hi[a]; }
  return cam_box_outside(cam_pixel_cone(*cam, px, py), b) ? 1 : 0;
}
int cl_tile_box_outside(const pt_camera_data* cam, uint32_t px, uint32_t py, const double* lo, const double* hi) {
  DBox b;
  for (int a = 0; a < 3; a++) { b.lo[a] = lo[a]; b.hi[a] = hi[a]; }
  return cam_box_outside(cam_tile_cone(*cam, px >> 3, py >> 3), b) ? 1 : 0;
}
float cl_entry_dist(const pt_camera_data* cam, const double* lo, const double* hi) {
  DBox b;
  for (int a = 0; a < 3; a++) { b.lo[a] = lo[a]; b.hi[a] = hi[a]; }
  return cam_entry_dist(cam_pixel_cone(*cam, 0, 0), b);
}
double cl_margin() { return kCamConeMargin; }
uint32_t cl_default_capacity() { return kCamListCapacity; }

}  // extern "C"

// analysis aid: every triangle the camera ray of (x, y, sample) hits (Moeller-Trumbore with tmax = inf), nearest first, up to `cap`:
// out[5 * k .. ] = t, u, v, instance, primitive.  Returns the number of hits.
extern "C" uint32_t cl_brute(void* h, uint32_t x, uint32_t y, uint32_t sample, double* out, uint32_t cap) {
  const Emu* e = (const Emu*)h;
  const DeviceScene& S = e->S;
  const RayGenOut rg = stage_raygen(S, x, y, sample);
  struct Hit { float t, u, v; uint32_t tri; };
  std::vector<Hit> hits;
  for (uint32_t s = 0; s < S.slot_count; s++) {
    const TriRec& tr = S.tris[s];
    float t, u, v;
    const vec3 v0 = v3(tr.q0[0], tr.q0[1], tr.q0[2]), v1 = v3(tr.q1[0], tr.q1[1], tr.q1[2]), v2 = v3(tr.q2[0], tr.q2[1], tr.q2[2]);
    if (intersect_triangle(rg.o, rg.d, 1e-3f, kInf, v0, v1 - v0, v2 - v0, &t, &u, &v)) hits.push_back({t, u, v, 2u * s});
    if (tr.gid_b != kInvalidRef) {
      const vec3 b0 = slot_corner(&tr, (tr.inst_code >> 26) & 3u), b1 = slot_corner(&tr, (tr.inst_code >> 28) & 3u), b2 = slot_corner(&tr, tr.inst_code >> 30);
      if (intersect_triangle(rg.o, rg.d, 1e-3f, kInf, b0, b1 - b0, b2 - b0, &t, &u, &v)) hits.push_back({t, u, v, 2u * s + 1u});
    }
  }
  std::sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) { return a.t < b.t; });
  for (uint32_t k = 0; k < hits.size() && k < cap; k++) {
    int32_t inst, prim;
    triangle_ids(S, hits[k].tri, &inst, &prim);
    out[5 * k] = hits[k].t; out[5 * k + 1] = hits[k].u; out[5 * k + 2] = hits[k].v; out[5 * k + 3] = inst; out[5 * k + 4] = prim;
  }
  return (uint32_t)hits.size();
}
