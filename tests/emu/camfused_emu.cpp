// TEST HARNESS ONLY (tests/emu) — the host side of the fused bounce-0 kernel (platinum_amd/csrc/kernels.hip k_camera_primary) for
// tests/test_camera_fused_host.py: the closed form that places a camera ray in its segment (pt_layout.h camera_rays_before) against k_raygen's
// own packing loop, and the per-lane list trace the kernels share (pt_camlist.h cam_trace_ray) against cam_trace_list, ray by ray.  Its own
// library (tests/_build/libptamd_camfused.so); it includes camlist_emu.cpp for the host lists.  With -DCAMFUSED_EMU_MAIN a program of its own
// (the sanitizer build) over every slot case and a small hand-made 6-wide tree.  Not part of libptamd.so, never loaded by platinum_amd.
#include "camlist_emu.cpp"

namespace {

// k_raygen's loop over segment sg, lane by lane: out[r] = the (tile, pixel lane, sample) of the segment's entry r, in the order the ballots pack them
struct PackedRay { uint32_t tile, pl, s; };
void pack_segment(uint32_t W, uint32_t H, uint32_t nseg, uint32_t bands, uint32_t tps, uint32_t ns, uint32_t sg, std::vector<PackedRay>* out,
                  std::vector<uint32_t>* iter_start) {
  const uint32_t tilesX = tiles_x(W), tiles = tile_count(W, H);
  const uint32_t first_tile = segment_first_tile(nseg, bands, tps, sg);
  out->clear(); iter_start->clear();
  for (uint32_t k = 0; k < tps * ns; k++) {
    const uint32_t tile = first_tile + k / ns;
    iter_start->push_back((uint32_t)out->size());
    if (tile >= tiles) { for (uint32_t k2 = k + 1; k2 < tps * ns; k2++) iter_start->push_back((uint32_t)out->size()); break; }
    for (uint32_t lane = 0; lane < 64; lane++) {
      const uint32_t r = (k % ns) * 64u + lane;
      const uint32_t pl = r / ns, s = r - pl * ns;
      const PixelXY q = tile_pixel(tile, pl, tilesX);
      if (q.x < W && q.y < H) out->push_back({tile, pl, s});
    }
  }
  iter_start->push_back((uint32_t)out->size());   // [tps * ns]: the segment's count
}

}  // namespace

extern "C" {

// Every segment of a W x H image cut into nseg segments of tps tiles over `bands` bands, at ns samples: the packing loop against the closed
// form.  out[0] rays packed, out[1] iterations whose first entry differs from camera_rays_before, out[2] rays whose entry differs from
// (valid pixels before the ray's pixel in the segment) * ns + sample, out[3] segments whose count differs, out[4] segments.
int cf_slot_check(uint32_t W, uint32_t H, uint32_t nseg, uint32_t bands, uint32_t tps, uint32_t ns, uint64_t* out) {
  for (int k = 0; k < 5; k++) out[k] = 0;
  const uint32_t tilesX = tiles_x(W), tiles = tile_count(W, H);
  if (nseg % bands != 0 || (uint64_t)nseg * tps < tiles) return -1;
  std::vector<PackedRay> rays;
  std::vector<uint32_t> start;
  for (uint32_t sg = 0; sg < nseg; sg++) {
    pack_segment(W, H, nseg, bands, tps, ns, sg, &rays, &start);
    const uint32_t first_tile = segment_first_tile(nseg, bands, tps, sg);
    out[4]++;
    out[0] += rays.size();
    for (uint32_t k = 0; k <= tps * ns; k++)
      if (camera_rays_before(first_tile, k, ns, tilesX, tiles, W, H) != start[k]) out[k == tps * ns ? 3 : 1]++;
    for (uint32_t r = 0; r < rays.size(); r++) {
      const PackedRay& p = rays[r];
      uint32_t pixels = 0;
      for (uint32_t t = first_tile; t < p.tile; t++) pixels += tile_valid_w(t, tilesX, W) * tile_valid_h(t, tilesX, H);
      pixels += tile_pixels_before(p.pl, tile_valid_w(p.tile, tilesX, W), tile_valid_h(p.tile, tilesX, H));
      if (pixels * ns + p.s != r) out[2]++;
    }
  }
  return 0;
}

// cam_trace_ray against cam_trace_list on the lists of every pixel (capacity `cap`), for every jitter: out[0] rays traced, out[1] rays whose
// (tri, gid, t, u, v) differ in a bit, out[2] rays that hit something, out[3] pixels flagged kCamWalk (their rays are skipped).
int cf_trace_check_scene(const DeviceScene& S, uint32_t cap, const float* jit, uint32_t njit, uint64_t* out) {
  for (int k = 0; k < 4; k++) out[k] = 0;
  if (!S.wide6 || S.root_ref == kInvalidRef || (S.root_ref & kLeafBit) || S.camera.apertureRadius > 0.0f) return -1;
  HostLists L;
  build_lists(S, cap, &L);
  const BvhNode6* nodes = reinterpret_cast<const BvhNode6*>(S.nodes);
  TravScratch scratch;
  for (uint32_t y = 0; y < S.height; y++)
    for (uint32_t x = 0; x < S.width; x++) {
      const uint32_t slot = tile_of_pixel(x, y, S.width) * 64u + lane_of_pixel(x, y);
      if (L.count[slot] == kCamWalk) { out[3]++; continue; }
      const CamListEntry* list = &L.entries[(size_t)slot * cap];
      const uint32_t len = L.count[slot];
      for (uint32_t j = 0; j < njit; j++) {
        vec3 o, d;
        camera_ray(S, x, y, jit[2 * j], jit[2 * j + 1], &o, &d);
        TravState ta, tb;
        if (trav_init(S, ta, o, d, 1e-3f, kInf, 0.0f, scratch.stack(), false, nullptr)) return -1;
        cam_trace_list(S, ta, list, len);
        if (trav_init(S, tb, o, d, 1e-3f, kInf, 0.0f, scratch.stack(), false, nullptr)) return -1;
        cam_trace_ray(S, tb, nodes, list, len);
        const RayHit &a = ta.best, &b = tb.best;
        out[0]++;
        if (a.tri != b.tri || (a.tri != kInvalidRef && a.gid != b.gid) || f2u(a.t) != f2u(b.t) || f2u(a.u) != f2u(b.u) || f2u(a.v) != f2u(b.v)) out[1]++;
        if (a.tri != kInvalidRef) out[2]++;
      }
    }
  return 0;
}
int cf_trace_check(void* h, uint32_t cap, const float* jit, uint32_t njit, uint64_t* out) {
  return cf_trace_check_scene(((const Emu*)h)->S, cap, jit, njit, out);
}

}  // extern "C"

#ifdef CAMFUSED_EMU_MAIN
// 16 triangles under a root with two internal and four leaf children: quads at several depths in front of a pinhole camera
int main() {
  uint64_t out[5];
  uint64_t cases = 0, rays = 0;
  for (uint32_t tps : {1u, 4u})
    for (uint32_t ns : {1u, 46u, 64u, 130u})
      for (uint32_t vw = 1; vw <= 8; vw++)
        for (uint32_t vh = 1; vh <= 8; vh++) {
          const uint32_t W = 16 + vw, H = 8 + vh, tiles = tile_count(W, H), nseg = (tiles + tps - 1) / tps;
          if (cf_slot_check(W, H, nseg, 1, tps, ns, out) != 0 || out[1] || out[2] || out[3]) { printf("slot check failed: %u x %u tps %u ns %u\n", W, H, tps, ns); return 1; }
          cases++; rays += out[0];
        }
  printf("slots: %llu cases, %llu rays\n", (unsigned long long)cases, (unsigned long long)rays);

  std::vector<TriRec> tris(16);
  std::vector<Box3> boxes(16);
  for (uint32_t i = 0; i < 16; i++) {
    const float x0 = -2.0f + (float)(i & 3u), y0 = -2.0f + (float)(i >> 2), z = -4.0f - 0.5f * (float)((i * 7u) % 5u);
    TriRec r{};
    r.q0[0] = x0; r.q0[1] = y0; r.q0[2] = z; r.q1[0] = x0 + 1.5f; r.q1[1] = y0; r.q1[2] = z - 0.25f; r.q2[0] = x0; r.q2[1] = y0 + 1.5f; r.q2[2] = z + 0.25f;
    r.q3[0] = x0; r.q3[1] = y0; r.q3[2] = z;
    r.gid_a = i << 2; r.gid_b = kInvalidRef; r.inst_code = 0; r._pad = 0;
    tris[i] = r;
    boxes[i] = tri_box(r, v3(r.q1[0], r.q1[1], r.q1[2]), v3(r.q2[0], r.q2[1], r.q2[2]));
  }
  auto unite = [&](uint32_t a, uint32_t n) {
    Box3 u = boxes[a];
    for (uint32_t i = a + 1; i < a + n; i++) for (int c = 0; c < 3; c++) { u.lo[c] = std::min(u.lo[c], boxes[i].lo[c]); u.hi[c] = std::max(u.hi[c], boxes[i].hi[c]); }
    return u;
  };
  std::vector<BvhNode> nodes(3);
  Box3 root_children[6] = {unite(4, 6), unite(10, 6), boxes[0], boxes[1], boxes[2], boxes[3]};
  const BvhNode6 n0 = quantize_node6(root_children, 2, 4, 1u, 0u), n1 = quantize_node6(&boxes[4], 0, 6, 0u, 4u), n2 = quantize_node6(&boxes[10], 0, 6, 0u, 10u);
  static_assert(sizeof(BvhNode6) == sizeof(BvhNode), "node records share one array");
  memcpy(&nodes[0], &n0, sizeof(n0)); memcpy(&nodes[1], &n1, sizeof(n1)); memcpy(&nodes[2], &n2, sizeof(n2));
  InstanceInfo inst{};
  DeviceScene S;
  memset(&S, 0, sizeof(S));
  S.nodes = nodes.data(); S.tris = tris.data(); S.slot_count = 16; S.tri_count = 16; S.root_ref = 0u; S.wide6 = 1u; S.instances = &inst;
  S.width = 37; S.height = 21;
  S.camera.position = {0.0f, 0.0f, 2.0f, 0.0f};
  S.camera.topLeft = {-1.0f, 0.6f, 1.0f, 0.0f};
  S.camera.pixelDeltaU = {2.0f / 37.0f, 0.0f, 0.0f, 0.0f};
  S.camera.pixelDeltaV = {0.0f, -1.2f / 21.0f, 0.0f, 0.0f};
  const float jit[] = {0.0f, 0.0f, 0.99999994f, 0.99999994f, 0.5f, 0.5f, 0.125f, 0.875f, 0.75f, 0.25f};
  for (uint32_t cap : {128u, 1u}) {
    if (cf_trace_check_scene(S, cap, jit, 5, out) != 0 || out[1] != 0) { printf("trace check failed at capacity %u: %llu mismatches\n", cap, (unsigned long long)out[1]); return 1; }
    printf("trace: capacity %u, %llu rays, %llu hits, %llu mismatches, %llu pixels left to the walk\n", cap, (unsigned long long)out[0], (unsigned long long)out[2],
           (unsigned long long)out[1], (unsigned long long)out[3]);
    if (cap == 128u && (out[2] == 0 || out[3] != 0)) { printf("the hand-made scene is not hit\n"); return 1; }
  }
  return 0;
}
#endif
