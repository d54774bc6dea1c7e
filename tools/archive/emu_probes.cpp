// ARCHIVE (tools/archive) — host probes of three experiments that DESIGN.md section 6 lists as closed by measurement: the packet probe (r3,
// profiles/r03_tcp_bound.md), the origin-sort probe (r5, profiles/r05_experiments.md) and the L2 replay (r6, profiles/r06_experiments.md).
// Each needs only a host scene (Emu) and the product's traverse<>, so they live beside the scripts that drove them and not in the test
// harness: this unit includes the harness (tests/emu/host_harness.cpp) and adds the probes' entry points; origin_sort_probe.py and
// l2_probe.py build it into tools/_build/libemu_probes.so through tests/host_build.py.  No test uses it.
#include "../../tests/emu/host_harness.cpp"

// The packet probe walks a 4-wide tree whose leaf slots hold ONE triangle (it is only run without EMU_PAIRS): triangle A of a slot
static bool probe_intersect(vec3 o, vec3 d, float tmin, float tmax, const TriRec& tr, float* t, float* u, float* v) {
  const vec3 v0 = v3(tr.q0[0], tr.q0[1], tr.q0[2]), v1 = v3(tr.q1[0], tr.q1[1], tr.q1[2]), v2 = v3(tr.q2[0], tr.q2[1], tr.q2[2]);
  return intersect_triangle(o, d, tmin, tmax, v0, v1 - v0, v2 - v0, t, u, v);
}

extern "C" {

// ---- experiment (emu_packet_probe): camera rays of one 8x8 pixel tile traced as ONE packet (a wave that walks the tree once for its 64
// rays: a node is visited when any ray's slab test passes with that ray's current best t; children ordered by the smallest entry
// distance among the rays that hit them; a leaf's triangle is tested by every ray whose slab test passed).  Counts node visits and
// triangle rounds per PACKET against the per-ray traversal's totals over the same 64 rays.  out: {packets, packet node visits, packet
// triangle rounds, per-ray node visits (sum), per-ray triangle tests (sum), mismatching hits}
void emu_packet_probe(void* h, uint32_t sample, double out[6]) {
  Emu* e = (Emu*)h;
  const DeviceScene& S = e->S;
  TravScratch scratch;
  double packets = 0, pn = 0, pt_ = 0, rn = 0, rt = 0, mism = 0;
  const uint32_t tilesX = tiles_x(S.width);
  for (uint32_t ty = 0; ty < tiles_y(S.height); ty++)
    for (uint32_t tx = 0; tx < tilesX; tx++) {
      struct R { vec3 o, d, inv; RayHit best; bool on; } r[64];
      int n = 0;
      for (uint32_t l = 0; l < 64; l++) {
        const PixelXY p = tile_pixel(ty * tilesX + tx, l, tilesX);
        const uint32_t x = p.x, y = p.y;
        if (x >= S.width || y >= S.height) continue;
        const RayGenOut rg = stage_raygen(S, x, y, sample);
        R& q = r[n++];
        q.o = rg.o; q.d = rg.d; q.inv = v3(1.0f / rg.d.x, 1.0f / rg.d.y, 1.0f / rg.d.z); q.on = true;
        q.best.t = kInf; q.best.u = q.best.v = 0; q.best.tri = kInvalidRef; q.best.gid = kInvalidRef;
        TraversalStack st = scratch.stack();
        TraversalCount tc;
        const RayHit ref = traverse<false, true>(S, rg.o, rg.d, 1e-3f, kInf, 0.0f, st, &tc);
        rn += tc.nodes; rt += tc.tris;
        q.best.gid = ref.tri;  // (stash the per-ray answer for the comparison below)
      }
      if (n == 0 || S.root_ref == kInvalidRef || (S.root_ref & kLeafBit)) continue;
      uint32_t want[64];
      for (int k = 0; k < n; k++) { want[k] = r[k].best.gid; r[k].best.gid = kInvalidRef; }
      packets++;
      std::vector<uint32_t> stack;
      uint32_t cur = S.root_ref;
      for (;;) {
        const BvhNode nd = S.nodes[cur];
        pn++;
        float tmin_child[4] = {kInf, kInf, kInf, kInf};
        bool any[4] = {false, false, false, false};
        bool hitk[64][4];
        for (int k = 0; k < n; k++) {
          const R& q = r[k];
          for (int c = 0; c < 4; c++) {
            hitk[k][c] = false;
            if (nd.ref[c] == kInvalidRef) continue;
            float lo[3], hi[3];
            for (int a = 0; a < 3; a++) {
              lo[a] = nd.origin[a] + (float)((nd.qlo[a] >> (8 * c)) & 0xffu) * node_scale(nd.exp[a]);
              hi[a] = nd.origin[a] + (float)((nd.qhi[a] >> (8 * c)) & 0xffu) * node_scale(nd.exp[a]);
            }
            const float tn = slab_entry(lo, hi, q.o, q.inv, 1e-3f, q.best.t * kCullSlack);
            if (tn < 0.0f) continue;
            hitk[k][c] = true; any[c] = true; tmin_child[c] = fminf(tmin_child[c], tn);
          }
        }
        // leaves: one triangle round per hit leaf child (all rays whose slab test passed take part)
        for (int c = 0; c < 4; c++) {
          if (!any[c] || !(nd.ref[c] & kLeafBit)) continue;
          pt_++;
          const uint32_t ti = nd.ref[c] & ~kLeafBit;
          const TriRec& tr = S.tris[ti];
          for (int k = 0; k < n; k++) {
            if (!hitk[k][c]) continue;
            R& q = r[k];
            float t, u, v;
            if (probe_intersect(q.o, q.d, 1e-3f, q.best.t, tr, &t, &u, &v) && (t < q.best.t || q.best.tri == kInvalidRef || tr.gid_a < q.best.gid)) {
              q.best.t = t; q.best.u = u; q.best.v = v; q.best.tri = 2 * ti; q.best.gid = tr.gid_a;
            }
          }
        }
        std::pair<float, uint32_t> inner[4]; int ni = 0;
        for (int c = 0; c < 4; c++) if (any[c] && !(nd.ref[c] & kLeafBit)) inner[ni++] = {tmin_child[c], nd.ref[c]};
        std::stable_sort(inner, inner + ni, [](const std::pair<float, uint32_t>& a, const std::pair<float, uint32_t>& b) { return a.first < b.first; });
        for (int k = ni - 1; k >= 1; k--) stack.push_back(inner[k].second);
        if (ni > 0) { cur = inner[0].second; continue; }
        if (stack.empty()) break;
        cur = stack.back(); stack.pop_back();
      }
      for (int k = 0; k < n; k++) if (r[k].best.tri != want[k]) mism++;
    }
  out[0] = packets; out[1] = pn; out[2] = pt_; out[3] = rn; out[4] = rt; out[5] = mism;
}
// ---- experiment (emu_origin_sort_probe, r5): would sorting a segment's SECONDARY rays by the cell of their origin make its 64-ray chunks touch
// fewer distinct lines?  The rays entering bounce `b` of ONE 8x8 tile under `ns` samples (a segment of the wavefront) are cut into 64-ray chunks
// (a) in the order the stage leaves them (pixel-major, sample-minor, survivors compacted) and (b) sorted by the Morton code of their origin in a
// 32^3 grid over the origins' bounds; per chunk: the number of DISTINCT 64-byte lines (6-wide nodes + leaf slots) its rays fetch, against the
// sum over its rays.  out: {rays, chunks, lines summed over rays, distinct per chunk summed (arrival order), the same (sorted)}.  6-wide trees only.
static void trace_lines(const DeviceScene& S, vec3 o, vec3 d, TravScratch& scratch, std::vector<uint32_t>* lines) {
  TraversalStack st = scratch.stack();
  TravState ts;
  if (trav_init(S, ts, o, d, 1e-3f, kInf, 0.0f, st, false, nullptr)) return;
  while (!(ts.cur == kInvalidRef && ts.st.npend == 0)) {
    if (ts.cur != kInvalidRef && ts.st.npend <= kPendLeaves6 - 1) { lines->push_back(ts.cur); trav_node6<false>(S.nodes, ts, nullptr); }
    while (ts.st.npend > 0) {
      const uint32_t e = ts.st.pend[(ts.st.npend - 1) * ts.st.lds_stride];
      lines->push_back(0x80000000u | ((e >> 6) + (uint32_t)__builtin_ctz(e & 63u)));
      trav_pending_leaf6<false, false>(S, ts, nullptr);
    }
  }
}
void emu_origin_sort_probe(void* h, uint32_t tile_x, uint32_t tile_y, uint32_t ns, uint32_t bounce, double out[5]) {
  Emu* e = (Emu*)h;
  const DeviceScene& S = e->S;
  for (int i = 0; i < 5; i++) out[i] = 0;
  if (!S.wide6) return;
  TravScratch scratch;
  struct R { vec3 o, d; };
  std::vector<R> rays;
  for (uint32_t pl = 0; pl < 64; pl++)
    for (uint32_t smp = 0; smp < ns; smp++) {
      const uint32_t tilesX = tiles_x(S.width);
      const PixelXY p = tile_pixel(tile_y * tilesX + tile_x, pl, tilesX);
      const uint32_t x = p.x, y = p.y;
      if (x >= S.width || y >= S.height) continue;
      RayGenOut rg = stage_raygen(S, x, y, smp);
      vec3 o = rg.o, d = rg.d, att = v3(1.0f);
      float lastPdf = 0.0f; bool lastSpec = false; uint32_t dim = rg.dim;
      bool alive = true;
      for (uint32_t b = 0; b < bounce && alive; b++) {
        TraversalStack st = scratch.stack();
        const RayHit hit = traverse<false, false>(S, o, d, 1e-3f, kInf, 0.0f, st, nullptr);
        if (hit.tri == kInvalidRef) { alive = false; break; }
        const vec4 qO{o.x, o.y, o.z, lastPdf}, qD{d.x, d.y, d.z, 0.0f};
        ShadeIn in; in.o = o; in.d = d; in.att = att; in.rayO = &qO; in.rayD = &qD; in.lastSpecular = lastSpec; in.offset = rg.offset;
        in.dim = dim + 1; in.bounce = b; in.t = hit.t; in.u = hit.u; in.v = hit.v; in.tri = hit.tri;
        const ShadeOut so = stage_shade(S, in);
        if (!so.alive) { alive = false; break; }
        o = so.next_o; d = so.next_d; att = so.next_att; lastPdf = so.next_pdf; lastSpec = so.next_specular; dim = so.dim & kMetaDimMask;
      }
      if (alive) rays.push_back({o, d});
    }
  if (rays.empty()) return;
  std::vector<std::vector<uint32_t>> lines(rays.size());
  double total = 0;
  for (size_t i = 0; i < rays.size(); i++) { trace_lines(S, rays[i].o, rays[i].d, scratch, &lines[i]); total += (double)lines[i].size(); }
  auto distinct = [&](const std::vector<uint32_t>& order) {
    double sum = 0;
    for (size_t c = 0; c < order.size(); c += 64) {
      std::vector<uint32_t> u;
      for (size_t k = c; k < std::min(order.size(), c + 64); k++) u.insert(u.end(), lines[order[k]].begin(), lines[order[k]].end());
      std::sort(u.begin(), u.end());
      sum += (double)(std::unique(u.begin(), u.end()) - u.begin());
    }
    return sum;
  };
  std::vector<uint32_t> order(rays.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
  const double arrival = distinct(order);
  vec3 lo = rays[0].o, hi = rays[0].o;
  for (auto& r : rays) { lo = v3(fminf(lo.x, r.o.x), fminf(lo.y, r.o.y), fminf(lo.z, r.o.z)); hi = v3(fmaxf(hi.x, r.o.x), fmaxf(hi.y, r.o.y), fmaxf(hi.z, r.o.z)); }
  const float ext = fmaxf(fmaxf(hi.x - lo.x, hi.y - lo.y), fmaxf(hi.z - lo.z, 1e-20f));
  std::vector<uint64_t> key(rays.size());
  for (size_t i = 0; i < rays.size(); i++) {
    const uint64_t cx = (uint64_t)fminf(31.0f, (rays[i].o.x - lo.x) / ext * 32.0f), cy = (uint64_t)fminf(31.0f, (rays[i].o.y - lo.y) / ext * 32.0f),
                   cz = (uint64_t)fminf(31.0f, (rays[i].o.z - lo.z) / ext * 32.0f);
    key[i] = expand21(cx) << 2 | expand21(cy) << 1 | expand21(cz);
  }
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  const double sorted = distinct(order);
  out[0] = (double)rays.size(); out[1] = (double)((rays.size() + 63) / 64); out[2] = total; out[3] = arrival; out[4] = sorted;
}
// ---- experiment (emu_l2_probe, r6): would SCENE-SPACE ray queues keep the closest-hit kernel's BVH lines inside the XCDs' L2s?
// The rays entering bounce `bounce` of a window of the image (tiles [s0, s0 + T) of each of the 4 segment bands, `ns` samples: what the chunk
// tables list consecutively today) are traced on the product's 6-wide tree with every 64-byte line (node or leaf slot) they fetch recorded, then
// REPLAYED through a model of the chip's eight L2s — 4 MB each, 64-byte lines (the counters' miss = one 64-byte fetch: 116 B / 1.93 per ray,
// profiles/r05_pmc_c3.json), 16-way LRU — fed by 768 resident waves per XCD (32 CUs x 4 SIMDs x 6 waves), every wave stepping its 64 rays one
// line per tick, all waves of the chip round-robin, chunks claimed 8 at a time:
//   mode 0  today: ONE cursor over the chunk list in segment order (whichever wave asks next gets the run: XCDs interleave)
//   mode 1  rays sorted by the Morton cell of their ORIGIN (10 bits per axis over the origins' bounds), cut into 8 contiguous ranges, one per
//           XCD, each XCD's waves claiming from their own cursor — the scheduler DESIGN section 7 names
//   mode 2  the sorted list behind ONE cursor (what the sort alone buys, without the partition)
// At bounce 1 the window's ray density per cell equals the full frame's (origins = the window's own primary hits); at bounce >= 2 origins
// scatter and the window's density is LOWER than the full frame's: modes 1 / 2 are then pessimistic (emu_l2_probe_dense covers that case).
// out[mode][6] = {rays counted (chunks claimed after the first fifth of the list), BVH line touches, BVH misses, queue lines streamed,
//                wave-steps, wave-steps in which at least one lane missed (a wave-step waits for its slowest lane)}
struct ProbeRay { float o[3]; uint32_t first, count; };
struct L2Sim {
  static constexpr uint32_t kWays = 16;
  uint32_t sets;
  std::vector<uint32_t> tag, stamp;
  uint32_t clock = 1;
  explicit L2Sim(uint32_t bytes) : sets(bytes / 64u / kWays), tag((size_t)sets * kWays, 0xffffffffu), stamp((size_t)sets * kWays, 0u) {}
  bool touch(uint32_t line) {   // true = hit
    const uint32_t s = (line * 2654435761u >> 7) % sets;   // (the hardware hashes addresses over channels / sets; a plain modulo would alias the two arrays)
    uint32_t* t = &tag[(size_t)s * kWays]; uint32_t* st = &stamp[(size_t)s * kWays];
    uint32_t victim = 0;
    for (uint32_t w = 0; w < kWays; w++) {
      if (t[w] == line) { st[w] = clock++; return true; }
      if (st[w] < st[victim]) victim = w;
    }
    t[victim] = line; st[victim] = clock++;
    return false;
  }
};
static void gen_tile_rays(const Emu* e, uint32_t tile_x, uint32_t tile_y, uint32_t ns, uint32_t bounce, std::vector<ProbeRay>* rays, std::vector<uint32_t>* lines,
                          TravScratch& scratch) {
  const DeviceScene& S = e->S;
  std::vector<uint32_t> tmp;
  for (uint32_t pl = 0; pl < 64; pl++)
    for (uint32_t smp = 0; smp < ns; smp++) {
      const uint32_t tilesX = tiles_x(S.width);
      const PixelXY p = tile_pixel(tile_y * tilesX + tile_x, pl, tilesX);
      const uint32_t x = p.x, y = p.y;
      if (x >= S.width || y >= S.height) continue;
      RayGenOut rg = stage_raygen(S, x, y, smp);
      vec3 o = rg.o, d = rg.d, att = v3(1.0f);
      float lastPdf = 0.0f; bool lastSpec = false; uint32_t dim = rg.dim;
      bool alive = true;
      for (uint32_t b = 0; b < bounce && alive; b++) {
        TraversalStack st = scratch.stack();
        const RayHit hit = traverse<false, false>(S, o, d, 1e-3f, kInf, 0.0f, st, nullptr);
        if (hit.tri == kInvalidRef) { alive = false; break; }
        const vec4 qO{o.x, o.y, o.z, lastPdf}, qD{d.x, d.y, d.z, 0.0f};
        ShadeIn in; in.o = o; in.d = d; in.att = att; in.rayO = &qO; in.rayD = &qD; in.lastSpecular = lastSpec; in.offset = rg.offset;
        in.dim = dim + 1; in.bounce = b; in.t = hit.t; in.u = hit.u; in.v = hit.v; in.tri = hit.tri;
        const ShadeOut so = stage_shade(S, in);
        if (!so.alive) { alive = false; break; }
        o = so.next_o; d = so.next_d; att = so.next_att; lastPdf = so.next_pdf; lastSpec = so.next_specular; dim = so.dim & kMetaDimMask;
      }
      if (!alive) continue;
      tmp.clear();
      trace_lines(S, o, d, scratch, &tmp);
      ProbeRay r; r.o[0] = o.x; r.o[1] = o.y; r.o[2] = o.z; r.first = (uint32_t)lines->size(); r.count = (uint32_t)tmp.size();
      for (uint32_t l : tmp) lines->push_back((l & 0x80000000u) ? S.node_count + (l & 0x7fffffffu) : l);   // one 64-byte line address space: nodes, then slots
      rays->push_back(r);
    }
}
struct ChunkRef { uint32_t first, count; };   // rays order[first .. first + count)
static void l2_replay(const std::vector<ProbeRay>& rays, const std::vector<uint32_t>& lines, const std::vector<uint32_t>& order,
                      const std::vector<std::vector<ChunkRef>>& queues /* 1 (shared) or 8 (one per XCD) */, uint32_t waves_per_xcd, uint32_t l2_bytes,
                      uint32_t line_space, double out[6]) {
  struct Wave { uint32_t next_c = 0, end_c = 0, first = 0, count = 0, step = 0, maxlen = 0; bool active = false, counted = false; };
  std::vector<L2Sim> l2; for (int x = 0; x < 8; x++) l2.emplace_back(l2_bytes);
  std::vector<std::vector<Wave>> waves(8, std::vector<Wave>(waves_per_xcd));
  std::vector<uint32_t> cursor(queues.size(), 0);
  uint32_t stream_line = line_space;   // queue entries: lines nobody has seen before
  double n_rays = 0, touches = 0, misses = 0, streamed = 0, wave_steps = 0, wave_steps_missing = 0;
  bool any = true;
  while (any) {
    any = false;
    for (uint32_t w = 0; w < waves_per_xcd; w++)
      for (int x = 0; x < 8; x++) {
        Wave& wv = waves[x][w];
        const size_t q = queues.size() == 1 ? 0 : (size_t)x;
        if (!wv.active) {
          if (wv.next_c == wv.end_c) {
            if (cursor[q] >= queues[q].size()) continue;
            wv.next_c = cursor[q]; cursor[q] += 8; wv.end_c = std::min<uint32_t>(cursor[q], (uint32_t)queues[q].size());
          }
          const ChunkRef c = queues[q][wv.next_c];
          wv.counted = wv.next_c * 5u >= queues[q].size();
          wv.next_c++;
          wv.first = c.first; wv.count = c.count; wv.step = 0; wv.maxlen = 0; wv.active = true;
          for (uint32_t k = 0; k < c.count; k++) wv.maxlen = std::max(wv.maxlen, rays[order[c.first + k]].count);
          // the chunk's rays: rayO + rayD = 32 B each = 32 lines per 64 rays, streamed in (misses by construction); hit records (16 lines) are written
          for (uint32_t k = 0; k < (c.count * 32u + 63u) / 64u + (c.count * 16u + 63u) / 64u; k++) (void)l2[x].touch(stream_line++);
          if (wv.counted) { n_rays += c.count; streamed += (c.count * 48.0) / 64.0; }
        }
        bool step_missed = false;
        for (uint32_t k = 0; k < wv.count; k++) {
          const ProbeRay& r = rays[order[wv.first + k]];
          if (wv.step < r.count) {
            const bool hit = l2[x].touch(lines[r.first + wv.step]);
            if (wv.counted) { touches += 1; misses += hit ? 0 : 1; }
            step_missed |= !hit;
          }
        }
        if (wv.counted) { wave_steps += 1; wave_steps_missing += step_missed ? 1 : 0; }   // a wave-step waits for its slowest lane
        wv.step++;
        if (wv.step >= wv.maxlen) wv.active = false;
        any = true;
      }
  }
  out[0] = n_rays; out[1] = touches; out[2] = misses; out[3] = streamed; out[4] = wave_steps; out[5] = wave_steps_missing;
}
static void l2_three_modes(const std::vector<ProbeRay>& rays, const std::vector<uint32_t>& lines, const std::vector<uint32_t>& arrival_order,
                           const std::vector<uint32_t>& seg_end /* arrival_order positions where a segment ends */, uint32_t line_space,
                           uint32_t waves_per_xcd, uint32_t l2_bytes, uint32_t cell_bits, double out[18]) {
  auto cut = [](uint32_t first, uint32_t end, std::vector<ChunkRef>* q) { for (uint32_t c = first; c < end; c += 64) q->push_back({c, std::min(64u, end - c)}); };
  // mode 0: segment order, chunks never straddle segments
  {
    std::vector<std::vector<ChunkRef>> q(1);
    uint32_t at = 0;
    for (uint32_t e_ : seg_end) { cut(at, e_, &q[0]); at = e_; }
    l2_replay(rays, lines, arrival_order, q, waves_per_xcd, l2_bytes, line_space, &out[0]);
  }
  // origin cells
  float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
  for (auto& r : rays) for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], r.o[a]); hi[a] = fmaxf(hi[a], r.o[a]); }
  const float ext = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), fmaxf(hi[2] - lo[2], 1e-20f));
  const float cells = (float)(1u << cell_bits);
  std::vector<uint64_t> key(rays.size());
  for (size_t i = 0; i < rays.size(); i++) {
    uint64_t c[3];
    for (int a = 0; a < 3; a++) c[a] = (uint64_t)fminf(cells - 1.0f, (rays[i].o[a] - lo[a]) / ext * cells);
    key[i] = expand21(c[0]) << 2 | expand21(c[1]) << 1 | expand21(c[2]);
  }
  std::vector<uint32_t> sorted(arrival_order);
  std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  {
    std::vector<std::vector<ChunkRef>> q(8);
    const uint32_t n = (uint32_t)sorted.size();
    for (uint32_t x = 0; x < 8; x++) cut((uint32_t)((uint64_t)n * x / 8), (uint32_t)((uint64_t)n * (x + 1) / 8), &q[x]);
    l2_replay(rays, lines, sorted, q, waves_per_xcd, l2_bytes, line_space, &out[6]);
  }
  {
    std::vector<std::vector<ChunkRef>> q(1);
    cut(0, (uint32_t)sorted.size(), &q[0]);
    l2_replay(rays, lines, sorted, q, waves_per_xcd, l2_bytes, line_space, &out[12]);
  }
}
void emu_l2_probe(void* h, uint32_t bounce, uint32_t ns, uint32_t s0, uint32_t T, uint32_t waves_per_xcd, uint32_t l2_bytes, uint32_t cell_bits,
                  uint32_t threads, double out[18]) {
  Emu* e = (Emu*)h;
  const DeviceScene& S = e->S;
  for (int i = 0; i < 18; i++) out[i] = 0;
  if (!S.wide6) return;
  const uint32_t tilesX = tiles_x(S.width), tiles = tile_count(S.width, S.height), per_band = tiles / 4;
  // today's table order: segment sg = 4 * idx + band  ->  tile band * per_band + idx (pt_layout.h segment_first_tile)
  std::vector<uint32_t> seg_tile;
  for (uint32_t idx = s0; idx < s0 + T && idx < per_band; idx++) for (uint32_t band = 0; band < 4; band++) seg_tile.push_back(band * per_band + idx);
  std::vector<std::vector<ProbeRay>> tr(seg_tile.size());
  std::vector<std::vector<uint32_t>> tl(seg_tile.size());
  std::atomic<uint32_t> cursor{0};
  auto worker = [&]() {
    TravScratch scratch;
    for (;;) {
      const uint32_t i = cursor.fetch_add(1);
      if (i >= seg_tile.size()) return;
      gen_tile_rays(e, seg_tile[i] % tilesX, seg_tile[i] / tilesX, ns, bounce, &tr[i], &tl[i], scratch);
    }
  };
  { std::vector<std::thread> pool; for (uint32_t i = 1; i < std::max(1u, threads); i++) pool.emplace_back(worker); worker(); for (auto& t : pool) t.join(); }
  std::vector<ProbeRay> rays; std::vector<uint32_t> lines, order, seg_end;
  for (size_t i = 0; i < seg_tile.size(); i++) {
    const uint32_t base = (uint32_t)lines.size();
    for (auto r : tr[i]) { r.first += base; order.push_back((uint32_t)rays.size()); rays.push_back(r); }
    lines.insert(lines.end(), tl[i].begin(), tl[i].end());
    seg_end.push_back((uint32_t)rays.size());
    std::vector<ProbeRay>().swap(tr[i]); std::vector<uint32_t>().swap(tl[i]);
  }
  if (rays.empty()) return;
  l2_three_modes(rays, lines, order, seg_end, S.node_count + S.slot_count, waves_per_xcd, l2_bytes, cell_bits, out);
}

}  // extern "C"
