// camera_lists.hip — once per pt_start_render, after the BVH build: for every pixel of a pinhole camera the 6-wide nodes whose leaf children
// the pixel's cone can touch (pt_camlist.h), sorted by the distance at which a ray can first enter them.  k_camera_primary (kernels.hip) traces
// bounce 0 of every batch of the render from these lists instead of walking the tree from the root once per sample.
//
// One wave per 8x8 tile.  The wave walks the tree with the TILE's cone, all lanes in step (lanes 0..5 test one child each, a ballot makes the
// verdict wave-uniform; the node stack is the wave's, in LDS).  At every node that has a leaf child inside the tile's cone each lane — one per
// pixel — filters those children with its own pixel's cone and, when one is left, inserts the node into its list.  The plane arithmetic is
// double: the kernel runs once per render and takes a fraction of a batch's bounce 0.
#include <hip/hip_runtime.h>

#include "camera_lists.h"
#include "kernels.h"

namespace pt {

__global__ void __launch_bounds__(kBlock) k_camera_lists(DeviceScene S, CamListEntry* __restrict__ entries, uint32_t* __restrict__ count, uint32_t cap,
                                                         uint32_t tilesX, uint32_t tiles, CamListCounters* __restrict__ out) {
  __shared__ uint32_t lds_stack[kBlock / 64][kCamStack];
  const uint32_t lane = wave_lane(), w = threadIdx.x >> 6;
  const uint32_t tile = blockIdx.x * (kBlock / 64) + w;
  if (tile >= tiles) return;   // (wave-uniform; the kernel has no barrier)
  uint32_t* stack = lds_stack[w];
  const uint32_t ty = tile / tilesX, tx = tile - ty * tilesX;
  const PixelXY q = tile_pixel(tile, lane, tilesX);
  const bool valid = q.x < S.width && q.y < S.height;
  const CamCone tile_cone = cam_tile_cone(S.camera, tx, ty);
  const CamCone pix_cone = cam_pixel_cone(S.camera, q.x, q.y);
  const BvhNode6* __restrict__ nodes = reinterpret_cast<const BvhNode6*>(S.nodes);
  CamListEntry* list = entries + (size_t)(tile * 64u + lane) * cap;
  uint32_t len = 0;          // this pixel's nodes so far (keeps counting past cap: the histogram shows what a capacity would have to hold)
  bool overflow = false;     // wave-uniform: the tile's walk ran out of stack
  uint32_t sp = 0, cur = S.root_ref;
  while (cur != kInvalidRef) {
    const BvhNode6 n = nodes[cur];
    const uint32_t n_int = n.counts & 7u, n_all = n_int + ((n.counts >> 3) & 7u);
    const bool touched = lane < n_all && !cam_box_outside(tile_cone, cam_child_box(n, lane < 6u ? lane : 0u));
    const uint32_t mask = (uint32_t)__ballot(touched) & 63u;
    const uint32_t leaves = mask >> n_int;
    uint32_t inner = mask & ((1u << n_int) - 1u);
    if (leaves && valid) {
      float dist = 0.0f;
      const uint32_t mine = cam_node_leaves(n, pix_cone, leaves, &dist);
      if (mine) {
        if (len < cap) cam_list_insert(list, len, cur << 6 | mine, dist);
        len++;
      }
    }
    while (inner) {
      const uint32_t k = (uint32_t)__builtin_ctz(inner);
      inner &= inner - 1u;
      if (sp < kCamStack) stack[sp++] = n.base_node + k; else overflow = true;
    }
    cur = sp ? stack[--sp] : kInvalidRef;
    cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur);
  }
  const bool fits = !overflow && len <= cap;
  count[tile * 64u + lane] = !valid ? 0u : fits ? len : kCamWalk;
  // the counters, one atomic per wave and value (per pixel they would queue up behind one L2 address: ~88 returning atomics per microsecond)
  const unsigned long long m_listed = __ballot(valid && fits), m_walk = __ballot(valid && !fits);
  uint32_t total = valid && fits ? len : 0u;
  for (int off = 32; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
  if (lane == 0) {
    if (m_listed) atomicAdd(&out->listed, (unsigned long long)__popcll(m_listed));
    if (m_walk) atomicAdd(&out->walk, (unsigned long long)__popcll(m_walk));
    if (total) atomicAdd(&out->entries, (unsigned long long)total);
  }
  const uint32_t bin = len < kCamHistBins - 1u ? len : kCamHistBins - 1u;
  unsigned long long left = __ballot(valid);
  while (left) {
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bin, __builtin_ctzll(left));
    const unsigned long long same = __ballot(valid && bin == b);
    if (lane == 0) atomicAdd(&out->hist[b], (uint32_t)__popcll(same));
    left &= ~same;
  }
}

void launch_camera_lists(hipStream_t s, const DeviceScene& S, CamListEntry* entries, uint32_t* count, uint32_t cap, CamListCounters* counters) {
  const uint32_t tiles = tile_count(S.width, S.height);
  hipLaunchKernelGGL(k_camera_lists, dim3((tiles + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, s, S, entries, count, cap, tiles_x(S.width), tiles,
                     counters);
}

}  // namespace pt
