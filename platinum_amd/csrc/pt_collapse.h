// pt_collapse.h — the collapse of a binary BVH to 6-wide nodes that minimises what a ray pays: the area-weighted number of wide nodes
// (Ylitie, Karras, Laine 2017, section 3.1, without its leaf merging: a leaf here is one triangle slot and stays one).  A leaf child is
// tested inside its parent whatever the collapse is, so leaves cost nothing.
//
// For every binary node n and every budget k = 1..6, bottom-up (a parent after both of its children):
//   F(n, k)     the least cost of representing n's subtree as at most k children of some wide node;  F(leaf, k) = 0
//   F(n, 1)   = area(n) + G(n, 6)                                   n becomes a wide node
//   G(n, k)   = min over i = 1..k-1 of F(left, i) + F(right, k - i)   n is opened: its k slots go to its two children
//   F(n, k)   = min(F(n, 1), G(n, k))                               k >= 2
// collapse_step is one node's row of that table and the word of its decisions; collapse_expand walks the decisions from a wide node's
// binary node down to its children.  Both are PT_HD: lbvh.hip runs them on the device (the step where PLOC creates the node, the walk in
// emit_sah_node6), tests/cpp/collapse_check.cpp on the host against an enumeration of every collapse.
//
// Ties: the smaller i wins (a strict `<` over i = 1, 2, ...), and an opened node wins over a kept one of the same cost (one node fewer), so
// the wide tree is a function of the binary tree alone.  Float addition is monotone, so the table's minimum IS the minimum over all
// collapses in the float expression the table itself evaluates: cost(kept n) = area(n) + (term(left) + term(right)), term(leaf) = 0,
// term(kept c) = cost(c), term(opened c) = term(c.left) + term(c.right).
#pragma once
#include "pt_math.h"

namespace pt {

constexpr int kCollapseWidth = 6;
constexpr uint32_t kCollapseLeafBit = 0x80000000u;  // (pt_device.h kLeafBit: a binary ref with this bit is a leaf)

// the word of one node's decisions: bits 3 (k - 2) .. + 2 = the i of G(n, k), k = 2..6; bit 15 + (k - 2) = as one of at most k children n is
// opened (G(n, k) <= F(n, 1)) rather than kept as a node
PT_HD uint32_t collapse_split(uint32_t word, int k) { return (word >> (3 * (k - 2))) & 7u; }
PT_HD bool collapse_opened(uint32_t word, int k) { return ((word >> (15 + (k - 2))) & 1u) != 0; }

// the area measure of the table and of the area rule (lbvh.hip open_by_area): half the surface area
PT_HD float collapse_half_area(const float (&lo)[3], const float (&hi)[3]) {
  const float x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
  return x * y + y * z + z * x;
}

// One node's row: fl / fr = F(left, 1..6) / F(right, 1..6) (zeros for a leaf), area = the node's own; f = F(n, 1..6).  Returns the word.
PT_HD uint32_t collapse_step(float area, const float (&fl)[kCollapseWidth], const float (&fr)[kCollapseWidth], float (&f)[kCollapseWidth]) {
  uint32_t word = 0;
  float g[kCollapseWidth + 1];
  for (int k = 2; k <= kCollapseWidth; k++) {
    float best = fl[0] + fr[k - 2];
    uint32_t bi = 1;
    for (int i = 2; i < k; i++) {
      const float c = fl[i - 1] + fr[k - i - 1];
      if (c < best) { best = c; bi = (uint32_t)i; }
    }
    g[k] = best;
    word |= bi << (3 * (k - 2));
  }
  f[0] = area + g[kCollapseWidth];
  for (int k = 2; k <= kCollapseWidth; k++) {
    const bool open = g[k] <= f[0];
    f[k - 1] = open ? g[k] : f[0];
    if (open) word |= 1u << (15 + (k - 2));
  }
  return word;
}

// The children of the wide node made of binary node `node`: node's two children share six slots as G(node, 6) says; a child that is
// internal, has a budget of two or more and is marked opened for it gives its slot to its left child and the next free slot to its right
// child (the first such child first), until none is left.  children[n] = n's two binary refs (.x, .y), words[n] = n's word.  Returns the
// number of slots used (2..6); refs[] are binary refs in no particular order.
template <class Pair>
PT_HD int collapse_expand(uint32_t node, const Pair* children, const uint32_t* words, uint32_t (&refs)[kCollapseWidth]) {
  uint32_t budget[kCollapseWidth];
  for (int k = 0; k < kCollapseWidth; k++) { refs[k] = kCollapseLeafBit; budget[k] = 1; }
  {
    const Pair ch = children[node];
    const uint32_t i = collapse_split(words[node], kCollapseWidth);
    refs[0] = ch.x; budget[0] = i;
    refs[1] = ch.y; budget[1] = (uint32_t)kCollapseWidth - i;
  }
  int count = 2;
  for (int round = 0; round < kCollapseWidth - 2; round++) {
    // the first slot that opens (compare-selects over the six slots: an array indexed at run time would sit in scratch on the device)
    int at = -1;
    uint32_t ref = 0, b = 0, word = 0;
    for (int k = kCollapseWidth - 1; k >= 0; k--) {
      if (k < count && !(refs[k] & kCollapseLeafBit) && budget[k] >= 2) {
        const uint32_t w = words[refs[k]];
        if (collapse_opened(w, (int)budget[k])) { at = k; ref = refs[k]; b = budget[k]; word = w; }
      }
    }
    if (at < 0) break;
    const Pair ch = children[ref];
    const uint32_t i = collapse_split(word, (int)b);
    for (int k = 0; k < kCollapseWidth; k++) {
      if (k == at) { refs[k] = ch.x; budget[k] = i; }
      if (k == count) { refs[k] = ch.y; budget[k] = b - i; }
    }
    count++;
  }
  return count;
}

}  // namespace pt
