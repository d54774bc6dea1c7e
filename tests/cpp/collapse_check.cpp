// TEST HARNESS ONLY — the least-cost 6-wide collapse (platinum_amd/csrc/pt_collapse.h: the very functions lbvh.hip runs on the device) on the
// host, against an enumeration of EVERY collapse of small binary trees.  tests/test_collapse_host.py compiles and runs it, once more under
// -fsanitize=address,undefined.  Exit status 0 and a last line "collapse_check ok: <cases> trees" when everything holds.
//
// Per tree (2..12 leaves; random shapes, chains, balanced trees; random, equal, zero-area and nested boxes):
//   * F(root, 1) of the table equals, bit for bit, the minimum over all collapses: every subset of the internal nodes that contains the root
//     is a collapse (its members become wide nodes) when no wide node gets more than six children; its cost is evaluated in the float expression
//     the table uses (pt_collapse.h, head comment);
//   * the tree collapse_expand makes of the table's decisions is valid (every leaf exactly once; 2..6 children per node) and costs F(root, 1);
//   * it costs no more than the tree the area rule makes (the rule of lbvh.hip's open_by_area, written out again here);
//   * a second run gives the same words and the same tree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../platinum_amd/csrc/pt_collapse.h"

namespace {

struct Pair { uint32_t x, y; };
struct BoxF { float lo[3], hi[3]; };
constexpr uint32_t kLeaf = pt::kCollapseLeafBit;

struct Tree {
  int leaves = 0;
  std::vector<Pair> children;   // internal node -> two binary refs; children before parents, the root is the last one (as PLOC numbers them)
  std::vector<BoxF> leaf_box, node_box;
  std::vector<float> area;      // per internal node
};

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }
float rndf() { return (float)(rnd() >> 8) * (1.0f / 16777216.0f); }

BoxF box_of(const Tree& t, uint32_t ref) { return (ref & kLeaf) ? t.leaf_box[ref & ~kLeaf] : t.node_box[ref]; }

// shape 0: random merges of random clusters; 1: a chain; 2: balanced (adjacent pairs, level by level)
// boxes 0: random; 1: every leaf the same box (equal areas everywhere); 2: zero-area boxes (points and segments); 3: nested (areas over decades)
Tree make_tree(int leaves, int shape, int boxes) {
  Tree t;
  t.leaves = leaves;
  for (int i = 0; i < leaves; i++) {
    BoxF b;
    for (int a = 0; a < 3; a++) {
      if (boxes == 1) { b.lo[a] = 0.25f; b.hi[a] = 0.75f; }
      else if (boxes == 2) { b.lo[a] = (i & 1) && a == 0 ? rndf() : 0.5f; b.hi[a] = b.lo[a]; }
      else if (boxes == 3) { const float s = 1.0f / (float)(1u << (2 * i)); b.lo[a] = -s; b.hi[a] = s * (1.0f + rndf()); }
      else { const float c = rndf(), e = rndf() * 0.2f; b.lo[a] = c - e; b.hi[a] = c + e; }
    }
    t.leaf_box.push_back(b);
  }
  std::vector<uint32_t> cl;
  for (int i = 0; i < leaves; i++) cl.push_back(kLeaf | (uint32_t)i);
  auto merge = [&](size_t i, size_t j) {   // i < j: the merged cluster takes i's place
    const BoxF x = box_of(t, cl[i]), y = box_of(t, cl[j]);
    BoxF m;
    for (int a = 0; a < 3; a++) { m.lo[a] = x.lo[a] < y.lo[a] ? x.lo[a] : y.lo[a]; m.hi[a] = x.hi[a] > y.hi[a] ? x.hi[a] : y.hi[a]; }
    t.children.push_back(Pair{cl[i], cl[j]});
    t.node_box.push_back(m);
    t.area.push_back(pt::collapse_half_area(m.lo, m.hi));
    cl[i] = (uint32_t)t.children.size() - 1u;
    cl.erase(cl.begin() + (long)j);
  };
  while (cl.size() > 1) {
    if (shape == 1) merge(0, 1);
    else if (shape == 2) { for (size_t i = 0; i + 1 < cl.size(); i++) merge(i, i + 1); }
    else { const size_t i = rnd() % (cl.size() - 1); merge(i, i + 1 + rnd() % (cl.size() - 1 - i)); }
  }
  return t;
}

// ---- the table, as the device fills it: one step per node, children first ----
struct Table { std::vector<float> f; std::vector<uint32_t> words; };
Table fill(const Tree& t) {
  Table tb;
  const size_t n = t.children.size();
  tb.f.assign(6 * n, 0.0f);
  tb.words.assign(n, 0u);
  for (size_t i = 0; i < n; i++) {
    float fl[6], fr[6], f[6];
    const Pair ch = t.children[i];
    for (int k = 0; k < 6; k++) {
      fl[k] = (ch.x & kLeaf) ? 0.0f : tb.f[6 * ch.x + (size_t)k];
      fr[k] = (ch.y & kLeaf) ? 0.0f : tb.f[6 * ch.y + (size_t)k];
    }
    tb.words[i] = pt::collapse_step(t.area[i], fl, fr, f);
    for (int k = 0; k < 6; k++) tb.f[6 * i + (size_t)k] = f[k];
  }
  return tb;
}

// ---- every collapse: a subset `kept` of the internal nodes (bit per node) ----
float term(const Tree& t, uint32_t kept, uint32_t ref);
float cost_kept(const Tree& t, uint32_t kept, uint32_t n) { return t.area[n] + (term(t, kept, t.children[n].x) + term(t, kept, t.children[n].y)); }
float term(const Tree& t, uint32_t kept, uint32_t ref) {
  if (ref & kLeaf) return 0.0f;
  if (kept & (1u << ref)) return cost_kept(t, kept, ref);
  return term(t, kept, t.children[ref].x) + term(t, kept, t.children[ref].y);
}
int slots(const Tree& t, uint32_t kept, uint32_t ref) {   // children that `ref` contributes to the wide node above it
  if ((ref & kLeaf) || (kept & (1u << ref))) return 1;
  return slots(t, kept, t.children[ref].x) + slots(t, kept, t.children[ref].y);
}
bool feasible(const Tree& t, uint32_t kept) {
  for (uint32_t n = 0; n < t.children.size(); n++)
    if ((kept & (1u << n)) && slots(t, kept, t.children[n].x) + slots(t, kept, t.children[n].y) > 6) return false;
  return true;
}
bool brute_minimum(const Tree& t, float* out) {
  const uint32_t n = (uint32_t)t.children.size(), root = n - 1;
  bool any = false;
  float best = 0.0f;
  for (uint32_t rest = 0; rest < (1u << root); rest++) {
    const uint32_t kept = rest | (1u << root);
    if (!feasible(t, kept)) continue;
    const float c = cost_kept(t, kept, root);
    if (!any || c < best) { best = c; any = true; }
  }
  *out = best;
  return any;
}

// ---- a wide tree: per wide node its binary node and its children; cost in the same expression (kept = the nodes that are wide nodes) ----
struct Wide { std::vector<uint32_t> node; std::vector<std::vector<uint32_t>> kids; };

Wide expand_by_cost(const Tree& t, const Table& tb) {
  Wide w;
  std::vector<uint32_t> todo{(uint32_t)t.children.size() - 1u};
  while (!todo.empty()) {
    const uint32_t n = todo.back();
    todo.pop_back();
    uint32_t refs[6];
    const int count = pt::collapse_expand(n, t.children.data(), tb.words.data(), refs);
    w.node.push_back(n);
    w.kids.emplace_back(refs, refs + count);
    for (int k = 0; k < count; k++) if (!(refs[k] & kLeaf)) todo.push_back(refs[k]);
  }
  return w;
}
// lbvh.hip open_by_area<6>: the node's two children, then the internal child with the largest half area is opened (strict `>`: the first of
// equal ones), its left child in its slot, its right child in the next free one
Wide expand_by_area(const Tree& t) {
  Wide w;
  std::vector<uint32_t> todo{(uint32_t)t.children.size() - 1u};
  while (!todo.empty()) {
    const uint32_t n = todo.back();
    todo.pop_back();
    std::vector<uint32_t> refs{t.children[n].x, t.children[n].y};
    while (refs.size() < 6) {
      int best = -1;
      float best_area = -1.0f;
      for (size_t k = 0; k < refs.size(); k++)
        if (!(refs[k] & kLeaf)) { const BoxF b = box_of(t, refs[k]); const float a = pt::collapse_half_area(b.lo, b.hi); if (a > best_area) { best_area = a; best = (int)k; } }
      if (best < 0) break;
      const Pair g = t.children[refs[(size_t)best]];
      refs[(size_t)best] = g.x;
      refs.push_back(g.y);
    }
    w.node.push_back(n);
    w.kids.push_back(refs);
    for (uint32_t r : refs) if (!(r & kLeaf)) todo.push_back(r);
  }
  return w;
}
uint32_t kept_of(const Wide& w) { uint32_t kept = 0; for (uint32_t n : w.node) kept |= 1u << n; return kept; }

// the leaves under binary ref `ref`, in order
void leaves_under(const Tree& t, uint32_t ref, std::vector<uint32_t>* out) {
  if (ref & kLeaf) { out->push_back(ref & ~kLeaf); return; }
  leaves_under(t, t.children[ref].x, out);
  leaves_under(t, t.children[ref].y, out);
}

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d (%s): ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); return false; } } while (0)

bool valid(const Tree& t, const Wide& w, const char* what) {
  std::vector<int> seen((size_t)t.leaves, 0);
  uint32_t wide_nodes = 0;
  for (size_t i = 0; i < w.node.size(); i++) {
    const size_t c = w.kids[i].size();
    CHECK(c >= 1 && c <= 6, "%s: node %u has %zu children", what, w.node[i], c);
    CHECK(c >= 2 || (t.leaves == 2 && w.node.size() == 1), "%s: one child under something else than a 2-leaf root", what);
    CHECK(!(wide_nodes & (1u << w.node[i])), "%s: binary node %u is two wide nodes", what, w.node[i]);
    wide_nodes |= 1u << w.node[i];
    // the children partition the leaves of the node's binary subtree
    std::vector<uint32_t> mine, theirs;
    leaves_under(t, w.node[i], &mine);
    for (uint32_t r : w.kids[i]) {
      leaves_under(t, r, &theirs);
      if (r & kLeaf) seen[r & ~kLeaf]++;
    }
    std::vector<int> cnt((size_t)t.leaves, 0);
    for (uint32_t l : mine) cnt[l]++;
    for (uint32_t l : theirs) cnt[l]--;
    for (int l = 0; l < t.leaves; l++) CHECK(cnt[(size_t)l] == 0, "%s: node %u: leaf %d is not covered exactly once by its children", what, w.node[i], l);
  }
  for (int l = 0; l < t.leaves; l++) CHECK(seen[(size_t)l] == 1, "%s: leaf %d is a child %d times", what, l, seen[(size_t)l]);
  return true;
}

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

bool check_tree(const Tree& t, int id) {
  const uint32_t root = (uint32_t)t.children.size() - 1u;
  const Table tb = fill(t);
  const float f1 = tb.f[6 * (size_t)root];
  float brute = 0.0f;
  CHECK(brute_minimum(t, &brute), "tree %d: no feasible collapse", id);
  CHECK(same_bits(f1, brute), "tree %d (%d leaves): F(root, 1) = %.9g, the minimum over all collapses = %.9g", id, t.leaves, f1, brute);
  for (int k = 1; k < 6; k++) CHECK(tb.f[6 * (size_t)root + (size_t)k] <= tb.f[6 * (size_t)root + (size_t)k - 1], "tree %d: F(root, k) rises at k = %d", id, k + 1);
  const Wide w = expand_by_cost(t, tb);
  if (!valid(t, w, "least cost")) return false;
  CHECK(feasible(t, kept_of(w)), "tree %d: the expanded tree is not a collapse", id);
  const float c = cost_kept(t, kept_of(w), root);
  CHECK(same_bits(c, f1), "tree %d: the expanded tree costs %.9g, F(root, 1) = %.9g", id, c, f1);
  const Wide wa = expand_by_area(t);
  if (!valid(t, wa, "area rule")) return false;
  const float ca = cost_kept(t, kept_of(wa), root);
  CHECK(c <= ca, "tree %d: least cost %.9g > area rule %.9g", id, c, ca);
  // ties and reruns: the same words, the same tree
  const Table tb2 = fill(t);
  CHECK(tb2.words == tb.words && std::memcmp(tb2.f.data(), tb.f.data(), tb.f.size() * sizeof(float)) == 0, "tree %d: the table differs on a rerun", id);
  const Wide w2 = expand_by_cost(t, tb2);
  CHECK(w2.node == w.node && w2.kids == w.kids, "tree %d: the tree differs on a rerun", id);
  return true;
}

}  // namespace

int main() {
  int cases = 0;
  long better = 0;
  for (int leaves = 2; leaves <= 12; leaves++)
    for (int shape = 0; shape < 3; shape++)
      for (int boxes = 0; boxes < 4; boxes++)
        for (int rep = 0; rep < (shape == 0 ? 6 : 2); rep++) {
          const Tree t = make_tree(leaves, shape, boxes);
          if (!check_tree(t, cases)) { std::printf("  (leaves %d, shape %d, boxes %d, rep %d)\n", leaves, shape, boxes, rep); return 1; }
          const Table tb = fill(t);
          const uint32_t root = (uint32_t)t.children.size() - 1u;
          if (tb.f[6 * (size_t)root] < cost_kept(t, kept_of(expand_by_area(t)), root)) better++;
          cases++;
        }
  std::printf("collapse_check ok: %d trees (%ld strictly cheaper than the area rule's)\n", cases, better);
  return 0;
}
