// 96-B exact search-tree node ("near4x") and its slot-indexed triangle array
// ("tri4"), derived node by node from the finished near4 tree.
// Host and device code: mcpt_scene_upload converts in a loop, the device upload
// in small kernels, and both give the same bytes.
//
// A 128-B Node4Rec is 96 B of boxes, 16 B of links and 16 B of pad; k_render
// fetches it with seven 16-B gathers, the seventh for the links alone.  Here
// the links are folded into the boxes:
//  * Slot order: the internal slots first (in near4's order), then the empty
//    ones, the leaf slots last, the j-th leaf of near4's order in slot 3 - j.
//  * Slot type: the slab test is symmetric in the order of a (min, max) pair.
//    An internal slot stores its x pair as (max, min) with max > min (a box
//    flat in x gets its max moved up and its min down one float), a leaf slot
//    as (min, max), so `q[6k] > q[6k + 1]` is "slot k is internal".
//  * Empty slot: all six planes +inf.  Each axis' slab interval is then the
//    point +inf, -inf or NaN, so either some axis gives tfar = -inf < tmin
//    (fails the slab test), or every ordered axis gives tnear = +inf, which
//    exceeds every pruning limit (k_render's limit is finite: at most FLT_MAX).
//    A slab box that fails for every ray on the slab test alone does not exist
//    (the mirrored ray passes), hence the pruning half.  Only a direction
//    whose three reciprocals are all +-0 (three infinite components) leaves
//    nothing ordered; no ray has one.
//  * Child ids: nodes are renumbered so that a node's internal children have
//    consecutive ids, new id = 1 + (internal slots of all nodes with a smaller
//    near4 id) + (rank among its parent's internal slots); the root stays 0.
//    A node stores its first child's id in the low bytes of slot 0's miny,
//    maxy and minz, which are moved outward (down, up, down) to the nearest
//    float with that low byte: at most 256 floats away.  Every other internal
//    plane is exact.  Internal boxes only grow, which the candidate-set
//    argument allows; leaf boxes are copied bit for bit.
//  * A plane never moves alone on a flat axis: where an internal box is flat
//    (min == max) on an axis whose planes may move, both planes move outward,
//    at least one float.  With a +-0 direction component and the origin on
//    that plane the exact box is unconstrained on the axis (NaN, NaN); moved on
//    one side only it would fail there (NaN, +-inf), moved on both it is
//    unconstrained again (-inf, +inf).  So a 96-B slot passes whenever the
//    exact slot does, that corner included.
//  * Leaf links are implicit: the leaf in slot k of node n (new id) has its
//    64-B triangle record at tri4[4n + 3 - k], and its stack code is
//    ~(4n + 3 - k).  A node's leaves fill its 256-B block from the front.
//    The record is the DevTri of the reference triangle with the reference
//    triangle id in aux.y (k_render recomputes the minors kept there).
// Range: ids of 24 bits (at most 2^24 nodes) and planes below 2^100 in
// magnitude (moving a plane outward never reaches infinity).
#pragma once
#include <cstdint>
#include <vector>

#include "mcpt_bvh4.h"

#if defined(__HIPCC__)
#define N96_HD __host__ __device__
#else
#define N96_HD
#endif

namespace mcpt {

struct Node96 {
  float q[24];  // slot k: q[6k..6k+5], Node4Rec::q's order but for an internal slot's swapped x pair
};
static_assert(sizeof(Node96) == 96, "six 16-B loads");

constexpr int64_t kNode96MaxNodes = 1ll << 24;
constexpr float kNode96MaxPlane = 0x1p100f;

N96_HD inline uint32_t n96_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
N96_HD inline float n96_float(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
N96_HD inline bool n96_link_internal(int32_t l) { return l >= 0; }
N96_HD inline bool n96_link_leaf(int32_t l) { return l < 0 && l != kEmptySlot4; }
N96_HD inline int n96_count_internal(const Node4Rec &n) {
  int c = 0;
  for (int k = 0; k < 4; ++k) c += n96_link_internal(n.link[k]) ? 1 : 0;
  return c;
}

// The largest float <= v whose lowest byte is `byte` (v finite, |v| < kNode96MaxPlane).
// Floats in value order: k >= 0 has the bits k, k < 0 the bits 0x80000000 | -k.
N96_HD inline float n96_down(float v, uint32_t byte) {
  const uint32_t b = n96_bits(v), mag = b & 0x7FFFFFFFu;
  if (!(b >> 31)) {
    uint32_t c = (mag & ~0xFFu) | byte;
    if (c <= mag) return n96_float(c);
    if (c >= 0x100u) return n96_float(c - 0x100u);
    return n96_float(0x80000000u | byte);  // below the smallest positive candidate: -byte denormal steps (or -0)
  }
  uint32_t c = (mag & ~0xFFu) | byte;
  if (c < mag) c += 0x100u;
  return n96_float(0x80000000u | c);
}
N96_HD inline float n96_up(float v, uint32_t byte) { return -n96_down(-v, byte); }  // negation keeps the low byte
N96_HD inline float n96_next_up(float v) {
  const uint32_t b = n96_bits(v), mag = b & 0x7FFFFFFFu;
  if (mag == 0) return n96_float(1u);
  return n96_float((b >> 31) ? b - 1u : b + 1u);
}
N96_HD inline float n96_next_down(float v) { return -n96_next_up(-v); }

// Decode (what k_render's T step does with v_perm_b32 and selects).
N96_HD inline bool n96_slot_internal(const float *q, int k) { return q[6 * k] > q[6 * k + 1]; }
N96_HD inline int32_t n96_first_child(const float *q) {
  return (int32_t)((n96_bits(q[2]) & 0xFFu) | ((n96_bits(q[3]) & 0xFFu) << 8) | ((n96_bits(q[4]) & 0xFFu) << 16));
}
// the stack code of slot k of node n: a child's id, or ~(its tri4 index)
N96_HD inline int32_t n96_link(const float *q, int32_t n, int k) {
  return (n96_slot_internal(q, k) ? n96_first_child(q) : ~(4 * n + 3)) + k;
}

// Converts near4 node `in`, whose new id is self and whose internal children
// get the new ids first_child, first_child + 1, ... in slot order.  out: the
// 96-B node; leaf_tri[j]: the reference triangle of tri4[4 * self + j], or -1.
N96_HD inline void n96_convert(const Node4Rec &in, int32_t first_child, Node96 &out, int32_t leaf_tri[4]) {
  const float inf = __builtin_inff();
  for (int i = 0; i < 24; ++i) out.q[i] = inf;
  for (int j = 0; j < 4; ++j) leaf_tri[j] = -1;
  int ni = 0, nl = 0;
  for (int k = 0; k < 4; ++k) {
    const float *b = in.q + 6 * k;
    if (n96_link_internal(in.link[k])) {
      float *o = out.q + 6 * ni++;
      const bool flat = !(b[1] > b[0]);  // (max, min), strictly ordered: a flat axis moves out on both sides
      o[0] = flat ? n96_next_up(b[1]) : b[1];
      o[1] = flat ? n96_next_down(b[0]) : b[0];
      for (int i = 2; i < 6; ++i) o[i] = b[i];
    } else if (n96_link_leaf(in.link[k])) {
      float *o = out.q + 6 * (3 - nl);
      for (int i = 0; i < 6; ++i) o[i] = b[i];
      leaf_tri[nl++] = ~in.link[k];
    }
  }
  if (ni > 0) {
    const uint32_t id = (uint32_t)first_child;
    float *o = out.q;
    if (!(o[3] > o[2])) o[2] = n96_next_down(o[2]), o[3] = n96_next_up(o[3]);  // flat in y, in z: both sides move
    if (!(o[5] > o[4])) o[4] = n96_next_down(o[4]), o[5] = n96_next_up(o[5]);
    o[2] = n96_down(o[2], id & 0xFFu);
    o[3] = n96_up(o[3], (id >> 8) & 0xFFu);
    o[4] = n96_down(o[4], (id >> 16) & 0xFFu);
  }
}

// New ids: first[p] = 1 + the internal slots of all nodes before p (n96_first,
// a prefix sum); node p gives its internal children first[p], first[p] + 1, ...
// in slot order; the root keeps 0.  Returns false when the counts do not add
// up to a tree of cnt.size() nodes.
inline bool n96_first(const std::vector<int32_t> &cnt, std::vector<int32_t> &first) {
  first.resize(cnt.size());
  int64_t run = 1;
  for (size_t p = 0; p < cnt.size(); ++p) first[p] = (int32_t)run, run += cnt[p];
  return run == (int64_t)cnt.size();
}
N96_HD inline void n96_assign_ids(const Node4Rec *near4, int32_t p, int32_t n, const int32_t *first, int32_t *newid) {
  if (p == 0) newid[0] = 0;
  int r = 0;
  for (int k = 0; k < 4; ++k) {
    const int32_t l = near4[p].link[k];
    if (n96_link_internal(l) && l < n) newid[l] = first[p] + r++;
  }
}

// A relabelled copy of a reference-tree node (nodes4): leaf links become
// ~(tri4 index), so the fallback search reaches the same triangle array.
N96_HD inline void n96_relabel(const Node4Rec &in, const int32_t *tri4_of, Node4Rec &out) {
  out = in;
  for (int k = 0; k < 4; ++k)
    if (n96_link_leaf(in.link[k])) out.link[k] = ~tri4_of[~in.link[k]];
}

}  // namespace mcpt
