// CPU check of the SAH search tree's optimisation (montecarlopathtracing_amd/csrc/mcpt_sah.cpp:
// subtree reinsertion, then the collapse under a stack-need cap), built and run by
// tests/test_sah_optimize.py.
//   sah_optimize_check gen <n_leaves> <seed> <clustered 0|1>     sah_check.cpp's generator
//   sah_optimize_check obj <dir/> <file.obj>                      the reference's leaves of a scene
//   sah_optimize_check sim <dir/> <file.obj> px py pz lx ly lz fov paths
// gen / obj print "ok ..." with the figures of both trees and an FNV-1a hash of the plain tree's bytes,
// or the first violated invariant.  sim prints node steps and triangle tests per segment of both trees
// (tools/top_pop_sim.cpp's estimator: uniform hemisphere bounces, Moller-Trumbore; not a parity tool).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mcpt_hip.h"
#include "mcpt_bvh4.h"

using mcpt::LeafRef;
using mcpt::Node4Rec;

static int fail(const char *what, long a, long b) {
  std::printf("FAIL %s %ld %ld\n", what, a, b);
  return 1;
}

static std::vector<LeafRef> generate(int n, unsigned seed, bool clustered) {  // as tests/native/sah_check.cpp
  std::mt19937 g(seed);
  std::uniform_real_distribution<float> u(-50.0f, 50.0f), e(0.0f, 0.5f);
  std::vector<LeafRef> L(n);
  for (int i = 0; i < n; ++i) {
    float c[3] = {u(g), u(g), u(g)};
    if (clustered && i % 3 == 0) c[0] = c[1] = c[2] = 1.0f;  // identical centroids: no SAH split
    for (int a = 0; a < 3; ++a) {
      L[i].box[2 * a] = c[a] - e(g);
      L[i].box[2 * a + 1] = c[a] + e(g);
    }
    if (i % 5 == 1) L[i].box[2 * (i % 3)] = L[i].box[2 * (i % 3) + 1];  // flat on one axis
    if (i % 11 == 2) L[i].box[2 * (i % 3)] = 0.0f, L[i].box[2 * (i % 3) + 1] = std::max(0.0f, L[i].box[2 * (i % 3) + 1]);
    if (i % 13 == 3) L[i].box[2 * (i % 3) + 1] = 0.0f, L[i].box[2 * (i % 3)] = std::min(0.0f, L[i].box[2 * (i % 3)]);
    L[i].tri = (int)(((long)i * 7919) % n);  // a permutation (n is not a multiple of 7919)
  }
  return L;
}

static int load(const char *dir, const char *file, std::vector<mcpt_triangle> &T, std::vector<LeafRef> &L) {
  int64_t n = 0;
  int32_t nm = 0;
  if (mcpt_load_obj(dir, file, nullptr, nullptr, &n, nullptr, &nm)) return 1;
  T.resize(n);
  std::vector<int32_t> mid(n);
  std::vector<mcpt_material> M(nm);
  if (mcpt_load_obj(dir, file, T.data(), mid.data(), &n, M.data(), &nm)) return 1;
  mcpt_pack_triangles(T.data(), mid.data(), n);
  std::vector<mcpt_bvh_node> B(2 * n - 1);
  mcpt_build_hlbvh(T.data(), n, B.data());
  for (auto &b : B)
    if (b.left == b.right) {
      LeafRef r;
      const float bx[6] = {b.bbmin[0], b.bbmax[0], b.bbmin[1], b.bbmax[1], b.bbmin[2], b.bbmax[2]};
      std::memcpy(r.box, bx, sizeof bx);
      r.tri = b.left;
      L.push_back(r);
    }
  return 0;
}

// sah_check.cpp's invariants: every leaf once with its own box, every slot box the exact union of its
// child's slots, children after parents, at least two slots per node, the stack bound as reported
static int check_tree(const std::vector<LeafRef> &L, const std::vector<Node4Rec> &t, int need_reported) {
  const int n = (int)L.size();
  std::vector<int> leaf_of(n, -1);
  for (int i = 0; i < n; ++i) {
    if (L[i].tri < 0 || L[i].tri >= n || leaf_of[L[i].tri] >= 0) return fail("input: tri is no permutation", i, L[i].tri);
    leaf_of[L[i].tri] = i;
  }
  std::vector<int> seen(n, 0), visited(t.size(), 0), need(t.size(), -1);
  for (long k = (long)t.size() - 1; k >= 0; --k) {
    int ns = 0, below = 0;
    for (int s = 0; s < 4; ++s) {
      const int32_t l = t[k].link[s];
      if (l == mcpt::kEmptySlot4) continue;
      ++ns;
      if (l >= 0) {
        if (l <= k || l >= (long)t.size()) return fail("child id order", k, l);
        below = std::max(below, need[l]);
      }
    }
    if (ns < 2) return fail("node with < 2 slots", k, ns);
    need[k] = ns - 1 + below;
  }
  if (std::max(need[0], 1) != need_reported) return fail("stack need", need[0], need_reported);
  for (size_t k = 0; k < t.size(); ++k)
    for (int s = 0; s < 4; ++s) {
      const int32_t l = t[k].link[s];
      if (l == mcpt::kEmptySlot4) continue;
      const float *b = t[k].q + 6 * s;
      if (l < 0) {
        const int tri = ~l;
        if (tri < 0 || tri >= n) return fail("leaf id", (long)k, tri);
        if (seen[tri]++) return fail("leaf twice", (long)k, tri);
        if (std::memcmp(b, L[leaf_of[tri]].box, sizeof(float) * 6)) return fail("leaf box", (long)k, tri);
      } else {
        if (visited[l]++) return fail("node twice", (long)k, l);
        float un[6] = {1e30f, -1e30f, 1e30f, -1e30f, 1e30f, -1e30f};
        for (int c = 0; c < 4; ++c) {
          if (t[l].link[c] == mcpt::kEmptySlot4) continue;
          for (int a = 0; a < 3; ++a) {
            un[2 * a] = std::min(un[2 * a], t[l].q[6 * c + 2 * a]);
            un[2 * a + 1] = std::max(un[2 * a + 1], t[l].q[6 * c + 2 * a + 1]);
          }
        }
        if (std::memcmp(un, b, sizeof(un))) return fail("slot box != union of child", (long)k, l);
      }
    }
  for (int i = 0; i < n; ++i)
    if (seen[i] != 1) return fail("leaf missing", i, seen[i]);
  for (size_t k = 1; k < t.size(); ++k)
    if (visited[k] != 1) return fail("unreachable node", (long)k, visited[k]);
  return 0;
}

static unsigned long long fnv1a(const void *p, size_t n) {
  unsigned long long h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
  return h;
}
static bool same(const std::vector<Node4Rec> &a, const std::vector<Node4Rec> &b) {
  return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(Node4Rec)));
}

static int check(const std::vector<LeafRef> &L) {
  using clk = std::chrono::steady_clock;
  std::vector<Node4Rec> plain, off, on1, on8, forced;
  int need_plain = 0, need_off = 0, need1 = 0, need8 = 0, need_forced = 0;
  const auto t0 = clk::now();
  if (mcpt::build_sah4(L, plain, &need_plain, 1)) return fail("build plain", 0, 0);
  const auto t1 = clk::now();
  mcpt::SahOptimize o_off, o1, o8, o_forced;
  o_off.passes = 0;
  if (mcpt::build_sah4(L, off, &need_off, 4, &o_off)) return fail("build off", 0, 0);
  const auto t2 = clk::now();
  if (mcpt::build_sah4(L, on1, &need1, 1, &o1)) return fail("build on", 0, 0);
  const auto t3 = clk::now();
  if (mcpt::build_sah4(L, on8, &need8, 8, &o8)) return fail("build on, 8 threads", 0, 0);
  o_forced.need_cap = 1;  // two leaf slots at the most: infeasible from three leaves on
  if (mcpt::build_sah4(L, forced, &need_forced, 1, &o_forced)) return fail("build forced", 0, 0);
  if (L.size() == 1) {
    if (!plain.empty() || !on1.empty() || !off.empty()) return fail("single", 0, 0);
    std::printf("ok leaves=1 nodes_off=0 nodes_on=0 need_off=%d need_on=%d optimized=0 hash_off=0\n", need_plain, need1);
    return 0;
  }
  // the pass off: the plain tree, byte for byte, whichever way it is asked for
  if (!same(plain, off) || need_plain != need_off || o_off.optimized) return fail("passes = 0 differs from no options", 0, 0);
  if (!same(on1, on8) || need1 != need8) return fail("thread-dependent tree", (long)on1.size(), (long)on8.size());
  if (check_tree(L, plain, need_plain) || check_tree(L, on1, need1)) return 1;
  if (need1 > need_plain) return fail("need(on) > need(off)", need1, need_plain);
  if (o1.need_plain != need_plain) return fail("need_plain", o1.need_plain, need_plain);
  if (!(o1.cost_out <= o1.cost_plain)) return fail("cost(on) > cost(off)", (long)o1.cost_out, (long)o1.cost_plain);
  if (!o1.optimized && !same(plain, on1)) return fail("not optimized, yet another tree", 0, 0);
  if (L.size() >= 3 && (o_forced.optimized || !same(plain, forced) || need_forced != need_plain))
    return fail("forced infeasible cap did not return the plain tree", need_forced, need_plain);
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  std::printf("ok leaves=%zu nodes_off=%zu nodes_on=%zu need_off=%d need_on=%d cost_off=%.9g cost_on=%.9g optimized=%d "
              "moved=%lld extra_bytes=%lld ms_off=%.1f ms_on=%.1f hash_off=%016llx\n",
              L.size(), plain.size(), on1.size(), need_plain, need1, o1.cost_plain, o1.cost_out, (int)o1.optimized,
              (long long)o1.moved, (long long)o1.extra_bytes, ms(t0, t1), ms(t2, t3),
              fnv1a(plain.data(), plain.size() * sizeof(Node4Rec)));
  return 0;
}

// ---- the estimator (tools/top_pop_sim.cpp's search: nearest first, the other passing slots pushed)
namespace {
struct V {
  float x, y, z;
};
V sub(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V norm(V a) {
  const float l = std::sqrt(dot(a, a));
  return {a.x / l, a.y / l, a.z / l};
}
struct Ray {
  V o, d, ri;
};
bool slab(const float *b, const Ray &r, float tmin, float lim, float &tn) {
  float t0 = -INFINITY, t1 = INFINITY;
  const float o[3] = {r.o.x, r.o.y, r.o.z}, ri[3] = {r.ri.x, r.ri.y, r.ri.z};
  for (int a = 0; a < 3; ++a) {
    const float u = (b[2 * a] - o[a]) * ri[a], v = (b[2 * a + 1] - o[a]) * ri[a];
    t0 = std::fmax(t0, std::fmin(u, v));
    t1 = std::fmin(t1, std::fmax(u, v));
  }
  tn = t0;
  return !(t1 < t0 || t1 < tmin) && !(t0 > lim);
}
float tri_hit(const mcpt_triangle &t, const Ray &r) {
  const V v0{t.v[0][0], t.v[0][1], t.v[0][2]}, v1{t.v[1][0], t.v[1][1], t.v[1][2]}, v2{t.v[2][0], t.v[2][1], t.v[2][2]};
  const V e1 = sub(v1, v0), e2 = sub(v2, v0), p = cross(r.d, e2);
  const float det = dot(e1, p);
  if (std::fabs(det) < 1e-12f) return INFINITY;
  const float inv = 1.0f / det;
  const V s = sub(r.o, v0);
  const float u = dot(s, p) * inv;
  if (u < 0 || u > 1) return INFINITY;
  const V q = cross(s, e1);
  const float v = dot(r.d, q) * inv;
  if (v < 0 || u + v > 1) return INFINITY;
  const float tt = dot(e2, q) * inv;
  return tt > 1e-3f ? tt : INFINITY;
}
struct Counts {
  long steps = 0, tests = 0, segments = 0;
};
float trace(const std::vector<Node4Rec> &N, const std::vector<mcpt_triangle> &T, const Ray &r, float margin, Counts &c,
            int &hit) {
  float best = INFINITY;
  hit = -1;
  std::vector<int> st;
  int cur = 0;
  for (;;) {
    if (cur < 0 && cur != mcpt::kEmptySlot4) {
      ++c.tests;
      const float t = tri_hit(T[~cur], r);
      if (t < best) best = t, hit = ~cur;
      cur = mcpt::kEmptySlot4;
    }
    if (cur == mcpt::kEmptySlot4) {
      if (st.empty()) break;
      cur = st.back();
      st.pop_back();
      continue;
    }
    ++c.steps;
    const Node4Rec &n = N[cur];
    std::pair<float, int> h[4];
    int nh = 0;
    for (int s = 0; s < 4; ++s) {
      if (n.link[s] == mcpt::kEmptySlot4) continue;
      float tn;
      if (slab(n.q + 6 * s, r, 1e-3f, best + margin, tn)) h[nh++] = {tn, s};
    }
    if (!nh) {
      cur = mcpt::kEmptySlot4;
      continue;
    }
    int sel = 0;
    for (int i = 1; i < nh; ++i)
      if (h[i].first < h[sel].first) sel = i;
    for (int i = nh - 1; i >= 0; --i)
      if (i != sel) st.push_back(n.link[h[i].second]);
    cur = n.link[h[sel].second];
  }
  return best;
}
Counts simulate(const std::vector<Node4Rec> &t4, const std::vector<mcpt_triangle> &T, float margin, V eye, V at, float fov,
                int paths) {
  const V fw = norm(sub(at, eye)), rt = norm(cross(fw, V{0, 1, 0})), up = cross(rt, fw);
  Counts c;
  std::mt19937 g(1);
  std::uniform_real_distribution<float> u01(0.0f, 1.0f);
  for (int k = 0; k < paths; ++k) {
    const float a = (u01(g) - 0.5f) * 2 * std::tan(fov / 2), b = (u01(g) - 0.5f) * 2 * std::tan(fov / 2);
    Ray r;
    r.o = eye;
    r.d = norm(V{fw.x + a * rt.x + b * up.x, fw.y + a * rt.y + b * up.y, fw.z + a * rt.z + b * up.z});
    for (int bounce = 0; bounce < 8; ++bounce) {
      r.ri = {1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z};
      int h;
      const float t = trace(t4, T, r, margin, c, h);
      ++c.segments;
      if (h < 0) break;
      const V p{r.o.x + t * r.d.x, r.o.y + t * r.d.y, r.o.z + t * r.d.z};
      V nn{T[h].normal[0], T[h].normal[1], T[h].normal[2]};
      if (dot(nn, r.d) > 0) nn = {-nn.x, -nn.y, -nn.z};
      V d;
      do {
        d = {u01(g) * 2 - 1, u01(g) * 2 - 1, u01(g) * 2 - 1};
      } while (dot(d, d) > 1 || dot(d, d) < 1e-6f);
      d = norm(d);
      if (dot(d, nn) < 0) d = {-d.x, -d.y, -d.z};
      r.o = {p.x + 1e-3f * d.x, p.y + 1e-3f * d.y, p.z + 1e-3f * d.z};
      r.d = d;
    }
  }
  return c;
}
}  // namespace

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "gen" && argc == 5) return check(generate(std::atoi(argv[2]), (unsigned)std::atoi(argv[3]), std::atoi(argv[4]) != 0));
  std::vector<mcpt_triangle> T;
  std::vector<LeafRef> L;
  if (mode == "obj" && argc == 4) return load(argv[2], argv[3], T, L) ? fail("load", 0, 0) : check(L);
  if (mode == "sim" && argc == 12) {
    if (load(argv[2], argv[3], T, L)) return fail("load", 0, 0);
    float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
    for (const LeafRef &l : L)
      for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], l.box[2 * a]), hi[a] = std::max(hi[a], l.box[2 * a + 1]);
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    const float margin = std::ldexp(std::sqrt(dx * dx + dy * dy + dz * dz), -10);
    const V eye{(float)atof(argv[4]), (float)atof(argv[5]), (float)atof(argv[6])};
    const V at{(float)atof(argv[7]), (float)atof(argv[8]), (float)atof(argv[9])};
    const float fov = (float)atof(argv[10]) * 3.14159265f / 180.0f;
    const int paths = atoi(argv[11]);
    std::vector<Node4Rec> off, on;
    int need_off = 0, need_on = 0;
    mcpt::SahOptimize o;
    if (mcpt::build_sah4(L, off, &need_off, 4) || mcpt::build_sah4(L, on, &need_on, 4, &o)) return fail("build", 0, 0);
    const Counts a = simulate(off, T, margin, eye, at, fov, paths), b = simulate(on, T, margin, eye, at, fov, paths);
    std::printf("ok segments_off=%ld segments_on=%ld steps_off=%.4f steps_on=%.4f tests_off=%.4f tests_on=%.4f need_off=%d "
                "need_on=%d nodes_off=%zu nodes_on=%zu\n",
                a.segments, b.segments, (double)a.steps / a.segments, (double)b.steps / b.segments,
                (double)a.tests / a.segments, (double)b.tests / b.segments, need_off, need_on, off.size(), on.size());
    return 0;
  }
  std::fprintf(stderr, "usage: gen n seed clustered | obj dir file | sim dir file px py pz lx ly lz fov paths\n");
  return 2;
}
