// mcpt_host.cpp — host half of libmcpt_hip.so: the scene-side code the
// reference runs on the CPU before/after the per-sample loop.
//
//   parseCamera            MCPT/auxiliary.cpp:20-71
//   material classification MCPT/thirdpartywrapper.cpp:65-97
//   OBJ/MTL loading        MCPT/thirdpartywrapper.cpp:25-63 (+ tinyobjloader 2.0.0rc number
//                          parsing, MCPT/tiny_obj_loader.h:805-954)
//   triangle packing       MCPT/scenebuild.cpp:58-62
//   HLBVH build            MCPT/BVH/hlbvh.cpp:12-200
//   RGBE (.hdr) writer     MCPT/thirdpartywrapper.cpp:14-23 -> stb_image_write v1.13 (:579-724)
//
// Host arithmetic follows the reference host build: IEEE binary32, no FMA
// contraction (MSVC /fp:precise on SSE2), so this file is compiled with
// -ffp-contract=off.
#include "../../include/mcpt_hip.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace mcpt {
// thread-local last error shared with the device half (mcpt_device.hip)
thread_local std::string g_last_error;
int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}
}  // namespace mcpt

using mcpt::fail;

namespace {

// host float4 helpers with the reference host semantics (MCPT/oclbasic.h:119-237):
// component loops over all 4 lanes, plain IEEE ops, std::min/std::max.
struct V4 {
  float s[4];
};
inline V4 v4(const float *p) { return V4{{p[0], p[1], p[2], p[3]}}; }
inline V4 sub(const V4 &a, const V4 &b) {
  V4 r;
  for (int i = 0; i < 4; ++i) r.s[i] = a.s[i] - b.s[i];
  return r;
}
inline V4 add(const V4 &a, const V4 &b) {
  V4 r;
  for (int i = 0; i < 4; ++i) r.s[i] = a.s[i] + b.s[i];
  return r;
}
inline V4 vmin(const V4 &a, const V4 &b) {
  V4 r;
  for (int i = 0; i < 4; ++i) r.s[i] = std::min(a.s[i], b.s[i]);
  return r;
}
inline V4 vmax(const V4 &a, const V4 &b) {
  V4 r;
  for (int i = 0; i < 4; ++i) r.s[i] = std::max(a.s[i], b.s[i]);
  return r;
}
inline V4 cross_host(const V4 &a, const V4 &b) {  // oclbasic.h:119-127 (w = 0)
  V4 r{{0, 0, 0, 0}};
  r.s[0] = a.s[1] * b.s[2] - a.s[2] * b.s[1];
  r.s[1] = -a.s[0] * b.s[2] + a.s[2] * b.s[0];
  r.s[2] = a.s[0] * b.s[1] - a.s[1] * b.s[0];
  return r;
}
inline float dot_host(const V4 &a, const V4 &b) {  // oclbasic.h:129-137: float sum from 0
  float acc = 0.0f;
  for (int i = 0; i < 4; ++i) acc += a.s[i] * b.s[i];
  return acc;
}
inline V4 normalize_host(const V4 &a) {  // oclbasic.h:139-147: divide by sqrtf(dot)
  float len = std::sqrt(dot_host(a, a));
  V4 r = a;
  for (int i = 0; i < 4; ++i) r.s[i] /= len;
  return r;
}
inline void store(float *dst, const V4 &v) { std::memcpy(dst, v.s, 16); }

// The reference host's pi (oclbasic.h:192) — deliberately short.
constexpr double kRefPi = 3.14159265358;

}  // namespace

extern "C" {

const char *mcpt_last_error(void) { return mcpt::g_last_error.c_str(); }

int mcpt_parse_camera(const double position[3], const double lookat[3], const double up[3],
                      double fov_deg, mcpt_camera *out) {
  if (!position || !lookat || !up || !out) return fail(MCPT_ERR_ARG, "parse_camera: null argument");
  mcpt_camera c;
  std::memset(&c, 0, sizeof(c));
  V4 center{{0, 0, 0, 0}}, look{{0, 0, 0, 0}}, upv{{0, 0, 0, 0}};
  for (int i = 0; i < 3; ++i) {
    center.s[i] = (float)position[i];
    look.s[i] = (float)lookat[i];
    upv.s[i] = (float)up[i];
  }
  V4 dir = sub(look, center);
  dir.s[3] = 0.0f;
  // fov: float(json) * M_PI / 180.0f evaluated in double, stored as float
  c.arg = (float)((double)(float)fov_deg * kRefPi / 180.0f);
  V4 horizontal = cross_host(dir, upv);
  V4 realup = cross_host(horizontal, dir);
  c.tmin = 0.0f;
  c.camera_type = 0;  // always perspective (auxiliary.cpp:22)
  store(c.center, center);
  store(c.direction, normalize_host(dir));
  store(c.up, normalize_host(realup));
  store(c.horizontal, normalize_host(horizontal));
  *out = c;
  return MCPT_OK;
}

int mcpt_classify_material(float ior, const float ambient[3], const float diffuse[3],
                           const float specular[3], float shininess, mcpt_material *out) {
  if (!ambient || !diffuse || !specular || !out) return fail(MCPT_ERR_ARG, "classify_material: null argument");
  mcpt_material m;
  std::memset(&m, 0, sizeof(m));
  if (ior != 1.0f) {
    m.type = MCPT_TRANSPARENT;
    m.Ni = ior;
  } else if (ambient[0] > 0.0f || ambient[1] > 0.0f || ambient[2] > 0.0f) {
    m.type = MCPT_LIGHT;
    for (int i = 0; i < 3; ++i) m.ka_ks[i] = ambient[i];
  } else if (shininess != 1.0f) {
    m.type = MCPT_GLOSSY;
    m.Ns = shininess;
    // (Ns + 2) * (2.0 / M_PI) * ks: scalar deduced as double, per-lane double product
    double sc = (double)(shininess + 2) * (2.0 / kRefPi);
    for (int i = 0; i < 3; ++i) m.ka_ks[i] = (float)(sc * (double)specular[i]);
    for (int i = 0; i < 3; ++i) m.kd[i] = (float)((1.0 / kRefPi) * (double)diffuse[i]);
  } else {
    m.type = MCPT_DIFFUSE;
    for (int i = 0; i < 3; ++i) m.kd[i] = (float)((1.0 / kRefPi) * (double)diffuse[i]);
  }
  *out = m;
  return MCPT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ OBJ / MTL
namespace {

// tinyobjloader's number reader: digits accumulated in double, fraction digits
// weighted by 10^-k, exponent applied as ldexp(m * 5^e, e); result cast to float.
bool parse_number(const char *s, const char *end, double *out) {
  if (s >= end) return false;
  const char *p = s;
  double mant = 0.0;
  int exponent = 0, ndig = 0;
  char sign = '+', esign = '+';
  bool leading_dot = false;
  if (*p == '+' || *p == '-') {
    sign = *p++;
    if (p != end && *p == '.') leading_dot = true;
  } else if (*p >= '0' && *p <= '9') {
  } else if (*p == '.') {
    leading_dot = true;
  } else {
    return false;
  }
  bool more = p != end;
  if (!leading_dot) {
    while (more && *p >= '0' && *p <= '9') {
      mant *= 10;
      mant += (int)(*p - '0');
      ++p, ++ndig;
      more = p != end;
    }
    if (ndig == 0) return false;
  }
  if (!more) goto done;
  if (*p == '.') {
    ++p;
    int k = 1;
    more = p != end;
    static const double lut[] = {1.0, 0.1, 0.01, 0.001, 0.0001, 0.00001, 0.000001, 0.0000001};
    while (more && *p >= '0' && *p <= '9') {
      mant += (int)(*p - '0') * (k < 8 ? lut[k] : std::pow(10.0, -k));
      ++k, ++p;
      more = p != end;
    }
  } else if (*p == 'e' || *p == 'E') {
  } else {
    goto done;
  }
  if (!more) goto done;
  if (*p == 'e' || *p == 'E') {
    ++p;
    more = p != end;
    if (more && (*p == '+' || *p == '-')) {
      esign = *p++;
    } else if (!(more && *p >= '0' && *p <= '9')) {
      return false;
    }
    int nexp = 0;
    more = p != end;
    while (more && *p >= '0' && *p <= '9') {
      exponent = exponent * 10 + (int)(*p - '0');
      ++p, ++nexp;
      more = p != end;
    }
    exponent *= (esign == '+' ? 1 : -1);
    if (nexp == 0) return false;
  }
done:
  *out = (sign == '+' ? 1 : -1) * (exponent ? std::ldexp(mant * std::pow(5.0, exponent), exponent) : mant);
  return true;
}

struct Tok {
  const char *p, *e;
};
Tok next_token(const char *&p, const char *end) {
  while (p < end && (*p == ' ' || *p == '\t')) ++p;
  const char *b = p;
  while (p < end && *p != ' ' && *p != '\t' && *p != '\r' && *p != '\n') ++p;
  return Tok{b, p};
}
float read_float(const char *&p, const char *end, double dflt) {
  Tok t = next_token(p, end);
  double v = dflt;
  parse_number(t.p, t.e, &v);
  return (float)v;
}

struct MtlRec {
  std::string name;
  float ka[3] = {0, 0, 0}, kd[3] = {0, 0, 0}, ks[3] = {0, 0, 0};
  float ns = 1.0f, ni = 1.0f;  // tinyobj defaults (tiny_obj_loader.h:1297-1298)
};

bool read_file(const std::string &path, std::string *out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::stringstream ss;
  ss << f.rdbuf();
  *out = ss.str();
  return true;
}

void parse_mtl(const std::string &text, std::vector<MtlRec> *mats, std::map<std::string, int> *index) {
  const char *p = text.data(), *end = p + text.size();
  MtlRec cur;
  bool have = false;
  auto flush = [&]() {
    if (have) {
      if (!index->count(cur.name)) (*index)[cur.name] = (int)mats->size();
      mats->push_back(cur);
    }
  };
  while (p < end) {
    const char *eol = (const char *)std::memchr(p, '\n', end - p);
    if (!eol) eol = end;
    const char *q = p;
    while (q < eol && (*q == ' ' || *q == '\t')) ++q;
    Tok key = next_token(q, eol);
    std::string k(key.p, key.e);
    auto rgb = [&](float *dst) {
      dst[0] = read_float(q, eol, 0.0);
      dst[1] = read_float(q, eol, 0.0);
      dst[2] = read_float(q, eol, 0.0);
    };
    if (k == "newmtl") {
      flush();
      cur = MtlRec();
      have = true;
      while (q < eol && (*q == ' ' || *q == '\t')) ++q;
      const char *ne = eol;
      while (ne > q && (ne[-1] == '\r' || ne[-1] == ' ' || ne[-1] == '\t')) --ne;
      cur.name.assign(q, ne);
    } else if (k == "Ka") {
      rgb(cur.ka);
    } else if (k == "Kd") {
      rgb(cur.kd);
    } else if (k == "Ks") {
      rgb(cur.ks);
    } else if (k == "Ns") {
      cur.ns = read_float(q, eol, 0.0);
    } else if (k == "Ni") {
      cur.ni = read_float(q, eol, 0.0);
    }
    p = eol + 1;
  }
  flush();
}

// fan/ear triangulation: convex polygons give (0,1,2), (0,2,3), ... which is
// what tinyobj's ear clipper (tiny_obj_loader.h:1359-1500) emits for them.
struct Face {
  int v[3];
  int mat;
};

}  // namespace

extern "C" int mcpt_load_obj(const char *directory, const char *objname, mcpt_triangle *tris,
                             int32_t *mat_index, int64_t *n_tris, mcpt_material *mats, int32_t *n_mats) {
  if (!directory || !objname || !n_tris || !n_mats) return fail(MCPT_ERR_ARG, "load_obj: null argument");
  std::string dir(directory), text;
  if (!read_file(dir + objname, &text)) return fail(MCPT_ERR_IO, "load_obj: cannot read " + dir + objname);
  std::vector<float> verts;
  std::vector<Face> faces;
  std::vector<MtlRec> mtl;
  std::map<std::string, int> mtl_index;
  int cur_mat = -1;
  const char *p = text.data(), *end = p + text.size();
  std::vector<int> poly;
  while (p < end) {
    const char *eol = (const char *)std::memchr(p, '\n', end - p);
    if (!eol) eol = end;
    const char *q = p;
    while (q < eol && (*q == ' ' || *q == '\t')) ++q;
    if (q + 1 < eol && q[0] == 'v' && (q[1] == ' ' || q[1] == '\t')) {
      q += 2;
      float x = read_float(q, eol, 0.0), y = read_float(q, eol, 0.0), z = read_float(q, eol, 0.0);
      verts.push_back(x), verts.push_back(y), verts.push_back(z);
    } else if (q + 1 < eol && q[0] == 'f' && (q[1] == ' ' || q[1] == '\t')) {
      q += 2;
      poly.clear();
      int nv = (int)(verts.size() / 3);
      for (;;) {
        Tok t = next_token(q, eol);
        if (t.p == t.e) break;
        int idx = std::atoi(std::string(t.p, t.e).c_str());  // "v", "v/vt", "v//vn", "v/vt/vn"
        if (idx == 0) return fail(MCPT_ERR_PARSE, "load_obj: bad face index");
        poly.push_back(idx > 0 ? idx - 1 : nv + idx);
      }
      if (poly.size() < 3) continue;  // tinyobj drops faces with < 3 vertices
      for (size_t k = 1; k + 1 < poly.size(); ++k) faces.push_back(Face{{poly[0], poly[k], poly[k + 1]}, cur_mat});
    } else if (eol - q >= 6 && std::strncmp(q, "usemtl", 6) == 0 && (q[6] == ' ' || q[6] == '\t')) {
      q += 7;
      while (q < eol && (*q == ' ' || *q == '\t')) ++q;
      const char *ne = eol;
      while (ne > q && (ne[-1] == '\r' || ne[-1] == ' ' || ne[-1] == '\t')) --ne;
      auto it = mtl_index.find(std::string(q, ne));
      cur_mat = it == mtl_index.end() ? -1 : it->second;
    } else if (eol - q >= 6 && std::strncmp(q, "mtllib", 6) == 0 && (q[6] == ' ' || q[6] == '\t')) {
      q += 7;
      for (;;) {
        Tok t = next_token(q, eol);
        if (t.p == t.e) break;
        std::string mt;
        if (read_file(dir + std::string(t.p, t.e), &mt)) {
          parse_mtl(mt, &mtl, &mtl_index);
          break;  // tinyobj uses the first library that loads
        }
      }
    }
    p = eol + 1;
  }
  for (const Face &f : faces)
    for (int k = 0; k < 3; ++k)
      if (f.v[k] < 0 || (size_t)(3 * f.v[k] + 2) >= verts.size()) return fail(MCPT_ERR_PARSE, "load_obj: face index out of range");
  if (tris) {
    if (*n_tris < (int64_t)faces.size()) return fail(MCPT_ERR_ARG, "load_obj: triangle buffer too small");
    for (size_t i = 0; i < faces.size(); ++i) {
      mcpt_triangle t;
      std::memset(&t, 0, sizeof(t));
      for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) t.v[k][j] = verts[3 * faces[i].v[k] + j];
      tris[i] = t;
      if (mat_index) mat_index[i] = faces[i].mat;
    }
  }
  if (mats) {
    if (*n_mats < (int32_t)mtl.size()) return fail(MCPT_ERR_ARG, "load_obj: material buffer too small");
    for (size_t i = 0; i < mtl.size(); ++i)
      mcpt_classify_material(mtl[i].ni, mtl[i].ka, mtl[i].kd, mtl[i].ks, mtl[i].ns, &mats[i]);
  }
  *n_tris = (int64_t)faces.size();
  *n_mats = (int32_t)mtl.size();
  return MCPT_OK;
}

// --------------------------------------------------------- triangle packing
extern "C" int mcpt_pack_triangles(mcpt_triangle *tris, const int32_t *mat_index, int64_t n) {
  if (n < 0 || (n > 0 && (!tris || !mat_index))) return fail(MCPT_ERR_ARG, "pack_triangles: bad argument");
  for (int64_t i = 0; i < n; ++i) {
    V4 a = v4(tris[i].v[0]), b = v4(tris[i].v[1]), c = v4(tris[i].v[2]);
    V4 nrm = normalize_host(cross_host(sub(b, a), sub(c, a)));
    store(tris[i].normal, nrm);
    std::memcpy(&tris[i].normal[3], &mat_index[i], 4);
  }
  return MCPT_OK;
}

// -------------------------------------------------------------------- HLBVH
namespace {

inline uint32_t spread_bits10(uint32_t x) {  // hlbvh.cpp:12-23 (1024 clamps to 1023)
  if (x == (1u << 10)) --x;
  x = (x | (x << 16)) & 0x030000FFu;
  x = (x | (x << 8)) & 0x0300F00Fu;
  x = (x | (x << 4)) & 0x030C30C3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}

// (cl_uint)roundf(v) as the reference's MSVC x64 build evaluates it: the
// conversion goes through a 64-bit cvttss2si, so NaN (0/0 on a flat axis)
// and out-of-range values keep the low 32 bits of 0x8000000000000000 = 0.
inline uint32_t to_uint_like_msvc(float v) {
  float r = std::round(v);
  if (!(r > -9.2233720368547758e18f && r < 9.2233720368547758e18f)) return 0u;
  return (uint32_t)(int64_t)r;
}

inline int clz_ref(int a) {  // hlbvh.cpp:138-146
  if (a == 0) return 32;
  int n = 0;
  uint32_t u = (uint32_t)a;
  while ((int32_t)u > 0) {
    u <<= 1;
    ++n;
  }
  return n;
}

struct Prim {
  int id;
  int code;
};

}  // namespace

extern "C" int mcpt_build_hlbvh(const mcpt_triangle *tris, int64_t n, mcpt_bvh_node *nodes) {
  if (n <= 0 || !tris || !nodes) return fail(MCPT_ERR_ARG, "build_hlbvh: empty scene or null pointer");
  if (n > (int64_t)0x3FFFFFFF) return fail(MCPT_ERR_LIMIT, "build_hlbvh: too many triangles");
  std::vector<V4> bmin(n), bmax(n), cen(n);
  for (int64_t i = 0; i < n; ++i) {
    V4 a = v4(tris[i].v[0]), b = v4(tris[i].v[1]), c = v4(tris[i].v[2]);
    a.s[3] = b.s[3] = c.s[3] = 0.0f;  // packFloat zero-initialises .w (thirdpartywrapper.cpp:38)
    bmin[i] = vmin(vmin(a, b), c);
    bmax[i] = vmax(vmax(a, b), c);
    V4 s = add(bmin[i], bmax[i]);
    for (int k = 0; k < 4; ++k) cen[i].s[k] = 0.5f * s.s[k];
  }
  V4 gmin{{FLT_MAX, FLT_MAX, FLT_MAX, FLT_MAX}}, gmax{{-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX}};
  for (int64_t i = 0; i < n; ++i) {
    gmin = vmin(gmin, cen[i]);
    gmax = vmax(gmax, cen[i]);
  }
  V4 gsize = sub(gmax, gmin);
  std::vector<Prim> prims(n);
  for (int64_t i = 0; i < n; ++i) {
    V4 d = sub(cen[i], gmin);
    uint32_t q[3];
    for (int k = 0; k < 3; ++k) {
      float x = d.s[k] / gsize.s[k];
      x *= 1024.0f;
      q[k] = to_uint_like_msvc(x);
    }
    uint32_t code = (spread_bits10(q[2]) << 2) | (spread_bits10(q[1]) << 1) | spread_bits10(q[0]);
    prims[i] = Prim{(int)i, (int)code};
  }
  // 5 stable LSD passes of 6 bits over the 30-bit code == a stable sort on the code
  std::stable_sort(prims.begin(), prims.end(), [](const Prim &a, const Prim &b) {
    return (uint32_t)(a.code & 0x3FFFFFFF) < (uint32_t)(b.code & 0x3FFFFFFF);
  });
  const int64_t nn = 2 * n - 1;
  std::memset(nodes, 0, sizeof(mcpt_bvh_node) * (size_t)nn);
  nodes[0].parent = -1;
  auto delta = [&](int64_t a, int64_t b) { return clz_ref(prims[a].code ^ prims[b].code); };
  auto split = [&](int64_t left, int64_t right) -> int64_t {  // hlbvh.cpp:152-161
    int target = delta(left, right);
    if (target == 32) return (right + left) >> 1;
    do {
      int64_t mid = (right + left) >> 1;
      if (delta(left, mid) > target)
        left = mid;
      else
        right = mid;
    } while (right > left + 1);
    return left;
  };
  if (n > 1) {
    struct Range {
      int64_t lo, hi, node;
    };
    std::deque<Range> work;  // breadth-first, hlbvh.cpp:165-188
    work.push_back(Range{0, n - 1, 0});
    while (!work.empty()) {
      Range r = work.front();
      work.pop_front();
      int64_t s = split(r.lo, r.hi);
      int64_t li = (s != r.lo) ? s : s + n - 1;
      int64_t ri = (s + 1 != r.hi) ? s + 1 : s + n;
      nodes[r.node].left = (int32_t)li;
      nodes[li].parent = (int32_t)r.node;
      nodes[r.node].right = (int32_t)ri;
      nodes[ri].parent = (int32_t)r.node;
      if (li == s) work.push_back(Range{r.lo, s, s});
      if (ri == s + 1) work.push_back(Range{s + 1, r.hi, s + 1});
    }
  }
  for (int64_t i = n - 1; i < nn; ++i) {
    int id = prims[i - (n - 1)].id;
    nodes[i].left = nodes[i].right = id;
    store(nodes[i].bbmin, bmin[id]);
    store(nodes[i].bbmax, bmax[id]);
  }
  if (n == 1) return MCPT_OK;  // the reference indexes past its 1-node array here (hlbvh.cpp:176-181)
  // refit (hlbvh.cpp:64-76), iterative post-order so deep trees cannot blow the C stack
  std::vector<std::pair<int64_t, int>> st;
  st.push_back({0, 0});
  while (!st.empty()) {
    auto &top = st.back();
    int64_t id = top.first;
    mcpt_bvh_node &nd = nodes[id];
    if (nd.left == nd.right) {
      st.pop_back();
      continue;
    }
    if (top.second == 0) {
      top.second = 1;
      st.push_back({nd.left, 0});
    } else if (top.second == 1) {
      top.second = 2;
      st.push_back({nd.right, 0});
    } else {
      V4 lmin = v4(nodes[nd.left].bbmin), lmax = v4(nodes[nd.left].bbmax);
      V4 rmin = v4(nodes[nd.right].bbmin), rmax = v4(nodes[nd.right].bbmax);
      store(nd.bbmin, vmin(lmin, rmin));
      store(nd.bbmax, vmax(lmax, rmax));
      st.pop_back();
    }
  }
  return MCPT_OK;
}

extern "C" int mcpt_bvh_stack_depth(const mcpt_bvh_node *nodes, int64_t n_nodes, int32_t *depth) {
  if (!nodes || n_nodes <= 0 || !depth) return fail(MCPT_ERR_ARG, "bvh_stack_depth: bad argument");
  // left-first DFS pushes the right child at every internal node it descends
  // through; the stack holds at most (#internal ancestors) entries.
  int32_t best = 1;
  std::vector<std::pair<int32_t, int32_t>> st;  // node, pushes so far
  st.push_back({0, 0});
  while (!st.empty()) {
    auto [id, d] = st.back();
    st.pop_back();
    if (id < 0 || id >= n_nodes) return fail(MCPT_ERR_ARG, "bvh_stack_depth: child index out of range");
    const mcpt_bvh_node &nd = nodes[id];
    best = std::max(best, d + 1);
    if (nd.left == nd.right) continue;
    if ((int64_t)st.size() > 4 * n_nodes) return fail(MCPT_ERR_ARG, "bvh_stack_depth: cyclic tree");
    st.push_back({nd.left, d + 1});
    st.push_back({nd.right, d});
  }
  *depth = best;
  return MCPT_OK;
}

// BVH::TEST::SAH (bvhtest.cpp:97-108): float products summed in double,
// Cinn for nodes [0, size/2), Ctri for the rest, over the root's area.
extern "C" int mcpt_bvh_sah(const mcpt_bvh_node *nodes, int64_t n_nodes, double *out) {
  if (!nodes || n_nodes <= 0 || !out) return fail(MCPT_ERR_ARG, "bvh_sah: bad argument");
  auto area = [](const mcpt_bvh_node &b) {  // auxiliary.cpp:15-18
    const float x = b.bbmax[0] - b.bbmin[0], y = b.bbmax[1] - b.bbmin[1], z = b.bbmax[2] - b.bbmin[2];
    return 2.0f * (x * y + x * z + y * z);
  };
  const float cinn = 1.2f, ctri = 1.0f;  // auxiliary.h:9-11
  double sah = 0.0f;
  const size_t size = (size_t)n_nodes;
  for (size_t i = 0; i < (size >> 1); ++i) sah += cinn * area(nodes[i]);
  for (size_t i = (size >> 1); i < size; ++i) sah += ctri * area(nodes[i]);
  sah /= area(nodes[0]);
  *out = (double)(float)sah;  // SAH returns float
  return MCPT_OK;
}

// ---------------------------------------------------------------------- HDR
namespace {

void rgbe_pixel(uint8_t *o, const float *lin) {  // stb_image_write.h:579-593
  auto mx = [](float a, float b) { return a > b ? a : b; };
  float maxcomp = mx(lin[0], mx(lin[1], lin[2]));
  if (maxcomp < 1e-32f) {
    o[0] = o[1] = o[2] = o[3] = 0;
    return;
  }
  int e;
  float norm = (float)std::frexp(maxcomp, &e) * 256.0f / maxcomp;
  for (int i = 0; i < 3; ++i) o[i] = (uint8_t)(int)(lin[i] * norm);
  o[3] = (uint8_t)(e + 128);
}

struct Sink {
  uint8_t *buf;
  int64_t cap, n;
  void put(const void *p, int64_t len) {
    if (buf && n + len <= cap) std::memcpy(buf + n, p, (size_t)len);
    n += len;
  }
  void byte(uint8_t b) { put(&b, 1); }
};

void scanline(Sink &s, int w, const float *row, std::vector<uint8_t> &scr) {
  uint8_t rgbe[4];
  if (w < 8 || w >= 32768) {  // no RLE
    for (int x = 0; x < w; ++x) {
      rgbe_pixel(rgbe, row + 4 * x);
      s.put(rgbe, 4);
    }
    return;
  }
  for (int x = 0; x < w; ++x) {
    rgbe_pixel(rgbe, row + 4 * x);
    for (int c = 0; c < 4; ++c) scr[x + w * c] = rgbe[c];
  }
  uint8_t hdr[4] = {2, 2, (uint8_t)((w & 0xff00) >> 8), (uint8_t)(w & 0xff)};
  s.put(hdr, 4);
  for (int c = 0; c < 4; ++c) {  // per-component RLE (stb_image_write.h:650-690)
    const uint8_t *comp = &scr[(size_t)w * c];
    int x = 0;
    while (x < w) {
      int r = x;
      while (r + 2 < w && !(comp[r] == comp[r + 1] && comp[r] == comp[r + 2])) ++r;
      if (r + 2 >= w) r = w;
      while (x < r) {
        int len = std::min(r - x, 128);
        s.byte((uint8_t)len);
        s.put(comp + x, len);
        x += len;
      }
      if (r + 2 < w) {
        while (r < w && comp[r] == comp[x]) ++r;
        while (x < r) {
          int len = std::min(r - x, 127);
          s.byte((uint8_t)(len + 128));
          s.byte(comp[x]);
          x += len;
        }
      }
    }
  }
}

int64_t encode_hdr(Sink &s, int w, int h, const float *rgba, int flip) {
  static const char head[] = "#?RADIANCE\n# Written by stb_image_write.h\nFORMAT=32-bit_rle_rgbe\n";
  s.put(head, sizeof(head) - 1);
  char buf[128];
  int len = std::snprintf(buf, sizeof(buf), "EXPOSURE=          1.0000000000000\n\n-Y %d +X %d\n", h, w);
  s.put(buf, len);
  std::vector<uint8_t> scr((size_t)w * 4);
  for (int i = 0; i < h; ++i) scanline(s, w, rgba + (size_t)4 * w * (flip ? h - 1 - i : i), scr);
  return s.n;
}

}  // namespace

extern "C" int64_t mcpt_encode_hdr(int32_t width, int32_t height, const float *rgba, int32_t flip,
                                   uint8_t *out, int64_t cap) {
  if (width <= 0 || height <= 0 || !rgba) return fail(MCPT_ERR_ARG, "encode_hdr: bad argument");
  Sink s{out, cap, 0};
  const int64_t n = encode_hdr(s, width, height, rgba, flip);
  if (out && n > cap) return fail(MCPT_ERR_ARG, "encode_hdr: output buffer too small");
  return n;
}

// Radiance RGBE reader, the inverse of the encoder above for the files it and
// stb_image_write produce, decoding as stb_image.h does (stbi__hdr_load,
// stbi__hdr_convert).  A parser of files from outside: every read is checked
// against `len` and every write against the scanline.
namespace {

struct Source {
  const uint8_t *p;
  int64_t len, at;
  bool get(uint8_t *b) {
    if (at >= len) return false;
    *b = p[at++];
    return true;
  }
  // one header line without its '\n'; false at the end of the input
  bool line(std::string *out) {
    out->clear();
    if (at >= len) return false;
    while (at < len && p[at] != '\n') {
      if (out->size() >= 1024) return false;
      out->push_back((char)p[at++]);
    }
    if (at >= len) return false;  // a header line ends with its newline
    ++at;
    return true;
  }
};

inline void rgbe_to_float(float *out, const uint8_t *in) {  // stb_image.h stbi__hdr_convert
  if (in[3] != 0) {
    const float f1 = std::ldexp(1.0f, (int)in[3] - (128 + 8));
    out[0] = in[0] * f1, out[1] = in[1] * f1, out[2] = in[2] * f1;
  } else {
    out[0] = out[1] = out[2] = 0.0f;
  }
}

// "-Y h +X w": positive decimal numbers, nothing else on the line
bool parse_resolution(const std::string &s, int64_t *w, int64_t *h) {
  size_t i = 0;
  auto number = [&](int64_t *v) {
    if (i >= s.size() || s[i] < '0' || s[i] > '9') return false;
    int64_t x = 0;
    while (i < s.size() && s[i] >= '0' && s[i] <= '9') {
      x = x * 10 + (s[i++] - '0');
      if (x > (int64_t)1 << 32) return false;
    }
    *v = x;
    return true;
  };
  if (s.compare(0, 3, "-Y ") != 0) return false;
  i = 3;
  if (!number(h)) return false;
  while (i < s.size() && s[i] == ' ') ++i;
  if (s.compare(i, 3, "+X ") != 0) return false;
  i += 3;
  if (!number(w)) return false;
  return i == s.size();
}

}  // namespace

extern "C" int mcpt_decode_hdr(const uint8_t *bytes, int64_t len, int32_t *width, int32_t *height, float *rgb_out,
                               int64_t cap) {
  if (!bytes || len < 0 || !width || !height) return fail(MCPT_ERR_ARG, "decode_hdr: bad argument");
  Source s{bytes, len, 0};
  std::string tok;
  if (!s.line(&tok) || (tok != "#?RADIANCE" && tok != "#?RGBE")) return fail(MCPT_ERR_PARSE, "decode_hdr: not a Radiance file");
  bool format = false;
  for (;;) {
    if (!s.line(&tok)) return fail(MCPT_ERR_PARSE, "decode_hdr: truncated header");
    if (tok.empty()) break;
    if (tok == "FORMAT=32-bit_rle_rgbe") format = true;
  }
  if (!format) return fail(MCPT_ERR_PARSE, "decode_hdr: not the 32-bit_rle_rgbe format");
  int64_t w = 0, h = 0;
  if (!s.line(&tok) || !parse_resolution(tok, &w, &h)) return fail(MCPT_ERR_PARSE, "decode_hdr: bad resolution line");
  if (w < 1 || h < 1 || w > INT32_MAX || h > INT32_MAX || w * h > ((int64_t)1 << 26))
    return fail(MCPT_ERR_PARSE, "decode_hdr: dimensions out of range (width * height <= 2^26)");
  *width = (int32_t)w, *height = (int32_t)h;
  if (!rgb_out) return MCPT_OK;  // the size query
  if (cap < w * h * 3) return fail(MCPT_ERR_ARG, "decode_hdr: output buffer too small");
  uint8_t px[4];
  auto pixel = [&](uint8_t *o) { return s.get(o) && s.get(o + 1) && s.get(o + 2) && s.get(o + 3); };
  auto flat = [&](int64_t first) {  // flat RGBE pixels from pixel index `first` on
    for (int64_t k = first; k < w * h; ++k) {
      if (!pixel(px)) return false;
      rgbe_to_float(rgb_out + 3 * k, px);
    }
    return true;
  };
  if (w < 8 || w >= 32768) {
    if (!flat(0)) return fail(MCPT_ERR_PARSE, "decode_hdr: truncated pixel data");
    return MCPT_OK;
  }
  std::vector<uint8_t> scan((size_t)w * 4);
  for (int64_t j = 0; j < h; ++j) {
    if (!pixel(px)) return fail(MCPT_ERR_PARSE, "decode_hdr: truncated scanline");
    if (px[0] != 2 || px[1] != 2 || (px[2] & 0x80)) {
      // not run-length encoded: a flat file whose first pixel this is (stb
      // takes that turn at any scanline; only the first can be meant)
      if (j != 0) return fail(MCPT_ERR_PARSE, "decode_hdr: bad scanline header");
      rgbe_to_float(rgb_out, px);
      if (!flat(1)) return fail(MCPT_ERR_PARSE, "decode_hdr: truncated pixel data");
      return MCPT_OK;
    }
    if ((((int64_t)px[2] << 8) | px[3]) != w) return fail(MCPT_ERR_PARSE, "decode_hdr: scanline width disagrees with the header");
    for (int c = 0; c < 4; ++c) {
      uint8_t *comp = scan.data() + (size_t)w * c;
      int64_t i = 0;
      while (i < w) {
        uint8_t count, value;
        if (!s.get(&count)) return fail(MCPT_ERR_PARSE, "decode_hdr: truncated scanline");
        const bool run = count > 128;
        int64_t n = run ? count - 128 : count;
        if (n == 0 || n > w - i) return fail(MCPT_ERR_PARSE, "decode_hdr: run longer than the scanline");
        if (run) {
          if (!s.get(&value)) return fail(MCPT_ERR_PARSE, "decode_hdr: truncated scanline");
          std::memset(comp + i, value, (size_t)n);
        } else {
          if (s.len - s.at < n) return fail(MCPT_ERR_PARSE, "decode_hdr: truncated scanline");
          std::memcpy(comp + i, s.p + s.at, (size_t)n);
          s.at += n;
        }
        i += n;
      }
    }
    for (int64_t i = 0; i < w; ++i) {
      const uint8_t q[4] = {scan[(size_t)i], scan[(size_t)(w + i)], scan[(size_t)(2 * w + i)], scan[(size_t)(3 * w + i)]};
      rgbe_to_float(rgb_out + 3 * (j * w + i), q);
    }
  }
  return MCPT_OK;
}

extern "C" int mcpt_write_hdr(const char *path, int32_t width, int32_t height, const float *rgba,
                              int32_t flip) {
  if (!path) return fail(MCPT_ERR_ARG, "write_hdr: null path");
  int64_t n = mcpt_encode_hdr(width, height, rgba, flip, nullptr, 0);
  if (n < 0) return (int)n;
  std::vector<uint8_t> bytes((size_t)n);
  mcpt_encode_hdr(width, height, rgba, flip, bytes.data(), n);
  FILE *f = std::fopen(path, "wb");
  if (!f) return fail(MCPT_ERR_IO, std::string("write_hdr: cannot open ") + path);
  size_t wr = std::fwrite(bytes.data(), 1, bytes.size(), f);
  std::fclose(f);
  if (wr != bytes.size()) return fail(MCPT_ERR_IO, "write_hdr: short write");
  return MCPT_OK;
}

// ---------------------------------------------------------- vertex normals
// Smooth shading's host half (opt-in, no reference counterpart; the normative
// text is in include/mcpt_hip.h): vertex normals generated from the packed
// triangles, and authored ones read from an OBJ file's `vn` records.
namespace {

inline uint32_t weld_bits(float f) {  // a position component's bits, -0 as +0
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u == 0x80000000u ? 0u : u;
}
struct Corner {
  uint32_t key[3];
  uint32_t id;  // 3 * triangle + corner
};
constexpr int64_t kMaxPairwiseValence = 65536;  // mcpt_vertex_normals' pairwise path (include/mcpt_hip.h)
inline bool corner_less(const Corner &a, const Corner &b) {
  for (int k = 0; k < 3; ++k)
    if (a.key[k] != b.key[k]) return a.key[k] < b.key[k];
  return a.id < b.id;  // ascending triangle index inside a welded vertex
}

// one OBJ corner "v", "v/vt", "v//vn" or "v/vt/vn": the first and third integer (0: absent or malformed)
void corner_indices(const char *p, const char *e, long *v, long *vn) {
  long f[3] = {0, 0, 0};
  for (int k = 0; k < 3 && p < e; ++k) {
    const char *s = p;
    while (p < e && *p != '/') ++p;
    if (p - s > 0 && p - s < 24) f[k] = std::strtol(std::string(s, p).c_str(), nullptr, 10);
    if (p < e) ++p;  // the slash
  }
  *v = f[0], *vn = f[2];
}

}  // namespace

extern "C" int mcpt_vertex_normals(const mcpt_triangle *tris, int64_t n, double crease_deg, float *vn) {
  if (n < 0 || (n > 0 && (!tris || !vn))) return fail(MCPT_ERR_ARG, "vertex_normals: bad argument");
  if (!(crease_deg >= 0.0 && crease_deg <= 180.0)) return fail(MCPT_ERR_ARG, "vertex_normals: crease outside [0, 180] degrees");
  if (n > (int64_t)0x3FFFFFFF) return fail(MCPT_ERR_LIMIT, "vertex_normals: too many triangles");
  const double cosc = std::cos(crease_deg * (3.14159265358979323846 / 180.0));
  // a face normal that is not finite or not unit: the triangle is degenerate, joins no vertex and stays flat
  std::vector<uint8_t> valid((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const float *g = tris[i].normal;
    const double l2 = (double)g[0] * g[0] + (double)g[1] * g[1] + (double)g[2] * g[2];
    valid[(size_t)i] = std::isfinite(l2) && std::fabs(std::sqrt(l2) - 1.0) <= 1e-3;
    for (int k = 0; k < 3; ++k) std::memcpy(vn + 9 * i + 3 * k, g, 12);
  }
  // weld: corners sorted by their position's bits; a run of equal keys is one vertex
  std::vector<Corner> cs;
  cs.reserve((size_t)n * 3);
  for (int64_t i = 0; i < n; ++i) {
    if (!valid[(size_t)i]) continue;
    for (int k = 0; k < 3; ++k) {
      const float *p = tris[i].v[k];
      cs.push_back(Corner{{weld_bits(p[0]), weld_bits(p[1]), weld_bits(p[2])}, (uint32_t)(3 * i + k)});
    }
  }
  std::sort(cs.begin(), cs.end(), corner_less);
  std::vector<double> wn;  // per corner of the run: angle * ng
  for (size_t lo = 0; lo < cs.size();) {
    size_t hi = lo + 1;
    while (hi < cs.size() && std::memcmp(cs[hi].key, cs[lo].key, 12) == 0) ++hi;
    wn.resize(3 * (hi - lo));
    for (size_t a = lo; a < hi; ++a) {  // triangle j's interior angle at this corner, times its face normal
      const mcpt_triangle &t = tris[cs[a].id / 3];
      const int k = (int)(cs[a].id % 3);
      const float *p = t.v[k], *q = t.v[(k + 1) % 3], *r = t.v[(k + 2) % 3];
      const double e[3] = {(double)q[0] - p[0], (double)q[1] - p[1], (double)q[2] - p[2]};
      const double f[3] = {(double)r[0] - p[0], (double)r[1] - p[1], (double)r[2] - p[2]};
      const double cx = e[1] * f[2] - e[2] * f[1], cy = e[2] * f[0] - e[0] * f[2], cz = e[0] * f[1] - e[1] * f[0];
      const double ang = std::atan2(std::sqrt(cx * cx + cy * cy + cz * cz), e[0] * f[0] + e[1] * f[1] + e[2] * f[2]);
      for (int c = 0; c < 3; ++c) wn[3 * (a - lo) + c] = ang * (double)t.normal[c];
    }
    // A vertex of many corners (a pole, a fan's apex) whose normals all sit in one narrow cone: every pair
    // is then inside the crease, every corner's sum is the whole run's, in the same order: one sum, O(m).
    // Sufficient, not necessary (angles to the run's mean direction, the triangle inequality, and margins
    // far above the rounding of the dots); a run that fails it takes the pairwise loop below.
    const size_t m = hi - lo;
    bool one_cone = crease_deg >= 1.0 && crease_deg <= 179.0, identical = true;
    double sum[3] = {0.0, 0.0, 0.0};
    {
      const float *g0 = tris[cs[lo].id / 3].normal;
      double c[3] = {0.0, 0.0, 0.0};
      for (size_t b = lo; b < hi; ++b) {
        const float *gj = tris[cs[b].id / 3].normal;
        identical = identical && std::memcmp(g0, gj, 12) == 0;
        for (int k = 0; k < 3; ++k) c[k] += gj[k], sum[k] += wn[3 * (b - lo) + k];
      }
      const double cl = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
      const double half = std::cos(0.5 * crease_deg * (3.14159265358979323846 / 180.0) - 1e-4);
      one_cone = one_cone && cl > 0.5 * (double)m;
      for (size_t b = lo; one_cone && b < hi; ++b) {
        const float *gj = tris[cs[b].id / 3].normal;
        const double l2 = (double)gj[0] * gj[0] + (double)gj[1] * gj[1] + (double)gj[2] * gj[2];
        const double d = (c[0] * gj[0] + c[1] * gj[1] + c[2] * gj[2]) / cl;
        one_cone = std::fabs(l2 - 1.0) <= 2e-6 && d >= half * (1.0 + 2e-6);
      }
    }
    if (one_cone) {
      const double len = std::sqrt(sum[0] * sum[0] + sum[1] * sum[1] + sum[2] * sum[2]);
      if (!identical && len >= 1e-12)
        for (size_t a = lo; a < hi; ++a)
          for (int k = 0; k < 3; ++k) vn[3 * (size_t)cs[a].id + k] = (float)(sum[k] / len);
      lo = hi;
      continue;
    }
    // the general case costs m^2 pair tests: bounded, so that no input runs for hours
    if (m > (size_t)kMaxPairwiseValence)
      return fail(MCPT_ERR_LIMIT, "vertex_normals: a vertex is shared by more than 65536 corners whose face normals "
                                  "spread beyond half the crease angle");
    for (size_t a = lo; a < hi; ++a) {
      const float *gi = tris[cs[a].id / 3].normal;
      double s[3] = {0.0, 0.0, 0.0};
      bool all_equal = true;
      for (size_t b = lo; b < hi; ++b) {
        const float *gj = tris[cs[b].id / 3].normal;
        const bool same = std::memcmp(gi, gj, 12) == 0;
        const double dot = (double)gi[0] * gj[0] + (double)gi[1] * gj[1] + (double)gi[2] * gj[2];
        if (!(same || (crease_deg > 0.0 && dot >= cosc))) continue;
        all_equal = all_equal && same;
        for (int c = 0; c < 3; ++c) s[c] += wn[3 * (b - lo) + c];
      }
      const double len = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
      if (all_equal || !(len >= 1e-12)) continue;  // stays the face normal, bit for bit
      float *out = vn + 3 * (size_t)cs[a].id;
      for (int c = 0; c < 3; ++c) out[c] = (float)(s[c] / len);
    }
    lo = hi;
  }
  return MCPT_OK;
}

extern "C" int mcpt_obj_normals_from_text(const char *text, int64_t len, float *vn, uint8_t *has, int64_t *n_tris) {
  if (!n_tris || len < 0 || (len > 0 && !text)) return fail(MCPT_ERR_ARG, "obj_normals: bad argument");
  std::vector<double> normals;  // the vn records, as parsed
  struct FaceN {
    long n[3];  // 0-based vn index per corner, -1: none
  };
  std::vector<FaceN> faces;
  std::vector<long> poly;
  const char *p = text, *end = text + len;
  while (p < end) {
    const char *eol = (const char *)std::memchr(p, '\n', end - p);
    if (!eol) eol = end;
    const char *q = p;
    while (q < eol && (*q == ' ' || *q == '\t')) ++q;
    if (q + 2 < eol && q[0] == 'v' && q[1] == 'n' && (q[2] == ' ' || q[2] == '\t')) {
      q += 3;
      for (int k = 0; k < 3; ++k) {
        Tok t = next_token(q, eol);
        double v = 0.0;
        parse_number(t.p, t.e, &v);
        normals.push_back(v);
      }
    } else if (q + 1 < eol && q[0] == 'f' && (q[1] == ' ' || q[1] == '\t')) {
      q += 2;
      poly.clear();
      const long nvn = (long)(normals.size() / 3);
      for (;;) {
        Tok t = next_token(q, eol);
        if (t.p == t.e) break;
        long v, n;
        corner_indices(t.p, t.e, &v, &n);
        if (v == 0) return fail(MCPT_ERR_PARSE, "obj_normals: bad face index");  // as mcpt_load_obj
        if (n < 0 && nvn + n < 0) return fail(MCPT_ERR_PARSE, "obj_normals: vn index out of range");
        poly.push_back(n > 0 ? n - 1 : (n < 0 ? nvn + n : -1));
      }
      if (poly.size() < 3) {
        p = eol + 1;
        continue;
      }
      for (size_t k = 1; k + 1 < poly.size(); ++k) faces.push_back(FaceN{{poly[0], poly[k], poly[k + 1]}});
    }
    p = eol + 1;
  }
  const long nvn = (long)(normals.size() / 3);
  for (const FaceN &f : faces)
    for (int k = 0; k < 3; ++k)
      if (f.n[k] >= nvn) return fail(MCPT_ERR_PARSE, "obj_normals: vn index out of range");
  if (vn || has) {
    if (!vn || !has) return fail(MCPT_ERR_ARG, "obj_normals: vn and has come together");
    if (*n_tris < (int64_t)faces.size()) return fail(MCPT_ERR_ARG, "obj_normals: buffers too small");
    for (size_t i = 0; i < faces.size(); ++i) {
      bool ok = true;
      float out[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int k = 0; k < 3 && ok; ++k) {
        if (faces[i].n[k] < 0) {
          ok = false;
          break;
        }
        const double *v = &normals[3 * (size_t)faces[i].n[k]];
        const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        ok = std::isfinite(l) && l > 0.0;
        for (int c = 0; c < 3 && ok; ++c) out[3 * k + c] = (float)(v[c] / l);
      }
      if (!ok) std::memset(out, 0, sizeof out);
      std::memcpy(vn + 9 * i, out, sizeof out);
      has[i] = ok ? 1 : 0;
    }
  }
  *n_tris = (int64_t)faces.size();
  return MCPT_OK;
}

extern "C" int mcpt_load_obj_normals(const char *directory, const char *objname, float *vn, uint8_t *has,
                                     int64_t *n_tris) {
  if (!directory || !objname || !n_tris) return fail(MCPT_ERR_ARG, "load_obj_normals: null argument");
  std::string dir(directory), text;
  if (!read_file(dir + objname, &text)) return fail(MCPT_ERR_IO, "load_obj_normals: cannot read " + dir + objname);
  return mcpt_obj_normals_from_text(text.data(), (int64_t)text.size(), vn, has, n_tris);
}

// ------------------------------------------------- texture maps (opt-in)
namespace {

// Field k (0: v, 1: vt, 2: vn) of an OBJ face corner "v", "v/vt", "v//vn",
// "v/vt/vn": 0 absent or empty, 1 a number in *out, -1 not a usable number
int corner_field(const char *p, const char *e, int k, long *out) {
  for (int f = 0; f < k; ++f) {
    while (p < e && *p != '/') ++p;
    if (p == e) return 0;
    ++p;  // the slash
  }
  const char *s = p;
  while (p < e && *p != '/') ++p;
  if (p == s) return 0;
  if (p - s >= 24) return -1;
  const std::string t(s, p);
  char *stop = nullptr;
  *out = std::strtol(t.c_str(), &stop, 10);  // saturates: an overflowing index is out of range below
  return stop == t.c_str() + t.size() ? 1 : -1;
}

bool whole_number(const char *p, const char *e) {
  if (p == e || e - p >= 64) return false;
  const std::string t(p, e);
  char *stop = nullptr;
  (void)std::strtod(t.c_str(), &stop);
  return stop == t.c_str() + t.size();
}

// The file name of a map_Kd line's arguments [q, eol): options first (skipped,
// not honoured), then the name, which may hold spaces; backslashes become slashes.
// bm: where the value of a usable `-bm` option goes (the bump multiplier of
// map_Bump, bump and norm lines), wherever among the options it stands
std::string map_name(const char *q, const char *eol, double *bm = nullptr) {
  static const char *const one[] = {"-blendu", "-blendv", "-clamp", "-cc", "-imfchan", "-type", "-texres", "-boost", "-bm"};
  for (;;) {
    while (q < eol && (*q == ' ' || *q == '\t')) ++q;
    const char *save = q;
    Tok t = next_token(q, eol);
    if (t.p == t.e) return std::string();
    const std::string k(t.p, t.e);
    int fixed = -1;
    for (const char *o : one)
      if (k == o) fixed = 1;
    if (k == "-mm") fixed = 2;
    if (bm && k == "-bm") {
      Tok n = next_token(q, eol);
      double v = 0.0;
      if (n.e - n.p < 64 && parse_number(n.p, n.e, &v) && std::isfinite(v)) *bm = v;
      continue;
    }
    if (fixed >= 0) {
      for (int a = 0; a < fixed; ++a) (void)next_token(q, eol);
      continue;
    }
    if (k == "-o" || k == "-s" || k == "-t") {  // one to three numbers
      for (int a = 0; a < 3; ++a) {
        const char *peek = q;
        Tok n = next_token(peek, eol);
        if (!whole_number(n.p, n.e)) break;
        q = peek;
      }
      continue;
    }
    const char *ne = eol;
    while (ne > save && (ne[-1] == '\r' || ne[-1] == ' ' || ne[-1] == '\t' || ne[-1] == '\n')) --ne;
    std::string name(save, ne);
    for (char &c : name)
      if (c == '\\') c = '/';
    return name;
  }
}

// parse_mtl's records, their map_Kd names alone (the same order: one per
// newmtl); `word`: another map statement's instead (map_d, the cutouts')
void parse_mtl_maps(const char *p, const char *end, std::vector<std::string> *maps, const char *word = "map_Kd") {
  bool have = false;
  while (p < end) {
    const char *eol = (const char *)std::memchr(p, '\n', end - p);
    if (!eol) eol = end;
    const char *q = p;
    Tok key = next_token(q, eol);
    const std::string k(key.p, key.e);
    if (k == "newmtl") {
      maps->push_back(std::string());
      have = true;
    } else if (k == word && have) {
      maps->back() = map_name(q, eol);
    }
    p = eol + 1;
  }
}

int emit_maps(const std::vector<std::string> &maps, char *names, int64_t *n_bytes, int64_t *n_materials) {
  int64_t need = 0;
  for (const std::string &m : maps) need += (int64_t)m.size() + 1;
  if (names) {
    if (*n_bytes < need) return fail(MCPT_ERR_ARG, "mtl_maps: name buffer too small");
    char *w = names;
    for (const std::string &m : maps) {
      // (a name never holds '\0': an embedded one ends it here)
      const size_t l = std::strlen(m.c_str());
      std::memcpy(w, m.c_str(), l);
      w += l;
      *w++ = '\0';
    }
    need = (int64_t)(w - names);
  }
  *n_bytes = need;
  *n_materials = (int64_t)maps.size();
  return MCPT_OK;
}

}  // namespace

extern "C" int mcpt_obj_uvs_from_text(const char *text, int64_t len, float *uv, uint8_t *has, int64_t *n_tris) {
  if (!n_tris || len < 0 || (len > 0 && !text)) return fail(MCPT_ERR_ARG, "obj_uvs: bad argument");
  std::vector<double> coords;  // the vt records' (u, v), as parsed
  struct FaceT {
    long t[3];  // 0-based vt index per corner, -1: none
  };
  std::vector<FaceT> faces;
  std::vector<long> poly;
  const char *p = text, *end = text + len;
  while (p < end) {
    const char *eol = (const char *)std::memchr(p, '\n', end - p);
    if (!eol) eol = end;
    const char *q = p;
    while (q < eol && (*q == ' ' || *q == '\t')) ++q;
    if (q + 2 < eol && q[0] == 'v' && q[1] == 't' && (q[2] == ' ' || q[2] == '\t')) {
      q += 3;
      for (int k = 0; k < 2; ++k) {
        Tok t = next_token(q, eol);
        double v = 0.0;
        if (!parse_number(t.p, t.e, &v)) v = k == 0 ? NAN : 0.0;  // "vt u" alone is (u, 0); no u: not usable
        coords.push_back(v);
      }
    } else if (q + 1 < eol && q[0] == 'f' && (q[1] == ' ' || q[1] == '\t')) {
      q += 2;
      poly.clear();
      const long nvt = (long)(coords.size() / 2);
      for (;;) {
        Tok t = next_token(q, eol);
        if (t.p == t.e) break;
        long v = 0, vt = 0;
        if (corner_field(t.p, t.e, 0, &v) != 1 || v == 0) return fail(MCPT_ERR_PARSE, "obj_uvs: bad face index");  // as mcpt_load_obj
        const int got = corner_field(t.p, t.e, 1, &vt);
        if (got < 0 || (got == 1 && vt == 0)) return fail(MCPT_ERR_PARSE, "obj_uvs: bad vt index");
        if (got == 1 && (vt > nvt || (vt < 0 && vt < -nvt))) return fail(MCPT_ERR_PARSE, "obj_uvs: vt index out of range");
        poly.push_back(got == 0 ? -1 : (vt > 0 ? vt - 1 : nvt + vt));
      }
      if (poly.size() < 3) {
        p = eol + 1;
        continue;
      }
      for (size_t k = 1; k + 1 < poly.size(); ++k) faces.push_back(FaceT{{poly[0], poly[k], poly[k + 1]}});
    }
    p = eol + 1;
  }
  if (uv || has) {
    if (!uv || !has) return fail(MCPT_ERR_ARG, "obj_uvs: uv and has come together");
    if (*n_tris < (int64_t)faces.size()) return fail(MCPT_ERR_ARG, "obj_uvs: buffers too small");
    for (size_t i = 0; i < faces.size(); ++i) {
      bool ok = true;
      float out[6] = {0, 0, 0, 0, 0, 0};
      for (int k = 0; k < 3 && ok; ++k) {
        if (faces[i].t[k] < 0) {
          ok = false;
          break;
        }
        const double *c = &coords[2 * (size_t)faces[i].t[k]];
        out[2 * k] = (float)c[0], out[2 * k + 1] = (float)c[1];
        ok = std::isfinite(out[2 * k]) && std::isfinite(out[2 * k + 1]);
      }
      if (!ok) std::memset(out, 0, sizeof out);
      std::memcpy(uv + 6 * i, out, sizeof out);
      has[i] = ok ? 1 : 0;
    }
  }
  *n_tris = (int64_t)faces.size();
  return MCPT_OK;
}

extern "C" int mcpt_load_obj_uvs(const char *directory, const char *objname, float *uv, uint8_t *has, int64_t *n_tris) {
  if (!directory || !objname || !n_tris) return fail(MCPT_ERR_ARG, "load_obj_uvs: null argument");
  std::string dir(directory), text;
  if (!read_file(dir + objname, &text)) return fail(MCPT_ERR_IO, "load_obj_uvs: cannot read " + dir + objname);
  return mcpt_obj_uvs_from_text(text.data(), (int64_t)text.size(), uv, has, n_tris);
}

extern "C" int mcpt_mtl_maps_from_text(const char *text, int64_t len, char *names, int64_t *n_bytes,
                                       int64_t *n_materials) {
  if (!n_bytes || !n_materials || len < 0 || (len > 0 && !text)) return fail(MCPT_ERR_ARG, "mtl_maps: bad argument");
  std::vector<std::string> maps;
  parse_mtl_maps(text, text + len, &maps);
  return emit_maps(maps, names, n_bytes, n_materials);
}

namespace {
// mcpt_load_mtl_maps for the map statement `word`
int load_mtl_maps_of(const char *word, const char *directory, const char *objname, char *names, int64_t *n_bytes,
                     int64_t *n_materials) {
  if (!directory || !objname || !n_bytes || !n_materials) return fail(MCPT_ERR_ARG, "load_mtl_maps: null argument");
  std::string dir(directory), text;
  if (!read_file(dir + objname, &text)) return fail(MCPT_ERR_IO, "load_mtl_maps: cannot read " + dir + objname);
  std::vector<std::string> maps;
  const char *p = text.data(), *end = p + text.size();
  while (p < end) {  // mcpt_load_obj's mtllib rule: of each line, the first library that loads
    const char *eol = (const char *)std::memchr(p, '\n', end - p);
    if (!eol) eol = end;
    const char *q = p;
    while (q < eol && (*q == ' ' || *q == '\t')) ++q;
    if (eol - q >= 6 && std::strncmp(q, "mtllib", 6) == 0 && (q[6] == ' ' || q[6] == '\t')) {
      q += 7;
      for (;;) {
        Tok t = next_token(q, eol);
        if (t.p == t.e) break;
        std::string mt;
        if (read_file(dir + std::string(t.p, t.e), &mt)) {
          parse_mtl_maps(mt.data(), mt.data() + mt.size(), &maps, word);
          break;
        }
      }
    }
    p = eol + 1;
  }
  return emit_maps(maps, names, n_bytes, n_materials);
}
}  // namespace

extern "C" int mcpt_load_mtl_maps(const char *directory, const char *objname, char *names, int64_t *n_bytes,
                                  int64_t *n_materials) {
  return load_mtl_maps_of("map_Kd", directory, objname, names, n_bytes, n_materials);
}

// ------------------------------------------------ alpha cutouts (opt-in): map_d
extern "C" int mcpt_mtl_alpha_maps_from_text(const char *text, int64_t len, char *names, int64_t *n_bytes,
                                             int64_t *n_materials) {
  if (!n_bytes || !n_materials || len < 0 || (len > 0 && !text)) return fail(MCPT_ERR_ARG, "mtl_alpha_maps: bad argument");
  std::vector<std::string> maps;
  parse_mtl_maps(text, text + len, &maps, "map_d");
  return emit_maps(maps, names, n_bytes, n_materials);
}

extern "C" int mcpt_load_mtl_alpha_maps(const char *directory, const char *objname, char *names, int64_t *n_bytes,
                                        int64_t *n_materials) {
  return load_mtl_maps_of("map_d", directory, objname, names, n_bytes, n_materials);
}

// ------------------------------------------- bump and normal maps (opt-in)
namespace {

struct BumpMap {
  std::string name;
  int32_t kind = MCPT_BUMP_NONE;
  double bm = 1.0;
};

// parse_mtl's records, their norm / map_Bump / map_bump / bump lines alone (one
// per newmtl): `norm` wins over a height map whatever their order
void parse_mtl_bump_maps(const char *p, const char *end, std::vector<BumpMap> *maps) {
  bool have = false;
  while (p < end) {
    const char *eol = (const char *)std::memchr(p, '\n', end - p);
    if (!eol) eol = end;
    const char *q = p;
    Tok key = next_token(q, eol);
    const std::string k(key.p, key.e);
    if (k == "newmtl") {
      maps->push_back(BumpMap());
      have = true;
    } else if (have && (k == "norm" || k == "map_Bump" || k == "map_bump" || k == "bump")) {
      const int32_t kind = k == "norm" ? MCPT_BUMP_NORMAL : MCPT_BUMP_HEIGHT;
      BumpMap &m = maps->back();
      if (kind >= m.kind || m.name.empty()) {
        double bm = 1.0;
        const std::string name = map_name(q, eol, &bm);
        if (!name.empty()) m.name = name, m.kind = kind, m.bm = bm;
      }
    }
    p = eol + 1;
  }
}

int emit_bump_maps(const std::vector<BumpMap> &maps, char *names, int32_t *kinds, float *bm, int64_t *n_bytes,
                   int64_t *n_materials) {
  std::vector<std::string> ns;
  for (const BumpMap &m : maps) ns.push_back(m.name);
  if (names) {
    if (!kinds || !bm) return fail(MCPT_ERR_ARG, "mtl_bump_maps: names, kinds and bm come together");
    if (*n_materials < (int64_t)maps.size()) return fail(MCPT_ERR_ARG, "mtl_bump_maps: kinds and bm too small");
  }
  const int rc = emit_maps(ns, names, n_bytes, n_materials);
  if (rc != MCPT_OK) return rc;
  if (names)
    for (size_t i = 0; i < maps.size(); ++i) {
      const bool on = std::strlen(maps[i].name.c_str()) > 0;
      kinds[i] = on ? maps[i].kind : MCPT_BUMP_NONE;
      bm[i] = on ? (float)maps[i].bm : 1.0f;
    }
  return MCPT_OK;
}

}  // namespace

extern "C" int mcpt_mtl_bump_maps_from_text(const char *text, int64_t len, char *names, int32_t *kinds, float *bm,
                                            int64_t *n_bytes, int64_t *n_materials) {
  if (!n_bytes || !n_materials || len < 0 || (len > 0 && !text)) return fail(MCPT_ERR_ARG, "mtl_bump_maps: bad argument");
  std::vector<BumpMap> maps;
  parse_mtl_bump_maps(text, text + len, &maps);
  return emit_bump_maps(maps, names, kinds, bm, n_bytes, n_materials);
}

extern "C" int mcpt_load_mtl_bump_maps(const char *directory, const char *objname, char *names, int32_t *kinds, float *bm,
                                       int64_t *n_bytes, int64_t *n_materials) {
  if (!directory || !objname || !n_bytes || !n_materials) return fail(MCPT_ERR_ARG, "load_mtl_bump_maps: null argument");
  std::string dir(directory), text;
  if (!read_file(dir + objname, &text)) return fail(MCPT_ERR_IO, "load_mtl_bump_maps: cannot read " + dir + objname);
  std::vector<BumpMap> maps;
  const char *p = text.data(), *end = p + text.size();
  while (p < end) {  // mcpt_load_obj's mtllib rule: of each line, the first library that loads
    const char *eol = (const char *)std::memchr(p, '\n', end - p);
    if (!eol) eol = end;
    const char *q = p;
    while (q < eol && (*q == ' ' || *q == '\t')) ++q;
    if (eol - q >= 7 && std::strncmp(q, "mtllib", 6) == 0 && (q[6] == ' ' || q[6] == '\t')) {
      q += 7;
      for (;;) {
        Tok t = next_token(q, eol);
        if (t.p == t.e) break;
        std::string mt;
        if (read_file(dir + std::string(t.p, t.e), &mt)) {
          parse_mtl_bump_maps(mt.data(), mt.data() + mt.size(), &maps);
          break;
        }
      }
    }
    p = eol + 1;
  }
  return emit_bump_maps(maps, names, kinds, bm, n_bytes, n_materials);
}
