// attr_check.cpp — TEST INFRASTRUCTURE.  The host half of the texture and
// normal-map setters (csrc/mcpt_attr.h: the pool layout, the index and uv range
// checks, the texel rules, TexRec and BumpRec packing) under AddressSanitizer +
// UndefinedBehaviorSanitizer (built with -fsanitize=address,undefined and run
// by tests/test_texture_cpu.py, on the CPU).  Every rejected input the setters
// document, with the message they report, and one valid two-triangle,
// two-image set whose packed fields are compared with the layouts written in
// csrc/mcpt_texture.h and csrc/mcpt_bump.h.  Every input lives in a heap block
// of exactly its size, so a read past it is a sanitizer report.
//   attr_asan
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../montecarlopathtracing_amd/csrc/mcpt_attr.h"

namespace {

using namespace mcpt;

int failures = 0;

void expect(bool ok, const std::string &what) {
  if (!ok) {
    ++failures;
    std::printf("FAIL %s\n", what.c_str());
  }
}

template <class T>
std::unique_ptr<T[]> exact(std::initializer_list<T> v) {
  std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
  size_t i = 0;
  for (const T &x : v) p[i++] = x;
  return p;
}

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

const AttrNames kTex = {"set_textures", "texture"}, kMap = {"set_normal_maps", "map"};

// one image of w x h over `px` (which the layout never reads)
std::string layout_of(const float *px, int32_t w, int32_t h) {
  const auto im = exact<mcpt_texture_image>({{px, w, h}});
  std::vector<int64_t> base;
  int64_t total = -1;
  return pool_layout(kTex, im.get(), 1, &mcpt_texture_image::rgb, base, &total);
}

std::string index_uv(int32_t t0, int32_t t1, float bad_uv, int at) {
  const auto idx = exact<int32_t>({t0, t1});
  auto uv = exact<float>({0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1});
  if (at >= 0) uv[at] = bad_uv;
  return check_index_uv(kTex, idx.get(), uv.get(), 2, 2);
}

std::string texture_pool(float r, float g, float b) {
  const auto px = exact<float>({0.5f, 0.5f, 0.5f, r, g, b});
  const auto im = exact<mcpt_texture_image>({{px.get(), 2, 1}});
  std::vector<int64_t> base;
  int64_t total = 0;
  std::vector<Quad> pool;
  if (!pool_layout(kTex, im.get(), 1, &mcpt_texture_image::rgb, base, &total).empty()) return "layout";
  return pack_pool(kTex, im.get(), 1, &mcpt_texture_image::rgb, base, total, {0, 0, 0, 0}, texture_texel,
                   "has a negative or non-finite texel", pool);
}

std::string map_pool(float x, float y, float z) {
  const auto px = exact<float>({0.0f, 0.0f, 1.0f, x, y, z});
  const auto im = exact<mcpt_normal_map_image>({{px.get(), 1, 2}});
  std::vector<int64_t> base;
  int64_t total = 0;
  std::vector<Quad> pool;
  if (!pool_layout(kMap, im.get(), 1, &mcpt_normal_map_image::xyz, base, &total).empty()) return "layout";
  return pack_pool(kMap, im.get(), 1, &mcpt_normal_map_image::xyz, base, total, {0, 0, 1, 0}, normal_map_texel,
                   "has a texel that is not unit or has z <= 0", pool);
}

}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const auto one = exact<float>({0.0f, 0.0f, 1.0f});
  const std::string side = "set_textures: texture 0 has no texels or a side outside 1..16384";

  // ---- the sizes: a null image, a side of 0 or 16385, more than 2^27 texels
  expect(layout_of(nullptr, 1, 1) == side, "a null image");
  expect(layout_of(one.get(), 0, 1) == side && layout_of(one.get(), 1, 0) == side, "a side of 0");
  expect(layout_of(one.get(), 16385, 1) == side && layout_of(one.get(), 1, 16385) == side, "a side of 16385");
  expect(layout_of(one.get(), -1, 1) == side, "a negative side");
  expect(layout_of(one.get(), 16384, 1).empty() && layout_of(one.get(), 1, 1).empty(), "sides of 1 and 16384");
  {
    // 2^24 texels each: eight fill the pool exactly, the ninth is one too many (no texel is read)
    std::unique_ptr<mcpt_normal_map_image[]> im(new mcpt_normal_map_image[9]);
    for (int k = 0; k < 9; ++k) im[k] = {one.get(), 16384, 1024};
    std::vector<int64_t> base;
    int64_t total = 0;
    expect(pool_layout(kMap, im.get(), 8, &mcpt_normal_map_image::xyz, base, &total).empty() && total == (1ll << 27) &&
               base.size() == 8 && base[7] == 7ll << 24,
           "2^27 texels fit");
    expect(pool_layout(kMap, im.get(), 9, &mcpt_normal_map_image::xyz, base, &total) == "set_normal_maps: more than 2^27 texels in all",
           "a pool over 2^27 texels");
    im[3].xyz = nullptr;
    expect(pool_layout(kMap, im.get(), 8, &mcpt_normal_map_image::xyz, base, &total) ==
               "set_normal_maps: map 3 has no texels or a side outside 1..16384",
           "the map's name and number");
    expect(pool_layout(kMap, im.get(), 0, &mcpt_normal_map_image::xyz, base, &total).empty() && total == 0 && base.empty(),
           "no images");
  }

  // ---- the index and the uv values
  expect(index_uv(-1, 1, 0, -1).empty() && index_uv(0, 0, 1048576.0f, 3).empty() && index_uv(0, 0, -1048576.0f, 11).empty(),
         "indices -1..n-1 and |uv| = 2^20 pass");
  expect(index_uv(-2, 0, 0, -1) == "set_textures: texture index out of range (triangle 0)", "an index of -2");
  expect(index_uv(0, 2, 0, -1) == "set_textures: texture index out of range (triangle 1)", "an index of n");
  const std::string coord = "set_textures: a texture coordinate is not finite or beyond 2^20 (triangle 1)";
  expect(index_uv(0, 1, nan, 6) == coord && index_uv(0, 1, inf, 8) == coord, "a uv value that is NaN or infinite");
  expect(index_uv(0, 1, 1048577.0f, 11) == coord && index_uv(0, 1, -1048577.0f, 7) == coord, "a uv value of 2^20 + 1");
  expect(index_uv(0, -1, nan, 9).empty(), "a triangle without an image may carry any uv");
  {
    const auto idx = exact<int32_t>({1});
    const auto uv = exact<float>({0, 0, 1, 0, 0, 1});
    expect(check_index_uv(kMap, idx.get(), uv.get(), 1, 1) == "set_normal_maps: map index out of range (triangle 0)",
           "the map's name");
    expect(check_index_uv(kMap, idx.get(), uv.get(), 0, 0).empty(), "no triangles");
  }

  // ---- the texels
  const std::string texel = "set_textures: texture 0 has a negative or non-finite texel";
  expect(texture_pool(0.0f, 1.0f, 3.0e38f).empty(), "texels of 0 and up pass");
  expect(texture_pool(-1e-30f, 0, 0) == texel && texture_pool(0, 0, -1) == texel, "a negative texel");
  expect(texture_pool(0, inf, 0) == texel && texture_pool(nan, 0, 0) == texel, "an infinite or NaN texel");
  const std::string unit = "set_normal_maps: map 0 has a texel that is not unit or has z <= 0";
  expect(map_pool(0.6f, 0.0f, 0.8f).empty() && map_pool(0.0f, 0.0f, 1.0009f).empty(), "unit texels within 1e-3 pass");
  expect(map_pool(0.6f, 0.0f, 0.81f) == unit && map_pool(0, 0, 0.99f) == unit && map_pool(nan, 0, 1) == unit, "a non-unit texel");
  expect(map_pool(1.0f, 0.0f, 0.0f) == unit && map_pool(0.6f, 0.0f, -0.8f) == unit, "a texel with z <= 0");

  // ---- one valid set: two triangles, two images (2 x 1 and 3 x 2)
  {
    const auto px0 = exact<float>({0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f});
    std::unique_ptr<float[]> px1(new float[18]);
    for (int k = 0; k < 18; ++k) px1[k] = 1.0f + (float)k;
    const auto im = exact<mcpt_texture_image>({{px0.get(), 2, 1}, {px1.get(), 3, 2}});
    const auto idx = exact<int32_t>({1, 0});
    const auto uv = exact<float>({0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f, 0.25f, -3.0f, 7.5f, 0.5f, 2.0f, 1048576.0f});
    std::vector<int64_t> base;
    int64_t total = 0;
    std::vector<Quad> pool;
    expect(pool_layout(kTex, im.get(), 2, &mcpt_texture_image::rgb, base, &total).empty() && total == 8 && base[0] == 0 && base[1] == 2,
           "valid: the layout");
    expect(check_index_uv(kTex, idx.get(), uv.get(), 2, 2).empty(), "valid: the ranges");
    expect(pack_pool(kTex, im.get(), 2, &mcpt_texture_image::rgb, base, total, {0, 0, 0, 0}, texture_texel, "", pool).empty() &&
               pool.size() == 8 && pool[1] == Quad{0.4f, 0.5f, 0.6f, 1.0f} && pool[2] == Quad{1.0f, 2.0f, 3.0f, 1.0f} &&
               pool[7] == Quad{16.0f, 17.0f, 18.0f, 1.0f},
           "valid: texels at their base, opaque");
    const std::vector<TexRecHost> rec = pack_tex_records(im.get(), base, idx.get(), uv.get(), 2);
    // q[0] = (pool offset as bits, width | height << 16 as bits, u0, v0), q[1] = (u1, v1, u2, v2)
    expect(rec.size() == 2 && bits(rec[0][0][0]) == 2u && bits(rec[0][0][1]) == (3u | (2u << 16)) && rec[0][0][2] == 0.0f &&
               rec[0][0][3] == 0.0f && rec[0][1] == Quad{1.0f, 0.0f, 0.0f, 1.0f},
           "valid: TexRec of triangle 0");
    expect(bits(rec[1][0][0]) == 0u && bits(rec[1][0][1]) == (2u | (1u << 16)) && rec[1][0][2] == 0.25f && rec[1][0][3] == -3.0f &&
               rec[1][1] == Quad{7.5f, 0.5f, 2.0f, 1048576.0f},
           "valid: TexRec of triangle 1");
    {
      const auto none = exact<int32_t>({-1, -1});
      const std::vector<TexRecHost> r0 = pack_tex_records(im.get(), base, none.get(), uv.get(), 2);
      expect(r0[0] == TexRecHost{} && r0[1] == TexRecHost{}, "an untextured triangle's record is zeros");
    }

    // the same set as normal maps on two triangles in the plane z = 0: rows v0, nab = -(v1 - v0), nac = -(v2 - v0),
    // aux, the face normal (0, 0, 1) in the first three rows' .w.  Triangle 1's UVs are mirrored.
    const auto mx0 = exact<float>({0.0f, 0.0f, 1.0f, 0.6f, 0.0f, 0.8f});
    std::unique_ptr<float[]> mx1(new float[18]);
    for (int k = 0; k < 6; ++k) mx1[3 * k] = 0.0f, mx1[3 * k + 1] = 0.6f, mx1[3 * k + 2] = 0.8f;
    const auto maps = exact<mcpt_normal_map_image>({{mx0.get(), 2, 1}, {mx1.get(), 3, 2}});
    const auto rows = exact<float>({0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 1, 9, 9, 9, 9,     // (0,0,0) (1,0,0) (0,1,0)
                                    2, 0, 0, 0, -2, 0, 0, 0, 0, -2, 0, 1, 9, 9, 9, 9});   // (2,0,0) (4,0,0) (2,2,0)
    const auto muv = exact<float>({0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 0.0f});
    expect(pack_pool(kMap, maps.get(), 2, &mcpt_normal_map_image::xyz, base, total, {0, 0, 1, 0}, normal_map_texel, "", pool).empty() &&
               pool[1] == Quad{0.6f, 0.0f, 0.8f, 0.0f} && pool[7] == Quad{0.0f, 0.6f, 0.8f, 0.0f},
           "valid: map texels at their base");
    const std::vector<BumpRecHost> br = pack_bump_records(maps.get(), base, idx.get(), muv.get(), rows.get(), 2);
    // q[0], q[1] as TexRec's, q[2] = (unit tangent, handedness)
    expect(br.size() == 2 && bits(br[0][0][0]) == 2u && bits(br[0][0][1]) == (3u | (2u << 16)) && br[0][1] == Quad{1.0f, 0.0f, 0.0f, 1.0f} &&
               br[0][2] == Quad{1.0f, 0.0f, 0.0f, 1.0f},
           "valid: BumpRec of triangle 0: tangent +x, right-handed");
    expect(bits(br[1][0][0]) == 0u && bits(br[1][0][1]) == (2u | (1u << 16)) && br[1][1] == Quad{0.0f, 1.0f, 1.0f, 0.0f} &&
               br[1][2] == Quad{0.0f, 1.0f, 0.0f, -1.0f},
           "valid: BumpRec of triangle 1: tangent +y, mirrored");

    // ---- degenerate UVs: the triangle stays unmapped (a record of zeros)
    for (const auto &d : {exact<float>({0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0, 0, 1, 0, 0, 1}),    // one point
                          exact<float>({0.0f, 0.0f, 1.0f, 1.0f, 2.0f, 2.0f, 0, 0, 1, 0, 0, 1}),    // on a line
                          exact<float>({0.0f, 0.0f, 3e-30f, 0.0f, 0.0f, 3e-30f, 0, 0, 1, 0, 0, 1})}) {  // det underflows in float, not in double
      const std::vector<BumpRecHost> r = pack_bump_records(maps.get(), base, idx.get(), d.get(), rows.get(), 2);
      const bool tiny = d[2] == 3e-30f;
      expect((r[0] == BumpRecHost{}) == !tiny && !(r[1] == BumpRecHost{}), tiny ? "tiny UVs keep their frame" : "degenerate UVs");
    }
    Quad q;
    const auto flat = exact<float>({0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 9, 9, 9, 9});  // a triangle of one point: no tangent
    expect(!tangent_frame(flat.get(), muv.get(), &q), "a zero tangent");
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
