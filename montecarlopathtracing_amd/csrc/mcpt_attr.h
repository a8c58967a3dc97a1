// mcpt_attr.h — the host half of the per-triangle image attributes (diffuse textures,
// mcpt_scene_set_textures; normal maps, mcpt_scene_set_normal_maps): where each image lies in
// the one texel pool, the range checks of the per-triangle index and uv, the texels, and the
// records of mcpt_texture.h (TexRec) and mcpt_bump.h (BumpRec).  Float and double arithmetic, no
// HIP header: it is checked on the CPU (tests/native/attr_check.cpp).  A check returns the
// message of the first rule an input breaks, whole as the setter reports it, or "" for none; the
// setters call them in this file's order, so what they validate first stays what it was.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcpt_hip.h"

namespace mcpt {

using Quad = std::array<float, 4>;  // one float4 of a record or a texel, as the device reads it
using TexRecHost = std::array<Quad, 2>;   // TexRec's bytes
using BumpRecHost = std::array<Quad, 3>;  // BumpRec's bytes

constexpr int32_t kAttrMaxSide = 16384;          // an image's width and height: 1..kAttrMaxSide (14 bits of the record's 16)
constexpr int64_t kAttrMaxTexels = 1ll << 27;    // all images of one set: the record's offset is 32 bits
constexpr float kAttrMaxUv = 1048576.0f;         // |u|, |v| <= 2^20: u - floor(u) stays in [0, 1] (texture_factor)

// How a setter names itself and its images in a message: {"set_textures", "texture"}, {"set_normal_maps", "map"}.
struct AttrNames {
  const char *who, *image;
};

// Each image's first texel in the pool (base) and the pool's size; the sizes alone, before a texel is read.
// Image: mcpt_texture_image or mcpt_normal_map_image, `texels` its pointer member.
template <class Image>
inline std::string pool_layout(const AttrNames &nm, const Image *images, int32_t n_images, const float *Image::*texels,
                               std::vector<int64_t> &base, int64_t *total) {
  base.resize((size_t)n_images);
  *total = 0;
  for (int32_t k = 0; k < n_images; ++k) {
    const Image &im = images[k];
    if (!(im.*texels) || im.width < 1 || im.width > kAttrMaxSide || im.height < 1 || im.height > kAttrMaxSide)
      return std::string(nm.who) + ": " + nm.image + " " + std::to_string(k) + " has no texels or a side outside 1..16384";
    base[(size_t)k] = *total;
    *total += (int64_t)im.width * im.height;
    if (*total > kAttrMaxTexels) return std::string(nm.who) + ": more than 2^27 texels in all";
  }
  return "";
}

// Every triangle's image index in -1..n_images-1, and the six uv values of a triangle that has an image
// finite and within kAttrMaxUv (a triangle without one may carry anything).
inline std::string check_index_uv(const AttrNames &nm, const int32_t *index, const float *uv, int64_t n_tris, int32_t n_images) {
  for (int64_t i = 0; i < n_tris; ++i) {
    const int32_t t = index[i];
    if (t < -1 || t >= n_images)
      return std::string(nm.who) + ": " + nm.image + " index out of range (triangle " + std::to_string(i) + ")";
    for (int k = 0; k < 6 && t >= 0; ++k)
      if (!(std::fabs(uv[6 * i + k]) <= kAttrMaxUv))
        return std::string(nm.who) + ": a texture coordinate is not finite or beyond 2^20 (triangle " + std::to_string(i) + ")";
  }
  return "";
}

// The pool: every image's texels at its base, each made by rule(x, y, z, &texel), which returns false for a
// texel the setter refuses (`refused` then ends the message); texel 0 of a set without images is `first`.
template <class Image, class Rule>
inline std::string pack_pool(const AttrNames &nm, const Image *images, int32_t n_images, const float *Image::*texels,
                             const std::vector<int64_t> &base, int64_t total, Quad first, Rule rule, const char *refused,
                             std::vector<Quad> &pool) {
  pool.resize((size_t)(total > 1 ? total : 1));
  pool[0] = first;
  for (int32_t k = 0; k < n_images; ++k) {
    const Image &im = images[k];
    const float *px = im.*texels;
    const int64_t m = (int64_t)im.width * im.height;
    for (int64_t j = 0; j < m; ++j)
      if (!rule(px[3 * j], px[3 * j + 1], px[3 * j + 2], &pool[(size_t)(base[(size_t)k] + j)]))
        return std::string(nm.who) + ": " + nm.image + " " + std::to_string(k) + " " + refused;
  }
  return "";
}

// a texture's texel: rgb finite and >= 0, opaque (.w = 1) until an alpha is set
inline bool texture_texel(float r, float g, float b, Quad *out) {
  *out = {r, g, b, 1.0f};
  return r >= 0.0f && r < INFINITY && g >= 0.0f && g < INFINITY && b >= 0.0f && b < INFINITY;
}
// a normal map's texel: unit within 1e-3 and on the surface's outer side
inline bool normal_map_texel(float x, float y, float z, Quad *out) {
  *out = {x, y, z, 0.0f};
  const double len = std::sqrt((double)x * x + (double)y * y + (double)z * z);
  return std::fabs(len - 1.0) <= 1e-3 && z > 0.0f;
}

inline float bits_as_float(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// q[0] and q[1] of either record: where the image lies, its size, and the triangle's six uv values
inline void pack_lookup(Quad *q, int64_t base, int32_t width, int32_t height, const float *uv) {
  const uint32_t off = (uint32_t)base, size = (uint32_t)width | ((uint32_t)height << 16);
  q[0] = {bits_as_float(off), bits_as_float(size), uv[0], uv[1]};
  q[1] = {uv[2], uv[3], uv[4], uv[5]};
}

// The texture records: zeros for a triangle without a texture.
template <class Image>
inline std::vector<TexRecHost> pack_tex_records(const Image *images, const std::vector<int64_t> &base, const int32_t *index,
                                                const float *uv, int64_t n_tris) {
  std::vector<TexRecHost> rec((size_t)n_tris, TexRecHost{});
  for (int64_t i = 0; i < n_tris; ++i) {
    const int32_t t = index[i];
    if (t >= 0) pack_lookup(rec[(size_t)i].data(), base[(size_t)t], images[t].width, images[t].height, uv + 6 * i);
  }
  return rec;
}

// q[2] of a BumpRec: the unit tangent (the direction of growing u) and the handedness of the uv frame,
// in double from the uploaded triangle rows (16 floats: v0, nab = -(v1 - v0), nac = -(v2 - v0), aux; the
// packed face normal in the first three rows' .w).  False for degenerate UVs: the triangle stays unmapped.
inline bool tangent_frame(const float *rows, const float *u, Quad *out) {
  const double e1[3] = {-(double)rows[4], -(double)rows[5], -(double)rows[6]};
  const double e2[3] = {-(double)rows[8], -(double)rows[9], -(double)rows[10]};
  const double ng[3] = {rows[3], rows[7], rows[11]};
  const double du1 = (double)u[2] - u[0], dv1 = (double)u[3] - u[1];
  const double du2 = (double)u[4] - u[0], dv2 = (double)u[5] - u[1];
  const double det = du1 * dv2 - du2 * dv1;
  if (!(det != 0.0 && std::isfinite(det))) return false;
  double Tn[3], Bn[3];
  for (int k = 0; k < 3; ++k) Tn[k] = (dv2 * e1[k] - dv1 * e2[k]) / det, Bn[k] = (du1 * e2[k] - du2 * e1[k]) / det;
  const double tl = std::sqrt(Tn[0] * Tn[0] + Tn[1] * Tn[1] + Tn[2] * Tn[2]);
  if (!(tl > 0.0 && std::isfinite(tl))) return false;
  const double c[3] = {ng[1] * Tn[2] - ng[2] * Tn[1], ng[2] * Tn[0] - ng[0] * Tn[2], ng[0] * Tn[1] - ng[1] * Tn[0]};
  const float h = c[0] * Bn[0] + c[1] * Bn[1] + c[2] * Bn[2] >= 0.0 ? 1.0f : -1.0f;
  *out = {(float)(Tn[0] / tl), (float)(Tn[1] / tl), (float)(Tn[2] / tl), h};
  return true;
}

// The normal-map records: zeros for a triangle without a map or with degenerate UVs.  tri_rows: the
// scene's 64-B triangle records, 16 floats each.
template <class Image>
inline std::vector<BumpRecHost> pack_bump_records(const Image *images, const std::vector<int64_t> &base, const int32_t *index,
                                                  const float *uv, const float *tri_rows, int64_t n_tris) {
  std::vector<BumpRecHost> rec((size_t)n_tris, BumpRecHost{});
  for (int64_t i = 0; i < n_tris; ++i) {
    const int32_t t = index[i];
    Quad frame;
    if (t < 0 || !tangent_frame(tri_rows + 16 * i, uv + 6 * i, &frame)) continue;
    BumpRecHost &r = rec[(size_t)i];
    pack_lookup(r.data(), base[(size_t)t], images[t].width, images[t].height, uv + 6 * i);
    r[2] = frame;
  }
  return rec;
}

}  // namespace mcpt
