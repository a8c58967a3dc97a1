// mcpt_texture.h — diffuse texture maps (opt-in, no reference counterpart): the
// factor on a material's kd at a hit, as include/mcpt_hip.h defines it at
// mcpt_scene_set_textures.  One expression tree, texture_factor, shared by
// k_render's textured forms, k_primary_tex, k_shade_tex and k_texture_eval
// (mcpt_texture.hip), so the four give the same bits for the same hit; every
// TU that includes this is built with the device flags of mcpt_device.hip.
#pragma once
#include <cstdint>

#include "../../include/mcpt_hip.h"
#include "mcpt_refmath.h"

namespace mcpt {

// A triangle's texture record in HBM: q[0] = (pool offset of its texture's
// first texel as bits, width | height << 16 as bits, u0, v0), q[1] = (u1, v1,
// u2, v2).  Size bits 0: no texture, the lookup reads q[0] alone and returns
// ones.  The record carries where its texture lies, so resolving it adds no
// dependent load.  32 B per triangle, indexed like the triangle array of the
// launch that reads it (reference ids, or tri4's slots with the 96-B nodes).
struct __attribute__((aligned(16))) TexRec {
  f4 q[2];
};
static_assert(sizeof(TexRec) == 32, "32-B texture record");

// What a kernel needs of a scene's textures: the records and the one pool of
// float4 texels (rgb, .w the alpha of mcpt_scene_set_texture_alpha, 1.0f
// without one; each texture's rows top first).
struct TexView {
  const TexRec *rec;
  const f4 *texels;
  int64_t n_texels;  // (MCPT_DEBUG builds check the four texel indices against it)
};

#ifdef __HIPCC__
// kd's factor (xyz) and the cutout alpha (.w: the same bilinear, repeating
// lookup on the texels' .w, the same weights and fma order; 1 on an untextured
// triangle and exactly 1.0f on a texture without an alpha image) at point pt (xyz) on the triangle whose rows are v0, nab = -(v1 -
// v0), nac = -(v2 - v0) (DevTri's, or formed the same way from the quantized
// path's vertices) and texture record V.rec[idx].  The caller bounds idx.
// CHECK (MCPT_DEBUG builds): the texel indices are tested against the pool
// before use; a violation is counted in *viol and reads texel 0.  Without it
// they are in bounds by construction: the barycentrics are clamped to [0, 1]
// (a NaN point gives 0) and |uv| <= 2^20, so u - floor(u) lies in [0, 1], x in
// [-0.5, W - 0.5], i0 = floor(x) in [-1, W - 1]; one wrap step each way and a
// clamp bring every column and row into the texture, whose texels the setter
// placed inside the pool.
template <bool CHECK = false>
__device__ inline f4 texture_factor(const TexView &V, int64_t idx, f3 v0, f3 nab, f3 nac, f4 pt,
                                    unsigned long long *viol = nullptr) {
  const f4 *__restrict__ q = V.rec[idx].q;
  const f4 q0 = q[0];
  const uint32_t size = as_u(q0.y);
  if (size == 0) return (f4){1.0f, 1.0f, 1.0f, 1.0f};
  const f4 q1 = q[1];
  // the barycentrics of shading_normal (mcpt_smooth.h), restated: the same
  // rows, fmas, one v_rcp_f32 and clamps
  const f3 w = pt.xyz - v0;
  const float d11 = cl_dot3(nab, nab), d12 = cl_dot3(nab, nac), d22 = cl_dot3(nac, nac);
  const float w1 = -cl_dot3(w, nab), w2 = -cl_dot3(w, nac);
  const float den = __builtin_fmaf(d11, d22, -(d12 * d12));
  const float rden = __builtin_amdgcn_rcpf(den);
  float b1 = __builtin_fmaf(d22, w1, -(d12 * w2)) * rden;
  float b2 = __builtin_fmaf(d11, w2, -(d12 * w1)) * rden;
  b1 = __builtin_fminf(__builtin_fmaxf(b1, 0.0f), 1.0f);
  b2 = __builtin_fminf(__builtin_fmaxf(b2, 0.0f), 1.0f);
  if (!(den != 0.0f && __builtin_fabsf(den) < __builtin_inff())) b1 = b2 = 0.0f;  // a sliver: corner 0's uv
  const float b0 = __builtin_fmaxf((1.0f - b1) - b2, 0.0f);
  float u = __builtin_fmaf(b2, q1.z, __builtin_fmaf(b1, q1.x, b0 * q0.z));
  float v = __builtin_fmaf(b2, q1.w, __builtin_fmaf(b1, q1.y, b0 * q0.w));
  u = u - __builtin_floorf(u);  // every texture repeats on both axes
  v = v - __builtin_floorf(v);
  const int32_t tw = (int32_t)(size & 0xFFFFu), th = (int32_t)(size >> 16);
  const float x = __builtin_fmaf(u, (float)tw, -0.5f);
  const float y = __builtin_fmaf(1.0f - v, (float)th, -0.5f);  // OBJ's v axis points up, row 0 is the top
  const float xf = __builtin_floorf(x), yf = __builtin_floorf(y);
  const float fx = x - xf, fy = y - yf;
  int32_t i0 = (int32_t)xf, j0 = (int32_t)yf;
  int32_t i1 = i0 + 1, j1 = j0 + 1;
  i0 = i0 < 0 ? i0 + tw : i0, j0 = j0 < 0 ? j0 + th : j0;  // columns and rows wrap
  i1 = i1 >= tw ? i1 - tw : i1, j1 = j1 >= th ? j1 - th : j1;
  if constexpr (!CHECK) {  // (never moves an index: see above)
    i0 = min(max(i0, 0), tw - 1), i1 = min(max(i1, 0), tw - 1);
    j0 = min(max(j0, 0), th - 1), j1 = min(max(j1, 0), th - 1);
  }
  const int64_t base = (int64_t)as_u(q0.x);
  int64_t k00 = base + (int64_t)j0 * tw + i0, k10 = base + (int64_t)j0 * tw + i1;
  int64_t k01 = base + (int64_t)j1 * tw + i0, k11 = base + (int64_t)j1 * tw + i1;
  if constexpr (CHECK) {
    const bool ok = i0 >= 0 && i0 < tw && i1 >= 0 && i1 < tw && j0 >= 0 && j0 < th && j1 >= 0 && j1 < th &&
                    base + (int64_t)tw * th <= V.n_texels;
    if (!ok) {
      atomicAdd(viol, 1ull);
      k00 = k10 = k01 = k11 = 0;
    }
  }
  const f4 t00 = V.texels[k00], t10 = V.texels[k10], t01 = V.texels[k01], t11 = V.texels[k11];
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
  f4 r;
  r.x = __builtin_fmaf(w11, t11.x, __builtin_fmaf(w01, t01.x, __builtin_fmaf(w10, t10.x, w00 * t00.x)));
  r.y = __builtin_fmaf(w11, t11.y, __builtin_fmaf(w01, t01.y, __builtin_fmaf(w10, t10.y, w00 * t00.y)));
  r.z = __builtin_fmaf(w11, t11.z, __builtin_fmaf(w01, t01.z, __builtin_fmaf(w10, t10.z, w00 * t00.z)));
  // the four fp32 weights sum to 1 only within an ulp: a channel whose four
  // texels are equal is that value exactly (so a texture of ones is 1.0f)
  if (t00.x == t10.x && t00.x == t01.x && t00.x == t11.x) r.x = t00.x;
  if (t00.y == t10.y && t00.y == t01.y && t00.y == t11.y) r.y = t00.y;
  if (t00.z == t10.z && t00.z == t01.z && t00.z == t11.z) r.z = t00.z;
  r.w = __builtin_fmaf(w11, t11.w, __builtin_fmaf(w01, t01.w, __builtin_fmaf(w10, t10.w, w00 * t00.w)));
  if (t00.w == t10.w && t00.w == t01.w && t00.w == t11.w) r.w = t00.w;
  return r;
}
#endif

// mcpt_device.hip (the opaque handles are defined there): what k_texture_eval
// needs of a scene; *on = 0 when it has no textures.  tris: the scene's 64-B
// triangle records, the texture records in the same (reference) order.
struct TextureScene {
  const f4 *tris;
  TexView tex;
  int64_t n_tris;
};
int texture_scene(const mcpt_scene *scene, TextureScene *out, int *on, int *device);

}  // namespace mcpt
