// mcpt_bump.h — bump and normal maps (opt-in, no reference counterpart): the
// shading normal of a hit, perturbed by a tangent-space normal map, as
// include/mcpt_hip.h defines it at mcpt_scene_set_normal_maps.  One expression
// tree, bump_normal, shared by k_render's mapped forms, k_primary_bump,
// k_intersect_bump and k_bump_eval (mcpt_bump.hip), so the four give the same
// bits for the same hit; every TU that includes this is built with the device
// flags of mcpt_device.hip.
#pragma once
#include <cstdint>

#include "../../include/mcpt_hip.h"
#include "mcpt_refmath.h"

namespace mcpt {

// A triangle's normal-map record in HBM: q[0] = (pool offset of its map's first
// texel as bits, width | height << 16 as bits, u0, v0), q[1] = (u1, v1, u2,
// v2), q[2] = (unit tangent t.xyz, handedness h = +-1).  Size bits 0: unmapped,
// the lookup reads q[0] alone and returns N.  48 B per triangle, indexed like
// the triangle array of the launch that reads it (reference ids, or tri4's
// slots with the 96-B nodes).
struct __attribute__((aligned(16))) BumpRec {
  f4 q[3];
};
static_assert(sizeof(BumpRec) == 48, "48-B normal-map record");

// What a kernel needs of a scene's normal maps: the records and the one pool
// of float4 texels ((mx, my, mz), .w unused; each map's rows top first).
// rec null: the scene has none (tested uniformly by the kernels that may run
// without).
struct BumpView {
  const BumpRec *rec;
  const f4 *texels;
  int64_t n_texels;  // (MCPT_DEBUG builds check the four texel indices against it)
};

#ifdef __HIPCC__
// The mapped shading normal at point pt (xyz) of a ray with direction d (xyz)
// on the triangle whose rows are v0, nab = -(v1 - v0), nac = -(v2 - v0), packed
// face normal ng and record V.rec[idx]; N is the normal that would be shaded
// without maps (ray-facing).  The caller bounds idx.
// The lookup of m is texture_factor's (mcpt_texture.h), restated over this
// pool: the same barycentrics, fma chains, wrap, clamps and the rule that a
// channel whose four texels are equal is that value exactly.  The fma order of
// the frame, fixed here once:
//   nt = dot(N, t) (cl_dot3); tp = fma(-nt, N, t) per component;
//   l2 = dot(tp, tp); T' = cl_normalize(tp);
//   B' = (h f) * cl_cross(N, T');
//   n = fma(mz, N, fma(my, B', mx * T')) per component; n' = cl_normalize(n).
// CHECK (MCPT_DEBUG builds): the texel indices and the record's extent are
// tested against the pool before use; a violation is counted in *viol and
// reads texel 0.  Without it they are in bounds by texture_factor's argument.
template <bool CHECK = false>
__device__ inline f4 bump_normal(const BumpView &V, int64_t idx, f3 v0, f3 nab, f3 nac, f3 ng, f4 pt, f4 d, f4 N,
                                 unsigned long long *viol = nullptr) {
  const f4 *__restrict__ q = V.rec[idx].q;
  const f4 q0 = q[0];
  const uint32_t size = as_u(q0.y);
  if (size == 0) return N;
  const f4 q1 = q[1];
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
  u = u - __builtin_floorf(u);  // every map repeats on both axes
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
  if constexpr (!CHECK) {  // (never moves an index: see texture_factor)
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
  float mx = __builtin_fmaf(w11, t11.x, __builtin_fmaf(w01, t01.x, __builtin_fmaf(w10, t10.x, w00 * t00.x)));
  float my = __builtin_fmaf(w11, t11.y, __builtin_fmaf(w01, t01.y, __builtin_fmaf(w10, t10.y, w00 * t00.y)));
  float mz = __builtin_fmaf(w11, t11.z, __builtin_fmaf(w01, t01.z, __builtin_fmaf(w10, t10.z, w00 * t00.z)));
  if (t00.x == t10.x && t00.x == t01.x && t00.x == t11.x) mx = t00.x;
  if (t00.y == t10.y && t00.y == t01.y && t00.y == t11.y) my = t00.y;
  if (t00.z == t10.z && t00.z == t01.z && t00.z == t11.z) mz = t00.z;
  if (mx == 0.0f && my == 0.0f) return N;  // straight up: the unmapped bits
  // the frame: the stored tangent made orthogonal to N (Gram-Schmidt), the
  // bitangent by the handedness and the side the ray sees
  const f4 q2 = q[2];
  const float f = cl_dot3(N.xyz, ng) < 0 ? -1.0f : 1.0f;
  const float nt = cl_dot3(N.xyz, q2.xyz);
  f4 tp;
  tp.x = __builtin_fmaf(-nt, N.x, q2.x);
  tp.y = __builtin_fmaf(-nt, N.y, q2.y);
  tp.z = __builtin_fmaf(-nt, N.z, q2.z);
  tp.w = 0.0f;
  const float l2 = cl_dot3(tp.xyz, tp.xyz);
  if (!(l2 > 0.0f && l2 < __builtin_inff())) return N;
  const f4 Tp = cl_normalize(tp);
  const float hf = q2.w * f;
  const f4 Bp = hf * cl_cross((f4){N.x, N.y, N.z, 0.0f}, Tp);
  f4 n;
  n.x = __builtin_fmaf(mz, N.x, __builtin_fmaf(my, Bp.x, mx * Tp.x));
  n.y = __builtin_fmaf(mz, N.y, __builtin_fmaf(my, Bp.y, mx * Tp.y));
  n.z = __builtin_fmaf(mz, N.z, __builtin_fmaf(my, Bp.z, mx * Tp.z));
  n.w = 0.0f;
  const float n2 = cl_dot3(n.xyz, n.xyz);
  if (!(n2 > 0.0f && n2 < __builtin_inff())) return N;
  n = cl_normalize(n);
  if (!(__builtin_fabsf(n.x) < __builtin_inff() && __builtin_fabsf(n.y) < __builtin_inff() &&
        __builtin_fabsf(n.z) < __builtin_inff()))
    return N;
  if (!(cl_dot3(n.xyz, d.xyz) < 0)) return N;  // turned away from the viewer
  n.w = N.w;
  return n;
}
#endif

// mcpt_device.hip (the opaque handles are defined there): what k_bump_eval
// needs of a scene; *on = 0 when it has no normal maps.  tris: the scene's 64-B
// triangle records, the map records in the same (reference) order.
struct BumpScene {
  const f4 *tris;
  BumpView bump;
  int64_t n_tris;
};
int bump_scene(const mcpt_scene *scene, BumpScene *out, int *on, int *device);

}  // namespace mcpt
