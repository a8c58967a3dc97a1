// mcpt_smooth.h — smooth shading (opt-in, no reference counterpart): the
// shading normal of a hit, interpolated from the scene's vertex normals, as
// include/mcpt_hip.h defines it at mcpt_scene_set_vertex_normals.  One
// expression tree, shading_normal, shared by k_render's S phase, k_primary,
// k_intersect and k_shading_normals (mcpt_smooth.hip), so the four give the
// same bits for the same hit; every TU that includes this is built with the
// device flags of mcpt_device.hip.
#pragma once
#include <cstdint>

#include "../../include/mcpt_hip.h"
#include "mcpt_refmath.h"

namespace mcpt {

// A triangle's vertex normals in HBM: three 16-B quads (n0, n1, n2 in .xyz).
// q[0].w = 1.0f marks a flat triangle (all three bit-equal to the packed
// normal): the lookup then reads that one quad and returns the reference's
// flipped face normal.  48 B per triangle, indexed like the triangle array of
// the launch that reads it (reference ids, or tri4's slots with the 96-B nodes).
struct __attribute__((aligned(16))) VtxNormals {
  f4 q[3];
};
static_assert(sizeof(VtxNormals) == 48, "48-B vertex normals");

#ifdef __HIPCC__
// The shading normal at point pt (xyz) of a ray with direction d (xyz) on the
// triangle whose rows are v0, nab = -(v1 - v0), nac = -(v2 - v0) (DevTri's, or
// formed the same way from the quantized path's vertices), packed normal ng
// and vertex normals vn[idx].  The caller bounds idx.  Returns .w = +-0.
__device__ inline f4 shading_normal(const VtxNormals *__restrict__ vn, int64_t idx, f3 v0, f3 nab, f3 nac, f3 ng,
                                    f4 pt, f4 d) {
  f4 ngf = (f4){ng.x, ng.y, ng.z, 0.0f};
  if (cl_dot3(d.xyz, ngf.xyz) > 0) ngf = -ngf;  // intersect.cl:23-25
  const f4 *__restrict__ q = vn[idx].q;
  const f4 n0 = q[0];
  if (n0.w != 0.0f) return ngf;  // flat: the bits of a scene without vertex normals
  const f4 n1 = q[1], n2 = q[2];
  // barycentrics of pt from the stored rows: e1 = -nab, e2 = -nac, so the
  // products of two rows keep their sign and w . e = -(w . row)
  const f3 w = pt.xyz - v0;
  const float d11 = cl_dot3(nab, nab), d12 = cl_dot3(nab, nac), d22 = cl_dot3(nac, nac);
  const float w1 = -cl_dot3(w, nab), w2 = -cl_dot3(w, nac);
  const float den = __builtin_fmaf(d11, d22, -(d12 * d12));
  const float rden = __builtin_amdgcn_rcpf(den);
  float b1 = __builtin_fmaf(d22, w1, -(d12 * w2)) * rden;
  float b2 = __builtin_fmaf(d11, w2, -(d12 * w1)) * rden;
  b1 = __builtin_fminf(__builtin_fmaxf(b1, 0.0f), 1.0f);
  b2 = __builtin_fminf(__builtin_fmaxf(b2, 0.0f), 1.0f);
  const float b0 = __builtin_fmaxf((1.0f - b1) - b2, 0.0f);
  f4 ns;
  ns.x = __builtin_fmaf(b2, n2.x, __builtin_fmaf(b1, n1.x, b0 * n0.x));
  ns.y = __builtin_fmaf(b2, n2.y, __builtin_fmaf(b1, n1.y, b0 * n0.y));
  ns.z = __builtin_fmaf(b2, n2.z, __builtin_fmaf(b1, n1.z, b0 * n0.z));
  ns.w = 0.0f;
  const float l2 = cl_dot3(ns.xyz, ns.xyz);
  // den or |ns|^2 zero or not finite (a sliver, opposed normals): the face normal
  const bool ok = den != 0.0f && __builtin_fabsf(den) < __builtin_inff() && l2 > 0.0f && l2 < __builtin_inff();
  if (!ok) return ngf;
  ns = cl_normalize(ns);
  if (cl_dot3(ns.xyz, ngf.xyz) < 0) ns = -ns;  // on the side of the ray-facing face normal
  return ns;
}
#endif

// mcpt_device.hip (the opaque handles are defined there): what
// k_shading_normals needs of a scene; *on = 0 when it has no vertex normals.
// tris: the scene's 64-B triangle records (v0, nab, nac with the packed
// normal in their .w lanes), vn in the same (reference) order.
struct SmoothScene {
  const f4 *tris;
  const VtxNormals *vn;
  int64_t n_tris;
};
int smooth_scene(const mcpt_scene *scene, SmoothScene *out, int *on, int *device);

}  // namespace mcpt
