// mcpt_env.h — environment lighting (opt-in, no reference counterpart): the
// radiance a ray that leaves the scene picks up, as include/mcpt_hip.h defines
// it at mcpt_scene_set_environment.  One expression tree, env_radiance, shared
// by k_render's miss branch, k_shade's and k_env_eval (mcpt_env.hip), so the
// three give the same bits for the same direction; every TU that includes this
// is built with the device flags of mcpt_device.hip.
#pragma once
#include <cstdint>

#include "../../include/mcpt_hip.h"
#include "mcpt_refmath.h"

namespace mcpt {

// What a kernel needs of a scene's environment.  map: width * height float4
// texels in HBM (rgb, .w unused), row 0 the top (+Y), or nullptr: the constant
// `scale`.  rot_c / rot_s: cos and sin of the rotation about +Y, computed in
// double on the host and rounded once.
struct __attribute__((aligned(16))) EnvView {
  f4 scale;  // .w = 0
  const f4 *map;
  int32_t width, height;
  float rot_c, rot_s;
};
static_assert(sizeof(EnvView) == 48, "48-B environment view");

#ifdef __HIPCC__
// L for the unit direction d.xyz.  CHECK (MCPT_DEBUG builds of k_render): the
// four texel indices are tested against the map before use and a violation is
// counted in *viol and reads texel 0 instead.  Without it they are in bounds
// by construction: u and v are clamped to [0, 1] (a NaN direction gives 0), so
// x lies in [-0.5, (float)width] and i0 = floor(x) in [-1, width + 2] ((float)
// width rounds by at most 2 below 2^26), one wrap step each way brings a
// column into [0, width) and the rows are clamped.
template <bool CHECK = false>
__device__ inline f4 env_radiance(const EnvView &E, f4 d, unsigned long long *viol = nullptr) {
  const f4 sc = E.scale;
  if (E.map == nullptr) return (f4){sc.x, sc.y, sc.z, 0.0f};
  const float rx = __builtin_fmaf(E.rot_c, d.x, E.rot_s * d.z);
  const float rz = __builtin_fmaf(E.rot_c, d.z, -(E.rot_s * d.x));
  const float ry = __builtin_fminf(__builtin_fmaxf(d.y, -1.0f), 1.0f);
  constexpr float kInv2Pi = (float)(0.5 / kClPi), kInvPi = (float)(1.0 / kClPi);
  float u = __builtin_fmaf(__ocml_atan2_f32(rx, -rz), kInv2Pi, 0.5f);
  float v = __ocml_acos_f32(ry) * kInvPi;
  u = __builtin_fminf(__builtin_fmaxf(u, 0.0f), 1.0f);
  v = __builtin_fminf(__builtin_fmaxf(v, 0.0f), 1.0f);
  const int32_t w = E.width, h = E.height;
  const float x = __builtin_fmaf(u, (float)w, -0.5f), y = __builtin_fmaf(v, (float)h, -0.5f);
  const float xf = __builtin_floorf(x), yf = __builtin_floorf(y);
  const float fx = x - xf, fy = y - yf;
  int32_t i0 = (int32_t)xf, j0 = (int32_t)yf;
  i0 = i0 < 0 ? i0 + w : (i0 >= w ? i0 - w : i0);  // columns wrap
  int32_t i1 = i0 + 1;
  i1 = i1 >= w ? i1 - w : i1;
  const int32_t j1 = min(max(j0 + 1, 0), h - 1);  // rows clamp
  j0 = min(max(j0, 0), h - 1);
  int64_t k00 = (int64_t)j0 * w + i0, k10 = (int64_t)j0 * w + i1;
  int64_t k01 = (int64_t)j1 * w + i0, k11 = (int64_t)j1 * w + i1;
  if constexpr (CHECK) {
    const bool ok = i0 >= 0 && i0 < w && i1 >= 0 && i1 < w && j0 >= 0 && j0 < h && j1 >= 0 && j1 < h;
    if (!ok) {
      atomicAdd(viol, 1ull);
      k00 = k10 = k01 = k11 = 0;
    }
  }
  const f4 t00 = E.map[k00], t10 = E.map[k10], t01 = E.map[k01], t11 = E.map[k11];
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
  f4 L;
  L.x = sc.x * __builtin_fmaf(w11, t11.x, __builtin_fmaf(w01, t01.x, __builtin_fmaf(w10, t10.x, w00 * t00.x)));
  L.y = sc.y * __builtin_fmaf(w11, t11.y, __builtin_fmaf(w01, t01.y, __builtin_fmaf(w10, t10.y, w00 * t00.y)));
  L.z = sc.z * __builtin_fmaf(w11, t11.z, __builtin_fmaf(w01, t01.z, __builtin_fmaf(w10, t10.z, w00 * t00.z)));
  L.w = 0.0f;
  return L;
}
#endif

// mcpt_device.hip (the opaque handles are defined there): a scene's
// environment and its GPU; *on = 0 when none is set
int env_scene(const mcpt_scene *scene, EnvView *out, int *on, int *device);

}  // namespace mcpt
