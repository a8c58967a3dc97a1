// mcpt_bump.hip — mcpt_bump_eval: the mapped shading normal for an array of
// (triangle, point, direction, normal) queries (opt-in bump and normal maps,
// no reference counterpart).  The lookup itself is bump_normal (mcpt_bump.h),
// the expression k_render, k_primary_bump and k_intersect_bump apply to a hit;
// this kernel is its test hook.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/mcpt_hip.h"
#include "mcpt_bump.h"

namespace mcpt {
int fail(int code, const std::string &msg);  // mcpt_host.cpp
}

namespace {

using mcpt::f3;
using mcpt::f4;

// one lane per query; a triangle index outside the scene reads nothing and gives zeros
__global__ void __launch_bounds__(256) k_bump_eval(mcpt::BumpScene S, const int32_t *__restrict__ ids,
                                                   const f4 *__restrict__ pts, const f4 *__restrict__ dirs,
                                                   const f4 *__restrict__ nrms, int64_t n, f4 *__restrict__ out) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  const int64_t t = ids[id];
  if (t < 0 || t >= S.n_tris) {
    out[id] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
    return;
  }
  const f4 *__restrict__ T = S.tris + 4 * t;
  const f4 v0 = T[0], nab = T[1], nac = T[2];
  out[id] = mcpt::bump_normal(S.bump, t, v0.xyz, nab.xyz, nac.xyz, (f3){v0.w, nab.w, nac.w}, pts[id], dirs[id], nrms[id]);
}

}  // namespace

extern "C" int mcpt_bump_eval(mcpt_ctx *ctx, const mcpt_scene *scene, const int32_t *tri_ids_dev, const float *points_dev,
                              const float *dirs_dev, const float *normals_dev, int64_t n, float *out_dev, void *stream) {
  if (!ctx || !scene || !tri_ids_dev || !points_dev || !dirs_dev || !normals_dev || !out_dev || n < 0)
    return mcpt::fail(MCPT_ERR_ARG, "bump_eval: bad argument");
  if (((uintptr_t)points_dev | (uintptr_t)dirs_dev | (uintptr_t)normals_dev | (uintptr_t)out_dev) & 15)
    return mcpt::fail(MCPT_ERR_ARG, "bump_eval: points, dirs, normals and out must be 16-byte aligned");
  if ((n + 255) / 256 > (int64_t)INT32_MAX) return mcpt::fail(MCPT_ERR_ARG, "bump_eval: too many queries");
  mcpt::BumpScene S;
  int on = 0, device = 0;
  mcpt::bump_scene(scene, &S, &on, &device);
  if (!on) return mcpt::fail(MCPT_ERR_ARG, "bump_eval: the scene has no normal maps");
  if (n == 0) return MCPT_OK;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_bump_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, S, tri_ids_dev,
                       (const f4 *)points_dev, (const f4 *)dirs_dev, (const f4 *)normals_dev, n, (f4 *)out_dev);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return mcpt::fail(MCPT_ERR_HIP, std::string("bump_eval: ") + hipGetErrorString(e));
  return MCPT_OK;
}
