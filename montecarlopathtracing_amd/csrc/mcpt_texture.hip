// mcpt_texture.hip — mcpt_texture_eval: the texture lookup for an array of
// (triangle, point) queries (opt-in texture maps, no reference counterpart).
// The lookup itself is texture_factor (mcpt_texture.h), the expression
// k_render and k_shade_tex apply to a hit; this kernel is its test hook.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/mcpt_hip.h"
#include "mcpt_texture.h"

namespace mcpt {
int fail(int code, const std::string &msg);  // mcpt_host.cpp
}

namespace {

using mcpt::f4;

// one lane per query; a triangle index outside the scene reads nothing and gives zeros
__global__ void __launch_bounds__(256) k_texture_eval(mcpt::TextureScene S, const int32_t *__restrict__ ids,
                                                      const f4 *__restrict__ pts, int64_t n, f4 *__restrict__ out) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  const int64_t t = ids[id];
  if (t < 0 || t >= S.n_tris) {
    out[id] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
    return;
  }
  const f4 *__restrict__ T = S.tris + 4 * t;
  const f4 v0 = T[0], nab = T[1], nac = T[2];
  out[id] = mcpt::texture_factor(S.tex, t, v0.xyz, nab.xyz, nac.xyz, pts[id]);
}

}  // namespace

extern "C" int mcpt_texture_eval(mcpt_ctx *ctx, const mcpt_scene *scene, const int32_t *tri_ids_dev,
                                 const float *points_dev, int64_t n, float *out_dev, void *stream) {
  if (!ctx || !scene || !tri_ids_dev || !points_dev || !out_dev || n < 0)
    return mcpt::fail(MCPT_ERR_ARG, "texture_eval: bad argument");
  if (((uintptr_t)points_dev | (uintptr_t)out_dev) & 15)
    return mcpt::fail(MCPT_ERR_ARG, "texture_eval: points and out must be 16-byte aligned");
  if ((n + 255) / 256 > (int64_t)INT32_MAX) return mcpt::fail(MCPT_ERR_ARG, "texture_eval: too many queries");
  mcpt::TextureScene S;
  int on = 0, device = 0;
  mcpt::texture_scene(scene, &S, &on, &device);
  if (!on) return mcpt::fail(MCPT_ERR_ARG, "texture_eval: the scene has no textures");
  if (n == 0) return MCPT_OK;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_texture_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, S,
                       tri_ids_dev, (const f4 *)points_dev, n, (f4 *)out_dev);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return mcpt::fail(MCPT_ERR_HIP, std::string("texture_eval: ") + hipGetErrorString(e));
  return MCPT_OK;
}
