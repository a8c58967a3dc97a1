// mcpt_env.hip — mcpt_env_eval: a scene's environment radiance for an array of
// rays (opt-in environment lighting, no reference counterpart).  The lookup
// itself is env_radiance (mcpt_env.h), the expression k_render and k_shade
// apply to a ray that misses; this kernel is its test hook and a public way to
// a background plate (mcpt_generate_rays, then this).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/mcpt_hip.h"
#include "mcpt_env.h"

namespace mcpt {
int fail(int code, const std::string &msg);  // mcpt_host.cpp
}

namespace {

using mcpt::f4;

// one lane per ray; without an environment (on == 0) every ray reads black
__global__ void __launch_bounds__(256) k_env_eval(mcpt::EnvView env, int on, const mcpt_ray *__restrict__ rays,
                                                  int64_t n, f4 *__restrict__ out) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= n) return;
  const f4 d = *(const f4 *)rays[id].direction;
  out[id] = on ? mcpt::env_radiance(env, d) : (f4){0.0f, 0.0f, 0.0f, 0.0f};
}

}  // namespace

extern "C" int mcpt_env_eval(mcpt_ctx *ctx, const mcpt_scene *scene, const mcpt_ray *rays_dev, int64_t n,
                             float *out_rgba_dev, void *stream) {
  if (!ctx || !scene || !rays_dev || !out_rgba_dev || n < 0) return mcpt::fail(MCPT_ERR_ARG, "env_eval: bad argument");
  if (((uintptr_t)rays_dev | (uintptr_t)out_rgba_dev) & 15)
    return mcpt::fail(MCPT_ERR_ARG, "env_eval: rays and out must be 16-byte aligned");
  if ((n + 255) / 256 > (int64_t)INT32_MAX) return mcpt::fail(MCPT_ERR_ARG, "env_eval: too many rays");
  if (n == 0) return MCPT_OK;
  mcpt::EnvView env;
  int on = 0, device = 0;
  mcpt::env_scene(scene, &env, &on, &device);
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_env_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, env, on,
                       rays_dev, n, (f4 *)out_rgba_dev);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return mcpt::fail(MCPT_ERR_HIP, std::string("env_eval: ") + hipGetErrorString(e));
  return MCPT_OK;
}
