// mcpt_adaptive.h — the half-buffer noise estimate of include/mcpt_hip.h
// (mcpt_tile_error, mcpt_merge_halves): the per-pixel rules as device functions,
// one expression tree for both kernels of mcpt_adaptive.hip, and what that file
// needs of the opaque context, whose definition stays in mcpt_device.hip.
#pragma once
#include <cstdint>

#include "../../include/mcpt_hip.h"
#include "mcpt_refmath.h"

namespace mcpt {

// mcpt_device.hip: the context's GPU
int adaptive_device(const mcpt_ctx *ctx);

#if defined(__HIPCC__)
// The merged mean of two halves (mcpt_hip.h: the cases in this order).
__device__ __forceinline__ f4 merge_mean(f4 a, int32_t na, f4 b, int32_t nb) {
  if (nb == 0) return a;
  if (na == 0) return b;
  const float fa = (float)na, fb = (float)nb, ft = (float)(na + nb);
  return (f4){__fmaf_rn(fa, a.x, fb * b.x) / ft, __fmaf_rn(fa, a.y, fb * b.y) / ft, __fmaf_rn(fa, a.z, fb * b.z) / ft,
              0.0f};
}

// A pixel's error estimate: half the halves' L1 difference over the root of the floored brightness.
__device__ __forceinline__ float pixel_error(f4 a, int32_t na, f4 b, int32_t nb, float floor) {
  if (na == 0 || nb == 0) return __builtin_inff();
  const f4 m = merge_mean(a, na, b, nb);
  const float d = (__builtin_fabsf(a.x - b.x) + __builtin_fabsf(a.y - b.y)) + __builtin_fabsf(a.z - b.z);
  const float s = __builtin_fmaxf(((floor + m.x) + m.y) + m.z, floor);
  return (0.5f * d) / __builtin_sqrtf(s);
}
#endif

}  // namespace mcpt
