// mcpt_lens.h — the thin-lens camera (opt-in depth of field, no reference
// counterpart), as include/mcpt_hip.h defines it at mcpt_render_frames_lens.
// One expression tree, lens_ray, shared by k_render's jittered forms and
// k_generate_lens, so the two give the same bits for the same seed; every TU
// that includes this is built with the device flags of mcpt_device.hip.
#pragma once
#include <cstdint>

#include "../../include/mcpt_hip.h"
#include "mcpt_refmath.h"

namespace mcpt {

// A launch's lens: the camera's unit axes and the two parameters.  64 B: in
// k_render it sits in LDS behind the other per-launch constants (jittered
// launches only; radius 0 = no lens, and then nothing else is read).
struct __attribute__((aligned(16))) LensView {
  f4 h, u;  // normalize(camera.horizontal.xyz), normalize(camera.up.xyz); .w = 0
  f4 c;     // normalize(camera.direction.xyz); .w = 0
  float radius, focus, pad0, pad1;
};
static_assert(sizeof(LensView) == 64, "64-B lens view");

#ifdef __HIPCC__
// The unit axes, once per launch (on the device: cl_normalize's rsq).
__device__ inline LensView lens_view(const mcpt_camera &cam, float radius, float focus) {
  LensView L;
  L.h = cl_normalize((f4){cam.horizontal[0], cam.horizontal[1], cam.horizontal[2], 0.0f});
  L.u = cl_normalize((f4){cam.up[0], cam.up[1], cam.up[2], 0.0f});
  L.c = cl_normalize((f4){cam.direction[0], cam.direction[1], cam.direction[2], 0.0f});
  L.radius = radius, L.focus = focus, L.pad0 = L.pad1 = 0.0f;
  return L;
}

// The lens ray of the jittered generateRay's (o, d): two draws from `seed`
// (r1 the radius, r2 the angle), then o' on the lens and d' through the
// sample's point on the focus plane.  o.w and d.w keep their bits.
__device__ inline void lens_ray(f4 lh, f4 lu, f4 lc, float radius, float focus, uint32_t &seed, f4 &o, f4 &d) {
  const uint32_t r1 = lcg15(seed);
  const uint32_t r2 = lcg15(seed);
  const float rho = __builtin_amdgcn_sqrtf(r1 * 1.0f * 0x1p-15f);  // r1 * 2^-15 is 0 or >= 2^-15: never scaled
  float s, c;
  sincos_small(random_phi(r2), s, c);
  const float a = radius * (rho * c), b = radius * (rho * s);
  f4 off;
  off.x = __builtin_fmaf(a, lh.x, b * lu.x);
  off.y = __builtin_fmaf(a, lh.y, b * lu.y);
  off.z = __builtin_fmaf(a, lh.z, b * lu.z);
  off.w = 0.0f;
  const float k = cl_div(focus, cl_dot3(d.xyz, lc.xyz));
  f4 t;  // P - o' = k * d - off
  t.x = __builtin_fmaf(k, d.x, -off.x);
  t.y = __builtin_fmaf(k, d.y, -off.y);
  t.z = __builtin_fmaf(k, d.z, -off.z);
  t.w = 0.0f;
  t = cl_normalize(t);
  const float ow = o.w, dw = d.w;
  o = o + off;
  o.w = ow;
  d = t;
  d.w = dw;
}
#endif

}  // namespace mcpt
