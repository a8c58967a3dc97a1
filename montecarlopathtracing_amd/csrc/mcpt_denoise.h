// mcpt_denoise.h — what mcpt_denoise.hip (the denoise post-pass) needs of the
// opaque handles, whose definitions stay in mcpt_device.hip.
#pragma once
#include <cstdint>

#include "../../include/mcpt_hip.h"

namespace mcpt {

constexpr int64_t kDenoiseBytesPerPixel = 64;  // 2 x (colour, weight) ping-pong + 2 guide planes, float4 each

struct DenoiseScene {
  int device;
  const mcpt_material *mats;  // device
  int32_t n_mats;
  float root_min[3], root_max[3];  // the scene root box (its diagonal scales sigma_plane)
};

// mcpt_device.hip
int denoise_scene(const mcpt_scene *scene, DenoiseScene *out);
// the context's denoise scratch, grown to n_px pixels (kDenoiseBytesPerPixel
// each) and freed by mcpt_ctx_destroy; *device = the context's GPU
int denoise_scratch(mcpt_ctx *ctx, int64_t n_px, void **scratch, int *device);

}  // namespace mcpt
