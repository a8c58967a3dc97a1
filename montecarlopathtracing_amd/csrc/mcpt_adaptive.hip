// mcpt_adaptive.hip — mcpt_tile_error and mcpt_merge_halves: the two-half-buffer
// noise estimate behind adaptive sampling (opt-in, no reference counterpart;
// include/mcpt_hip.h states the rules, mcpt_adaptive.h holds them).  Both kernels
// are bandwidth work: 40 B read per pixel, and 20 B written by the merge.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/mcpt_hip.h"
#include "mcpt_adaptive.h"
#include "mcpt_queue.h"  // tile_pixel: a tile's pixel k, as k_render lays it out

namespace mcpt {
int fail(int code, const std::string &msg);  // mcpt_host.cpp
}

namespace {

using mcpt::f4;

// One wave per 8x8 tile, one pixel per lane: two 16-B loads and two counts, the
// pixel's error, a butterfly sum in a fixed order (every lane ends with the same
// bits), one store per tile.  Lanes outside the image load nothing and add 0.
__global__ void __launch_bounds__(64) k_tile_error(int32_t W, int32_t H, int32_t tiles_x, const f4 *__restrict__ hA,
                                                   const int32_t *__restrict__ nA, const f4 *__restrict__ hB,
                                                   const int32_t *__restrict__ nB, float floor,
                                                   float *__restrict__ err) {
  const int32_t t = (int32_t)blockIdx.x, k = (int32_t)threadIdx.x;
  const mcpt::TilePixel tp = mcpt::tile_pixel(t, k, tiles_x);
  const bool in = tp.x < W && tp.lr < H;
  float e = 0.0f;
  if (in) {
    const size_t p = (size_t)tp.lr * (size_t)W + (size_t)tp.x;
    e = mcpt::pixel_error(hA[p], nA[p], hB[p], nB[p], floor);
  }
  for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
  if (k == 0) {
    const int32_t nx = min(8, W - (t % tiles_x) * 8), ny = min(8, H - (t / tiles_x) * 8);
    err[t] = e / (float)(nx * ny);
  }
}

__global__ void __launch_bounds__(256) k_merge_halves(const f4 *__restrict__ hA, const int32_t *__restrict__ nA,
                                                      const f4 *__restrict__ hB, const int32_t *__restrict__ nB,
                                                      int64_t n, f4 *__restrict__ out, int32_t *__restrict__ n_out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int32_t a = nA[p], b = nB[p];
  out[p] = mcpt::merge_mean(hA[p], a, hB[p], b);
  n_out[p] = a + b;
}

int launched(const char *who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mcpt::fail(MCPT_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  return MCPT_OK;
}

}  // namespace

extern "C" int mcpt_tile_error(mcpt_ctx *ctx, int32_t width, int32_t height, const float *histA, const int32_t *countA,
                               const float *histB, const int32_t *countB, float floor, float *err, void *stream) {
  if (!ctx || !histA || !countA || !histB || !countB || !err || width <= 0 || height <= 0)
    return mcpt::fail(MCPT_ERR_ARG, "tile_error: bad argument");
  if (!std::isfinite(floor) || !(floor > 0.0f)) return mcpt::fail(MCPT_ERR_ARG, "tile_error: floor must be finite and > 0");
  if (((uintptr_t)histA | (uintptr_t)histB) & 15)
    return mcpt::fail(MCPT_ERR_ARG, "tile_error: the histories must be 16-byte aligned");
  const int64_t tiles_x = (width + 7) / 8, tiles = tiles_x * ((height + 7) / 8);
  if (tiles > (int64_t)INT32_MAX) return mcpt::fail(MCPT_ERR_ARG, "tile_error: too many tiles");
  if (hipSetDevice(mcpt::adaptive_device(ctx)) != hipSuccess) return mcpt::fail(MCPT_ERR_HIP, "tile_error: hipSetDevice");
  hipLaunchKernelGGL(k_tile_error, dim3((unsigned)tiles), dim3(64), 0, (hipStream_t)stream, width, height,
                     (int32_t)tiles_x, (const f4 *)histA, countA, (const f4 *)histB, countB, floor, err);
  return launched("tile_error");
}

extern "C" int mcpt_merge_halves(mcpt_ctx *ctx, const float *histA, const int32_t *countA, const float *histB,
                                 const int32_t *countB, int64_t n, float *hist_out, int32_t *count_out, void *stream) {
  if (!ctx || !histA || !countA || !histB || !countB || !hist_out || !count_out || n < 0)
    return mcpt::fail(MCPT_ERR_ARG, "merge_halves: bad argument");
  if (((uintptr_t)histA | (uintptr_t)histB | (uintptr_t)hist_out) & 15)
    return mcpt::fail(MCPT_ERR_ARG, "merge_halves: the histories must be 16-byte aligned");
  if ((n + 255) / 256 > (int64_t)INT32_MAX) return mcpt::fail(MCPT_ERR_ARG, "merge_halves: too many pixels");
  if (n == 0) return MCPT_OK;
  if (hipSetDevice(mcpt::adaptive_device(ctx)) != hipSuccess) return mcpt::fail(MCPT_ERR_HIP, "merge_halves: hipSetDevice");
  hipLaunchKernelGGL(k_merge_halves, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const f4 *)histA, countA, (const f4 *)histB, countB, n, (f4 *)hist_out, count_out);
  return launched("merge_halves");
}
