// mcpt_denoise.hip — the opt-in denoise post-pass of libmcpt_hip.so
// (mcpt_denoise, include/mcpt_hip.h): a count-aware, geometry-guided a-trous
// filter over the accumulated image.  No reference counterpart: the reference
// has no denoiser.  The filter is specified in DESIGN.md §3.11 and restated in
// float64 by tests/denoise_ref.py.
//
// The history kernel keeps the mean over a pixel's NON-ZERO samples, so a
// pixel's count says how much its mean knows: every tap is weighted by its
// count (a count-0 pixel carries no information instead of carrying black),
// and the summed weight of an iteration is the next iteration's count.
//
//  * k_denoise_prepare — one pass over the 48-B AoS first hits, hist, count and
//    the material table into float4 planes, so the 25 taps of an iteration
//    issue 16-B coalesced loads: (c.xyz, W), (n.xyz, material id bits or the
//    pass-through sentinel), (x.xyz, unused).
//  * k_denoise_iter — one lane per pixel, a wave = 64 pixels of one image row;
//    the step 2^i is an argument; reads one (c, W) plane and writes the other
//    (the last iteration writes the caller's image).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/mcpt_hip.h"
#include "mcpt_denoise.h"

namespace mcpt {
int fail(int code, const std::string &msg);  // mcpt_host.cpp
}

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f3 __attribute__((ext_vector_type(3)));

constexpr float kFltMax = 3.402823466e+38f;
constexpr uint32_t kPassThrough = 0xFFFFFFFFu;  // never a material id: ids are < n_mats <= INT32_MAX
constexpr int kTileW = 64, kTileH = 4;          // a workgroup: four waves, one 64-pixel row each

__device__ inline uint32_t bits(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ inline float dot3(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// A pixel is filtered when its first hit is a hit on a DIFFUSE or GLOSSY
// material; every other pixel (miss, light, transparent, unknown type, id out
// of range) passes through and is no tap: its planes are zero (weight 0) under
// the sentinel, in BOTH colour planes, since the iterations never write it.
__global__ __launch_bounds__(256) void k_denoise_prepare(const mcpt_hit *__restrict__ hits,
                                                         const f4 *__restrict__ hist,
                                                         const int32_t *__restrict__ count,
                                                         const mcpt_material *__restrict__ mats, int32_t n_mats,
                                                         int64_t n, f4 *__restrict__ cw_a, f4 *__restrict__ cw_b,
                                                         f4 *__restrict__ gn, f4 *__restrict__ gx) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const f4 *h = reinterpret_cast<const f4 *>(hits + p);
  const f4 nrm = h[0], pt = h[1], rest = h[2];  // rest: t, triangle id, material id, pad
  const uint32_t mid = bits(rest.z);
  bool filtered = rest.x < kFltMax && mid < (uint32_t)n_mats;
  if (filtered) {  // an out-of-range id never indexes the table
    const int32_t type = mats[mid].type;
    filtered = type == MCPT_DIFFUSE || type == MCPT_GLOSSY;
  }
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  if (filtered) {
    const f4 c = hist[p];
    cw_a[p] = (f4){c.x, c.y, c.z, (float)count[p]};
    gn[p] = (f4){nrm.x, nrm.y, nrm.z, __builtin_bit_cast(float, mid)};
    gx[p] = (f4){pt.x, pt.y, pt.z, 0.f};
  } else {
    cw_a[p] = zero;
    cw_b[p] = zero;
    gn[p] = (f4){0.f, 0.f, 0.f, __builtin_bit_cast(float, kPassThrough)};
    gx[p] = zero;
  }
}

struct IterArgs {
  const f4 *cw_in;  // (c.xyz, W) of this iteration
  f4 *cw_out;       // the next iteration's (LAST: unused)
  const f4 *gn, *gx;
  const f4 *hist;   // LAST: a pass-through pixel's output
  f4 *out;          // LAST: the caller's image
  int32_t w, h, step;
  uint32_t tiles_x;
  float inv_sn2;    // 1 / sigma_normal^2
  float inv_sx2;    // 1 / (sigma_plane * D)^2
  float inv_sc2;    // 1 / (sigma_color * 2^-i)^2, 0: no colour term
};

// A filtered centre pixel and its running sums over the taps, fed in the
// order dy outer, dx inner.
struct Centre {
  f3 n, x, c;
  uint32_t mid;
  float inv_sn2, inv_sx2, inv_sc2;
  float sw = 0.f;
  f3 sc = {0.f, 0.f, 0.f};

  __device__ Centre(const IterArgs &A, f4 n4, f4 x4, f4 c4)
      : n(n4.xyz), x(x4.xyz), c(c4.xyz), mid(bits(n4.w)), inv_sn2(A.inv_sn2), inv_sx2(A.inv_sx2),
        inv_sc2(c4.w > 0.f ? A.inv_sc2 : 0.f) {}  // the colour term needs a centre that knows its colour

  // A tap that fails a rule adds weight 0 through selects on both factors,
  // never a branch: exp runs for every tap (on 0 for a failed one, whose
  // guides may be garbage), so the taps stay one basic block and the
  // scheduler keeps a whole row of loads in flight.
  __device__ void tap(float kk, bool in, f4 nq, f4 xq, f4 cq) {
    const bool ok = in && bits(nq.w) == mid && cq.w > 0.f;
    const f3 dn = n - nq.xyz, dc = c - cq.xyz;
    const float d = dot3(n, xq.xyz - x);
    const float e = dot3(dn, dn) * inv_sn2 + d * d * inv_sx2 + dot3(dc, dc) * inv_sc2;
    const float wq = (ok ? kk * cq.w : 0.f) * expf(ok ? -e : 0.f);
    sw += wq;
    sc += wq * cq.xyz;
  }

  template <bool LAST>
  __device__ void store(const IterArgs &A, int64_t p) const {
    f4 o = {c.x, c.y, c.z, 0.f};  // no tap counted: the colour stays, the weight is 0 (no division)
    if (sw > 0.f) o = (f4){sc.x / sw, sc.y / sw, sc.z / sw, sw};
    if (LAST) {
      o.w = 0.f;
      A.out[p] = o;
    } else {
      A.cw_out[p] = o;
    }
  }
};

__device__ inline float tap_weight(int dy, int dx) {
  const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  return k[dy + 2] * k[dx + 2];
}

// Taps straight from global memory (any step): a wave's 64 lanes are 64
// pixels of one row, so every tap row is one coalesced 1-KiB load per plane.
template <bool LAST>
__global__ __launch_bounds__(256) void k_denoise_iter(const IterArgs A) {
  const uint32_t ty = blockIdx.x / A.tiles_x, tx = blockIdx.x - ty * A.tiles_x;
  const int64_t x = (int64_t)tx * kTileW + threadIdx.x, y = (int64_t)ty * kTileH + threadIdx.y;
  if (x >= A.w || y >= A.h) return;
  const int64_t p = y * A.w + x;
  const f4 np4 = A.gn[p];
  if (bits(np4.w) == kPassThrough) {
    if (LAST) A.out[p] = A.hist[p];
    return;
  }
  Centre C(A, np4, A.gx[p], A.cw_in[p]);
  // A row's 15 loads are written ahead of its arithmetic.  With the taps free
  // of branches (Centre::tap) the compiler keeps them ahead: 15 loads in flight
  // per wave instead of one tap's 3.
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int64_t yy = y + (int64_t)dy * A.step;
    const bool in_y = yy >= 0 && yy < A.h;
    f4 nq[5], xq[5], cq[5];
    bool in[5];
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int64_t xx = x + (int64_t)dx * A.step;
      in[dx + 2] = in_y && xx >= 0 && xx < A.w;
      const int64_t q = in[dx + 2] ? yy * A.w + xx : p;  // a tap outside the image is skipped: it loads the centre, weight 0
      nq[dx + 2] = A.gn[q], xq[dx + 2] = A.gx[q], cq[dx + 2] = A.cw_in[q];
    }
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) C.tap(tap_weight(dy, dx), in[dx + 2], nq[dx + 2], xq[dx + 2], cq[dx + 2]);
  }
  C.store<LAST>(A, p);
}

#define HIP_OK(expr)                                                                                          \
  do {                                                                                                        \
    hipError_t e_ = (expr);                                                                                   \
    if (e_ != hipSuccess) return mcpt::fail(MCPT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

}  // namespace

extern "C" int mcpt_denoise(mcpt_ctx *ctx, const mcpt_scene *scene, const mcpt_hit *hits, const float *hist,
                            const int32_t *count, int32_t width, int32_t height, const mcpt_denoise_params *params,
                            float *out, void *stream) {
  if (!ctx || !scene || !hits || !hist || !count || !params || !out)
    return mcpt::fail(MCPT_ERR_ARG, "denoise: null argument");
  if (width <= 0 || height <= 0) return mcpt::fail(MCPT_ERR_ARG, "denoise: width and height must be positive");
  if (params->iterations < 0 || params->iterations > 8)
    return mcpt::fail(MCPT_ERR_ARG, "denoise: iterations must be 0..8");
  if (!(params->sigma_normal > 0.f) || !std::isfinite(params->sigma_normal))
    return mcpt::fail(MCPT_ERR_ARG, "denoise: sigma_normal must be positive and finite");
  if (!(params->sigma_plane > 0.f) || !std::isfinite(params->sigma_plane))
    return mcpt::fail(MCPT_ERR_ARG, "denoise: sigma_plane must be positive and finite");
  if (!(params->sigma_color >= 0.f) || !std::isfinite(params->sigma_color))
    return mcpt::fail(MCPT_ERR_ARG, "denoise: sigma_color must be non-negative and finite");
  if (out == hist) return mcpt::fail(MCPT_ERR_ARG, "denoise: out must not be hist (the filter never writes the state)");
  if (((uintptr_t)hits | (uintptr_t)hist | (uintptr_t)out) & 15)
    return mcpt::fail(MCPT_ERR_ARG, "denoise: hits, hist and out must be 16-byte aligned");
  const int64_t n = (int64_t)width * height;
  const int64_t tiles_x = ((int64_t)width + kTileW - 1) / kTileW, tiles_y = ((int64_t)height + kTileH - 1) / kTileH;
  if (tiles_x * tiles_y > INT32_MAX || (n + 255) / 256 > INT32_MAX)
    return mcpt::fail(MCPT_ERR_ARG, "denoise: image too large");
  mcpt::DenoiseScene S;
  mcpt::denoise_scene(scene, &S);
  double d2 = 0;
  for (int k = 0; k < 3; ++k) d2 += ((double)S.root_max[k] - S.root_min[k]) * ((double)S.root_max[k] - S.root_min[k]);
  const double diag = std::sqrt(d2);
  if (!(diag > 0) || !std::isfinite(diag)) return mcpt::fail(MCPT_ERR_ARG, "denoise: the scene's root box has no extent");
  const hipStream_t st = (hipStream_t)stream;
  if (params->iterations == 0) {
    HIP_OK(hipSetDevice(S.device));
    HIP_OK(hipMemcpyAsync(out, hist, (size_t)n * sizeof(f4), hipMemcpyDeviceToDevice, st));
    return MCPT_OK;
  }
  void *scratch = nullptr;
  int device = 0;
  HIP_OK(hipSetDevice(S.device));
  const int rc = mcpt::denoise_scratch(ctx, n, &scratch, &device);
  if (rc) return rc;
  if (device != S.device) return mcpt::fail(MCPT_ERR_ARG, "denoise: scene and context are on different GPUs");
  f4 *cw[2] = {(f4 *)scratch, (f4 *)scratch + n};
  f4 *gn = (f4 *)scratch + 2 * n, *gx = (f4 *)scratch + 3 * n;
  hipLaunchKernelGGL(k_denoise_prepare, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, hits, (const f4 *)hist,
                     count, S.mats, S.n_mats, n, cw[0], cw[1], gn, gx);
  IterArgs A;
  A.gn = gn, A.gx = gx, A.hist = (const f4 *)hist, A.out = (f4 *)out;
  A.w = width, A.h = height, A.tiles_x = (uint32_t)tiles_x;
  // finite factors: 0 * inf would make a NaN of an exponent term that is 0
  const auto inv_sq = [](double sigma) { return (float)std::fmin(1.0 / (sigma * sigma), (double)kFltMax); };
  A.inv_sn2 = inv_sq((double)params->sigma_normal);
  A.inv_sx2 = inv_sq((double)params->sigma_plane * diag);
  const dim3 grid((unsigned)(tiles_x * tiles_y)), block(kTileW, kTileH);
  for (int i = 0; i < params->iterations; ++i) {
    A.cw_in = cw[i & 1], A.cw_out = cw[(i & 1) ^ 1];
    A.step = 1 << i;
    A.inv_sc2 = params->sigma_color > 0.f ? inv_sq(std::ldexp((double)params->sigma_color, -i)) : 0.f;  // sigma * 2^-i
    if (i == params->iterations - 1)
      hipLaunchKernelGGL(k_denoise_iter<true>, grid, block, 0, st, A);
    else
      hipLaunchKernelGGL(k_denoise_iter<false>, grid, block, 0, st, A);
  }
  HIP_OK(hipGetLastError());
  return MCPT_OK;
}
