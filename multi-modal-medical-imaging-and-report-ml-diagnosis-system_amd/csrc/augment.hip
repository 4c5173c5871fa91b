// Training augmentation of a batch of normalised images: a per-image affine warp (bilinear,
// black outside) followed by a per-image contrast / brightness change, in one launch.
//
//   dx = j - (W-1)/2, dy = i - (H-1)/2
//   sx = a00 dx + a01 dy + ((W-1)/2 + ox),  sy = a10 dx + a11 dy + ((H-1)/2 + oy)
//   v  = bilinear blend of the taps (floor(sy) | +1, floor(sx) | +1); a tap outside the image
//        reads fill_c = (0 - mean_c) / std_c, the normalised value of a black pixel
//   v' = gain v + ((gain - 1)(mean_c - 0.5) + delta) / std_c, clamped to [lo_c, hi_c]
//
// with params[b] = (a00, a01, ox, a10, a11, oy, gain, delta).  The warp runs in normalised
// space: at integer source positions the weights are exactly 1 and 0, so the identity, flips,
// quarter turns and whole-pixel shifts return the input's own bits.
//
// One thread owns one output pixel of one image and writes its C channels: the coordinates and
// weights are computed once and shared by the channels, consecutive lanes write consecutive
// addresses (the flat pixel index runs along W, rows follow each other in memory), and the image
// index is a grid dimension, so the parameter row is uniform per block.  No workspace, no
// atomics: every output value has one owner, so the result is bit-reproducible.
#include <math.h>

#include "common.h"
#include "../../include/mmdx.h"

namespace mmdx {

constexpr int AUG_NT = 256;
constexpr int AUG_MAX_C = 4;
constexpr int AUG_MAX_HW = 4096;
constexpr int AUG_MAX_B = 65535;

struct AugConst {
  float fill[AUG_MAX_C];  // (0 - mean) / std: a black pixel, and the lower clamp
  float hi[AUG_MAX_C];    // (1 - mean) / std
  float mid[AUG_MAX_C];   // mean - 0.5
  float stdv[AUG_MAX_C];
};

template <int C>
__global__ __launch_bounds__(AUG_NT) void augment_affine_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ params,
                                                                int H, int W, AugConst k,
                                                                int clamp,
                                                                float* __restrict__ out) {
  const float* p = params + (size_t)blockIdx.y * 8;  // uniform per block
  const float a00 = p[0], a01 = p[1], ox = p[2], a10 = p[3], a11 = p[4], oy = p[5];
  const float gain = p[6], delta = p[7];
  const int HW = H * W;  // <= 2^24
  const int e = blockIdx.x * AUG_NT + threadIdx.x;
  if (e >= HW) return;
  const int i = e / W, j = e - i * W;
  const float cx = 0.5f * (float)(W - 1), cy = 0.5f * (float)(H - 1);
  const float dx = (float)j - cx, dy = (float)i - cy;
  float sx = a00 * dx + a01 * dy + (cx + ox);
  float sy = a10 * dx + a11 * dy + (cy + oy);
  // past -1 and past the size all four taps are outside: clamping there keeps the result and
  // makes the conversion to int safe for every parameter row (fmaxf / fminf drop a NaN)
  sx = fminf(fmaxf(sx, -1.5f), (float)W + 0.5f);
  sy = fminf(fmaxf(sy, -1.5f), (float)H + 0.5f);
  const float fx = floorf(sx), fy = floorf(sy);
  const float wx = sx - fx, wy = sy - fy;
  const int x0 = (int)fx, y0 = (int)fy;
  const bool inx0 = (unsigned)x0 < (unsigned)W, inx1 = (unsigned)(x0 + 1) < (unsigned)W;
  const bool iny0 = (unsigned)y0 < (unsigned)H, iny1 = (unsigned)(y0 + 1) < (unsigned)H;
  const bool in00 = iny0 && inx0, in01 = iny0 && inx1, in10 = iny1 && inx0, in11 = iny1 && inx1;
  const int o00 = y0 * W + x0;  // read only where the tap is inside
  const float* xb = x + (size_t)blockIdx.y * C * HW;
  float* ob = out + (size_t)blockIdx.y * C * HW + e;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float* xc = xb + (size_t)c * HW;
    const float f = k.fill[c];
    const float v00 = in00 ? xc[o00] : f;
    const float v01 = in01 ? xc[o00 + 1] : f;
    const float v10 = in10 ? xc[o00 + W] : f;
    const float v11 = in11 ? xc[o00 + W + 1] : f;
    const float top = v00 * (1.f - wx) + v01 * wx;
    const float bot = v10 * (1.f - wx) + v11 * wx;
    float v = top * (1.f - wy) + bot * wy;
    v = gain * v + ((gain - 1.f) * k.mid[c] + delta) / k.stdv[c];
    if (clamp) v = fminf(fmaxf(v, f), k.hi[c]);
    ob[(size_t)c * HW] = v;
  }
}

}  // namespace mmdx

using namespace mmdx;

extern "C" int mmdx_augment_affine(const float* x, const float* params, int B, int C, int H,
                                   int W, const float* mean, const float* stdv, int clamp,
                                   float* out, void* stream) {
  MMDX_CHECK_ARG(x && params && mean && stdv && out, "augment_affine: null pointer");
  MMDX_CHECK_ARG(B >= 1 && B <= AUG_MAX_B, "augment_affine: B = %d not in [1, %d]", B, AUG_MAX_B);
  MMDX_CHECK_ARG(C >= 1 && C <= AUG_MAX_C, "augment_affine: C = %d not in [1, %d]", C, AUG_MAX_C);
  MMDX_CHECK_ARG(H >= 1 && H <= AUG_MAX_HW && W >= 1 && W <= AUG_MAX_HW,
                 "augment_affine: H = %d, W = %d not in [1, %d]", H, W, AUG_MAX_HW);
  const size_t bytes = (size_t)B * C * H * W * sizeof(float);
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
  MMDX_CHECK_ARG(xa + bytes <= oa || oa + bytes <= xa, "augment_affine: out overlaps x");
  AugConst k;
  for (int c = 0; c < AUG_MAX_C; ++c) {
    const float m = c < C ? mean[c] : 0.f, s = c < C ? stdv[c] : 1.f;
    MMDX_CHECK_ARG(isfinite(m) && isfinite(s) && s > 0.f,
                   "augment_affine: mean[%d] = %g, std[%d] = %g", c, (double)m, c, (double)s);
    // as preprocess.hip normalises the pixel values 0 and 255: (float(v) / 255 - mean) / std
    k.fill[c] = (0.f - m) / s;
    k.hi[c] = (1.f - m) / s;
    k.mid[c] = m - 0.5f;
    k.stdv[c] = s;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((H * W + AUG_NT - 1) / AUG_NT), (unsigned)B);
  const int cl = clamp ? 1 : 0;
  switch (C) {
    case 1:
      hipLaunchKernelGGL(augment_affine_kernel<1>, grid, dim3(AUG_NT), 0, st, x, params, H, W, k,
                         cl, out);
      break;
    case 2:
      hipLaunchKernelGGL(augment_affine_kernel<2>, grid, dim3(AUG_NT), 0, st, x, params, H, W, k,
                         cl, out);
      break;
    case 3:
      hipLaunchKernelGGL(augment_affine_kernel<3>, grid, dim3(AUG_NT), 0, st, x, params, H, W, k,
                         cl, out);
      break;
    default:
      hipLaunchKernelGGL(augment_affine_kernel<4>, grid, dim3(AUG_NT), 0, st, x, params, H, W, k,
                         cl, out);
      break;
  }
  MMDX_LAUNCH_CHECK();
  return 0;
}
