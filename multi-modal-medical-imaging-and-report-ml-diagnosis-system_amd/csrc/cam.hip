// Grad-CAM at the last conv stage: the two kernels between the trunk's NHWC feature map and a
// heatmap at image resolution.
//
//   cam_fwd:    raw[b][c][p] = max(0, sum_k alpha[b][c][k] * fmap[b][p][k])      (fp32 accumulate)
//   cam_resize: out[m] = bilinear(raw[m] / max(raw[m])) at [Ho][Wo], half-pixel centres
//
// Both are deterministic: one wave owns each raw value and sums it in a fixed order, one thread
// owns each output pixel.  No workspace, no atomics.
#include <math.h>

#include "common.h"
#include "../../include/mmdx.h"

namespace mmdx {

constexpr int CAM_NT = 256;        // 4 waves
constexpr int CAM_NW = CAM_NT / WAVE;
constexpr int CAM_CT = 16;         // classes per block (accumulators per pixel and lane)
constexpr int CAM_KT = 8 * WAVE;   // K per pass: 8 channels per lane (one 16-byte bf16 vector)
constexpr int CAM_MAX_C = 64;
constexpr int CAM_MAX_HW = 1024;
constexpr int CAM_MAX_OUT = 4096;
constexpr int CAM_TY = 32;         // output rows per resize block

// 8 consecutive channels of one pixel as floats: one 16-byte load (bf16 / fp16) or two (fp32)
template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ p, float (&f)[8]) {
  const typename Vec16<T>::type v = *reinterpret_cast<const typename Vec16<T>::type*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = to_f(v[j]);
}
template <>
__device__ __forceinline__ void load8<float>(const float* __restrict__ p, float (&f)[8]) {
  const f32x4 a = reinterpret_cast<const f32x4*>(p)[0];
  const f32x4 b = reinterpret_cast<const f32x4*>(p)[1];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = a[j];
    f[4 + j] = b[j];
  }
}

// Sums N per-lane values over the 64 lanes of a wave with N - 1 + log2(64 / N) shuffles instead
// of 6 N: at every step a lane keeps one half of its values and hands the other half to its
// partner (a reduce-scatter), until one value is left; the remaining steps are a plain
// butterfly.  Returns the total of value `idx` (same idx on the 64 / N lanes that differ only
// in the low lane bits).  Registers only: every index below is static after unrolling.
template <int N, int O>
struct WaveScatter {
  static __device__ __forceinline__ void run(float (&v)[N], int lane, int& idx) {
    constexpr int H = N / 2;
    const bool up = (lane & O) != 0;
    float r[H];
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const float keep = up ? v[i + H] : v[i];
      const float send = up ? v[i] : v[i + H];
      r[i] = keep + __shfl_xor(send, O, 64);
    }
    if (up) idx += H;
    if constexpr (H > 1) {
      WaveScatter<H, O / 2>::run(r, lane, idx);
      v[0] = r[0];
    } else {
      float s = r[0];
#pragma unroll
      for (int o = O / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      v[0] = s;
    }
  }
};

// A block owns (sample b, a tile of <= 4 PW pixels, a tile of <= 16 classes).  Wave w owns the
// pixels p0 + w + 4 j, j < PW; lane l owns the channels k0 + 8 l .. + 7 of every K pass, read
// as one contiguous 16-byte vector per pixel.  alpha[b][c0 .. c0 + 16)[k0 .. k0 + 512) is staged
// in LDS once per pass (zero-filled past C and K) and reused by the block's pixels; its layout
// [c][half][lane] makes a lane's two 16-byte reads conflict-free.  The PW * 16 partial sums of a
// lane meet in registers (WaveScatter), the ReLU is applied, one lane writes each value.
template <typename T, int PW>
__global__ __launch_bounds__(CAM_NT) void cam_fwd_kernel(const T* __restrict__ fmap,
                                                         const float* __restrict__ alpha,
                                                         int HW, int K, int C, int ntiles,
                                                         int tile_px, float* __restrict__ raw) {
  __shared__ f32x4 as4[CAM_CT * 2 * WAVE];  // 32 KiB
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int b = blockIdx.x / ntiles, tile = blockIdx.x - b * ntiles;
  const int c0 = blockIdx.y * CAM_CT;
  const int cn = min(CAM_CT, C - c0);
  const int p0 = tile * tile_px;
  const int p1 = min(HW, p0 + tile_px);  // tile_px <= CAM_NW * PW
  const T* fb = fmap + (size_t)b * HW * K;
  const float* ab = alpha + ((size_t)b * C + c0) * K;

  float acc[PW * CAM_CT];
#pragma unroll
  for (int i = 0; i < PW * CAM_CT; ++i) acc[i] = 0.f;

  for (int k0 = 0; k0 < K; k0 += CAM_KT) {
    const int k = k0 + l * 8;  // K % 8 == 0: the lane's 8 channels are all inside K or all outside
    float f[PW][8];
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      const int p = p0 + w + CAM_NW * j;
      if (k < K && p < p1) {
        load8<T>(fb + (size_t)p * K + k, f[j]);
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) f[j][q] = 0.f;
      }
    }
    __syncthreads();  // the previous pass has been read by every wave
    for (int q = t; q < CAM_CT * 2 * WAVE; q += CAM_NT) {
      const int c = q >> 7, kq = q & 127;  // kq: the 4-channel group within the pass
      const int kk = k0 + kq * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (c < cn && kk < K) v = *reinterpret_cast<const f32x4*>(ab + (size_t)c * K + kk);
      as4[(c * 2 + (kq & 1)) * WAVE + (kq >> 1)] = v;
    }
    __syncthreads();
    if (p0 + w < p1) {  // wave-uniform
#pragma unroll
      for (int c = 0; c < CAM_CT; ++c) {
        const f32x4 a0 = as4[(c * 2) * WAVE + l];
        const f32x4 a1 = as4[(c * 2 + 1) * WAVE + l];
#pragma unroll
        for (int j = 0; j < PW; ++j) {
          float s = acc[j * CAM_CT + c];
#pragma unroll
          for (int q = 0; q < 4; ++q) s = fmaf(a0[q], f[j][q], s);
#pragma unroll
          for (int q = 0; q < 4; ++q) s = fmaf(a1[q], f[j][4 + q], s);
          acc[j * CAM_CT + c] = s;
        }
      }
    }
  }

  int idx = 0;
  WaveScatter<PW * CAM_CT, 32>::run(acc, l, idx);
  const int j = idx / CAM_CT, c = idx % CAM_CT;
  const int p = p0 + w + CAM_NW * j;
  if ((l & (WAVE / (PW * CAM_CT) - 1)) == 0 && c < cn && p < p1)
    raw[((size_t)b * C + c0 + c) * HW + p] = fmaxf(acc[0], 0.f);
}

// One block = (map m, CAM_TY output rows).  The whole source map (<= 1024 values) is staged in
// LDS, divided by its maximum when `normalize` (a maximum <= 0 gives an all-zero map), and
// sampled as torch's upsample_bilinear2d does with align_corners = False: source coordinate
// (d + 0.5) * in / out - 0.5 in fp32, clamped at 0, the far neighbour clamped to the edge.
__global__ __launch_bounds__(CAM_NT) void cam_resize_kernel(const float* __restrict__ raw, int H,
                                                            int W, int Ho, int Wo, int normalize,
                                                            float* __restrict__ out) {
  __shared__ float s[CAM_MAX_HW];
  __shared__ float red[CAM_NW];
  const int t = threadIdx.x;
  const int n = H * W;
  const float* src = raw + (size_t)blockIdx.x * n;
  float m = -INFINITY;
  for (int i = t; i < n; i += CAM_NT) {
    const float v = src[i];
    s[i] = v;
    m = fmaxf(m, v);
  }
  if (normalize) {
    m = wave_max(m);
    if ((t & 63) == 0) red[t >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    for (int i = t; i < n; i += CAM_NT) s[i] = m > 0.f ? s[i] / m : 0.f;  // the thread's own
  }
  __syncthreads();

  const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
  const int y_lo = blockIdx.y * CAM_TY;
  const int rows = min(CAM_TY, Ho - y_lo);
  float* dst = out + (size_t)blockIdx.x * Ho * Wo;
  const bool vec = (Wo & 3) == 0;  // rows then start 16-byte aligned
  const int per = vec ? 4 : 1;
  const int nx = Wo / per;
  for (int e = t; e < rows * nx; e += CAM_NT) {
    const int y = y_lo + e / nx;
    const int x_lo = (e % nx) * per;
    const float fy = fmaxf(sy * ((float)y + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)fy, H - 1);
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0);
    const float ly1 = fy - (float)y0, ly0 = 1.f - ly1;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q >= per) break;
      const int x = x_lo + q;
      const float fx = fmaxf(sx * ((float)x + 0.5f) - 0.5f, 0.f);
      const int x0 = min((int)fx, W - 1);
      const int x1 = x0 + (x0 < W - 1 ? 1 : 0);
      const float lx1 = fx - (float)x0, lx0 = 1.f - lx1;
      o[q] = ly0 * (lx0 * s[y0 * W + x0] + lx1 * s[y0 * W + x1]) +
             ly1 * (lx0 * s[y1 * W + x0] + lx1 * s[y1 * W + x1]);
    }
    float* d = dst + (size_t)y * Wo + x_lo;
    if (vec) {
      *reinterpret_cast<f32x4*>(d) = f32x4{o[0], o[1], o[2], o[3]};
    } else {
      d[0] = o[0];
    }
  }
}

template <typename T>
static void cam_fwd_launch(const void* fmap, const float* alpha, int B, int HW, int K, int C,
                           float* raw, hipStream_t st) {
  const int ctiles = (C + CAM_CT - 1) / CAM_CT;
  // more pixels per wave reuse each LDS read of alpha more often; fewer fill the chip at a
  // small batch: the largest PW that still gives two blocks per CU
  int pw = 4;
  while (pw > 1 && (long)B * ((HW + CAM_NW * pw - 1) / (CAM_NW * pw)) * ctiles < 512) pw >>= 1;
  const int ntiles = (HW + CAM_NW * pw - 1) / (CAM_NW * pw);
  const int tile_px = (HW + ntiles - 1) / ntiles;  // even tiles: 49 -> 13, 12, 12, 12
  const dim3 grid((unsigned)(B * ntiles), (unsigned)ctiles);
  const T* f = (const T*)fmap;
  if (pw == 4)
    hipLaunchKernelGGL((cam_fwd_kernel<T, 4>), grid, dim3(CAM_NT), 0, st, f, alpha, HW, K, C,
                       ntiles, tile_px, raw);
  else if (pw == 2)
    hipLaunchKernelGGL((cam_fwd_kernel<T, 2>), grid, dim3(CAM_NT), 0, st, f, alpha, HW, K, C,
                       ntiles, tile_px, raw);
  else
    hipLaunchKernelGGL((cam_fwd_kernel<T, 1>), grid, dim3(CAM_NT), 0, st, f, alpha, HW, K, C,
                       ntiles, tile_px, raw);
}

}  // namespace mmdx

using namespace mmdx;

extern "C" int mmdx_cam_fwd(int dtype, const void* fmap, const float* alpha, int B, int HW, int K,
                            int C, float* raw, void* stream) {
  MMDX_CHECK_ARG(fmap && alpha && raw, "cam_fwd: null pointer");
  MMDX_CHECK_ARG(dtype == F32 || dtype == BF16 || dtype == F16, "cam_fwd: dtype = %d", dtype);
  MMDX_CHECK_ARG(B >= 1 && HW >= 1 && K >= 1 && C >= 1,
                 "cam_fwd: empty (B = %d, HW = %d, K = %d, C = %d)", B, HW, K, C);
  MMDX_CHECK_ARG(K % 8 == 0, "cam_fwd: K = %d is no multiple of 8", K);
  MMDX_CHECK_ARG(C <= CAM_MAX_C, "cam_fwd: C = %d > %d", C, CAM_MAX_C);
  MMDX_CHECK_ARG(HW <= CAM_MAX_HW, "cam_fwd: HW = %d > %d", HW, CAM_MAX_HW);
  MMDX_CHECK_ARG((long)B * ((HW + CAM_NW - 1) / CAM_NW) <= 0x7fffffffL,
                 "cam_fwd: B = %d gives too many blocks at HW = %d", B, HW);
  MMDX_CHECK_ARG(((uintptr_t)fmap | (uintptr_t)alpha) % 16 == 0,
                 "cam_fwd: fmap and alpha must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  MMDX_DISPATCH(dtype, cam_fwd_launch<T>(fmap, alpha, B, HW, K, C, raw, st));
  MMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmdx_cam_resize(const float* raw, int BC, int H, int W, int Ho, int Wo,
                               int normalize, float* out, void* stream) {
  MMDX_CHECK_ARG(raw && out, "cam_resize: null pointer");
  MMDX_CHECK_ARG(BC >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1,
                 "cam_resize: empty (BC = %d, H = %d, W = %d, Ho = %d, Wo = %d)", BC, H, W, Ho,
                 Wo);
  MMDX_CHECK_ARG((long)H * W <= CAM_MAX_HW, "cam_resize: H * W = %ld > %d", (long)H * W,
                 CAM_MAX_HW);
  MMDX_CHECK_ARG(Ho <= CAM_MAX_OUT, "cam_resize: Ho = %d > %d", Ho, CAM_MAX_OUT);
  MMDX_CHECK_ARG(Wo <= CAM_MAX_OUT, "cam_resize: Wo = %d > %d", Wo, CAM_MAX_OUT);
  MMDX_CHECK_ARG((uintptr_t)out % 16 == 0, "cam_resize: out must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cam_resize_kernel, dim3((unsigned)BC, (unsigned)((Ho + CAM_TY - 1) / CAM_TY)),
                     dim3(CAM_NT), 0, st, raw, H, W, Ho, Wo, normalize ? 1 : 0, out);
  MMDX_LAUNCH_CHECK();
  return 0;
}
