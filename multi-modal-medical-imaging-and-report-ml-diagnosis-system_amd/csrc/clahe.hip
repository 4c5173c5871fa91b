// Contrast-limited adaptive histogram equalisation (CLAHE) of packed 8-bit images, the
// algorithm of OpenCV's CLAHE_Impl as mmdx/clahe.py defines it (`reference` there is the
// yardstick; this file equals it byte for byte).  Two passes over the HWC uint8 buffer
// `preprocess_batch` uploads, one descriptor per image:
//
//   LUT pass    one block per (image, tile), all channels of the tile: a 256-bin histogram of
//               the tile of the reflect-101 extended image (the extension is index arithmetic,
//               no padded copy), clip, redistribute in closed form, 256-wide prefix sum,
//               lut[i] = clamp(rint(float(cdf[i]) * lut_scale), 0, 255) -> 256 bytes at
//               luts[image][channel][tile row][tile column].
//   apply pass  out of place: a block owns a run of image rows, splits it where the pair of
//               tile rows the interpolation reads changes, stages those two LUT rows of every
//               channel in LDS (top | bottom << 8 per entry: one LDS read gives both) and blends
//               r = (L11 xa1 + L12 xa) ya1 + (L21 xa1 + L22 xa) ya per pixel.
//
// Arithmetic.  Counting is integer; every floating-point step is ONE correctly-rounded fp32
// operation.  hipcc contracts a * b + c into a fused multiply-add by default, and that changes
// bytes, so this whole file is compiled under `fp contract(off)` (below) and states the
// arithmetic with plain operators: the __fmul_rn / __fadd_rn wrappers are plain operators inside
// a header that is compiled with contraction on, and their results were fused here.  rintf
// rounds half to even; 1.0f / x is hipcc's correctly-rounded division.  Histogram counters are
// 32-bit LDS integers (a tile holds up to 2^24 equal pixels), one sub-histogram per wave;
// integer atomics commute, so two runs give identical bytes.
//
// Memory.  LUT pass: a tile whose rows are whole, 16-byte aligned 16-byte chunks (W * C and
// tile_w * C multiples of 16: 1024-wide radiographs with 8 tiles, say) is read with one 16-byte
// load per lane and chunk, four rows' loads in flight per thread before the first count; any
// other tile is walked as the aligned 4-byte words that cover a row, a word wholly inside the
// row as one dword load, the at most two partial words at a row's ends byte by byte.  Apply
// pass: a thread owns 4 consecutive bytes of a row (their tile columns and weights are computed
// once) and walks down the rows of its block; the 4 bytes are one dword load and one dword
// store where the row addresses are 4-byte aligned, byte accesses otherwise.  No access leaves
// the image whatever W, C and the image's offset are.  Flat regions (burnt-out margins,
// collimator shadow) put every lane of a wave on one bin: a word's 4 or a chunk's 16 equal bytes
// are one add, and on the 16-byte path a wave whose lanes all hold that same chunk adds the
// whole count from one lane.
#include <math.h>

#include "common.h"
#include "../../include/mmdx.h"

#pragma clang fp contract(off)

namespace mmdx {

constexpr int CL_NT = 256;          // threads per block = histogram bins
constexpr int CL_NW = CL_NT / 64;   // waves per block = sub-histograms per channel
constexpr int CL_MAX_TILES = 16;    // per axis
constexpr int CL_MAX_C = 3;
constexpr int CL_MAX_SIDE = 65535;
constexpr int CL_MAX_AREA = 1 << 24;
constexpr int CL_MAX_B = 65535;

// reflect-101 about the last element: n + k -> n - 2 - k (k < n - 1 is guaranteed by
// W >= 2 tiles_x, H >= 2 tiles_y and an extension of at most one tile count)
__device__ __forceinline__ int reflect101(int i, int n) { return i < n ? i : 2 * (n - 1) - i; }

// smallest power of two >= n, at most CL_NT (n >= 1)
__device__ __forceinline__ int lanes_per_row(int n) {
  int l = 1;
  while (l < n && l < CL_NT) l <<= 1;
  return l;
}

__device__ __forceinline__ int block_sum_int(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) red[w] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int i = 0; i < CL_NW; ++i) t += red[i];
  return t;
}

// inclusive prefix sum over the block's CL_NT values, thread order
__device__ __forceinline__ int block_scan_int(int v, int* red) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (l >= o) v += u;
  }
  __syncthreads();
  if (l == 63) red[w] = v;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int i = 0; i < CL_NW; ++i) base += i < w ? red[i] : 0;
  return v + base;
}

// Count the 4 bytes of w4 into the grey sub-histogram h.
__device__ __forceinline__ void count4_grey(int* h, uint32_t w4) {
  if (w4 == ((w4 << 8) | (w4 >> 24))) {  // four equal bytes
    atomicAdd(h + (w4 & 255), 4);
  } else {
    atomicAdd(h + (w4 & 255), 1);
    atomicAdd(h + ((w4 >> 8) & 255), 1);
    atomicAdd(h + ((w4 >> 16) & 255), 1);
    atomicAdd(h + (w4 >> 24), 1);
  }
}

// Count the 4 bytes of w4, the first of channel ch, into the sub-histograms h[channel * stride].
__device__ __forceinline__ int count4_rgb(int* h, int stride, uint32_t w4, int ch) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    atomicAdd(h + ch * stride + ((w4 >> (8 * j)) & 255), 1);
    ch = ch == 2 ? 0 : ch + 1;
  }
  return ch;
}

__global__ __launch_bounds__(CL_NT) void clahe_lut_kernel(const uint8_t* __restrict__ px,
                                                          const mmdx_clahe_desc* __restrict__ descs,
                                                          uint8_t* __restrict__ luts) {
  __shared__ int hist[CL_MAX_C][CL_NW][256];
  __shared__ int red[CL_NW];
  const mmdx_clahe_desc d = descs[blockIdx.y];
  const int ntiles = d.tiles_x * d.tiles_y;
  if ((int)blockIdx.x >= ntiles) return;  // uniform: the grid is sized for the largest image
  const int tyi = blockIdx.x / d.tiles_x, txi = blockIdx.x - tyi * d.tiles_x;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int c = d.c, W = d.w, H = d.h, tw = d.tile_w, th = d.tile_h;

  for (int i = tid; i < c * CL_NW * 256; i += CL_NT) (&hist[0][0][0])[i] = 0;
  __syncthreads();

  const uint8_t* img = px + d.src_off;
  const int x0 = txi * tw, y0 = tyi * th;
  const int win = min(max(W - x0, 0), tw);  // columns of the tile inside the image
  const int nref = tw - win;                // reflected columns (at most tiles_x of them)

  const int span = win * c;  // bytes of one tile row inside the image
  const uint8_t* colp = img + (size_t)x0 * c;  // the tile's first column in row 0
  const uintptr_t col0 = (uintptr_t)colp;
  const int rowbytes = W * c;
  int* const hw = &hist[0][wave][0];            // this wave's sub-histogram of channel 0
  constexpr int CH_STRIDE = CL_NW * 256;        // ints between the channels' sub-histograms
  if (win > 0 && ((col0 | (uintptr_t)rowbytes | (uintptr_t)span) & 15) == 0) {
    // whole aligned 16-byte chunks: four rows' loads in flight before the first count
    const int cpr = span >> 4;
    const int lpr = lanes_per_row(cpr);
    const int rstep = CL_NT / lpr;
    for (int q = tid & (lpr - 1); q < cpr; q += lpr) {
      for (int r = tid / lpr; r < th; r += 4 * rstep) {
        u32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          // a row past the tile's end is loaded (as the last row) but not counted
          const int rr = min(r + u * rstep, th - 1);
          v[u] = *(const u32x4*)(colp + (size_t)reflect101(y0 + rr, H) * rowbytes + 16 * q);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (r + u * rstep >= th) continue;
          const u32x4 t = v[u];
          if (c == 1) {
            const bool flat = t.x == t.y && t.x == t.z && t.x == t.w &&
                              t.x == ((t.x << 8) | (t.x >> 24));  // sixteen equal bytes
            if (__all(flat && t.x == (uint32_t)__builtin_amdgcn_readfirstlane((int)t.x))) {
              // every active lane holds the same flat chunk: one add for the wave
              const int n = 16 * __popcll(__ballot(1));
              if ((tid & 63) == (int)__builtin_amdgcn_readfirstlane(tid & 63))
                atomicAdd(hw + (t.x & 255), n);
            } else if (flat) {
              atomicAdd(hw + (t.x & 255), 16);
            } else {
              count4_grey(hw, t.x);
              count4_grey(hw, t.y);
              count4_grey(hw, t.z);
              count4_grey(hw, t.w);
            }
          } else {
            int ch = q % 3;  // byte 16 q of a row that starts on a pixel: 16 = 1 (mod 3)
            ch = count4_rgb(hw, CH_STRIDE, t.x, ch);
            ch = count4_rgb(hw, CH_STRIDE, t.y, ch);
            ch = count4_rgb(hw, CH_STRIDE, t.z, ch);
            count4_rgb(hw, CH_STRIDE, t.w, ch);
          }
        }
      }
    }
  } else if (win > 0) {
    // rows aligned to 4 bytes are covered by span / 4 words, any other row touches one more
    const bool rows4 = ((col0 | (uintptr_t)rowbytes) & 3) == 0;
    const int lpr = lanes_per_row((span + 3) / 4 + (rows4 ? 0 : 1));
    const int rstep = CL_NT / lpr, wi0 = tid & (lpr - 1);
    for (int r = tid / lpr; r < th; r += rstep) {
      const uint8_t* rowp = colp + (size_t)reflect101(y0 + r, H) * rowbytes;
      // byte offsets from rowp of the aligned words that cover [0, span): the first is -3 .. 0
      const int k_first = -(int)((uintptr_t)rowp & 3);
      for (int k0 = k_first + 4 * wi0; k0 < span; k0 += 4 * lpr) {
        if (k0 >= 0 && k0 + 4 <= span) {
          const uint32_t w4 = *(const uint32_t*)(rowp + k0);
          if (c == 1) count4_grey(hw, w4);
          else count4_rgb(hw, CH_STRIDE, w4, k0 % 3);
        } else {  // a partial word at an end of the row
          for (int k = max(k0, 0); k < min(k0 + 4, span); ++k)
            atomicAdd(hw + (c == 1 ? 0 : k % 3) * CH_STRIDE + rowp[k], 1);
        }
      }
    }
  }
  if (nref > 0) {  // the reflected columns of the tile: few, read byte by byte
    const int per_row = nref * c, n = th * per_row;
    for (int i = tid; i < n; i += CL_NT) {
      const int r = i / per_row, k = i - r * per_row;
      const int j = k / c, ch = k - j * c;
      const int ys = reflect101(y0 + r, H), xs = reflect101(x0 + win + j, W);
      atomicAdd(&hist[ch][wave][img[((size_t)ys * W + xs) * c + ch]], 1);
    }
  }
  __syncthreads();

  for (int ch = 0; ch < c; ++ch) {
    int h = 0;
#pragma unroll
    for (int w = 0; w < CL_NW; ++w) h += hist[ch][w][tid];
    if (d.clip > 0) {
      const int clipped = block_sum_int(max(h - d.clip, 0), red);
      const int batch = clipped >> 8, res = clipped - (batch << 8);
      h = min(h, d.clip) + batch;
      if (res > 0) {
        const int step = max(256 / res, 1);
        if (tid % step == 0 && tid / step < res) ++h;
      }
    }
    const int cdf = block_scan_int(h, red);  // <= tile area <= 2^24: exact as a float
    const float v = fminf(fmaxf(rintf((float)cdf * d.lut_scale), 0.f), 255.f);
    luts[d.lut_off + ((size_t)(ch * d.tiles_y + tyi) * d.tiles_x + txi) * 256 + tid] =
        (uint8_t)(int)v;
  }
}

// Interpolation position along one axis: first tile index before clamping and the weight of
// the second tile, fp32 operation by operation as the definition states them.
__device__ __forceinline__ void clahe_axis(int i, float inv, int& i1, float& a) {
  const float f = (float)i * inv - 0.5f;
  const float fl = floorf(f);
  i1 = (int)fl;
  a = f - fl;
}

__global__ __launch_bounds__(CL_NT) void clahe_apply_kernel(const uint8_t* __restrict__ px,
                                                            const mmdx_clahe_desc* __restrict__ descs,
                                                            const uint8_t* __restrict__ luts,
                                                            int rows_per_block,
                                                            uint8_t* __restrict__ out) {
  // [c][tiles_x][256]: top-row entry | bottom-row entry << 8
  extern __shared__ __attribute__((aligned(16))) uint16_t lut2[];
  const mmdx_clahe_desc d = descs[blockIdx.y];
  const int row0 = blockIdx.x * rows_per_block;
  if (row0 >= d.h) return;  // uniform
  const int row1 = min(row0 + rows_per_block, d.h);
  const int tid = threadIdx.x;
  const int c = d.c, W = d.w, tx = d.tiles_x, ty = d.tiles_y;
  const int rowbytes = W * c;
  const float inv_w = 1.f / (float)d.tile_w, inv_h = 1.f / (float)d.tile_h;
  const uint8_t* src = px + d.src_off;
  uint8_t* dst = out + d.dst_off;
  const int nwords = (rowbytes + 3) >> 2;  // a thread owns the 4 bytes of one word of a row
  const int lpr = lanes_per_row(nwords);
  const int rstep = CL_NT / lpr, wi0 = tid & (lpr - 1), rlane = tid / lpr;
  const uint8_t* lbase = luts + d.lut_off;
  const int lrow = tx * 256;  // bytes of one tile row of one channel

  int r = row0;
  while (r < row1) {
    // rows [r, e) read the same pair of tile rows
    int y1;
    float ya_unused;
    clahe_axis(r, inv_h, y1, ya_unused);
    int e = r + 1;
    for (; e < row1; ++e) {
      int y1e;
      clahe_axis(e, inv_h, y1e, ya_unused);
      if (y1e != y1) break;
    }
    const int t1 = max(y1, 0), t2 = min(y1 + 1, ty - 1);
    __syncthreads();  // the previous segment's readers are done
    for (int i = tid; i < c * lrow / 4; i += CL_NT) {  // four entries per thread
      const int ch = i / (lrow / 4), k = i - ch * (lrow / 4);
      const uint8_t* chan = lbase + (size_t)ch * ty * lrow;
      const uint32_t top = *(const uint32_t*)(chan + (size_t)t1 * lrow + 4 * k);
      const uint32_t bot = *(const uint32_t*)(chan + (size_t)t2 * lrow + 4 * k);
      uint32_t* o = (uint32_t*)(lut2 + (size_t)ch * lrow + 4 * k);
      o[0] = (top & 255) | ((bot & 255) << 8) | (((top >> 8) & 255) << 16) |
             (((bot >> 8) & 255) << 24);
      o[1] = ((top >> 16) & 255) | (((bot >> 16) & 255) << 8) | ((top >> 24) << 16) |
             ((bot >> 24) << 24);
    }
    __syncthreads();

    for (int wi = wi0; wi < nwords; wi += lpr) {
      // the four bytes' tile columns (as LDS offsets) and weights: the same for every row
      int o1[4], o2[4];
      float xa[4], xa1[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // a byte past the row's end is computed on the last one's position and never stored
        const int k = min(4 * wi + j, rowbytes - 1);
        const int x = c == 1 ? k : k / 3, ch = k - x * c;
        int x1;
        clahe_axis(x, inv_w, x1, xa[j]);
        xa1[j] = 1.f - xa[j];
        o1[j] = (ch * tx + max(x1, 0)) * 256;
        o2[j] = (ch * tx + min(x1 + 1, tx - 1)) * 256;
      }
      const int nb = min(4, rowbytes - 4 * wi);  // bytes of this word inside the row
      for (int y = r + rlane; y < e; y += rstep) {
        int yy1;
        float ya;
        clahe_axis(y, inv_h, yy1, ya);
        const float ya1 = 1.f - ya;
        const uint8_t* sp = src + (size_t)y * rowbytes + 4 * wi;
        uint8_t* dp = dst + (size_t)y * rowbytes + 4 * wi;
        const bool vec = nb == 4 && ((((uintptr_t)sp) | ((uintptr_t)dp)) & 3) == 0;
        uint32_t w4 = 0;
        if (vec) {
          w4 = *(const uint32_t*)sp;
        } else {
          for (int j = 0; j < nb; ++j) w4 |= (uint32_t)sp[j] << (8 * j);
        }
        uint32_t res = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int v = (w4 >> (8 * j)) & 255;
          const uint32_t p1 = lut2[o1[j] + v], p2 = lut2[o2[j] + v];
          const float l11 = (float)(p1 & 255), l21 = (float)(p1 >> 8);
          const float l12 = (float)(p2 & 255), l22 = (float)(p2 >> 8);
          const float top = l11 * xa1[j] + l12 * xa[j];
          const float bot = l21 * xa1[j] + l22 * xa[j];
          const float rr = top * ya1 + bot * ya;
          const float q = fminf(fmaxf(rintf(rr), 0.f), 255.f);
          res |= (uint32_t)(int)q << (8 * j);
        }
        if (vec) {
          *(uint32_t*)dp = res;
        } else {
          for (int j = 0; j < nb; ++j) dp[j] = (uint8_t)(res >> (8 * j));
        }
      }
    }
    r = e;
  }
}

// Host validation of a descriptor table against the buffers it indexes; `check_dst` adds the
// destination offsets.  Sets the error text and returns false on the first violation.
static bool clahe_check(const char* who, const mmdx_clahe_desc* h, int B, size_t pixel_bytes,
                        size_t lut_bytes, bool check_dst, size_t out_bytes) {
  long lut_end = 0, dst_end = 0;
  for (int b = 0; b < B; ++b) {
    const mmdx_clahe_desc& d = h[b];
#define CL_REQUIRE(cond, ...)       \
  do {                              \
    if (!(cond)) {                  \
      mmdx_set_error(__VA_ARGS__);  \
      return false;                 \
    }                               \
  } while (0)
    CL_REQUIRE(d.c == 1 || d.c == 3, "%s: image %d has c = %d, not 1 or 3", who, b, d.c);
    CL_REQUIRE(d.tiles_x >= 1 && d.tiles_x <= CL_MAX_TILES && d.tiles_y >= 1 &&
                   d.tiles_y <= CL_MAX_TILES,
               "%s: image %d tiles %d x %d not in [1, %d]", who, b, d.tiles_x, d.tiles_y,
               CL_MAX_TILES);
    CL_REQUIRE(d.w >= 2 * d.tiles_x && d.h >= 2 * d.tiles_y && d.w <= CL_MAX_SIDE &&
                   d.h <= CL_MAX_SIDE,
               "%s: image %d is %d x %d: needs W >= 2 tiles_x, H >= 2 tiles_y, sides <= %d", who,
               b, d.h, d.w, CL_MAX_SIDE);
    const bool fits = d.w % d.tiles_x == 0 && d.h % d.tiles_y == 0;
    const int w_ext = fits ? d.w : d.w + (d.tiles_x - d.w % d.tiles_x);
    const int h_ext = fits ? d.h : d.h + (d.tiles_y - d.h % d.tiles_y);
    CL_REQUIRE(d.tile_w == w_ext / d.tiles_x && d.tile_h == h_ext / d.tiles_y,
               "%s: image %d tile size %d x %d does not match its extension (%d x %d)", who, b,
               d.tile_w, d.tile_h, w_ext / d.tiles_x, h_ext / d.tiles_y);
    const long area = (long)d.tile_w * d.tile_h;
    CL_REQUIRE(area <= CL_MAX_AREA, "%s: image %d tile area %ld exceeds 2^24", who, b, area);
    CL_REQUIRE(d.clip >= 0 && d.clip <= area, "%s: image %d clip = %d not in [0, %ld]", who, b,
               d.clip, area);
    CL_REQUIRE(d.lut_scale == 255.f / (float)area, "%s: image %d lut_scale is not 255 / area",
               who, b);
    const long nbytes = (long)d.w * d.h * d.c;
    CL_REQUIRE(d.src_off >= 0 && (size_t)d.src_off + nbytes <= pixel_bytes,
               "%s: image %d pixels leave the source buffer", who, b);
    const long lbytes = (long)d.c * d.tiles_x * d.tiles_y * 256;
    CL_REQUIRE(d.lut_off >= lut_end && d.lut_off % 256 == 0 &&
                   (size_t)d.lut_off + lbytes <= lut_bytes,
               "%s: image %d LUTs overlap the previous image's, are unaligned or leave the "
               "buffer", who, b);
    lut_end = d.lut_off + lbytes;
    if (check_dst) {
      CL_REQUIRE(d.dst_off >= dst_end && (size_t)d.dst_off + nbytes <= out_bytes,
                 "%s: image %d output overlaps the previous image's or leaves the buffer", who,
                 b);
      dst_end = d.dst_off + nbytes;
    }
#undef CL_REQUIRE
  }
  return true;
}

}  // namespace mmdx

using namespace mmdx;

extern "C" size_t mmdx_clahe_desc_size(void) { return sizeof(mmdx_clahe_desc); }

extern "C" int mmdx_clahe_luts(const uint8_t* pixels, size_t pixel_bytes,
                               const mmdx_clahe_desc* descs_host,
                               const mmdx_clahe_desc* descs_dev, int B, uint8_t* luts,
                               size_t lut_bytes, void* stream) {
  MMDX_CHECK_ARG(pixels && descs_host && descs_dev && luts, "clahe_luts: null pointer");
  MMDX_CHECK_ARG(B >= 1 && B <= CL_MAX_B, "clahe_luts: B = %d not in [1, %d]", B, CL_MAX_B);
  if (!clahe_check("clahe_luts", descs_host, B, pixel_bytes, lut_bytes, false, 0)) return -22;
  int max_tiles = 1;
  for (int b = 0; b < B; ++b)
    max_tiles = std::max(max_tiles, descs_host[b].tiles_x * descs_host[b].tiles_y);
  hipLaunchKernelGGL(clahe_lut_kernel, dim3(max_tiles, B), dim3(CL_NT), 0, (hipStream_t)stream,
                     pixels, descs_dev, luts);
  MMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmdx_clahe_apply(const uint8_t* pixels, size_t pixel_bytes,
                                const mmdx_clahe_desc* descs_host,
                                const mmdx_clahe_desc* descs_dev, int B, const uint8_t* luts,
                                size_t lut_bytes, uint8_t* out, size_t out_bytes, void* stream) {
  MMDX_CHECK_ARG(pixels && descs_host && descs_dev && luts && out, "clahe_apply: null pointer");
  MMDX_CHECK_ARG(B >= 1 && B <= CL_MAX_B, "clahe_apply: B = %d not in [1, %d]", B, CL_MAX_B);
  MMDX_CHECK_ARG((uintptr_t)luts % 4 == 0, "clahe_apply: luts must be 4-byte aligned");
  const uintptr_t pa = (uintptr_t)pixels, oa = (uintptr_t)out;
  MMDX_CHECK_ARG(pa + pixel_bytes <= oa || oa + out_bytes <= pa,
                 "clahe_apply: out overlaps pixels");
  if (!clahe_check("clahe_apply", descs_host, B, pixel_bytes, lut_bytes, true, out_bytes))
    return -22;
  long rows = 0;
  int max_h = 1, max_ctx = 1;
  for (int b = 0; b < B; ++b) {
    rows += descs_host[b].h;
    max_h = std::max(max_h, descs_host[b].h);
    max_ctx = std::max(max_ctx, descs_host[b].c * descs_host[b].tiles_x);
  }
  // rows per block: about a thousand blocks when the batch has the rows for it, at least 8 rows
  // so that the LUT staging (c * tiles_x * 512 bytes per tile-row pair) is shared, at most 64
  const int rpb = (int)std::min<long>(64, std::max<long>(8, rows / 1024));
  const size_t lds = (size_t)max_ctx * 256 * sizeof(uint16_t);  // <= 24 KB
  hipLaunchKernelGGL(clahe_apply_kernel, dim3((max_h + rpb - 1) / rpb, B), dim3(CL_NT), lds,
                     (hipStream_t)stream, pixels, descs_dev, luts, rpb, out);
  MMDX_LAUNCH_CHECK();
  return 0;
}
