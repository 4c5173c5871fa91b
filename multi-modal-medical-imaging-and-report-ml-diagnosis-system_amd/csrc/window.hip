// Grey-level windowing of packed 16-bit images to 8 bits, as mmdx/window.py defines it
// (`reference` there is the yardstick; this file equals it byte for byte).  Three kernels over
// the uint16 buffer `preprocess_batch` uploads, one descriptor per image:
//
//   histogram   a block owns a span of one image's pixels and counts them into a 65536-bin
//               histogram in LDS, then adds its non-zero bins to the image's uint32 histogram
//               in the workspace (integer atomics).
//   select      one block per image: prefix sums over the 65536 bins, the two order statistics
//               k_lo and k_hi, the flat-image rule, (lo, hi) as int32 and
//               scale = 255.0f / float(hi - lo) into `levels`; it stores zeros over the
//               histogram it read, so the workspace is zero again when the stream gets there.
//   apply       y = clamp(rint((float(v) - lo) * scale), 0, 255), 255 - y when inverted, into
//               the back-to-back uint8 layout of mmdx_clahe_* and mmdx_image_preprocess.
//               Fixed mode is this kernel alone, with lo and scale from the descriptor.
//
// Histogram layout.  65536 32-bit counters are 256 KiB and do not fit the 160 KiB of LDS, so
// the LDS counters are 16 bits wide, two to a 32-bit word (128 KiB): level v counts in word
// v & 32767, half v >> 15, so that the few hundred neighbouring levels a radiograph piles its
// pixels into are neighbouring WORDS (different banks) and never share one.  A block walks its
// span in chunks of 32768 pixels.  Before a chunk every half is at most 32767, a chunk adds at
// most 32768, so no half passes 65535 and no carry crosses into its neighbour; after a chunk
// the words with a half above 32767 are added to the global histogram and cleared (rare:
// a level needs half a chunk's pixels), after the last chunk every non-zero word is.  The
// checks read four words per LDS load and test them with one mask.  A thread's four 16-byte
// loads of a chunk are issued together, and those of the next chunk before this one is
// counted: one block fits a CU (128 KiB of LDS), so nothing else hides the load latency.  Flat
// regions (burnt-out margins, collimator shadow) would put every lane on one counter: a lane
// adds runs of equal neighbours among its 8 pixels once, and a wave whose lanes all hold
// eight pixels of one level adds the whole count from one lane.
//
// Arithmetic.  Counting is integer, and integer atomics commute: two runs give identical
// bytes.  The mapping is one exact fp32 subtraction, one fp32 multiply and rintf (half to
// even); 255.0f / x is hipcc's correctly-rounded division.  The file is compiled under
// `fp contract(off)` and states the arithmetic with plain operators (see csrc/clahe.hip).
//
// Memory.  Every image starts at a 16-byte boundary of the source buffer and the buffer ends
// at one, so each lane reads its 8 pixels with one 16-byte load, the image's last, possibly
// partial group included (pixels past the image's end are loaded and neither counted nor
// written).  The apply pass writes 8 bytes per lane: one 8-byte store where the destination is
// 8-byte aligned, two 4-byte stores where it is 4-byte aligned, bytes otherwise and in the
// last partial group.  No access leaves an image's padded source or its destination.
#include <math.h>

#include <mutex>
#include <set>
#include <utility>

#include "common.h"
#include "../../include/mmdx.h"

#pragma clang fp contract(off)

namespace mmdx {

constexpr int WN_BINS = 65536;
constexpr int WN_WORDS = WN_BINS / 2;     // LDS words: two 16-bit counters each
constexpr int WN_HIST_NT = 1024;          // threads of a histogram / select block
constexpr int WN_CHUNK = 32768;           // pixels between two overflow checks
constexpr int WN_MAX_SPAN = 8;            // chunks per block, at most
constexpr int WN_APPLY_NT = 256;
constexpr int WN_APPLY_GROUPS = 4;        // 16-byte groups per thread of the apply pass
constexpr int WN_APPLY_PX = WN_APPLY_NT * WN_APPLY_GROUPS * 8;
constexpr int WN_MAX_SIDE = 65535;
constexpr long WN_MAX_PIXELS = 1L << 30;
constexpr int WN_MAX_B = 65535;

__device__ __forceinline__ long wn_min(long a, long b) { return a < b ? a : b; }

__device__ __forceinline__ void wn_add(uint32_t* cnt, uint32_t v, uint32_t n) {
  atomicAdd(cnt + (v & (WN_WORDS - 1)), n << ((v >> 15) << 4));
}

// Add the words of `cnt` with a half above `thr` (0 or WN_CHUNK - 1) to the global histogram
// `gh` and clear them; four words per LDS read.
template <uint32_t THR>
__device__ __forceinline__ void wn_flush(uint32_t* cnt, uint32_t* __restrict__ gh) {
  // a half above 32767 has its top bit set; a half above 0 is any set bit
  constexpr uint32_t MASK = THR == 0 ? 0xffffffffu : 0x80008000u;
  for (int i = threadIdx.x; i < WN_WORDS / 4; i += WN_HIST_NT) {
    const u32x4 q = ((const u32x4*)cnt)[i];
    if (((q.x | q.y | q.z | q.w) & MASK) == 0) continue;
    const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t w = w4[j];
      if ((w & MASK) == 0) continue;
      const uint32_t lo = w & 0xffffu, hi = w >> 16;
      if (lo) atomicAdd(gh + 4 * i + j, lo);
      if (hi) atomicAdd(gh + WN_WORDS + 4 * i + j, hi);
      cnt[4 * i + j] = 0;
    }
  }
}

constexpr int WN_GROUPS = WN_CHUNK / (8 * WN_HIST_NT);  // 16-byte groups per thread and chunk
static_assert(WN_GROUPS * 8 * WN_HIST_NT == WN_CHUNK, "a chunk is whole groups per thread");

// The thread's groups of the chunk [c0, c1): all loads are issued before any is used.
__device__ __forceinline__ void wn_load(u32x4 (&t)[WN_GROUPS], const uint16_t* img, long c0,
                                        long c1) {
#pragma unroll
  for (int u = 0; u < WN_GROUPS; ++u) {
    const long g = c0 + 8L * (u * WN_HIST_NT + (int)threadIdx.x);
    // 16-byte aligned; the image is padded past its end
    t[u] = g < c1 ? *(const u32x4*)(img + g) : u32x4{0u, 0u, 0u, 0u};
  }
}

// Count the first nv (1 .. 8) pixels of the group t.
__device__ __forceinline__ void wn_count(uint32_t* cnt, const u32x4 t, int nv) {
  const int lane = threadIdx.x & 63;
  const bool flat = nv == 8 && t.x == t.y && t.x == t.z && t.x == t.w &&
                    (t.x & 0xffffu) == (t.x >> 16);  // eight equal pixels
  if (__all(flat && t.x == (uint32_t)__builtin_amdgcn_readfirstlane((int)t.x))) {
    // every active lane holds the same flat group: one add for the wave (<= 512)
    const uint32_t n = 8u * (uint32_t)__popcll(__ballot(1));
    if (lane == (int)__builtin_amdgcn_readfirstlane(lane)) wn_add(cnt, t.x & 0xffffu, n);
  } else if (flat) {
    wn_add(cnt, t.x & 0xffffu, 8);
  } else {
    const uint32_t w4[4] = {t.x, t.y, t.z, t.w};
    uint32_t cur = w4[0] & 0xffffu, run = 1;  // nv >= 1
#pragma unroll
    for (int j = 1; j < 8; ++j) {
      const uint32_t v = (w4[j >> 1] >> ((j & 1) << 4)) & 0xffffu;
      if (j < nv) {
        if (v == cur) {
          ++run;
        } else {
          wn_add(cnt, cur, run);
          cur = v;
          run = 1;
        }
      }
    }
    wn_add(cnt, cur, run);
  }
}

__global__ __launch_bounds__(WN_HIST_NT) void window_hist_kernel(
    const uint16_t* __restrict__ px, const mmdx_window_desc* __restrict__ descs, int span_chunks,
    uint32_t* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cnt[];  // WN_WORDS
  const mmdx_window_desc d = descs[blockIdx.y];
  const long n = (long)d.w * d.h;
  const long p0 = (long)blockIdx.x * span_chunks * WN_CHUNK;
  if (p0 >= n) return;  // uniform: the grid is sized for the largest image
  const long p1 = wn_min(n, p0 + (long)span_chunks * WN_CHUNK);
  const int tid = threadIdx.x;
  const uint16_t* img = px + (d.src_off >> 1);
  uint32_t* gh = hist + (size_t)blockIdx.y * WN_BINS;

  u32x4 cur[WN_GROUPS], nxt[WN_GROUPS];
  wn_load(cur, img, p0, wn_min(p1, p0 + (long)WN_CHUNK));  // in flight while the counters clear
  for (int i = tid; i < WN_WORDS / 4; i += WN_HIST_NT) ((u32x4*)cnt)[i] = u32x4{0u, 0u, 0u, 0u};
  __syncthreads();

  for (long c0 = p0; c0 < p1; c0 += WN_CHUNK) {
    const long c1 = wn_min(p1, c0 + (long)WN_CHUNK);
    const bool more = c1 < p1;  // uniform
    // the next chunk's loads are in flight while this one is counted and checked
    if (more) wn_load(nxt, img, c1, wn_min(p1, c1 + (long)WN_CHUNK));
#pragma unroll
    for (int u = 0; u < WN_GROUPS; ++u) {
      const long g = c0 + 8L * (u * WN_HIST_NT + tid);
      if (g < c1) wn_count(cnt, cur[u], (int)wn_min(8, c1 - g));
    }
    __syncthreads();
    if (more) {
      wn_flush<WN_CHUNK - 1>(cnt, gh);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < WN_GROUPS; ++u) cur[u] = nxt[u];
    }
  }
  wn_flush<0>(cnt, gh);
}

__global__ __launch_bounds__(WN_HIST_NT) void window_select_kernel(
    const mmdx_window_desc* __restrict__ descs, uint32_t* __restrict__ hist,
    int* __restrict__ levels) {
  __shared__ uint32_t wsum[WN_HIST_NT / 64];
  __shared__ int found[2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const mmdx_window_desc d = descs[b];
  // thread t owns the 64 bins [64 t, 64 t + 64)
  u32x4* mine = (u32x4*)(hist + (size_t)b * WN_BINS + 64 * tid);
  u32x4 r[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) r[i] = mine[i];
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += r[i].x + r[i].y + r[i].z + r[i].w;
#pragma unroll
  for (int i = 0; i < 16; ++i) mine[i] = u32x4{0u, 0u, 0u, 0u};  // the workspace is zero again

  uint32_t inc = s;  // inclusive prefix over the block, thread order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) wsum[wave] = inc;
  if (tid < 2) found[tid] = 0;
  __syncthreads();
  uint32_t base = 0;
#pragma unroll
  for (int i = 0; i < WN_HIST_NT / 64; ++i) base += i < wave ? wsum[i] : 0u;
  const uint32_t ex = base + inc - s;  // pixels below this thread's first bin

#pragma unroll
  for (int which = 0; which < 2; ++which) {
    // the k-th order statistic is the first level whose cumulative count exceeds k
    const uint32_t k = (uint32_t)(which ? d.k_hi : d.k_lo);
    if (ex <= k && k < ex + s) {
      uint32_t c = ex;
      int level = -1;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t q[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          c += q[j];
          if (level < 0 && c > k) level = 64 * tid + 4 * i + j;
        }
      }
      found[which] = level;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int lo = found[0];
    const int hi = found[1] == lo ? lo + 1 : found[1];  // a flat image
    levels[4 * b + 0] = lo;
    levels[4 * b + 1] = hi;
    levels[4 * b + 2] = __float_as_int(255.f / (float)(hi - lo));
    levels[4 * b + 3] = 0;
  }
}

__global__ __launch_bounds__(WN_APPLY_NT) void window_apply_kernel(
    const uint16_t* __restrict__ px, const mmdx_window_desc* __restrict__ descs,
    const int* __restrict__ levels, uint8_t* __restrict__ out) {
  const mmdx_window_desc d = descs[blockIdx.y];
  const long n = (long)d.w * d.h;
  const long g0 = (long)blockIdx.x * WN_APPLY_PX;
  if (g0 >= n) return;  // uniform
  float flo, scale;
  if (d.mode == 0) {
    flo = (float)levels[4 * blockIdx.y];  // <= 65535: exact
    scale = __int_as_float(levels[4 * blockIdx.y + 2]);
  } else {
    flo = d.lo;
    scale = d.scale;
  }
  const uint16_t* img = px + (d.src_off >> 1);
  uint8_t* dst = out + d.dst_off;
  u32x4 t[WN_APPLY_GROUPS];
#pragma unroll
  for (int u = 0; u < WN_APPLY_GROUPS; ++u) {
    const long g = g0 + 8L * (u * WN_APPLY_NT + (int)threadIdx.x);
    t[u] = g < n ? *(const u32x4*)(img + g) : u32x4{0u, 0u, 0u, 0u};
  }
#pragma unroll
  for (int u = 0; u < WN_APPLY_GROUPS; ++u) {
    const long g = g0 + 8L * (u * WN_APPLY_NT + (int)threadIdx.x);
    if (g >= n) continue;
    const uint32_t w4[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
    uint32_t res[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t v = (w4[j >> 1] >> ((j & 1) << 4)) & 0xffffu;
      const float y = fminf(fmaxf(rintf(((float)v - flo) * scale), 0.f), 255.f);
      uint32_t q = (uint32_t)(int)y;
      if (d.invert) q = 255u - q;
      res[j >> 2] |= q << ((j & 3) << 3);
    }
    uint8_t* dp = dst + g;
    const int nv = (int)wn_min(8, n - g);
    if (nv == 8 && ((uintptr_t)dp & 7) == 0) {
      *(uint2*)dp = make_uint2(res[0], res[1]);
    } else if (nv == 8 && ((uintptr_t)dp & 3) == 0) {
      ((uint32_t*)dp)[0] = res[0];
      ((uint32_t*)dp)[1] = res[1];
    } else {
      for (int j = 0; j < nv; ++j) dp[j] = (uint8_t)(res[j >> 2] >> ((j & 3) << 3));
    }
  }
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per device: the launch path itself
// then issues nothing but the kernels
static void window_lds_once() {
  static std::mutex mu;
  static std::set<int> done;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> g(mu);
  if (done.insert(dev).second)
    (void)hipFuncSetAttribute((const void*)window_hist_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

// Host validation of a descriptor table against the buffers it indexes.  `mode`: the mode every
// descriptor must have, -1 for either; `check_dst` adds the destination offsets.  Sets the error
// text and returns false on the first violation.
static bool window_check(const char* who, const mmdx_window_desc* h, int B, size_t pixel_bytes,
                         int mode, bool check_dst, size_t out_bytes) {
  long src_end = 0, dst_end = 0;
  for (int b = 0; b < B; ++b) {
    const mmdx_window_desc& d = h[b];
#define WN_REQUIRE(cond, ...)       \
  do {                              \
    if (!(cond)) {                  \
      mmdx_set_error(__VA_ARGS__);  \
      return false;                 \
    }                               \
  } while (0)
    WN_REQUIRE(d.w >= 1 && d.h >= 1 && d.w <= WN_MAX_SIDE && d.h <= WN_MAX_SIDE,
               "%s: image %d is %d x %d: sides must be in [1, %d]", who, b, d.h, d.w,
               WN_MAX_SIDE);
    const long n = (long)d.w * d.h;
    WN_REQUIRE(n <= WN_MAX_PIXELS, "%s: image %d has %ld pixels, more than 2^30", who, b, n);
    WN_REQUIRE(d.mode == 0 || d.mode == 1, "%s: image %d has mode %d, not 0 or 1", who, b,
               d.mode);
    WN_REQUIRE(mode < 0 || d.mode == mode, "%s: image %d has mode %d, this entry takes %d", who,
               b, d.mode, mode);
    WN_REQUIRE(d.invert == 0 || d.invert == 1, "%s: image %d has invert = %d", who, b, d.invert);
    if (d.mode == 0) {
      WN_REQUIRE(d.k_lo >= 0 && d.k_lo <= d.k_hi && d.k_hi < n,
                 "%s: image %d ranks (%d, %d) not ordered inside [0, %ld)", who, b, d.k_lo,
                 d.k_hi, n);
    } else {
      WN_REQUIRE(d.lo >= -65536.f && d.lo < d.hi && d.hi <= 131072.f &&
                     d.lo * 2.f == rintf(d.lo * 2.f) && d.hi * 2.f == rintf(d.hi * 2.f),
                 "%s: image %d fixed window (%g, %g): needs multiples of 0.5 with "
                 "-65536 <= lo < hi <= 131072", who, b, (double)d.lo, (double)d.hi);
      WN_REQUIRE(d.scale == 255.f / (d.hi - d.lo), "%s: image %d scale is not 255 / (hi - lo)",
                 who, b);
    }
    const long padded = (2 * n + 15) / 16 * 16;
    WN_REQUIRE(d.src_off >= src_end && d.src_off % 16 == 0 &&
                   (size_t)d.src_off + padded <= pixel_bytes,
               "%s: image %d pixels overlap the previous image's, are not 16-byte aligned or "
               "leave the source buffer (with its padding to 16 bytes)", who, b);
    src_end = d.src_off + padded;
    if (check_dst) {
      WN_REQUIRE(d.dst_off >= dst_end && (size_t)d.dst_off + n <= out_bytes,
                 "%s: image %d output overlaps the previous image's or leaves the buffer", who,
                 b);
      dst_end = d.dst_off + n;
    }
#undef WN_REQUIRE
  }
  return true;
}

}  // namespace mmdx

using namespace mmdx;

extern "C" size_t mmdx_window_desc_size(void) { return sizeof(mmdx_window_desc); }

extern "C" size_t mmdx_window_workspace_size(int B) {
  return B >= 1 && B <= WN_MAX_B ? (size_t)B * WN_BINS * sizeof(uint32_t) : 0;
}

extern "C" int mmdx_window_levels(const uint16_t* pixels, size_t pixel_bytes,
                                  const mmdx_window_desc* descs_host,
                                  const mmdx_window_desc* descs_dev, int B, void* workspace,
                                  size_t workspace_bytes, int* levels, void* stream) {
  MMDX_CHECK_ARG(pixels && descs_host && descs_dev && workspace && levels,
                 "window_levels: null pointer");
  MMDX_CHECK_ARG(B >= 1 && B <= WN_MAX_B, "window_levels: B = %d not in [1, %d]", B, WN_MAX_B);
  MMDX_CHECK_ARG((uintptr_t)pixels % 16 == 0 && (uintptr_t)workspace % 16 == 0 &&
                     (uintptr_t)levels % 4 == 0,
                 "window_levels: pixels and workspace must be 16-byte aligned");
  MMDX_CHECK_ARG(workspace_bytes >= mmdx_window_workspace_size(B),
                 "window_levels: workspace of %zu bytes, needs %zu", workspace_bytes,
                 mmdx_window_workspace_size(B));
  if (!window_check("window_levels", descs_host, B, pixel_bytes, 0, false, 0)) return -22;
  long total = 0, max_n = 1;
  for (int b = 0; b < B; ++b) {
    const long n = (long)descs_host[b].w * descs_host[b].h;
    total += n;
    max_n = std::max(max_n, n);
  }
  // chunks per block: about 512 blocks when the batch has the pixels for it (a longer
  // span adds fewer bins to the global histogram per pixel), at most WN_MAX_SPAN
  // (MMDX_WINDOW_SPAN = 1 .. 8 fixes it: tests of the multi-chunk path on small images)
  const int span = knobs().window_span > 0
                       ? knobs().window_span
                       : (int)std::min<long>(WN_MAX_SPAN,
                                             std::max<long>(1, total / (512L * WN_CHUNK)));
  const long per_block = (long)span * WN_CHUNK;
  window_lds_once();
  hipLaunchKernelGGL(window_hist_kernel, dim3((unsigned)((max_n + per_block - 1) / per_block), B),
                     dim3(WN_HIST_NT), WN_WORDS * sizeof(uint32_t), (hipStream_t)stream, pixels,
                     descs_dev, span, (uint32_t*)workspace);
  MMDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(window_select_kernel, dim3(B), dim3(WN_HIST_NT), 0, (hipStream_t)stream,
                     descs_dev, (uint32_t*)workspace, levels);
  MMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmdx_window_apply(const uint16_t* pixels, size_t pixel_bytes,
                                 const mmdx_window_desc* descs_host,
                                 const mmdx_window_desc* descs_dev, int B, const int* levels,
                                 uint8_t* out, size_t out_bytes, void* stream) {
  MMDX_CHECK_ARG(pixels && descs_host && descs_dev && out, "window_apply: null pointer");
  MMDX_CHECK_ARG(B >= 1 && B <= WN_MAX_B, "window_apply: B = %d not in [1, %d]", B, WN_MAX_B);
  MMDX_CHECK_ARG((uintptr_t)pixels % 16 == 0 && (uintptr_t)levels % 4 == 0,
                 "window_apply: pixels must be 16-byte aligned, levels 4-byte aligned");
  const uintptr_t pa = (uintptr_t)pixels, oa = (uintptr_t)out;
  MMDX_CHECK_ARG(pa + pixel_bytes <= oa || oa + out_bytes <= pa,
                 "window_apply: out overlaps pixels");
  if (!window_check("window_apply", descs_host, B, pixel_bytes, levels ? -1 : 1, true,
                    out_bytes))
    return -22;
  long max_n = 1;
  for (int b = 0; b < B; ++b)
    max_n = std::max(max_n, (long)descs_host[b].w * descs_host[b].h);
  hipLaunchKernelGGL(window_apply_kernel,
                     dim3((unsigned)((max_n + WN_APPLY_PX - 1) / WN_APPLY_PX), B),
                     dim3(WN_APPLY_NT), 0, (hipStream_t)stream, pixels, descs_dev, levels, out);
  MMDX_LAUNCH_CHECK();
  return 0;
}
