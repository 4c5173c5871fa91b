// ViT explanations: the head-averaged attention map of one encoder block, plain (attention
// rollout, Abnar & Zuidema 2020) or gradient-weighted (Chefer, Gur & Wolf 2021), and one step
// of the class-token recursion over the layers.
//
//   attention_relevance: P_h = softmax_j(scale Q_h K_h^T)                       [L][L] per head
//     plain     abar = (1/H) sum_h P_h
//     weighted  abar = (1/H) sum_h relu(P_h o dP_h),   dP_h = dO_h V_h^T
//   rollout_step:        r_out[j] = alpha r_in[j] + beta sum_i r_in[i] abar[i][j]
//   token_relevance_step: both in one launch under a key mask, abar never written (the BERT
//                         text tower; described at the kernel)
//
// The attention core (attention.hip) is flash-style and never holds P; this kernel recomputes
// it from the block's qkv buffer.  One workgroup owns (batch, 32 query rows), loops over the
// heads in the order h = 0 .. H-1 and keeps its abar tile [32][L] in registers, so there is no
// workspace, no atomic and one writer per output element: the result is bit-reproducible and
// every row is computed by the same instruction sequence whatever the grid.
#include <math.h>

#include <mutex>
#include <set>
#include <utility>

#include "class_reduce.h"
#include "igemm.h"
#include "../../include/mmdx.h"

namespace mmdx {

constexpr int XHD = 64;            // head dim
constexpr int XMAXKT = 16;         // 16-key tiles: L <= 256
constexpr int XMAXL = 16 * XMAXKT;
constexpr int XMAXH = 16;
constexpr int XNW = 2;             // waves per block, 16 query rows each
constexpr int XQB = XNW * 16;
constexpr int XNT = XNW * WAVE;
constexpr int RS_NT = 64;          // rollout_step: columns per block

__host__ __device__ constexpr int x_lp(int L) { return (L + 15) & ~15; }
// LDS row of one 64-element head slice plus one 16-byte vector of padding: operand rows 16
// apart then start on different banks (fp32: 68 floats, 16-bit: 72 elements = 144 B)
template <typename T> __host__ __device__ constexpr int x_ld() { return XHD + Vec16<T>::N; }
template <typename T>
static size_t x_smem(int L, bool weighted) {
  return ((size_t)x_lp(L) * (weighted ? 2 : 1) + XQB * (weighted ? 2 : 1)) * x_ld<T>() * sizeof(T);
}

// rows x 64 elements of one head, global (row stride src_ld) -> LDS (row stride LD), 16-byte
// vectors, zero from rows_valid on.  A thread issues the XU loads of a round before its first
// LDS store, so a round costs one memory latency, not XU of them.
constexpr int XU = 8;
template <typename T>
__device__ __forceinline__ void x_stage(T* dst, const T* __restrict__ src, long src_ld, int rows,
                                        int rows_valid) {
  typedef typename Vec16<T>::type V;
  constexpr int VEC = Vec16<T>::N, VPR = XHD / VEC, LD = x_ld<T>();
  const int total = rows * VPR;
  for (int i0 = threadIdx.x; i0 < total; i0 += XU * XNT) {
    V v[XU];
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int i = i0 + u * XNT, r = i / VPR, c = (i - r * VPR) * VEC;
      v[u] = V{};
      if (i < total && r < rows_valid) v[u] = *(const V*)(src + r * src_ld + c);
    }
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int i = i0 + u * XNT, r = i / VPR, c = (i - r * VPR) * VEC;
      if (i < total) *(V*)(dst + r * LD + c) = v[u];
    }
  }
}

__device__ __forceinline__ float x_group_max(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float x_group_sum(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// MFMA 16x16 tiles: lane l supplies row (l & 15), k = (l >> 4) * FRAG .. of both operands and
// receives rows (l >> 4) * 4 + r, column (l & 15) of the product.  A wave's 16 query rows
// against all LP keys are XMAXKT accumulator tiles; a query row's softmax is spread over the 16
// lanes of its group (shuffles 1, 2, 4, 8) and the tiles j.
// (launch bounds: s[] and acc[] are 128 VGPRs; the default 1024-thread budget would spill)
template <typename T, bool WEIGHTED>
__global__ __launch_bounds__(XNT) void attention_relevance_kernel(
    const T* __restrict__ qkv, const T* __restrict__ dout, int L, int H, float scale, int ntiles,
    float* __restrict__ out) {
  typedef MfmaOp<T> Op;
  constexpr int LD = x_ld<T>(), NK = XHD / Op::KS;
  extern __shared__ __attribute__((aligned(16))) char x_smem_raw[];
  const int LP = x_lp(L), nkt = LP / 16;
  T* Ks = (T*)x_smem_raw;                        // [LP][LD]
  T* Vs = Ks + LP * LD;                          // [LP][LD]   (weighted)
  T* Qs = Vs + (WEIGHTED ? LP * LD : 0);         // [XQB][LD]
  T* Ds = Qs + XQB * LD;                         // [XQB][LD]  (weighted)
  const int b = blockIdx.x / ntiles, q0 = (blockIdx.x - b * ntiles) * XQB;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const long row_ld = 3L * H * XHD, d_ld = (long)H * XHD;
  const T* qb = qkv + (long)b * L * row_ld;
  const T* db = WEIGHTED ? dout + (long)b * L * d_ld : nullptr;
  const int qrows = min(XQB, L - q0);
  const bool live = q0 + wid * 16 < L;           // wave-uniform: some row of the wave exists

  f32x4 acc[XMAXKT];
#pragma unroll
  for (int j = 0; j < XMAXKT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int h = 0; h < H; ++h) {
    if (h) __syncthreads();                      // the previous head has been read
    x_stage<T>(Ks, qb + d_ld + h * XHD, row_ld, LP, L);
    if (WEIGHTED) x_stage<T>(Vs, qb + 2 * d_ld + h * XHD, row_ld, LP, L);
    x_stage<T>(Qs, qb + (long)q0 * row_ld + h * XHD, row_ld, XQB, qrows);
    if (WEIGHTED) x_stage<T>(Ds, db + (long)q0 * d_ld + h * XHD, d_ld, XQB, qrows);
    __syncthreads();
    if (!live) continue;

    const int frag_off = (wid * 16 + col) * LD + grp * Op::FRAG;
    typename Op::frag_t aq[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) aq[k] = Op::ld(Qs + frag_off + k * Op::KS);
    f32x4 s[XMAXKT];
#pragma unroll
    for (int j = 0; j < XMAXKT; ++j) {
      s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (j < nkt) {
        const T* b_s = Ks + (j * 16 + col) * LD + grp * Op::FRAG;
#pragma unroll
        for (int k = 0; k < NK; ++k) s[j] = Op::mma(aq[k], Op::ld(b_s + k * Op::KS), s[j]);
      }
    }
    // row softmax in fp32, the maximum subtracted; a key beyond L is -inf: exp gives exactly 0
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < XMAXKT; ++j) {
      if (j >= nkt) continue;
      const bool valid = j * 16 + col < L;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[j][r] = valid ? s[j][r] * scale : -INFINITY;
        mx[r] = fmaxf(mx[r], s[j][r]);
      }
    }
    float sum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mx[r] = x_group_max(mx[r]);                // key 0 is valid: the maximum is finite
      sum[r] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < XMAXKT; ++j) {
      if (j >= nkt) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[j][r] = __expf(s[j][r] - mx[r]);
        sum[r] += s[j][r];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[r] = 1.f / x_group_sum(sum[r]);   // P = e * (1 / sum)

    if (WEIGHTED) {
      typename Op::frag_t ad[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) ad[k] = Op::ld(Ds + frag_off + k * Op::KS);
#pragma unroll
      for (int j = 0; j < XMAXKT; ++j) {
        if (j >= nkt) continue;
        const T* v_s = Vs + (j * 16 + col) * LD + grp * Op::FRAG;
        f32x4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NK; ++k) dp = Op::mma(ad[k], Op::ld(v_s + k * Op::KS), dp);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[j][r] += fmaxf((s[j][r] * sum[r]) * dp[r], 0.f);
      }
    } else {
#pragma unroll
      for (int j = 0; j < XMAXKT; ++j) {
        if (j >= nkt) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[j][r] += s[j][r] * sum[r];
      }
    }
  }

  if (!live) return;
  const float heads = (float)H;
#pragma unroll
  for (int j = 0; j < XMAXKT; ++j) {
    if (j >= nkt) continue;
    const int key = j * 16 + col;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + wid * 16 + grp * 4 + r;
      if (q < L && key < L) out[((long)b * L + q) * L + key] = acc[j][r] / heads;
    }
  }
}

// The head loop of attention_relevance_kernel with a key mask, for token_relevance_step_kernel
// (the kernel above keeps its own copy: its instructions are pinned).  On return acc[j][r] holds
// H * abar[q][key] for q = q0 + wid * 16 + grp * 4 + r, key = j * 16 + col (zero in a wave none
// of whose rows exists).  Every thread of the block calls it and passes the same number of
// barriers.  mask [B][L] int64, 1 = a real key (null: all real), applies to the keys only; a
// masked key's logit is -inf, so its probability is exactly 0 (what the additive MASK_NEG of
// attention.hip gives in fp32 for a row with a real key), and a row without any real key has a
// running maximum of -inf, which is replaced before the exponential: P = 0 there.
template <typename T, bool WEIGHTED>
__device__ __forceinline__ void x_masked_abar_tile(const T* qkv, const T* dout,
                                                   const int64_t* mask, int L, int H, float scale,
                                                   int b, int q0, f32x4 (&acc)[XMAXKT]) {
  typedef MfmaOp<T> Op;
  constexpr int LD = x_ld<T>(), NK = XHD / Op::KS;
  extern __shared__ __attribute__((aligned(16))) char x_smem_raw[];
  const int LP = x_lp(L), nkt = LP / 16;
  T* Ks = (T*)x_smem_raw;                        // [LP][LD]
  T* Vs = Ks + LP * LD;                          // [LP][LD]   (weighted)
  T* Qs = Vs + (WEIGHTED ? LP * LD : 0);         // [XQB][LD]
  T* Ds = Qs + XQB * LD;                         // [XQB][LD]  (weighted)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  const long row_ld = 3L * H * XHD, d_ld = (long)H * XHD;
  const T* qb = qkv + (long)b * L * row_ld;
  const T* db = WEIGHTED ? dout + (long)b * L * d_ld : nullptr;
  const int qrows = min(XQB, L - q0);
  const bool live = q0 + wid * 16 < L;           // wave-uniform: some row of the wave exists

  unsigned real = 0;                             // bit j: key j * 16 + col is a real key
#pragma unroll
  for (int j = 0; j < XMAXKT; ++j) {
    const int key = j * 16 + col;
    if (key < L && (!mask || mask[(long)b * L + key] != 0)) real |= 1u << j;
  }

#pragma unroll
  for (int j = 0; j < XMAXKT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int h = 0; h < H; ++h) {
    if (h) __syncthreads();                      // the previous head has been read
    x_stage<T>(Ks, qb + d_ld + h * XHD, row_ld, LP, L);
    if (WEIGHTED) x_stage<T>(Vs, qb + 2 * d_ld + h * XHD, row_ld, LP, L);
    x_stage<T>(Qs, qb + (long)q0 * row_ld + h * XHD, row_ld, XQB, qrows);
    if (WEIGHTED) x_stage<T>(Ds, db + (long)q0 * d_ld + h * XHD, d_ld, XQB, qrows);
    __syncthreads();
    if (!live) continue;

    const int frag_off = (wid * 16 + col) * LD + grp * Op::FRAG;
    typename Op::frag_t aq[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) aq[k] = Op::ld(Qs + frag_off + k * Op::KS);
    f32x4 s[XMAXKT];
#pragma unroll
    for (int j = 0; j < XMAXKT; ++j) {
      s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (j < nkt) {
        const T* b_s = Ks + (j * 16 + col) * LD + grp * Op::FRAG;
#pragma unroll
        for (int k = 0; k < NK; ++k) s[j] = Op::mma(aq[k], Op::ld(b_s + k * Op::KS), s[j]);
      }
    }
    // row softmax in fp32, the maximum subtracted; a masked key or one beyond L is -inf: exp
    // gives exactly 0
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < XMAXKT; ++j) {
      if (j >= nkt) continue;
      const bool valid = (real >> j) & 1u;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[j][r] = valid ? s[j][r] * scale : -INFINITY;
        mx[r] = fmaxf(mx[r], s[j][r]);
      }
    }
    float sum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mx[r] = x_group_max(mx[r]);
      if (mx[r] == -INFINITY) mx[r] = 0.f;       // no real key: never exp(-inf + inf)
      sum[r] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < XMAXKT; ++j) {
      if (j >= nkt) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[j][r] = __expf(s[j][r] - mx[r]);
        sum[r] += s[j][r];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                // P = e * (1 / sum); no real key: P = 0
      const float total = x_group_sum(sum[r]);
      sum[r] = total == 0.f ? 0.f : 1.f / total;
    }

    if (WEIGHTED) {
      typename Op::frag_t ad[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) ad[k] = Op::ld(Ds + frag_off + k * Op::KS);
#pragma unroll
      for (int j = 0; j < XMAXKT; ++j) {
        if (j >= nkt) continue;
        const T* v_s = Vs + (j * 16 + col) * LD + grp * Op::FRAG;
        f32x4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NK; ++k) dp = Op::mma(ad[k], Op::ld(v_s + k * Op::KS), dp);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[j][r] += fmaxf((s[j][r] * sum[r]) * dp[r], 0.f);
      }
    } else {
#pragma unroll
      for (int j = 0; j < XMAXKT; ++j) {
        if (j >= nkt) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[j][r] += s[j][r] * sum[r];
      }
    }
  }
}

// One layer of the relevance recursion for a row vector without the [L][L] map in memory:
//   r_out[b][key] = alpha r_in[b][key] + beta sum_q r_in[b][q] abar[b][q][key].
// A workgroup scales row q of its abar tile by r_in[q] and adds its 32 queries in a fixed order:
// a lane's 4 rows, the 4 lane groups (shuffles 16, 32), the 2 waves (through LDS, where the K
// slice was).  A sample of more than 32 tokens has ntiles = ceil(L / 32) such partial rows: each
// block stores its own in the workspace and draws a ticket from the sample's counter
// (class_reduce.h); the block with the last ticket adds them in tile order, writes r_out and
// stores 0 in the counter for the next launch.  So the order of every addition is a function of
// L alone: the same bits whatever B, whichever block comes last.
template <typename T, bool WEIGHTED>
__global__ __launch_bounds__(XNT) void token_relevance_step_kernel(
    const T* __restrict__ qkv, const T* __restrict__ dout, const int64_t* __restrict__ mask,
    const float* __restrict__ r_in, int L, int H, float scale, int ntiles, float alpha, float beta,
    float* __restrict__ r_out, unsigned* __restrict__ counters, unsigned* __restrict__ parts) {
  extern __shared__ __attribute__((aligned(16))) char x_smem_raw[];
  const int LP = x_lp(L), nkt = LP / 16;
  const int b = blockIdx.x / ntiles, tile = blockIdx.x - b * ntiles, q0 = tile * XQB;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int col = lane & 15, grp = lane >> 4;
  f32x4 acc[XMAXKT];
  x_masked_abar_tile<T, WEIGHTED>(qkv, dout, mask, L, H, scale, b, q0, acc);

  const float* rb = r_in + (long)b * L;
  float rq[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + wid * 16 + grp * 4 + r;
    rq[r] = q < L ? rb[q] : 0.f;                 // (a row beyond L holds a finite filler)
  }
  __syncthreads();                               // the last head has been read
  float* wave_part = (float*)x_smem_raw;         // [XNW][LP], over Ks
  const float heads = (float)H;
#pragma unroll
  for (int j = 0; j < XMAXKT; ++j) {
    if (j >= nkt) continue;
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) t = fmaf(acc[j][r] / heads, rq[r], t);
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
    if (grp == 0) wave_part[wid * LP + j * 16 + col] = t;
  }
  __syncthreads();
  float* ro = r_out + (long)b * L;
  if (ntiles == 1) {
    for (int key = threadIdx.x; key < L; key += XNT)
      ro[key] = fmaf(alpha, rb[key], beta * (wave_part[key] + wave_part[LP + key]));
    return;
  }
  unsigned* mine = parts + (long)b * ntiles * L;
  for (int key = threadIdx.x; key < L; key += XNT)
    cls_part_store(mine + tile * L + key, wave_part[key] + wave_part[LP + key]);
  if (!cls_last_of_group(counters + b, (unsigned)ntiles)) return;
  for (int key = threadIdx.x; key < L; key += XNT) {
    float s = cls_part_f32(mine + key);
    for (int t = 1; t < ntiles; ++t) s += cls_part_f32(mine + t * L + key);
    ro[key] = fmaf(alpha, rb[key], beta * s);
  }
  if (threadIdx.x == 0) cls_part_store(counters + b, 0u);   // every tile has drawn by now
}

// One thread owns column j of sample b and sums i in ascending order: fixed order, one writer.
__global__ __launch_bounds__(RS_NT) void rollout_step_kernel(const float* __restrict__ r_in,
                                                             const float* __restrict__ abar,
                                                             int Ls, int ntiles, float alpha,
                                                             float beta,
                                                             float* __restrict__ r_out) {
  const int b = blockIdx.x / ntiles;
  const int j = (blockIdx.x - b * ntiles) * RS_NT + threadIdx.x;
  if (j >= Ls) return;
  const float* r = r_in + (long)b * Ls;
  const float* a = abar + (long)b * Ls * Ls + j;
  float s = 0.f;
  for (int i = 0; i < Ls; ++i) s = fmaf(r[i], a[(long)i * Ls], s);
  r_out[(long)b * Ls + j] = fmaf(alpha, r[j], beta * s);
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel and device: the launch path
// itself then issues nothing but the kernel
// (static_lds: the kernel's own __shared__ variables, which count against the same 160 KB)
static void x_lds_max_once(const void* kern, int static_lds = 0) {
  static std::mutex mu;
  static std::set<std::pair<int, const void*>> done;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> g(mu);
  if (done.insert({dev, kern}).second)
    (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024 - static_lds);
}

template <typename T, bool WEIGHTED>
static void attention_relevance_launch(const void* qkv, const void* dout, int B, int L, int H,
                                       float scale, float* out, hipStream_t st) {
  const int ntiles = (L + XQB - 1) / XQB;
  auto kern = attention_relevance_kernel<T, WEIGHTED>;
  x_lds_max_once((const void*)kern);
  hipLaunchKernelGGL(kern, dim3((unsigned)(B * ntiles)), dim3(XNT), x_smem<T>(L, WEIGHTED), st,
                     (const T*)qkv, (const T*)dout, L, H, scale, ntiles, out);
}

constexpr int TOKEN_STATIC_LDS = 16;   // cls_last_block's ticket, as the compiler pads it

// workspace of token_relevance_step: one counter per sample (padded to 16 bytes in all), then
// the tiles' partial rows [B][ntiles][L]; nothing for a sample of one tile
static size_t token_ws_head(int B) { return ((size_t)B * sizeof(unsigned) + 15) & ~(size_t)15; }
static size_t token_ws_size(int B, int L) {
  const int ntiles = (L + XQB - 1) / XQB;
  return ntiles == 1 ? 0 : token_ws_head(B) + (size_t)B * ntiles * L * sizeof(unsigned);
}

template <typename T, bool WEIGHTED>
static void token_relevance_step_launch(const void* qkv, const void* dout, const int64_t* mask,
                                        const float* r_in, int B, int L, int H, float scale,
                                        float alpha, float beta, float* r_out, void* ws,
                                        hipStream_t st) {
  const int ntiles = (L + XQB - 1) / XQB;
  auto kern = token_relevance_step_kernel<T, WEIGHTED>;
  x_lds_max_once((const void*)kern, TOKEN_STATIC_LDS);
  unsigned* counters = (unsigned*)ws;
  unsigned* parts = ws ? (unsigned*)((char*)ws + token_ws_head(B)) : nullptr;
  hipLaunchKernelGGL(kern, dim3((unsigned)(B * ntiles)), dim3(XNT), x_smem<T>(L, WEIGHTED), st,
                     (const T*)qkv, (const T*)dout, mask, r_in, L, H, scale, ntiles, alpha, beta,
                     r_out, counters, parts);
}

static_assert(((size_t)XMAXL * 2 + XQB * 2) * x_ld<float>() * sizeof(float) + TOKEN_STATIC_LDS <=
                  160 * 1024,
              "the fp32 weighted kernels at L = 256 must fit the 160 KB of LDS");

}  // namespace mmdx

using namespace mmdx;

extern "C" int mmdx_attention_relevance(int dtype, const void* qkv, const void* dout, int B,
                                        int Ls, int H, float scale, float* out, void* stream) {
  MMDX_CHECK_ARG(qkv && out, "attention_relevance: null pointer");
  MMDX_CHECK_ARG(dtype == F32 || dtype == BF16 || dtype == F16,
                 "attention_relevance: dtype = %d", dtype);
  MMDX_CHECK_ARG(B >= 1, "attention_relevance: B = %d", B);
  MMDX_CHECK_ARG(Ls >= 1 && Ls <= XMAXL, "attention_relevance: Ls = %d outside [1, %d]", Ls,
                 XMAXL);
  MMDX_CHECK_ARG(H >= 1 && H <= XMAXH, "attention_relevance: H = %d outside [1, %d]", H, XMAXH);
  MMDX_CHECK_ARG(isfinite(scale), "attention_relevance: scale is not finite");
  MMDX_CHECK_ARG((long)B * ((Ls + XQB - 1) / XQB) <= 0x7fffffffL,
                 "attention_relevance: B = %d gives too many blocks at Ls = %d", B, Ls);
  MMDX_CHECK_ARG(((uintptr_t)qkv | (uintptr_t)dout) % 16 == 0,
                 "attention_relevance: qkv and dout must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (dout)
    MMDX_DISPATCH(dtype, attention_relevance_launch<T, true>(qkv, dout, B, Ls, H, scale, out, st));
  else
    MMDX_DISPATCH(dtype, attention_relevance_launch<T, false>(qkv, dout, B, Ls, H, scale, out, st));
  MMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmdx_rollout_step(const float* r_in, const float* abar, int B, int Ls, float alpha,
                                 float beta, float* r_out, void* stream) {
  MMDX_CHECK_ARG(r_in && abar && r_out, "rollout_step: null pointer");
  MMDX_CHECK_ARG(B >= 1, "rollout_step: B = %d", B);
  MMDX_CHECK_ARG(Ls >= 1 && Ls <= 4096, "rollout_step: Ls = %d outside [1, 4096]", Ls);
  MMDX_CHECK_ARG((long)B * ((Ls + RS_NT - 1) / RS_NT) <= 0x7fffffffL,
                 "rollout_step: B = %d gives too many blocks at Ls = %d", B, Ls);
  const uintptr_t n = (uintptr_t)B * Ls * sizeof(float);
  MMDX_CHECK_ARG((uintptr_t)r_out + n <= (uintptr_t)r_in || (uintptr_t)r_in + n <= (uintptr_t)r_out,
                 "rollout_step: r_out overlaps r_in");
  const int ntiles = (Ls + RS_NT - 1) / RS_NT;
  hipLaunchKernelGGL(rollout_step_kernel, dim3((unsigned)(B * ntiles)), dim3(RS_NT), 0,
                     (hipStream_t)stream, r_in, abar, Ls, ntiles, alpha, beta, r_out);
  MMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t mmdx_token_relevance_workspace_size(int B, int Ls) {
  if (B < 1 || Ls < 1 || Ls > XMAXL) return 0;
  return token_ws_size(B, Ls);
}

extern "C" int mmdx_token_relevance_step(int dtype, const void* qkv, const void* dout,
                                         const int64_t* mask, const float* r_in, int B, int Ls,
                                         int H, float scale, float alpha, float beta,
                                         float* r_out, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  MMDX_CHECK_ARG(qkv && r_in && r_out, "token_relevance_step: null pointer");
  MMDX_CHECK_ARG(dtype == F32 || dtype == BF16 || dtype == F16,
                 "token_relevance_step: dtype = %d", dtype);
  MMDX_CHECK_ARG(B >= 1, "token_relevance_step: B = %d", B);
  MMDX_CHECK_ARG(Ls >= 1 && Ls <= XMAXL, "token_relevance_step: Ls = %d outside [1, %d]", Ls,
                 XMAXL);
  MMDX_CHECK_ARG(H >= 1 && H <= XMAXH, "token_relevance_step: H = %d outside [1, %d]", H, XMAXH);
  MMDX_CHECK_ARG(isfinite(scale) && isfinite(alpha) && isfinite(beta),
                 "token_relevance_step: scale, alpha or beta is not finite");
  MMDX_CHECK_ARG((long)B * ((Ls + XQB - 1) / XQB) <= 0x7fffffffL,
                 "token_relevance_step: B = %d gives too many blocks at Ls = %d", B, Ls);
  MMDX_CHECK_ARG(((uintptr_t)qkv | (uintptr_t)dout) % 16 == 0,
                 "token_relevance_step: qkv and dout must be 16-byte aligned");
  MMDX_CHECK_ARG((uintptr_t)mask % 8 == 0 && ((uintptr_t)r_in | (uintptr_t)r_out) % 4 == 0,
                 "token_relevance_step: mask, r_in or r_out is misaligned");
  const size_t n = (size_t)B * Ls * sizeof(float);
  MMDX_CHECK_ARG(!ranges_overlap(r_out, n, r_in, n), "token_relevance_step: r_out overlaps r_in");
  const size_t need = token_ws_size(B, Ls);
  MMDX_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need &&
                               (uintptr_t)workspace % 16 == 0),
                 "token_relevance_step: workspace of %zu bytes, %zu needed (16-byte aligned)",
                 workspace ? workspace_bytes : (size_t)0, need);
  MMDX_CHECK_ARG(need == 0 || !ranges_overlap(workspace, need, r_out, n),
                 "token_relevance_step: the workspace overlaps r_out");
  hipStream_t st = (hipStream_t)stream;
  void* ws = need ? workspace : nullptr;
  if (dout)
    MMDX_DISPATCH(dtype, token_relevance_step_launch<T, true>(qkv, dout, mask, r_in, B, Ls, H,
                                                              scale, alpha, beta, r_out, ws, st));
  else
    MMDX_DISPATCH(dtype, token_relevance_step_launch<T, false>(qkv, dout, mask, r_in, B, Ls, H,
                                                               scale, alpha, beta, r_out, ws, st));
  MMDX_LAUNCH_CHECK();
  return 0;
}
