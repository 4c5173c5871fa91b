// Validation metrics: the integer sufficient statistics of AUROC (Mann-Whitney pair counts)
// and of a precision / recall threshold sweep, from the fp32 [N][C] logits and multi-hot
// targets exactly as the model and the loader lay them out.
//
// Everything here counts in integers and combines workgroups with 64-bit integer atomics, so
// the results do not depend on the order of accumulation: two runs give identical bytes and a
// CPU reference can be matched exactly.  No float atomics, no sort, no workspace.
#include <math.h>

#include "class_reduce.h"  // u64, CLS_MAX_C, upper_bound_lds
#include "../../include/mmdx.h"

namespace mmdx {

constexpr int MET_NT = 256;
constexpr long MET_MAX_ITEMS = 1L << 24;  // N * C
constexpr int AUROC_TILE = 4096;          // j items (floats) staged per pass: 16 KiB
constexpr int AUROC_CHUNK = 1024;         // i items per block (its positives: 256 per round)
constexpr int AUROC_BLOCKS = 2048;        // grid target: 8 blocks per CU
constexpr int GRID_MAX_T = 256;
constexpr int GRID_HIST = 12288;          // histogram counters per block: 48 KiB

// contribution of one (i, j) pair: 2 if si > sj, 1 if equal, 0 otherwise (and 0 when either is
// NaN: both IEEE compares are then false)
__device__ __forceinline__ unsigned pair2(float si, float sj) {
  return (unsigned)(si > sj) + (unsigned)(si >= sj);
}

// Tiled all-pairs counting.  A block owns AUROC_CHUNK consecutive items of the flattened
// [N*C] array as its `i` side.  Only positives can win a pair, so the block first compacts its
// positives (score, class) into an LDS list; a thread then keeps ONE positive in registers per
// round (256 per round, one round for up to 25 % positives), which keeps the lanes of a wave
// busy at the usual 15-20 % positive rate instead of idling four out of five.
// The `j` side is staged through LDS a tile of whole rows at a time, loaded contiguously
// (coalesced although one class is a column of stride C), with every item that is no negative
// replaced by NaN, which loses every compare.  One staged tile serves both statistics:
//   micro:     against every item of the tile (all lanes read the same 16 bytes: a broadcast);
//   per class: against column c of the tile, c = the item's own class (lanes of one class
//              broadcast, different classes sit on different banks for C <= 32).
// blockIdx.y strides over the row tiles, so that mid-sized problems still fill the chip.
// Counts are 32-bit within a tile pass (at most 2 * AUROC_TILE) and widened to 64 bits between
// passes; per block they meet in LDS, and the block issues one global atomic per destination.
__global__ __launch_bounds__(MET_NT) void auroc_pairs_kernel(const float* __restrict__ scores,
                                                             const float* __restrict__ target,
                                                             int N, int C,
                                                             u64* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float tile[AUROC_TILE];
  __shared__ float pos_s[AUROC_CHUNK];
  __shared__ unsigned char pos_c[AUROC_CHUNK];
  __shared__ u64 acc[(CLS_MAX_C + 1) * 4];
  __shared__ int n_list;
  const int t = threadIdx.x;
  const int M = N * C;
  for (int q = t; q < (C + 1) * 4; q += MET_NT) acc[q] = 0;
  if (t == 0) n_list = 0;
  __syncthreads();

  // the block's items: label counts (once per chunk: blockIdx.y == 0) and the positive list
  const bool count = blockIdx.y == 0;
  for (int q = 0; q < AUROC_CHUNK / MET_NT; ++q) {
    const int k = blockIdx.x * AUROC_CHUNK + q * MET_NT + t;
    const bool live = k < M;
    const int c = live ? k % C : 0;
    const float s = live ? scores[k] : 0.f;
    const float y = live ? target[k] : 0.f;
    const bool isn = live && s != s;
    const bool pos = live && !isn && y > 0.5f;
    if (pos) {
      const int e = atomicAdd(&n_list, 1);  // < AUROC_CHUNK: one slot per item of the chunk
      pos_s[e] = s;
      pos_c[e] = (unsigned char)c;
    }
    if (count) {
      const bool neg = live && !isn && !pos;
      const u64 npos = __popcll(__ballot(pos)), nneg = __popcll(__ballot(neg)),
                nnan = __popcll(__ballot(isn));
      if ((t & 63) == 0) {  // per wave: the micro row
        u64* a = acc + C * 4;
        if (npos) atomicAdd(a + 1, npos);
        if (nneg) atomicAdd(a + 2, nneg);
        if (nnan) atomicAdd(a + 3, nnan);
      }
      if (live) atomicAdd(acc + c * 4 + (pos ? 1 : neg ? 2 : 3), (u64)1);
    }
  }
  __syncthreads();
  const int P = n_list;  // block-uniform

  const int R = AUROC_TILE / C;  // rows per tile, >= 64
  for (int p0 = 0; p0 < P; p0 += MET_NT) {
    const bool have = p0 + t < P;
    const float si = have ? pos_s[p0 + t] : NAN;
    const int c = have ? pos_c[p0 + t] : 0;
    const bool wave_has = __ballot(have) != 0;  // wave-uniform
    u64 u_mic = 0, u_cls = 0;
    for (int row0 = blockIdx.y * R; row0 < N; row0 += gridDim.y * R) {
      const int rows = min(R, N - row0);
      const int ne = rows * C;
      const int n4 = (ne + 3) >> 2;  // n4 * 4 <= AUROC_TILE
      const int base = row0 * C;
      __syncthreads();  // the previous tile has been read by every wave
      for (int e = t; e < n4 * 4; e += MET_NT) {
        float v = NAN;
        if (e < ne) {
          const float sj = scores[base + e];
          if (!(target[base + e] > 0.5f)) v = sj;  // a NaN score stays NaN
        }
        tile[e] = v;
      }
      __syncthreads();
      if (wave_has) {
        const f32x4* t4 = reinterpret_cast<const f32x4*>(tile);
        unsigned g = 0;
#pragma unroll 4
        for (int q = 0; q < n4; ++q) {
          const f32x4 v = t4[q];
          g += pair2(si, v[0]) + pair2(si, v[1]) + pair2(si, v[2]) + pair2(si, v[3]);
        }
        u_mic += g;
        const float* col = tile + c;
        unsigned h = 0;
#pragma unroll 4
        for (int j = 0; j < rows; ++j) h += pair2(si, col[j * C]);
        u_cls += h;
      }
    }
    // per wave: the micro row (one destination for all lanes); per lane: its class row
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) u_mic += __shfl_xor(u_mic, o, 64);
    if ((t & 63) == 0 && u_mic) atomicAdd(acc + C * 4, u_mic);
    if (u_cls) atomicAdd(acc + c * 4, u_cls);
  }
  __syncthreads();
  for (int q = t; q < (C + 1) * 4; q += MET_NT) {
    const u64 v = acc[q];
    if (v) atomicAdd(out + q, v);
  }
}

// Threshold sweep.  Per element k = #{t : thr[t] <= logit} by binary search over the sorted
// thresholds in LDS (a NaN logit gives 0), counted into a per-block LDS histogram split by
// label and class; a suffix sum over k turns it into "logit >= thr[t]" counts, which leave the
// block as one 64-bit atomic per non-zero (label, class, t).  A block covers the classes
// [blockIdx.y * CC, + CC) so that the histogram fits LDS for every legal (C, T).
__global__ __launch_bounds__(MET_NT) void confusion_grid_kernel(
    const float* __restrict__ logits, const float* __restrict__ target, int N, int C,
    const float* __restrict__ thr, int T, int CC, u64* __restrict__ tp, u64* __restrict__ fp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char met_smem[];
  float* sthr = reinterpret_cast<float*>(met_smem);            // [T]
  unsigned* hist = reinterpret_cast<unsigned*>(sthr + T);      // [2][cc][T + 1]
  const int t = threadIdx.x;
  const int c0 = blockIdx.y * CC;
  const int cc = min(CC, C - c0);
  const int T1 = T + 1;
  for (int q = t; q < T; q += MET_NT) sthr[q] = thr[q];
  for (int q = t; q < 2 * cc * T1; q += MET_NT) hist[q] = 0;
  __syncthreads();

  const int M = N * C;
  for (int e = blockIdx.x * MET_NT + t; e < M; e += gridDim.x * MET_NT) {
    const int cl = e % C - c0;
    if ((unsigned)cl >= (unsigned)cc) continue;
    const float x = logits[e];
    const int neg = target[e] > 0.5f ? 0 : 1;
    const int lo = upper_bound_lds(sthr, T, x);
    if (lo) atomicAdd(&hist[(neg * cc + cl) * T1 + lo], 1u);  // lo <= T
  }
  __syncthreads();
  // hist[p][t + 1] <- sum over k > t of hist[p][k]
  for (int p = t; p < 2 * cc; p += MET_NT) {
    unsigned* h = hist + p * T1;
    unsigned run = 0;
    for (int k = T; k >= 1; --k) {
      run += h[k];
      h[k] = run;
    }
  }
  __syncthreads();
  for (int q = t; q < 2 * cc * T; q += MET_NT) {
    const int p = q / T, tt = q - p * T;
    const unsigned v = hist[p * T1 + tt + 1];
    if (v) {
      u64* dst = p < cc ? tp : fp;
      const int cl = c0 + (p < cc ? p : p - cc);
      atomicAdd(dst + (long)cl * T + tt, (u64)v);
    }
  }
}

}  // namespace mmdx

using namespace mmdx;

extern "C" int mmdx_auroc_pairs(const float* scores, const float* target, int N, int C,
                                int64_t* out, void* stream) {
  MMDX_CHECK_ARG(scores && target && out, "auroc_pairs: null pointer");
  MMDX_CHECK_ARG(N > 0 && C > 0, "auroc_pairs: empty (N = %d, C = %d)", N, C);
  MMDX_CHECK_ARG(C <= CLS_MAX_C, "auroc_pairs: C = %d > %d", C, CLS_MAX_C);
  MMDX_CHECK_ARG((long)N * C <= MET_MAX_ITEMS,
                 "auroc_pairs: N * C = %ld exceeds the all-pairs limit 2^24", (long)N * C);
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(out, 0, (size_t)(C + 1) * 4 * sizeof(int64_t), st);
  MMDX_CHECK_ARG(e == hipSuccess, "auroc_pairs: hipMemsetAsync: %s", hipGetErrorString(e));
  const int M = N * C;
  const int gx = (M + AUROC_CHUNK - 1) / AUROC_CHUNK;
  const int R = AUROC_TILE / C;
  const int tiles = (N + R - 1) / R;
  const int gy = std::max(1, std::min(tiles, (AUROC_BLOCKS + gx - 1) / gx));
  hipLaunchKernelGGL(auroc_pairs_kernel, dim3(gx, gy), dim3(MET_NT), 0, st, scores, target, N,
                     C, (u64*)out);
  MMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmdx_confusion_grid(const float* logits, const float* target, int N, int C,
                                   const float* thr, int T, int64_t* tp, int64_t* fp,
                                   void* stream) {
  MMDX_CHECK_ARG(logits && target && thr && tp && fp, "confusion_grid: null pointer");
  MMDX_CHECK_ARG(N > 0 && C > 0, "confusion_grid: empty (N = %d, C = %d)", N, C);
  MMDX_CHECK_ARG(C <= CLS_MAX_C, "confusion_grid: C = %d > %d", C, CLS_MAX_C);
  MMDX_CHECK_ARG((long)N * C <= MET_MAX_ITEMS,
                 "confusion_grid: N * C = %ld exceeds the limit 2^24", (long)N * C);
  MMDX_CHECK_ARG(T >= 1 && T <= GRID_MAX_T, "confusion_grid: T = %d outside [1, %d]", T,
                 GRID_MAX_T);
  hipStream_t st = (hipStream_t)stream;
  const size_t nb = (size_t)C * T * sizeof(int64_t);
  hipError_t e = hipMemsetAsync(tp, 0, nb, st);
  if (e == hipSuccess) e = hipMemsetAsync(fp, 0, nb, st);
  MMDX_CHECK_ARG(e == hipSuccess, "confusion_grid: hipMemsetAsync: %s", hipGetErrorString(e));
  const int CC = std::min(C, GRID_HIST / (2 * (T + 1)));  // >= 23 classes per block
  const int M = N * C;
  const int gx = std::max(1, std::min((M + 4095) / 4096, 128));
  const size_t smem = (size_t)T * sizeof(float) + (size_t)2 * CC * (T + 1) * sizeof(unsigned);
  hipLaunchKernelGGL(confusion_grid_kernel, dim3(gx, (C + CC - 1) / CC), dim3(MET_NT), smem, st,
                     logits, target, N, C, thr, T, CC, (u64*)tp, (u64*)fp);
  MMDX_LAUNCH_CHECK();
  return 0;
}
