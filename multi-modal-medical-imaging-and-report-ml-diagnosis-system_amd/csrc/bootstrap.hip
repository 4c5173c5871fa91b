// Non-parametric bootstrap over rows for the validation metrics: the integer resampling weights
// of R replicates, and per replicate the weighted sufficient statistics of AUROC (Mann-Whitney
// with midrank ties), sensitivity, specificity and F1, per class and micro.
//
// Resampling only changes integer multiplicities, never the score order of a class, so every
// replicate shares one sort (made once by the caller: include/mmdx.h "bootstrap") and a
// replicate is a weighted exclusive prefix scan over it: O(R N C) integer work instead of the
// O((N C)^2) of the all-pairs kernel per replicate.  Everything is integer arithmetic with a
// fixed owner per output, so results are bit-reproducible and equal a CPU reference exactly.
#include "bootstrap_rng.h"
#include "class_reduce.h"  // u64, CLS_MAX_C
#include "../../include/mmdx.h"

namespace mmdx {

constexpr int BOOT_NT = 256;
constexpr long BOOT_MAX_ITEMS = 1L << 24;    // N * C
constexpr long BOOT_MAX_WEIGHTS = 1L << 26;  // R * N per call
constexpr int BOOT_LDS_N = 16384;            // rows whose histogram fits 64 KiB of LDS
constexpr int BOOT_LDS_WINDOWS = 8;          // LDS histograms up to this many windows per row
constexpr int BOOT_G = 8;                    // replicates per block
constexpr int BOOT_PER = 8;                  // consecutive items per thread
constexpr int BOOT_SEG = BOOT_NT * BOOT_PER; // items per block: one segment of a column
constexpr int BOOT_PART = 3;                 // 64-bit words of a segment's partial

// A block owns a window of BOOT_LDS_N rows of one replicate (blockIdx.x the replicate,
// blockIdx.y the window): it makes all N draws, counts those that fall into its window in an LDS
// histogram (integer LDS atomics: the result does not depend on their order) and writes the
// window out with plain coalesced stores.  The draws are two hashes each and cost far less than
// a global atomic, so redoing them per window wins up to BOOT_LDS_WINDOWS windows
// (profiles/bootstrap_kernels.txt).
__global__ __launch_bounds__(BOOT_NT) void boot_weights_lds_kernel(int N, long r0, uint64_t seed,
                                                                   int* __restrict__ w) {
  extern __shared__ __attribute__((aligned(16))) int boot_hist[];
  const int t = threadIdx.x;
  const int lo = blockIdx.y * BOOT_LDS_N, n_win = min(BOOT_LDS_N, N - lo);
  for (int i = t; i < n_win; i += BOOT_NT) boot_hist[i] = 0;
  __syncthreads();
  const uint64_t key = boot_key(seed, (uint64_t)r0 + blockIdx.x);
  for (int k = t; k < N; k += BOOT_NT) {
    const unsigned d = boot_draw(key, k, N) - (unsigned)lo;
    if (d < (unsigned)n_win) atomicAdd(&boot_hist[d], 1);
  }
  __syncthreads();
  int* row = w + (size_t)blockIdx.x * N + lo;
  for (int i = t; i < n_win; i += BOOT_NT) row[i] = boot_hist[i];
}

// Longer rows: integer atomics on the zeroed output.  blockIdx.y is the replicate.
__global__ __launch_bounds__(BOOT_NT) void boot_weights_atomic_kernel(int N, long r0,
                                                                      uint64_t seed,
                                                                      int* __restrict__ w) {
  const uint64_t key = boot_key(seed, (uint64_t)r0 + blockIdx.y);
  int* row = w + (size_t)blockIdx.y * N;
  for (int k = blockIdx.x * BOOT_NT + threadIdx.x; k < N; k += gridDim.x * BOOT_NT)
    atomicAdd(&row[boot_draw(key, k, N)], 1);
}

// An item of a sorted column: (row << 3) | flags.
constexpr int ITEM_POS = 1, ITEM_LIVE = 2, ITEM_PRED = 4;

// How the columns are cut into segments of BOOT_SEG items: sc per class column, sm for the
// micro column; per tie order the segments are numbered class 0's, class 1's, ..., micro's.
struct BootGeom {
  int n_pad, m_pad, sc, sm, s_tot;
};
static inline BootGeom boot_geom(int N, int C) {
  BootGeom g;
  g.n_pad = (N + 3) & ~3;
  g.m_pad = (N * C + 3) & ~3;
  g.sc = (g.n_pad + BOOT_SEG - 1) / BOOT_SEG;
  g.sm = (g.m_pad + BOOT_SEG - 1) / BOOT_SEG;
  g.s_tot = C * g.sc + g.sm;  // <= 2 * 2^24 / BOOT_SEG + 65: twice it is a legal gridDim.y
  return g;
}

// weights [R][N] -> wt [N][rp], rp = R rounded up to a multiple of BOOT_G, the pad columns 0:
// an item's BOOT_G replicate weights then sit in 32 contiguous bytes instead of in BOOT_G
// different cache lines.  64 x 64 tiles through LDS (row pitch 65: conflict-free both ways),
// both sides coalesced; the tiles are a 1-D grid, R tiles fastest.
constexpr int BOOT_TT = 64;
__global__ __launch_bounds__(BOOT_NT) void boot_transpose_kernel(const int* __restrict__ w, int R,
                                                                 int N, int rp,
                                                                 int* __restrict__ wt) {
  __shared__ int tile[BOOT_TT][BOOT_TT + 1];
  const int tiles_r = (rp + BOOT_TT - 1) / BOOT_TT;
  const int r0 = (blockIdx.x % tiles_r) * BOOT_TT, n0 = (blockIdx.x / tiles_r) * BOOT_TT;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int k = ty; k < BOOT_TT; k += BOOT_NT / BOOT_TT) {
    const int r = r0 + k, n = n0 + tx;
    tile[k][tx] = r < R && n < N ? w[(size_t)r * N + n] : 0;
  }
  __syncthreads();
  for (int k = ty; k < BOOT_TT; k += BOOT_NT / BOOT_TT) {
    const int n = n0 + k, r = r0 + tx;
    if (n < N && r < rp) wt[(size_t)n * rp + r] = tile[tx][k];
  }
}

// The weighted scan, first half.  With
//   T(order) = sum over positives k of w_k * (negative weight strictly earlier in the order),
// order A (ascending score, positives first within ties) sees the negatives of strictly lower
// score and order B (negatives first) those and the tied ones, so u2 = T(A) + T(B) with no tie
// logic here.  T splits over segments: T = sum_s T_local(s) + WP(s) * (WN of the segments
// before s), so a block takes ONE segment of one column in one order for BOOT_G replicates (the
// item loads are shared by its replicates) and stores (T_local, WP, WN, TP, FP) per replicate;
// boot_combine_kernel adds the cross terms.  A thread takes 8 consecutive items (two 16-byte
// loads) and gathers, per item, the G weights of its row from the transposed weights (two
// 16-byte loads); the negative weights are prefix-summed in 32 bits (thread, wave shuffles, the
// four wave totals through LDS: one barrier per block) and every product is accumulated in 64
// bits.  Plain stores only: no atomics, no memset.
__global__ __launch_bounds__(BOOT_NT) void boot_segments_kernel(
    const int* __restrict__ class_items, const int* __restrict__ micro_items,
    const int* __restrict__ wt, int R, int rp, int C, BootGeom geo, u64* __restrict__ part) {
  constexpr int G = BOOT_G, NW = BOOT_NT / WAVE;
  __shared__ unsigned wave_tot[NW][G];
  __shared__ u64 red[NW][G][4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int rg = blockIdx.x * G;
  const int ord = blockIdx.y >= geo.s_tot ? 1 : 0;
  const int s = blockIdx.y - ord * geo.s_tot;
  const int* base;
  int len, seg;
  if (s < C * geo.sc) {
    const int col = s / geo.sc;
    seg = s - col * geo.sc;
    base = class_items + ((long)ord * C + col) * geo.n_pad;
    len = geo.n_pad;
  } else {
    seg = s - C * geo.sc;
    base = micro_items + (long)ord * geo.m_pad;
    len = geo.m_pad;
  }
  const int first = seg * BOOT_SEG + t * BOOT_PER;  // a multiple of 4, as len is
  int e[BOOT_PER];
#pragma unroll
  for (int k = 0; k < BOOT_PER / 4; ++k) {
    int4 v = {0, 0, 0, 0};  // past the column's end: dead items of row 0
    if (first + 4 * k < len) v = *reinterpret_cast<const int4*>(base + first + 4 * k);
    e[4 * k] = v.x, e[4 * k + 1] = v.y, e[4 * k + 2] = v.z, e[4 * k + 3] = v.w;
  }
  static_assert(G == 8, "two 16-byte loads per item");
  const int* wg = wt + rg;  // rg + G <= rp, and (row * rp + rg) * 4 is a multiple of 32

  u64 acc[G];
  unsigned tot[G], swp[G], tp[G], fp[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = 0, tot[g] = swp[g] = tp[g] = fp[g] = 0;
#pragma unroll
  for (int j = 0; j < BOOT_PER; ++j) {
    const int row = e[j] >> 3;  // < N for every item, dead ones included
    const bool live = e[j] & ITEM_LIVE, pos = e[j] & ITEM_POS, pred = e[j] & ITEM_PRED;
    const int4* p = reinterpret_cast<const int4*>(wg + (size_t)row * rp);
    const int4 lo = p[0], hi = p[1];
    const int xs[G] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const unsigned x = live ? (unsigned)xs[g] : 0u;
      const unsigned xp = pos ? x : 0u, xn = pos ? 0u : x;
      acc[g] += (u64)xp * tot[g];  // the negatives earlier within the thread
      tot[g] += xn;
      swp[g] += xp;
      if (pred) tp[g] += xp, fp[g] += xn;
    }
  }
  // exclusive prefix of tot over the block
  unsigned inc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) inc[g] = tot[g];
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const unsigned u = __shfl_up(inc[g], o, WAVE);
      if (lane >= o) inc[g] += u;
    }
  }
  if (lane == WAVE - 1) {
#pragma unroll
    for (int g = 0; g < G; ++g) wave_tot[wv][g] = inc[g];
  }
  __syncthreads();
  unsigned all[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    unsigned before = 0;
    all[g] = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const unsigned x = wave_tot[k][g];
      before += k < wv ? x : 0u;
      all[g] += x;
    }
    acc[g] += (u64)swp[g] * (before + (inc[g] - tot[g]));
  }
  // the block's sums: T_local, WP, TP, FP (WN = all[] is already block-uniform)
#pragma unroll
  for (int g = 0; g < G; ++g) {
    u64 v[4] = {acc[g], swp[g], tp[g], fp[g]};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, WAVE);
      if (lane == 0) red[wv][g][k] = v[k];
    }
  }
  __syncthreads();
  if (t < G && rg + t < R) {
    u64 v[4] = {0, 0, 0, 0};
    for (int k = 0; k < NW; ++k)
      for (int c = 0; c < 4; ++c) v[c] += red[k][t][c];
    u64 neg = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) neg = g == t ? all[g] : neg;
    // WP, WN, TP, FP of a segment are sums of at most BOOT_SEG weights: 32 bits each
    u64* p = part + ((size_t)blockIdx.y * R + rg + t) * BOOT_PART;
    p[0] = v[0], p[1] = v[1] | (neg << 32), p[2] = v[2] | (v[3] << 32);
  }
}

// Second half: one thread per (replicate, column) walks the column's segments in order, adds
// the cross terms and writes the output row.
__global__ __launch_bounds__(BOOT_NT) void boot_combine_kernel(const u64* __restrict__ part,
                                                               int R, int C, BootGeom geo,
                                                               u64* __restrict__ out) {
  const int r = blockIdx.x * BOOT_NT + threadIdx.x, col = blockIdx.y;
  if (r >= R) return;
  const int s0 = col < C ? col * geo.sc : C * geo.sc, ns = col < C ? geo.sc : geo.sm;
  u64 u2 = 0, wp = 0, wn = 0, tp = 0, fp = 0;
  for (int ord = 0; ord < 2; ++ord) {
    u64 carry = 0;  // the negative weight of the segments before
    for (int k = 0; k < ns; ++k) {
      const u64* p = part + ((size_t)(ord * geo.s_tot + s0 + k) * R + r) * BOOT_PART;
      const u64 a = p[1], b = p[2];
      u2 += p[0] + (a & 0xffffffffu) * carry;
      carry += a >> 32;
      if (ord == 0) wp += a & 0xffffffffu, tp += b & 0xffffffffu, fp += b >> 32;
    }
    if (ord == 0) wn = carry;
  }
  u64* o = out + ((size_t)r * (C + 1) + col) * 5;
  o[0] = u2, o[1] = wp, o[2] = wn, o[3] = tp, o[4] = fp;
}

}  // namespace mmdx

using namespace mmdx;

extern "C" int mmdx_bootstrap_weights(int R, long r0, int N, uint64_t seed, int* w,
                                      void* stream) {
  MMDX_CHECK_ARG(w, "bootstrap_weights: null pointer");
  MMDX_CHECK_ARG(R > 0 && N > 0, "bootstrap_weights: empty (R = %d, N = %d)", R, N);
  MMDX_CHECK_ARG(r0 >= 0, "bootstrap_weights: r0 = %ld < 0", r0);
  MMDX_CHECK_ARG((long)R * N <= BOOT_MAX_WEIGHTS,
                 "bootstrap_weights: R * N = %ld exceeds the limit 2^26", (long)R * N);
  hipStream_t st = (hipStream_t)stream;
  if (N <= BOOT_LDS_N * BOOT_LDS_WINDOWS) {
    hipLaunchKernelGGL(boot_weights_lds_kernel, dim3(R, (N + BOOT_LDS_N - 1) / BOOT_LDS_N),
                       dim3(BOOT_NT), (size_t)std::min(N, BOOT_LDS_N) * sizeof(int), st, N, r0,
                       seed, w);
  } else {  // R < 2^26 / 2^17: a legal gridDim.y
    const hipError_t e = hipMemsetAsync(w, 0, (size_t)R * N * sizeof(int), st);
    MMDX_CHECK_ARG(e == hipSuccess, "bootstrap_weights: hipMemsetAsync: %s",
                   hipGetErrorString(e));
    const int gx = std::min((N + BOOT_NT * 8 - 1) / (BOOT_NT * 8), 1024);
    hipLaunchKernelGGL(boot_weights_atomic_kernel, dim3(gx, R), dim3(BOOT_NT), 0, st, N, r0,
                       seed, w);
  }
  MMDX_LAUNCH_CHECK();
  return 0;
}

static bool boot_counts_legal(int R, int N, int C) {
  return R > 0 && N > 0 && C > 0 && C <= CLS_MAX_C && (long)N * C <= BOOT_MAX_ITEMS &&
         (long)R * N <= BOOT_MAX_WEIGHTS;
}

// the workspace: the transposed weights [N][rp], then the segment partials
static inline size_t boot_wt_bytes(int R, int N) {
  return (size_t)N * ((R + BOOT_G - 1) / BOOT_G * BOOT_G) * sizeof(int);  // a multiple of 32
}

extern "C" size_t mmdx_bootstrap_counts_workspace_size(int R, int N, int C) {
  if (!boot_counts_legal(R, N, C)) return 0;
  return boot_wt_bytes(R, N) + (size_t)2 * boot_geom(N, C).s_tot * R * BOOT_PART * sizeof(u64);
}

extern "C" int mmdx_bootstrap_counts(const int* class_items, const int* micro_items,
                                     const int* weights, int R, int N, int C, int64_t* out,
                                     void* workspace, size_t ws_bytes, void* stream) {
  MMDX_CHECK_ARG(class_items && micro_items && weights && out && workspace,
                 "bootstrap_counts: null pointer");
  MMDX_CHECK_ARG(R > 0 && N > 0 && C > 0, "bootstrap_counts: empty (R = %d, N = %d, C = %d)", R,
                 N, C);
  MMDX_CHECK_ARG(C <= CLS_MAX_C, "bootstrap_counts: C = %d > %d", C, CLS_MAX_C);
  MMDX_CHECK_ARG((long)N * C <= BOOT_MAX_ITEMS,
                 "bootstrap_counts: N * C = %ld exceeds the limit 2^24", (long)N * C);
  MMDX_CHECK_ARG((long)R * N <= BOOT_MAX_WEIGHTS,
                 "bootstrap_counts: R * N = %ld exceeds the limit 2^26", (long)R * N);
  MMDX_CHECK_ARG((((uintptr_t)class_items | (uintptr_t)micro_items) & 15) == 0,
                 "bootstrap_counts: the item arrays must be 16-byte aligned");
  MMDX_CHECK_ARG(((uintptr_t)workspace & 15) == 0,
                 "bootstrap_counts: the workspace must be 16-byte aligned");
  const size_t need = mmdx_bootstrap_counts_workspace_size(R, N, C);
  MMDX_CHECK_ARG(ws_bytes >= need, "bootstrap_counts: workspace of %zu bytes, %zu needed",
                 ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const BootGeom geo = boot_geom(N, C);
  const int rp = (R + BOOT_G - 1) / BOOT_G * BOOT_G;
  int* wt = (int*)workspace;
  u64* part = (u64*)((char*)workspace + boot_wt_bytes(R, N));
  // <= 2^26 / 4096 + 2^20 + 2^18 + 1 tiles: a legal gridDim.x
  const long tiles = (long)((rp + BOOT_TT - 1) / BOOT_TT) * ((N + BOOT_TT - 1) / BOOT_TT);
  hipLaunchKernelGGL(boot_transpose_kernel, dim3((unsigned)tiles), dim3(BOOT_NT), 0, st, weights,
                     R, N, rp, wt);
  MMDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(boot_segments_kernel, dim3(rp / BOOT_G, 2 * geo.s_tot), dim3(BOOT_NT), 0,
                     st, class_items, micro_items, wt, R, rp, C, geo, part);
  MMDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(boot_combine_kernel, dim3((R + BOOT_NT - 1) / BOOT_NT, C + 1),
                     dim3(BOOT_NT), 0, st, (const u64*)part, R, C, geo, (u64*)out);
  MMDX_LAUNCH_CHECK();
  return 0;
}
