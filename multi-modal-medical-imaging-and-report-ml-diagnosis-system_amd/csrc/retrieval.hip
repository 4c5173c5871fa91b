// Similar-case retrieval: exact top-k inner-product search of nq queries against an [N][d] index
// (mmdx_topk_similar, the definition in include/mmdx.h and mmdx/retrieval.py: reference_search).
//
// Two launches on one stream, no atomics in global memory, no counter:
//   topk_select_kernel  one streaming pass over the index per group of 16 queries.  A block
//                       stages its 16 queries in LDS and walks chunks of TK_ROWS index rows
//                       (chunk = blockIdx.x, + gridDim.x, ...); each of its 4 waves scores two
//                       16-row tiles per chunk with MFMA over the whole of d (index rows are the
//                       A operand, straight from global memory at 16 bytes per lane; queries the
//                       B operand, from LDS) and offers the scores that beat the query's current
//                       k-th best to the query's candidate buffer in LDS.  The block's k best
//                       per query go to the workspace, sorted.
//   topk_merge_kernel   one block per query selects the k best of the blocks' sorted lists,
//                       rank by rank, and stops at the first rank at which no list's key passes.
//
// A candidate is ONE 64-bit key: the score's bits mapped to an unsigned that orders like the
// float (NaN as -inf, -0 as +0) in the high word, ~row in the low word.  A larger key is a better
// candidate under (score descending, id ascending); keys of distinct rows are distinct, 0 is "no
// candidate".  Selection is exact on the keys, so the result is the same whatever the grid and
// whatever order the LDS appends happen in; the score bits of a (query, row) pair come from one
// MFMA chain over d in a fixed order that depends on neither the row's tile nor its neighbours.
#include "common.h"

#include <mutex>
#include <set>

namespace mmdx {

typedef unsigned long long u64;

constexpr int TK_NT = 256;                        // 4 waves
constexpr int TK_QG = 16;                         // queries per group: the MFMA's B columns
constexpr int TK_ROWS = 128;                      // index rows per block step (2 tiles per wave)
constexpr int TK_MAX_K = 64;
constexpr int TK_MAX_NQ = 64;
constexpr int TK_MAX_D = 4096;
constexpr long TK_MAX_N = 1L << 24;
constexpr int TK_CAP = TK_MAX_K + 2 * TK_ROWS;    // candidate slots per query in LDS
constexpr int TK_CAP_E = TK_CAP / WAVE;           // ... per lane of the compacting wave
constexpr int TK_SEG = 2048;                      // staged bytes of a query row per d segment
constexpr int TK_QSTRIDE = TK_SEG + 16;           // + one access width: conflict-free b128 reads
constexpr int TK_MAX_BLOCKS = 512;                // select blocks over all query groups
static_assert(TK_CAP % WAVE == 0 && TK_CAP >= TK_MAX_K + TK_NT, "merge appends 256 per step");

__device__ __forceinline__ u64 tk_key(float s, int row) {
  unsigned b = __float_as_uint(s);
  if (s != s) b = 0xFF800000u;          // NaN counts as -inf
  if ((b << 1) == 0u) b = 0u;           // -0 ties with +0
  const unsigned o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((u64)o << 32) | (u64)(0xFFFFFFFFu - (unsigned)row);
}
__device__ __forceinline__ float tk_key_score(u64 key) {
  const unsigned o = (unsigned)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ int tk_key_row(u64 key) {
  return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
}

// One wave keeps the k largest of the n <= TK_CAP distinct keys in buf[0 .. n), sorted
// descending in buf[0 .. min(n, k)): every lane ranks its keys against all n (broadcast LDS
// reads), then stores the ones of rank < k at their rank.  Returns min(n, k).
template <int NE> __device__ __forceinline__ void tk_compact_ne(u64* buf, int n, int k, int lane) {
  u64 e[NE];
  int rank[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int idx = lane + i * WAVE;
    e[i] = idx < n ? buf[idx] : 0ull;
    rank[i] = 0;
  }
  for (int j = 0; j < n; ++j) {
    const u64 o = buf[j];
#pragma unroll
    for (int i = 0; i < NE; ++i) rank[i] += o > e[i] ? 1 : 0;
  }
#pragma unroll
  for (int i = 0; i < NE; ++i)
    if (lane + i * WAVE < n && rank[i] < k) buf[rank[i]] = e[i];
}
__device__ __forceinline__ int tk_compact(u64* buf, int n, int k, int lane) {
  const int ne = (n + WAVE - 1) / WAVE;   // wave-uniform
  if (ne <= 1) tk_compact_ne<1>(buf, n, k, lane);
  else if (ne == 2) tk_compact_ne<2>(buf, n, k, lane);
  else if (ne == 3) tk_compact_ne<3>(buf, n, k, lane);
  else tk_compact_ne<TK_CAP_E>(buf, n, k, lane);
  return n < k ? n : k;
}

// the 16 x 16 score tile: rows of A against rows of B over the 16 bytes each lane holds
template <typename T> struct TkMma;
template <> struct TkMma<f16> {
  static __device__ __forceinline__ f32x4 run(const u32x4& a, const u32x4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(*(const f16x8*)&a, *(const f16x8*)&b, c, 0, 0, 0);
  }
};
template <> struct TkMma<bf16> {
  static __device__ __forceinline__ f32x4 run(const u32x4& a, const u32x4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)&a, *(const bf16x8*)&b, c, 0, 0,
                                                   0);
  }
};
template <> struct TkMma<float> {   // exact fp32: four k-ordered fmaf chains of 4 products each
  static __device__ __forceinline__ f32x4 run(const u32x4& a, const u32x4& b, f32x4 c) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[e]), __uint_as_float(b[e]), c, 0,
                                               0, 0);
    return c;
  }
};

// LDS: [TK_QG][qstride] query bytes | u64 [TK_QG][TK_CAP] candidates | u64 thr[TK_QG] | int cnt[TK_QG]
static inline size_t tk_select_lds(long row_bytes) {
  const long seg = std::min<long>(row_bytes, TK_SEG);
  return (size_t)TK_QG * (seg + 16) + (size_t)TK_QG * TK_CAP * 8 + TK_QG * 8 + TK_QG * 4;
}

// Lane l of a wave holds bytes [64 s + 16 (l >> 4), + 16) of row (l & 15) of its tile in step s:
// the same bytes of the index row (A) and of the query row (B), so each product pairs equal t.
template <typename T>
__global__ __launch_bounds__(TK_NT) void topk_select_kernel(
    const T* __restrict__ queries, const T* __restrict__ index, int N, int d, int nq, int k,
    const int* __restrict__ exclude, u64* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * TK_QG, nqg = min(TK_QG, nq - q0);
  const long row_bytes = (long)d * (long)sizeof(T);
  const int seg_max = (int)min(row_bytes, (long)TK_SEG), qstride = seg_max + 16;
  const int nseg = (int)((row_bytes + TK_SEG - 1) / TK_SEG);
  unsigned char* qs = tk_smem;
  u64* buf = (u64*)(tk_smem + (size_t)TK_QG * qstride);
  u64* thr_s = buf + TK_QG * TK_CAP;
  int* cnt_s = (int*)(thr_s + TK_QG);
  if (tid < TK_QG) thr_s[tid] = 0ull, cnt_s[tid] = 0;

  const int qq = lane & 15, lq = lane >> 4;
  const int ex = (exclude && qq < nqg) ? exclude[q0 + qq] : -1;
  const unsigned char* qbase = (const unsigned char*)queries + (long)q0 * row_bytes;
  const unsigned char* bp = qs + qq * qstride + 16 * lq;
  const int nchunks = (N + TK_ROWS - 1) / TK_ROWS;
  bool staged = false;

  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int row0 = chunk * TK_ROWS + wave * 32;
    // rows past the end read row N - 1 (in bounds) and are dropped at the selection
    const unsigned char* ap0 = (const unsigned char*)index +
                               (long)min(row0 + qq, N - 1) * row_bytes + 16 * lq;
    const unsigned char* ap1 = (const unsigned char*)index +
                               (long)min(row0 + 16 + qq, N - 1) * row_bytes + 16 * lq;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int seg = 0; seg < nseg; ++seg) {
      const long seg_off = (long)seg * TK_SEG;
      const int seg_bytes = (int)min((long)TK_SEG, row_bytes - seg_off);
      if (!staged || nseg > 1) {   // block-uniform
        __syncthreads();
        const int vpr = seg_bytes >> 4;   // 16-byte vectors per query row
        for (int i = tid; i < TK_QG * vpr; i += TK_NT) {
          const int r = i / vpr, c = i - r * vpr;
          u32x4 v = {0u, 0u, 0u, 0u};
          if (r < nqg) v = *(const u32x4*)(qbase + (long)r * row_bytes + seg_off + 16 * c);
          *(u32x4*)(qs + r * qstride + 16 * c) = v;
        }
        __syncthreads();
        staged = true;
      }
      const int steps = seg_bytes >> 6;
      const unsigned char* a0 = ap0 + seg_off;
      const unsigned char* a1 = ap1 + seg_off;
      int s = 0;
      for (; s + 4 <= steps; s += 4) {   // eight 16-byte index loads in flight per lane
        u32x4 va0[4], va1[4], vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          va0[u] = *(const u32x4*)(a0 + 64 * (s + u));
          va1[u] = *(const u32x4*)(a1 + 64 * (s + u));
          vb[u] = *(const u32x4*)(bp + 64 * (s + u));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {    // ascending steps: the same chain as the tail loop
          acc0 = TkMma<T>::run(va0[u], vb[u], acc0);
          acc1 = TkMma<T>::run(va1[u], vb[u], acc1);
        }
      }
      for (; s < steps; ++s) {
        const u32x4 vb = *(const u32x4*)(bp + 64 * s);
        acc0 = TkMma<T>::run(*(const u32x4*)(a0 + 64 * s), vb, acc0);
        acc1 = TkMma<T>::run(*(const u32x4*)(a1 + 64 * s), vb, acc1);
      }
    }
    // C/D: lane holds query (lane & 15), rows 4 (lane >> 4) + j of each tile.  At most
    // TK_ROWS appends per query and chunk, onto at most TK_CAP - TK_ROWS kept ones.
    const u64 thr = thr_s[qq];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = row0 + t * 16 + lq * 4 + j;
        const float s = t == 0 ? acc0[j] : acc1[j];
        const bool valid = row < N && qq < nqg && row != ex;
        const u64 key = valid ? tk_key(s, row) : 0ull;
        if (key > thr) {
          const int pos = atomicAdd(&cnt_s[qq], 1);
          buf[qq * TK_CAP + pos] = key;
        }
      }
    __syncthreads();
    for (int i = 0; i < TK_QG / 4; ++i) {   // wave w owns queries 4 w .. 4 w + 3
      const int q = wave * (TK_QG / 4) + i;
      const int n = cnt_s[q];
      if (n > TK_CAP - TK_ROWS) {
        const int m = tk_compact(buf + q * TK_CAP, n, k, lane);
        if (lane == 0) cnt_s[q] = m, thr_s[q] = m >= k ? buf[q * TK_CAP + k - 1] : 0ull;
      }
    }
    __syncthreads();
  }
  // (every block has run at least one chunk: gridDim.x <= nchunks)
  for (int i = 0; i < TK_QG / 4; ++i) {
    const int q = wave * (TK_QG / 4) + i;
    if (q >= nqg) continue;
    const int m = tk_compact(buf + q * TK_CAP, cnt_s[q], k, lane);
    u64* dst = part + ((long)blockIdx.x * nq + (q0 + q)) * k;
    if (lane < k) dst[lane] = lane < m ? buf[q * TK_CAP + lane] : 0ull;
  }
}

// One block per query: the k best of the nparts sorted lists part[p][q][0 .. k).
__global__ __launch_bounds__(TK_NT) void topk_merge_kernel(const u64* __restrict__ part, int nparts,
                                                           int nq, int k,
                                                           float* __restrict__ out_scores,
                                                           int* __restrict__ out_ids) {
  __shared__ u64 buf[TK_CAP];
  __shared__ u64 thr_s;
  __shared__ int cnt_s;
  const int tid = threadIdx.x, lane = tid & 63, q = blockIdx.x;
  if (tid == 0) thr_s = 0ull, cnt_s = 0;
  __syncthreads();
  // Rank i of every list, best ranks first: after the heads the threshold is already the k-th
  // best head, and a rank at which no list's key passes ends the walk (the lists descend).
  int kept = 0;   // block-uniform: cnt_s behind the last compaction
  for (int i = 0; i < k; ++i) {
    int accepted = 0;
    for (int p0 = 0; p0 < nparts; p0 += TK_NT) {
      const int p = p0 + tid;
      const u64 key = p < nparts ? part[((long)p * nq + q) * k + i] : 0ull;
      if (key > thr_s) buf[atomicAdd(&cnt_s, 1)] = key;   // <= k kept + 256 new <= TK_CAP
      __syncthreads();
      const int n = cnt_s;
      accepted += n - kept;
      __syncthreads();   // every thread has read cnt_s and thr_s before wave 0 rewrites them
      if (tid < WAVE && n > k) {
        const int m = tk_compact(buf, n, k, lane);
        if (lane == 0) cnt_s = m, thr_s = buf[k - 1];
      }
      __syncthreads();
      kept = n < k ? n : k;
    }
    if (accepted == 0) break;
  }
  if (tid < WAVE) {
    const int m = tk_compact(buf, cnt_s, k, lane);
    if (lane < k) {
      const bool have = lane < m;
      const u64 e = have ? buf[lane] : 0ull;
      out_scores[(long)q * k + lane] = have ? tk_key_score(e) : -INFINITY;
      out_ids[(long)q * k + lane] = have ? tk_key_row(e) : -1;
    }
  }
}

static inline bool tk_shape_ok(long N, int d, int nq, int k) {
  return N >= 1 && N <= TK_MAX_N && d >= 32 && d <= TK_MAX_D && d % 32 == 0 && nq >= 1 &&
         nq <= TK_MAX_NQ && k >= 1 && k <= TK_MAX_K;
}
// select blocks per query group: a function of (N, nq) alone
static inline int tk_parts(long N, int nq) {
  const long nchunks = (N + TK_ROWS - 1) / TK_ROWS;
  const int groups = (nq + TK_QG - 1) / TK_QG;
  return (int)std::min<long>(nchunks, TK_MAX_BLOCKS / groups);
}

static void tk_lds_max_once(const void* kern) {
  static std::mutex mu;
  static std::set<std::pair<int, const void*>> done;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> g(mu);
  if (done.insert({dev, kern}).second)
    (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

template <typename T>
static void tk_select_launch(const void* queries, const void* index, int N, int d, int nq, int k,
                             const int* exclude, u64* part, hipStream_t st) {
  auto kern = topk_select_kernel<T>;
  tk_lds_max_once((const void*)kern);
  const dim3 grid((unsigned)tk_parts(N, nq), (unsigned)((nq + TK_QG - 1) / TK_QG));
  hipLaunchKernelGGL(kern, grid, dim3(TK_NT), tk_select_lds((long)d * sizeof(T)), st,
                     (const T*)queries, (const T*)index, N, d, nq, k, exclude, part);
}

}  // namespace mmdx

using namespace mmdx;

extern "C" int mmdx_topk_rows_per_block(void) { return TK_ROWS; }

extern "C" size_t mmdx_topk_similar_workspace_size(long N, int d, int nq, int k) {
  if (!tk_shape_ok(N, d, nq, k)) return 0;
  return (size_t)tk_parts(N, nq) * nq * k * sizeof(u64);
}

extern "C" int mmdx_topk_similar(void* stream, int dtype, const void* queries, const void* index,
                                 long N, int d, int nq, int k, const int* exclude,
                                 float* out_scores, int* out_ids, void* workspace,
                                 size_t ws_bytes) {
  MMDX_CHECK_ARG(dtype == F32 || dtype == BF16 || dtype == F16, "topk_similar: dtype %d", dtype);
  MMDX_CHECK_ARG(queries && index && out_scores && out_ids, "topk_similar: null pointer");
  MMDX_CHECK_ARG(N >= 1 && N <= TK_MAX_N, "topk_similar: N = %ld outside [1, 2^24]", N);
  MMDX_CHECK_ARG(d >= 32 && d <= TK_MAX_D && d % 32 == 0,
                 "topk_similar: d = %d (a multiple of 32 in [32, %d])", d, TK_MAX_D);
  MMDX_CHECK_ARG(nq >= 1 && nq <= TK_MAX_NQ, "topk_similar: nq = %d outside [1, %d]", nq,
                 TK_MAX_NQ);
  MMDX_CHECK_ARG(k >= 1 && k <= TK_MAX_K, "topk_similar: k = %d outside [1, %d]", k, TK_MAX_K);
  MMDX_CHECK_ARG((((uintptr_t)queries | (uintptr_t)index) & 15) == 0,
                 "topk_similar: queries and index must be 16-byte aligned");
  const size_t need = mmdx_topk_similar_workspace_size(N, d, nq, k);
  MMDX_CHECK_ARG(workspace && ws_bytes >= need && ((uintptr_t)workspace & 15) == 0,
                 "topk_similar: workspace null, unaligned or smaller than %zu bytes", need);
  const size_t es = dtype == F32 ? 4 : 2, ob = (size_t)nq * k * 4;
  const void* outs[3] = {out_scores, out_ids, workspace};
  const size_t outs_n[3] = {ob, ob, need};
  const void* ins[3] = {queries, index, exclude};
  const size_t ins_n[3] = {(size_t)nq * d * es, (size_t)N * d * es, (size_t)nq * 4};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) {
      const uintptr_t x = (uintptr_t)outs[a], y = (uintptr_t)ins[b];
      MMDX_CHECK_ARG(!(ins[b] && x < y + ins_n[b] && y < x + outs_n[a]),
                     "topk_similar: an output overlaps an input");
    }
    for (int b = a + 1; b < 3; ++b) {
      const uintptr_t x = (uintptr_t)outs[a], y = (uintptr_t)outs[b];
      MMDX_CHECK_ARG(!(x < y + outs_n[b] && y < x + outs_n[a]),
                     "topk_similar: two outputs overlap");
    }
  }
  // `exclude` lives on the device: its range [-1, N) is the caller's to check (functional.py
  // does, in one device reduction); an entry outside it matches no row and excludes nothing.
  hipStream_t st = (hipStream_t)stream;
  u64* part = (u64*)workspace;
  MMDX_DISPATCH(dtype, tk_select_launch<T>(queries, index, (int)N, d, nq, k, exclude, part, st));
  MMDX_LAUNCH_CHECK();
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)nq), dim3(TK_NT), 0, st, part,
                     tk_parts(N, nq), nq, k, out_scores, out_ids);
  MMDX_LAUNCH_CHECK();
  return 0;
}
