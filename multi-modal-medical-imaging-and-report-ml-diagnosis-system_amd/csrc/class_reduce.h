// The class-aligned reduction of the validation-path kernels: per-class sums over an [N][C] array
// in a fixed order, across blocks, without float atomics: disease_loss_fwd_kernel (loss.hip, one
// float and one count per class) and calib_fit_kernel (calibration.hip, seven doubles).  Also what
// else these and the metrics kernels share: sigmoid, edge search, class cap, overlap check.
//
// Layout.  A block uses TB = cls_tb(C) of its CLS_NT threads, the largest multiple of C; thread
// t = blockIdx * TB + tid walks elements t, t + S, t + 2S, ... with S = gridDim * TB.  TB and S
// are multiples of C, so a thread stays in class tid % C for the whole loop and the threads of a
// block form R = TB / C rows of C classes: the per-class sums are one LDS tree over the rows
// (rows_tree).  With more than one block, each block stores its C partial sums in the workspace
// (cls_part_store) and takes a ticket from an integer counter (cls_last_block); the block that
// draws the last ticket adds the partials in block order (cls_gather, then the same row tree), so
// the order of every addition is a function of (N, C) alone.  The element loop loads one element
// per lane: it is bound by its expf / logf / powf, not by the bytes it reads.
#pragma once
#include "common.h"

namespace mmdx {

typedef unsigned long long u64;

constexpr int CLS_NT = 256;          // threads per block
constexpr int CLS_MAX_C = 64;        // classes: the loss, the calibration and the metrics kernels
constexpr int CLS_PER_THREAD = 8;    // elements per thread before the grid grows
constexpr int CLS_MAX_BLOCKS = 1024;
constexpr size_t CLS_WS_HEAD = 16;   // the ticket counter, padded to 16 bytes

__host__ __device__ inline int cls_tb(int C) { return (CLS_NT / C) * C; }
static inline int cls_grid(long n, int C) {
  const long per = (long)cls_tb(C) * CLS_PER_THREAD;
  return (int)std::max<long>(1, std::min<long>((n + per - 1) / per, CLS_MAX_BLOCKS));
}

// The caller's LDS arrays hold R rows of C values at [row * C + class]; afterwards row 0 is the
// sum over the rows, added pairwise in a fixed order.  add(dst, src) does the kernel's own `+=`
// on each of its arrays.  Every thread calls it, behind the barrier that follows the row writes.
template <typename Add> __device__ __forceinline__ void rows_tree(int tid, int C, int R, Add add) {
  int s = 1;
  while (s < R) s <<= 1;
  for (s >>= 1; s >= 1; s >>= 1) {
    if (tid < s * C && tid + s * C < R * C) add(tid, tid + s * C);
    __syncthreads();
  }
}

// A block's partial sums cross to the last block through relaxed agent-scope atomics on both
// sides (a plain load may come from a cache the store never reached); floats travel as bits.
template <typename U> __device__ __forceinline__ void cls_part_store(U* p, U v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename U> __device__ __forceinline__ U cls_part_load(const U* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cls_part_store(unsigned* p, float v) {
  cls_part_store(p, __float_as_uint(v));
}
__device__ __forceinline__ void cls_part_store(u64* p, double v) {
  cls_part_store(p, (u64)__double_as_longlong(v));
}
__device__ __forceinline__ float cls_part_f32(const unsigned* p) {
  return __uint_as_float(cls_part_load(p));
}
__device__ __forceinline__ double cls_part_f64(const u64* p) {
  return __longlong_as_double((long long)cls_part_load(p));
}

// The cross-block hand-off.  In a grid of more than one block, every thread of every block calls
// it once per launch, after the threads that hold the block's partials have ISSUED their
// cls_part_store calls.  It returns true in all threads of the block that drew the last ticket
// and false in all threads of every other block, which then leave.
// - Each storing wave drains its own stores (s_waitcnt vmcnt(0)) ahead of the barrier, so that
//   thread 0's release fence covers the whole block's partials before it draws the ticket.
// - After a true return the partials of every block are visible to this block (the acquire fence
//   behind the last ticket).  Read them with cls_part_load / _f32 / _f64, which are agent-scope
//   atomic loads, never through plain or scalar-cache loads.
// - The counter must be 0 when the first block of a launch arrives; zeroing it stays with the
//   caller: a memset per call in the loss; in the fit a memset in pass 0, then the last block
//   stores 0 for the next pass (by then every block has drawn).
__device__ __forceinline__ bool cls_last_block(unsigned* counter) {
  __shared__ unsigned ticket_s;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its stores
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned ticket =
        __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == gridDim.x - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    ticket_s = ticket;
  }
  __syncthreads();
  return ticket_s == gridDim.x - 1;
}

// The same hand-off for a grid that holds several independent groups of `nblocks` blocks, each
// group with a counter of its own (token_relevance_step_kernel: the query tiles of one sample).
// (A form of its own: routing the one above through it changed the instructions of its users.)
__device__ __forceinline__ bool cls_last_of_group(unsigned* counter, unsigned nblocks) {
  __shared__ unsigned ticket_s;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its stores
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned ticket =
        __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == nblocks - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    ticket_s = ticket;
  }
  __syncthreads();
  return ticket_s == nblocks - 1;
}

// The last block's walk over the partials: thread tid takes the blocks tid / C, tid / C + R, ...
// of class tid % C, in that order; f(blk, c) accumulates into the caller's registers.
template <typename F>
__device__ __forceinline__ void cls_gather(int tid, int C, int R, int nblocks, F f) {
  if (tid >= R * C) return;
  for (int blk = tid / C; blk < nblocks; blk += R) f(blk, tid % C);
}

// t = exp(-|z|) in [0, 1]: p = sigmoid(z) and q = sigmoid(-z) = 1 - p of either sign without
// overflow; softplus(+-z) = max(+-z, 0) + log1pf(t) where the caller needs it.
__device__ __forceinline__ void sigmoid_parts(float z, float* p, float* q, float* t) {
  *t = expf(-fabsf(z));
  const float hi = 1.f / (1.f + *t), lo = *t / (1.f + *t);
  *p = z >= 0.f ? hi : lo, *q = z >= 0.f ? lo : hi;
}

// #{k < n : edges[k] <= x} for sorted edges in LDS (the first k with edges[k] > x); 0 for a NaN
__device__ __forceinline__ int upper_bound_lds(const float* edges, int n, float x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (edges[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

static inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + nb && y < x + na;
}

// Host: every output against every input and every later output (null overlaps nothing).
enum { CLASH_NONE = 0, CLASH_INPUT, CLASH_OUTPUT };
static inline int ranges_clash(const void* const* outs, const size_t* outs_n, int n_out,
                               const void* const* ins, const size_t* ins_n, int n_in) {
  for (int a = 0; a < n_out; ++a) {
    for (int b = 0; b < n_in; ++b)
      if (ranges_overlap(outs[a], outs_n[a], ins[b], ins_n[b])) return CLASH_INPUT;
    for (int b = a + 1; b < n_out; ++b)
      if (ranges_overlap(outs[a], outs_n[a], outs[b], outs_n[b])) return CLASH_OUTPUT;
  }
  return CLASH_NONE;
}

}  // namespace mmdx
