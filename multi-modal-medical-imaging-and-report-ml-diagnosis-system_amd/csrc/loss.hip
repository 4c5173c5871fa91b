// Disease loss: weighted, masked, label-smoothed, focal BCE-with-logits (include/mmdx.h
// "disease loss"; the CPU statement is mmdx/losses.py: reference).
//
// One forward launch writes loss[0], stats [C][2], the normaliser and the un-normalised element
// gradient g; a second, elementwise launch scales g by dloss[0] / normaliser into dz.  No host
// sync, no float atomics: every sum meets in a fixed order, so the outputs are bit-reproducible.
//
// Layout.  A block uses TB = (256 / C) * C of its 256 threads; thread t = blockIdx * TB + tid
// walks elements t, t + S, t + 2S, ... with S = gridDim * TB.  TB and S are multiples of C, so
// a thread stays in class tid % C for the whole loop and the threads of a block form R = TB / C
// rows of C classes: the per-class sums are one LDS tree over the rows.  With more than one
// block, each block stores its C partial sums in the workspace and takes a ticket from an integer
// counter; the block that draws the last ticket adds the partials in block order (the same row
// tree), so the order is a function of (B, C) alone.  The hand-off is the agent-scope
// release / acquire pair around the ticket; the partials are read with agent-scope atomic loads,
// never through the scalar cache.  The loads are one element per lane: the loop is bound by its
// expf / logf / powf, not by the 8 bytes per element it reads.
#include "common.h"
#include "../../include/mmdx.h"

namespace mmdx {

constexpr int LOSS_NT = 256;          // threads per block
constexpr int LOSS_MAX_C = 64;        // as the metrics kernels
constexpr int LOSS_PER_THREAD = 8;    // elements per thread before the grid grows
constexpr int LOSS_MAX_BLOCKS = 1024;
constexpr size_t LOSS_WS_HEAD = 16;   // the ticket counter, padded to 16 bytes

enum { FOCAL_NONE = 0, FOCAL_SQUARE = 1, FOCAL_POW = 2 };

static inline int loss_tb(int C) { return (LOSS_NT / C) * C; }
static inline int loss_grid(long n, int C) {
  const long per = (long)loss_tb(C) * LOSS_PER_THREAD;
  return (int)std::max<long>(1, std::min<long>((n + per - 1) / per, LOSS_MAX_BLOCKS));
}

// red_e / red_m hold R rows of C values; afterwards row 0 is the sum over the rows, added
// pairwise in a fixed order.  Every thread of the block calls it.
__device__ __forceinline__ void rows_tree(float* red_e, unsigned* red_m, int tid, int C, int R) {
  int s = 1;
  while (s < R) s <<= 1;
  for (s >>= 1; s >= 1; s >>= 1) {
    if (tid < s * C && tid + s * C < R * C) {
      red_e[tid] += red_e[tid + s * C];
      red_m[tid] += red_m[tid + s * C];
    }
    __syncthreads();
  }
}

template <typename T, int FOCAL>
__global__ __launch_bounds__(LOSS_NT) void disease_loss_fwd_kernel(
    const T* __restrict__ z, const float* __restrict__ y, long n, int C,
    const float* __restrict__ pos_weight, const float* __restrict__ class_weight, float gamma,
    float eps, int mean, float* __restrict__ loss, float* __restrict__ stats,
    float* __restrict__ norm, float* __restrict__ g, unsigned* counter, unsigned* part_e,
    unsigned* part_m) {
  __shared__ float red_e[LOSS_NT];
  __shared__ unsigned red_m[LOSS_NT];
  __shared__ unsigned ticket_s;
  const int tid = threadIdx.x;
  const int TB = (LOSS_NT / C) * C, R = TB / C;
  const int c = tid % C;
  const long S = (long)gridDim.x * TB;

  float acc = 0.f;
  unsigned cnt = 0;
  if (tid < TB) {
    const float pw = pos_weight ? pos_weight[c] : 1.f;
    const float cw = class_weight ? class_weight[c] : 1.f;
    for (long i = (long)blockIdx.x * TB + tid; i < n; i += S) {
      const float zi = to_f(z[i]), yi = y[i];
      float e = 0.f, gi = 0.f;
      if (yi == yi) {  // a NaN target is "no label"
        const float ys = yi * (1.f - eps) + 0.5f * eps;
        // t = exp(-|z|) in [0, 1]: sigmoid and softplus of either sign without overflow
        const float t = expf(-fabsf(zi));
        const float l1p = log1pf(t);
        const float hi = 1.f / (1.f + t), lo = t / (1.f + t);
        const float p = zi >= 0.f ? hi : lo, q = zi >= 0.f ? lo : hi;  // sigmoid(z), 1 - sigmoid(z)
        const float sp_pos = fmaxf(zi, 0.f) + l1p;                      // softplus(z)
        const float sp_neg = fmaxf(-zi, 0.f) + l1p;                     // softplus(-z)
        const float bce = pw * ys * sp_neg + (1.f - ys) * sp_pos;
        const float dbce = (1.f - ys) * p - pw * ys * q;                // d bce / dz
        if (FOCAL == FOCAL_NONE) {
          e = cw * bce;
          gi = cw * dbce;
        } else {
          const float d = p - ys, ad = fabsf(d);
          // w1 = |d|^(gamma - 1), w = |d|^gamma
          const float w1 = FOCAL == FOCAL_SQUARE ? ad : powf(ad, gamma - 1.f);
          const float w = w1 * ad;
          const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
          // p q is exactly 0 wherever |z| is large enough for bce to overflow
          const float pq = p * q;
          const float pqb = pq == 0.f ? 0.f : pq * bce;
          e = cw * (w * bce);
          gi = cw * (gamma * w1 * sgn * pqb + w * dbce);
        }
        cnt += 1;
      }
      acc += e;
      if (g) g[i] = gi;
    }
  }
  red_e[tid] = acc;
  red_m[tid] = cnt;
  __syncthreads();
  rows_tree(red_e, red_m, tid, C, R);

  if (gridDim.x > 1) {
    if (tid < C) {
      __hip_atomic_store(part_e + (long)blockIdx.x * C + tid, __float_as_uint(red_e[tid]),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(part_m + (long)blockIdx.x * C + tid, red_m[tid], __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its stores
    __syncthreads();
    if (tid == 0) {
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
    if (ticket_s != gridDim.x - 1) return;
    // the last block: every block's partials are visible; add them in block order
    float pe = 0.f;
    unsigned pm = 0;
    if (tid < TB) {
      const long total = (long)gridDim.x * C;
      for (long j = tid; j < total; j += TB) {
        pe += __uint_as_float(
            __hip_atomic_load(part_e + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        pm += __hip_atomic_load(part_m + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    red_e[tid] = pe;
    red_m[tid] = pm;
    __syncthreads();
    rows_tree(red_e, red_m, tid, C, R);
  }

  if (tid < C) {
    stats[2 * tid] = red_e[tid];
    stats[2 * tid + 1] = (float)red_m[tid];
  }
  if (tid == 0) {
    float e = 0.f;
    unsigned m = 0;
    for (int k = 0; k < C; ++k) {
      e += red_e[k];
      m += red_m[k];
    }
    const float nrm = mean ? (float)(m > 0u ? m : 1u) : 1.f;
    norm[0] = nrm;
    loss[0] = e / nrm;
  }
}

template <typename T>
__global__ void disease_loss_bwd_kernel(const float* __restrict__ g, long n,
                                        const float* __restrict__ dloss,
                                        const float* __restrict__ norm, T* __restrict__ dz) {
  const float s = (dloss ? dloss[0] : 1.f) / norm[0];
  GRID_STRIDE(i, n) dz[i] = from_f<T>(g[i] * s);
}

static inline bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + nb && y < x + na;
}

}  // namespace mmdx

using namespace mmdx;

extern "C" size_t mmdx_disease_loss_workspace_size(long B, int C) {
  if (B <= 0 || C <= 0 || C > LOSS_MAX_C || B > (long)INT32_MAX / C) return 0;
  return LOSS_WS_HEAD + (size_t)loss_grid(B * C, C) * C * 2 * sizeof(float);
}

extern "C" int mmdx_disease_loss_fwd(int dtype, const void* logits, const float* target, long B,
                                     int C, const float* pos_weight, const float* class_weight,
                                     float gamma, float label_smoothing, int mean, float* loss,
                                     float* stats, float* norm, float* g, void* workspace,
                                     size_t ws_bytes, void* stream) {
  MMDX_CHECK_ARG(dtype == F32 || dtype == BF16 || dtype == F16, "disease_loss: dtype %d", dtype);
  MMDX_CHECK_ARG(logits && target && loss && stats && norm, "disease_loss: null pointer");
  MMDX_CHECK_ARG(B > 0 && C > 0, "disease_loss: empty (B = %ld, C = %d)", B, C);
  MMDX_CHECK_ARG(C <= LOSS_MAX_C, "disease_loss: C = %d > %d", C, LOSS_MAX_C);
  MMDX_CHECK_ARG(B <= (long)INT32_MAX / C, "disease_loss: B * C exceeds 2^31 - 1 (B = %ld)", B);
  MMDX_CHECK_ARG(gamma == 0.f || (gamma >= 1.f && gamma < INFINITY),
                 "disease_loss: gamma = %g (0 or a finite value >= 1)", (double)gamma);
  MMDX_CHECK_ARG(label_smoothing >= 0.f && label_smoothing < 1.f,
                 "disease_loss: label_smoothing = %g outside [0, 1)", (double)label_smoothing);
  const long n = B * C;
  const size_t zb = (size_t)n * (dtype == F32 ? 4 : 2), fb = (size_t)n * 4, cb = (size_t)C * 4;
  const size_t need = mmdx_disease_loss_workspace_size(B, C);
  MMDX_CHECK_ARG(workspace && ws_bytes >= need && ((uintptr_t)workspace & 15) == 0,
                 "disease_loss: workspace null, unaligned or smaller than %zu bytes", need);
  // outputs against the inputs and against each other
  const void* outs[5] = {loss, stats, norm, g, workspace};
  const size_t outs_n[5] = {4, 2 * cb, 4, fb, need};
  const void* ins[4] = {logits, target, pos_weight, class_weight};
  const size_t ins_n[4] = {zb, fb, cb, cb};
  for (int a = 0; a < 5; ++a) {
    for (int b = 0; b < 4; ++b)
      MMDX_CHECK_ARG(!overlaps(outs[a], outs_n[a], ins[b], ins_n[b]),
                     "disease_loss: an output overlaps an input");
    for (int b = a + 1; b < 5; ++b)
      MMDX_CHECK_ARG(!overlaps(outs[a], outs_n[a], outs[b], outs_n[b]),
                     "disease_loss: two outputs overlap");
  }
  hipStream_t st = (hipStream_t)stream;
  const int grid = loss_grid(n, C);
  unsigned* counter = (unsigned*)workspace;
  unsigned* part_e = (unsigned*)((char*)workspace + LOSS_WS_HEAD);
  unsigned* part_m = part_e + (size_t)grid * C;
  if (grid > 1) {  // the ticket counter starts at 0 in every call (and every graph replay)
    const hipError_t e = hipMemsetAsync(workspace, 0, LOSS_WS_HEAD, st);
    MMDX_CHECK_ARG(e == hipSuccess, "disease_loss: hipMemsetAsync: %s", hipGetErrorString(e));
  }
#define LOSS_LAUNCH(FOCAL)                                                                      \
  MMDX_DISPATCH(dtype, hipLaunchKernelGGL((disease_loss_fwd_kernel<T, FOCAL>), dim3(grid),      \
                                          dim3(LOSS_NT), 0, st, (const T*)logits, target, n, C, \
                                          pos_weight, class_weight, gamma, label_smoothing,     \
                                          mean, loss, stats, norm, g, counter, part_e, part_m))
  if (gamma == 0.f)
    LOSS_LAUNCH(FOCAL_NONE);
  else if (gamma == 2.f)
    LOSS_LAUNCH(FOCAL_SQUARE);
  else
    LOSS_LAUNCH(FOCAL_POW);
#undef LOSS_LAUNCH
  MMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmdx_disease_loss_bwd(int dtype, const float* g, long n, const float* dloss,
                                     const float* norm, void* dlogits, void* stream) {
  MMDX_CHECK_ARG(dtype == F32 || dtype == BF16 || dtype == F16, "disease_loss_bwd: dtype %d",
                 dtype);
  MMDX_CHECK_ARG(g && norm && dlogits, "disease_loss_bwd: null pointer");
  MMDX_CHECK_ARG(n > 0 && n <= (long)INT32_MAX, "disease_loss_bwd: n = %ld", n);
  MMDX_CHECK_ARG(!overlaps(dlogits, (size_t)n * (dtype == F32 ? 4 : 2), g, (size_t)n * 4),
                 "disease_loss_bwd: dlogits overlaps g");
  MMDX_DISPATCH(dtype, hipLaunchKernelGGL(disease_loss_bwd_kernel<T>, dim3(grid_for(n)),
                                          dim3(LOSS_NT), 0, (hipStream_t)stream, g, n, dloss,
                                          norm, (T*)dlogits));
  MMDX_LAUNCH_CHECK();
  return 0;
}
