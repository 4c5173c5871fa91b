// Disease loss: weighted, masked, label-smoothed, focal BCE-with-logits (include/mmdx.h
// "disease loss"; the CPU statement is mmdx/losses.py: reference).
//
// One forward launch writes loss[0], stats [C][2], the normaliser and the un-normalised element
// gradient g; a second, elementwise launch scales g by dloss[0] / normaliser into dz.  No host
// sync, no float atomics: every sum meets in a fixed order, so the outputs are bit-reproducible.
// The layout and the cross-block hand-off are those of class_reduce.h.
#include "class_reduce.h"
#include "../../include/mmdx.h"

namespace mmdx {

enum { FOCAL_NONE = 0, FOCAL_SQUARE = 1, FOCAL_POW = 2 };

template <typename T, int FOCAL>
__global__ __launch_bounds__(CLS_NT) void disease_loss_fwd_kernel(
    const T* __restrict__ z, const float* __restrict__ y, long n, int C,
    const float* __restrict__ pos_weight, const float* __restrict__ class_weight, float gamma,
    float eps, int mean, float* __restrict__ loss, float* __restrict__ stats,
    float* __restrict__ norm, float* __restrict__ g, unsigned* counter, unsigned* part_e,
    unsigned* part_m) {
  __shared__ float red_e[CLS_NT];
  __shared__ unsigned red_m[CLS_NT];
  const int tid = threadIdx.x;
  const int TB = cls_tb(C), R = TB / C;
  const auto add = [&](int d, int s) { red_e[d] += red_e[s], red_m[d] += red_m[s]; };
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
        float p, q, t;  // sigmoid(z), 1 - sigmoid(z), exp(-|z|)
        sigmoid_parts(zi, &p, &q, &t);
        const float l1p = log1pf(t);
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
  rows_tree(tid, C, R, add);

  if (gridDim.x > 1) {
    if (tid < C) {
      cls_part_store(part_e + (long)blockIdx.x * C + tid, red_e[tid]);
      cls_part_store(part_m + (long)blockIdx.x * C + tid, red_m[tid]);
    }
    if (!cls_last_block(counter)) return;
    float pe = 0.f;
    unsigned pm = 0;
    cls_gather(tid, C, R, gridDim.x, [&](int blk, int k) {
      pe += cls_part_f32(part_e + (long)blk * C + k);
      pm += cls_part_load(part_m + (long)blk * C + k);
    });
    red_e[tid] = pe;
    red_m[tid] = pm;
    __syncthreads();
    rows_tree(tid, C, R, add);
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

}  // namespace mmdx

using namespace mmdx;

extern "C" size_t mmdx_disease_loss_workspace_size(long B, int C) {
  if (B <= 0 || C <= 0 || C > CLS_MAX_C || B > (long)INT32_MAX / C) return 0;
  return CLS_WS_HEAD + (size_t)cls_grid(B * C, C) * C * 2 * sizeof(float);
}

extern "C" int mmdx_disease_loss_fwd(int dtype, const void* logits, const float* target, long B,
                                     int C, const float* pos_weight, const float* class_weight,
                                     float gamma, float label_smoothing, int mean, float* loss,
                                     float* stats, float* norm, float* g, void* workspace,
                                     size_t ws_bytes, void* stream) {
  MMDX_CHECK_ARG(dtype == F32 || dtype == BF16 || dtype == F16, "disease_loss: dtype %d", dtype);
  MMDX_CHECK_ARG(logits && target && loss && stats && norm, "disease_loss: null pointer");
  MMDX_CHECK_ARG(B > 0 && C > 0, "disease_loss: empty (B = %ld, C = %d)", B, C);
  MMDX_CHECK_ARG(C <= CLS_MAX_C, "disease_loss: C = %d > %d", C, CLS_MAX_C);
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
  const int clash = ranges_clash(outs, outs_n, 5, ins, ins_n, 4);
  MMDX_CHECK_ARG(clash != CLASH_INPUT, "disease_loss: an output overlaps an input");
  MMDX_CHECK_ARG(clash != CLASH_OUTPUT, "disease_loss: two outputs overlap");
  hipStream_t st = (hipStream_t)stream;
  const int grid = cls_grid(n, C);
  unsigned* counter = (unsigned*)workspace;
  unsigned* part_e = (unsigned*)((char*)workspace + CLS_WS_HEAD);
  unsigned* part_m = part_e + (size_t)grid * C;
  if (grid > 1) {  // the ticket counter starts at 0 in every call (and every graph replay)
    const hipError_t e = hipMemsetAsync(workspace, 0, CLS_WS_HEAD, st);
    MMDX_CHECK_ARG(e == hipSuccess, "disease_loss: hipMemsetAsync: %s", hipGetErrorString(e));
  }
#define LOSS_LAUNCH(FOCAL)                                                                      \
  MMDX_DISPATCH(dtype, hipLaunchKernelGGL((disease_loss_fwd_kernel<T, FOCAL>), dim3(grid),      \
                                          dim3(CLS_NT), 0, st, (const T*)logits, target, n, C,  \
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
  MMDX_CHECK_ARG(!ranges_overlap(dlogits, (size_t)n * (dtype == F32 ? 4 : 2), g, (size_t)n * 4),
                 "disease_loss_bwd: dlogits overlaps g");
  MMDX_DISPATCH(dtype, hipLaunchKernelGGL(disease_loss_bwd_kernel<T>, dim3(grid_for(n)),
                                          dim3(CLS_NT), 0, (hipStream_t)stream, g, n, dloss,
                                          norm, (T*)dlogits));
  MMDX_LAUNCH_CHECK();
  return 0;
}
