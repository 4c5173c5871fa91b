// Probability calibration of the disease head (include/mmdx.h "calibration"; the CPU statement
// is mmdx/calibration.py: reference_fit, calibration_from_bins).
//
// calib_fit_kernel is ONE damped-Newton pass of the temperature / Platt fit z' = a_c z + b_c:
// the seven per-class sums (NLL, ga, gb, haa, hab, hbb, labelled count) of the whole [N][C]
// problem, then the accept / reject decision and the next trial point, all in one launch.  A fit
// is iters + 1 such launches on one stream with no host sync between them; the state (trial
// point, accepted point and its sums, lambda) lives in the workspace.
//
// Layout and hand-off: the class-aligned reduction of class_reduce.h.  The element terms are
// fp32 (one max-shifted expf, one log1pf); the sums are fp64 from the thread upward.  No float
// atomics: the result is a function of (N, C, data) alone, bit-reproducible.
//
// reliability_bins_kernel counts, per class and probability bin, the elements, the positives and
// the fixed-point sums of p and (p - y)^2: the upper-bound search over LDS-resident edges and
// the per-block LDS histogram of confusion_grid_kernel (metrics.hip), integer atomics only.
#include <math.h>

#include "class_reduce.h"
#include "../../include/mmdx.h"

namespace mmdx {

constexpr int CAL_NSUM = 7;          // NLL, ga, gb, haa, hab, hbb, labelled count
constexpr int CAL_STATE = 16;        // doubles of state per class
constexpr double CAL_LAMBDA0 = 1e-3, CAL_LAMBDA_MIN = 1e-9, CAL_LAMBDA_MAX = 1e12;
constexpr double CAL_SLACK = 1e-9;   // relative slack of the acceptance test
constexpr long REL_MAX_ITEMS = 1L << 24;
constexpr int REL_MAX_BINS = 64;
constexpr int REL_CELLS = 1536;      // (class, bin) cells of 4 x u64 per block: 48 KiB

// the state row of a class (doubles)
enum { ST_A = 0, ST_B, ST_LAMBDA, ST_A_ACC, ST_B_ACC, ST_F_ACC, ST_GA, ST_GB, ST_HAA, ST_HAB,
       ST_HBB, ST_F0, ST_N };

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) < INFINITY; }

__global__ __launch_bounds__(CLS_NT) void calib_fit_kernel(
    const float* __restrict__ z, const float* __restrict__ y, long n, int C,
    const double* __restrict__ counts, int smooth, int temperature, int first, int last,
    double min_count, double tol, float* __restrict__ scale, float* __restrict__ bias,
    int* __restrict__ status, double* __restrict__ info, unsigned* counter, double* state,
    u64* part) {
  __shared__ double red[CAL_NSUM * CLS_NT];  // CAL_NSUM planes of R rows of C values
  const int tid = threadIdx.x;
  const int TB = cls_tb(C), R = TB / C;
  const auto add = [&](int dst, int src) {
#pragma unroll
    for (int k = 0; k < CAL_NSUM; ++k) red[k * CLS_NT + dst] += red[k * CLS_NT + src];
  };
  const int c = tid % C;
  const long S = (long)gridDim.x * TB;

  double acc[CAL_NSUM] = {};
  if (tid < TB) {
    // the trial point, as fp32: the first pass starts at the identity whatever the state holds
    const float a = first ? 1.f : (float)state[c * CAL_STATE + ST_A];
    const float b = first ? 0.f : (float)state[c * CAL_STATE + ST_B];
    float t_neg = 0.f, t_pos = 1.f;
    if (smooth) {  // Platt's targets from the label counts
      t_pos = (float)((counts[2 * c] + 1.0) / (counts[2 * c] + 2.0));
      t_neg = (float)(1.0 / (counts[2 * c + 1] + 2.0));
    }
    const float t_dif = t_pos - t_neg;
    for (long i = (long)blockIdx.x * TB + tid; i < n; i += S) {
      const float zi = z[i], yi = y[i];
      if (yi == yi) {  // a NaN target is "no label"
        const float u = __fadd_rn(__fmul_rn(a, zi), b);  // never contracted: z' as the host has it
        const float tt = t_neg + yi * t_dif;
        float pf, qf, e;  // sigmoid(u), sigmoid(-u), exp(-|u|)
        sigmoid_parts(u, &pf, &qf, &e);
        const float l1p = log1pf(e);
        const double p = pf, q = qf, ud = u, zd = zi, td = tt;
        const double d = p - td, w = p * q;
        acc[0] += fmax(ud, 0.0) + (double)l1p - td * ud;
        acc[1] += d * zd;
        acc[2] += d;
        acc[3] += w * zd * zd;
        acc[4] += w * zd;
        acc[5] += w;
        acc[6] += 1.0;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CAL_NSUM; ++k) red[k * CLS_NT + tid] = acc[k];
  __syncthreads();
  rows_tree(tid, C, R, add);

  if (gridDim.x > 1) {
    if (tid < C) {
#pragma unroll
      for (int k = 0; k < CAL_NSUM; ++k)
        cls_part_store(part + ((long)blockIdx.x * CAL_NSUM + k) * C + tid, red[k * CLS_NT + tid]);
    }
    if (!cls_last_block(counter)) return;
#pragma unroll
    for (int k = 0; k < CAL_NSUM; ++k) acc[k] = 0.0;
    cls_gather(tid, C, R, gridDim.x, [&](int blk, int cls) {
#pragma unroll
      for (int k = 0; k < CAL_NSUM; ++k)
        acc[k] += cls_part_f64(part + ((long)blk * CAL_NSUM + k) * C + cls);
    });
#pragma unroll
    for (int k = 0; k < CAL_NSUM; ++k) red[k * CLS_NT + tid] = acc[k];
    __syncthreads();
    rows_tree(tid, C, R, add);
    // every block has drawn its ticket: the counter is ready for the next launch on the stream
    if (tid == 0) cls_part_store(counter, 0u);
  }

  if (tid >= C) return;
  // ---- the solver step of class tid (temperature: every class computes the same pooled step)
  double s[CAL_NSUM], n_pos, n_neg;
  if (temperature) {
#pragma unroll
    for (int k = 0; k < CAL_NSUM; ++k) s[k] = 0.0;
    n_pos = n_neg = 0.0;
    for (int j = 0; j < C; ++j) {  // class order
#pragma unroll
      for (int k = 0; k < CAL_NSUM; ++k) s[k] += red[k * CLS_NT + j];
      n_pos += counts[2 * j];
      n_neg += counts[2 * j + 1];
    }
  } else {
#pragma unroll
    for (int k = 0; k < CAL_NSUM; ++k) s[k] = red[k * CLS_NT + tid];
    n_pos = counts[2 * tid];
    n_neg = counts[2 * tid + 1];
  }
  double* st = state + tid * CAL_STATE;
  const double a_t = first ? 1.0 : (double)(float)st[ST_A];
  const double b_t = first ? 0.0 : (double)(float)st[ST_B];
  double lam = first ? CAL_LAMBDA0 : st[ST_LAMBDA];
  double a_acc = first ? 1.0 : st[ST_A_ACC], b_acc = first ? 0.0 : st[ST_B_ACC];
  double f_acc = first ? (double)INFINITY : st[ST_F_ACC];
  double ga = first ? 0.0 : st[ST_GA], gb = first ? 0.0 : st[ST_GB];
  double haa = first ? 0.0 : st[ST_HAA], hab = first ? 0.0 : st[ST_HAB];
  double hbb = first ? 0.0 : st[ST_HBB];
  const double f0 = first ? s[0] : st[ST_F0];
  const double nl = first ? s[6] : st[ST_N];
  // a NaN NLL fails the compare and is rejected
  if (s[0] <= f_acc + CAL_SLACK * fabs(f_acc)) {
    a_acc = a_t, b_acc = b_t, f_acc = s[0];
    ga = s[1], gb = s[2], haa = s[3], hab = s[4], hbb = s[5];
    lam = fmax(lam / 10.0, CAL_LAMBDA_MIN);
  } else {
    lam = fmin(lam * 10.0, CAL_LAMBDA_MAX);
  }

  if (!last) {
    double da = 0.0, db = 0.0;
    if (temperature) {
      const double den = haa * (1.0 + lam);
      if (finite_d(den) && den > 0.0 && finite_d(ga)) da = ga / den;
    } else {
      const double A = haa * (1.0 + lam), D = hbb * (1.0 + lam);
      const double det = A * D - hab * hab;
      if (finite_d(det) && det > 0.0 && finite_d(ga) && finite_d(gb)) {
        da = (D * ga - hab * gb) / det;
        db = (A * gb - hab * ga) / det;
      }
    }
    st[ST_A] = (double)(float)(a_acc - da);  // the next pass evaluates at the fp32 rounding
    st[ST_B] = (double)(float)(b_acc - db);
    st[ST_LAMBDA] = lam;
    st[ST_A_ACC] = a_acc, st[ST_B_ACC] = b_acc, st[ST_F_ACC] = f_acc;
    st[ST_GA] = ga, st[ST_GB] = gb, st[ST_HAA] = haa, st[ST_HAB] = hab, st[ST_HBB] = hbb;
    st[ST_F0] = f0, st[ST_N] = nl;
    return;
  }
  // ---- the final pass: the Newton decrement at the accepted point and the status rules
  const double quad = hbb * ga * ga - 2.0 * hab * ga * gb + haa * gb * gb;
  double dec = temperature ? ga * ga / haa : quad / (haa * hbb - hab * hab);
  dec /= fmax(nl, 1.0);
  const bool fin = finite_d(f_acc) && finite_d(dec) && finite_d(a_acc) && finite_d(b_acc);
  int code = 0;
  if (n_pos < min_count || n_neg < min_count || nl < 1.0) code = 1;
  else if (!fin || !(dec <= tol)) code = 2;
  else if (a_acc <= 0.0) code = 3;
  scale[tid] = code == 0 ? (float)a_acc : 1.f;
  bias[tid] = code == 0 ? (float)b_acc : 0.f;
  status[tid] = code;
  info[4 * tid + 0] = f0;
  info[4 * tid + 1] = f_acc;
  info[4 * tid + 2] = dec;
  info[4 * tid + 3] = nl;
}

// Per element: z' (an explicit multiply and add, or z itself), its bin k = #{edges <= z'} by
// binary search over the sorted edges in LDS, p = sigmoid(z') and (p - y)^2 with 1 - p taken as
// sigmoid(-z'), both rounded to multiples of 2^-30.  A block covers the classes
// [blockIdx.y * CC, + CC) so that the histogram fits LDS for every legal (C, n_bins); the micro
// row is the sum of the block's class rows, so the element loop has no single hot cell.
__global__ __launch_bounds__(CLS_NT) void reliability_bins_kernel(
    const float* __restrict__ logits, const float* __restrict__ target, int N, int C,
    const float* __restrict__ scale, const float* __restrict__ bias,
    const float* __restrict__ edges, int n_bins, int CC, u64* __restrict__ out) {
  __shared__ u64 hist[REL_CELLS * 4];           // [cc][n_bins][4]
  __shared__ unsigned nanc[CLS_MAX_C];
  __shared__ float sedge[REL_MAX_BINS];
  const int t = threadIdx.x;
  const int c0 = blockIdx.y * CC;
  const int cc = min(CC, C - c0);
  const int T = n_bins - 1;
  for (int q = t; q < T; q += CLS_NT) sedge[q] = edges[q];
  for (int q = t; q < cc * n_bins * 4; q += CLS_NT) hist[q] = 0;
  for (int q = t; q < cc; q += CLS_NT) nanc[q] = 0;
  __syncthreads();

  const int M = N * C;
  for (int e = blockIdx.x * CLS_NT + t; e < M; e += gridDim.x * CLS_NT) {
    const int cg = e % C, cl = cg - c0;
    if ((unsigned)cl >= (unsigned)cc) continue;
    float x = logits[e];
    if (scale) x = __fadd_rn(__fmul_rn(x, scale[cg]), bias[cg]);
    if (x != x) {
      atomicAdd(&nanc[cl], 1u);
      continue;
    }
    const bool pos = target[e] > 0.5f;
    const int lo = upper_bound_lds(sedge, T, x);
    float p, q, ex;
    sigmoid_parts(x, &p, &q, &ex);
    const float d = pos ? q : p;  // |p - y|
    u64* h = hist + (cl * n_bins + lo) * 4;  // lo <= n_bins - 1
    atomicAdd(h + 0, (u64)1);
    if (pos) atomicAdd(h + 1, (u64)1);
    atomicAdd(h + 2, (u64)__float2ll_rn(p * 1073741824.f));
    atomicAdd(h + 3, (u64)__float2ll_rn(d * d * 1073741824.f));
  }
  __syncthreads();
  const int cells = n_bins * 4;
  for (int q = t; q < cc * cells; q += CLS_NT) {
    const u64 v = hist[q];
    if (v) atomicAdd(out + (long)c0 * cells + q, v);
  }
  for (int q = t; q < cells; q += CLS_NT) {  // micro: the block's classes, in class order
    u64 v = 0;
    for (int j = 0; j < cc; ++j) v += hist[j * cells + q];
    if (v) atomicAdd(out + (long)C * cells + q, v);
  }
  u64* out_nan = out + (long)(C + 1) * cells;
  for (int q = t; q < cc; q += CLS_NT)
    if (nanc[q]) atomicAdd(out_nan + c0 + q, (u64)nanc[q]);
  if (t == 0) {
    u64 v = 0;
    for (int j = 0; j < cc; ++j) v += nanc[j];
    if (v) atomicAdd(out_nan + C, v);
  }
}

}  // namespace mmdx

using namespace mmdx;

extern "C" size_t mmdx_calib_fit_workspace_size(long N, int C) {
  if (N <= 0 || C <= 0 || C > CLS_MAX_C || N > (long)INT32_MAX / C) return 0;
  return CLS_WS_HEAD + (size_t)C * CAL_STATE * sizeof(double) +
         (size_t)cls_grid(N * C, C) * CAL_NSUM * C * sizeof(double);
}

extern "C" int mmdx_calib_fit_step(const float* logits, const float* target, long N, int C,
                                   const double* counts, int smooth, int mode, int pass, int last,
                                   long min_count, double tol, float* scale, float* bias,
                                   int* status, double* info, void* workspace, size_t ws_bytes,
                                   void* stream) {
  MMDX_CHECK_ARG(logits && target && counts, "calib_fit_step: null pointer");
  MMDX_CHECK_ARG(N > 0 && C > 0, "calib_fit_step: empty (N = %ld, C = %d)", N, C);
  MMDX_CHECK_ARG(C <= CLS_MAX_C, "calib_fit_step: C = %d > %d", C, CLS_MAX_C);
  MMDX_CHECK_ARG(N <= (long)INT32_MAX / C, "calib_fit_step: N * C exceeds 2^31 - 1 (N = %ld)", N);
  MMDX_CHECK_ARG(mode == MMDX_CALIB_TEMPERATURE || mode == MMDX_CALIB_PLATT,
                 "calib_fit_step: mode %d", mode);
  MMDX_CHECK_ARG(pass >= 0, "calib_fit_step: pass %d", pass);
  MMDX_CHECK_ARG(min_count >= 0 && tol > 0.0 && tol < INFINITY,
                 "calib_fit_step: min_count = %ld, tol = %g", min_count, tol);
  MMDX_CHECK_ARG(!last || (scale && bias && status && info),
                 "calib_fit_step: the final pass needs scale, bias, status and info");
  const size_t need = mmdx_calib_fit_workspace_size(N, C);
  MMDX_CHECK_ARG(workspace && ws_bytes >= need && ((uintptr_t)workspace & 15) == 0,
                 "calib_fit_step: workspace null, unaligned or smaller than %zu bytes", need);
  MMDX_CHECK_ARG(((uintptr_t)counts & 7) == 0 && (!info || ((uintptr_t)info & 7) == 0),
                 "calib_fit_step: counts / info not 8-byte aligned");
  const long n = N * C;
  const size_t fb = (size_t)n * 4, cb = (size_t)C * 4;
  const void* outs[5] = {scale, bias, status, info, workspace};
  const size_t outs_n[5] = {cb, cb, cb, (size_t)C * 32, need};
  const void* ins[3] = {logits, target, counts};
  const size_t ins_n[3] = {fb, fb, (size_t)C * 16};
  const int clash = ranges_clash(outs, outs_n, 5, ins, ins_n, 3);
  MMDX_CHECK_ARG(clash != CLASH_INPUT, "calib_fit_step: an output overlaps an input");
  MMDX_CHECK_ARG(clash != CLASH_OUTPUT, "calib_fit_step: two outputs overlap");
  hipStream_t st = (hipStream_t)stream;
  const int grid = cls_grid(n, C);
  unsigned* counter = (unsigned*)workspace;
  double* state = (double*)((char*)workspace + CLS_WS_HEAD);
  u64* part = (u64*)(state + (size_t)C * CAL_STATE);
  if (pass == 0 && grid > 1) {  // later passes find the counter reset by the last block
    const hipError_t e = hipMemsetAsync(workspace, 0, CLS_WS_HEAD, st);
    MMDX_CHECK_ARG(e == hipSuccess, "calib_fit_step: hipMemsetAsync: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(calib_fit_kernel, dim3(grid), dim3(CLS_NT), 0, st, logits, target, n, C,
                     counts, smooth != 0, mode == MMDX_CALIB_TEMPERATURE, pass == 0, last != 0,
                     (double)min_count, tol, scale, bias, status, info, counter, state, part);
  MMDX_LAUNCH_CHECK();
  return 0;
}

extern "C" int mmdx_reliability_bins(const float* logits, const float* target, int N, int C,
                                     const float* scale, const float* bias, const float* edges,
                                     int n_bins, int64_t* out, void* stream) {
  MMDX_CHECK_ARG(logits && target && out, "reliability_bins: null pointer");
  MMDX_CHECK_ARG(N > 0 && C > 0, "reliability_bins: empty (N = %d, C = %d)", N, C);
  MMDX_CHECK_ARG(C <= CLS_MAX_C, "reliability_bins: C = %d > %d", C, CLS_MAX_C);
  MMDX_CHECK_ARG((long)N * C <= REL_MAX_ITEMS,
                 "reliability_bins: N * C = %ld exceeds the limit 2^24", (long)N * C);
  MMDX_CHECK_ARG(n_bins >= 1 && n_bins <= REL_MAX_BINS,
                 "reliability_bins: n_bins = %d outside [1, %d]", n_bins, REL_MAX_BINS);
  MMDX_CHECK_ARG(edges || n_bins == 1, "reliability_bins: null edges");
  MMDX_CHECK_ARG((scale == nullptr) == (bias == nullptr),
                 "reliability_bins: scale and bias come together");
  hipStream_t st = (hipStream_t)stream;
  const size_t nb = ((size_t)(C + 1) * n_bins * 4 + (C + 1)) * sizeof(int64_t);
  const hipError_t e = hipMemsetAsync(out, 0, nb, st);
  MMDX_CHECK_ARG(e == hipSuccess, "reliability_bins: hipMemsetAsync: %s", hipGetErrorString(e));
  const int CC = std::min(C, REL_CELLS / n_bins);  // >= 24 classes per block
  const int M = N * C;
  const int gx = std::max(1, std::min((M + 4095) / 4096, 256));
  hipLaunchKernelGGL(reliability_bins_kernel, dim3(gx, (C + CC - 1) / CC), dim3(CLS_NT), 0, st,
                     logits, target, N, C, scale, bias, edges, n_bins, CC, (u64*)out);
  MMDX_LAUNCH_CHECK();
  return 0;
}
