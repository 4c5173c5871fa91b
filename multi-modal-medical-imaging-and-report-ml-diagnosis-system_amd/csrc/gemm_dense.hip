// Dense GEMM C entry points (nn.Linear forward / dX / dW); the kernels are instantiated in
// gemm_dense_{bf16,bf16f,f16,f16f,f32}.hip (gemm_dense.h).
#include "gemm_dense.h"

using namespace mmdx;

// mmdx_gemm_bias_grad's choice of the fused weight + bias gradient (gemm_wgrad_bias_typed);
// shared with mmdx_gemm_describe.
static bool wgrad_bias_fused(int dtype, const SplitPlan& p, int M, int N, int K, long lda,
                             unsigned a_low4, long ldb, unsigned b_low4) {
  const long abytes = (long)K * lda * 2, bbytes = (long)K * ldb * 2;
  return wgrad_bias_fused_on() && dtype != F32 && p.splits > 1 && p.bm == 128 && M % 8 == 0 &&
         N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && (a_low4 & 15) == 0 &&
         (b_low4 & 15) == 0 && abytes < (1L << 31) && bbytes < (1L << 31);
}

extern "C" size_t mmdx_gemm_bias_grad_workspace_size(int dtype, int M, int N, int K) {
  const SplitPlan p = plan_dense(dtype, M, N, K);
  const size_t fused = p.splits > 1 ? (size_t)p.splits * ((size_t)M * N + M) * sizeof(float) : 0;
  const size_t plain = std::max(mmdx_gemm_workspace_size(dtype, M, N, K),
                                mmdx_bias_grad_workspace_size(K, M));
  return std::max(fused, plain);
}

extern "C" int mmdx_gemm_bias_grad(int dtype, int M, int N, int K, const void* A, long lda,
                                   const void* B, long ldb, void* C, long ldc, int c_dtype,
                                   float* db, void* ws, size_t ws_bytes, void* stream) {
  MMDX_CHECK_ARG(lda >= M && ldb >= N && ldc >= N && db, "gemm bias grad: bad arguments");
  MMDX_CHECK_ARG(ws && ws_bytes >= mmdx_gemm_bias_grad_workspace_size(dtype, M, N, K),
                 "gemm bias grad: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const SplitPlan p = plan_dense(dtype, M, N, K);
  const bool fused = wgrad_bias_fused(dtype, p, M, N, K, lda, (unsigned)((uintptr_t)A & 15), ldb,
                                      (unsigned)((uintptr_t)B & 15));
  if (fused) {
    if (dtype == F16) {
      if (c_dtype == F32)
        return gemm_wgrad_bias_f16f(p, M, N, K, A, lda, B, ldb, C, ldc, db, ws, st);
      return gemm_wgrad_bias_f16(p, M, N, K, A, lda, B, ldb, C, ldc, db, ws, st);
    }
    if (c_dtype == F32)
      return gemm_wgrad_bias_bf16f(p, M, N, K, A, lda, B, ldb, C, ldc, db, ws, st);
    return gemm_wgrad_bias_bf16(p, M, N, K, A, lda, B, ldb, C, ldc, db, ws, st);
  }
  // the GEMM, then the column sums of dY = A^T ([K][lda], M columns)
  MMDX_CHECK_ARG(lda == M, "gemm bias grad: unfused path needs lda == M");
  int rc = mmdx_gemm(dtype, M, N, K, A, lda, 0, B, ldb, 0, C, ldc, c_dtype, nullptr, nullptr,
                     ACT_NONE, 1.f, 0.f, nullptr, ws, ws_bytes, stream);
  if (rc) return rc;
  return mmdx_bias_grad(dtype, A, K, M, db, 0.f, ws, ws_bytes, stream);
}

extern "C" size_t mmdx_gemm_workspace_size(int dtype, int M, int N, int K) {
  const SplitPlan p = plan_dense(dtype, M, N, K);
  return p.splits > 1 ? (size_t)p.splits * M * N * sizeof(float) : 0;
}

static int gemm_entry(int dtype, int M, int N, int K, const void* A, long lda, int a_kmajor,
                         const void* B, long ldb, int b_kmajor, void* C, long ldc, int c_dtype,
                         const float* bias, const float* addend, int act, float alpha,
                         float beta, void* preact, void* workspace, size_t ws_bytes,
                         void* stream, const void* res) {
  MMDX_CHECK_ARG(M > 0 && N > 0 && K > 0, "mmdx_gemm: empty problem M=%d N=%d K=%d", M, N, K);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == F32) {
    MMDX_CHECK_ARG(c_dtype == F32, "mmdx_gemm: fp32 compute needs fp32 output");
    return gemm_typed_f32(M, N, K, A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, bias,
                                    addend, act, alpha, beta, preact, workspace, ws_bytes, st, res);
  }
  if (dtype == F16) {
    if (c_dtype == F32)
      return gemm_typed_f16f(M, N, K, A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, bias,
                                    addend, act, alpha, beta, preact, workspace, ws_bytes, st, res);
    MMDX_CHECK_ARG(c_dtype == F16, "mmdx_gemm: fp16 compute writes fp16 or fp32");
    return gemm_typed_f16(M, N, K, A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, bias,
                                addend, act, alpha, beta, preact, workspace, ws_bytes, st, res);
  }
  MMDX_CHECK_ARG(dtype == BF16, "mmdx_gemm: bad dtype %d", dtype);
  MMDX_CHECK_ARG(c_dtype == F32 || c_dtype == BF16, "mmdx_gemm: bf16 compute writes bf16/fp32");
  if (c_dtype == F32)
    return gemm_typed_bf16f(M, N, K, A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, bias,
                                   addend, act, alpha, beta, preact, workspace, ws_bytes, st, res);
  return gemm_typed_bf16(M, N, K, A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, bias, addend, act,
                                alpha, beta, preact, workspace, ws_bytes, st, res);
}

extern "C" int mmdx_gemm(int dtype, int M, int N, int K, const void* A, long lda, int a_kmajor,
                         const void* B, long ldb, int b_kmajor, void* C, long ldc, int c_dtype,
                         const float* bias, const float* addend, int act, float alpha,
                         float beta, void* preact, void* workspace, size_t ws_bytes,
                         void* stream) {
  return gemm_entry(dtype, M, N, K, A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, c_dtype, bias,
                    addend, act, alpha, beta, preact, workspace, ws_bytes, stream, nullptr);
}

extern "C" int mmdx_gemm_res(int dtype, int M, int N, int K, const void* A, long lda,
                             int a_kmajor, const void* B, long ldb, int b_kmajor, void* C,
                             long ldc, int c_dtype, const float* bias, const float* addend,
                             int act, float alpha, float beta, void* preact,
                             const void* residual, void* workspace, size_t ws_bytes,
                             void* stream) {
  MMDX_CHECK_ARG(residual != C, "mmdx_gemm_res: the residual must not alias C");
  return gemm_entry(dtype, M, N, K, A, lda, a_kmajor, B, ldb, b_kmajor, C, ldc, c_dtype, bias,
                    addend, act, alpha, beta, preact, workspace, ws_bytes, stream, residual);
}

// Host only: which kernel the dense dispatcher launches for this problem (plan_dense +
// dense_path, the functions the launches themselves call).
extern "C" int mmdx_gemm_describe(int dtype, int M, int N, int K, long lda, int a_kmajor,
                                  int a_addr_low4, long ldb, int b_kmajor, int b_addr_low4,
                                  int bias_sum, char* out, size_t n) {
  MMDX_CHECK_ARG(out && n > 0, "mmdx_gemm_describe: no output buffer");
  out[0] = 0;
  MMDX_CHECK_ARG(dtype == F32 || dtype == BF16 || dtype == F16,
                 "mmdx_gemm_describe: bad dtype %d", dtype);
  MMDX_CHECK_ARG(M > 0 && N > 0 && K > 0, "mmdx_gemm_describe: empty problem M=%d N=%d K=%d", M,
                 N, K);
  const SplitPlan p = plan_dense(dtype, M, N, K);
  const char* pre = "";
  bool bsum = false;
  if (bias_sum) {  // mmdx_gemm_bias_grad: both operands R-major
    MMDX_CHECK_ARG(!a_kmajor && !b_kmajor,
                   "mmdx_gemm_describe: the bias sum needs R-major operands");
    bsum = wgrad_bias_fused(dtype, p, M, N, K, lda, (unsigned)a_addr_low4, ldb,
                            (unsigned)b_addr_low4);
    pre = bsum ? "wb-fused/" : "wb-unfused/";
  }
  const DensePath d = dense_path(dtype == F32 ? 4 : 2, p.bm, p.bn, M, N, K, lda, a_kmajor != 0,
                                 (unsigned)a_addr_low4, ldb, b_kmajor != 0, (unsigned)b_addr_low4,
                                 bsum, p.splits, p.kper);
  static const char* const fam[] = {"kload", "dma4", "dma8"};
  const int w = snprintf(out, n, "%s%s/%dx%d/ns%d/s%d/k%d", pre, fam[d.family], d.bm, d.bn, d.ns,
                         p.splits, p.kper);
  MMDX_CHECK_ARG(w >= 0 && (size_t)w < n, "mmdx_gemm_describe: buffer of %zu bytes too small", n);
  return 0;
}
