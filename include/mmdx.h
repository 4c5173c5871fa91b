/*
 * mmdx — MI355X-native (gfx950) kernels for the multimodal diagnosis hot path of
 * PravCoder/Multi-Modal-Medical-Imaging-and-Report-ML-Diagnosis-System.
 *
 * C ABI of libmmdx_hip.so.  Plain pointers and sizes only; every buffer is owned by the
 * caller (PyTorch's caching allocator in the shipped host code); the library never
 * allocates or frees caller memory.  Where a call needs scratch, the caller queries
 * `*_workspace_size` and passes a buffer of at least that many bytes.
 *
 * The reference has no native code and no FFI: its hot path is pure PyTorch-CPU
 * (backend/ml/pipelines/training_pipeline.py, "TP" below).  Each entry point names the
 * reference operator it replaces; the Python host layer (mmdx.training_pipeline) keeps
 * the reference's class/function surface and binds these symbols with ctypes.
 *
 * Conventions
 *   dtype:      0 = fp32 (parity path, exact-f32 MFMA), 1 = bf16 (throughput path),
 *               2 = fp16 (C5's "fp16 MFMA": dense GEMM, attention, LayerNorm, text / ViT
 *               kernels; the ResNet and BiLSTM entry points reject it)
 *   images:     NHWC, channels innermost; conv weights packed [Cout][R][S][Cin] ("KRSC")
 *               for fwd and [Cin][R][S][Cout] ("CRSK") for dgrad; fp32 master weights
 *               and gradients stay in PyTorch's [Cout][Cin][R][S] ("KCRS") layout.
 *   matrices:   row-major; "kmajor" = the contraction index is the contiguous one.
 *   stream:     a hipStream_t passed as void*; every call is stream-ordered, reentrant,
 *               graph-capturable (no allocation, no sync, no host readback).
 *   return:     0 on success, negative errno / -hipError_t on failure;
 *               mmdx_last_error() gives a thread-local message.
 */
#ifndef MMDX_H_
#define MMDX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MMDX_F32 = 0, MMDX_BF16 = 1, MMDX_F16 = 2 };
enum { MMDX_ACT_NONE = 0, MMDX_ACT_RELU = 1, MMDX_ACT_GELU = 2, MMDX_ACT_GELU_BWD = 3 };

int mmdx_version(void);
const char* mmdx_last_error(void);
/* Re-read the MMDX_* launch-heuristic environment knobs (tile / split choices; read once per
 * process otherwise).  For tests and A/B runs that switch a knob between launches; not to be
 * called while another thread issues launches. */
int mmdx_reload_config(void);
/* A non-blocking HIP stream on `cus` of the device's compute units (evenly spread; 0 = all)
 * with the given priority (cus < all: hipExtStreamCreateWithCUMask, default priority).  Used
 * for the trunk's weight-gradient stream (MMDX_WGRAD_CUS).  *out: the hipStream_t. */
int mmdx_stream_create(int priority, int cus, void** out);
int mmdx_stream_destroy(void* stream);

/* ---------------------------------------------------------------- GEMM (nn.Linear)
 * C[M,N] = act(alpha * sum_k A(m,k) B(n,k) + bias[n] + addend[m,n]) + beta * C
 * (addend: optional fp32, leading dim ldc — lets a concat-input Linear run as two GEMMs)
 * A(m,k) = A[m*lda + k] if a_kmajor else A[k*lda + m];  same for B with (n,k).
 * c_dtype may differ from dtype (bf16 compute -> fp32 weight-gradient output).
 * preact (optional, c_dtype, ld = ldc) receives alpha*acc + bias before the activation.
 * act = MMDX_ACT_GELU_BWD: preact is an INPUT (the forward's pre-activation, read, not
 * written) and C = alpha*acc * gelu'(preact) (+ beta*C): the GELU backward fused into the
 * GEMM that produces the post-activation gradient (BERT / ViT FFN, fusion MLP).
 * Replaces: nn.Linear fwd/bwd in ImageEncoderCNN.proj/classifier (TP:189,194),
 * TextEncoderTransformer.proj/classifier (TP:365,367), BERT dense layers (TP:360 ->
 * transformers BertModel), fusion_mlp[0] + GELU (TP:534-536), disease_head (TP:542). */
size_t mmdx_gemm_workspace_size(int dtype, int M, int N, int K);
/* Host only (no GPU needed): the kernel mmdx_gemm / mmdx_gemm_res launch for this problem, from
 * the functions the launch itself calls, as "<family>/<bm>x<bn>/ns<stages>/s<splits>/k<kper>":
 * family kload (register-staged loaders) | dma4 | dma8 (LDS-DMA kernels of 4 / 8 waves), kper
 * the K extent of one split.  *_addr_low4: the low four bits of the operand's address.
 * bias_sum != 0 describes mmdx_gemm_bias_grad instead (both operands R-major): the string gains
 * the prefix "wb-fused/" (bias sums inside the split-K GEMM) or "wb-unfused/" (mmdx_gemm, then
 * mmdx_bias_grad).  Writes a NUL-terminated string of fewer than n bytes to out. */
int mmdx_gemm_describe(int dtype, int M, int N, int K, long lda, int a_kmajor, int a_addr_low4,
                       long ldb, int b_kmajor, int b_addr_low4, int bias_sum, char* out,
                       size_t n);
/* mmdx_gemm plus a residual [M][ldc] of C's dtype added last (after the activation and
 * beta*C): C = act(alpha*A B^T + bias) + beta*C + residual; residual must not alias C.
 * Replaces: the residual adds of torchvision's EncoderBlock (x + mlp(ln_2(x)), vit_b_16). */
int mmdx_gemm_res(int dtype, int M, int N, int K, const void* A, long lda, int a_kmajor,
                  const void* B, long ldb, int b_kmajor, void* C, long ldc, int c_dtype,
                  const float* bias, const float* addend, int act, float alpha, float beta,
                  void* preact, const void* residual, void* workspace, size_t ws_bytes,
                  void* stream);
/* Weight gradient of a Linear layer with its bias gradient: C = A B for A = dY^T and B = X
 * both R-major (element (m, k) of A at A[k*lda + m]: dY [K tokens][lda]), alpha 1, beta 0,
 * and db[m] = sum_k A(m, k) (the column sums of dY) — for 16-bit split-K problems computed by
 * the GEMM blocks of column tile 0 from their own A fragments (one extra MFMA per fragment
 * against a ones operand) and reduced over the splits, so dY is not read again; otherwise
 * (fp32, unsplit grids, unaligned operands, MMDX_WGRAD_BIAS_FUSED=0) mmdx_gemm followed by
 * mmdx_bias_grad (needs lda == M).
 * Replaces: the weight and bias gradients of nn.Linear in the BERT / ViT layers (TP:360). */
size_t mmdx_gemm_bias_grad_workspace_size(int dtype, int M, int N, int K);
int mmdx_gemm_bias_grad(int dtype, int M, int N, int K, const void* A, long lda, const void* B,
                        long ldb, void* C, long ldc, int c_dtype, float* db, void* workspace,
                        size_t ws_bytes, void* stream);
int mmdx_gemm(int dtype, int M, int N, int K,
              const void* A, long lda, int a_kmajor,
              const void* B, long ldb, int b_kmajor,
              void* C, long ldc, int c_dtype,
              const float* bias, const float* addend, int act, float alpha, float beta,
              void* preact, void* workspace, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- convolution
 * Replaces: every nn.Conv2d of torchvision resnet18/50 reached through
 * ImageEncoderCNN._backbone_forward_grad/_nograd (TP:279-289, TP:183). */
typedef struct {
  int N, H, W, C;      /* input NHWC */
  int K;               /* output channels */
  int R, S;            /* filter height, width */
  int stride_h, stride_w, pad_h, pad_w;
  int P, Q;            /* output height, width */
} mmdx_conv_desc;

/* fp32 KCRS master -> packed compute-dtype copies (either output may be NULL).
 * Channel padding: desc->C may exceed the master's Cin (c_master); pad lanes are 0. */
int mmdx_conv_pack_weight(int dtype, const mmdx_conv_desc* d, int c_master,
                          const float* w_kcrs, void* w_krsc, void* w_crsk, void* stream);
/* Every conv weight of a network in one launch.  items: DEVICE array of n_items, sorted by
 * first_block; item i owns blocks [first_block_i, first_block_{i+1}) (the last runs to
 * total_blocks), mmdx_conv_pack_blocks(K, C, R*S) of them.  Same packing as
 * mmdx_conv_pack_weight for unpadded weights: c_master must equal C (channel-padded weights
 * use mmdx_conv_pack_weight).  Items with RS = 1 and no crsk are plain [K][C] casts: the
 * transformer encoder stacks cast every layer's weights with one such launch (bf16 / fp16). */
typedef struct {
  const float* w;      /* fp32 KCRS master */
  void* krsc;          /* packed [K][R][S][C] or NULL */
  void* crsk;          /* packed [C][R][S][K] or NULL */
  int K, C, c_master, RS;
  long first_block;
} mmdx_pack_item;
long mmdx_conv_pack_blocks(int K, int C, int RS);
int mmdx_conv_pack_multi(int dtype, const mmdx_pack_item* items, int n_items, long total_blocks,
                         void* stream);
/* stat_part (optional, fp32 pairs [K][mmdx_conv_fwd_stat_blocks(d)], channel-major): per-channel
 * (mean, M2) of each mmdx_conv_fwd_stat_rows(d)-row block of the output (128 rows; the direct
 * pixel-pair stem kernel: one block of 2 output rows), computed from the fp32 accumulators in
 * the GEMM epilogue — the BatchNorm batch statistics without a separate pass over y
 * (replaces the BatchNorm2d reduction after backbone convs, TP:183 / torchvision). */
int mmdx_conv_fwd_stat_blocks(const mmdx_conv_desc* d);
int mmdx_conv_fwd_stat_rows(const mmdx_conv_desc* d);
int mmdx_conv_fwd(int dtype, const mmdx_conv_desc* d, const void* x, const void* w_krsc,
                  void* y, float* stat_part, void* stream);
/* The same with the statistics slab size the caller allocated stat_part for (stat_rows =
 * mmdx_conv_fwd_stat_rows(d) when the buffer was sized; a plan built once keeps its layout
 * whatever MMDX_STEM_DIRECT says later; a size the kernels cannot write is an error). */
int mmdx_conv_fwd_rows(int dtype, const mmdx_conv_desc* d, const void* x, const void* w_krsc,
                       void* y, float* stat_part, int stat_rows, void* stream);
/* Eval-mode conv + BatchNorm2d (running statistics) (+residual) (+ReLU) in one launch:
 * y = act(conv(x, w) * s + t + residual), s = gamma / sqrt(running_var + eps),
 * t = beta - running_mean * s, applied in the conv epilogue on the fp32 accumulators.
 * Replaces conv + bn_apply for the backbone in eval mode (TP:206 freeze_backbone, TP:1000
 * encoders in eval, IP:170 inference).  residual may be NULL. */
int mmdx_conv_fwd_bn_eval(int dtype, const mmdx_conv_desc* d, const void* x,
                          const void* w_krsc, void* y, const float* gamma, const float* beta,
                          const float* running_mean, const float* running_var, float eps,
                          const void* residual, int relu, void* stream);
/* dx = dgrad + beta * dx  (beta = 1 sums the residual-path gradient in the epilogue) */
int mmdx_conv_dgrad(int dtype, const mmdx_conv_desc* d, const void* dy,
                    const void* w_crsk, void* dx, float beta, void* stream);
/* dx = dgrad + beta * dx and, in the same epilogue, the backward statistics of the
 * BatchNorm whose output gradient the final dx is (its input bn_y, affine, saved mean/rstd):
 * stat_part [C][mmdx_conv_dgrad_stat_blocks()] (sum g, sum g*xhat) per 128-row tile, for
 * mmdx_bn_bwd.  The ReLU mask is bn_out > 0 for a residual unit (bn_out = its output
 * relu(bn(y) + res)), else recomputed from bn_y with the forward's scale/shift (bn_out NULL).
 * beta != 0 (accumulating a residual branch's gradient) needs a stride-1 conv.
 * stat_blocks == 0: the fusion does not apply to this conv. */
int mmdx_conv_dgrad_stat_blocks(int dtype, const mmdx_conv_desc* d);
int mmdx_conv_dgrad_bnstat(int dtype, const mmdx_conv_desc* d, const void* dy,
                           const void* w_crsk, void* dx, float beta, const void* bn_y,
                           const void* bn_out, const float* gamma, const float* bn_beta,
                           const float* save_mean, const float* save_rstd, int relu,
                           float* stat_part, void* stream);
/* stride-1 dgrad whose epilogue adds a masked tensor: dx = dgrad(dy) + (bit ? acc_src : 0),
 * the bit from a 1-bit ReLU mask written by mmdx_bn_fwd_ex ([rows][C / (16 / elem)] bytes).
 * An identity block's conv1 dgrad adds the gradient that reached the block output through
 * the residual unit's ReLU (its dout, masked) — mmdx_bn_bwd then writes no d_residual.
 * Equals mmdx_conv_dgrad with beta 1 onto that masked gradient, bit for bit. */
int mmdx_conv_dgrad_accmask(int dtype, const mmdx_conv_desc* d, const void* dy,
                            const void* w_crsk, void* dx, const void* acc_src,
                            const uint8_t* acc_mask, void* stream);
size_t mmdx_conv_wgrad_workspace_size(int dtype, const mmdx_conv_desc* d);
/* dw_kcrs (fp32, master layout, Cin = c_master) = dw_kcrs*beta + grad */
int mmdx_conv_wgrad(int dtype, const mmdx_conv_desc* d, int c_master, const void* x,
                    const void* dy, float* dw_kcrs, float beta, void* workspace,
                    size_t ws_bytes, void* stream);
/* Host only (no GPU needed): the kernel path a conv launch takes for this descriptor under the
 * MMDX_* knobs in force, from the functions the launch itself calls.  pass 0: mmdx_conv_fwd
 * (mmdx_conv_fwd_bn_eval takes the same path, except that it never runs the direct stem
 * kernel); 1: mmdx_conv_dgrad with this beta (it decides which phases of a strided conv are
 * launched); 2: mmdx_conv_wgrad.  dtype: MMDX_F32 | MMDX_BF16.
 *   fwd, stride-1 dgrad: "<operand>/<loader>/<tile>[/ns<stages>]", operand point | fast |
 *     generic, loader kload | dma | dma-lanetap, tile 128x64 | 128x128 | 128x128-8w | 256x64;
 *     the stage count where the grid rule picks it (the 4-wave LDS-DMA tiles).
 *   strided dgrad: "phases-merged/dma/<tile>" | "phases-each/kload/<tile>".
 *   wgrad: "<bm>x<bn>/<operand>[/ns<stages>]/<reduction>/s<splits>/k<kper>", operand DmaRq |
 *     DmaR | DmaR-point | RLoad, reduction reduce | reduce-z, kper the pixels of one split.
 *   the direct pixel-pair stem kernels: "stem-direct" (fwd), "stem-direct/<reduction>/s../k..".
 * Writes a NUL-terminated string of fewer than n bytes to out. */
int mmdx_conv_describe(int dtype, int pass, const mmdx_conv_desc* d, float beta, char* out,
                       size_t n);

/* ResNet stem (backbone.0, TP:183: 7x7 / stride 2 / pad 3 over the 3-channel image) as an
 * ordinary conv over PIXEL PAIRS (bf16 path): the NCHW fp32 batch of
 * image_transfom_into_tensor (TP:112-119) is written once, zero-bordered, as
 * [N][H+2p][(W+2p)/2][8] bf16 (two adjacent padded pixels x 4 channels per "pixel"); the
 * stem is then a stride (2,1), unpadded R x ceil(S/2) conv with 8 channels (K = 224 instead of
 * 392 for the channel-padded image, no border taps) run by mmdx_conv_fwd / mmdx_conv_wgrad
 * with the descriptor mmdx_stem_pair_desc returns.  Needs stride 2, C <= 4, even W + 2p.
 *   pack:  w_kcrs fp32 [K][C][R][S] -> w_packed [K][R][ceil(S/2)][8] bf16 (the pair conv's KRSC)
 *   grad:  dw_pair fp32 [K][8][R][ceil(S/2)] (mmdx_conv_wgrad of the pair conv, c_master 8)
 *          -> dw_kcrs (master layout) = beta * dw_kcrs + grad */
int mmdx_stem_pair_desc(int N, int C, int H, int W, int K, int R, int S, int stride, int pad,
                        mmdx_conv_desc* out);
int mmdx_stem_pair_input(const float* x_nchw, int N, int C, int H, int W, int pad, void* out,
                         void* stream);
int mmdx_stem_pair_pack_weight(const float* w_kcrs, int K, int C, int R, int S, void* w_packed,
                               void* stream);
int mmdx_stem_pair_grad(const float* dw_pair, int K, int C, int R, int S, float* dw_kcrs,
                        float beta, void* stream);

/* ---------------------------------------------------------------- batch norm (+res)(+ReLU)
 * x, y, residual: [rows, C] (NHWC flattened).  Train mode computes batch statistics
 * (biased var for normalisation, unbiased for running_var, momentum update as
 * nn.BatchNorm2d(eps, momentum)); eval mode uses running stats.
 * save_mean/save_rstd: [C] fp32, consumed by the backward.
 * Replaces: BatchNorm2d + ReLU (+ Bottleneck residual add) inside the resnet trunk
 * (train mode: unfreeze_backbone TP:223; eval: freeze_backbone TP:206, IP:170). */
/* Enough for either dtype (fp32 needs C % 4 == 0, bf16 C % 8 == 0; sized for the widths C is
 * a multiple of); 0 when C fits neither, which no entry point accepts as a workspace. */
size_t mmdx_bn_workspace_size(long rows, int C);
/* stat_part: optional precomputed per-block (mean, M2) pairs [C][stat_blocks] over
 * consecutive stat_rows-row blocks (e.g. from mmdx_conv_fwd's epilogue); NULL = reduce x.
 * The blocks must cover the rows exactly, the last one holding 1..stat_rows of them:
 * (stat_blocks - 1) * stat_rows < rows <= stat_blocks * stat_rows, else an error. */
int mmdx_bn_fwd(int dtype, int train, const void* x, long rows, int C,
                const float* stat_part, int stat_blocks, long stat_rows,
                const float* gamma, const float* beta, float* running_mean,
                float* running_var, float momentum, float eps,
                float* save_mean, float* save_rstd,
                const void* residual, int relu, void* y,
                void* workspace, size_t ws_bytes, void* stream);
/* y == NULL (train): statistics only — save_mean/save_rstd and the running-stat update, no
 * apply pass (the consumer normalises on the fly, e.g. mmdx_maxpool_bn_fwd). */
/* mmdx_bn_fwd plus, when relu_mask != NULL (relu units): one byte per 16-B channel vector of
 * each row ([rows][C / (16 / sizeof(dtype))]), bit e set iff the stored y element e is > 0 —
 * the ReLU mask mmdx_bn_bwd_ex reads instead of y (1 bit per element instead of 16). */
int mmdx_bn_fwd_ex(int dtype, int train, const void* x, long rows, int C,
                   const float* stat_part, int stat_blocks, long stat_rows,
                   const float* gamma, const float* beta, float* running_mean,
                   float* running_var, float momentum, float eps,
                   float* save_mean, float* save_rstd,
                   const void* residual, int relu, void* y, uint8_t* relu_mask,
                   void* workspace, size_t ws_bytes, void* stream);
/* The two halves of the train forward above: the finalize of precomputed slabs (mean,
 * rstd, running stats, scale = gamma*rstd, shift = beta - mean*scale), and the apply pass
 * y = act(x*scale + shift (+ residual)) with the optional ReLU bit mask. */
int mmdx_bn_finalize(const float* stat_part, int stat_blocks, long stat_rows, long rows, int C,
                     const float* gamma, const float* beta, float* running_mean,
                     float* running_var, float momentum, float eps, float* save_mean,
                     float* save_rstd, float* scale, float* shift, void* stream);
int mmdx_bn_apply(int dtype, const void* x, const void* residual, long rows, int C,
                  const float* scale, const float* shift, int relu, void* y,
                  uint8_t* relu_mask, void* stream);
/* dy: grad w.r.t. y; y: forward output (ReLU mask source).  Writes dx, d_residual
 * (may be NULL), and dgamma/dbeta (fp32, accumulated with beta_acc). */
int mmdx_bn_bwd(int dtype, int train, const void* x, const void* y, const void* dy,
                long rows, int C, const float* gamma, const float* bn_beta,
                const float* save_mean, const float* save_rstd, int relu,
                const float* stat_part, int stat_blocks, void* dx,
                void* d_residual, float* dgamma, float* dbeta, float beta_acc,
                void* workspace, size_t ws_bytes, void* stream);
/* mmdx_bn_bwd with the ReLU mask taken from relu_mask (written by mmdx_bn_fwd_ex) when it is
 * not NULL — a residual unit's backward then reads 1 bit per element instead of its output;
 * results are identical to mmdx_bn_bwd with y. */
int mmdx_bn_bwd_ex(int dtype, int train, const void* x, const void* y, const void* dy,
                   long rows, int C, const float* gamma, const float* bn_beta,
                   const float* save_mean, const float* save_rstd, int relu,
                   const float* stat_part, int stat_blocks, void* dx,
                   void* d_residual, float* dgamma, float* dbeta, float beta_acc,
                   const uint8_t* relu_mask, void* workspace, size_t ws_bytes, void* stream);
/* BN backward (no ReLU, no residual: a downsample branch's BN) whose upstream gradient is
 * dy with a 1-bit ReLU mask applied on the fly (dy_mask from mmdx_bn_fwd_ex of the residual
 * unit whose identity path feeds it) — equals mmdx_bn_bwd on the materialised masked dy. */
int mmdx_bn_bwd_masked_dy(int dtype, int train, const void* x, const void* dy,
                          const uint8_t* dy_mask, long rows, int C, const float* gamma,
                          const float* bn_beta, const float* save_mean,
                          const float* save_rstd, void* dx, float* dgamma, float* dbeta,
                          float beta_acc, void* workspace, size_t ws_bytes, void* stream);
/* The two BatchNorm backwards at the end of a block with a downsample branch
 * (torchvision Bottleneck / BasicBlock: out = relu(bn3(conv3) + downsample(x)), TP:279-289) in
 * one reduce, one finalize and one apply pass.  Both read the same upstream gradient
 * g = dy with the block's 1-bit ReLU mask applied: side a (the residual unit's BN) as
 * mmdx_bn_bwd_ex(relu = 1, relu_mask = dy_mask, d_residual = NULL) does, side b (the
 * downsample BN) as mmdx_bn_bwd_masked_dy does.  dy and the mask are streamed twice instead of
 * four times; every output is bit-identical to the two separate calls.  Both sides are
 * [rows][C].  workspace: mmdx_bn_pair_workspace_size(rows, C) bytes. */
typedef struct {
  const void* x;           /* the BN's input (its conv's raw output) */
  const float* gamma;
  const float* bn_beta;
  const float* save_mean;
  const float* save_rstd;
  void* dx;
  float* dgamma;
  float* dbeta;
} mmdx_bn_side;
size_t mmdx_bn_pair_workspace_size(long rows, int C);
int mmdx_bn_bwd_pair(int dtype, int train, const void* dy, const uint8_t* dy_mask, long rows,
                     int C, const mmdx_bn_side* a, const mmdx_bn_side* b, float beta_acc,
                     void* workspace, size_t ws_bytes, void* stream);
/* MMDX_BN_BWD_PAIR (default 1): whether the ResNet trunk's backward plan issues
 * mmdx_bn_bwd_pair for its downsample blocks (0: the two separate calls, for A/B runs). */
int mmdx_bn_bwd_pair_enabled(void);
/* stat_part (optional, [C][stat_blocks] pairs (sum g, sum g*xhat)): the reduction already
 * made by mmdx_conv_dgrad_bnstat in the epilogue that produced dy — the BN backward then
 * skips its own pass over (dy, x).  ReLU units only (with y = the unit's output for a
 * residual unit, y == NULL otherwise). */
/* relu with y == NULL (a unit without residual): the ReLU mask is recomputed from x as
 * x*scale + shift > 0 with the forward's own scale/shift (gamma, bn_beta, save_mean,
 * save_rstd), so the post-activation tensor is not read. */

/* The stem's BN backward reading its upstream gradient straight from the 3x3 / stride-2
 * pool's output gradient dy_pooled [N][P][Q][C] and argmax (mmdx_maxpool_fwd /
 * mmdx_maxpool_bn_fwd): dL/d(pool input) is gathered on the fly (rounded to the compute dtype,
 * as mmdx_maxpool_bwd stores it), so the result equals mmdx_maxpool_bwd followed by
 * mmdx_bn_bwd (y == NULL, no residual) without materialising the [N][H][W][C] gradient.
 * x: the stem conv's raw output [N][H][W][C]. */
int mmdx_bn_bwd_pool(int dtype, int train, const void* x, const uint8_t* argmax,
                     const void* dy_pooled, int N, int H, int W, int C, int k, int s, int p,
                     int P, int Q, const float* gamma, const float* bn_beta,
                     const float* save_mean, const float* save_rstd, int relu, void* dx,
                     float* dgamma, float* dbeta, float beta_acc, void* workspace,
                     size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- launch plans
 * A plan is a host array of operations over caller-owned buffers, recorded once by the
 * host layer (the ResNet trunk forward or backward for one batch shape and parameter set)
 * and replayed with ONE call per step, so the per-step host cost is the launches alone.
 * Operand j of an op is o.p[j] itself when o.ext[j] < 0, else ext[o.ext[j]] + (intptr)o.p[j]
 * (per-call buffers: the image batch, the upstream gradient, the gradient arena).
 * Each op runs on streams[o.stream] (streams[0] = the caller's stream).  MMDX_OP_EVENT
 * records timing event events[o.i[0]] (skipped when events is NULL); MMDX_OP_SIGNAL records
 * the hipEvent_t o.p[0] on the op's stream and MMDX_OP_WAIT makes the op's stream wait on it
 * (cross-stream order inside a plan: e.g. weight gradients on a side stream).
 * Argument packing per op: see csrc/plan.cpp (each op forwards to the entry point of the
 * same name above/below with its i/l/f/p fields in signature order).
 * Replaces: the per-layer Python dispatch of ImageEncoderCNN's trunk (TP:279-289) and of
 * the BERT / ViT encoder layers (TP:360/470 AutoModel's BertLayer stack; vit_b_16). */
enum {
  MMDX_OP_EVENT = 1, MMDX_OP_NCHW2NHWC, MMDX_OP_CONV_PACK, MMDX_OP_CONV_FWD, MMDX_OP_BN_FWD,
  MMDX_OP_MAXPOOL_FWD, MMDX_OP_AVGPOOL_FWD, MMDX_OP_CAST, MMDX_OP_AVGPOOL_BWD,
  MMDX_OP_MAXPOOL_BWD, MMDX_OP_BN_BWD, MMDX_OP_CONV_WGRAD, MMDX_OP_CONV_DGRAD,
  MMDX_OP_SIGNAL, MMDX_OP_WAIT, MMDX_OP_CONV_DGRAD_BNSTAT, MMDX_OP_STEM_PAIR_INPUT,
  MMDX_OP_STEM_PAIR_PACK, MMDX_OP_STEM_PAIR_GRAD, MMDX_OP_CONV_PACK_MULTI,
  MMDX_OP_CONV_FWD_BNEVAL, MMDX_OP_MAXPOOL_BN_FWD, MMDX_OP_BN_BWD_POOL,
  MMDX_OP_CONV_DGRAD_ACCMASK, MMDX_OP_BN_BWD_MASKED_DY,
  /* transformer layer stacks (BERT / ViT encoders, one plan per stack and direction) */
  MMDX_OP_GEMM, MMDX_OP_ATTN_FWD, MMDX_OP_ATTN_BWD, MMDX_OP_LN_FWD, MMDX_OP_LN_BWD,
  MMDX_OP_GELU_BWD, MMDX_OP_BIAS_GRAD, MMDX_OP_ADD, MMDX_OP_DROPOUT_FWD, MMDX_OP_DROPOUT_BWD,
  MMDX_OP_AXPBY, MMDX_OP_ATTN_FWD_LSE, MMDX_OP_ATTN_BWD_LSE, MMDX_OP_LN_FWD_DROP,
  MMDX_OP_LN_BWD_DROP, MMDX_OP_GEMM_BIAS_GRAD,
  /* (42: the retired conv + fused BN finalize op, tools/lab/RETIRED.md) and the BN apply pass
   * (i: C, relu; l: rows; p: x, residual, scale, shift, y, relu_mask) */
  MMDX_OP_RETIRED_42, MMDX_OP_BN_APPLY,
  /* mmdx_bn_bwd_pair (i: train, C; l: rows, ws_bytes; f: beta_acc; p: dy, dy_mask, x_a, dx_a,
   * dgamma_a, dbeta_a, x_b, dx_b, dgamma_b, dbeta_b, ws, and a host table of 8 const float*:
   * gamma, bn_beta, save_mean, save_rstd of side a, then of side b) */
  MMDX_OP_BN_BWD_PAIR
};
typedef struct {
  int op, dtype, stream;
  int i[8];
  long l[4];
  float f[4];
  const void* p[12];
  int ext[12];
  mmdx_conv_desc d;
} mmdx_plan_op;
int mmdx_plan_run(const mmdx_plan_op* ops, int n_ops, void* const* ext, void* const* events,
                  void* const* streams, int n_streams);
size_t mmdx_plan_op_size(void); /* sizeof(mmdx_plan_op): binding layout check */

/* ---------------------------------------------------------------- pooling
 * Replaces: resnet maxpool 3x3/2 (backbone[3]) and AdaptiveAvgPool2d(1) (backbone[8])
 * followed by flatten(1) (TP:281/288). */
/* argmax: uint8 window index (r*k+s) of the first maximum, as PyTorch CPU max_pool2d */
int mmdx_maxpool_fwd(int dtype, const void* x, int N, int H, int W, int C, int k, int s,
                     int p, void* y, uint8_t* argmax, int P, int Q, void* stream);
/* The stem's BN(+ReLU) fused into its 3x3 / stride-2 pool (train forward): x is the RAW stem
 * conv output; every tap is normalised with the batch statistics mmdx_bn_fwd saved (called
 * with y == NULL: statistics, running stats and save_mean/save_rstd only, no apply pass), as
 * scale = gamma*rstd, shift = beta - mean*gamma*rstd, ReLU'd and rounded to the compute dtype
 * before the compare — y and argmax are bit-identical to mmdx_bn_fwd's apply followed by
 * mmdx_maxpool_fwd, without writing or re-reading the post-activation tensor.
 * Replaces: backbone[1..3] (BatchNorm2d, ReLU, MaxPool2d) of the trunk, TP:183/279-281. */
int mmdx_maxpool_bn_fwd(int dtype, const void* x, int N, int H, int W, int C, int k, int s,
                        int p, const float* gamma, const float* beta, const float* save_mean,
                        const float* save_rstd, int relu, void* y, uint8_t* argmax, int P, int Q,
                        void* stream);
int mmdx_maxpool_bwd(int dtype, const uint8_t* argmax, const void* dy, int N, int H, int W,
                     int C, int k, int s, int p, int P, int Q, void* dx, void* stream);
int mmdx_avgpool_fwd(int dtype, const void* x, int N, int HW, int C, void* y, void* stream);
int mmdx_avgpool_bwd(int dtype, const void* dy, int N, int HW, int C, void* dx,
                     void* stream);

/* ---------------------------------------------------------------- layout / casts
 * NCHW fp32 image batch (output of image_transfom_into_tensor, TP:112-119) ->
 * NHWC compute dtype with channels zero-padded to c_pad. */
int mmdx_nchw_to_nhwc(int dtype, const float* x, int N, int C, int H, int W, int c_pad,
                      void* y, void* stream);
int mmdx_cast(int dst_dtype, int src_dtype, const void* x, long n, void* y, void* stream);
/* out = a*x + b*y (fp32; y may be NULL) — bias folding (LSTM b_ih + b_hh), grad copies */
int mmdx_axpby(long n, float a, const float* x, float b, const float* y, float* out,
               void* stream);

/* ---------------------------------------------------------------- ViT-B/16 tower (C5)
 * torchvision vit_b_16 (build-defined backbone name):
 * patchify: x NCHW fp32 -> [N*(H/p)*(W/p)][C*p*p] rows in (c, ky, kx) order, so the
 *   Conv2d(C, D, p, stride p) patch embedding is one GEMM against its [D][C*p*p] weight;
 * vit_tokens: tokens[n][0] = class_token + pos[0], tokens[n][1+q] = emb[n][q] + pos[1+q];
 *   backward returns d emb (the class-token / pos gradients are column sums, bias_grad);
 * rows_copy: strided row copy (class-token rows in and out of the token matrix);
 * add: out = x + y in the compute dtype (residual gradient sums). */
int mmdx_patchify(int dtype, const float* x, int N, int C, int H, int W, int p, void* out,
                  void* stream);
int mmdx_vit_tokens_fwd(int dtype, const void* emb, const float* cls, const float* pos, int N,
                        int S, int D, void* tokens, void* stream);
int mmdx_vit_tokens_bwd(int dtype, const void* dtokens, int N, int S, int D, void* demb,
                        void* stream);
int mmdx_rows_copy(int dtype, const void* src, long src_ld, void* dst, long dst_ld, long rows,
                   int D, void* stream);
int mmdx_add(int dtype, long n, const void* x, const void* y, void* out, void* stream);

/* ---------------------------------------------------------------- image preprocessing
 * Batched GPU version of image_transfom_into_tensor (TP:112-119): torchvision
 * Resize(256, antialias=True) on a PIL image (= PIL ImagingResample, bilinear filter, two
 * fixed-point passes, horizontal first, 22-bit coefficients, uint8 clipped after each pass),
 * CenterCrop(224), ToTensor, gray->RGB repeat, Normalize(ImageNet).  Bit-exact with the CPU
 * transform.  pixels: the batch's decoded HWC uint8 images (JPEG decode stays on the host,
 * PIL, TP:146) packed back to back; descs/coef: per-image geometry and PIL coefficient
 * tables (host-computed, mmdx.preprocess); temp: >= sum of trows*out_w*c bytes;
 * out: [B][3][out_h][out_w] fp32. */
typedef struct {
  long src_off;         /* byte offset of the image's HWC pixels */
  long kh_off, kv_off;  /* int offsets into coef: per crop column / row {min, count, k[ksize]} */
  long temp_off;        /* byte offset of the image's [trows][out_w][c] intermediate */
  int w, h, c;          /* source width, height, channels (1 = L, 3 = RGB) */
  int left, top;        /* crop origin in the resized image */
  int need_h, need_v;   /* which PIL resample passes run */
  int ksize_h, ksize_v; /* coefficients per output column / row */
  int trow0, trows;     /* source rows the horizontal pass covers */
} mmdx_img_desc;
size_t mmdx_img_desc_size(void); /* sizeof(mmdx_img_desc): binding layout check */
int mmdx_image_preprocess(const uint8_t* pixels, const mmdx_img_desc* descs, int B,
                          const int* coef, int max_trows, int out_h, int out_w, uint8_t* temp,
                          float* out, void* stream);

/* ---------------------------------------------------------------- elementwise / norms
 * LayerNorm over the last dim D (fusion_mlp[3] TP:538, BERT LayerNorms);
 * optional residual added before the norm (BERT "Add & Norm"). */
int mmdx_layernorm_fwd(int dtype, const void* x, const void* residual, long rows, int D,
                       const float* gamma, const float* beta, float eps, void* y,
                       void* sum_out, float* save_mean, float* save_rstd, void* stream);
int mmdx_layernorm_bwd(int dtype, const void* xsum, const void* dy, long rows, int D,
                       const float* gamma, const float* save_mean, const float* save_rstd,
                       void* dx, float* dgamma, float* dbeta, float beta_acc,
                       void* workspace, size_t ws_bytes, void* stream);
size_t mmdx_layernorm_workspace_size(long rows, int D);
/* LayerNorm(dropout(x) + residual) in one pass (BertSelfOutput / BertOutput in train mode):
 * element e of x is kept with the keep bit mmdx_dropout_fwd would draw for it (seed,
 * *counter), scaled by 1/(1-p) and rounded to dtype as that kernel stores it, so the outputs
 * are bit-identical to mmdx_dropout_fwd + mmdx_layernorm_fwd with neither the dropped tensor
 * nor its mask written.  rng[0] (device uint64) receives the stream base for the backward;
 * counter (may be NULL) is incremented after the launch.
 * Replaces: BertSelfOutput.dropout + LayerNorm, BertOutput.dropout + LayerNorm (TP:360). */
int mmdx_layernorm_fwd_dropout(int dtype, const void* x, const void* residual, long rows,
                               int D, const float* gamma, const float* beta, float eps, float p,
                               uint64_t seed, uint64_t* counter, void* y, void* sum_out,
                               float* save_mean, float* save_rstd, uint64_t* rng, void* stream);
/* mmdx_layernorm_bwd with a residual branch's gradient added to dx before its one rounding:
 * dx = LN'(dy) + residual_grad (the pre-LN encoder block's "x + f(LN(x))" backward, vit_b_16);
 * residual_grad must not alias dx. */
int mmdx_layernorm_bwd_residual(int dtype, const void* xsum, const void* dy, long rows, int D,
                                const float* gamma, const float* save_mean,
                                const float* save_rstd, const void* residual_grad, void* dx,
                                float* dgamma, float* dbeta, float beta_acc, void* workspace,
                                size_t ws_bytes, void* stream);
/* mmdx_layernorm_bwd plus dx_drop = the dropout backward of dx with the keep bits of rng[0]
 * (bit-identical to mmdx_dropout_bwd on dx and the forward's mask). */
int mmdx_layernorm_bwd_dropout(int dtype, const void* xsum, const void* dy, long rows, int D,
                               const float* gamma, const float* save_mean,
                               const float* save_rstd, float p, const uint64_t* rng, void* dx,
                               void* dx_drop, float* dgamma, float* dbeta, float beta_acc,
                               void* workspace, size_t ws_bytes, void* stream);
/* GELU backward from the pre-activation: dx = dy * gelu'(pre) */
int mmdx_gelu_bwd(int dtype, const void* pre, const void* dy, long n, void* dx,
                  void* stream);
/* bias gradient: db[N] (+)= sum_m dy[m, N] */
int mmdx_bias_grad(int dtype, const void* dy, long M, int N, float* db, float beta_acc,
                   void* workspace, size_t ws_bytes, void* stream);
size_t mmdx_bias_grad_workspace_size(long M, int N);
/* dropout with a counter-based hash RNG: y = x * mask / (1-p); mask saved as uint8.
 * counter: optional device uint64.  When given, the RNG stream is (seed, offset + *counter
 * << 32) and *counter is incremented after the launch (stream-ordered), so the call can be
 * captured in a hipGraph and every replay draws a fresh mask (torch.nn.Dropout, TP:538). */
int mmdx_dropout_fwd(int dtype, const void* x, long n, float p, uint64_t seed,
                     uint64_t offset, uint64_t* counter, void* y, uint8_t* mask, void* stream);
int mmdx_dropout_bwd(int dtype, const void* dy, const uint8_t* mask, long n, float p,
                     void* dx, void* stream);

/* ---------------------------------------------------------------- loss / heads
 * BCEWithLogitsLoss (mean) (TP:843,1015,1049): loss[0] = mean over B*C;
 * dlogits = (sigmoid(z) - y) / (B*C) * dloss_scale. */
int mmdx_bce_logits_fwd(const float* logits, const float* target, int B, int C,
                        float* loss, void* stream);
int mmdx_bce_logits_bwd(const float* logits, const float* target, int B, int C,
                        const float* dloss, float* dlogits, void* stream);

/* Disease loss: BCE-with-logits with pos_weight, class weights, ignored labels, label smoothing
 * and focal modulation, for imbalanced and partly labelled targets (no counterpart in the
 * reference, which trains with the plain loss above).  logits [B][C] in `dtype` (fp32, bf16 or
 * fp16), target fp32 [B][C]; a NaN target means "no label" (mask m = 0), any other target is a
 * label in [0, 1].  pos_weight / class_weight: fp32 [C] on the device, or NULL for all ones.
 * All arithmetic is fp32.  Per element, with eps = label_smoothing:
 *   y' = y (1 - eps) + eps / 2,  p = sigmoid(z),
 *   bce = pw_c y' softplus(-z) + (1 - y') softplus(z)        (softplus in the max-shifted form),
 *   e   = m cw_c |y' - p|^gamma bce                          (gamma == 0: no pow, factor 1),
 *   g   = de/dz = m cw_c [gamma |d|^(gamma-1) sign(d) p (1-p) bce
 *                         + |d|^gamma ((1 - y') p - pw_c y' (1 - p))],   d = p - y'.
 * gamma is 0 or >= 1 (for 0 < gamma < 1 the gradient is unbounded at p = y').
 *
 * mmdx_disease_loss_fwd, ONE kernel launch (plus a 16-byte memset of the ticket counter when the
 * grid has more than one block), no host sync, no float atomics:
 *   stats fp32 [C][2]: per class (sum_b e, sum_b m);
 *   norm[0]: max(sum m, 1) with mean != 0 (the mean over LABELLED elements), 1 otherwise (sum);
 *   loss[0] = sum e / norm[0] - an all-ignored batch gives 0, never NaN;
 *   g fp32 [B][C] (NULL: no gradient wanted): the UN-normalised element gradient; exactly +0
 *   where the label is ignored.
 * mmdx_disease_loss_bwd: dlogits[i] (in `dtype`) = g[i] * (dloss[0] / norm[0]), rounded once;
 * dloss (NULL = 1) and norm are device scalars, so a scaled loss back-propagates with no sync.
 * The grid grows with B * C; per-block partial sums go through the workspace
 * (mmdx_disease_loss_workspace_size(B, C) bytes, 16-byte aligned; 0 for illegal B, C) and are
 * added by the last block in block order: loss, stats and g are bit-reproducible run to run.
 * Finite for every finite logit whose loss term is representable in fp32 (cw pw |z| below
 * FLT_MAX); g is finite and bounded by cw (gamma + 1) max(pw, 1) for ANY finite logit.
 * Argument errors: C > 64, B * C > 2^31 - 1, gamma or label_smoothing out of range, a NULL or
 * unaligned required pointer, a short workspace, outputs that overlap an input or each other. */
size_t mmdx_disease_loss_workspace_size(long B, int C);
int mmdx_disease_loss_fwd(int dtype, const void* logits, const float* target, long B, int C,
                          const float* pos_weight, const float* class_weight, float gamma,
                          float label_smoothing, int mean, float* loss, float* stats,
                          float* norm, float* g, void* workspace, size_t ws_bytes,
                          void* stream);
int mmdx_disease_loss_bwd(int dtype, const float* g, long n, const float* dloss,
                          const float* norm, void* dlogits, void* stream);

/* ---------------------------------------------------------------- text towers
 * BERT embeddings: word[id] + pos[i] + type[tt] -> LayerNorm (transformers BertEmbeddings,
 * reached from TextEncoderTransformer.encode TP:470/473).  ids/tt int64 [B,L]. */
int mmdx_embed_ln_fwd(int dtype, const int64_t* ids, const int64_t* tt, int B, int L,
                      int D, const float* word, const float* pos, const float* type,
                      const float* gamma, const float* beta, float eps, void* y,
                      void* xsum, float* save_mean, float* save_rstd, void* stream);
/* scatter-add (+=) of dx (= grad of the pre-LN sum) into dense fp32 table grads;
 * rows with id == pad_id get no gradient (nn.Embedding padding_idx; -1 = none) */
int mmdx_embed_bwd(int dtype, const int64_t* ids, const int64_t* tt, int B, int L, int D,
                   const void* dsum, float* dword, float* dpos, float* dtype_tab,
                   int pad_id, void* stream);
/* masked mean pool (TP:452-459): out[b,:] = sum_l h[b,l,:]*m[b,l] / max(sum_l m, 1e-6) */
int mmdx_masked_mean_fwd(int dtype, const void* h, const int64_t* mask, int B, int L,
                         int D, void* out, void* stream);
int mmdx_masked_mean_bwd(int dtype, const void* dout, const int64_t* mask, int B, int L,
                         int D, void* dh, void* stream);
/* fused embedding gather + masked mean (build-defined C2 text tower):
 * out[b,:] = sum_l E[ids[b,l],:]*m[b,l] / max(sum_l m, 1e-6) */
int mmdx_embed_mean_fwd(int dtype, const int64_t* ids, const int64_t* mask, int B, int L,
                        int D, const float* table, void* out, void* stream);
int mmdx_embed_mean_bwd(int dtype, const int64_t* ids, const int64_t* mask, int B, int L,
                        int D, const void* dout, float* dtable, void* stream);
/* embedding gather (rows of an fp32 table -> compute dtype), for the BiLSTM tower */
int mmdx_embed_gather(int dtype, const int64_t* ids, long n, int D, const float* table,
                      void* out, void* stream);
int mmdx_embed_scatter(int dtype, const int64_t* ids, long n, int D, const void* dout,
                       float* dtable, void* stream);

/* Multi-head self-attention core, head dim 64, L <= 256, additive key mask
 * (BertSelfAttention: softmax(QK^T*scale + (1-mask)*(-huge)) V; mask may be NULL = ViT).
 * qkv: [B, L, 3, H, 64] (fused projection output); out: [B, L, H, 64];
 * probs saved for backward: [B, H, L, L] fp32 (NULL in inference).
 * p_drop > 0 (training, BertSelfAttention's dropout on attention_probs): O = (P*keep/(1-p)) V
 * with keep drawn from a counter-based hash of (seed, *counter, b, h, q, key); the saved
 * probabilities carry keep in their sign bit (dropped: -P), so the backward needs neither
 * RNG nor a mask.  counter (device uint64, may be NULL) is incremented after the launch.
 * dqkv: [B, L, 3, H, 64]; workspace holds dS ([B,H,L,roundup32(L)] compute dtype). */
int mmdx_attention_fwd(int dtype, const void* qkv, const int64_t* mask, int B, int L,
                       int H, float scale, float p_drop, uint64_t seed, uint64_t* counter,
                       void* out, float* probs, void* stream);
/* As mmdx_attention_fwd, plus an additive fp32 score bias [H][L][L] shared by the batch
 * (T5's relative position bias; NULL = none) and a causal mask (key > query masked). */
int mmdx_attention_fwd_ex(int dtype, const void* qkv, const int64_t* mask, const float* bias,
                          int causal, int B, int L, int H, float scale, float p_drop,
                          uint64_t seed, uint64_t* counter, void* out, float* probs,
                          void* stream);
/* The backward leaves dS (the score gradient = the bias gradient) in the workspace as
 * [B][H][L][roundup32(L)] compute dtype, for mmdx_t5_position_bias_bwd. */
size_t mmdx_attention_workspace_size(int dtype, int B, int L, int H);
int mmdx_attention_bwd(int dtype, const void* qkv, const float* probs, const void* dout,
                       const int64_t* mask, int B, int L, int H, float scale, float p_drop,
                       void* dqkv, void* workspace, size_t ws_bytes, void* stream);
/* Flash-style variant (16-bit dtypes, no score bias / causal mask): the forward saves the
 * row log-sum-exp lse [B, H, L] fp32 instead of P, and rng[0] (device uint64) receives the
 * dropout stream's base (seed and *counter as the launch read them).  The backward
 * recomputes P from Q, K and lse, the keep bits from the same hash, and the softmax row term
 * rowsum(P o dP) as dO . out (out = the forward's output, which the attention output
 * projection keeps anyway), so no [B, H, L, L] tensor is written or read.  The workspace
 * holds that row term ([B, H, L] fp32).  Same arguments and results otherwise.
 * Replaces: BertSelfAttention / torchvision MultiheadAttention as above (TP:360, vit_b_16). */
int mmdx_attention_fwd_lse(int dtype, const void* qkv, const int64_t* mask, int B, int L,
                           int H, float scale, float p_drop, uint64_t seed, uint64_t* counter,
                           void* out, float* lse, uint64_t* rng, void* stream);
size_t mmdx_attention_lse_workspace_size(int dtype, int B, int L, int H);
int mmdx_attention_bwd_lse(int dtype, const void* qkv, const void* out, const float* lse,
                           const uint64_t* rng, const void* dout, const int64_t* mask, int B,
                           int L, int H, float scale, float p_drop, void* dqkv,
                           void* workspace, size_t ws_bytes, void* stream);

/* LSTM recurrence for one layer, both directions (build-defined C3/C4 tower).
 * xg: [B, L, 2, H, 4] precomputed input gates (x W_ih^T + b_ih + b_hh), the four gates
 *     (i,f,g,o) of a unit adjacent;
 * w_hh: [2][4H][H] compute dtype; h_out: [B, L, 2H]; saved c: [2, L, B, H] fp32,
 * gates: [2, L, B, H, 4] fp32 post-activation, the four gates of a unit adjacent (for
 * backward). */
/* Workspace for the cooperative bf16 forward (H = 256, B <= 256): h exchange + counters.
 * 0 when that path does not apply (then ws may be NULL and the batch-partitioned kernel
 * runs).
 * status: DEVICE int, caller-owned, zero-initialised and STICKY: the cooperative kernel sets
 * it to 1 when a peer workgroup never arrives within spin_limit polls (<= 0: the default,
 * ~2 s) — every workgroup then leaves and the outputs are invalid.  The kernel never clears
 * it; the caller copies it to the host at a sync point and raises (bilstm.py).  A non-zero
 * status on entry makes the kernel leave at its first wait.  debug_flags bit 0 (tests
 * only): workgroup 0 of direction 0 never signals, forcing the timeout path; bit 1 (lab
 * probe, tools/lab/lstm_probe.py): per-step phase timestamps after the workspace (the
 * caller passes [groups][2][8][L][8] u64 more).
 * Returns -22 if the device cannot hold the cooperative grid resident. */
size_t mmdx_lstm_fwd_workspace_size(int dtype, int B, int L, int H);
int mmdx_lstm_fwd(int dtype, const void* xg, const void* w_hh, int B, int L, int H,
                  void* h_out, float* c_save, float* gates_save, void* workspace,
                  size_t ws_bytes, int* status, long spin_limit, int debug_flags,
                  void* stream);
size_t mmdx_lstm_workspace_size(int dtype, int B, int L, int H);
/* Backward.  status (may be NULL): the forward's device status word; with it, bf16, H = 256
 * and B <= 512 run the cooperative recurrence (4 workgroups per 16-row block and direction
 * exchanging dG slices, W_hh^T held in registers), whose bounded wait sets *status = 2 when
 * a peer never arrives within spin_limit polls (<= 0: the default).  NULL: the
 * batch-partitioned kernel.  Both use the same bf16 dG operand, packed fragments and k order;
 * their fp32 cell math may contract a multiply-add differently, and the recurrence carries
 * such a difference on, so the outputs agree to one bf16 ulp of the tensor's scale (most
 * elements exactly; tests/test_text_gpu.py).  debug_flags bit 0 (tests only): workgroup 0 of
 * direction 0 of the cooperative kernel never signals, so the peers' waits time out. */
int mmdx_lstm_bwd(int dtype, const void* w_hh, const void* h_out, const float* c_save,
                  const float* gates_save, const void* dh_out, int B, int L, int H,
                  void* dxg, float* dw_hh, void* workspace, size_t ws_bytes, int* status,
                  long spin_limit, int debug_flags, void* stream);

/* ---------------------------------------------------------------- T5 report head
 * (TP:545-618 cond_proj + T5ForConditionalGeneration, TP:983-991 /
 * TP:1049-1053 teacher-forced CE, IP:190-196 beam generate).  transformers' T5 arithmetic:
 * T5LayerNorm (RMSNorm, no mean / bias), unscaled self-attention with a relative-position
 * bias and a causal mask (mmdx_attention_fwd_ex), cross-attention over the K condition
 * tokens, ReLU FFN, tied lm_head on d_model^-0.5-scaled states, CE with ignore_index -100.
 * rmsnorm: y = w * x * rsqrt(mean(x^2) + eps); save_rstd [rows] fp32.
 * rmsnorm_bwd: dx = (grad) + beta * dx (beta = 1 adds onto a residual gradient);
 * dw (+)= dw_beta * dw + sum_rows dy * x * rstd (dw may be NULL). */
int mmdx_rmsnorm_fwd(int dtype, const void* x, long rows, int D, const float* w, float eps,
                     void* y, float* save_rstd, void* stream);
size_t mmdx_rmsnorm_workspace_size(long rows, int D);
int mmdx_rmsnorm_bwd(int dtype, const void* x, const void* dy, long rows, int D,
                     const float* w, const float* save_rstd, void* dx, float beta, float* dw,
                     float dw_beta, void* workspace, size_t ws_bytes, void* stream);
/* bias[h][q][k] = table[bucket(q - k)][h], table [num_buckets][H] (relative_attention_bias
 * .weight), causal (decoder) buckets of T5Attention._relative_position_bucket. */
int mmdx_t5_position_bias(const float* table, int H, int L, int num_buckets, int max_distance,
                          float* bias, void* stream);
/* dtable (+)= bucketed sum over batch and cells of dscores [B][H][L][ld] (compute dtype). */
int mmdx_t5_position_bias_bwd(int dtype, const void* dscores, int B, int H, int L, int ld,
                              int num_buckets, int max_distance, float* dtable, float beta,
                              void* stream);
/* Cross-attention over Lk <= 16 keys (the K condition tokens), head dim 64, no mask:
 * q rows [B][Lq] of ldq elements (head h at h*64); kv [B][Lk][2][H][64] (k then v);
 * out [B][Lq][H][64]; probs [B][H][Lq][Lk] fp32 (dropout keep bit in the sign, as
 * mmdx_attention_fwd).  dq rows of lddq elements; dkv like kv. */
int mmdx_xattn_fwd(int dtype, const void* q, long ldq, const void* kv, int B, int Lq, int Lk,
                   int H, float scale, float p_drop, uint64_t seed, uint64_t* counter,
                   void* out, float* probs, void* stream);
size_t mmdx_xattn_workspace_size(int B, int Lq, int Lk, int H);
int mmdx_xattn_bwd(int dtype, const void* q, long ldq, const void* kv, const float* probs,
                   const void* dout, int B, int Lq, int Lk, int H, float scale, float p_drop,
                   void* dq, long lddq, void* dkv, void* workspace, size_t ws_bytes,
                   void* stream);
/* CrossEntropyLoss(ignore_index=-100) mean over the rows whose target is in [0, V):
 * loss, count (device scalars).  The workspace keeps per-row log-sum-exp for the backward:
 * dlogits = (softmax - onehot) * dloss / count (dloss device scalar or NULL = 1). */
size_t mmdx_cross_entropy_workspace_size(long rows);
int mmdx_cross_entropy_fwd(const float* logits, const int64_t* targets, long rows, long V,
                           float* loss, float* count, void* workspace, size_t ws_bytes,
                           void* stream);
int mmdx_cross_entropy_bwd(int dtype, const float* logits, const int64_t* targets, long rows,
                           long V, const float* dloss, const float* count,
                           const void* workspace, void* dlogits, void* stream);
/* row-wise log_softmax (beam search scores) */
int mmdx_log_softmax(const float* logits, long rows, long V, float* out, void* stream);
/* dx = dy * (y > 0) (T5 DenseReluDense backward from the ReLU output) */
int mmdx_relu_bwd(int dtype, const void* y, const void* dy, long n, void* dx, void* stream);
/* One incremental decoder step of T5's causal self-attention over a KV cache (beam search of
 * report_model.generate, IP:190-196 / TP:613-618): qkv [R][3*H*64] of position `pos`;
 * caches [R][Lmax][H*64]; key j of row r is read from cache row slots[r*Lmax + j] (the beam's
 * ancestry, so reordering beams moves no cache data); bias [H][Lmax][Lmax] fp32 relative-
 * position bias (mmdx_t5_position_bias); out [R][H*64].  The step's K/V are appended at
 * (row r, pos).  Lmax <= 512. */
int mmdx_t5_decode_attn(int dtype, const void* qkv, int R, int H, int pos, int Lmax,
                        void* k_cache, void* v_cache, const int* slots, const float* bias,
                        void* out, void* stream);
/* Beam-search candidate step (GenerationMixin._beam_search's topk, IP:190 num_beams): per
 * batch row b, the k (<= 16) largest log_probs[b*nb + i][v] + run_scores[b*nb + i] over
 * (i, v), ordered by value desc then flat index i*V + v asc; out_idx = that flat index.
 * First writes -inf into log_probs at the n_ban (row, token) int pairs of ban_pairs
 * (no_repeat_ngram_size) and, when eos_ban >= 0, at column eos_ban (min_new_tokens). */
int mmdx_beam_topk(float* log_probs, int B, int nb, long V, const float* run_scores,
                   const int* ban_pairs, int n_ban, int eos_ban, int k, float* out_val,
                   long* out_idx, void* stream);

/* ---------------------------------------------------------------- optimizer
 * torch.optim.AdamW (decoupled weight decay) over every tensor of every param group in
 * one launch (build_optimizer groups TP:238-269, TP:408-432; fusion optimiser
 * TP:1018-1023).  `table` is a DEVICE array of chunk descriptors: each parameter tensor is
 * split into chunks (host side, <= 64K elements) and each descriptor carries the chunk's
 * p/g/m/v pointers, its length n and its group's lr/wd; one workgroup per chunk.
 * step_dev (device fp32) is incremented by the call, so the update replays inside a
 * graph.  grad_scale (device scalar or NULL) multiplies every gradient: the clip
 * coefficient of clip_grad_norm_ (TP:1058). */
typedef struct {
  float* p;
  const float* g;
  float* m;
  float* v;
  long n;
  long off;   /* informational: element offset of the chunk in its tensor */
  float lr;
  float wd;
} mmdx_adamw_tensor;
int mmdx_adamw_multi(int nchunks, const mmdx_adamw_tensor* table, float beta1, float beta2,
                     float eps, float* step_dev, const float* grad_scale, void* stream);
/* global L2 norm of the .g fields of `table`; scale[0] = min(1, max_norm/(norm+1e-6))
 * (torch.nn.utils.clip_grad_norm_); max_norm <= 0 gives scale 1. */
size_t mmdx_grad_norm_workspace_size(int nchunks);
int mmdx_grad_norm(int nchunks, const mmdx_adamw_tensor* table, float max_norm, float* norm,
                   float* scale, void* workspace, size_t ws_bytes, void* stream);
/* in-place g *= scale[0] over the .g fields (the mul_ of clip_grad_norm_) */
int mmdx_scale_grads(int nchunks, const mmdx_adamw_tensor* table, const float* scale,
                     void* stream);
/* Refresh the .g column of a device chunk table in stream order, without a host->device
 * copy (the optimizer's gradient buffers move between steps): row r, whose tensor index is
 * row_tensor[r] (a DEVICE int array built with the table), gets
 * g = grads[row_tensor[r]] + off.  `grads` is a HOST array of n_tensors device pointers;
 * they travel as kernel arguments (256 per launch).  A small hipMemcpyAsync from pinned
 * memory made the issuing host thread wait for the stream on this runtime. */
int mmdx_adamw_patch_grads(int nchunks, mmdx_adamw_tensor* table, const int* row_tensor,
                           int n_tensors, const float* const* grads, void* stream);

/* Mixed-precision loss scaling: torch.cuda.amp.GradScaler as the fusion loop drives it
 * (TP:1025-1026 GradScaler(enabled=use_amp), TP:1056 scaler.scale(loss).backward(), TP:1058
 * clip_grad_norm_, TP:1060-1061 scaler.step / scaler.update).
 * mmdx_grad_norm_amp: as mmdx_grad_norm over gradients that hold loss_scale[0] * g;
 * found_inf[0] = 1 if any gradient is inf/NaN; scale[0] = clip coefficient / loss_scale[0],
 * the clip coefficient taken on the unscaled norm (unscale_first != 0: scaler.unscale_ before
 * the clip) or on the scaled one (0: the reference's order, clip then scaler.step).
 * mmdx_adamw_multi_amp: mmdx_adamw_multi that skips the whole step (no update, no step
 * count) when found_inf[0] != 0 (scaler.step's skip).
 * mmdx_amp_update_scale: scaler.update() (torch._amp_update_scale_): overflow -> scale *=
 * backoff_factor, tracker = 0; else every growth_interval clean steps scale *= growth_factor.
 * mmdx_mul_dev_scalar: out = x * s[0], fp32 (scaler.scale(loss) and its backward). */
int mmdx_grad_norm_amp(int nchunks, const mmdx_adamw_tensor* table, float max_norm,
                       const float* loss_scale, int unscale_first, float* norm, float* scale,
                       float* found_inf, void* workspace, size_t ws_bytes, void* stream);
int mmdx_adamw_multi_amp(int nchunks, const mmdx_adamw_tensor* table, float beta1, float beta2,
                         float eps, float* step_dev, const float* grad_scale,
                         const float* found_inf, void* stream);
int mmdx_amp_update_scale(float* scale, int* growth_tracker, const float* found_inf,
                          float growth_factor, float backoff_factor, int growth_interval,
                          void* stream);
int mmdx_mul_dev_scalar(const float* x, long n, const float* s, float* out, void* stream);

/* ---------------------------------------------------------------- validation metrics
 * Integer sufficient statistics of the multi-label validation metrics, computed from the
 * fp32 [N][C] row-major logits / multi-hot targets as the model and the loader produce them
 * (no transpose, no sort, no workspace).  A target is positive iff target > 0.5.  Every output
 * is an int64 count accumulated with integer atomics, so the results do not depend on the
 * order of accumulation: bit-reproducible run to run and exactly comparable with a CPU
 * reference.  Limits (argument errors): 1 <= C <= 64 and N*C <= 2^24.
 *
 * mmdx_auroc_pairs: out int64 [(C+1)][4], zeroed by the entry point.  Row c < C is
 * {u2, n_pos, n_neg, n_nan} of class c with
 *   u2 = sum over (i positive, j negative) of 2*[s_i > s_j] + [s_i == s_j]   (IEEE compares:
 *   -0 == +0 ties, +-inf order like any value; an item with a NaN score adds 0 and is counted
 *   in n_nan only, so n_pos + n_neg + n_nan = N);
 * row C is the same statistic over all N*C (score, target) pairs as one class (micro).
 * AUROC = u2 / (2 n_pos n_neg): Mann-Whitney U with midranks for ties.  Tiled all-pairs
 * counting: O(N^2 C) compares per-class plus O((N C)^2) micro, which the N*C limit bounds
 * (u2 <= 2 * 2^48).
 *
 * mmdx_confusion_grid: thr fp32 [T], non-decreasing, in LOGIT space, 1 <= T <= 256; tp / fp
 * int64 [C][T], zeroed by the entry point: tp[c][t] = #{i : target_ic positive and
 * logit_ic >= thr[t]}, fp[c][t] the same over the negatives (a NaN logit counts nowhere). */
int mmdx_auroc_pairs(const float* scores, const float* target, int N, int C, int64_t* out,
                     void* stream);
int mmdx_confusion_grid(const float* logits, const float* target, int N, int C,
                        const float* thr, int T, int64_t* tp, int64_t* fp, void* stream);

/* ---------------------------------------------------------------- calibration
 * Post-hoc calibration of the disease probabilities: a monotone per-class map z' = a_c z + b_c,
 * p = sigmoid(z'), fitted on held-out fp32 [N][C] logits and targets, and the reliability
 * statistics that measure it.  The CPU statement (float64) is mmdx/calibration.py.
 *
 * mmdx_calib_fit_step is ONE pass of a damped-Newton (Levenberg-Marquardt) fit; a fit is
 * iters + 1 calls on one stream, pass = 0 ... iters with last != 0 in the final one, all with
 * the same arguments otherwise and the same workspace, which carries the solver state from pass
 * to pass (mmdx_calib_fit_workspace_size(N, C) bytes, 16-byte aligned, no initialisation
 * needed; 0 for illegal N, C).  No host sync, no data-dependent launch count, no float atomics.
 *   mode MMDX_CALIB_PLATT: a free (a_c, b_c) per class; MMDX_CALIB_TEMPERATURE: one scalar a
 *   for all classes, b = 0 (NLL, ga, haa summed over the classes in class order).
 *   A NaN target means "no label" (m = 0), any other target is a label y in [0, 1].
 *   counts fp64 [C][2] on the device: (n_pos_c, n_neg_c) = (sum m y, sum m (1 - y)).  With
 *   smooth != 0 the targets are Platt's, t = t_neg + y (t_pos - t_neg), t_pos = (n_pos + 1) /
 *   (n_pos + 2), t_neg = 1 / (n_neg + 2) (finite optimum on separable data); else t = y.
 *   Objective: NLL_c = sum_i m (softplus(z') - t z').
 * Per pass, one launch: z' = a z + b with (a, b) the trial point rounded to fp32, as a separate
 * multiply and add (never an fma, so the host reproduces z' bit for bit); fp32 element terms
 * (one max-shifted expf, one log1pf, 1 - p as sigmoid(-z')); the seven per-class sums (NLL, ga,
 * gb, haa, hab, hbb, labelled count) in fp64 from the thread upward, through a fixed-order LDS
 * tree and per-block partials that the last block (integer ticket) adds in block order:
 * bit-reproducible.  The last block then takes the solver step in fp64: pass 0 evaluates
 * (1, 0) with lambda = 1e-3; a trial point whose NLL is <= NLL_accepted (1 + 1e-9) is accepted
 * and lambda /= 10 (floor 1e-9), else it is rejected and lambda *= 10 (cap 1e12); the next
 * trial point is theta_acc - (H_acc with its diagonal scaled by (1 + lambda))^-1 g_acc.  It
 * leaves the ticket counter at 0 for the next pass.
 * The final pass (last != 0) evaluates the last trial point, and writes for the accepted point
 *   status int32 [C]: 0 fitted; 1 inactive (n_pos < min_count or n_neg < min_count, or nothing
 *     labelled); 2 not converged (Newton decrement g^T H^-1 g per labelled element > tol, or a
 *     value not finite); 3 non-positive slope.  In temperature mode the pooled counts and sums
 *     decide one status for all classes.
 *   scale, bias fp32 [C]: (a_c, b_c) where status is 0, the identity (1, 0) elsewhere;
 *   info fp64 [C][4]: NLL at the identity, NLL at the result, Newton decrement per labelled
 *     element, labelled count (temperature mode: the pooled values, repeated per class).
 * scale, bias, status and info may be NULL in the other passes.  pass = 0 with last != 0 is a
 * plain evaluation of the NLL at the identity.  Argument errors: C > 64, N * C > 2^31 - 1, an
 * unknown mode, min_count < 0, tol not in (0, inf), a NULL or unaligned required pointer, a
 * short workspace, outputs that overlap an input or each other.
 *
 * mmdx_reliability_bins: the integer sufficient statistics of a reliability diagram with n_bins
 * equal-width probability bins, 1 <= n_bins <= 64.  z' = z * scale[c] + bias[c] (an explicit
 * multiply and add; scale = bias = NULL: z' = z exactly); edges fp32 [n_bins - 1], the interior
 * bin edges in LOGIT space, non-decreasing (NULL allowed for n_bins = 1); the bin of an element
 * is #{k : edges[k] <= z'}, so an edge belongs to the upper bin.  A target is positive iff
 * target > 0.5; an element with a NaN z' is dropped and counted.  out int64, zeroed by the
 * entry point: [(C + 1)][n_bins][4] = {count, positives, sum round(p 2^30),
 * sum round((p - y)^2 2^30)} with p = sigmoid(z') in fp32 and y in {0, 1}, followed by
 * [(C + 1)] NaN counts; row C pools all classes (micro).  Integer atomics only:
 * bit-reproducible and exactly comparable with a CPU reference.  Limits as the validation
 * metrics: C <= 64, N * C <= 2^24. */
enum { MMDX_CALIB_TEMPERATURE = 0, MMDX_CALIB_PLATT = 1 };
size_t mmdx_calib_fit_workspace_size(long N, int C);
int mmdx_calib_fit_step(const float* logits, const float* target, long N, int C,
                        const double* counts, int smooth, int mode, int pass, int last,
                        long min_count, double tol, float* scale, float* bias, int* status,
                        double* info, void* workspace, size_t ws_bytes, void* stream);
int mmdx_reliability_bins(const float* logits, const float* target, int N, int C,
                          const float* scale, const float* bias, const float* edges, int n_bins,
                          int64_t* out, void* stream);

/* ---------------------------------------------------------------- bootstrap
 * Non-parametric bootstrap over ROWS for the validation metrics: a row is resampled with all of
 * its C labels.  Integer arithmetic with one owner per output: bit-reproducible and exactly
 * comparable with a CPU reference (mmdx/bootstrap.py: reference_weights, reference_counts).
 *
 * mmdx_bootstrap_weights: w int32 [R][N]; w[r][i] = how often row i is drawn among the N draws
 * of replicate r0 + r, so every row of w sums to N.  Draw k of replicate r is
 *   idx = mulhi64(mix64(mix64(seed ^ ((r + 1) G)) + (k + 1) G), N),  G = 0x9E3779B97F4A7C15,
 * mix64 the SplitMix64 output function (csrc/bootstrap_rng.h): it depends on (seed, r, k, N)
 * alone, so batching with r0 is invisible.  N <= 131072: a block per replicate and window of
 * 16384 rows makes all N draws and keeps the histogram of its window in LDS, plain stores; longer
 * rows: integer atomics on w, which the entry point zeroes.
 * Limits: R, N >= 1, r0 >= 0, R * N <= 2^26.
 *
 * mmdx_bootstrap_counts: out int64 [R][(C + 1)][5] = {u2, w_pos, w_neg, tp, fp}; row c < C is
 * class c, row C the flattened (micro) problem in which element (i, c) carries w[r][i]:
 *   w_pos / w_neg = sum of w[r][i] over the live positives / negatives,
 *   u2 = sum over live (positive i, negative j) of w[r][i] w[r][j] ([s_i > s_j] + [s_i >= s_j])
 *        (mmdx_auroc_pairs' u2 with multiplicities; AUROC = u2 / (2 w_pos w_neg)),
 *   tp / fp = sum of w[r][i] over the live positives / negatives whose PRED flag is set.
 * The score order does not depend on the replicate, so the caller sorts ONCE and passes items:
 * an item is (row << 3) | flags, flags = 1 positive | 2 live (score not NaN) | 4 predicted; an
 * item that is not live counts nowhere, and every item's row is < N.
 *   class_items int32 [2][C][n_pad], n_pad = N rounded up to a multiple of 4: column c in
 *     ascending score order, within equal scores positives first ([0]: order A) or negatives
 *     first ([1]: order B); the pad items are 0;
 *   micro_items int32 [2][m_pad], m_pad = N * C rounded up likewise: all N * C elements.
 * With T(order) = sum over positives k of w_k * (negative weight strictly earlier in the order),
 * u2 = T(A) + T(B): a weighted exclusive prefix scan, no tie logic.  Three launches: the weights
 * are transposed to [N][R rounded up to 8] (the 8 replicate weights of a row then share 32
 * contiguous bytes); a block scans one 2048-item segment of one column in one order for 8
 * replicates and stores the segment's partial sums; then one thread per (replicate, column) adds
 * the segments in order with their cross terms and writes the output row.  Plain stores
 * throughout: no atomics, no memset.  workspace: mmdx_bootstrap_counts_workspace_size(R, N, C)
 * bytes (0 for illegal R, N, C; the transposed weights plus 48 bytes per replicate and segment),
 * 16-byte aligned, no initialisation needed.
 * weights int32 [R][N], non-negative, every row summing to at most 2^31 / C (a bootstrap row sums
 * to N): the prefix sums are 32-bit, the products 64-bit (u2 <= 2^49).  Neither is checked.
 * Limits (argument errors): 1 <= C <= 64, N * C <= 2^24, R * N <= 2^26, item arrays 16-byte
 * aligned, a short or misaligned workspace. */
int mmdx_bootstrap_weights(int R, long r0, int N, uint64_t seed, int* w, void* stream);
size_t mmdx_bootstrap_counts_workspace_size(int R, int N, int C);
int mmdx_bootstrap_counts(const int* class_items, const int* micro_items, const int* weights,
                          int R, int N, int C, int64_t* out, void* workspace, size_t ws_bytes,
                          void* stream);

/* ---------------------------------------------------------------- Grad-CAM
 * Heatmaps of the disease head at the trunk's last conv stage.  Between that feature map and
 * the logits there is only the global average pool and the heads, so the Grad-CAM channel
 * weights are alpha[b][c][k] = (d logit_c / d pooled_k) / (H W); these two kernels do the rest.
 * Both are bit-reproducible (fixed summation order, no atomics) and need no workspace.
 *
 * mmdx_cam_fwd: raw[b][c][p] = max(0, sum_k alpha[b][c][k] * fmap[b][p][k]), accumulated in
 * fp32.  fmap [B][HW][K] in `dtype` (the trunk's NHWC activation), alpha fp32 [B][C][K], raw
 * fp32 [B][C][HW].  K % 8 == 0, C <= 64, HW <= 1024; fmap and alpha 16-byte aligned.
 *
 * mmdx_cam_resize: out fp32 [BC][Ho][Wo] = bilinear resize of raw fp32 [BC][H][W] with
 * half-pixel centres (torch's interpolate(mode="bilinear", align_corners=False): source
 * coordinate (d + 0.5) * in / out - 0.5 clamped at 0, edges replicated).  normalize != 0 first
 * divides every map by its own maximum; a maximum <= 0 gives an all-zero map, never NaN.
 * H * W <= 1024, Ho and Wo <= 4096; out 16-byte aligned. */
int mmdx_cam_fwd(int dtype, const void* fmap, const float* alpha, int B, int HW, int K, int C,
                 float* raw, void* stream);
int mmdx_cam_resize(const float* raw, int BC, int H, int W, int Ho, int Wo, int normalize,
                    float* out, void* stream);

/* ---------------------------------------------------------------- ViT explanations
 * The transformer tower has no conv stage for Grad-CAM; its explanations are built on the
 * attention probabilities, which the flash-style attention core never stores.  These two
 * kernels recompute them per layer and walk the class-token row down the layers.  Both are
 * bit-reproducible (fixed summation order, one writer per element, no atomics), independent of
 * the launch geometry, and need no workspace.
 *
 * mmdx_attention_relevance: out fp32 [B][Ls][Ls] = the head-averaged attention map of one
 * block from its qkv buffer [B*Ls][3][H][64] in `dtype`.  P_h = softmax_j(scale Q_h K_h^T)
 * (no key mask; MFMA products with fp32 accumulation, fp32 softmax with the row maximum
 * subtracted).  dout == NULL: out = (1/H) sum_h P_h (rows sum to 1).  dout [B*Ls][H][64] in
 * `dtype` (the gradient of a scalar with respect to the attention core's output):
 * out = (1/H) sum_h relu(P_h o dP_h), dP_h = dO_h V_h^T.  The head sum runs h = 0 .. H-1 in
 * fp32.  1 <= Ls <= 256, 1 <= H <= 16, head dim 64; qkv and dout 16-byte aligned.
 *
 * mmdx_rollout_step: r_out[b][j] = alpha r_in[b][j] + beta sum_i r_in[b][i] abar[b][i][j], all
 * fp32, r [B][Ls], abar [B][Ls][Ls]; i is summed in ascending order by the thread that owns
 * column j.  (alpha, beta) = (a, 1 - a) is one layer of attention rollout with residual a,
 * (1, 1) one layer of the relevance recursion R <- R + abar R, both for the class-token row
 * taken from the last layer down.  Ls <= 4096; r_out must not overlap r_in. */
int mmdx_attention_relevance(int dtype, const void* qkv, const void* dout, int B, int Ls, int H,
                             float scale, float* out, void* stream);
int mmdx_rollout_step(const float* r_in, const float* abar, int B, int Ls, float alpha,
                      float beta, float* r_out, void* stream);

/* ---------------------------------------------------------------- text explanations
 * mmdx_token_relevance_step: one layer of the relevance recursion for a row vector, fused with
 * the recomputation of the attention probabilities under a key mask, in ONE launch that never
 * writes the [Ls][Ls] map:
 *   P_h[i][j] = softmax over the real keys j of (scale Q_h[i] . K_h[j]); exactly 0 for a masked j
 *   abar      = (1/H) sum_h relu(P_h o dP_h), dP_h = dO_h V_h^T   (dout given)
 *               (1/H) sum_h P_h                                   (dout == NULL)
 *   r_out[b][j] = alpha r_in[b][j] + beta sum_i r_in[b][i] abar[b][i][j]
 * qkv [B*Ls][3][H][64] and dout [B*Ls][H][64] in `dtype` as for mmdx_attention_relevance; mask
 * int64 [B][Ls], 1 = a real token (NULL: all real), the tensor the attention forward takes; it
 * applies to the keys only (every query row is computed).  A sample without a real key has
 * abar = 0, so r_out = alpha r_in; nothing is NaN or inf.  A masked column j gets alpha r_in[j]
 * exactly.  r_in, r_out fp32 [B][Ls], not overlapping.  1 <= Ls <= 256, 1 <= H <= 16, head dim
 * 64; qkv and dout 16-byte aligned.
 *
 * No float atomics, bit-reproducible, and row b depends neither on B nor on the other samples:
 * a workgroup adds its 32 queries in a fixed order, and the ceil(Ls / 32) workgroups of a sample
 * meet through the workspace, where the last one to arrive adds their partial rows in tile order.
 * The workspace (mmdx_token_relevance_workspace_size bytes, 16-byte aligned; 0 for Ls <= 32, then
 * NULL will do) starts with one integer counter per sample, B in all, padded to 16 bytes: these
 * must be ZERO before the first launch on a buffer; every launch leaves them zero.  The partial
 * rows follow them, so a buffer is reused as it is only by launches of the same B (another B:
 * zero the counters again).  Launches that share a workspace must be ordered (one stream). */
size_t mmdx_token_relevance_workspace_size(int B, int Ls);
int mmdx_token_relevance_step(int dtype, const void* qkv, const void* dout, const int64_t* mask,
                              const float* r_in, int B, int Ls, int H, float scale, float alpha,
                              float beta, float* r_out, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ---------------------------------------------------------------- training augmentation
 * Per-image affine warp + contrast / brightness of normalised images, one launch, no workspace,
 * no atomics, bit-reproducible.  x, out fp32 [B][C][H][W] (NCHW, contiguous, out must not
 * overlap x); params fp32 [B][8] on the DEVICE, row b = (a00, a01, ox, a10, a11, oy, gain,
 * delta); mean, stdv: HOST arrays of C floats (the normalisation x carries, stdv > 0).
 *
 * With cx = (W-1)/2, cy = (H-1)/2, dx = j - cx, dy = i - cy, output pixel (i, j) samples the
 * source position sx = a00 dx + a01 dy + (cx + ox), sy = a10 dx + a11 dy + (cy + oy) (pixel
 * index coordinates) as the bilinear blend of the four taps (floor(sy) | +1, floor(sx) | +1);
 * a tap outside the image reads fill_c = (0 - mean_c) / std_c (black).  The blend weights are
 * exactly 1 and 0 at integer positions, so identity / flip / quarter-turn / whole-pixel-shift
 * rows return input bits.  sx, sy are clamped in floating point to [-1.5, size + 0.5] before
 * the conversion to int (all taps are outside there anyway): any parameter row is safe.
 * Then v' = gain v + ((gain - 1)(mean_c - 0.5) + delta) / std_c, i.e. the pixel-space
 * p' = gain (p - 0.5) + 0.5 + delta, and with clamp != 0 v' is clamped to
 * [(0 - mean_c) / std_c, (1 - mean_c) / std_c], the fp32 values mmdx_image_preprocess writes
 * for the pixel values 0 and 255.  Limits: 1 <= C <= 4, H, W <= 4096, B <= 65535. */
int mmdx_augment_affine(const float* x, const float* params, int B, int C, int H, int W,
                        const float* mean, const float* stdv, int clamp, float* out,
                        void* stream);

/* ---------------------------------------------------------------- CLAHE
 * Contrast-limited adaptive histogram equalisation of 8-bit images (the algorithm of OpenCV's
 * CLAHE_Impl; mmdx/clahe.py states it and its numpy `reference` is the definition these
 * kernels equal byte for byte).  pixels: decoded HWC uint8 images packed back to back, the
 * buffer mmdx_image_preprocess takes; one descriptor per image.  Each channel is an
 * independent plane.
 *
 * mmdx_clahe_luts: per (image, channel, tile) the 256-bin histogram of the tile of the
 * reflect-101 extended image, clipped at `clip` (0 = no clipping) with the excess redistributed
 * (clipped / 256 to every bin, the remainder res to the bins i with i % step == 0 and
 * i / step < res, step = max(256 / res, 1)), prefix-summed, and
 * lut[i] = clamp(rint(float(cdf[i]) * lut_scale), 0, 255) written as 256 bytes at
 * luts[lut_off + ((channel * tiles_y + tile row) * tiles_x + tile column) * 256].
 *
 * mmdx_clahe_apply: out of place into a buffer of the same packed layout.  Pixel (y, x) blends
 * the LUTs of the tile rows max(y1, 0), min(y1 + 1, tiles_y - 1) and columns alike, where
 * f = float(y) * (1.0f / tile_h) - 0.5f, y1 = floor(f), ya = f - y1, ya1 = 1.0f - ya:
 * r = (L11 xa1 + L12 xa) ya1 + (L21 xa1 + L22 xa) ya, every operation a correctly-rounded fp32
 * one (no fused multiply-add), out = clamp(rint(r), 0, 255).
 *
 * Both take the descriptor table twice: descs_host (HOST memory) is validated in full before
 * any launch - geometry, limits, and every offset against pixel_bytes / lut_bytes / out_bytes -
 * and sizes the grid; descs_dev is the same table in DEVICE memory, which the kernels read.
 * Limits: c in {1, 3}; 1 <= tiles_x, tiles_y <= 16; w >= 2 tiles_x, h >= 2 tiles_y; w, h <=
 * 65535; tile_w * tile_h <= 2^24; B <= 65535; lut_off a multiple of 256, LUTs and outputs in
 * descriptor order without overlap; luts 4-byte aligned; out must not overlap pixels.
 * No workspace; integer atomics in LDS only, so the result is bit-reproducible. */
typedef struct {
  long src_off, dst_off; /* byte offsets of the image's HWC pixels: source, destination */
  long lut_off;          /* byte offset of the image's [c][tiles_y][tiles_x][256] LUTs */
  int w, h, c;           /* width, height, channels (1 or 3) */
  int tiles_x, tiles_y;  /* tiles per row, per column */
  int tile_w, tile_h;    /* tile size of the extended image */
  int clip;              /* histogram clip in counts, 0 = none */
  float lut_scale;       /* 255.0f / (tile_w * tile_h) */
} mmdx_clahe_desc;
size_t mmdx_clahe_desc_size(void); /* sizeof(mmdx_clahe_desc): binding layout check */
int mmdx_clahe_luts(const uint8_t* pixels, size_t pixel_bytes, const mmdx_clahe_desc* descs_host,
                    const mmdx_clahe_desc* descs_dev, int B, uint8_t* luts, size_t lut_bytes,
                    void* stream);
int mmdx_clahe_apply(const uint8_t* pixels, size_t pixel_bytes,
                     const mmdx_clahe_desc* descs_host, const mmdx_clahe_desc* descs_dev, int B,
                     const uint8_t* luts, size_t lut_bytes, uint8_t* out, size_t out_bytes,
                     void* stream);

/* ---------------------------------------------------------------- 16-bit windowing
 * Grey-level windowing of 16-bit single-channel images to 8 bits (mmdx/window.py states it and
 * its numpy `reference` is the definition these kernels equal byte for byte).  pixels: the
 * images' uint16 pixels, every image starting at a 16-byte boundary and padded to one
 * (src_off and the buffer's size are multiples of 16; the padding is read, never used).
 * out: the (H, W, 1) uint8 images packed back to back, the buffer mmdx_clahe_* and
 * mmdx_image_preprocess take.  One descriptor per image.
 *
 * mmdx_window_levels (mode 0 descriptors only): per image a 65536-bin uint32 histogram in
 * `workspace` (integer atomics), then lo = the k_lo-th and hi = the k_hi-th order statistic
 * (0-based) of its pixels, hi = lo + 1 when they are equal, written to
 * levels[4 b + {0, 1, 2, 3}] = lo, hi, the bits of 255.0f / float(hi - lo), 0 on the device.
 * workspace: mmdx_window_workspace_size(B) bytes (0 for a B outside the limits), 16-byte
 * aligned, ALL ZERO on entry; it is all zero again when the call's work on `stream` is done,
 * so a second call needs no reset.
 *
 * mmdx_window_apply: y = clamp(rint((float(v) - lo) * scale), 0, 255), one exact fp32
 * subtraction, one fp32 multiply, rounding half to even; 255 - y when invert.  Mode 0 takes lo
 * and scale from `levels` (the array mmdx_window_levels wrote), mode 1 from the descriptor;
 * levels may be NULL when every descriptor has mode 1.
 *
 * Both take the descriptor table twice, as the CLAHE entries do: descs_host (HOST memory) is
 * validated in full before any launch and sizes the grid; descs_dev is the same table in
 * DEVICE memory.  Limits: 1 <= w, h <= 65535; w * h <= 2^30; B <= 65535; mode 0:
 * 0 <= k_lo <= k_hi < w * h; mode 1: lo, hi multiples of 0.5 with
 * -65536 <= lo < hi <= 131072 and scale == 255.0f / (hi - lo); sources and outputs in
 * descriptor order without overlap; out must not overlap pixels.  Integer atomics only, so the
 * result is bit-reproducible, and an image's result does not depend on the rest of the batch. */
typedef struct {
  long src_off, dst_off; /* byte offsets: uint16 source (multiple of 16), uint8 destination */
  int w, h;              /* width, height */
  int mode;              /* 0 = percentile (ranks below), 1 = fixed (lo, hi, scale below) */
  int invert;            /* 0 / 1: write 255 - y */
  int k_lo, k_hi;        /* mode 0: 0-based ranks of the two order statistics */
  float lo, hi, scale;   /* mode 1: the window and 255.0f / (hi - lo) */
} mmdx_window_desc;
size_t mmdx_window_desc_size(void); /* sizeof(mmdx_window_desc): binding layout check */
size_t mmdx_window_workspace_size(int B);
int mmdx_window_levels(const uint16_t* pixels, size_t pixel_bytes,
                       const mmdx_window_desc* descs_host, const mmdx_window_desc* descs_dev,
                       int B, void* workspace, size_t workspace_bytes, int* levels, void* stream);
int mmdx_window_apply(const uint16_t* pixels, size_t pixel_bytes,
                      const mmdx_window_desc* descs_host, const mmdx_window_desc* descs_dev, int B,
                      const int* levels, uint8_t* out, size_t out_bytes, void* stream);

/* ---------------------------------------------------------------- similar-case retrieval
 * Exact top-k inner-product search (mmdx/retrieval.py: reference_search is the definition).
 * index [N][d] row-major, queries [nq][d], both `dtype` (fp32, bf16 or fp16), 16-byte aligned.
 * score[i][j] = sum_t q[i][t] x[j][t], accumulated in fp32 by one MFMA chain over d in a fixed
 * order: the bits of a score depend on the query row and the index row alone, not on N, nq, k,
 * the row's position or the grid.  A NaN score counts as -inf; a zero score is +0.0.  Row
 * exclude[i] (int32 [nq] on the device, -1 = none, NULL = none for all; entries outside [-1, N)
 * match no row: the caller checks the range) is removed for query i.  out_ids int32 [nq][k] and
 * out_scores fp32 [nq][k]: the first k remaining rows under (score descending, id ascending);
 * slots past the number of remaining rows hold id -1 and score -inf.
 *
 * Two launches on `stream` (select: one streaming pass over the index per group of 16 queries,
 * each block's k best per query into the workspace; merge: one block per query), no [nq][N]
 * score matrix, no atomics in global memory, no counter: bit-reproducible, and a search over
 * slices of the index merged under the same order equals the search over the whole.
 * Limits (rejected before any launch): 1 <= N <= 2^24, d % 32 == 0, 32 <= d <= 4096,
 * 1 <= nq <= 64, 1 <= k <= 64.  workspace: mmdx_topk_similar_workspace_size bytes (blocks * nq *
 * k pairs; 0 for an unsupported shape), 16-byte aligned; outputs overlap neither each other nor
 * an input.  mmdx_topk_rows_per_block: the index rows of one block step (a tile edge for tests). */
int mmdx_topk_rows_per_block(void);
size_t mmdx_topk_similar_workspace_size(long N, int d, int nq, int k);
int mmdx_topk_similar(void* stream, int dtype, const void* queries, const void* index, long N,
                      int d, int nq, int k, const int* exclude, float* out_scores, int* out_ids,
                      void* workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* MMDX_H_ */
