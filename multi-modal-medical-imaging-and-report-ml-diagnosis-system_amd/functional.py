"""Autograd functions over the HIP kernels (the only compute path; no fallback).

Every forward/backward here is a sequence of C-ABI calls on torch's current HIP stream,
so a whole train step (forward, backward, optimizer) can be captured into one hipGraph.
Parameters stay fp32 (PyTorch layouts, state_dict-identical to the reference); the
compute dtype of activations is fp32 (parity path) or bf16 (throughput path).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib as L
from ._lib import call, ptr, stream

__all__ = [
    "gemm", "cast", "linear", "fusion_linear", "layer_norm", "dropout", "bce_with_logits",
    "masked_mean", "embed_mean", "auroc_counts", "confusion_grid", "cam_raw", "cam_resize",
    "augment_affine", "disease_loss", "calib_fit", "reliability_bins", "clahe",
    "window16", "window_passes",
    "attention_relevance", "rollout_step", "token_relevance_step",
]


class _NoTimer:
    active = False


# bench.py installs a HIP-event timer here to measure the dense GEMM launches (C5 roofline):
# while it is `active`, timer(cost) is a context manager around each launch (_timed)
GEMM_TIMER = _NoTimer()


def attn_flash(T) -> bool:
    """The flash-style attention path (mmdx_attention_fwd_lse / _bwd_lse: row log-sum-exp
    saved, P recomputed in the backward) for the 16-bit compute dtypes; MMDX_ATTN_FLASH=0
    saves P [B,H,L,L] fp32 instead (the previous path, kept for A/B runs)."""
    return T != torch.float32 and os.environ.get("MMDX_ATTN_FLASH", "1") != "0"


def attention_fwd(qkv, mask, B, Ls, H, scale, p_drop, seed, counter, out, keep):
    """Self-attention forward of the eager per-layer nodes (BERT, ViT): returns what
    attention_bwd needs besides qkv / out — (lse, rng) on the flash-style path, (probs,)
    otherwise ((None,) when nothing is kept for a backward)."""
    T = qkv.dtype
    dev = qkv.device
    if keep and attn_flash(T):
        lse = torch.empty((B, H, Ls), dtype=torch.float32, device=dev)
        rng = torch.empty(1, dtype=torch.int64, device=dev)
        call("mmdx_attention_fwd_lse", L.dtype_code(T), ptr(qkv), ptr(mask), B, Ls, H,
             float(scale), float(p_drop), seed, ptr(counter), ptr(out), ptr(lse), ptr(rng),
             stream())
        return (lse, rng)
    probs = torch.empty((B, H, Ls, Ls), dtype=torch.float32, device=dev) if keep else None
    call("mmdx_attention_fwd", L.dtype_code(T), ptr(qkv), ptr(mask), B, Ls, H, float(scale),
         float(p_drop), seed, ptr(counter), ptr(out), ptr(probs), stream())
    return (probs,)


def attention_bwd(qkv, saved, out, dout, mask, B, Ls, H, scale, p_drop, dqkv):
    T = qkv.dtype
    dc = L.dtype_code(T)
    if len(saved) == 2:
        n = L.lib().mmdx_attention_lse_workspace_size(dc, B, Ls, H)
        w = torch.empty(max(1, n), dtype=torch.uint8, device=qkv.device)
        call("mmdx_attention_bwd_lse", dc, ptr(qkv), ptr(out), ptr(saved[0]), ptr(saved[1]),
             ptr(dout), ptr(mask), B, Ls, H, float(scale), float(p_drop), ptr(dqkv), ptr(w), n,
             stream())
        return
    n = L.lib().mmdx_attention_workspace_size(dc, B, Ls, H)
    w = torch.empty(max(1, n), dtype=torch.uint8, device=qkv.device)
    call("mmdx_attention_bwd", dc, ptr(qkv), ptr(saved[0]), ptr(dout), ptr(mask), B, Ls, H,
         float(scale), float(p_drop), ptr(dqkv), ptr(w), n, stream())


def gemm_cost(M, N, K, dt, c_dt, beta=0.0, act=L.ACT_NONE, preact=None):
    """LaunchCost of one GEMM: 2MNK FLOPs; A, B read once, C written (read too when
    beta != 0), the pre-activation written (GELU) or read (GELU backward)."""
    from .resnet import LaunchCost
    e = 4 if dt == L.F32 else 2
    ce = 4 if c_dt == L.F32 else 2
    b = (M * K + N * K) * e + M * N * ce * (2 if beta else 1)
    if preact is not None:
        b += M * N * ce
    return LaunchCost("gemm", 2 * M * N * K, b, f"{M}x{N}x{K}")


def _timed(cost, name, *args):
    """One dense-GEMM launch, between the timer's events while a timer is active (as the
    launch plans ask: plan._OpList.run); its cost record (gemm_cost's arguments) is built
    only then."""
    if getattr(GEMM_TIMER, "active", False):
        with GEMM_TIMER(gemm_cost(*cost)):
            call(name, *args)
    else:
        call(name, *args)


# ----------------------------------------------------------------------------- primitives
def gemm(A, lda, a_kmajor, B, ldb, b_kmajor, M, N, K, Cout, ldc, *, bias=None, addend=None,
         act=L.ACT_NONE, alpha=1.0, beta=0.0, preact=None, compute_dtype=None, residual=None):
    """C[M,N] = act(alpha * A.B^T + bias) + beta*C (+ residual) on the MFMA implicit-GEMM
    core."""
    dt = L.dtype_code(compute_dtype if compute_dtype is not None else A.dtype)
    ws_n = L.lib().mmdx_gemm_workspace_size(dt, M, N, K)
    ws = L.workspace(ws_n, Cout.device)
    c_dt = L.dtype_code(Cout.dtype)
    res = () if residual is None else (ptr(residual),)
    _timed((M, N, K, dt, c_dt, 1.0 if residual is not None else beta, act, preact),
           "mmdx_gemm_res" if res else "mmdx_gemm", dt, M, N, K, ptr(A), lda, int(a_kmajor),
           ptr(B), ldb, int(b_kmajor), ptr(Cout), ldc, c_dt, ptr(bias), ptr(addend), act,
           float(alpha), float(beta), ptr(preact), *res, ptr(ws), ws_n, stream())
    return Cout


def gemm_wgrad_bias(dY, ldy, X, ldx, M, N, K, dW, ldw, db, *, compute_dtype=None):
    """dW[M,N] = dY^T X (both R-major: dY [K][ldy], X [K][ldx]) and db[M] = column sums of
    dY, in one launch sequence (mmdx_gemm_bias_grad)."""
    dt = L.dtype_code(compute_dtype if compute_dtype is not None else dY.dtype)
    ws_n = L.lib().mmdx_gemm_bias_grad_workspace_size(dt, M, N, K)
    ws = L.workspace(ws_n, dW.device)
    c_dt = L.dtype_code(dW.dtype)
    _timed((M, N, K, dt, c_dt, 0.0, L.ACT_NONE, None), "mmdx_gemm_bias_grad", dt, M, N, K,
           ptr(dY), ldy, ptr(X), ldx, ptr(dW), ldw, c_dt, ptr(db), ptr(ws), ws_n, stream())
    return dW, db


def cast(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Device cast through the mmdx kernel (fp32 master weights -> compute dtype)."""
    if x.dtype == dtype:
        return x
    L.require_device(x)
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    call("mmdx_cast", L.dtype_code(dtype), L.dtype_code(x.dtype), ptr(x), x.numel(), ptr(y),
         stream())
    return y


def cat_cast(ws, T, device):
    """Concatenate fp32 tensors along dim 0 into one compute-dtype buffer (device casts)."""
    rows = sum(w.shape[0] for w in ws)
    out = torch.empty((rows,) + tuple(ws[0].shape[1:]), dtype=T, device=device)
    o = 0
    for w in ws:
        n = w.shape[0]
        call("mmdx_cast", L.dtype_code(T), L.F32, ptr(w), w.numel(), ptr(out[o:o + n]), stream())
        o += n
    return out


def add(x, y, out=None):
    out = torch.empty_like(x) if out is None else out
    call("mmdx_add", L.dtype_code(x.dtype), x.numel(), ptr(x), ptr(y), ptr(out), stream())
    return out


# Eager one-op wrappers: they allocate what they return; `out=` (the same tuple) writes into
# the caller's buffers instead.
def _f32(n, like):
    return torch.empty(n, dtype=torch.float32, device=like.device)


def ln_fwd(x, res, gamma, beta, eps, want_sum=True):
    """LayerNorm(x (+ res)) over the last dim -> (y, x + res or None, mean, rstd); the sum
    is what the backward reads (x itself when there is no residual)."""
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty_like(x)
    xs = torch.empty_like(x) if want_sum else None
    mean, rstd = _f32(rows, x), _f32(rows, x)
    call("mmdx_layernorm_fwd", L.dtype_code(x.dtype), ptr(x), ptr(res), rows, D, ptr(gamma),
         ptr(beta), float(eps), ptr(y), ptr(xs), ptr(mean), ptr(rstd), stream())
    return y, xs, mean, rstd


def ln_fwd_drop(x, res, gamma, beta, eps, p, seed):
    """LayerNorm(dropout(x) + res) in one pass -> (y, xsum, mean, rstd, rng); rng is the
    dropout stream base the backward redraws the keep bits from.  seed: L.dropout_seed's."""
    D = x.shape[-1]
    rows = x.numel() // D
    y, xs = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = _f32(rows, x), _f32(rows, x)
    rng = torch.empty(1, dtype=torch.int64, device=x.device)
    call("mmdx_layernorm_fwd_dropout", L.dtype_code(x.dtype), ptr(x), ptr(res), rows, D,
         ptr(gamma), ptr(beta), float(eps), float(p), seed, ptr(L.rng_counter(x.device)),
         ptr(y), ptr(xs), ptr(mean), ptr(rstd), ptr(rng), stream())
    return y, xs, mean, rstd, rng


def ln_bwd(xs, dy, gamma, mean, rstd, addin=None, out=None):
    """LayerNorm backward -> (dx, dgamma, dbeta); addin: a residual branch's gradient added
    to dx in the same pass (mmdx_layernorm_bwd_residual)."""
    D = xs.shape[-1]
    rows = xs.numel() // D
    dx, dg, db = out or (torch.empty_like(xs), _f32(D, xs), _f32(D, xs))
    n = L.lib().mmdx_layernorm_workspace_size(rows, D)
    w = L.workspace(n, xs.device)
    if addin is not None:
        call("mmdx_layernorm_bwd_residual", L.dtype_code(xs.dtype), ptr(xs), ptr(dy), rows, D,
             ptr(gamma), ptr(mean), ptr(rstd), ptr(addin), ptr(dx), ptr(dg), ptr(db), 0.0,
             ptr(w), n, stream())
    else:
        call("mmdx_layernorm_bwd", L.dtype_code(xs.dtype), ptr(xs), ptr(dy), rows, D,
             ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dg), ptr(db), 0.0, ptr(w), n,
             stream())
    return dx, dg, db


def ln_bwd_drop(xs, dy, gamma, mean, rstd, p, rng, out=None):
    """Backward of ln_fwd_drop -> (d xsum, its dropout backward, dgamma, dbeta)."""
    D = xs.shape[-1]
    rows = xs.numel() // D
    dx, dxd, dg, db = out or (torch.empty_like(xs), torch.empty_like(xs), _f32(D, xs),
                              _f32(D, xs))
    n = L.lib().mmdx_layernorm_workspace_size(rows, D)
    w = L.workspace(n, xs.device)
    call("mmdx_layernorm_bwd_dropout", L.dtype_code(xs.dtype), ptr(xs), ptr(dy), rows, D,
         ptr(gamma), ptr(mean), ptr(rstd), float(p), ptr(rng), ptr(dx), ptr(dxd), ptr(dg),
         ptr(db), 0.0, ptr(w), n, stream())
    return dx, dxd, dg, db


def dropout_fwd(x, p, seed, offset=0):
    """-> (dropped x, uint8 keep mask); seed: L.dropout_seed's.  The device counter
    (L.rng_counter) advances per launch."""
    y = torch.empty_like(x)
    mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    call("mmdx_dropout_fwd", L.dtype_code(x.dtype), ptr(x), x.numel(), float(p), seed, offset,
         ptr(L.rng_counter(x.device)), ptr(y), ptr(mask), stream())
    return y, mask


def dropout_bwd(dy, mask, p):
    dx = torch.empty_like(dy)
    call("mmdx_dropout_bwd", L.dtype_code(dy.dtype), ptr(dy), ptr(mask), dy.numel(), float(p),
         ptr(dx), stream())
    return dx


def _bias_grad(dy, M, N, out):
    ws_n = L.lib().mmdx_bias_grad_workspace_size(M, N)
    ws = L.workspace(ws_n, dy.device)
    call("mmdx_bias_grad", L.dtype_code(dy.dtype), ptr(dy), M, N, ptr(out), 0.0, ptr(ws), ws_n,
         stream())
    return out


def _gelu_bwd(pre, dy):
    dx = torch.empty_like(dy)
    call("mmdx_gelu_bwd", L.dtype_code(dy.dtype), ptr(pre), ptr(dy), dy.numel(), ptr(dx),
         stream())
    return dx


# ----------------------------------------------------------------------------- Linear
class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, act, out_dtype):
        L.require_device(x, w, b)
        M, K = x.shape
        N = w.shape[0]
        T = x.dtype
        wc = cast(w, T)
        y = torch.empty((M, N), dtype=out_dtype, device=x.device)
        pre = torch.empty((M, N), dtype=out_dtype, device=x.device) if act == L.ACT_GELU else None
        gemm(x, K, True, wc, K, True, M, N, K, y, N, bias=b, act=act, preact=pre,
             compute_dtype=T)
        ctx.save_for_backward(x, wc, pre if pre is not None else y)
        ctx.act, ctx.has_b, ctx.T = act, b is not None, T
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wc, saved = ctx.saved_tensors
        T = ctx.T
        M, K = x.shape
        N = wc.shape[0]
        dy = dy.contiguous()
        if ctx.act == L.ACT_GELU:
            dy = _gelu_bwd(saved, dy)
        elif ctx.act == L.ACT_RELU:
            raise NotImplementedError("relu epilogue backward is fused in the trunk, not here")
        dy = cast(dy, T)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((M, K), dtype=T, device=x.device)
            gemm(dy, N, True, wc, K, False, M, K, N, dx, K, compute_dtype=T)
        if ctx.needs_input_grad[1]:
            dw = torch.empty((N, K), dtype=torch.float32, device=x.device)
            gemm(dy, N, False, x, K, False, N, K, M, dw, K, compute_dtype=T)
        if ctx.has_b and ctx.needs_input_grad[2]:
            db = torch.empty((N,), dtype=torch.float32, device=x.device)
            _bias_grad(dy, M, N, db)
        return dx, dw, db, None, None


def linear(x, weight, bias=None, act=L.ACT_NONE, out_dtype=None):
    """y = act(x @ W^T + b); x in the compute dtype, W/b fp32 masters."""
    return _LinearFn.apply(x, weight, bias, act, out_dtype or x.dtype)


class _FusionLinearFn(torch.autograd.Function):
    """fusion_mlp[0] on cat([z_img, z_txt]) without materialising the concat (TP:586-589):
    y = act(z_img W[:, :Di]^T + z_txt W[:, Di:]^T + b) as two accumulating GEMMs."""

    @staticmethod
    def forward(ctx, za, zb, w, b, act):
        L.require_device(za, zb, w, b)
        M, Da = za.shape
        Db = zb.shape[1]
        N, Kt = w.shape
        assert Kt == Da + Db, "fusion weight must be [N, d_img + d_txt]"
        T = za.dtype
        wc = cast(w, T)
        y = torch.empty((M, N), dtype=T, device=za.device)
        pre = torch.empty((M, N), dtype=T, device=za.device) if act == L.ACT_GELU else None
        # acc = za Wa^T (fp32), then y = act(zb Wb^T + b + acc) in the second epilogue
        acc = torch.empty((M, N), dtype=torch.float32, device=za.device)
        gemm(za, Da, True, wc, Kt, True, M, N, Da, acc, N, compute_dtype=T)
        gemm(zb, Db, True, wc[:, Da:], Kt, True, M, N, Db, y, N, bias=b, addend=acc, act=act,
             preact=pre, compute_dtype=T)
        ctx.save_for_backward(za, zb, wc, pre if pre is not None else y)
        ctx.act, ctx.T, ctx.Da = act, T, Da
        return y

    @staticmethod
    def backward(ctx, dy):
        za, zb, wc, saved = ctx.saved_tensors
        T, Da = ctx.T, ctx.Da
        M, N = dy.shape
        Kt = wc.shape[1]
        Db = Kt - Da
        dy = dy.contiguous()
        if ctx.act == L.ACT_GELU:
            dy = _gelu_bwd(saved, dy)
        dy = cast(dy, T)
        dza = torch.empty((M, Da), dtype=T, device=dy.device)
        dzb = torch.empty((M, Db), dtype=T, device=dy.device)
        gemm(dy, N, True, wc, Kt, False, M, Da, N, dza, Da, compute_dtype=T)
        gemm(dy, N, True, wc[:, Da:], Kt, False, M, Db, N, dzb, Db, compute_dtype=T)
        dw = torch.empty((N, Kt), dtype=torch.float32, device=dy.device)
        gemm(dy, N, False, za, Da, False, N, Da, M, dw, Kt, compute_dtype=T)
        gemm(dy, N, False, zb, Db, False, N, Db, M, dw[:, Da:], Kt, compute_dtype=T)
        db = torch.empty((N,), dtype=torch.float32, device=dy.device)
        _bias_grad(dy, M, N, db)
        return dza, dzb, dw, db, None


def fusion_linear(z_img, z_txt, weight, bias, act=L.ACT_GELU):
    return _FusionLinearFn.apply(z_img, z_txt, weight, bias, act)


# ----------------------------------------------------------------------------- LayerNorm
class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, gamma, beta, eps):
        L.require_device(x, residual, gamma, beta)
        y, xs, mean, rstd = ln_fwd(x, residual, gamma, beta, eps)
        ctx.save_for_backward(xs, gamma, mean, rstd)
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        xs, gamma, mean, rstd = ctx.saved_tensors
        dx, dg, db = ln_bwd(xs, cast(dy.contiguous(), xs.dtype), gamma, mean, rstd)
        return dx, (dx if ctx.has_res else None), dg, db, None


def layer_norm(x, gamma, beta, eps, residual=None):
    return _LayerNormFn.apply(x, residual, gamma, beta, eps)


# ----------------------------------------------------------------------------- Dropout
_DROPOUT_SEED = [0x5EED]


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, offset):
        y, mask = dropout_fwd(x, p, seed, offset)
        ctx.save_for_backward(mask)
        ctx.p = p
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        return dropout_bwd(dy.contiguous(), mask, ctx.p), None, None, None


def dropout(x, p, training):
    if not training or p == 0.0:
        return x
    # the device counter (L.rng_counter) advances per launch; the host seed stays fixed so
    # the call is graph-replayable
    return _DropoutFn.apply(x, p, L.dropout_seed(_DROPOUT_SEED[0]), 0)


# ----------------------------------------------------------------------------- BCE
class _BCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        L.require_device(logits, target)
        if logits.dtype != torch.float32 or target.dtype != torch.float32:
            raise TypeError("BCEWithLogitsLoss kernel takes fp32 logits and targets")
        B, Cn = logits.shape
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        call("mmdx_bce_logits_fwd", ptr(logits), ptr(target), B, Cn, ptr(loss), stream())
        ctx.save_for_backward(logits, target)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, target = ctx.saved_tensors
        B, Cn = logits.shape
        dloss = dloss.contiguous().float()
        dz = torch.empty_like(logits)
        call("mmdx_bce_logits_bwd", ptr(logits), ptr(target), B, Cn, ptr(dloss), ptr(dz),
             stream())
        return dz, None


def bce_with_logits(logits, target):
    return _BCEFn.apply(logits.contiguous(), target.contiguous())


# ----------------------------------------------------------------------------- disease loss
class _DiseaseLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, pw, cw, gamma, eps, mean):
        B, Cn = logits.shape
        dev = logits.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        norm = torch.empty(1, dtype=torch.float32, device=dev)
        stats = torch.empty((Cn, 2), dtype=torch.float32, device=dev)
        want = ctx.needs_input_grad[0]
        g = torch.empty((B, Cn), dtype=torch.float32, device=dev) if want else None
        n = L.lib().mmdx_disease_loss_workspace_size(B, Cn)
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        call("mmdx_disease_loss_fwd", L.dtype_code(logits.dtype), ptr(logits), ptr(target), B,
             Cn, ptr(pw), ptr(cw), gamma, eps, int(mean), ptr(loss), ptr(stats), ptr(norm),
             ptr(g), ptr(ws), n, stream())
        if want:
            ctx.save_for_backward(g, norm)
        ctx.dt = logits.dtype
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        g, norm = ctx.saved_tensors
        dloss = dloss.contiguous().float()
        dz = torch.empty(g.shape, dtype=ctx.dt, device=g.device)
        call("mmdx_disease_loss_bwd", L.dtype_code(ctx.dt), ptr(g), g.numel(), ptr(dloss),
             ptr(norm), ptr(dz), stream())
        return dz, None, None, None, None, None, None


def disease_loss(logits, target, pos_weight=None, class_weight=None, gamma=0.0,
                 label_smoothing=0.0, reduction="mean"):
    """(loss, stats) of the weighted / masked / smoothed / focal BCE defined in mmdx.losses:
    logits [B, C] fp32, bf16 or fp16; target fp32 [B, C] with NaN = "no label"; pos_weight and
    class_weight fp32 [C] on the logits' device (or None).  stats [C, 2] (per-class loss sum and
    labelled count) stays on the device.  One forward launch; the backward scales the saved
    element gradient by the device scalars dloss / normaliser (no sync, GradScaler-safe) and
    rounds once to the logits' dtype.  Every argument is checked on the host first: ValueError /
    TypeError, never a copy behind the caller's back (a non-contiguous input is an error)."""
    from .losses import MAX_CLASSES, check_loss_args, check_weight
    gamma, eps = check_loss_args(gamma, label_smoothing, reduction)
    if not torch.is_tensor(logits) or not torch.is_tensor(target):
        raise TypeError("disease_loss: logits and target must be tensors")
    if logits.dim() != 2 or target.shape != logits.shape:
        raise ValueError(f"disease_loss: logits {tuple(logits.shape)} and target "
                         f"{tuple(target.shape)} must both be [B, C]")
    B, Cn = logits.shape
    if B < 1 or Cn < 1 or Cn > MAX_CLASSES or B * Cn > 2 ** 31 - 1:
        raise ValueError(f"disease_loss: [B, C] = [{B}, {Cn}] outside 1 <= C <= {MAX_CLASSES}, "
                         "1 <= B * C <= 2^31 - 1")
    check_weight("pos_weight", pos_weight, Cn)
    check_weight("class_weight", class_weight, Cn)
    if logits.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError(f"disease_loss: logits must be float32, bfloat16 or float16, got "
                        f"{logits.dtype}")
    if target.dtype != torch.float32:
        raise TypeError(f"disease_loss: target must be float32, got {target.dtype}")
    for name, t in (("logits", logits), ("target", target), ("pos_weight", pos_weight),
                    ("class_weight", class_weight)):
        if t is None:
            continue
        if not t.is_contiguous():
            raise ValueError(f"disease_loss: {name} is not contiguous (it is never copied here)")
        if not t.is_cuda or t.device != logits.device:
            raise ValueError(f"disease_loss: {name} is on {t.device}; every tensor must be on "
                             "the logits' GPU (there is no CPU path)")
    return _DiseaseLossFn.apply(logits, target, pos_weight, class_weight, gamma, eps,
                                reduction == "mean")


# ----------------------------------------------------------------------------- pooling
class _MaskedMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, mask):
        L.require_device(h, mask)
        B, Ls, D = h.shape
        out = torch.empty((B, D), dtype=h.dtype, device=h.device)
        call("mmdx_masked_mean_fwd", L.dtype_code(h.dtype), ptr(h), ptr(mask), B, Ls, D,
             ptr(out), stream())
        ctx.save_for_backward(mask)
        ctx.shape = (B, Ls, D)
        ctx.dt = h.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        (mask,) = ctx.saved_tensors
        B, Ls, D = ctx.shape
        dout = cast(dout.contiguous(), ctx.dt)
        dh = torch.empty((B, Ls, D), dtype=ctx.dt, device=dout.device)
        call("mmdx_masked_mean_bwd", L.dtype_code(ctx.dt), ptr(dout), ptr(mask), B, Ls, D,
             ptr(dh), stream())
        return dh, None


def masked_mean(h, mask):
    """TextEncoderTransformer.mean_pool (TP:452-459) with an int64 attention mask."""
    return _MaskedMeanFn.apply(h.contiguous(), mask.contiguous())


class _EmbedMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, mask, table, dt):
        L.require_device(ids, mask, table)
        B, Ls = ids.shape
        D = table.shape[1]
        out = torch.empty((B, D), dtype=dt, device=ids.device)
        call("mmdx_embed_mean_fwd", L.dtype_code(dt), ptr(ids), ptr(mask), B, Ls, D, ptr(table),
             ptr(out), stream())
        ctx.save_for_backward(ids, mask)
        ctx.tshape = table.shape
        ctx.dt = dt
        return out

    @staticmethod
    def backward(ctx, dout):
        ids, mask = ctx.saved_tensors
        B, Ls = ids.shape
        dout = cast(dout.contiguous(), ctx.dt)
        dtab = torch.zeros(ctx.tshape, dtype=torch.float32, device=dout.device)
        call("mmdx_embed_mean_bwd", L.dtype_code(ctx.dt), ptr(ids), ptr(mask), B, Ls,
             ctx.tshape[1], ptr(dout), ptr(dtab), stream())
        return None, None, dtab, None


def embed_mean(ids, mask, table, dt):
    return _EmbedMeanFn.apply(ids.contiguous(), mask.contiguous(), table, dt)


# ----------------------------------------------------------------------------- metrics
def _metric_inputs(name, scores, target):
    L.require_device(scores, target)
    if scores.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(f"{name} takes fp32 scores and targets")
    if scores.dim() != 2 or scores.shape != target.shape:
        raise ValueError(f"{name} takes scores and targets of one shape [N, C], got "
                         f"{tuple(scores.shape)} and {tuple(target.shape)}")
    return scores.shape


def auroc_counts(scores, target):
    """Pair counts of the AUROC of every class and of the flattened (micro) problem, from
    fp32 contiguous [N, C] scores and multi-hot targets (positive iff > 0.5): int64
    [(C + 1), 4] on the device, row c = (u2, n_pos, n_neg, n_nan), row C = micro
    (mmdx_auroc_pairs; mmdx.metrics.auroc_from_counts turns it into AUROC values on the host).
    Exact and bit-reproducible; all-pairs counting, so N * C <= 2^24 (and C <= 64).  The
    inputs are taken as they are: a non-contiguous tensor is an error, not a hidden copy."""
    N, C = _metric_inputs("auroc_counts", scores, target)
    out = torch.empty((C + 1, 4), dtype=torch.int64, device=scores.device)
    call("mmdx_auroc_pairs", ptr(scores), ptr(target), N, C, ptr(out), stream())
    return out


def confusion_grid(logits, target, thr):
    """(tp, fp), int64 [C, T] on the device: the positives / negatives of every class whose
    logit is >= thr[t], for a non-decreasing fp32 device vector thr [T] of LOGIT-space
    thresholds, 1 <= T <= 256 (mmdx_confusion_grid).  Sortedness is the caller's contract: it
    is not checked (that would be a device-to-host sync)."""
    N, C = _metric_inputs("confusion_grid", logits, target)
    L.require_device(thr)
    if thr.dtype != torch.float32 or thr.dim() != 1:
        raise TypeError("confusion_grid takes a 1-D fp32 threshold vector")
    T = thr.numel()
    tp = torch.empty((C, T), dtype=torch.int64, device=logits.device)
    fp = torch.empty((C, T), dtype=torch.int64, device=logits.device)
    call("mmdx_confusion_grid", ptr(logits), ptr(target), N, C, ptr(thr), T, ptr(tp), ptr(fp),
         stream())
    return tp, fp


# ----------------------------------------------------------------------------- calibration
def _calib_inputs(name, logits, target):
    """_metric_inputs with the errors of an argument check: TypeError / ValueError before any
    launch, never a hidden copy."""
    if not torch.is_tensor(logits) or not torch.is_tensor(target):
        raise TypeError(f"{name}: logits and target must be tensors")
    if logits.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(f"{name} takes fp32 logits and targets, got {logits.dtype} and "
                        f"{target.dtype}")
    if logits.dim() != 2 or logits.shape != target.shape:
        raise ValueError(f"{name} takes logits and targets of one shape [N, C], got "
                         f"{tuple(logits.shape)} and {tuple(target.shape)}")
    for what, t in (("logits", logits), ("target", target)):
        if not t.is_cuda or t.device != logits.device:
            raise ValueError(f"{name}: {what} is on {t.device}; every tensor must be on one GPU "
                             "(there is no CPU path)")
        if not t.is_contiguous():
            raise ValueError(f"{name}: {what} is not contiguous (it is never copied here)")
    return logits.shape


def calib_fit(logits, target, mode="platt", iters=32, smooth=True, min_count=1, tol=1e-7):
    """Fit the calibration map z' = a_c z + b_c of mmdx.calibration (mode "platt": per class;
    "temperature": one scalar a, b = 0) on fp32 contiguous [N, C] logits and targets (NaN
    target = no label) by damped Newton: iters + 1 launches of mmdx_calib_fit_step on the
    current stream, no host sync.  Returns device tensors (scale fp32 [C], bias fp32 [C],
    status int32 [C], info fp64 [C, 4]); scale / bias are the identity wherever status != 0
    (mmdx.calibration: the status codes; info = NLL at the identity, NLL at the result, Newton
    decrement per labelled element, labelled count).  iters = 0 evaluates the NLL at the
    identity.  Bit-reproducible.  C <= 64, N * C <= 2^31 - 1."""
    from .calibration import MAX_CLASSES, MODES, check_fit_args
    tol = check_fit_args(mode, iters, min_count, tol)
    N, C = _calib_inputs("calib_fit", logits, target)
    if N < 1 or C < 1 or C > MAX_CLASSES or N * C > 2 ** 31 - 1:
        raise ValueError(f"calib_fit: [N, C] = [{N}, {C}] outside 1 <= C <= {MAX_CLASSES}, "
                         "1 <= N * C <= 2^31 - 1")
    dev = logits.device
    # the label counts of Platt's targets and of the min_count rule: torch ops, no sync
    lab = ~torch.isnan(target)
    n_lab = lab.sum(0, dtype=torch.float64)
    n_pos = torch.where(lab, target, target.new_zeros(())).sum(0, dtype=torch.float64)
    counts = torch.stack([n_pos, n_lab - n_pos], dim=1).contiguous()
    scale = torch.empty(C, dtype=torch.float32, device=dev)
    bias = torch.empty(C, dtype=torch.float32, device=dev)
    status = torch.empty(C, dtype=torch.int32, device=dev)
    info = torch.empty((C, 4), dtype=torch.float64, device=dev)
    n = L.lib().mmdx_calib_fit_workspace_size(N, C)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    code = MODES.index(mode)
    st = stream()
    for k in range(iters + 1):
        call("mmdx_calib_fit_step", ptr(logits), ptr(target), N, C, ptr(counts), int(bool(smooth)),
             code, k, int(k == iters), min_count, tol, ptr(scale), ptr(bias), ptr(status),
             ptr(info), ptr(ws), n, st)
    return scale, bias, status, info


def reliability_bins(logits, target, scale=None, bias=None, n_bins=15):
    """(bins, n_nan) of a reliability diagram with n_bins equal-width probability bins, from fp32
    contiguous [N, C] logits and targets (positive iff > 0.5), optionally after the calibration
    map z' = z * scale + bias (fp32 [C] device tensors, both or neither).  bins int64
    [(C + 1), n_bins, 4] = (count, positives, sum round(p 2^30), sum round((p - y)^2 2^30)),
    n_nan int64 [(C + 1)] the dropped NaN logits; row C is micro (mmdx_reliability_bins;
    mmdx.calibration.calibration_from_bins turns them into ECE / MCE / Brier on the host).
    Exact counts, bit-reproducible.  N * C <= 2^24, C <= 64, 1 <= n_bins <= 64."""
    from .calibration import MAX_CLASSES, bin_edges
    edges_host = bin_edges(n_bins)
    N, C = _calib_inputs("reliability_bins", logits, target)
    if N < 1 or C < 1 or C > MAX_CLASSES or N * C > 2 ** 24:
        raise ValueError(f"reliability_bins: [N, C] = [{N}, {C}] outside 1 <= C <= "
                         f"{MAX_CLASSES}, 1 <= N * C <= 2^24")
    if (scale is None) != (bias is None):
        raise ValueError("reliability_bins: scale and bias come together")
    for what, t in (("scale", scale), ("bias", bias)):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise TypeError(f"reliability_bins: {what} must be an fp32 tensor")
        if t.shape != (C,) or not t.is_contiguous():
            raise ValueError(f"reliability_bins: {what} must be contiguous [{C}], got "
                             f"{tuple(t.shape)}")
        if t.device != logits.device:
            raise ValueError(f"reliability_bins: {what} is on {t.device}, the logits on "
                             f"{logits.device}")
    edges = torch.from_numpy(edges_host).to(logits.device) if n_bins > 1 else None
    out = torch.empty((C + 1) * n_bins * 4 + (C + 1), dtype=torch.int64, device=logits.device)
    call("mmdx_reliability_bins", ptr(logits), ptr(target), N, C, ptr(scale), ptr(bias),
         ptr(edges), n_bins, ptr(out), stream())
    return out[:(C + 1) * n_bins * 4].view(C + 1, n_bins, 4), out[(C + 1) * n_bins * 4:]


# ----------------------------------------------------------------------------- bootstrap
def bootstrap_weights(R, N, seed, r0=0, device=None):
    """int32 [R, N] on `device`: the resampling weights of bootstrap replicates r0 ... r0 + R - 1
    (mmdx_bootstrap_weights; mmdx.bootstrap.reference_weights is the numpy statement).  Every
    row sums to N.  Draw k of replicate r depends on (seed, r, k, N) alone, so a run split into
    batches with r0 equals the unsplit one.  Bit-reproducible.  R * N <= 2^26."""
    from .bootstrap import MAX_WEIGHTS
    for what, v in (("R", R), ("N", N), ("seed", seed), ("r0", r0)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"bootstrap_weights: {what} must be an int, got {type(v).__name__}")
    if R < 1 or N < 1 or r0 < 0 or R * N > MAX_WEIGHTS or r0 + R >= 2 ** 62:
        raise ValueError(f"bootstrap_weights: R = {R}, N = {N}, r0 = {r0} outside R, N >= 1, "
                         "r0 >= 0, R * N <= 2^26")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ValueError(f"bootstrap_weights: device {device} is not a GPU (there is no CPU path)")
    w = torch.empty((R, N), dtype=torch.int32, device=device)
    with torch.cuda.device(w.device):
        call("mmdx_bootstrap_weights", R, r0, N, seed & 0xFFFFFFFFFFFFFFFF, ptr(w), stream())
    return w


def _boot_items(key, flags, n_pad):
    """int32 [2, cols, n_pad] from key fp32 / flags int32 [n, cols]: per column the items
    (row << 3) | flags in ascending key order, positives first within ties ([0]) and negatives
    first ([1]), zero-padded.  Two stable sorts each: by label, then by key."""
    n, cols = key.shape
    out = torch.zeros((2, cols, n_pad), dtype=torch.int32, device=key.device)
    neg = 1 - (flags & 1)
    for o, first in enumerate((neg, 1 - neg)):          # the label that goes first sorts as 0
        p1 = torch.sort(first.to(torch.uint8), dim=0, stable=True)[1]
        p2 = torch.sort(torch.gather(key, 0, p1), dim=0, stable=True)[1]
        row = torch.gather(p1, 0, p2)
        item = (row << 3) | torch.gather(flags, 0, row).to(torch.int64)
        out[o, :, :n] = item.t().to(torch.int32)
    return out


def bootstrap_plan(scores, target, pred=None):
    """Everything of the bootstrap that does not depend on the replicate: the sorted orders and
    the per-element flags, from fp32 contiguous [N, C] scores and targets (positive iff > 0.5;
    a NaN score drops the element) and an optional bool [N, C] `pred` (the elements predicted
    positive, for tp / fp).  torch sorts and elementwise ops on the device, done once; no host
    sync.  Returns an opaque tuple for bootstrap_counts.  1 <= C <= 64, N * C <= 2^24."""
    from .bootstrap import MAX_CLASSES, MAX_ITEMS
    N, C = _calib_inputs("bootstrap_plan", scores, target)
    if N < 1 or C < 1 or C > MAX_CLASSES or N * C > MAX_ITEMS:
        raise ValueError(f"bootstrap_plan: [N, C] = [{N}, {C}] outside 1 <= C <= {MAX_CLASSES}, "
                         "1 <= N * C <= 2^24")
    if pred is not None:
        if not torch.is_tensor(pred) or pred.dtype != torch.bool:
            raise TypeError("bootstrap_plan: pred must be a bool tensor")
        if pred.shape != scores.shape or pred.device != scores.device:
            raise ValueError(f"bootstrap_plan: pred {tuple(pred.shape)} on {pred.device} for "
                             f"scores {tuple(scores.shape)} on {scores.device}")
    flags = (target > 0.5).to(torch.int32) | ((~torch.isnan(scores)).to(torch.int32) << 1)
    if pred is not None:
        flags = flags | (pred.to(torch.int32) << 2)
    key = scores + 0.0   # -0.0 becomes +0.0: the two tie under any sort
    class_items = _boot_items(key, flags, (N + 3) & ~3)
    # the micro column sorts all N * C elements; an element's weight row is element // C
    m = N * C
    micro = _boot_items(key.reshape(m, 1), flags.reshape(m, 1), (m + 3) & ~3)[:, 0]
    e = micro >> 3
    micro = torch.where(torch.arange(micro.shape[1], device=micro.device) < m,
                        (torch.div(e, C, rounding_mode="floor") << 3) | (micro & 7),
                        torch.zeros_like(micro))
    return class_items, micro.contiguous(), N, C


def bootstrap_counts(plan, weights, out=None):
    """int64 [R, C + 1, 5] = (u2, w_pos, w_neg, tp, fp) per replicate and class, row C micro
    (mmdx_bootstrap_counts; mmdx.bootstrap: the definition, reference_counts and intervals),
    from a bootstrap_plan and non-negative contiguous int32 [R, N] weights on the plan's device
    (bootstrap_weights, or any multiplicities whose rows sum to at most 2^31 / C; neither is
    checked: that would be a host sync).  A weighted prefix scan over the plan's shared sort:
    exact integers, bit-reproducible.  `out` (int64 contiguous [R, C + 1, 5]) is filled in
    place when given.  R * N <= 2^26."""
    from .bootstrap import MAX_WEIGHTS
    try:
        class_items, micro_items, N, C = plan
    except (TypeError, ValueError):
        raise TypeError("bootstrap_counts: plan must come from bootstrap_plan") from None
    if not torch.is_tensor(weights) or weights.dtype != torch.int32:
        raise TypeError("bootstrap_counts takes int32 weights")
    if weights.dim() != 2 or weights.shape[1] != N or weights.shape[0] < 1:
        raise ValueError(f"bootstrap_counts: weights {tuple(weights.shape)} for a plan of "
                         f"{N} rows: [R, {N}] expected")
    R = weights.shape[0]
    if R * N > MAX_WEIGHTS:
        raise ValueError(f"bootstrap_counts: R * N = {R * N} exceeds 2^26: split the replicates")
    if weights.device != class_items.device:
        raise ValueError(f"bootstrap_counts: weights on {weights.device}, the plan on "
                         f"{class_items.device}")
    if not weights.is_contiguous():
        raise ValueError("bootstrap_counts: weights are not contiguous (never copied here)")
    if out is None:
        out = torch.empty((R, C + 1, 5), dtype=torch.int64, device=weights.device)
    elif (not torch.is_tensor(out) or out.dtype != torch.int64 or out.shape != (R, C + 1, 5)
          or out.device != weights.device or not out.is_contiguous()):
        raise ValueError(f"bootstrap_counts: out must be contiguous int64 [{R}, {C + 1}, 5] on "
                         f"{weights.device}")
    n = L.lib().mmdx_bootstrap_counts_workspace_size(R, N, C)
    ws = torch.empty(n, dtype=torch.uint8, device=weights.device)
    call("mmdx_bootstrap_counts", ptr(class_items), ptr(micro_items), ptr(weights), R, N, C,
         ptr(out), ptr(ws), n, stream())
    return out


# ----------------------------------------------------------------------------- Grad-CAM
def cam_raw(fmap, alpha):
    """raw[b, c, h, w] = relu(sum_k alpha[b, c, k] * fmap[b, h, w, k]), fp32 [B, C, H, W], from
    the NHWC feature map fmap [B, H, W, K] (fp32, bf16 or fp16) and the fp32 channel weights
    alpha [B, C, K] (mmdx_cam_fwd: fp32 accumulation, bit-reproducible).  K % 8 == 0, C <= 64,
    H * W <= 1024.  The inputs are taken as they are: a non-contiguous tensor is an error."""
    L.require_device(fmap, alpha)
    if alpha.dtype != torch.float32:
        raise TypeError("cam_raw takes fp32 channel weights (alpha)")
    dt = L.dtype_code(fmap.dtype)
    if fmap.dim() != 4 or alpha.dim() != 3 or alpha.shape[0] != fmap.shape[0] or \
            alpha.shape[2] != fmap.shape[3]:
        raise ValueError(f"cam_raw takes fmap [B, H, W, K] and alpha [B, C, K], got "
                         f"{tuple(fmap.shape)} and {tuple(alpha.shape)}")
    B, H, W, K = fmap.shape
    C = alpha.shape[1]
    raw = torch.empty((B, C, H, W), dtype=torch.float32, device=fmap.device)
    call("mmdx_cam_fwd", dt, ptr(fmap), ptr(alpha), B, H * W, K, C, ptr(raw), stream())
    return raw


def cam_resize(raw, out_size, normalize=True):
    """Bilinear resize (half-pixel centres, as torch's interpolate with align_corners=False) of
    the fp32 maps raw [..., H, W] to [..., Ho, Wo]; normalize=True first divides every map by
    its own maximum, an all-zero map staying all zero (mmdx_cam_resize).  H * W <= 1024,
    Ho, Wo <= 4096."""
    L.require_device(raw)
    if raw.dtype != torch.float32:
        raise TypeError("cam_resize takes fp32 maps")
    if raw.dim() < 2:
        raise ValueError(f"cam_resize takes maps [..., H, W], got {tuple(raw.shape)}")
    Ho, Wo = (int(v) for v in out_size)
    H, W = raw.shape[-2:]
    out = torch.empty((*raw.shape[:-2], Ho, Wo), dtype=torch.float32, device=raw.device)
    call("mmdx_cam_resize", ptr(raw), raw.numel() // (H * W) if H * W else 0, H, W, Ho, Wo,
         int(bool(normalize)), ptr(out), stream())
    return out


# ----------------------------------------------------------------------------- ViT explanations
ATTN_REL_MAX_L, ATTN_REL_MAX_H, ATTN_REL_HD, ROLLOUT_MAX_L = 256, 16, 64, 4096


def _shares_memory(a, b):
    """Whether the storage ranges of two contiguous tensors overlap (host arithmetic only)."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _f32_out(name, out, shape, *inputs):
    """The operands of an explanation wrapper checked for layout, aliasing and device (in this
    order, so that everything but the device can be checked on the host), then `out`: the
    caller's, or a new fp32 tensor."""
    for i, t in enumerate(inputs):
        if not t.is_contiguous():
            raise ValueError(f"{name}: operand {i} is not contiguous (never copied here)")
    if out is not None:
        if (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != shape
                or not out.is_contiguous()):
            raise ValueError(f"{name}: out must be contiguous fp32 {list(shape)}")
        if any(_shares_memory(out, t) for t in inputs):
            raise ValueError(f"{name}: out shares memory with an input")
    for t in (*inputs, *(() if out is None else (out,))):
        if not t.is_cuda or t.device != inputs[0].device:
            raise ValueError(f"{name}: an operand is on {t.device}; the kernel runs on the GPU, "
                             f"all operands on one device")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=inputs[0].device)
    return out


def attention_relevance(qkv, B, Ls, H, scale, dout=None, out=None):
    """The head-averaged attention map [B, Ls, Ls] fp32 of one block, recomputed from its qkv
    buffer [B * Ls, 3, H, 64] (fp32, bf16 or fp16; any shape of B * Ls * 3 * H * 64 elements in
    that order, e.g. the block's [B * Ls, 3 * H * 64]) by mmdx_attention_relevance:
    P_h = softmax(scale Q_h K_h^T), no key mask.  dout=None: mean_h P_h (rows sum to 1).
    dout [B * Ls, H, 64] in qkv's dtype, the gradient of a scalar with respect to the attention
    core's output: mean_h relu(P_h * dP_h) with dP_h = dO_h V_h^T.  fp32 accumulation, the heads
    summed in order, bit-reproducible.  1 <= Ls <= 256, 1 <= H <= 16.  A wrong dtype is a
    TypeError; a wrong shape, device or layout, a limit exceeded or an `out` that shares memory
    with an input is a ValueError; nothing is copied or launched then."""
    name = "attention_relevance"
    if not torch.is_tensor(qkv) or (dout is not None and not torch.is_tensor(dout)):
        raise TypeError(f"{name} takes tensors")
    dt = L.dtype_code(qkv.dtype)
    if dout is not None and dout.dtype != qkv.dtype:
        raise TypeError(f"{name}: dout is {dout.dtype}, qkv {qkv.dtype}")
    B, Ls, H = int(B), int(Ls), int(H)
    if B < 1 or not 1 <= Ls <= ATTN_REL_MAX_L or not 1 <= H <= ATTN_REL_MAX_H:
        raise ValueError(f"{name}: B = {B}, Ls = {Ls}, H = {H} outside B >= 1, 1 <= Ls <= "
                         f"{ATTN_REL_MAX_L}, 1 <= H <= {ATTN_REL_MAX_H}")
    if not np.isfinite(float(scale)):
        raise ValueError(f"{name}: scale = {scale}")
    if qkv.numel() != B * Ls * 3 * H * ATTN_REL_HD:
        raise ValueError(f"{name}: qkv {tuple(qkv.shape)} is not [{B * Ls}, 3, {H}, "
                         f"{ATTN_REL_HD}]")
    if dout is not None and dout.numel() != B * Ls * H * ATTN_REL_HD:
        raise ValueError(f"{name}: dout {tuple(dout.shape)} is not [{B * Ls}, {H}, "
                         f"{ATTN_REL_HD}]")
    out = _f32_out(name, out, (B, Ls, Ls), qkv, *(() if dout is None else (dout,)))
    call("mmdx_attention_relevance", dt, ptr(qkv), ptr(dout), B, Ls, H, float(scale), ptr(out),
         stream())
    return out


def rollout_step(r, abar, alpha, beta, out=None):
    """One layer of the class-token recursion: out[b, j] = alpha r[b, j] + beta sum_i r[b, i]
    abar[b, i, j], fp32, r [B, Ls], abar [B, Ls, Ls] (mmdx_rollout_step: i summed in ascending
    order, bit-reproducible).  (alpha, beta) = (a, 1 - a): attention rollout with residual a;
    (1, 1): the relevance recursion.  `out` must not share memory with r or abar.  Errors as
    attention_relevance."""
    name = "rollout_step"
    if not torch.is_tensor(r) or not torch.is_tensor(abar):
        raise TypeError(f"{name} takes tensors")
    if r.dtype != torch.float32 or abar.dtype != torch.float32:
        raise TypeError(f"{name} takes fp32 tensors, got {r.dtype} and {abar.dtype}")
    if r.dim() != 2 or abar.dim() != 3 or tuple(abar.shape) != (*r.shape, r.shape[1]) or \
            r.numel() == 0:
        raise ValueError(f"{name} takes r [B, Ls] and abar [B, Ls, Ls], got {tuple(r.shape)} "
                         f"and {tuple(abar.shape)}")
    B, Ls = r.shape
    if Ls > ROLLOUT_MAX_L:
        raise ValueError(f"{name}: Ls = {Ls} > {ROLLOUT_MAX_L}")
    if not (np.isfinite(float(alpha)) and np.isfinite(float(beta))):
        raise ValueError(f"{name}: alpha = {alpha}, beta = {beta}")
    out = _f32_out(name, out, (B, Ls), r, abar)
    call("mmdx_rollout_step", ptr(r), ptr(abar), B, Ls, float(alpha), float(beta), ptr(out),
         stream())
    return out


# ----------------------------------------------------------------------------- text explanations
# token_relevance_step's workspace per (device, stream, B): the kernel needs the B counters at
# its head zero before the first launch and leaves them zero, so one zero-filled buffer serves
# every later call of that batch size on that stream and the call itself stays a single launch.
# (Another B moves the boundary between the counters and the partial rows: a buffer of its own.)
_TOKEN_WS: dict = {}


def _token_workspace(B, Ls, dev):
    n = L.lib().mmdx_token_relevance_workspace_size(B, Ls)
    if n == 0:
        return None, 0
    key = (dev.index, stream(), B)
    w = _TOKEN_WS.get(key)
    if w is None or w.numel() < n:
        w = _TOKEN_WS[key] = torch.zeros(n, dtype=torch.uint8, device=dev)
    return w, w.numel()


def token_relevance_step(r, qkv, B, Ls, H, scale, alpha, beta, mask=None, dout=None, out=None):
    """One layer of the relevance recursion for the row vector r [B, Ls] fp32, fused with the
    recomputation of the attention probabilities from the layer's qkv buffer [B * Ls, 3, H, 64]
    (fp32, bf16 or fp16, as attention_relevance takes it) in one launch that never writes the
    [Ls, Ls] map (mmdx_token_relevance_step):

        out[b, j] = alpha r[b, j] + beta sum_i r[b, i] abar[b, i, j]

    with abar = mean_h P_h (dout=None) or mean_h relu(P_h * dP_h), dP_h = dO_h V_h^T (dout
    [B * Ls, H, 64] in qkv's dtype), and P_h the softmax over the REAL keys: mask int64 [B, Ls],
    1 = a real token (None: all real), the tensor the attention forward takes.  A masked key's
    probability is exactly 0, so a masked column comes out as alpha r exactly; a sample without
    a real key gives alpha r.  Bit-reproducible, row b independent of B.  1 <= Ls <= 256,
    1 <= H <= 16.  A wrong dtype is a TypeError; a wrong shape, device or layout, a limit
    exceeded, a non-finite scalar or an `out` that shares memory with an input is a ValueError;
    nothing is copied or launched then."""
    name = "token_relevance_step"
    ops = (r, qkv) + tuple(t for t in (mask, dout) if t is not None)
    if not all(torch.is_tensor(t) for t in ops):
        raise TypeError(f"{name} takes tensors")
    dt = L.dtype_code(qkv.dtype)
    if r.dtype != torch.float32:
        raise TypeError(f"{name}: r is {r.dtype}, not fp32")
    if dout is not None and dout.dtype != qkv.dtype:
        raise TypeError(f"{name}: dout is {dout.dtype}, qkv {qkv.dtype}")
    if mask is not None and mask.dtype != torch.int64:
        raise TypeError(f"{name}: mask is {mask.dtype}, not int64")
    B, Ls, H = int(B), int(Ls), int(H)
    if B < 1 or not 1 <= Ls <= ATTN_REL_MAX_L or not 1 <= H <= ATTN_REL_MAX_H:
        raise ValueError(f"{name}: B = {B}, Ls = {Ls}, H = {H} outside B >= 1, 1 <= Ls <= "
                         f"{ATTN_REL_MAX_L}, 1 <= H <= {ATTN_REL_MAX_H}")
    if not all(np.isfinite(float(v)) for v in (scale, alpha, beta)):
        raise ValueError(f"{name}: scale = {scale}, alpha = {alpha}, beta = {beta}")
    if tuple(r.shape) != (B, Ls):
        raise ValueError(f"{name}: r {tuple(r.shape)} is not [{B}, {Ls}]")
    if mask is not None and tuple(mask.shape) != (B, Ls):
        raise ValueError(f"{name}: mask {tuple(mask.shape)} is not [{B}, {Ls}]")
    if qkv.numel() != B * Ls * 3 * H * ATTN_REL_HD:
        raise ValueError(f"{name}: qkv {tuple(qkv.shape)} is not [{B * Ls}, 3, {H}, "
                         f"{ATTN_REL_HD}]")
    if dout is not None and dout.numel() != B * Ls * H * ATTN_REL_HD:
        raise ValueError(f"{name}: dout {tuple(dout.shape)} is not [{B * Ls}, {H}, "
                         f"{ATTN_REL_HD}]")
    out = _f32_out(name, out, (B, Ls), *ops)
    ws, n = _token_workspace(B, Ls, r.device)
    call("mmdx_token_relevance_step", dt, ptr(qkv), ptr(dout), ptr(mask), ptr(r), B, Ls, H,
         float(scale), float(alpha), float(beta), ptr(out), ptr(ws), n, stream())
    return out


# ----------------------------------------------------------------------------- augmentation
def augment_affine(x, params, mean=None, std=None, clamp=True, out=None):
    """Per-image affine warp (bilinear, black outside) + contrast / brightness of the
    normalised fp32 NCHW batch x [B, C, H, W], in one launch (mmdx_augment_affine; the
    semantics are those of mmdx.augment, whose `reference` is the CPU statement of them).
    params: CPU [B, 8] fp32 tensor or ndarray, row = (a00, a01, ox, a10, a11, oy, gain, delta),
    validated on the host (augment.check_params) and then uploaded.  mean / std: the
    normalisation x carries (default: preprocess_batch's ImageNet constants).  clamp=False
    skips the clamp to the normalised [0, 1] pixel range.  Returns `out` (a new tensor unless
    given), which must not share memory with x.  C <= 4, H, W <= 4096, B <= 65535.  A wrong
    dtype, layout, shape or an aliasing `out` is a ValueError, never a hidden copy."""
    import ctypes
    from . import augment as A
    if x.dtype != torch.float32:
        raise ValueError(f"augment_affine takes fp32 images, got {x.dtype}")
    if x.dim() != 4:
        raise ValueError(f"augment_affine takes [B, C, H, W], got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError("augment_affine takes a contiguous NCHW tensor")
    B, C, H, W = x.shape
    if not (1 <= C <= A.MAX_C and 1 <= H <= A.MAX_HW and 1 <= W <= A.MAX_HW
            and 1 <= B <= A.MAX_B):
        raise ValueError(f"augment_affine: shape {tuple(x.shape)} outside 1 <= B <= {A.MAX_B}, "
                         f"C <= {A.MAX_C}, H, W <= {A.MAX_HW}")
    if out is not None:
        if out.dtype != torch.float32 or out.shape != x.shape or not out.is_contiguous() or \
                out.device != x.device:
            raise ValueError("augment_affine: out must be a contiguous fp32 tensor of x's shape "
                             "on x's device")
        nbytes = x.numel() * 4
        if out.data_ptr() < x.data_ptr() + nbytes and x.data_ptr() < out.data_ptr() + nbytes:
            raise ValueError("augment_affine: out must not alias x (the warp is a gather)")
    rows = A.check_params(params, B)
    m, s = A.norm_constants(C, mean, std)
    L.require_device(x)
    if out is None:
        out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        d_rows = torch.from_numpy(rows).to(x.device)
        call("mmdx_augment_affine", ptr(x), ptr(d_rows), B, C, H, W,
             (ctypes.c_float * C)(*m.tolist()), (ctypes.c_float * C)(*s.tolist()),
             int(bool(clamp)), ptr(out), stream())
    return out


# ----------------------------------------------------------------------------- CLAHE
def clahe_passes(px, descs, lut_bytes):
    """The two CLAHE launches (mmdx_clahe_luts, mmdx_clahe_apply) on the packed device pixel
    buffer `px` that the table `descs` of clahe.plan describes: returns (equalised buffer of
    the same layout, LUT buffer).  The C entries validate the table against the buffers before
    they launch; nothing here copies pixels or synchronises."""
    from . import clahe as K
    if px.dtype != torch.uint8 or px.dim() != 1 or not px.is_contiguous():
        raise ValueError("clahe: the pixel buffer must be a flat contiguous uint8 tensor")
    L.require_device(px)
    if call("mmdx_clahe_desc_size") != K.DESC.itemsize:
        raise RuntimeError("mmdx_clahe_desc layout differs between the library and clahe.DESC")
    B, total = len(descs), px.numel()
    with torch.cuda.device(px.device):
        d_desc = torch.from_numpy(descs.view(np.uint8).copy()).to(px.device, non_blocking=True)
        luts = torch.empty(lut_bytes, dtype=torch.uint8, device=px.device)
        out = torch.empty_like(px)
        call("mmdx_clahe_luts", ptr(px), total, descs.ctypes.data, ptr(d_desc), B, ptr(luts),
             lut_bytes, stream())
        call("mmdx_clahe_apply", ptr(px), total, descs.ctypes.data, ptr(d_desc), B, ptr(luts),
             lut_bytes, ptr(out), total, stream())
    return out, luts


def clahe(images, clip_limit=2.0, tiles=(8, 8), return_luts=False, device=None):
    """CLAHE (mmdx.clahe: the definition and its numpy `reference`, which this equals byte for
    byte) of a list of HxW / HxWx{1,3} uint8 arrays or PIL L / RGB images of any sizes, in two
    launches for the whole list.  Returns a list of device uint8 tensors of the inputs' shapes,
    and with return_luts also a list of the uint8 LUTs, [ty, tx, 256] for an HxW input and
    [C, ty, tx, 256] otherwise.  Limits (TypeError / ValueError before any launch): uint8 only,
    C in {1, 3}, 1 <= tx, ty <= 16, W >= 2 tx, H >= 2 ty, tile area <= 2^24, sides <= 65535,
    clip_limit finite."""
    from . import clahe as K
    setting = K.Clahe(clip_limit, tiles)
    if isinstance(images, (np.ndarray, torch.Tensor)) or hasattr(images, "mode"):
        raise TypeError("clahe takes a list of images")
    shapes = [np.asarray(im).shape for im in images]
    arrays = [K.as_planes(im) for im in images]
    descs, total, lut_bytes = K.plan(arrays, setting)   # every limit, before any upload
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("functional.clahe runs on the GPU (HIP); mmdx.clahe.reference is "
                           "the host statement")
    host = np.concatenate([a.reshape(-1) for a in arrays])
    with torch.cuda.device(device):
        out, luts = clahe_passes(torch.from_numpy(host).to(device), descs, lut_bytes)
    tx, ty = setting.tiles
    res, tabs = [], []
    for d, a, shp in zip(descs, arrays, shapes):
        h, w, c = a.shape
        o, lo = int(d["dst_off"]), int(d["lut_off"])
        res.append(out[o:o + h * w * c].view(shp))
        t = luts[lo:lo + c * ty * tx * 256].view(c, ty, tx, 256)
        tabs.append(t[0] if len(shp) == 2 else t)
    return (res, tabs) if return_luts else res


# ----------------------------------------------------------------------------- 16-bit windowing
_WINDOW_WS: dict = {}


def _window_workspace(B, device):
    """The histogram workspace of mmdx_window_levels for (device, current stream): allocated
    zeroed once (a memset on the stream) and left zero by every call, so it is reused without
    a reset; it grows when a larger batch comes."""
    need = call("mmdx_window_workspace_size", B)
    if need == 0:
        raise ValueError(f"window: a batch of {B} images is outside the limits")
    key = (device.index, stream())
    ws = _WINDOW_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _WINDOW_WS[key] = torch.zeros(need, dtype=torch.uint8, device=device)
    return ws


def window_passes(px16, descs):
    """The window launches (mmdx_window_levels in percentile mode, then mmdx_window_apply) on
    the packed device buffer `px16` of 16-bit pixels that the table `descs` of window.plan
    describes (a flat uint8 tensor of its bytes, or a flat int16 / uint16 one).  Returns (the
    packed uint8 buffer in the (H, W, 1) layout of clahe.plan and preprocess.plan_batch, the
    [B, 2] int32 windows (lo, hi) on the device; None in fixed mode, where the window is the
    setting's).  The C entries validate the table against the buffers before they launch;
    nothing here copies pixels or synchronises."""
    from . import window as W
    if px16.dim() != 1 or not px16.is_contiguous() or px16.element_size() not in (1, 2) or \
            px16.is_floating_point():
        raise ValueError("window: the pixel buffer must be a flat contiguous tensor of the "
                         "16-bit pixels (uint8 bytes, int16 or uint16)")
    L.require_device(px16)
    if call("mmdx_window_desc_size") != W.DESC.itemsize:
        raise RuntimeError("mmdx_window_desc layout differs between the library and window.DESC")
    B, src_bytes = len(descs), px16.numel() * px16.element_size()
    out_bytes = int(descs["dst_off"][-1]) + int(descs["w"][-1]) * int(descs["h"][-1])
    percentile = bool((descs["mode"] == 0).all())
    with torch.cuda.device(px16.device):
        d_desc = torch.from_numpy(descs.view(np.uint8).copy()).to(px16.device, non_blocking=True)
        out = torch.empty(out_bytes, dtype=torch.uint8, device=px16.device)
        levels = None
        if percentile:
            ws = _window_workspace(B, px16.device)
            levels = torch.empty((B, 4), dtype=torch.int32, device=px16.device)
            call("mmdx_window_levels", ptr(px16), src_bytes, descs.ctypes.data, ptr(d_desc), B,
                 ptr(ws), ws.numel(), ptr(levels), stream())
        call("mmdx_window_apply", ptr(px16), src_bytes, descs.ctypes.data, ptr(d_desc), B,
             ptr(levels), ptr(out), out_bytes, stream())
    return out, (levels[:, :2] if percentile else None)


def window16(images, window, return_window=False, device=None):
    """Windowing of 16-bit images to 8 bits (mmdx.window: the definition and its numpy
    `reference`, which this equals byte for byte) for a list of HxW / HxWx1 uint16 arrays or
    PIL I;16 images of any sizes, in three launches for the whole list (one in fixed mode).
    Returns a list of device uint8 tensors [H, W], and with return_window also the list of
    (lo, hi) the images were mapped with (read back from the device in percentile mode).
    Limits (TypeError / ValueError before any launch): uint16 only, one channel, sides in
    [1, 65535], H * W <= 2^30, and those of mmdx.Window."""
    from . import window as W
    if not isinstance(window, W.Window):
        raise TypeError(f"window must be an mmdx.Window, got {type(window).__name__}")
    if isinstance(images, (np.ndarray, torch.Tensor)) or hasattr(images, "mode"):
        raise TypeError("window16 takes a list of images")
    planes = [W.as_plane(im) for im in images]
    descs, src_bytes, _ = W.plan(planes, window)   # every limit, before any upload
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("functional.window16 runs on the GPU (HIP); mmdx.window.reference "
                           "is the host statement")
    host = np.zeros(src_bytes, dtype=np.uint8)
    W.pack(planes, descs, host)
    with torch.cuda.device(device):
        out, levels = window_passes(torch.from_numpy(host).to(device), descs)
    res = []
    for d, a in zip(descs, planes):
        o = int(d["dst_off"])
        res.append(out[o:o + a.size].view(a.shape))
    if not return_window:
        return res
    if levels is None:
        return res, [(window.lo, window.hi)] * len(planes)
    return res, [(int(lo), int(hi)) for lo, hi in levels.cpu().tolist()]


# ----------------------------------------------------------------------------- retrieval
TOPK_MAX_N, TOPK_MAX_D, TOPK_MAX_NQ, TOPK_MAX_K = 1 << 24, 4096, 64, 64


def topk_rows_per_block() -> int:
    """The index rows one block of the select kernel scores per step (a tile edge for tests)."""
    return int(L.lib().mmdx_topk_rows_per_block())


def topk_similar(queries, index, k, exclude=None, out=None):
    """Exact top-k inner-product search (mmdx_topk_similar; mmdx.retrieval.reference_search is
    the definition): queries [nq, d] against index [N, d], both fp32, bf16 or fp16 on one GPU,
    contiguous; score = the fp32-accumulated dot product, NaN counting as -inf; row exclude[i]
    (int32 [nq], -1 = none) is removed for query i.  Returns (scores fp32 [nq, k], ids int32
    [nq, k]): the first k remaining rows under (score descending, id ascending), padded with
    (-inf, -1); `out` = (scores, ids) reuses the caller's tensors.  Limits: 1 <= N <= 2^24,
    d % 32 == 0, 32 <= d <= 4096, 1 <= nq <= 64, 1 <= k <= 64, exclude in [-1, N) (checked in one
    device reduction, the only host sync here, and only with `exclude`).  A wrong dtype is a
    TypeError; a wrong shape, device or layout or a limit exceeded a ValueError; nothing is
    copied, cast or launched then."""
    name = "topk_similar"
    if not torch.is_tensor(queries) or not torch.is_tensor(index):
        raise TypeError(f"{name} takes tensors")
    dt = L.dtype_code(index.dtype)
    if queries.dtype != index.dtype:
        raise TypeError(f"{name}: queries are {queries.dtype}, the index {index.dtype}")
    if exclude is not None and (not torch.is_tensor(exclude) or exclude.dtype != torch.int32):
        raise TypeError(f"{name}: exclude must be an int32 tensor")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"{name}: k must be an int, got {type(k).__name__}")
    k = int(k)
    if queries.dim() != 2 or index.dim() != 2 or queries.shape[1] != index.shape[1]:
        raise ValueError(f"{name}: queries {tuple(queries.shape)} and index "
                         f"{tuple(index.shape)} are not [nq, d] and [N, d]")
    (nq, d), N = queries.shape, index.shape[0]
    if not 1 <= N <= TOPK_MAX_N or d % 32 or not 32 <= d <= TOPK_MAX_D:
        raise ValueError(f"{name}: N = {N}, d = {d} outside 1 <= N <= 2^24, d a multiple of 32 "
                         f"in [32, {TOPK_MAX_D}]")
    if not 1 <= nq <= TOPK_MAX_NQ or not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"{name}: nq = {nq}, k = {k} outside [1, {TOPK_MAX_NQ}] and "
                         f"[1, {TOPK_MAX_K}]")
    if exclude is not None and tuple(exclude.shape) != (nq,):
        raise ValueError(f"{name}: exclude {tuple(exclude.shape)} is not [{nq}]")
    ins = [queries, index] + ([] if exclude is None else [exclude])
    outs = []
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise TypeError(f"{name}: out must be a pair (scores, ids)")
        for t, want in zip(out, (torch.float32, torch.int32)):
            if not torch.is_tensor(t) or t.dtype != want:
                raise TypeError(f"{name}: out must be (fp32 scores, int32 ids)")
            if tuple(t.shape) != (nq, k):
                raise ValueError(f"{name}: an out tensor is {tuple(t.shape)}, not [{nq}, {k}]")
        outs = list(out)
        if _shares_memory(outs[0], outs[1]) or any(_shares_memory(o, t) for o in outs
                                                   for t in ins):
            raise ValueError(f"{name}: out shares memory with an input or with itself")
    for t in ins + outs:
        if not t.is_contiguous():
            raise ValueError(f"{name}: an operand is not contiguous (never copied here)")
        if not t.is_cuda or t.device != index.device:
            raise ValueError(f"{name}: an operand is on {t.device}; the kernel runs on the GPU, "
                             f"all operands on one device")
    if queries.data_ptr() % 16 or index.data_ptr() % 16:
        raise ValueError(f"{name}: queries and index must be 16-byte aligned")
    if exclude is not None and bool(((exclude < -1) | (exclude >= N)).any()):
        raise ValueError(f"{name}: exclude has an entry outside [-1, {N})")
    need = int(L.lib().mmdx_topk_similar_workspace_size(N, d, nq, k))
    if need <= 0:
        raise ValueError(f"{name}: unsupported shape N = {N}, d = {d}, nq = {nq}, k = {k}")
    ws = L.workspace(need, index.device)
    if out is None:
        outs = [torch.empty((nq, k), dtype=torch.float32, device=index.device),
                torch.empty((nq, k), dtype=torch.int32, device=index.device)]
    call("mmdx_topk_similar", stream(), dt, ptr(queries), ptr(index), N, d, nq, k, ptr(exclude),
         ptr(outs[0]), ptr(outs[1]), ptr(ws), need)
    return outs[0], outs[1]
