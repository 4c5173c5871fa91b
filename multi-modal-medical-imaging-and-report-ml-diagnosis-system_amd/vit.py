"""ViT-B/16 image tower on the mmdx kernels (build-defined backbone name "vit_b_16", SURVEY
§8 a1 / BASELINE config C5), state_dict-identical to torchvision's `vit_b_16()` minus the
classification head: conv_proj, class_token, encoder.pos_embedding,
encoder.layers.encoder_layer_{i}.{ln_1, self_attention.{in_proj_weight, in_proj_bias,
out_proj}, ln_2, mlp.{0,3}}, encoder.ln.

Forward semantics (torchvision VisionTransformer, dropout 0): patch embedding Conv2d(3, 768,
16, stride 16) -> prepend class token -> + pos_embedding -> 12 pre-LN blocks
{x = x + MHA(LN1(x)); x = x + MLP(LN2(x))} (LN eps 1e-6, exact GELU) -> encoder.ln ->
class-token row (the [B, 768] feature the image encoder's `proj` consumes).

Kernels: patchify + one GEMM for the patch embedding, token assembly, per block the fused
QKV GEMM, attention core (no key mask), out-proj GEMM, LayerNorm with the residual sum
fused in (it emits both x + attn and LN2 of it), MLP GEMMs with the GELU in the epilogue
and the second residual read by the last GEMM's epilogue.  The block is written once, in
xlayers (vit_fwd / vit_bwd): _VitBlockFn here issues it call by call (inference, no_grad, a
frozen block parameter), xplan records the same body as a launch plan for the whole stack.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import _lib as L
from . import functional as F
from . import xlayers as XL
from . import xplan
from ._lib import call, ptr, stream
from .layers import LayerNorm, Linear

D_MODEL, HEADS, MLP_DIM, LAYERS, PATCH, IMG = 768, 12, 3072, 12, 16, 224
EPS = 1e-6


def _colsum(t, M, N):
    return F._bias_grad(t, M, N, torch.empty(N, dtype=torch.float32, device=t.device))


class _PatchTokensFn(torch.autograd.Function):
    """images [N,3,224,224] fp32 -> tokens [N,197,768] (class token + patches + pos)."""

    @staticmethod
    def forward(ctx, x, w, b, cls, pos, T):
        L.require_device(x)
        N, C, H, W = x.shape
        S = (H // PATCH) * (W // PATCH)
        K = C * PATCH * PATCH
        D = w.shape[0]
        dev = x.device
        patches = torch.empty((N * S, K), dtype=T, device=dev)
        call("mmdx_patchify", L.dtype_code(T), ptr(x.contiguous()), N, C, H, W, PATCH,
             ptr(patches), stream())
        wc = F.cast(w.reshape(D, K), T)
        emb = torch.empty((N * S, D), dtype=T, device=dev)
        F.gemm(patches, K, True, wc, K, True, N * S, D, K, emb, D, bias=b, compute_dtype=T)
        tok = torch.empty((N, S + 1, D), dtype=T, device=dev)
        call("mmdx_vit_tokens_fwd", L.dtype_code(T), ptr(emb), ptr(cls), ptr(pos), N, S + 1, D,
             ptr(tok), stream())
        ctx.save_for_backward(patches)
        ctx.dims = (N, S, K, D, tuple(w.shape))
        return tok

    @staticmethod
    def backward(ctx, dtok):
        (patches,) = ctx.saved_tensors
        N, S, K, D, wshape = ctx.dims
        T = patches.dtype
        dev = patches.device
        dtok = F.cast(dtok.contiguous(), T)
        demb = torch.empty((N * S, D), dtype=T, device=dev)
        call("mmdx_vit_tokens_bwd", L.dtype_code(T), ptr(dtok), N, S + 1, D, ptr(demb), stream())
        dpos = _colsum(dtok, N, (S + 1) * D)
        dcls = torch.empty(D, dtype=torch.float32, device=dev)
        call("mmdx_axpby", D, 1.0, ptr(dpos), 0.0, None, ptr(dcls), stream())
        dW = torch.empty((D, K), dtype=torch.float32, device=dev)
        F.gemm(demb, D, False, patches, K, False, D, K, N * S, dW, K, compute_dtype=T)
        db = _colsum(demb, N * S, D)
        return (None, dW.reshape(wshape), db, dcls.reshape(1, 1, D),
                dpos.reshape(1, S + 1, D), None)


class _VitBlockFn(torch.autograd.Function):
    """One torchvision EncoderBlock (pre-LN): xlayers.vit_fwd / vit_bwd issued at once."""

    @staticmethod
    def forward(ctx, h, heads, *params):
        N, S, D = h.shape
        keep = any(ctx.needs_input_grad)
        ctx.c = c = SimpleNamespace(B=N, Ls=S, D=D, H=heads, I=params[8].shape[0], eps=EPS)
        be = XL.Eager(h.dtype, h.device, keep)
        out, saved = XL.vit_fwd(be, 0, h.reshape(N * S, D), None, params, c)
        if keep:
            XL.save(ctx, saved)
        return out.reshape(N, S, D)

    @staticmethod
    def backward(ctx, dout):
        c, s = ctx.c, XL.load(ctx)
        x = s["x"]
        be = XL.Eager(x.dtype, x.device, True)
        table = XL.vit_grads(c.D, c.I)
        gd = be.grad_bufs(table)
        dO = F.cast(dout.contiguous().reshape(x.shape), x.dtype)
        dx = XL.vit_bwd(be, s, dO, None, gd, c)
        return (dx.reshape(c.B, c.Ls, c.D), None, *XL.in_param_order(table, gd, 12))


class _ClassTokenLNFn(torch.autograd.Function):
    """encoder.ln applied to the class-token rows only (the only rows the tower returns)."""

    @staticmethod
    def forward(ctx, h, g, b):
        N, S, D = h.shape
        T = h.dtype
        rows = torch.empty((N, D), dtype=T, device=h.device)
        call("mmdx_rows_copy", L.dtype_code(T), ptr(h), S * D, ptr(rows), D, N, D, stream())
        y, _, mean, rstd = F.ln_fwd(rows, None, g, b, EPS, want_sum=False)
        ctx.save_for_backward(rows, g, mean, rstd)
        ctx.S = S
        return y

    @staticmethod
    def backward(ctx, dy):
        rows, g, mean, rstd = ctx.saved_tensors
        N, D = rows.shape
        S = ctx.S
        T = rows.dtype
        drow, dg, db = F.ln_bwd(rows, F.cast(dy.contiguous(), T), g, mean, rstd)
        dh = torch.zeros((N, S, D), dtype=T, device=rows.device)
        call("mmdx_rows_copy", L.dtype_code(T), ptr(drow), D, ptr(dh), S * D, N, D, stream())
        return dh, dg, db


# ----------------------------------------------------------------------------- modules
class EncoderBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.ln_1 = LayerNorm(D_MODEL, eps=EPS)
        self.self_attention = nn.MultiheadAttention(D_MODEL, HEADS, batch_first=True)
        self.ln_2 = LayerNorm(D_MODEL, eps=EPS)
        self.mlp = nn.Sequential(OrderedDict([
            ("0", Linear(D_MODEL, MLP_DIM)), ("1", nn.GELU()), ("2", nn.Dropout(0.0)),
            ("3", Linear(MLP_DIM, D_MODEL)), ("4", nn.Dropout(0.0))]))
        for m in (self.mlp[0], self.mlp[3]):  # torchvision MLPBlock init
            nn.init.xavier_uniform_(m.weight)
            nn.init.normal_(m.bias, std=1e-6)

    def forward(self, h):
        at = self.self_attention
        return _VitBlockFn.apply(h, HEADS, self.ln_1.weight, self.ln_1.bias, at.in_proj_weight,
                                 at.in_proj_bias, at.out_proj.weight, at.out_proj.bias,
                                 self.ln_2.weight, self.ln_2.bias, self.mlp[0].weight,
                                 self.mlp[0].bias, self.mlp[3].weight, self.mlp[3].bias)


class Encoder(nn.Module):
    def __init__(self, seq_len, layers=LAYERS):
        super().__init__()
        self.pos_embedding = nn.Parameter(torch.empty(1, seq_len, D_MODEL).normal_(std=0.02))
        self.dropout = nn.Dropout(0.0)
        self.layers = nn.Sequential(OrderedDict(
            (f"encoder_layer_{i}", EncoderBlock()) for i in range(layers)))
        self.ln = LayerNorm(D_MODEL, eps=EPS)


class VitTrunk(nn.Module):
    """torchvision vit_b_16 without `heads`; forward -> class-token features [B, 768]."""

    def __init__(self, layers=LAYERS):
        super().__init__()
        self.conv_proj = nn.Conv2d(3, D_MODEL, PATCH, PATCH)
        fan_in = 3 * PATCH * PATCH
        nn.init.trunc_normal_(self.conv_proj.weight, std=math.sqrt(1 / fan_in))
        nn.init.zeros_(self.conv_proj.bias)
        self.class_token = nn.Parameter(torch.zeros(1, 1, D_MODEL))
        self.encoder = Encoder((IMG // PATCH) ** 2 + 1, layers)
        self.feat_dim = D_MODEL
        self.compute_dtype = torch.float32

    def forward(self, x):
        T = self.compute_dtype
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("expected images [B,3,H,W]")
        h = _PatchTokensFn.apply(x.float(), self.conv_proj.weight, self.conv_proj.bias,
                                 self.class_token, self.encoder.pos_embedding, T)
        params = []
        for blk in self.encoder.layers:
            at = blk.self_attention
            params += [blk.ln_1.weight, blk.ln_1.bias, at.in_proj_weight, at.in_proj_bias,
                       at.out_proj.weight, at.out_proj.bias, blk.ln_2.weight, blk.ln_2.bias,
                       blk.mlp[0].weight, blk.mlp[0].bias, blk.mlp[3].weight, blk.mlp[3].bias]
        # the 12 blocks as one native launch plan per direction (xplan); the eager per-block
        # nodes when gradients are off or a block parameter is frozen
        cfg = type("VitCfg", (), dict(heads=HEADS, eps=EPS))
        out = xplan.run_stack("vit", h, None, cfg, self.encoder, params) if params else None
        if out is not None:
            h = out
        else:
            for blk in self.encoder.layers:
                h = blk(h)
        return _ClassTokenLNFn.apply(h, self.encoder.ln.weight, self.encoder.ln.bias)

    def block_params(self):
        """The 12 parameters of every block, in xlayers.vit_fwd's order."""
        out = []
        for blk in self.encoder.layers:
            at = blk.self_attention
            out.append((blk.ln_1.weight, blk.ln_1.bias, at.in_proj_weight, at.in_proj_bias,
                        at.out_proj.weight, at.out_proj.bias, blk.ln_2.weight, blk.ln_2.bias,
                        blk.mlp[0].weight, blk.mlp[0].bias, blk.mlp[3].weight,
                        blk.mlp[3].bias))
        return out

    def forward_blocks(self, x, keep, on_block=None):
        """The patch tokens and the eager block bodies (xlayers.vit_fwd, the launches of
        forward() under no_grad) without autograd: -> (last block's output [B, S, 768], c, the
        per-block `saved` dicts when keep).  on_block(li, saved) runs after each block."""
        T = self.compute_dtype
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("expected images [B,3,H,W]")
        with torch.no_grad():
            h = _PatchTokensFn.apply(x.float(), self.conv_proj.weight, self.conv_proj.bias,
                                     self.class_token, self.encoder.pos_embedding, T)
            N, S, D = h.shape
            c = SimpleNamespace(B=N, Ls=S, D=D, H=HEADS, I=MLP_DIM, eps=EPS)
            be = XL.Eager(T, h.device, keep)
            h = h.reshape(N * S, D)
            kept = []
            for li, params in enumerate(self.block_params()):
                h, saved = XL.vit_fwd(be, 0, h, None, params, c)
                if on_block is not None:
                    on_block(li, saved)
                if keep:
                    kept.append(saved)
        return h.reshape(N, S, D), c, kept

    def forward_attention(self, x):
        """-> (feats [B, 768], abar [layers, B, S, S] fp32): forward()'s features under no_grad,
        bit for bit (the same launches), and every block's head-averaged attention map
        (functional.attention_relevance on the block's qkv buffer), for attention rollout."""
        maps = []
        B, scale = x.shape[0], 1.0 / math.sqrt(D_MODEL // HEADS)

        def grab(li, saved):
            qkv = saved["qkv"]
            maps.append(F.attention_relevance(qkv, B, qkv.shape[0] // B, HEADS, scale))

        h, _, _ = self.forward_blocks(x, False, grab)
        with torch.no_grad():
            feats = _ClassTokenLNFn.apply(h, self.encoder.ln.weight, self.encoder.ln.bias)
        return feats, torch.stack(maps)
