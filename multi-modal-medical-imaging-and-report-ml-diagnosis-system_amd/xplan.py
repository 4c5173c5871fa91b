"""Launch plans for the transformer encoder stacks (BERT-base text tower, ViT-B/16 image
tower; BASELINE config C5).

Each stack (all of its layers) is ONE autograd node, like the ResNet trunk (resnet._TrunkFn):
its forward and its backward are recorded once per (shape, dtype, mode, parameter set) as
op lists over a persistent buffer arena (include/mmdx.h launch plans, csrc/plan.cpp) and
replayed by one native call per step.  The eager per-layer nodes (bert._BertLayerFn,
vit._VitBlockFn) issue the same kernels in the same order from Python — ~35 ctypes calls and
~30 allocations per layer and direction, 32 ms of host time per C5 step, most of the step;
here the host cost per stack and direction is one call plus the launches themselves.

Same arithmetic as the eager nodes (the plan-vs-eager tests require bit-identical outputs
and gradients with dropout off).  Dropout draws from the per-device launch counter
(_lib.rng_counter) under a seed fixed per plan op, so every replay draws fresh masks.
Per-call buffers enter as external bases: the stack input and the attention mask (forward),
the upstream gradient, the parameter-gradient arena and the mask (backward).  The parameter
gradients are views of one flat fp32 buffer per backward (the data-parallel reducer finds it
by storage and all-reduces it in place, like the trunk's arena).
"""
from __future__ import annotations

import math
import os
import weakref

import torch

from . import _lib as L
from . import functional as F
from .plan import WS, _Arena, _Ext, _OpList, _Token, pack_multi_args, plan_cache_get

# ViT backward: residual-branch gradient added inside the LayerNorm backward (1, default) or
# by a separate add pass (0); read by vit.py's eager path too
VIT_LN_ADDIN = os.environ.get("MMDX_VIT_LN_ADDIN", "1") == "1"
_F32 = torch.float32


def enabled() -> bool:
    """MMDX_STACK_PLANS=0 runs the eager per-layer nodes instead (A/B, debugging)."""
    return os.environ.get("MMDX_STACK_PLANS", "1") != "0"


class _Rec:
    """Records C-ABI calls as plan ops; buffers come from the plan's arena."""

    def __init__(self, arena, T, ops):
        self.arena, self.T, self.ops = arena, T, ops
        self.dt = L.dtype_code(T)
        self.ws_need = 0

    def buf(self, shape, dtype=None):
        return self.arena.new(shape, dtype or self.T)

    def _ws(self, n):
        self.ws_need = max(self.ws_need, int(n))
        return WS if n > 0 else None

    def cast(self, src, dst):
        self.ops.add(L.OP_CAST, L.dtype_code(dst.dtype), i=(L.dtype_code(src.dtype),),
                     l=(src.numel(),), p=(src, dst))

    def cast_weight(self, w, dst):
        """fp32 [K][C] master -> compute-dtype copy; every one of the stack's is cast by ONE
        multi-tensor launch at the head of the forward (flush_weight_casts)."""
        K, Cc = w.shape[0], w.numel() // w.shape[0]
        self.packs = getattr(self, "packs", []) + [(w, dst, None, K, Cc, Cc, 1)]

    def flush_weight_casts(self):
        packs = getattr(self, "packs", [])
        if not packs:
            return
        head = _OpList()
        head.add(L.OP_CONV_PACK_MULTI, self.dt, **pack_multi_args(self.arena, packs))
        self.ops.prepend(head)

    def copy(self, src, dst, n):
        self.ops.add(L.OP_CAST, self.dt, i=(self.dt,), l=(n,), p=(src, dst))

    def axpby(self, n, a, x, b, y, out):
        self.ops.add(L.OP_AXPBY, i=(), l=(n,), f=(a, b), p=(x, y, out))

    def gemm(self, A, lda, akm, B, ldb, bkm, M, N, K, C, ldc, c_dtype, bias=None, act=0,
             preact=None, beta=0.0, residual=None):
        """residual: a [M][ldc] tensor of C's dtype added last (mmdx_gemm_res)."""
        n = L.lib().mmdx_gemm_workspace_size(self.dt, M, N, K)
        self.ops.timed(F.gemm_cost(M, N, K, self.dt, L.dtype_code(c_dtype),
                                   1.0 if residual is not None else beta, act, preact),
                       L.OP_GEMM, dtype=self.dt,
                       i=(M, N, K, int(akm), int(bkm), L.dtype_code(c_dtype), act),
                       l=(lda, ldb, ldc, n), f=(1.0, beta),
                       p=(A, B, C, bias, None, preact, self._ws(n), residual))

    def gemm_wgrad_bias(self, dY, ldy, X, ldx, M, N, K, dW, ldw, db):
        """dW = dY^T X (fp32) and db = column sums of dY (mmdx_gemm_bias_grad)."""
        n = L.lib().mmdx_gemm_bias_grad_workspace_size(self.dt, M, N, K)
        self.ops.timed(F.gemm_cost(M, N, K, self.dt, L.F32, 0.0, L.ACT_NONE, None),
                       L.OP_GEMM_BIAS_GRAD, dtype=self.dt, i=(M, N, K, L.F32),
                       l=(ldy, ldx, ldw, n), p=(dY, X, dW, db, self._ws(n)))

    def attn_fwd(self, qkv, mask, B, Ls, H, scale, p_drop, seed, counter, out):
        """Returns what the backward needs besides qkv / out: the row log-sum-exp and the
        dropout stream base (flash-style, 16-bit) or the saved probabilities [B,H,L,L]."""
        if F.attn_flash(self.T):
            lse, rng = self.buf((B, H, Ls), _F32), self.buf((1,), torch.int64)
            self.ops.add(L.OP_ATTN_FWD_LSE, self.dt, i=(B, Ls, H), f=(scale, p_drop),
                         l=(seed,), p=(qkv, mask, counter, out, lse, rng))
            return ("lse", lse, rng)
        probs = self.buf((B, H, Ls, Ls), _F32)
        self.ops.add(L.OP_ATTN_FWD, self.dt, i=(B, Ls, H), f=(scale, p_drop), l=(seed,),
                     p=(qkv, mask, counter, out, probs))
        return ("probs", probs)

    def attn_bwd(self, qkv, saved, out, dout, mask, B, Ls, H, scale, p_drop, dqkv):
        if saved[0] == "lse":
            n = L.lib().mmdx_attention_lse_workspace_size(self.dt, B, Ls, H)
            self.ops.add(L.OP_ATTN_BWD_LSE, self.dt, i=(B, Ls, H), f=(scale, p_drop), l=(n,),
                         p=(qkv, out, saved[1], saved[2], dout, mask, dqkv, self._ws(n)))
            return
        n = L.lib().mmdx_attention_workspace_size(self.dt, B, Ls, H)
        self.ops.add(L.OP_ATTN_BWD, self.dt, i=(B, Ls, H), f=(scale, p_drop), l=(n,),
                     p=(qkv, saved[1], dout, mask, dqkv, self._ws(n)))

    def ln_fwd(self, x, res, g, b, eps, rows, D, y, xsum, mean, rstd):
        self.ops.add(L.OP_LN_FWD, self.dt, i=(D,), l=(rows,), f=(eps,),
                     p=(x, res, g, b, y, xsum, mean, rstd))

    def ln_fwd_drop(self, x, res, g, b, eps, p, seed, counter, rows, D, y, xsum, mean, rstd):
        """LayerNorm(dropout(x) + res); returns the dropout stream base buffer (rng)."""
        rng = self.buf((1,), torch.int64)
        self.ops.add(L.OP_LN_FWD_DROP, self.dt, i=(D,), l=(rows, seed), f=(eps, p),
                     p=(x, res, g, b, y, xsum, mean, rstd, counter, rng))
        return rng

    def ln_bwd_drop(self, xsum, dy, g, mean, rstd, p, rng, rows, D, dx, dx_drop, dg, db):
        n = L.lib().mmdx_layernorm_workspace_size(rows, D)
        self.ops.add(L.OP_LN_BWD_DROP, self.dt, i=(D,), l=(rows, n), f=(0.0, p),
                     p=(xsum, dy, g, mean, rstd, dx, dg, db, self._ws(n), rng, dx_drop))

    def ln_bwd(self, xsum, dy, g, mean, rstd, rows, D, dx, dg, db, addin=None):
        """addin: a residual branch's gradient added to dx (mmdx_layernorm_bwd_residual)."""
        n = L.lib().mmdx_layernorm_workspace_size(rows, D)
        self.ops.add(L.OP_LN_BWD, self.dt, i=(D,), l=(rows, n), f=(0.0,),
                     p=(xsum, dy, g, mean, rstd, dx, dg, db, self._ws(n), addin))

    def gelu_bwd(self, pre, dy, n, dx):
        self.ops.add(L.OP_GELU_BWD, self.dt, l=(n,), p=(pre, dy, dx))

    def colsum(self, dy, M, N, db):
        n = L.lib().mmdx_bias_grad_workspace_size(M, N)
        self.ops.add(L.OP_BIAS_GRAD, self.dt, i=(N,), l=(M, n), f=(0.0,),
                     p=(dy, db, self._ws(n)))

    def add(self, x, y, n, out):
        self.ops.add(L.OP_ADD, self.dt, l=(n,), p=(x, y, out))

    def dropout_fwd(self, x, n, p, seed, counter, y, mask):
        self.ops.add(L.OP_DROPOUT_FWD, self.dt, f=(p,), l=(n, seed, 0), p=(x, counter, y, mask))

    def dropout_bwd(self, dy, mask, n, p, dx):
        self.ops.add(L.OP_DROPOUT_BWD, self.dt, f=(p,), l=(n,), p=(dy, mask, dx))


class _GradLayout:
    """Byte offsets of the parameter gradients in the flat fp32 gradient buffer."""

    def __init__(self):
        self.n = 0
        self.items = []   # (param index, shape, element offset)

    def take(self, shape, idx=None):
        off = self.n
        self.n += math.prod(shape)
        if idx is not None:
            self.items.append((idx, tuple(shape), off))
        return off

    @staticmethod
    def ext(off):
        return _Ext(1, 4 * off)


class _StackPlan:
    """Forward + backward op lists of one stack configuration over one arena."""

    def __init__(self, dev, T):
        self.arena = _Arena(dev)
        self.T = T
        self.fwd = _OpList()
        self.bwd = _OpList()
        self.out = None
        self.dx = None
        self.grads = _GradLayout()
        # [(lo, hi)] element ranges of the gradient buffer that are final at each backward
        # segment boundary (groups of SEG_LAYERS layers, last layer first)
        self.grad_regions = []

    def cut_after_layers(self, li, nl, start):
        """Segment boundary after layer li's backward (layers run nl-1 .. 0): every
        SEG_LAYERS layers, the gradients of layers li .. li+SEG_LAYERS-1 are final.
        start(j) = first gradient element of layer j (start(nl) = the buffer's end)."""
        seg = SEG_LAYERS
        if seg <= 0 or li == 0 or (nl - li) % seg:
            return
        self.bwd.cut()
        self.grad_regions.append((start(li), start(min(nl, li + seg))))

    def finish(self, recs):
        need = max(r.ws_need for r in recs)
        ws = self.arena.new((max(1, need),), torch.uint8)
        for lst in (self.fwd, self.bwd):
            lst.patch({WS: ws.data_ptr()})
            lst.freeze()


# Layers per backward segment of a stack plan.  Between segments the backward returns to the
# host, which calls STACK_SEGMENT_HOOK(grads, lo, hi) with the stream the backward runs on
# current: grads[lo:hi] (those layers' parameter gradients) is final once that stream reaches
# this point, so the data-parallel reducer issues its in-place all-reduce right there
# (dist.GradAllReducer.trunk_segment; RCCL's stream waits on the current one) and it runs
# beside the remaining layers' backward.  None = one native call for the whole backward.
SEG_LAYERS = int(os.environ.get("MMDX_DP_STACK_SEG_LAYERS", "3"))
STACK_SEGMENT_HOOK = None


def _plans_for(owner, key, build):
    cache = owner.__dict__.setdefault("_mmdx_stack_plans", {})
    return plan_cache_get(cache, key, build)


def _seed(base):
    """A dropout seed for a plan op, as the signed 64-bit value a plan field holds."""
    v = L.dropout_seed(base)
    return v - (1 << 64) if v >= (1 << 63) else v


# ------------------------------------------------------------------------ BERT encoder
# per layer, in bert.BertLayer.params() order:
# wq, bq, wk, bk, wv, bv, wo, bo, g1, b1, wi, bi, wo2, bo2, g2, b2
_BERT_NP = 16


def _build_bert(params, B, Ls, D, Hn, I, eps, p, pa, T, dev):
    pl = _StackPlan(dev, T)
    M = B * Ls
    scale = 1.0 / math.sqrt(D // Hn)
    counter = L.rng_counter(dev)
    nl = len(params) // _BERT_NP
    rf = _Rec(pl.arena, T, pl.fwd)
    x = _Ext(0)
    mask = _Ext(1)
    saves = []
    for li in range(nl):
        (wq, bq, wk, bk, wv, bv, wo, bo, g1, b1, wi, bi, wo2, bo2, g2,
         b2) = params[li * _BERT_NP:(li + 1) * _BERT_NP]
        wqkv = rf.buf((3 * D, D))
        for j, w in enumerate((wq, wk, wv)):
            rf.cast_weight(w, wqkv[j * D:(j + 1) * D])
        bqkv = rf.buf((3 * D,), _F32)
        for j, bb in enumerate((bq, bk, bv)):
            rf.axpby(D, 1.0, bb, 0.0, None, bqkv[j * D:(j + 1) * D])
        qkv = rf.buf((M, 3 * D))
        rf.gemm(x, D, True, wqkv, D, True, M, 3 * D, D, qkv, 3 * D, T, bias=bqkv)
        att = rf.buf((M, D))
        probs = rf.attn_fwd(qkv, mask, B, Ls, Hn, scale, pa,
                            _seed(0xA770 + 7919 * li) if pa > 0 else 0, counter, att)
        woc = rf.buf((D, D))
        rf.cast_weight(wo, woc)
        a = rf.buf((M, D))
        rf.gemm(att, D, True, woc, D, True, M, D, D, a, D, T, bias=bo)
        # BertSelfOutput: LayerNorm(dropout(a) + x), the dropout inside the LayerNorm pass
        # (no dropped tensor, no mask: the backward redraws the keep bits from rng)
        m1 = None
        h1, xs1 = rf.buf((M, D)), rf.buf((M, D))
        mu1, rs1 = rf.buf((M,), _F32), rf.buf((M,), _F32)
        if p > 0:
            m1 = rf.ln_fwd_drop(a, x, g1, b1, eps, p, _seed(0xD401 + 7919 * li), counter, M, D,
                                h1, xs1, mu1, rs1)
        else:
            rf.ln_fwd(a, x, g1, b1, eps, M, D, h1, xs1, mu1, rs1)
        wic = rf.buf((I, D))
        rf.cast_weight(wi, wic)
        f, pre = rf.buf((M, I)), rf.buf((M, I))
        rf.gemm(h1, D, True, wic, D, True, M, I, D, f, I, T, bias=bi, act=L.ACT_GELU,
                preact=pre)
        wo2c = rf.buf((D, I))
        rf.cast_weight(wo2, wo2c)
        f2 = rf.buf((M, D))
        rf.gemm(f, I, True, wo2c, I, True, M, D, I, f2, D, T, bias=bo2)
        m2 = None
        h2, xs2 = rf.buf((M, D)), rf.buf((M, D))
        mu2, rs2 = rf.buf((M,), _F32), rf.buf((M,), _F32)
        if p > 0:   # BertOutput: LayerNorm(dropout(f2) + h1)
            m2 = rf.ln_fwd_drop(f2, h1, g2, b2, eps, p, _seed(0xD402 + 7919 * li), counter, M,
                                D, h2, xs2, mu2, rs2)
        else:
            rf.ln_fwd(f2, h1, g2, b2, eps, M, D, h2, xs2, mu2, rs2)
        saves.append(dict(x=x, wqkv=wqkv, qkv=qkv, probs=probs, att=att, woc=woc, xs1=xs1,
                          mu1=mu1, rs1=rs1, h1=h1, wic=wic, pre=pre, f=f, wo2c=wo2c, xs2=xs2,
                          mu2=mu2, rs2=rs2, m1=m1, m2=m2))
        x = h2
    pl.out = x
    rf.flush_weight_casts()

    # backward: ext 0 = upstream gradient [M, D] (compute dtype), 1 = gradient buffer,
    # 2 = mask.  Shared temporaries across layers; Y carries d(layer output) downward.
    rb = _Rec(pl.arena, T, pl.bwd)
    mask = _Ext(2)
    X, Y = rb.buf((M, D)), rb.buf((M, D))
    DX2 = rb.buf((M, D)) if p > 0 else None
    DY1 = rb.buf((M, D)) if p > 0 else None
    dpre = rb.buf((M, I))
    datt, dqkv = rb.buf((M, D)), rb.buf((M, 3 * D))
    G = pl.grads
    offs = []
    for li in range(nl):  # gradient layout in forward order
        base = li * _BERT_NP
        o = {}
        o["wqkv"] = G.take((3 * D, D))
        for j in range(3):
            G.items.append((base + 2 * j, (D, D), o["wqkv"] + j * D * D))
        o["bqkv"] = G.take((3 * D,))
        for j in range(3):
            G.items.append((base + 2 * j + 1, (D,), o["bqkv"] + j * D))
        for name, idx, shape in (("wo", 6, (D, D)), ("bo", 7, (D,)), ("g1", 8, (D,)),
                                 ("b1", 9, (D,)), ("wi", 10, (I, D)), ("bi", 11, (I,)),
                                 ("wo2", 12, (D, I)), ("bo2", 13, (D,)), ("g2", 14, (D,)),
                                 ("b2", 15, (D,))):
            o[name] = G.take(shape, base + idx)
        offs.append(o)
    gx = G.ext
    dh = _Ext(0)
    for li in range(nl - 1, -1, -1):
        s, o = saves[li], offs[li]
        g1 = params[li * _BERT_NP + 8]
        g2 = params[li * _BERT_NP + 14]
        dX2 = X
        if p > 0:
            rb.ln_bwd_drop(s["xs2"], dh, g2, s["mu2"], s["rs2"], p, s["m2"], M, D, X, DX2,
                           gx(o["g2"]), gx(o["b2"]))
            dX2 = DX2
        else:
            rb.ln_bwd(s["xs2"], dh, g2, s["mu2"], s["rs2"], M, D, X, gx(o["g2"]), gx(o["b2"]))
        rb.gemm(dX2, D, True, s["wo2c"], I, False, M, I, D, dpre, I, T, act=L.ACT_GELU_BWD,
                preact=s["pre"])
        rb.gemm_wgrad_bias(dX2, D, s["f"], I, D, I, M, gx(o["wo2"]), I, gx(o["bo2"]))
        rb.gemm_wgrad_bias(dpre, I, s["h1"], D, I, D, M, gx(o["wi"]), D, gx(o["bi"]))
        rb.gemm(dpre, I, True, s["wic"], D, False, M, D, I, X, D, T, beta=1.0)
        dY1 = Y
        if p > 0:
            rb.ln_bwd_drop(s["xs1"], X, g1, s["mu1"], s["rs1"], p, s["m1"], M, D, Y, DY1,
                           gx(o["g1"]), gx(o["b1"]))
            dY1 = DY1
        else:
            rb.ln_bwd(s["xs1"], X, g1, s["mu1"], s["rs1"], M, D, Y, gx(o["g1"]), gx(o["b1"]))
        rb.gemm(dY1, D, True, s["woc"], D, False, M, D, D, datt, D, T)
        rb.gemm_wgrad_bias(dY1, D, s["att"], D, D, D, M, gx(o["wo"]), D, gx(o["bo"]))
        rb.attn_bwd(s["qkv"], s["probs"], s["att"], datt, mask, B, Ls, Hn, scale, pa, dqkv)
        xin = s["x"] if not isinstance(s["x"], _Ext) else _Ext(3)  # the stack input
        rb.gemm_wgrad_bias(dqkv, 3 * D, xin, D, 3 * D, D, M, gx(o["wqkv"]), D, gx(o["bqkv"]))
        rb.gemm(dqkv, 3 * D, True, s["wqkv"], D, False, M, D, 3 * D, Y, D, T, beta=1.0)
        dh = Y
        pl.cut_after_layers(li, nl, lambda j: offs[j]["wqkv"] if j < nl else G.n)
    pl.dx = Y
    pl.finish((rf, rb))
    return pl


# ------------------------------------------------------------------------ ViT encoder
# per block, in vit.EncoderBlock order:
# g1, b1, w_in, b_in, w_out, b_out, g2, b2, w1, bb1, w2, bb2
_VIT_NP = 12


def _build_vit(params, N, S, D, heads, I, eps, T, dev):
    pl = _StackPlan(dev, T)
    M = N * S
    scale = 1.0 / math.sqrt(D // heads)
    nl = len(params) // _VIT_NP
    rf = _Rec(pl.arena, T, pl.fwd)
    x = _Ext(0)
    saves = []
    for li in range(nl):
        g1, b1, w_in, b_in, w_out, b_out, g2, b2, w1, bb1, w2, bb2 = \
            params[li * _VIT_NP:(li + 1) * _VIT_NP]
        u1, mu1, rs1 = rf.buf((M, D)), rf.buf((M,), _F32), rf.buf((M,), _F32)
        rf.ln_fwd(x, None, g1, b1, eps, M, D, u1, None, mu1, rs1)
        wqkv = rf.buf((3 * D, D))
        rf.cast_weight(w_in, wqkv)
        qkv = rf.buf((M, 3 * D))
        rf.gemm(u1, D, True, wqkv, D, True, M, 3 * D, D, qkv, 3 * D, T, bias=b_in)
        att = rf.buf((M, D))
        probs = rf.attn_fwd(qkv, None, N, S, heads, scale, 0.0, 0, None, att)
        woc = rf.buf((D, D))
        rf.cast_weight(w_out, woc)
        o_ = rf.buf((M, D))
        rf.gemm(att, D, True, woc, D, True, M, D, D, o_, D, T, bias=b_out)
        u2, a = rf.buf((M, D)), rf.buf((M, D))
        mu2, rs2 = rf.buf((M,), _F32), rf.buf((M,), _F32)
        rf.ln_fwd(o_, x, g2, b2, eps, M, D, u2, a, mu2, rs2)
        w1c = rf.buf((I, D))
        rf.cast_weight(w1, w1c)
        f, pre = rf.buf((M, I)), rf.buf((M, I))
        rf.gemm(u2, D, True, w1c, D, True, M, I, D, f, I, T, bias=bb1, act=L.ACT_GELU,
                preact=pre)
        w2c = rf.buf((D, I))
        rf.cast_weight(w2, w2c)
        out = rf.buf((M, D))   # out = a + f W2^T + b2, the residual read by the epilogue
        rf.gemm(f, I, True, w2c, I, True, M, D, I, out, D, T, bias=bb2, residual=a)
        saves.append(dict(x=x, u1=u1, mu1=mu1, rs1=rs1, wqkv=wqkv, qkv=qkv, probs=probs,
                          att=att, woc=woc, a=a, u2=u2, mu2=mu2, rs2=rs2, w1c=w1c, pre=pre,
                          f=f, w2c=w2c))
        x = out
    pl.out = x
    rf.flush_weight_casts()

    # backward: ext 0 = upstream gradient, 1 = gradient buffer, 3 = the stack input
    rb = _Rec(pl.arena, T, pl.bwd)
    dpre = rb.buf((M, I))
    du2, DA, da_ln = rb.buf((M, D)), rb.buf((M, D)), rb.buf((M, D))
    datt, dqkv, du1 = rb.buf((M, D)), rb.buf((M, 3 * D)), rb.buf((M, D))
    DX = rb.buf((M, D))
    G = pl.grads
    offs = []
    for li in range(nl):
        base = li * _VIT_NP
        shapes = ((D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (I, D), (I,),
                  (D, I), (D,))
        offs.append([G.take(sh, base + j) for j, sh in enumerate(shapes)])
    gx = G.ext
    dO = _Ext(0)
    for li in range(nl - 1, -1, -1):
        s, o = saves[li], offs[li]
        g1 = params[li * _VIT_NP + 0]
        g2 = params[li * _VIT_NP + 6]
        rb.gemm(dO, D, True, s["w2c"], I, False, M, I, D, dpre, I, T, act=L.ACT_GELU_BWD,
                preact=s["pre"])
        rb.gemm_wgrad_bias(dO, D, s["f"], I, D, I, M, gx(o[10]), I, gx(o[11]))
        rb.gemm_wgrad_bias(dpre, I, s["u2"], D, I, D, M, gx(o[8]), D, gx(o[9]))
        rb.gemm(dpre, I, True, s["w1c"], D, False, M, D, I, du2, D, T)
        # da = dO + LN2'(du2): the residual branch's gradient added inside the LN backward
        # (mmdx_layernorm_bwd_residual; MMDX_VIT_LN_ADDIN=0: a separate add pass).  Within the
        # box-to-box spread on C5: -0.8 % and +1.2 % against the add pass on two boxes, paired
        # (profiles/r04_c5_ab_ln_addin.txt)
        if VIT_LN_ADDIN:
            rb.ln_bwd(s["a"], du2, g2, s["mu2"], s["rs2"], M, D, DA, gx(o[6]), gx(o[7]), addin=dO)
        else:
            rb.ln_bwd(s["a"], du2, g2, s["mu2"], s["rs2"], M, D, da_ln, gx(o[6]), gx(o[7]))
            rb.add(dO, da_ln, M * D, DA)
        rb.gemm(DA, D, True, s["woc"], D, False, M, D, D, datt, D, T)
        rb.gemm_wgrad_bias(DA, D, s["att"], D, D, D, M, gx(o[4]), D, gx(o[5]))
        rb.attn_bwd(s["qkv"], s["probs"], s["att"], datt, None, N, S, heads, scale, 0.0, dqkv)
        rb.gemm_wgrad_bias(dqkv, 3 * D, s["u1"], D, 3 * D, D, M, gx(o[2]), D, gx(o[3]))
        rb.gemm(dqkv, 3 * D, True, s["wqkv"], D, False, M, D, 3 * D, du1, D, T)
        xin = s["x"] if not isinstance(s["x"], _Ext) else _Ext(3)
        if VIT_LN_ADDIN:
            rb.ln_bwd(xin, du1, g1, s["mu1"], s["rs1"], M, D, DX, gx(o[0]), gx(o[1]), addin=DA)
        else:
            rb.ln_bwd(xin, du1, g1, s["mu1"], s["rs1"], M, D, da_ln, gx(o[0]), gx(o[1]))
            rb.add(DA, da_ln, M * D, DX)
        dO = DX
        pl.cut_after_layers(li, nl, lambda j: offs[j][0] if j < nl else G.n)
    pl.dx = DX
    pl.finish((rf, rb))
    return pl


# ------------------------------------------------------------------------ autograd node
class _StackFn(torch.autograd.Function):
    """forward(h, mask, spec, *params) -> stack output; spec: ("bert", cfg) / ("vit", cfg)."""

    @staticmethod
    def forward(ctx, h, mask, spec, owner, *params):
        kind, cfg = spec
        T = h.dtype
        dev = h.device
        h = h.contiguous()
        if kind == "bert":
            B, Ls, D = h.shape
            I = params[10].shape[0]
            key = ("bert", B, Ls, D, T, cfg.p, cfg.pa, tuple(q.data_ptr() for q in params))
            pl = _plans_for(owner, key, lambda: _build_bert(
                params, B, Ls, D, cfg.heads, I, cfg.eps, cfg.p, cfg.pa, T, dev))
            ext = [h.data_ptr(), mask.data_ptr()]
        else:
            N, S, D = h.shape
            I = params[8].shape[0]
            key = ("vit", N, S, D, T, tuple(q.data_ptr() for q in params))
            pl = _plans_for(owner, key, lambda: _build_vit(
                params, N, S, D, cfg.heads, I, cfg.eps, T, dev))
            ext = [h.data_ptr(), 0]
        strm = [torch.cuda.current_stream().cuda_stream]
        pl.fwd.run(ext, strm, timer=F.GEMM_TIMER)
        tok = _Token()
        pl.arena.owner = weakref.ref(tok)
        ctx.tok, ctx.plan, ctx.kind = tok, pl, kind
        ctx.save_for_backward(h, mask if kind == "bert" else None)
        ctx.nparams = len(params)
        return pl.out.clone().view(h.shape)

    @staticmethod
    def backward(ctx, dout):
        pl = ctx.plan
        h, mask = ctx.saved_tensors
        T = h.dtype
        dout = F.cast(dout.contiguous(), T)
        grads = torch.empty(pl.grads.n, dtype=_F32, device=h.device)
        ext = [dout.data_ptr(), grads.data_ptr(),
               mask.data_ptr() if mask is not None else 0, h.data_ptr()]
        hook = STACK_SEGMENT_HOOK
        between = None
        if hook is not None and pl.grad_regions:
            def between(k):
                lo, hi = pl.grad_regions[k]
                hook(grads, lo, hi)
        pl.bwd.run(ext, [torch.cuda.current_stream().cuda_stream], timer=F.GEMM_TIMER,
                   between=between)
        dx = pl.dx.clone().view(h.shape)
        out = [None] * ctx.nparams
        for idx, shape, off in pl.grads.items:
            out[idx] = grads[off:off + math.prod(shape)].view(shape)
        pl.arena.owner = None
        ctx.plan = ctx.tok = None
        return (dx, None, None, None, *out)


def run_stack(kind, h, mask, cfg, owner, params):
    """The stack through its plan, or None when the plan path does not apply (grad off or
    a frozen parameter: the eager nodes handle those)."""
    if not enabled() or not torch.is_grad_enabled():
        return None
    if not all(q.requires_grad for q in params):
        return None
    return _StackFn.apply(h, mask, (kind, cfg), owner, *params)
