"""Launch plans for the transformer encoder stacks (BERT-base text tower, ViT-B/16 image
tower; BASELINE config C5).

Each stack (all of its layers) is ONE autograd node, like the ResNet trunk (resnet._TrunkFn):
its forward and its backward are recorded once per (shape, dtype, mode, parameter set) as
op lists over a persistent buffer arena (include/mmdx.h launch plans, csrc/plan.cpp) and
replayed by one native call per step.  The layers themselves are written once, in xlayers
(bert_fwd / bert_bwd, vit_fwd / vit_bwd), over a recorder interface: _Rec here records their
calls as plan ops, xlayers.Eager (behind bert._BertLayerFn, vit._VitBlockFn) issues them at
once from Python — ~35 ctypes calls and ~30 allocations per layer and direction, 32 ms of
host time per C5 step, most of the step; here the host cost per stack and direction is one
call plus the launches themselves.

Same body, so the same kernels with the same operands in the same order as the eager nodes
(the plan-vs-eager tests require bit-identical outputs and gradients with dropout off;
tools/plan_dump.py --stacks diffs two revisions' plans on the CPU).  What differs is in the
back-end methods: weight casts hoisted into one launch, backward temporaries shared across
layers, gradients at offsets of one flat buffer.  Dropout draws from the per-device launch
counter (_lib.rng_counter) under a seed fixed per plan op, so every replay draws fresh masks.
Per-call buffers enter as external bases: the stack input and the attention mask (forward),
the upstream gradient, the parameter-gradient arena and the mask (backward).  The parameter
gradients are views of one flat fp32 buffer per backward (the data-parallel reducer finds it
by storage and all-reduces it in place, like the trunk's arena).
"""
from __future__ import annotations

import math
import os
import weakref
from types import SimpleNamespace

import torch

from . import _lib as L
from . import functional as F
from . import xlayers as XL
from .plan import WS, _Arena, _Ext, _OpList, _Token, pack_multi_args, plan_cache_get

_F32 = torch.float32


def enabled() -> bool:
    """MMDX_STACK_PLANS=0 runs the eager per-layer nodes instead (A/B, debugging)."""
    return os.environ.get("MMDX_STACK_PLANS", "1") != "0"


class _Rec:
    """Records C-ABI calls as plan ops; buffers come from the plan's arena."""

    def __init__(self, arena, T, ops):
        self.arena, self.T, self.ops = arena, T, ops
        self.dev = arena.dev
        self.dt = L.dtype_code(T)
        self.ws_need = 0
        self.packs = []
        self.shared = {}

    def buf(self, shape, dtype=None):
        return self.arena.new(shape, dtype or self.T)

    def scratch(self, name, shape):
        """A backward temporary: one per name, shared by all the layers."""
        if name not in self.shared:
            self.shared[name] = self.buf(shape)
        return self.shared[name]

    def weights(self, ws):
        """Compute-dtype copy of the fp32 masters, concatenated along dim 0; the casts are
        queued for the head of the forward (flush_weight_casts)."""
        dst = self.buf((sum(w.shape[0] for w in ws),) + tuple(ws[0].shape[1:]))
        o = 0
        for w in ws:
            self.cast_weight(w, dst[o:o + w.shape[0]])
            o += w.shape[0]
        return dst

    def seed(self, base, li):
        """A dropout seed fixed per plan op (every replay draws fresh masks from the device
        launch counter), as the signed 64-bit value a plan field holds."""
        v = L.dropout_seed(base + 7919 * li)
        return v - (1 << 64) if v >= (1 << 63) else v

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
        self.packs.append((w, dst, None, K, Cc, Cc, 1))

    def flush_weight_casts(self):
        if not self.packs:
            return
        head = _OpList()
        head.add(L.OP_CONV_PACK_MULTI, self.dt, **pack_multi_args(self.arena, self.packs))
        self.ops.prepend(head)

    def copy(self, src, dst, n):
        self.ops.add(L.OP_CAST, self.dt, i=(self.dt,), l=(n,), p=(src, dst))

    def axpby(self, n, a, x, b, y, out):
        self.ops.add(L.OP_AXPBY, i=(), l=(n,), f=(a, b), p=(x, y, out))

    def gemm(self, A, lda, akm, B, ldb, bkm, M, N, K, C, ldc, bias=None, act=0, preact=None,
             beta=0.0, residual=None):
        """C (compute dtype) = act(A B^T + bias) + beta C; residual: a [M][ldc] tensor of
        C's dtype added last (mmdx_gemm_res)."""
        n = L.lib().mmdx_gemm_workspace_size(self.dt, M, N, K)
        self.ops.timed(F.gemm_cost(M, N, K, self.dt, self.dt,
                                   1.0 if residual is not None else beta, act, preact),
                       L.OP_GEMM, dtype=self.dt,
                       i=(M, N, K, int(akm), int(bkm), self.dt, act),
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

    def ln_fwd(self, x, res, g, b, eps, rows, D, want_sum=True):
        """LayerNorm(x (+ res)) -> (y, x + res or None, mean, rstd)."""
        y = self.buf((rows, D))
        xsum = self.buf((rows, D)) if want_sum else None
        mean, rstd = self.buf((rows,), _F32), self.buf((rows,), _F32)
        self.ops.add(L.OP_LN_FWD, self.dt, i=(D,), l=(rows,), f=(eps,),
                     p=(x, res, g, b, y, xsum, mean, rstd))
        return y, xsum, mean, rstd

    def ln_fwd_drop(self, x, res, g, b, eps, p, seed, rows, D):
        """LayerNorm(dropout(x) + res) -> (y, xsum, mean, rstd, rng): rng is the dropout
        stream base buffer."""
        y, xsum = self.buf((rows, D)), self.buf((rows, D))
        mean, rstd = self.buf((rows,), _F32), self.buf((rows,), _F32)
        rng = self.buf((1,), torch.int64)
        self.ops.add(L.OP_LN_FWD_DROP, self.dt, i=(D,), l=(rows, seed), f=(eps, p),
                     p=(x, res, g, b, y, xsum, mean, rstd, L.rng_counter(self.dev), rng))
        return y, xsum, mean, rstd, rng

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


def _lay_out(G, base, table):
    """Append one layer's gradients (xlayers.bert_grads / vit_grads; base = index of the
    layer's first parameter) to the flat buffer -> {name: operand}."""
    gd = {}
    for name, idx, shape in table:
        if isinstance(idx, tuple):   # row blocks of one fused buffer
            off = G.take(shape)
            n = math.prod(shape) // len(idx)
            for j, i in enumerate(idx):
                G.items.append((base + i, (shape[0] // len(idx),) + shape[1:], off + j * n))
        else:
            off = G.take(shape, base + idx)
        gd[name] = G.ext(off)
    return gd


def _build(pl, params, npl, table, c, fwd, bwd, mask_fwd, mask_bwd):
    """Record a stack of layers: fwd(be, li, x, mask, layer params, c) -> (out, saved) and
    bwd(be, saved, dout, mask, gd, c) -> dx are the bodies the eager nodes run too.
    Forward externals: 0 = the stack input [M, D], 1 = mask.  Backward externals: 0 = the
    upstream gradient [M, D] (compute dtype), 1 = the gradient buffer, 2 = mask, 3 = the
    stack input."""
    nl = len(params) // npl
    rf = _Rec(pl.arena, pl.T, pl.fwd)
    x, saves = _Ext(0), []
    for li in range(nl):
        x, s = fwd(rf, li, x, mask_fwd, params[li * npl:(li + 1) * npl], c)
        saves.append(s)
    saves[0]["x"] = _Ext(3)
    pl.out = x
    rf.flush_weight_casts()

    rb = _Rec(pl.arena, pl.T, pl.bwd)
    G = pl.grads
    starts = [G.n]   # first gradient element of each layer, then the buffer's end
    gds = []
    for li in range(nl):   # gradient layout in forward order
        gds.append(_lay_out(G, li * npl, table))
        starts.append(G.n)
    d = _Ext(0)
    for li in range(nl - 1, -1, -1):
        d = bwd(rb, saves[li], d, mask_bwd, gds[li], c)
        pl.cut_after_layers(li, nl, starts.__getitem__)
    pl.dx = d
    pl.finish((rf, rb))
    return pl


# parameters per layer: bert.BertLayer.params() / vit.EncoderBlock order
_BERT_NP = 16
_VIT_NP = 12


def _build_bert(params, B, Ls, D, Hn, I, eps, p, pa, T, dev):
    c = SimpleNamespace(B=B, Ls=Ls, D=D, H=Hn, I=I, eps=eps, p=p, pa=pa)
    return _build(_StackPlan(dev, T), params, _BERT_NP, XL.bert_grads(D, I), c, XL.bert_fwd,
                  XL.bert_bwd, _Ext(1), _Ext(2))


def _build_vit(params, N, S, D, heads, I, eps, T, dev):
    c = SimpleNamespace(B=N, Ls=S, D=D, H=heads, I=I, eps=eps)
    return _build(_StackPlan(dev, T), params, _VIT_NP, XL.vit_grads(D, I), c, XL.vit_fwd,
                  XL.vit_bwd, None, None)


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
