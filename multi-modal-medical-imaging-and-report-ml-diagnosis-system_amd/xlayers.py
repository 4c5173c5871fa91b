"""The BERT layer and the ViT block, each written ONCE: forward and backward as plain
functions over a small recorder interface (buf, scratch, weights, seed, gemm,
gemm_wgrad_bias, attn_fwd / attn_bwd, ln_fwd / ln_fwd_drop / ln_bwd / ln_bwd_drop, axpby,
add).  Two back-ends implement it:

  Eager (here)   allocates with torch.empty and issues every call at once on the current
                 stream; behind bert._BertLayerFn / vit._VitBlockFn (inference, any forward
                 under no_grad, a frozen encoder parameter).
  xplan._Rec     appends the same calls as launch-plan ops over a buffer arena; behind the
                 benched C5 training step (xplan._build_bert / _build_vit).

Where the two paths differ (weight copies, dropout seeds, backward temporaries, what the
attention forward keeps) the difference is a back-end method, never a branch in a body.
A body takes the layer's dimensions as `c` (B, Ls, D, H, I, eps; BERT also p, pa: the
dropout probabilities in effect) and the gradient destinations as `gd` (name -> operand,
names and shapes from bert_grads / vit_grads).
"""
from __future__ import annotations

import math
import os

import torch

from . import _lib as L
from . import functional as F
from ._lib import call, ptr, stream

# ViT backward: residual-branch gradient added inside the LayerNorm backward (1, default) or
# by a separate add pass (0)
VIT_LN_ADDIN = os.environ.get("MMDX_VIT_LN_ADDIN", "1") == "1"
_F32 = torch.float32
_SEED = [0xB127]


class Eager:
    """Issues every call at once.  keep=False (nothing needs a gradient): the attention
    forward saves nothing and runs the non-flash kernel with a null probs pointer."""

    def __init__(self, T, dev, keep):
        self.T, self.dev, self.keep = T, dev, keep

    def buf(self, shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.T, device=self.dev)

    def scratch(self, name, shape):
        """A backward temporary: fresh per layer."""
        return torch.empty(shape, dtype=self.T, device=self.dev)

    def weights(self, ws):
        """Compute-dtype copy of the fp32 masters, concatenated along dim 0: cast per call."""
        return F.cat_cast(ws, self.T, self.dev) if len(ws) > 1 else F.cast(ws[0], self.T)

    def seed(self, base, li):
        """One increment of the module counter per active dropout site."""
        _SEED[0] += 1
        return L.dropout_seed(_SEED[0])

    def grad_bufs(self, table):
        return {name: self.buf(shape, _F32) for name, _, shape in table}

    def axpby(self, n, a, x, b, y, out):
        call("mmdx_axpby", n, a, ptr(x), b, ptr(y), ptr(out), stream())

    # same signatures as the recorder's: no wrapper in between (the compute dtype is the
    # A / dY operand's)
    gemm = staticmethod(F.gemm)
    gemm_wgrad_bias = staticmethod(F.gemm_wgrad_bias)
    attn_bwd = staticmethod(F.attention_bwd)

    def attn_fwd(self, qkv, mask, B, Ls, H, scale, p_drop, seed, counter, out):
        return F.attention_fwd(qkv, mask, B, Ls, H, scale, p_drop, seed, counter, out,
                               self.keep)

    def ln_fwd(self, x, res, g, b, eps, rows, D, want_sum=True):
        return F.ln_fwd(x, res, g, b, eps, want_sum)

    def ln_fwd_drop(self, x, res, g, b, eps, p, seed, rows, D):
        return F.ln_fwd_drop(x, res, g, b, eps, p, seed)

    def ln_bwd(self, xsum, dy, g, mean, rstd, rows, D, dx, dg, db, addin=None):
        F.ln_bwd(xsum, dy, g, mean, rstd, addin, out=(dx, dg, db))

    def ln_bwd_drop(self, xsum, dy, g, mean, rstd, p, rng, rows, D, dx, dx_drop, dg, db):
        F.ln_bwd_drop(xsum, dy, g, mean, rstd, p, rng, out=(dx, dx_drop, dg, db))

    def add(self, x, y, n, out):
        F.add(x, y, out)


def save(ctx, saved):
    """What a forward body returned, onto an autograd ctx: tensors through
    save_for_backward, the rest (None, the attention forward's tuple) as attributes."""
    ctx.names = [k for k, v in saved.items() if isinstance(v, torch.Tensor)]
    ctx.save_for_backward(*(saved[k] for k in ctx.names))
    ctx.rest = {k: v for k, v in saved.items() if k not in ctx.names}


def load(ctx):
    return dict(ctx.rest, **dict(zip(ctx.names, ctx.saved_tensors)))


def in_param_order(table, gd, n):
    """The gradients gd of one layer as a list in parameter order (n parameters)."""
    out = [None] * n
    for name, idx, shape in table:
        if isinstance(idx, tuple):
            r = shape[0] // len(idx)
            for j, i in enumerate(idx):
                out[i] = gd[name][j * r:(j + 1) * r]
        else:
            out[idx] = gd[name]
    return out


# ------------------------------------------------------------------------ BERT layer
def bert_grads(D, I):
    """(name, index in bert.BertLayer.params() order, shape) of one layer's gradients, in
    gradient-buffer order; a tuple of indices: equal row blocks of one fused buffer."""
    return (("wqkv", (0, 2, 4), (3 * D, D)), ("bqkv", (1, 3, 5), (3 * D,)),
            ("wo", 6, (D, D)), ("bo", 7, (D,)), ("g1", 8, (D,)), ("b1", 9, (D,)),
            ("wi", 10, (I, D)), ("bi", 11, (I,)), ("wo2", 12, (D, I)), ("bo2", 13, (D,)),
            ("g2", 14, (D,)), ("b2", 15, (D,)))


def _ln_drop(be, li, base, x, res, g, b, c, M):
    """LayerNorm(dropout(x) + res), the dropout inside the LayerNorm pass (no dropped
    tensor, no mask: the backward redraws the keep bits from rng) -> (y, xsum, mean, rstd,
    rng or None)."""
    if c.p > 0:
        return be.ln_fwd_drop(x, res, g, b, c.eps, c.p, be.seed(base, li), M, c.D)
    return (*be.ln_fwd(x, res, g, b, c.eps, M, c.D), None)


def bert_fwd(be, li, x, mask, params, c):
    """One transformers BertLayer (post-LN), layer li of its stack, on x [M, D] ->
    (output [M, D], what bert_bwd needs)."""
    wq, bq, wk, bk, wv, bv, wo, bo, g1, b1, wi, bi, wo2, bo2, g2, b2 = params
    B, Ls, D, I = c.B, c.Ls, c.D, c.I
    M = B * Ls
    wqkv = be.weights((wq, wk, wv))
    bqkv = be.buf((3 * D,), _F32)
    for j, bb in enumerate((bq, bk, bv)):
        be.axpby(D, 1.0, bb, 0.0, None, bqkv[j * D:(j + 1) * D])
    qkv = be.buf((M, 3 * D))
    be.gemm(x, D, True, wqkv, D, True, M, 3 * D, D, qkv, 3 * D, bias=bqkv)
    att = be.buf((M, D))
    # BertSelfAttention's dropout on attention_probs (train mode), fused in the kernel
    attn = be.attn_fwd(qkv, mask, B, Ls, c.H, 1.0 / math.sqrt(D // c.H), c.pa,
                       be.seed(0xA770, li) if c.pa > 0 else 0, L.rng_counter(be.dev), att)
    woc = be.weights((wo,))
    a = be.buf((M, D))
    be.gemm(att, D, True, woc, D, True, M, D, D, a, D, bias=bo)
    # BertSelfOutput: LayerNorm(dropout(a) + x)
    h1, xs1, mu1, rs1, m1 = _ln_drop(be, li, 0xD401, a, x, g1, b1, c, M)
    wic = be.weights((wi,))
    f, pre = be.buf((M, I)), be.buf((M, I))
    be.gemm(h1, D, True, wic, D, True, M, I, D, f, I, bias=bi, act=L.ACT_GELU, preact=pre)
    wo2c = be.weights((wo2,))
    f2 = be.buf((M, D))
    be.gemm(f, I, True, wo2c, I, True, M, D, I, f2, D, bias=bo2)
    # BertOutput: LayerNorm(dropout(f2) + h1)
    h2, xs2, mu2, rs2, m2 = _ln_drop(be, li, 0xD402, f2, h1, g2, b2, c, M)
    return h2, dict(x=x, wqkv=wqkv, qkv=qkv, attn=attn, att=att, woc=woc, xs1=xs1, mu1=mu1,
                    rs1=rs1, g1=g1, h1=h1, wic=wic, pre=pre, f=f, wo2c=wo2c, xs2=xs2, mu2=mu2,
                    rs2=rs2, g2=g2, m1=m1, m2=m2)


def bert_bwd(be, s, dh, mask, gd, c):
    """Backward of bert_fwd: dh = d(output) [M, D] -> d(x); the parameter gradients go to
    gd.  Residual gradients are summed inside GEMM epilogues (beta = 1)."""
    B, Ls, D, I = c.B, c.Ls, c.D, c.I
    M = B * Ls
    # LN2: X = d(f2 + h1), dX2 = d(f2)
    X = dX2 = be.scratch("X", (M, D))
    if s["m2"] is not None:
        dX2 = be.scratch("DX2", (M, D))
        be.ln_bwd_drop(s["xs2"], dh, s["g2"], s["mu2"], s["rs2"], c.p, s["m2"], M, D, X, dX2,
                       gd["g2"], gd["b2"])
    else:
        be.ln_bwd(s["xs2"], dh, s["g2"], s["mu2"], s["rs2"], M, D, X, gd["g2"], gd["b2"])
    # FFN down: f2 = f Wo2^T + bo2
    # dpre = (dX2 Wo2) * gelu'(pre): the GELU backward in the GEMM epilogue
    dpre = be.scratch("dpre", (M, I))
    be.gemm(dX2, D, True, s["wo2c"], I, False, M, I, D, dpre, I, act=L.ACT_GELU_BWD,
            preact=s["pre"])
    be.gemm_wgrad_bias(dX2, D, s["f"], I, D, I, M, gd["wo2"], I, gd["bo2"])
    be.gemm_wgrad_bias(dpre, I, s["h1"], D, I, D, M, gd["wi"], D, gd["bi"])
    # X := dpre Wi + X  (residual into h1)
    be.gemm(dpre, I, True, s["wic"], D, False, M, D, I, X, D, beta=1.0)
    # LN1: Y = d(a + x), dY1 = d(a)
    Y = dY1 = be.scratch("Y", (M, D))
    if s["m1"] is not None:
        dY1 = be.scratch("DY1", (M, D))
        be.ln_bwd_drop(s["xs1"], X, s["g1"], s["mu1"], s["rs1"], c.p, s["m1"], M, D, Y, dY1,
                       gd["g1"], gd["b1"])
    else:
        be.ln_bwd(s["xs1"], X, s["g1"], s["mu1"], s["rs1"], M, D, Y, gd["g1"], gd["b1"])
    datt = be.scratch("datt", (M, D))
    be.gemm(dY1, D, True, s["woc"], D, False, M, D, D, datt, D)
    be.gemm_wgrad_bias(dY1, D, s["att"], D, D, D, M, gd["wo"], D, gd["bo"])
    dqkv = be.scratch("dqkv", (M, 3 * D))
    be.attn_bwd(s["qkv"], s["attn"], s["att"], datt, mask, B, Ls, c.H,
                1.0 / math.sqrt(D // c.H), c.pa, dqkv)
    be.gemm_wgrad_bias(dqkv, 3 * D, s["x"], D, 3 * D, D, M, gd["wqkv"], D, gd["bqkv"])
    # Y := dqkv Wqkv + Y  (residual into x)
    be.gemm(dqkv, 3 * D, True, s["wqkv"], D, False, M, D, 3 * D, Y, D, beta=1.0)
    return Y


# ------------------------------------------------------------------------ ViT block
def vit_grads(D, I):
    """As bert_grads, in vit.EncoderBlock order."""
    return tuple((name, j, shape) for j, (name, shape) in enumerate((
        ("g1", (D,)), ("b1", (D,)), ("w_in", (3 * D, D)), ("b_in", (3 * D,)),
        ("w_out", (D, D)), ("b_out", (D,)), ("g2", (D,)), ("b2", (D,)), ("w1", (I, D)),
        ("bb1", (I,)), ("w2", (D, I)), ("bb2", (D,)))))


def vit_fwd(be, li, x, mask, params, c):
    """One torchvision EncoderBlock (pre-LN): x += MHA(LN1 x); x += MLP(LN2 x), on x [M, D]
    -> (output [M, D], what vit_bwd needs).  Same signature as bert_fwd; mask is None."""
    g1, b1, w_in, b_in, w_out, b_out, g2, b2, w1, bb1, w2, bb2 = params
    B, Ls, D, I = c.B, c.Ls, c.D, c.I
    M = B * Ls
    u1, _, mu1, rs1 = be.ln_fwd(x, None, g1, b1, c.eps, M, D, want_sum=False)
    wqkv = be.weights((w_in,))
    qkv = be.buf((M, 3 * D))
    be.gemm(u1, D, True, wqkv, D, True, M, 3 * D, D, qkv, 3 * D, bias=b_in)
    att = be.buf((M, D))
    attn = be.attn_fwd(qkv, mask, B, Ls, c.H, 1.0 / math.sqrt(D // c.H), 0.0, 0, None, att)
    woc = be.weights((w_out,))
    o = be.buf((M, D))
    be.gemm(att, D, True, woc, D, True, M, D, D, o, D, bias=b_out)
    # a = x + o and u2 = LN2(a) in one pass
    u2, a, mu2, rs2 = be.ln_fwd(o, x, g2, b2, c.eps, M, D)
    w1c = be.weights((w1,))
    f, pre = be.buf((M, I)), be.buf((M, I))
    be.gemm(u2, D, True, w1c, D, True, M, I, D, f, I, bias=bb1, act=L.ACT_GELU, preact=pre)
    w2c = be.weights((w2,))
    out = be.buf((M, D))   # out = a + f W2^T + b2, the residual read by the epilogue
    be.gemm(f, I, True, w2c, I, True, M, D, I, out, D, bias=bb2, residual=a)
    return out, dict(x=x, u1=u1, mu1=mu1, rs1=rs1, g1=g1, wqkv=wqkv, qkv=qkv, attn=attn,
                     att=att, woc=woc, a=a, u2=u2, mu2=mu2, rs2=rs2, g2=g2, w1c=w1c, pre=pre,
                     f=f, w2c=w2c)


def _ln_bwd_plus(be, xs, dy, g, mean, rstd, M, D, branch, name, dg, db):
    """branch + LN'(dy) into scratch `name`: the residual branch's gradient added inside the
    LayerNorm backward (mmdx_layernorm_bwd_residual) or, MMDX_VIT_LN_ADDIN=0, by a separate
    add pass.  Within the box-to-box spread on C5: -0.8 % and +1.2 % against the add pass on
    two boxes, paired (profiles/r04_c5_ab_ln_addin.txt)."""
    out = be.scratch(name, (M, D))
    if VIT_LN_ADDIN:
        be.ln_bwd(xs, dy, g, mean, rstd, M, D, out, dg, db, addin=branch)
    else:
        ln = be.scratch("da_ln", (M, D))
        be.ln_bwd(xs, dy, g, mean, rstd, M, D, ln, dg, db)
        be.add(branch, ln, M * D, out)
    return out


def vit_bwd(be, s, dO, mask, gd, c):
    """Backward of vit_fwd: dO = d(output) [M, D] -> d(x); the parameter gradients go to gd."""
    B, Ls, D, I = c.B, c.Ls, c.D, c.I
    M = B * Ls
    # dpre = (dO W2) * gelu'(pre): the GELU backward in the GEMM epilogue
    dpre = be.scratch("dpre", (M, I))
    be.gemm(dO, D, True, s["w2c"], I, False, M, I, D, dpre, I, act=L.ACT_GELU_BWD,
            preact=s["pre"])
    be.gemm_wgrad_bias(dO, D, s["f"], I, D, I, M, gd["w2"], I, gd["bb2"])
    be.gemm_wgrad_bias(dpre, I, s["u2"], D, I, D, M, gd["w1"], D, gd["bb1"])
    du2 = be.scratch("du2", (M, D))
    be.gemm(dpre, I, True, s["w1c"], D, False, M, D, I, du2, D)
    # da = dO + LN2'(du2)
    da = _ln_bwd_plus(be, s["a"], du2, s["g2"], s["mu2"], s["rs2"], M, D, dO, "DA", gd["g2"],
                      gd["b2"])
    datt = be.scratch("datt", (M, D))
    be.gemm(da, D, True, s["woc"], D, False, M, D, D, datt, D)
    be.gemm_wgrad_bias(da, D, s["att"], D, D, D, M, gd["w_out"], D, gd["b_out"])
    dqkv = be.scratch("dqkv", (M, 3 * D))
    be.attn_bwd(s["qkv"], s["attn"], s["att"], datt, mask, B, Ls, c.H,
                1.0 / math.sqrt(D // c.H), 0.0, dqkv)
    be.gemm_wgrad_bias(dqkv, 3 * D, s["u1"], D, 3 * D, D, M, gd["w_in"], D, gd["b_in"])
    du1 = be.scratch("du1", (M, D))
    be.gemm(dqkv, 3 * D, True, s["wqkv"], D, False, M, D, 3 * D, du1, D)
    # dx = da + LN1'(du1)
    return _ln_bwd_plus(be, s["x"], du1, s["g1"], s["mu1"], s["rs1"], M, D, da, "DX", gd["g1"],
                        gd["b1"])
