"""ResNet-18/50 image trunk on the mmdx HIP kernels (NHWC, implicit-GEMM MFMA convs).

Module tree and parameter names mirror torchvision's resnet (v1.5: stride on the 3x3
conv) exactly as ImageEncoderCNN wraps it — `nn.Sequential(*list(m.children())[:-1])`
(training_pipeline.py:183) — so `backbone.0.weight`, `backbone.4.0.conv1.weight`,
`backbone.4.0.downsample.1.running_mean`, ... round-trip with the reference's state_dict.

Execution does NOT walk the module tree: the whole trunk is one autograd node whose
forward and backward are hand-sequenced C-ABI calls (conv -> BN(+res)(+ReLU) per unit),
with the residual-path gradient summed inside the dgrad epilogue (beta = 1).
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
import math
import weakref

import torch
import torch.nn as nn

from . import _lib as L
from ._lib import call, ptr, stream
from .plan import (MAX_PLAN_KEYS, WS, WS2, _Arena, _Ext, _OpList, _Token,  # noqa: F401
                   pack_multi_args, plan_cache_get)

_VEC = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}


class _NoTimer:
    active = False

    def __call__(self, name):
        return self

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


# bench.py installs a HIP-event timer here to measure the implicit-GEMM conv launches: when
# `active`, `take(names)` hands out a (start, end) event pair per conv op of a plan run.
CONV_TIMER = _NoTimer()


class LaunchCost(tuple):
    """Tag of a timed launch: (kind, algorithmic FLOPs, algorithmic HBM bytes — every tensor
    it must read or write touched once).  bench.py prices each launch against its own roof,
    max(FLOPs / MFMA peak, bytes / HBM bandwidth)."""
    __slots__ = ()

    def __new__(cls, kind, flops, nbytes, label=""):
        return tuple.__new__(cls, (kind, int(flops), int(nbytes), label))

    kind = property(lambda s: s[0])
    flops = property(lambda s: s[1])
    nbytes = property(lambda s: s[2])


def conv_cost(kind, conv, N, H, W, P, Q, elt, extra_read=0):
    """LaunchCost of one conv launch over an N x H x W input (true channels, unpadded):
    fwd x + w + y; dgrad dy + w + dx (+ extra_read: a tensor the epilogue adds); wgrad
    x + dy + dw (fp32)."""
    k = conv.kernel_size
    macs = N * P * Q * conv.out_channels * conv.in_channels * k * k
    x = N * H * W * conv.in_channels * elt
    y = N * P * Q * conv.out_channels * elt
    w = conv.out_channels * conv.in_channels * k * k
    b = {"fwd": x + w * elt + y, "dgrad": y + w * elt + x + extra_read,
         "wgrad": x + y + w * 4}[kind]
    return LaunchCost(kind, 2 * macs, b,
                      f"C{conv.in_channels}->K{conv.out_channels} {k}x{k}/{conv.stride} "
                      f"in{N}x{H}x{W}")


# ----------------------------------------------------------------------------- modules
class Conv2d(nn.Module):
    def __init__(self, cin, cout, k, stride=1, padding=0):
        super().__init__()
        self.in_channels, self.out_channels = cin, cout
        self.kernel_size, self.stride, self.padding = k, stride, padding
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        # torchvision resnet init: kaiming_normal_(mode="fan_out", nonlinearity="relu")
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, "
                f"stride={self.stride}, padding={self.padding}")


class BatchNorm2d(nn.Module):
    def __init__(self, c, eps=1e-5, momentum=0.1):
        super().__init__()
        self.num_features, self.eps, self.momentum = c, eps, momentum
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))


class ReLU(nn.Module):
    pass


class MaxPool2d(nn.Module):
    def __init__(self, k=3, stride=2, padding=1):
        super().__init__()
        self.kernel_size, self.stride, self.padding = k, stride, padding


class AdaptiveAvgPool2d(nn.Module):
    def __init__(self, out=1):
        super().__init__()
        self.output_size = out


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 1)
        self.bn1 = BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, stride, 1)
        self.bn2 = BatchNorm2d(planes)
        self.conv3 = Conv2d(planes, planes * 4, 1)
        self.bn3 = BatchNorm2d(planes * 4)
        self.relu = ReLU()
        self.downsample = downsample
        self.stride = stride

    def units(self):
        return [(self.conv1, self.bn1, True), (self.conv2, self.bn2, True),
                (self.conv3, self.bn3, True)]


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 3, stride, 1)
        self.bn1 = BatchNorm2d(planes)
        self.relu = ReLU()
        self.conv2 = Conv2d(planes, planes, 3, 1, 1)
        self.bn2 = BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def units(self):
        return [(self.conv1, self.bn1, True), (self.conv2, self.bn2, True)]


ARCHS = {
    "resnet18": (BasicBlock, [2, 2, 2, 2]),
    "resnet34": (BasicBlock, [3, 4, 6, 3]),
    "resnet50": (Bottleneck, [3, 4, 6, 3]),
    "resnet101": (Bottleneck, [3, 4, 23, 3]),
}


def _make_layer(block, inplanes, planes, blocks, stride):
    downsample = None
    if stride != 1 or inplanes != planes * block.expansion:
        downsample = nn.Sequential(Conv2d(inplanes, planes * block.expansion, 1, stride),
                                   BatchNorm2d(planes * block.expansion))
    layers = [block(inplanes, planes, stride, downsample)]
    inplanes = planes * block.expansion
    for _ in range(1, blocks):
        layers.append(block(inplanes, planes))
    return nn.Sequential(*layers), inplanes


class ResNetTrunk(nn.Sequential):
    """`Sequential(conv1, bn1, relu, maxpool, layer1..4, avgpool)`; forward = fused engine.

    Input: fp32 NCHW images [B,3,H,W] (the tensor image_transfom_into_tensor makes,
    TP:112-119), or an already-converted NHWC compute-dtype tensor.  Output: [B, feat, 1, 1]
    like torchvision's trunk (flatten(1) is applied by the caller, TP:281/288).
    """

    def __init__(self, arch="resnet50"):
        block, counts = ARCHS[arch]
        conv1 = Conv2d(3, 64, 7, 2, 3)
        bn1 = BatchNorm2d(64)
        inplanes = 64
        l1, inplanes = _make_layer(block, inplanes, 64, counts[0], 1)
        l2, inplanes = _make_layer(block, inplanes, 128, counts[1], 2)
        l3, inplanes = _make_layer(block, inplanes, 256, counts[2], 2)
        l4, inplanes = _make_layer(block, inplanes, 512, counts[3], 2)
        super().__init__(conv1, bn1, ReLU(), MaxPool2d(), l1, l2, l3, l4, AdaptiveAvgPool2d(1))
        self.arch = arch
        self.feat_dim = inplanes
        self.compute_dtype = torch.float32
        # torchvision zero-inits no residual BN by default; bn weights 1, biases 0 (above).

    # parameters in engine order (conv.weight, bn.weight, bn.bias per unit)
    def engine_params(self):
        ps = [self[0].weight, self[1].weight, self[1].bias]
        for layer in list(self)[4:8]:
            for blk in layer:
                for conv, bn, _ in blk.units():
                    ps += [conv.weight, bn.weight, bn.bias]
                if blk.downsample is not None:
                    ps += [blk.downsample[0].weight, blk.downsample[1].weight,
                           blk.downsample[1].bias]
        return ps

    def forward(self, x):
        params = self.engine_params()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        # torch convs accept any strides (e.g. a channels-last view from a PIL transform)
        feats = _TrunkFn.apply(x.contiguous(), self, need_grad, *params)
        return feats.view(feats.shape[0], feats.shape[1], 1, 1)

    @torch.no_grad()
    def forward_features(self, x):
        """(feats [B, K], fmap [B, H, W, K]) in the compute dtype: the pooled features `forward`
        returns and the layer4 activation they are the spatial mean of (NHWC), for Grad-CAM
        (explain.py).  Inference only: eval mode, no autograd graph; the same plan and plan
        cache entry as an eval-mode `forward` under no_grad, both outputs cloned out of its
        arena."""
        if self.training:
            raise RuntimeError("forward_features is an eval-mode call: trunk.eval() first")
        plan = _run_fwd_plan(x.contiguous(), self, False, self.engine_params())
        return plan.feats.clone(), plan.top.clone()


# ----------------------------------------------------------------------------- engine
# The trunk is executed from launch plans (plan.py; include/mmdx.h, csrc/plan.cpp): the
# forward and the backward of one (batch shape, dtype, mode, parameter set) are recorded once
# as op lists over a buffer arena, then every step replays each with ONE C call.  _Rec
# records one op per method; the _record_* / _block_* functions below sequence them and
# _Plan.__init__ strings those together.  tools/plan_dump.py writes a recorded plan as
# pointer-free text, to diff the planner of two revisions op for op (on the CPU).

def _desc(N, H, W, C, conv):
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    P = (H + 2 * p - k) // s + 1
    Q = (W + 2 * p - k) // s + 1
    return L.ConvDesc(N, H, W, C, conv.out_channels, k, k, s, s, p, p, P, Q)


@dataclasses.dataclass(eq=False)
class _Unit:
    """One conv + BN(+res)(+ReLU) of a recorded plan: what it is made of, then the arena
    buffers its forward and its backward fill in (read by the per-launch parity test,
    tests/test_trunk_launches_gpu.py).  A field that does not apply is None."""
    conv: Conv2d
    bn: BatchNorm2d
    relu: bool
    d: L.ConvDesc
    in_hw: tuple          # true input H, W (the pair stem's d is over the pixel-pair image)
    elt: int              # bytes per element of the compute dtype
    x: object             # input: an arena buffer, or _Ext (the trunk input itself)
    res: object = None    # residual added before the ReLU
    pair: bool = False    # the stem as a conv over pixel pairs
    # forward
    y: object = None      # raw conv output (folded eval: never materialised)
    out: object = None    # post-activation tensor (statistics-only BN: never written)
    mean: object = None
    rstd: object = None
    wc: object = None     # CRSK weight copy the dgrad reads
    rmask: object = None  # 1-bit ReLU mask of a residual unit
    # backward
    dconv: object = None      # the BN backward's output, read by wgrad and dgrad
    dout: object = None       # the BN backward's upstream gradient ...
    dout_mask: object = None  # ... and the ReLU bit mask applied to it on the fly
    bwd_kind: str = None      # "plain" / "relu" / "res" / "masked" / "pool"
    dx: object = None         # the tensor the dgrad wrote or accumulated onto

    def cost(self, kind, extra=0):
        d = self.d
        return conv_cost(kind, self.conv, d.N, self.in_hw[0], self.in_hw[1], d.P, d.Q,
                         self.elt, extra)

    def in_bytes(self):
        d = self.d
        return d.N * d.H * d.W * d.C * self.elt


class _Rec:
    """Records the trunk's C-ABI calls as plan ops, one method per op, and holds what a
    recording shares: the arena, the two op lists, the dtype and mode, the workspace need per
    stream, the weights awaiting the multi-tensor pack and the gradient layout."""

    def __init__(self, trunk, N, T, train, keep, dev):
        self.N, self.T, self.dt, self.vec = N, T, L.dtype_code(T), _VEC[T]
        self.train, self.keep = train, keep
        self.fold = not train and not keep   # eval-mode BN folded into the conv epilogue
        self.arena = _Arena(dev)
        self.fw = _OpList()
        self.bw = _OpList() if keep else None
        self.ws_need = [0, 0]  # per stream: 0 = main, 1 = weight-gradient side stream
        self.packs = []
        self.ev_pack = None
        # the flat fp32 gradient arena, in engine_params order
        self.grad_off = {}
        off = 0
        for prm in trunk.engine_params():
            self.grad_off[id(prm)] = off
            off += (prm.numel() * 4 + 15) // 16 * 16  # 16-B aligned, dense for ResNets
        self.grad_bytes = off

    def buf(self, shape, dtype=None):
        return self.arena.new(shape, dtype or self.T)

    def ws(self, n, st=0):
        """The workspace operand of an op on stream `st` that needs n bytes."""
        self.ws_need[st] = max(self.ws_need[st], int(n))
        return WS2 if st else WS

    def g(self, prm):
        return _Ext(1, self.grad_off[id(prm)])

    def sync(self, ops, src, dst):
        """Stream `dst` waits for what stream `src` has been given so far."""
        ev = self.arena.event()
        ops.add(L.OP_SIGNAL, p=(ev,), stream=src)
        ops.add(L.OP_WAIT, p=(ev,), stream=dst)

    def unit(self, conv, bn, relu, x, hwc, res=None, pair=None):
        """A unit over the N x H x W x C input `x` (`pair`: the pixel-pair stem's desc)."""
        H, W, C = hwc
        d = pair if pair is not None else _desc(self.N, H, W, C, conv)
        return _Unit(conv, bn, relu, d, (H, W), self.T.itemsize, x, res, pair is not None)

    # ---- forward
    def _weights(self, u):
        """u's KRSC weights (returned) and, for a backward, the dgrad's CRSK copy (u.wc)."""
        d, conv = u.d, u.conv
        K, k, cm = conv.out_channels, conv.kernel_size, conv.in_channels
        wk = self.buf((K, d.R, d.S, d.C))
        if u.pair:  # stem over pixel pairs: its own weight map, no dgrad copy
            self.fw.add(L.OP_STEM_PAIR_PACK, i=(K, cm, k, k), p=(conv.weight, wk))
            return wk
        u.wc = self.buf((d.C, k, k, K)) if self.keep else None
        if d.C == cm:  # packed by the plan's single multi-tensor pack launch (pack_at_head)
            self.packs.append((conv.weight, wk, u.wc, K, d.C, cm, k * k))
        else:  # channel-padded input (fp32 stem): its own pack
            self.fw.add(L.OP_CONV_PACK, self.dt, i=(cm,), p=(conv.weight, wk, u.wc), d=d)
        return wk

    def conv_fwd(self, u, st=0):
        """u's conv on stream `st`; returns the BN statistics its epilogue leaves:
        (partials, slabs, rows per slab)."""
        d = u.d
        u.y = self.buf((d.N, d.P, d.Q, d.K))
        nstat = L.lib().mmdx_conv_fwd_stat_blocks(d) if self.train else 0
        part = self.buf((d.K, nstat, 2), torch.float32) if self.train else None
        wk = self._weights(u)
        rpb = L.lib().mmdx_conv_fwd_stat_rows(d)  # rows per statistics slab (part)
        self.fw.timed(u.cost("fwd"), L.OP_CONV_FWD, stream=st, dtype=self.dt,
                      i=(rpb if self.train else 0,), p=(u.x, wk, u.y, part), d=d)
        return part, nstat, rpb

    def bn_fwd(self, u, stats, out, st=0):
        """Statistics (train: from the conv's partials), then BN(+u.res)(+ReLU) into `out`.
        out None: the statistics only — u's consumer normalises on the fly and the
        post-activation tensor is never written."""
        part, nstat, rpb = stats
        d, bn = u.d, u.bn
        rows = d.N * d.P * d.Q
        u.out = out
        u.mean = self.buf((d.K,), torch.float32)
        u.rstd = self.buf((d.K,), torch.float32)
        # a residual unit's backward needs its ReLU mask: kept as 1 bit per element
        # (one byte per 16-B channel vector) instead of re-reading its output
        if self.keep and u.relu and u.res is not None and out is not None:
            u.rmask = self.buf((rows, d.K // self.vec), torch.uint8)
        wsn = L.lib().mmdx_bn_workspace_size(rows, d.K)
        self.fw.add(L.OP_BN_FWD, self.dt, i=(int(self.train), d.K, nstat, int(u.relu)),
                    l=(rows, rpb, wsn), f=(bn.momentum, bn.eps), stream=st,
                    p=(u.y, part, bn.weight, bn.bias, bn.running_mean, bn.running_var, u.mean,
                       u.rstd, u.res, out, self.ws(wsn, st), u.rmask))

    def conv_bneval(self, u, st=0):
        """eval forward without a backward (inference, frozen phase 1): BN on running
        statistics (+residual)(+ReLU) applied in the conv epilogue; y is never
        materialised and no bn_apply pass runs"""
        d, bn = u.d, u.bn
        u.out = self.buf((d.N, d.P, d.Q, d.K))
        wk = self._weights(u)
        self.fw.timed(u.cost("fwd"), L.OP_CONV_FWD_BNEVAL, stream=st, dtype=self.dt,
                      i=(int(u.relu),), f=(bn.eps,),
                      p=(u.x, wk, u.out, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                         u.res), d=d)

    def pack_join(self):
        """The multi-tensor weight pack (pack_at_head) runs on the side stream beside the stem
        when the stem's weights have their own pack on the main stream; the main stream joins
        it here, before the first conv that reads a packed weight (70 us off the critical
        path).  A stem weight already in the multi-tensor pack: the pack stays on the main
        stream, nothing to join."""
        if not self.packs:
            self.ev_pack = self.arena.event()
            self.fw.add(L.OP_WAIT, p=(self.ev_pack,), stream=0)

    def pack_at_head(self):
        """every conv weight packed (KRSC fwd + CRSK dgrad copies) in ONE launch, first op"""
        args = pack_multi_args(self.arena, self.packs)
        st = 0 if self.ev_pack is None else 1
        head = _OpList()
        if st:  # side stream: after whatever the main stream ran before the plan
            self.sync(head, 0, 1)
        head.add(L.OP_CONV_PACK_MULTI, self.dt, stream=st, **args)
        if st:
            head.add(L.OP_SIGNAL, p=(self.ev_pack,), stream=1)
        self.fw.prepend(head)

    # ---- backward (ext: 0 = dfeats in T, 1 = gradient arena base, 2 = trunk input x0)
    def _dconv(self, u, dout, kind, mask=None):
        # kept for the per-launch parity test (tests/test_trunk_launches_gpu.py):
        # the BN backward's upstream gradient and where its ReLU mask comes from
        u.dconv = self.buf(tuple(u.y.shape))
        u.dout, u.dout_mask, u.bwd_kind = dout, mask, kind
        return u.dconv

    def bn_bwd(self, u, dout, stats=None, want_dres=False):
        """BN(+res)(+ReLU) backward of u.  ReLU mask: a residual unit's bit mask from the
        forward (else its output); no residual: recomputed from y.  `stats`: u's partials
        (buffer, tiles), already made by the dgrad that produced `dout`.  `want_dres`: the
        residual's gradient written out too (returned)."""
        d, bn = u.d, u.bn
        rows = d.N * d.P * d.Q
        dconv = self._dconv(u, dout, "res" if u.res is not None else
                            "relu" if u.relu else "plain")
        dres = self.buf(tuple(u.y.shape)) if want_dres else None
        out = u.out if u.res is not None and u.rmask is None else None
        sp, sb = stats if stats is not None else (None, 0)
        wsn = L.lib().mmdx_bn_workspace_size(rows, d.K)
        self.bw.add(L.OP_BN_BWD, self.dt, i=(int(self.train), d.K, int(u.relu), sb),
                    l=(rows, wsn, sp.data_ptr() if sp is not None else 0,
                       u.rmask.data_ptr() if u.rmask is not None else 0), f=(0.0,),
                    p=(u.y, out, dout, bn.weight, bn.bias, u.mean, u.rstd, dconv, dres,
                       self.g(bn.weight), self.g(bn.bias), self.ws(wsn)))
        return dres

    def bn_bwd_masked(self, u, dout, mask):
        """a downsample BN: its upstream gradient is the residual unit's dout with that
        unit's ReLU bit mask applied on the fly (mmdx_bn_bwd_masked_dy)"""
        d, bn = u.d, u.bn
        rows = d.N * d.P * d.Q
        dconv = self._dconv(u, dout, "masked", mask)
        wsn = L.lib().mmdx_bn_workspace_size(rows, d.K)
        self.bw.add(L.OP_BN_BWD_MASKED_DY, self.dt, i=(int(self.train), d.K), l=(rows, wsn),
                    f=(0.0,),
                    p=(u.y, dout, mask, bn.weight, bn.bias, u.mean, u.rstd, dconv,
                       self.g(bn.weight), self.g(bn.bias), self.ws(wsn)))

    def bn_bwd_pool(self, u, dout, argmax, pool):
        """`dout` is the stem pool's OUTPUT gradient: the BN backward gathers
        dL/d(pool input) through the pool's argmax itself (mmdx_bn_bwd_pool)"""
        pN, pH, pW, pC, pk, ps_, pp, pP, pQ = pool
        d, bn = u.d, u.bn
        dconv = self._dconv(u, dout, "pool")
        wsn = L.lib().mmdx_bn_workspace_size(d.N * d.P * d.Q, d.K)
        self.bw.add(L.OP_BN_BWD_POOL, self.dt,
                    i=(int(self.train), pN, pH, pW, pC, int(u.relu), pP, pQ),
                    l=(wsn, pk, ps_, pp), f=(0.0,),
                    p=(u.y, argmax, dout, bn.weight, bn.bias, u.mean, u.rstd, dconv,
                       self.g(bn.weight), self.g(bn.bias), self.ws(wsn)))

    def bn_bwd_pair(self, u, v, dout):
        """bn3 (u) and the downsample BN (v) read the same masked gradient — `dout` under
        u's ReLU bit mask: one reduce, one finalize and one apply for both
        (mmdx_bn_bwd_pair)"""
        d = u.d
        rows = d.N * d.P * d.Q
        assert u.rmask is not None and tuple(v.y.shape) == tuple(u.y.shape)
        dconv = self._dconv(u, dout, "res")
        dconv_b = self._dconv(v, dout, "masked", u.rmask)
        wsn = L.lib().mmdx_bn_pair_workspace_size(rows, d.K)
        tab = (ctypes.c_void_p * 8)(*[t.data_ptr() for w in (u, v) for t in
                                      (w.bn.weight, w.bn.bias, w.mean, w.rstd)])
        self.arena.bufs.append(tab)  # host table the op points at: lives with the plan
        self.bw.add(L.OP_BN_BWD_PAIR, self.dt, i=(int(self.train), d.K), l=(rows, wsn),
                    f=(0.0,),
                    p=(dout, u.rmask, u.y, dconv, self.g(u.bn.weight), self.g(u.bn.bias),
                       v.y, dconv_b, self.g(v.bn.weight), self.g(v.bn.bias), self.ws(wsn),
                       ctypes.addressof(tab)))

    def wgrad(self, u):
        """u's weight gradient on the side stream (which already waits for u's dconv)."""
        d, cv = u.d, u.conv
        wsn = L.lib().mmdx_conv_wgrad_workspace_size(self.dt, d)
        x = _Ext(2) if isinstance(u.x, _Ext) else u.x
        # pair stem: the pair-conv gradient [K][8][R][S2], then mapped to the master layout
        dw = self.buf((d.K, d.C, d.R, d.S), torch.float32) if u.pair else self.g(cv.weight)
        self.bw.timed(u.cost("wgrad"), L.OP_CONV_WGRAD, stream=1, dtype=self.dt,
                      i=(d.C if u.pair else cv.in_channels,), l=(wsn,), f=(0.0,),
                      p=(x, u.dconv, dw, self.ws(wsn, 1)), d=d)
        if u.pair:
            self.bw.add(L.OP_STEM_PAIR_GRAD, stream=1,
                        i=(d.K, cv.in_channels, cv.kernel_size, cv.kernel_size), f=(0.0,),
                        p=(dw, self.g(cv.weight)))

    def wgrads_after_bn(self, *units):
        """one event after the BN backward(s): the side stream's wgrads wait on it"""
        self.sync(self.bw, 0, 1)
        for u in units:
            self.wgrad(u)

    def dx_buf(self, u):
        d = u.d
        return self.buf((d.N, d.H, d.W, d.C))

    def dgrad(self, u, dx, beta):
        """dx = dgrad(u) + beta dx"""
        self.bw.timed(u.cost("dgrad", u.in_bytes() if beta else 0), L.OP_CONV_DGRAD,
                      dtype=self.dt, f=(beta,), p=(u.dconv, u.wc, dx), d=u.d)
        u.dx = dx

    def dgrad_accmask(self, u, dx, src, mask):
        """dx = dgrad(u) + (ReLU bit ? src : 0)"""
        xb = u.in_bytes()
        self.bw.timed(u.cost("dgrad", xb + xb // 16), L.OP_CONV_DGRAD_ACCMASK, dtype=self.dt,
                      p=(u.dconv, u.wc, dx, src, mask), d=u.d)
        u.dx = dx

    def dgrad_bnstat(self, u, dx, feed, tiles):
        """dx = dgrad(u), which is `feed`'s dout: feed's BN-backward partials are made in
        the epilogue, `tiles` per channel (returned as bn_bwd's `stats`)."""
        d, fb = u.d, feed.bn
        part = self.buf((d.C, tiles, 2), torch.float32)
        self.bw.timed(u.cost("dgrad", u.in_bytes()), L.OP_CONV_DGRAD_BNSTAT, dtype=self.dt,
                      i=(1,), f=(0.0,),
                      p=(u.dconv, u.wc, dx, feed.y, fb.weight, fb.bias, feed.mean, feed.rstd,
                         part, None), d=d)
        u.dx = dx
        return part, tiles

    def finish(self):
        """one workspace per stream for the ops of this plan (each stream runs in order)"""
        ws = [self.buf((max(1, n),), torch.uint8) for n in self.ws_need]
        for lst in (self.fw, self.bw):
            if lst is not None:
                lst.patch({WS: ws[0].data_ptr(), WS2: ws[1].data_ptr()})


def _unit_fwd(r, u, st=0, join=None):
    """conv + BN(+res)(+ReLU) on stream `st`; `join`: an event that stream waits for before
    the first op that reads u.res (the downsample branch)."""
    if r.fold:
        if join is not None:
            r.fw.add(L.OP_WAIT, p=(join,), stream=st)
        r.conv_bneval(u, st)
        return
    stats = r.conv_fwd(u, st)
    if join is not None:
        r.fw.add(L.OP_WAIT, p=(join,), stream=st)
    r.bn_fwd(u, stats, r.buf(tuple(u.y.shape)), st)


def _record_stem(r, trunk, H, W, in_nchw, cin):
    """Input conversion, stem conv + BN + ReLU, max pool.  Returns the trunk input operand
    x0, the stem_pool record and the pooled tensor's (H, W, C)."""
    N, T, fw = r.N, r.T, r.fw
    stem_conv, bn0, mp = trunk[0], trunk[1], trunk[3]
    # bf16: the stem runs as a conv over pixel pairs of the zero-bordered image
    # (mmdx_stem_pair_*: K = 224, no border taps) instead of a channel-padded NHWC copy
    ks, ss, ps = stem_conv.kernel_size, stem_conv.stride, stem_conv.padding
    stem_pair = (in_nchw and T == torch.bfloat16 and ss == 2 and cin <= 4
                 and stem_conv.in_channels == cin and (W + 2 * ps) % 2 == 0)
    d_pair = None
    if stem_pair:
        d_pair = L.ConvDesc()
        call("mmdx_stem_pair_desc", N, cin, H, W, stem_conv.out_channels, ks, ks, ss, ps,
             ctypes.byref(d_pair))
        cp = 8
        x0 = r.buf((N, d_pair.H, d_pair.W, 8))
        fw.add(L.OP_STEM_PAIR_INPUT, i=(N, cin, H, W, ps), p=(_Ext(0), x0))
    elif in_nchw:
        cp = r.vec
        x0 = r.buf((N, H, W, cp))
        fw.add(L.OP_NCHW2NHWC, r.dt, i=(N, cin, H, W, cp), p=(_Ext(0), x0))
    else:
        cp = cin
        x0 = _Ext(0)
    # train forward: the stem's BN + ReLU run inside the 3x3/2 pool (mmdx_maxpool_bn_fwd,
    # bit-identical to apply-then-pool) — the 112x112x64 post-activation tensor is never
    # written or re-read; the stem's backward recomputes its ReLU mask from the raw output
    pool_bn = r.train and not r.fold and mp.kernel_size == 3 and mp.stride == 2
    su = r.unit(stem_conv, bn0, True, x0, (H, W, cp), pair=d_pair)
    if pool_bn:
        r.bn_fwd(su, r.conv_fwd(su), None)
    else:
        _unit_fwd(r, su)
    H, W, C = su.d.P, su.d.Q, su.d.K
    P = (H + 2 * mp.padding - mp.kernel_size) // mp.stride + 1
    Q = (W + 2 * mp.padding - mp.kernel_size) // mp.stride + 1
    pooled = r.buf((N, P, Q, C))
    am = r.buf((N, P, Q, C), torch.uint8)
    if pool_bn:
        fw.add(L.OP_MAXPOOL_BN_FWD, r.dt,
               i=(N, H, W, C, mp.kernel_size, mp.stride, mp.padding, P), l=(Q, 1),
               p=(su.y, pooled, am, bn0.weight, bn0.bias, su.mean, su.rstd))
    else:
        fw.add(L.OP_MAXPOOL_FWD, r.dt,
               i=(N, H, W, C, mp.kernel_size, mp.stride, mp.padding, P),
               l=(Q,), p=(su.out, pooled, am))
    stem_pool = dict(u=su, argmax=am, pooled=pooled, geom=(N, H, W, C, P, Q), fused=pool_bn)
    return x0, stem_pool, (P, Q, C)


def _block_fwd(r, blk, x_in, hwc):
    """One residual block over `x_in` (H, W, C = hwc).  Returns its units, its downsample
    unit (or None), its output and the output's (H, W, C)."""
    ds_u = ds_done = None
    idn = x_in
    if blk.downsample is not None:
        ds_u = r.unit(blk.downsample[0], blk.downsample[1], False, x_in, hwc)
        if DS_SIDE_STREAM:
            # the downsample branch (conv + BN) runs on the side stream beside the
            # block's conv1 / conv2 / conv3; the main stream joins it right before
            # the residual BN apply that reads it (the side stream is idle in the
            # forward: it carries the weight gradients in the backward)
            r.sync(r.fw, 0, 1)
            _unit_fwd(r, ds_u, st=1)
            ds_done = r.arena.event()
            r.fw.add(L.OP_SIGNAL, p=(ds_done,), stream=1)
        else:
            _unit_fwd(r, ds_u)
        idn = ds_u.out
    bu = []
    h = x_in
    specs = blk.units()
    for i, (conv, bn, relu) in enumerate(specs):
        last = i == len(specs) - 1
        u = r.unit(conv, bn, relu, h, hwc, res=idn if last else None)
        _unit_fwd(r, u, join=ds_done if last else None)
        h, hwc = u.out, (u.d.P, u.d.Q, u.d.K)
        bu.append(u)
    return bu, ds_u, h, hwc


def _dgrad_feeding(r, u, feed):
    """u's dgrad into a new tensor: the gradient of unit `feed`'s output (no residual inside
    a block), so it also makes feed's BN-backward partials where the kernel can.  Returns
    (dx, feed's `stats` or None)."""
    # (units with a residual are not fed: their producer is conv1's dgrad
    # accumulating onto the identity-path gradient; the ABI supports it
    # (beta 1, mask from the unit's output) but its heavier epilogue measured
    # 0.8 ms/step slower than the separate reduce at C4)
    dx = r.dx_buf(u)
    tiles = (L.lib().mmdx_conv_dgrad_stat_blocks(r.dt, u.d)
             if feed is not None and feed.relu else 0)
    if tiles > 0:
        return dx, r.dgrad_bnstat(u, dx, feed, tiles)
    r.dgrad(u, dx, 0.0)
    return dx, None


def _block_bwd(r, bu, ds_u, dx, pair_on):
    """Backward of one block from `dx`, the gradient of its output: per unit the BN backward,
    the wgrad (side stream) and the dgrad.  Returns the gradient of the block's input."""
    last = bu[-1]
    # identity block (bf16, 1-bit ReLU mask kept): conv1's dgrad adds the masked
    # block-output gradient itself, the residual unit writes no d_residual
    # (blocks with a downsample: its BN backward reads the same masked gradient)
    mask_id = r.T == torch.bfloat16 and len(bu) > 1 and last.rmask is not None
    acc_id = mask_id and ds_u is None
    # downsample block: its two BN backwards run as one paired op, issued where
    # bn3's is, and the downsample wgrad follows conv3's on the side stream
    paired = mask_id and ds_u is not None and pair_on
    dres = None
    if paired:
        r.bn_bwd_pair(last, ds_u, dx)
        r.wgrads_after_bn(last, ds_u)
    else:
        dres = r.bn_bwd(last, dx, want_dres=not mask_id)
        r.wgrads_after_bn(last)
    # unit i's dgrad produces the gradient of unit i-1's output (no residual
    # inside a block): it also makes unit i-1's BN-backward partials
    dh, fed = _dgrad_feeding(r, last, bu[-2] if len(bu) > 1 else None)
    for k in range(len(bu) - 2, -1, -1):
        uu = bu[k]
        if k == 0 and ds_u is not None and not paired:
            # the downsample BN's backward and wgrad (paired: issued with bn3's above)
            if mask_id:
                r.bn_bwd_masked(ds_u, dx, last.rmask)
            else:
                r.bn_bwd(ds_u, dres)
            r.wgrads_after_bn(ds_u)
        if k == 0 and ds_u is not None and ds_u.d.stride_h > 1:
            # d(block input) = dgrad(conv1) + dgrad(strided downsample): conv1's
            # dgrad writes it (beta 0), then the 1x1/2 downsample's dgrad adds
            # its one output phase (beta 1; the phases no tap reaches are left
            # alone) — instead of the downsample writing 3/4 zeros first and
            # conv1 re-reading the whole tensor to accumulate onto it
            r.bn_bwd(uu, dh, fed)
            r.wgrads_after_bn(uu)
            dh = r.dx_buf(uu)
            r.dgrad(uu, dh, 0.0)
            r.dgrad(ds_u, dh, 1.0)
        elif k == 0 and acc_id:
            r.bn_bwd(uu, dh, fed)
            r.wgrads_after_bn(uu)
            dh = r.dx_buf(uu)
            r.dgrad_accmask(uu, dh, dx, last.rmask)
        elif k == 0:
            # d(block input) = dgrad(conv1) + identity-path grad (beta = 1)
            if ds_u is not None:
                dxi = r.dx_buf(ds_u)
                r.dgrad(ds_u, dxi, 0.0)
            else:
                dxi = dres
            r.bn_bwd(uu, dh, fed)
            r.wgrads_after_bn(uu)
            r.dgrad(uu, dxi, 1.0)
            dh = dxi
        else:
            r.bn_bwd(uu, dh, fed)
            r.wgrads_after_bn(uu)
            dh, fed = _dgrad_feeding(r, uu, bu[k - 1])
    return dh


def _stem_bwd(r, mp, stem_pool, dx):
    """Max pool, stem BN + ReLU and stem wgrad from `dx`, the pooled tensor's gradient
    (no dgrad into the image)."""
    su, am = stem_pool["u"], stem_pool["argmax"]
    n0, h0, w0, c0, p0, q0 = stem_pool["geom"]
    if mp.kernel_size == 3 and mp.stride == 2 and mp.padding <= 1 and su.relu:
        # the pool's backward runs inside the stem BN backward: the 112x112x64
        # gradient of the pool input is never materialised
        r.bn_bwd_pool(su, dx, am, (n0, h0, w0, c0, mp.kernel_size, mp.stride, mp.padding,
                                   p0, q0))
    else:
        da = r.buf((n0, h0, w0, c0))
        r.bw.add(L.OP_MAXPOOL_BWD, r.dt, i=(n0, h0, w0, c0, mp.kernel_size, mp.stride,
                                            mp.padding, p0), l=(q0,), p=(am, dx, da))
        r.bn_bwd(su, da)
    r.wgrads_after_bn(su)


def _layer_regions(trunk, grad_off, grad_bytes):
    """Per-layer gradient regions for data parallelism.  engine_params is in forward
    order, so layer k's gradients are one contiguous slice of the arena and layers
    4, 3, 2 are its tail.  Returns {number of blocks (from the last) whose backward is
    enqueued when that layer's is complete: (lo, hi) of the layer} for layers 4, 3, 2, and
    layer 4's lo."""
    layer_lo = []
    for li in range(4, 8):
        ids_ = {id(q) for q in trunk[li].parameters()}
        layer_lo.append(min(o for i, o in grad_off.items() if i in ids_) // 4)
    layer_hi = layer_lo[1:] + [grad_bytes // 4]
    done_at = {}
    acc = 0
    for li in (3, 2, 1):           # layer4, layer3, layer2 (indices into layer_lo)
        acc += len(trunk[li + 4])
        done_at[acc] = (layer_lo[li], layer_hi[li])
    return done_at, layer_lo[3]


class _Plan:
    """Recorded forward / backward op lists of one trunk configuration (one arena)."""

    def __init__(self, trunk, N, H, W, in_nchw, cin, T, train, keep, dev):
        r = _Rec(trunk, N, T, train, keep, dev)
        self.arena = r.arena
        self.x0, self.stem_pool, hwc = _record_stem(r, trunk, H, W, in_nchw, cin)
        x = self.stem_pool["pooled"]
        blks = [b for layer in list(trunk)[4:8] for b in layer]
        if blks:  # (every block conv's weights go through the multi-tensor pack)
            r.pack_join()
        # the recorded blocks and stem pool buffers are read by the per-launch parity test
        self.blocks = []
        for blk in blks:
            bu, ds_u, y, hwc_out = _block_fwd(r, blk, x, hwc)
            self.blocks.append((bu, ds_u, hwc))
            x, hwc = y, hwc_out
        if r.packs:
            r.pack_at_head()
        H, W, C = hwc
        self.feats = r.buf((N, C))
        self.top = x  # layer4's output [N, H, W, C] (forward_features; Grad-CAM reads it)
        r.fw.add(L.OP_AVGPOOL_FWD, r.dt, i=(N, H * W, C), p=(x, self.feats))
        self.out_geom = (N, H, W, C)
        self.bwd = None
        self.grad_regions = []
        if keep:
            self.params = trunk.engine_params()
            self.grad_off, self.grad_bytes = r.grad_off, r.grad_bytes
            self._record_bwd(r, trunk)
        r.finish()
        self.fwd = r.fw.freeze()
        if self.bwd is not None:
            self.bwd.freeze()

    def _record_bwd(self, r, trunk):
        """The weight gradients (wgrad) run on a side stream: they depend on the BN backward
        of their unit but nothing on the critical dgrad chain depends on them, so they fill
        the CUs the chain's smaller launches leave idle.  The main stream joins the side
        stream once at the end, before the optimizer reads the gradients."""
        bw = self.bwd = r.bw
        # MMDX_BN_BWD_PAIR=0: the two separate BN backwards (A/B runs)
        pair_on = bool(L.lib().mmdx_bn_bwd_pair_enabled())
        N, H, W, C = self.out_geom
        dx = self.dtop = r.buf((N, H, W, C))
        bw.add(L.OP_AVGPOOL_BWD, r.dt, i=(N, H * W, C), p=(_Ext(0), dx))
        # A layer's gradients (_layer_regions) are final once the side stream has
        # run that layer's weight gradients (each waits for its unit's BN backward, which
        # also writes the BN parameter gradients on the main stream): the plan signals
        # one event on the side stream right after each layer's last wgrad, so the
        # all-reduce of layer 4 runs beside layers 3..1's backward, layer 3's beside
        # layers 2..1's, and so on.  The stem + layer 1 (the arena's head) are reduced
        # after the backward.  self.grad_regions: [(lo, hi, event)] in backward order.
        done_at, self.grad_tail = _layer_regions(trunk, self.grad_off, self.grad_bytes)
        for bi, (bu, ds_u, _shape) in enumerate(reversed(self.blocks)):
            if bi in done_at:
                bw.add(L.OP_SIGNAL, p=(r.arena.event(),), stream=1)
                bw.cut()  # TRUNK_SEGMENT_HOOK runs here (region k = segment k)
                self.grad_regions.append((*done_at[bi], r.arena.bufs[-1]))
            dx = _block_bwd(r, bu, ds_u, dx, pair_on)
        _stem_bwd(r, trunk[3], self.stem_pool, dx)
        r.sync(bw, 1, 0)


# TRUNK_GRAD_HOOK(grads, regions): called right after the trunk backward is enqueued with the
# flat fp32 gradient arena and [(lo, hi, event)] for layers 4, 3, 2 (backward order): after
# `event` fires, grads[lo:hi] is final (data parallelism: start that slice's all-reduce
# early from a comm stream waiting on the event, dist.GradAllReducer.launch_region).
# None = no hook.
TRUNK_GRAD_HOOK = None

# TRUNK_SEGMENT_HOOK(grads, lo, hi): the backward plan is replayed in segments, one per layer
# 4, 3, 2, and the hook is called between them with the weight-gradient stream current:
# everything that writes grads[lo:hi] is already enqueued on that stream (its wgrads wait for
# the layer's BN backward), so a collective issued from it (RCCL: its stream waits on the
# current one) starts when the slice is final, with no stream or event of its own
# (dist.GradAllReducer.trunk_segment).  Takes precedence over TRUNK_GRAD_HOOK.  None = off.
TRUNK_SEGMENT_HOOK = None

# Downsample branch of the forward on the side stream (False: in order on the main stream;
# read when a plan is built — for A/B runs, tools/step_probe.py --ds-main).
DS_SIDE_STREAM = True

# MMDX_WGRAD_CUS=n: the weight-gradient stream confined to n evenly spread compute units
# (mmdx_stream_create, a CU-masked HIP stream), leaving the rest to the dgrad / BN chain on
# the main stream; unset or 0 = all CUs (an ordinary stream).
WGRAD_CUS = int(os.environ.get("MMDX_WGRAD_CUS", "0") or 0)


class _NativeStream:
    """Owns a stream made by mmdx_stream_create; `.stream` is its torch.cuda.ExternalStream."""

    def __init__(self, dev, cus):
        h = ctypes.c_void_p()
        with torch.cuda.device(dev):
            L.call("mmdx_stream_create", 0, cus, ctypes.byref(h))
        self.handle = h.value
        self.stream = torch.cuda.ExternalStream(self.handle, device=dev)

    def __del__(self):
        if self.handle:
            try:
                L.lib().mmdx_stream_destroy(self.handle)
            except Exception:  # interpreter shutdown
                pass
            self.handle = None


def _side_stream(trunk, dev):
    key = "_mmdx_wgrad_stream_%d" % dev.index
    st = trunk.__dict__.get(key)
    if st is None:
        if WGRAD_CUS > 0:
            ns = trunk.__dict__[key + "_owner"] = _NativeStream(dev, WGRAD_CUS)
            st = ns.stream
        else:
            st = torch.cuda.Stream(device=dev)
        trunk.__dict__[key] = st
    return st


def _plans_for(trunk, key, build):
    """A free arena for `key` (recording a new one if every recorded arena is held)."""
    cache = trunk.__dict__.setdefault("_mmdx_plans", {})
    return plan_cache_get(cache, key, build)


def _run_fwd_plan(x, trunk, keep, params):
    """Replay the forward plan of (x's shape, the trunk's dtype and mode, keep, params),
    recording it first if need be; returns the plan, whose arena then holds the activations."""
    L.require_device(x)
    T = trunk.compute_dtype
    train = trunk.training
    dev = x.device
    if x.dim() != 4:
        raise ValueError("expected images [B,3,H,W]")
    if x.dtype == torch.float32 and x.shape[1] == 3:
        N, cin, H, W = x.shape
        in_nchw = True
    else:  # pre-converted NHWC, channel-padded
        N, H, W, cin = x.shape
        in_nchw = False
        if x.dtype != T:
            raise TypeError("NHWC trunk input must already be in the compute dtype")
    key = (N, H, W, cin, in_nchw, T, train, keep, dev.index,
           tuple(p.data_ptr() for p in params), L.lib().mmdx_bn_bwd_pair_enabled())
    plan = _plans_for(trunk, key,
                      lambda: _Plan(trunk, N, H, W, in_nchw, cin, T, train, keep, dev))
    # the downsample branches run on the side stream (joined inside the plan)
    plan.fwd.run([x.data_ptr()], [stream(), _side_stream(trunk, dev).cuda_stream],
                 timer=CONV_TIMER)
    if train:  # every BN's num_batches_tracked += 1, in one multi-tensor launch
        torch._foreach_add_([m.num_batches_tracked for m in trunk.modules()
                             if isinstance(m, BatchNorm2d)], 1)
    return plan


class _TrunkFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, trunk, need_grad, *params):
        keep = bool(need_grad)
        plan = _run_fwd_plan(x, trunk, keep, params)
        if keep:
            tok = _Token()
            plan.arena.owner = weakref.ref(tok)
            ctx.tok = tok
            ctx.plan = plan
            ctx.trunk_ref = trunk
            # the stem's wgrad reads the trunk input itself unless the plan converted it
            ctx.x = x if isinstance(plan.x0, _Ext) else None
        return plan.feats.clone()

    @staticmethod
    def backward(ctx, dfeats):
        plan = ctx.plan
        trunk_params = plan.params
        from .functional import cast
        dfeats = cast(dfeats.contiguous(), plan.feats.dtype)
        dev = dfeats.device
        grads = torch.empty(plan.grad_bytes // 4, dtype=torch.float32, device=dev)
        x0 = ctx.x.data_ptr() if isinstance(plan.x0, _Ext) else plan.x0.data_ptr()
        # weight gradients on a side stream (in order on the main stream measured 9.5 %
        # slower at C4: 7128 vs 7876 samples/s)
        side = _side_stream(ctx.trunk_ref, dev)
        seg_hook = TRUNK_SEGMENT_HOOK
        between = None
        if seg_hook is not None and plan.grad_regions:
            regions = plan.grad_regions

            def between(k):
                lo, hi, _ev = regions[k]
                with torch.cuda.stream(side):
                    seg_hook(grads, lo, hi)
        plan.bwd.run([dfeats.data_ptr(), grads.data_ptr(), x0], [stream(), side.cuda_stream],
                     timer=CONV_TIMER, between=between)
        hook = TRUNK_GRAD_HOOK
        if between is None and hook is not None and plan.grad_regions:
            hook(grads, plan.grad_regions)
        plan.arena.owner = None
        ctx.plan = ctx.x = ctx.tok = ctx.trunk_ref = None
        out = [None, None, None]
        for prm in trunk_params:
            if prm.requires_grad:
                o = plan.grad_off[id(prm)] // 4
                out.append(grads[o:o + prm.numel()].view(prm.shape))
            else:
                out.append(None)
        return tuple(out)
