"""Launch-plan machinery shared by the ResNet trunk (resnet.py) and the transformer encoder
stacks (xplan.py): op lists over a buffer arena (include/mmdx.h, csrc/plan.cpp), recorded
once per configuration and replayed with ONE C call per direction.  Per-call buffers (the
input batch, the upstream gradient, the gradient buffer) enter as external bases.  An arena
holds one forward's saved activations until its backward has run, so a second forward while a
backward is pending records a second arena instead of clobbering.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L
from ._lib import call

# placeholder operands for a plan's per-stream workspaces (WS: main stream, WS2: side
# stream), patched once the sizes are known (_OpList.patch)
WS, WS2 = 0x1, 0x2


class _Ext:
    """An operand taken from the per-call external base `k` (+ byte offset)."""
    __slots__ = ("k", "off")

    def __init__(self, k, off=0):
        self.k, self.off = k, off


class _OpList:
    def __init__(self):
        self.ops = []
        self.conv_names = []   # per timed op, its tag (a LaunchCost)
        self.cuts = []

    def add(self, code, dtype=0, i=(), l=(), f=(), p=(), d=None, stream=0):
        o = L.PlanOp()
        o.op, o.dtype, o.stream = code, dtype, stream
        for j, v in enumerate(i):
            o.i[j] = int(v)
        for j, v in enumerate(l):
            o.l[j] = int(v)
        for j, v in enumerate(f):
            o.f[j] = float(v)
        for j in range(12):
            o.ext[j] = -1
        for j, v in enumerate(p):
            if isinstance(v, _Ext):
                o.ext[j] = v.k
                o.p[j] = v.off
            elif isinstance(v, torch.Tensor):
                o.p[j] = v.data_ptr()
            else:
                o.p[j] = v  # None or int
        if d is not None:
            o.d = d
        self.ops.append(o)

    def timed(self, name, code, stream=0, **kw):
        k = len(self.conv_names)
        self.add(L.OP_EVENT, i=(2 * k,), stream=stream)
        self.add(code, stream=stream, **kw)
        self.add(L.OP_EVENT, i=(2 * k + 1,), stream=stream)
        self.conv_names.append(name)

    def cut(self):
        """Segment boundary at the current end of the list: run(between=...) returns to the
        caller here (the data-parallel hook issues a layer's all-reduce from the host
        between two segments, with nothing but the plan's own streams)."""
        self.cuts.append(len(self.ops))

    def prepend(self, head):
        """Put the ops of `head` (recorded later: they need what the body allocated; no timed
        op, no cut on either side) in front of this list's."""
        assert not head.conv_names and not head.cuts and not self.cuts
        self.ops = head.ops + self.ops

    def patch(self, workspaces):
        """Replace every workspace placeholder operand: {token: pointer}."""
        for o in self.ops:
            for j in range(12):
                if o.ext[j] == -1 and o.p[j] in workspaces:
                    o.p[j] = workspaces[o.p[j]]

    def freeze(self):
        arr = (L.PlanOp * len(self.ops))(*self.ops)
        self.arr, self.n = arr, len(self.ops)
        self.bounds = [0] + [c for c in self.cuts if 0 < c < self.n] + [self.n]
        self.ops = None
        return self

    def run(self, ext, streams, timer, between=None):
        """Replay the list.  timer: the launch timer of the timed ops (resnet.CONV_TIMER,
        functional.GEMM_TIMER).  between(k): called after segment k (k = 0 .. cuts-1) is
        enqueued and before segment k+1 is; None = one native call for the whole list."""
        exts = (ctypes.c_void_p * max(1, len(ext)))(*ext)
        sts = (ctypes.c_void_p * len(streams))(*streams)
        evs = None
        if getattr(timer, "active", False) and self.conv_names:
            evs = timer.take(self.conv_names)
            evs = (ctypes.c_void_p * len(evs))(*[e.cuda_event for e in evs])
        if between is None or len(self.bounds) == 2:
            call("mmdx_plan_run", self.arr, self.n, exts, evs, sts, len(streams))
            return
        sz = ctypes.sizeof(L.PlanOp)
        base = ctypes.addressof(self.arr)
        for k, (a, z) in enumerate(zip(self.bounds[:-1], self.bounds[1:])):
            seg = ctypes.cast(base + a * sz, ctypes.POINTER(L.PlanOp))
            call("mmdx_plan_run", seg, z - a, exts, evs, sts, len(streams))
            if k < len(self.bounds) - 2:
                between(k)


class _Arena:
    """Buffers of one recorded forward (+ backward) on device `dev`.  On the CPU a plan can
    be recorded (to inspect or diff its op lists) but never run."""

    def __init__(self, dev):
        self.dev = dev
        self.bufs = []
        self.owner = None  # weakref to the autograd ctx token holding the saved activations

    def new(self, shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=self.dev)
        self.bufs.append(t)
        return t

    def event(self):
        """A synchronisation event owned by the arena (recorded once so it exists); on the
        CPU the address of an 8-byte host stand-in."""
        if self.dev.type == "cpu":
            e = ctypes.c_uint64()
            self.bufs.append(e)
            return ctypes.addressof(e)
        e = torch.cuda.Event()
        e.record(torch.cuda.current_stream())
        self.bufs.append(e)
        return e.cuda_event

    def busy(self):
        return self.owner is not None and self.owner() is not None


def pack_multi_args(arena, packs):
    """Operands of ONE multi-tensor pack launch (OP_CONV_PACK_MULTI) over packs = [(fp32
    master, KRSC copy, CRSK copy or None, K, C, master C, R*S)]; its item table is an arena
    buffer."""
    items = (L.PackItem * len(packs))()
    nb = 0
    for j, (w, krsc, crsk, K, C, cm, rs) in enumerate(packs):
        items[j] = L.PackItem(w.data_ptr(), krsc.data_ptr(),
                              crsk.data_ptr() if crsk is not None else None, K, C, cm, rs, nb)
        nb += L.lib().mmdx_conv_pack_blocks(K, C, rs)
    raw = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8)
    tbl = arena.new((raw.numel(),), torch.uint8)
    tbl.copy_(raw)
    return dict(i=(len(packs),), l=(nb,), p=(tbl,))


# recorded configurations kept per module; older keys (another batch shape, re-allocated
# parameters) whose arenas are all idle are dropped, so their buffers can be freed
MAX_PLAN_KEYS = 4


def plan_cache_get(cache, key, build):
    """Shared by the trunk and the encoder-stack plans: an idle plan recorded for `key`, or a
    new one; least recently used keys beyond MAX_PLAN_KEYS are evicted when idle."""
    lst = cache.pop(key, [])
    cache[key] = lst   # most recently used last
    for old in [k for k in cache if k != key][:max(0, len(cache) - MAX_PLAN_KEYS)]:
        if not any(pl.arena.busy() for pl in cache[old]):
            del cache[old]
    for pl in lst:
        if not pl.arena.busy():
            return pl
    pl = build()
    lst.append(pl)
    return pl


class _Token:
    pass
