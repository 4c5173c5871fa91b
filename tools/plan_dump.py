#!/usr/bin/env python3
"""Pointer-free text dumps of recorded ResNet trunk launch plans (resnet._Plan), to diff two
revisions of the planner op for op.  Every address in an op (`p`, and OP_BN_BWD's two in `l`)
is written as name+offset: the arena buffer's allocation index, a parameter's or buffer's
qualified name, or extK; one that resolves to nothing is an error.  Plans are recorded, never
run, so the default device is the CPU (a revision whose arena cannot make events there gets a
host stand-in from this tool).  Per configuration DIR/<name>.txt, plus DIR/SHA256SUMS.
    python tools/plan_dump.py --matrix --out head_dumps
    PYTHONPATH=../parent python tools/plan_dump.py --matrix --out parent_dumps
    diff parent_dumps/SHA256SUMS head_dumps/SHA256SUMS
    python tools/plan_dump.py --config resnet50:bf16:1:1:nchw:224:1:1 --batch 128 \
        --device cuda:0 --out c4_gpu
(A worktree without a built library: point MMDX_LIB_PATH at this tree's libmmdx_hip.so.)
A configuration is arch:dtype:train:keep:layout:hw:ds_side_stream:bn_bwd_pair; --matrix is
the 384 of {resnet18, resnet50} x {bf16, fp16, fp32} x (train, keep) x {nchw, nhwc} x
{64, 65} x DS_SIDE_STREAM x MMDX_BN_BWD_PAIR at batch 2.

--stacks writes the same kind of dump for the transformer encoder-stack plans
(xplan._build_bert / _build_vit) over a fixed matrix of 144 configurations.  There a
parameter is p<index in params>, an external base extK+off, and an arena buffer b<k> with k
its order of first appearance in the op stream (its shape and dtype are listed at the end),
so the dump does not depend on the order in which the recorder allocates but does show which
ops share a buffer.
    python tools/plan_dump.py --stacks --out head_stacks
    PYTHONPATH=../parent python tools/plan_dump.py --stacks --out parent_stacks
"""
import argparse
import bisect
import ctypes
import hashlib
import itertools
import os
import sys

import torch

# appended: a PYTHONPATH naming another revision's tree wins over this one
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmdx  # noqa: E402
import mmdx._lib as L  # noqa: E402
import mmdx.resnet as RN  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def _host_event(self):
    e = ctypes.c_uint64()
    self.bufs.append(e)
    return ctypes.addressof(e)


class _Names:
    """Address -> name+offset over the arena's entries and the trunk's tensors."""

    def __init__(self, plan, trunk):
        spans = []
        self.bufs = []      # the arena's entries in allocation order, described
        self.tables = []    # (index, ctypes pointer table): contents resolved once all is known
        for k, b in enumerate(plan.arena.bufs):
            if isinstance(b, torch.Tensor):
                self.bufs.append(f"{tuple(b.shape)} {b.dtype}")
                spans.append((b.data_ptr(), b.numel() * b.element_size(), str(k)))
            elif isinstance(b, ctypes.Array):
                self.tables.append((k, b))
                self.bufs.append(None)
                spans.append((ctypes.addressof(b), ctypes.sizeof(b), str(k)))
            else:  # an event: a device event's handle, or the 8-byte host stand-in
                self.bufs.append("event")
                a = b.cuda_event if hasattr(b, "cuda_event") else ctypes.addressof(b)
                spans.append((a, 8, str(k)))
        for n, t in itertools.chain(trunk.named_parameters(), trunk.named_buffers()):
            spans.append((t.data_ptr(), t.numel() * t.element_size(), n))
        spans = sorted(s for s in spans if s[1] > 0)
        self.spans, self.starts = spans, [s[0] for s in spans]
        for k, tab in self.tables:
            self.bufs[k] = "table " + " ".join(self(v) for v in tab)

    def __call__(self, addr):
        if not addr:
            return "0"
        j = bisect.bisect_right(self.starts, addr) - 1
        if j < 0 or addr >= self.spans[j][0] + self.spans[j][1]:
            raise LookupError(f"address {addr:#x} is in no arena buffer, parameter or buffer")
        return f"{self.spans[j][2]}+{addr - self.spans[j][0]}"


def dump(plan, trunk):
    nm = _Names(plan, trunk)
    out = []
    for tag, lst in (("fwd", plan.fwd), ("bwd", plan.bwd)):
        if lst is None:
            out.append(f"{tag} None")
            continue
        out.append(f"{tag} n={lst.n} bounds={lst.bounds}")
        out += [f"  conv {tuple(c)}" for c in lst.conv_names]
        for k in range(lst.n):
            o = lst.arr[k]
            ll = [o.l[j] for j in range(4)]
            if o.op == L.OP_BN_BWD:
                ll[2:] = [nm(o.l[2]), nm(o.l[3])]
            p = [f"ext{o.ext[j]}+{o.p[j] or 0}" if o.ext[j] >= 0 else nm(o.p[j])
                 for j in range(12)]
            d = [getattr(o.d, f) for f, _ in L.ConvDesc._fields_]
            out.append(f"  op={o.op} dtype={o.dtype} stream={o.stream} i={list(o.i)} l={ll} "
                       f"f={list(o.f)} ext={list(o.ext)} p={p} d={d}")
    out.append("arena")
    out += [f"  {k} {b}" for k, b in enumerate(nm.bufs)]
    if plan.bwd is not None:
        out.append(f"grad_off {[plan.grad_off[id(q)] for q in trunk.engine_params()]}")
        out.append(f"grad_bytes {plan.grad_bytes} grad_tail {plan.grad_tail}")
    out.append(f"grad_regions {[(lo, hi) for lo, hi, _ in plan.grad_regions]}")
    out.append(f"out_geom {plan.out_geom} feats {tuple(plan.feats.shape)}")
    return "\n".join(out) + "\n"


def record(trunks, cfg, batch, dev):
    arch, dtype, train, keep, layout, hw, ds, pair = cfg.split(":")
    T, hw = DTYPES[dtype], int(hw)
    if arch not in trunks:
        torch.manual_seed(0)
        trunks[arch] = RN.ResNetTrunk(arch).to(dev)
    trunk = trunks[arch]
    trunk.compute_dtype = T
    RN.DS_SIDE_STREAM = ds == "1"
    os.environ["MMDX_BN_BWD_PAIR"] = pair
    L.reload_config()
    nchw = layout == "nchw"
    cin = 3 if nchw else (4 if T == torch.float32 else 8)
    plan = RN._Plan(trunk, batch, hw, hw, nchw, cin, T, train == "1", keep == "1", dev)
    return dump(plan, trunk)


def matrix():
    return [":".join(c) for c in itertools.product(
        ("resnet18", "resnet50"), DTYPES, "10", "10", ("nchw", "nhwc"), ("64", "65"), "10",
        "10")]


# ------------------------------------------------------------------ encoder-stack plans
def _knob(name, value):
    """Set a module-level switch read at record time, in whichever mmdx module defines it."""
    hit = [m for n, m in list(sys.modules.items())
           if n.startswith("mmdx.") and hasattr(m, name)]
    if not hit:
        raise LookupError(f"no mmdx module defines {name}")
    for m in hit:
        setattr(m, name, value)


class _StackNames:
    """Address -> name+offset for a stack plan.  A parameter is p<index in params>; an arena
    buffer is b<k>, k its order of first appearance in the op stream (so the allocation
    order does not show, but which ops share a buffer does)."""

    def __init__(self, plan, params, dev):
        fixed = [(q.data_ptr(), q.numel() * q.element_size(), f"p{k}")
                 for k, q in enumerate(params)]
        c = L.rng_counter(dev)
        fixed.append((c.data_ptr(), 8, "rng_counter"))
        self.fixed = sorted(fixed)
        self.arena = sorted((b.data_ptr(), b.numel() * b.element_size(), j)
                            for j, b in enumerate(plan.arena.bufs) if b.numel())
        self.bufs = plan.arena.bufs
        self.seen = {}      # arena index -> appearance index
        self.order = []

    @staticmethod
    def _find(spans, addr):
        j = bisect.bisect_right([s[0] for s in spans], addr) - 1
        if j >= 0 and addr < spans[j][0] + spans[j][1]:
            return spans[j]
        return None

    def buffer(self, addr):
        s = self._find(self.arena, addr)
        return self.bufs[s[2]] if s else None

    def __call__(self, addr):
        if not addr:
            return "0"
        s = self._find(self.fixed, addr)
        if s:
            return f"{s[2]}+{addr - s[0]}"
        s = self._find(self.arena, addr)
        if s is None:
            raise LookupError(f"address {addr:#x} is in no arena buffer or parameter")
        if s[2] not in self.seen:
            self.seen[s[2]] = len(self.order)
            self.order.append(s[2])
        return f"b{self.seen[s[2]]}+{addr - s[0]}"


def dump_stack(plan, params, dev):
    nm = _StackNames(plan, params, dev)
    G = plan.grads
    out = [f"grads.n {G.n}", f"grads.items {G.items}", f"grad_regions {plan.grad_regions}"]
    for tag, lst in (("fwd", plan.fwd), ("bwd", plan.bwd)):
        out.append(f"{tag} n={lst.n} bounds={lst.bounds}")
        out += [f"  gemm {tuple(c)}" for c in lst.conv_names]
        for k in range(lst.n):
            o = lst.arr[k]
            p = [f"ext{o.ext[j]}+{o.p[j] or 0}" if o.ext[j] >= 0 else nm(o.p[j])
                 for j in range(12)]
            out.append(f"  op={o.op} dtype={o.dtype} stream={o.stream} i={list(o.i)} "
                       f"l={list(o.l)} f={list(o.f)} p={p}")
            if o.op == L.OP_CONV_PACK_MULTI:   # its item table holds addresses too
                raw = bytes(nm.buffer(o.p[0]).numpy().tobytes())
                for it in (L.PackItem * o.i[0]).from_buffer_copy(raw):
                    out.append(f"    item w={nm(it.w)} krsc={nm(it.krsc)} crsk={nm(it.crsk)} "
                               f"K={it.K} C={it.C} c_master={it.c_master} RS={it.RS} "
                               f"first_block={it.first_block}")
    out.append(f"out {nm(plan.out.data_ptr())} dx {nm(plan.dx.data_ptr())}")
    out.append("arena (by first appearance)")
    for k, j in enumerate(nm.order):
        b = nm.bufs[j]
        out.append(f"  b{k} {tuple(b.shape)} {b.dtype}")
    return "\n".join(out) + "\n"


def _vit_params(nl, D, I):
    g = torch.Generator().manual_seed(0)
    shapes = ((D,), (D,), (3 * D, D), (3 * D,), (D, D), (D,), (D,), (D,), (I, D), (I,), (D, I),
              (D,))
    return [torch.randn(sh, generator=g) for _ in range(nl) for sh in shapes]


def stacks(dev):
    """The encoder-stack matrix: BERT@2 over dtype x dropout x shape, ViT over dtype x
    MMDX_VIT_LN_ADDIN x two model sizes, each over MMDX_ATTN_FLASH x
    MMDX_DP_STACK_SEG_LAYERS."""
    import mmdx.bert as MB
    import mmdx.xplan as XP
    torch.manual_seed(0)    # the recorded dropout seeds mix in torch.initial_seed()
    bert = MB.BertModel.from_name("bert-base-uncased@2")
    bp = [q for lay in bert.encoder.layer for q in lay.params()]
    vits = {"b2": (_vit_params(2, 768, 3072), 2, 197, 768, 12, 3072),
            "s12": (_vit_params(12, 64, 128), 2, 17, 64, 1, 128)}
    texts = {}
    for flash, seg in itertools.product("10", (3, 1, 0)):
        os.environ["MMDX_ATTN_FLASH"] = flash
        _knob("SEG_LAYERS", seg)
        tail = f"flash{flash}-seg{seg}"
        for (dn, T), (p, pa), (B, Ls) in itertools.product(
                DTYPES.items(), ((0.0, 0.0), (0.1, 0.1)), ((2, 16), (3, 37))):
            pl = XP._build_bert(bp, B, Ls, 768, 12, 3072, 1e-12, p, pa, T, dev)
            texts[f"bert-{dn}-p{p}-b{B}x{Ls}-{tail}"] = dump_stack(pl, bp, dev)
        for (dn, T), addin, (vn, (vp, N, S, D, H, I)) in itertools.product(
                DTYPES.items(), (True, False), vits.items()):
            _knob("VIT_LN_ADDIN", addin)
            pl = XP._build_vit(vp, N, S, D, H, I, 1e-6, T, dev)
            texts[f"vit-{vn}-{dn}-addin{int(addin)}-{tail}"] = dump_stack(pl, vp, dev)
    return texts


def _write(out_dir, texts):
    sums = []
    for name, text in texts.items():
        with open(os.path.join(out_dir, name + ".txt"), "w") as f:
            f.write(text)
        sums.append(f"{hashlib.sha256(text.encode()).hexdigest()}  {name}\n")
    with open(os.path.join(out_dir, "SHA256SUMS"), "w") as f:
        f.writelines(sums)
    print(f"{len(sums)} configurations, {len({s.split()[0] for s in sums})} distinct dumps")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", action="store_true")
    ap.add_argument("--stacks", action="store_true",
                    help="dump the BERT / ViT encoder-stack plans (mmdx.xplan) instead")
    ap.add_argument("--config", action="append", default=[])
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--out", required=True)
    o = ap.parse_args()
    dev = torch.device(o.device)
    try:
        import mmdx.plan  # noqa: F401  (its arena records events on either device)
    except ImportError:
        if dev.type == "cpu":
            RN._Arena.event = _host_event
    os.makedirs(o.out, exist_ok=True)
    if o.stacks:
        _write(o.out, stacks(dev))
        return
    trunks, texts = {}, {}
    for cfg in (matrix() if o.matrix else []) + o.config:
        texts[f"{cfg.replace(':', '-')}-n{o.batch}"] = record(trunks, cfg, o.batch, dev)
    _write(o.out, texts)


if __name__ == "__main__":
    main()
