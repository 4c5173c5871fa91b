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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", action="store_true")
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
    trunks, sums = {}, []
    for cfg in (matrix() if o.matrix else []) + o.config:
        text = record(trunks, cfg, o.batch, dev)
        name = f"{cfg.replace(':', '-')}-n{o.batch}"
        with open(os.path.join(o.out, name + ".txt"), "w") as f:
            f.write(text)
        sums.append(f"{hashlib.sha256(text.encode()).hexdigest()}  {name}\n")
    with open(os.path.join(o.out, "SHA256SUMS"), "w") as f:
        f.writelines(sums)
    print(f"{len(sums)} configurations, {len({s.split()[0] for s in sums})} distinct dumps")


if __name__ == "__main__":
    main()
