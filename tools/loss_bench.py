"""Time the fused disease loss (mmdx_disease_loss_fwd / _bwd, default settings) against the plain
pair it stands beside (mmdx_bce_logits_fwd / _bwd) and against the same loss composed from
torch's own elementwise ROCm ops.

    python tools/loss_bench.py [--samples 30] [--out FILE]

Training scale: forward + backward at [128, 13] and [1024, 13] fp32 logits.  Validation scale:
the forward alone at [2^20, 13] (what metrics.evaluate() runs over its whole buffer; the plain
forward is a single workgroup there).  Targets are hard 0 / 1 labels without NaN, so all three
compute the same number; that is checked before anything is timed.

Device events around back-to-back calls, after a warm-up of every shape; the ops alternate sample
by sample, so a drift of the shared machine hits all of them; per op the median with min / p10 /
p90 / max.  The kernels are timed through the C entry points with every buffer allocated before
the clock starts; the "autograd" rows go through functional.* and loss.backward() and include the
host's share (allocation, argument checks, autograd).  At the two small shapes a call is a few
microseconds of device work, so those rows measure launches, not bandwidth.  No gate: nobody has
measured these before; the numbers are a record.  Needs a GPU."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmdx  # noqa: E402,F401
import mmdx.functional as F  # noqa: E402
from mmdx import _lib as L  # noqa: E402
from mmdx._lib import call, ptr, stream  # noqa: E402


def torch_loss(z, y):
    """The definition with default settings from elementwise ops (mask, softplus, mean over the
    labelled elements)."""
    m = ~torch.isnan(y)
    ys = torch.where(m, y, torch.zeros_like(y))
    l1p = torch.log1p(torch.exp(-z.abs()))
    e = ys * ((-z).clamp(min=0) + l1p) + (1 - ys) * (z.clamp(min=0) + l1p)
    e = torch.where(m, e, torch.zeros_like(e))
    return e.sum() / m.sum().clamp(min=1)


def one(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def line(name, t):
    return (f"  {name:<46s} median {np.median(t) * 1e3:9.2f} us   min {t.min() * 1e3:9.2f}   "
            f"p10 {np.percentile(t, 10) * 1e3:9.2f}   p90 {np.percentile(t, 90) * 1e3:9.2f}   "
            f"max {t.max() * 1e3:9.2f}   ({len(t)} samples)")


def bench(dev, B, C, backward, samples, lines):
    g = torch.Generator().manual_seed(B)
    z = (4.0 * torch.randn(B, C, generator=g)).to(dev)
    y = (torch.rand(B, C, generator=g) < 0.2).float().to(dev)
    n = B * C
    loss = torch.empty((), dtype=torch.float32, device=dev)
    loss_old = torch.empty_like(loss)
    norm = torch.empty(1, dtype=torch.float32, device=dev)
    stats = torch.empty((C, 2), dtype=torch.float32, device=dev)
    grad = torch.empty((B, C), dtype=torch.float32, device=dev) if backward else None
    dz, dz_old = torch.empty_like(z), torch.empty_like(z)
    one_ = torch.ones((), dtype=torch.float32, device=dev)
    nws = L.lib().mmdx_disease_loss_workspace_size(B, C)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    zg = z.clone().requires_grad_(True)

    def new():
        call("mmdx_disease_loss_fwd", L.F32, ptr(z), ptr(y), B, C, None, None, 0.0, 0.0, 1,
             ptr(loss), ptr(stats), ptr(norm), ptr(grad), ptr(ws), nws, stream())
        if backward:
            call("mmdx_disease_loss_bwd", L.F32, ptr(grad), n, ptr(one_), ptr(norm), ptr(dz),
                 stream())

    def old():
        call("mmdx_bce_logits_fwd", ptr(z), ptr(y), B, C, ptr(loss_old), stream())
        if backward:
            call("mmdx_bce_logits_bwd", ptr(z), ptr(y), B, C, ptr(one_), ptr(dz_old), stream())

    def through(fn):
        def f():
            zg.grad = None
            if backward:
                fn(zg, y).backward()
            else:
                with torch.no_grad():
                    fn(zg, y)
        return f

    new()
    old()
    zg.grad = None
    lt = torch_loss(zg, y)
    if backward:
        lt.backward()
    torch.cuda.synchronize()
    if not abs(loss.item() - lt.item()) <= 1e-5 * abs(lt.item()):
        raise SystemExit(f"[{B}, {C}]: disease_loss {loss.item()} and the torch composition "
                         f"{lt.item()} disagree")
    # the plain forward adds B C / 256 terms per thread in fp32: its drift is recorded, not gated
    old_dev = abs(loss_old.item() - lt.item()) / abs(lt.item())
    if not old_dev <= 1e-3:
        raise SystemExit(f"[{B}, {C}]: bce_logits {loss_old.item()} vs {lt.item()}")
    if backward and not (torch.allclose(dz, zg.grad, rtol=1e-5, atol=1e-6)
                         and torch.allclose(dz_old, zg.grad, rtol=1e-5, atol=1e-6)):
        raise SystemExit(f"[{B}, {C}]: the three gradients disagree")

    what = "forward + backward" if backward else "forward alone"
    ops = [("disease_loss kernel(s), C entry points", new),
           ("bce_logits kernel(s), C entry points", old),
           ("torch elementwise composition", through(torch_loss)),
           ("functional.disease_loss, autograd", through(lambda a, b: F.disease_loss(a, b)[0])),
           ("functional.bce_with_logits, autograd", through(F.bce_with_logits))]
    inner = 50 if n <= (1 << 16) else 5
    for _, fn in ops:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in ops]
    for _ in range(samples):       # alternate the ops sample by sample
        for k, (_, fn) in enumerate(ops):
            ts[k].append(one(fn, inner))
    lines.append(f"[{B}, {C}] fp32, {what}; grid {max(1, (nws - 16) // (8 * C))} block(s); "
                 f"{n * 8 / 1e6:.2f} MB of logits + targets; {inner} calls per sample; loss vs "
                 f"torch: disease_loss {abs(loss.item() - lt.item()) / abs(lt.item()):.1e}, "
                 f"bce_logits {old_dev:.1e} relative")
    for k, (name, _) in enumerate(ops):
        lines.append(line(name, np.array(ts[k])))
    med = [float(np.median(t)) for t in ts]
    lines.append(f"  disease_loss / bce_logits = {med[0] / med[1]:.3f};   disease_loss / torch "
                 f"composition = {med[0] / med[2]:.3f}")
    if not backward:
        lines.append(f"  disease_loss forward: {n * 8 / 1e9 / (med[0] * 1e-3):.1f} GB/s of "
                     f"algorithmic bytes (logits and targets read once)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"Disease loss (default settings) vs the plain BCE pair vs torch's elementwise ops, "
             f"{torch.cuda.get_device_name(0)}"]
    bench(dev, 128, 13, True, a.samples, lines)
    bench(dev, 1024, 13, True, a.samples, lines)
    bench(dev, 1 << 20, 13, False, a.samples, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
