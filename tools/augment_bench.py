"""Time the augmentation kernel (functional.augment_affine, one launch) against the same
computation from torch's own ROCm ops (affine_grid + grid_sample + the elementwise photometry)
on the same tensors, and against a device-to-device copy of the same bytes.

    python tools/augment_bench.py [--batch 1 128] [--samples 30] [--out FILE] [--parity FILE]

The training geometry: [B, 3, 224, 224] fp32 normalised 8-bit pixels, default `Augment` draws
with hflip = 0.5.  Device events around back-to-back launches, after a warm-up of every shape;
the ops alternate sample by sample, so a drift of the shared machine hits all of them; per op
the median with min / p10 / p90 / max.  GB/s is against the algorithmic bytes: every element
read once and written once (8 bytes per element; the 4-tap gather's re-reads are cache traffic,
not counted).  The copy is the bandwidth ceiling of those bytes.  The parameter rows are on the
device before the clock starts on both sides (the kernel is timed through the C entry point, the
torch side gets its theta / gain / delta tensors prebuilt): what is compared is device work.
The torch side is checked against the kernel before anything is timed.  The gate: the kernel's
median is not above the torch composition's in the same run (exit status 1 otherwise).

--parity FILE: the kernel against augment.reference in fp64 on the shapes and draws that
tests/test_augment_gpu.py bounds by 1e-3.  Needs a GPU."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmdx  # noqa: E402,F401
import mmdx.functional as F  # noqa: E402
from mmdx import augment as A  # noqa: E402
from mmdx._lib import call, ptr, stream  # noqa: E402

C, H, W = 3, 224, 224
MEAN = torch.tensor(A.IMAGENET_MEAN, dtype=torch.float32)
STD = torch.tensor(A.IMAGENET_STD, dtype=torch.float32)


def pixels(shape, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(0, 256, shape, generator=g).float() / 255.0
    return (p - MEAN.view(1, -1, 1, 1)) / STD.view(1, -1, 1, 1)


class TorchSide:
    """torch's composition of the same map: theta for affine_grid(align_corners=False) in its
    normalised [-1, 1] coordinates, grid_sample with zero padding around x - fill, then the
    photometry and the clamp as elementwise ops."""

    def __init__(self, rows, dev):
        r = torch.from_numpy(rows).double()
        a00, a01, ox, a10, a11, oy, gain, delta = r.T
        # pixel index <-> normalised: x_n = (2 j + 1) / W - 1, so dx = W x_n / 2
        theta = torch.stack([torch.stack([a00, a01 * H / W, 2 * ox / W], -1),
                             torch.stack([a10 * W / H, a11, 2 * oy / H], -1)], -2)
        self.theta = theta.float().to(dev)
        m, s = MEAN.double().view(1, C, 1, 1), STD.double().view(1, C, 1, 1)
        g, d = gain.view(-1, 1, 1, 1), delta.view(-1, 1, 1, 1)
        self.gain = g.float().to(dev)
        self.off = (((g - 1) * (m - 0.5) + d) / s).float().to(dev)
        lo, hi = A.clamp_bounds(MEAN.numpy(), STD.numpy())
        self.lo = torch.from_numpy(lo).view(1, C, 1, 1).to(dev)
        self.hi = torch.from_numpy(hi).view(1, C, 1, 1).to(dev)

    def __call__(self, x):
        grid = TF.affine_grid(self.theta, list(x.shape), align_corners=False)
        v = TF.grid_sample(x - self.lo, grid, mode="bilinear", padding_mode="zeros",
                           align_corners=False) + self.lo
        return torch.minimum(torch.maximum(self.gain * v + self.off, self.lo), self.hi)


def one(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def line(name, t, gbytes=None):
    s = (f"  {name:<44s} median {np.median(t) * 1e3:9.2f} us   min {t.min() * 1e3:9.2f}   "
         f"p10 {np.percentile(t, 10) * 1e3:9.2f}   p90 {np.percentile(t, 90) * 1e3:9.2f}   "
         f"max {t.max() * 1e3:9.2f}   ({len(t)} samples)")
    if gbytes is not None:
        s += f"   {gbytes / (np.median(t) * 1e-3):8.1f} GB/s"
    return s


def bench_kernels(dev, batches, samples, lines):
    ok = True
    mean = (ctypes.c_float * C)(*A.IMAGENET_MEAN)
    std = (ctypes.c_float * C)(*A.IMAGENET_STD)
    for B in batches:
        x = pixels((B, C, H, W), seed=B).to(dev)
        rows = A.Augment(hflip=0.5, seed=B).draw(B, H, W)
        d_rows = torch.from_numpy(rows).to(dev)
        out, dst = torch.empty_like(x), torch.empty_like(x)
        side = TorchSide(rows, dev)

        def ours():
            call("mmdx_augment_affine", ptr(x), ptr(d_rows), B, C, H, W, mean, std, 1, ptr(out),
                 stream())

        ours()
        t = side(x)
        torch.cuda.synchronize()
        err = (out - t).abs().max().item()
        if not err <= 2e-3 or not torch.equal(out, F.augment_affine(x, rows)):
            raise SystemExit(f"B = {B}: the kernel and the torch composition disagree ({err})")
        gb = 2 * x.numel() * 4 / 1e9
        inner = 50 if B <= 8 else 10
        ops = [("augment_affine (1 launch)", ours),
               ("torch affine_grid/grid_sample/photometry", lambda: side(x)),
               ("device-to-device copy of the same bytes", lambda: dst.copy_(x)),
               ("augment_affine incl. validation + upload",
                lambda: F.augment_affine(x, rows, out=out))]
        for _, fn in ops:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ts = [[] for _ in ops]
        for _ in range(samples):       # alternate the ops sample by sample
            for k, (_, fn) in enumerate(ops):
                ts[k].append(one(fn, inner))
        med = [float(np.median(t)) for t in ts]
        lines.append(f"B = {B}: [{B}, 3, 224, 224] fp32 in and out; {gb * 1e3:.2f} MB algorithmic; "
                     f"kernel vs torch max abs diff {err:.1e}; {inner} calls per sample")
        for k, (name, _) in enumerate(ops):
            lines.append(line(name, np.array(ts[k]), gb))
        gate = med[0] <= med[1]
        ok = ok and gate
        lines.append(f"  kernel / torch composition = {med[0] / med[1]:.3f} (gate: <= 1, "
                     f"{'met' if gate else 'MISSED'});   kernel / copy = {med[0] / med[2]:.2f}")
    return ok


def parity(dev, path):
    lines = ["augment_affine vs augment.reference in fp64, uniform 8-bit pixels normalised, "
             "default draws with hflip = 0.5 (the cases of tests/test_augment_gpu.py, bound 1e-3)",
             torch.cuda.get_device_name(0)]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_augment_cpu import pixels as test_pixels
    worst = 0.0
    for shape in [(3, 3, 20, 28), (1, 3, 5, 300), (4, 3, 224, 224)]:
        B, _, h, w = shape
        x = test_pixels(shape, seed=h)
        p = A.Augment(hflip=0.5, seed=w).draw(B, h, w)
        for clamp in (True, False):
            got = F.augment_affine(x.to(dev), p, clamp=clamp).cpu().double()
            err = (got - A.reference(x, p, clamp=clamp, dtype=torch.float64)).abs().max().item()
            worst = max(worst, err)
            lines.append(f"  {str(list(shape)):<20s} clamp={clamp!s:<5s}: max abs err {err:.3e}")
    lines.append(f"worst: {worst:.3e}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 128])
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parity", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs a GPU")
    dev = torch.device("cuda:0")
    if a.parity:
        parity(dev, a.parity)
    lines = [f"Augmentation kernel vs torch's own ops vs a copy, [B, 3, 224, 224] fp32, "
             f"{torch.cuda.get_device_name(0)}"]
    ok = bench_kernels(dev, a.batch, a.samples, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
