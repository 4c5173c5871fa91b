"""Time the 16-bit window passes (mmdx_window_levels = histogram + select, mmdx_window_apply;
csrc/window.hip) against plain device copies of the same algorithmic bytes, and the whole
preprocess_batch(window=...) against windowing on the host first.

    python tools/window_bench.py [--samples 20] [--out profiles/window_kernels.txt]

Shapes: 128 x [1024, 1024] (a training batch of full-resolution radiographs), 1 x [3000, 2500]
(one detector image at inference) and 128 x [256, 256] (small images: the 256 KiB histogram
of an image is twice its pixel bytes).  Two kinds of pixels per shape, because the histogram's
LDS atomics depend on the data: uniform random 16-bit values (no two lanes agree on a level,
and a block leaves most of the 65536 bins non-zero), and a radiograph-like 12-bit field (a
smooth ramp with noise, a saturated flat margin of a quarter of the width and a black
collimator band: a few hundred neighbouring levels, whole waves on one of them).

Method: device events around back-to-back launches through the C entry points (descriptor
table, buffers and the zeroed workspace on the device before the clock starts), after a warm-up
of every op; the ops alternate sample by sample so that a drift of the shared machine hits all
of them; per op the median with min / p10 / p90 / max.  GB/s is against the algorithmic bytes:
the levels pass reads every pixel once (2 B/px), the apply pass reads every pixel and writes a
byte (3 B/px).  The copies are tensor.copy_ of that many bytes in total (half read, half
written), the bandwidth ceiling of those bytes.  The outputs are checked against
mmdx.window.reference on the first images of every case before anything is timed.
preprocess_batch is timed with a host clock around the call (it ends in a synchronise) and
includes the host's packing of the pixels into the pinned staging buffer; the host route is
mmdx.window.reference (vectorised numpy) of every image, then the 8-bit preprocess_batch.
Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmdx  # noqa: E402
import mmdx.functional as F  # noqa: E402
from mmdx import window as W  # noqa: E402
from mmdx._lib import call, ptr, stream  # noqa: E402

SHAPES = [(128, 1024, 1024), (1, 3000, 2500), (128, 256, 256)]


def make_images(kind, B, H, W_, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return [rng.integers(0, 65536, (H, W_), dtype=np.uint16) for _ in range(B)]
    y, x = np.mgrid[0:H, 0:W_].astype(np.float32)
    base = 640 + 2400 * (0.5 + 0.5 * np.sin(x * (6.0 / W_)) * np.cos(y * (4.0 / H)))
    out = []
    for _ in range(B):
        a = base + rng.normal(0, 12, (H, W_)).astype(np.float32)
        a[:, : W_ // 4] = 4095                  # burnt-out margin
        a[H - H // 8:, :] = 0                   # collimator shadow
        out.append(np.clip(np.rint(a), 0, 4095).astype(np.uint16))
    return out


def one(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def line(name, t, gbytes):
    return (f"  {name:<46s} median {np.median(t) * 1e3:9.2f} us   min {t.min() * 1e3:9.2f}   "
            f"p10 {np.percentile(t, 10) * 1e3:9.2f}   p90 {np.percentile(t, 90) * 1e3:9.2f}   "
            f"max {t.max() * 1e3:9.2f}   ({len(t)} samples)   "
            f"{gbytes / (np.median(t) * 1e-3):8.1f} GB/s")


def bench_case(dev, kind, B, H, W_, samples, lines):
    setting = mmdx.Window()
    planes = make_images(kind, B, H, W_, seed=H + B)
    descs, src, dst = W.plan(planes, setting)
    host = np.zeros(src, np.uint8)
    W.pack(planes, descs, host)
    px = torch.from_numpy(host).to(dev)
    d_desc = torch.from_numpy(descs.view(np.uint8).copy()).to(dev)
    ws = F._window_workspace(B, dev)
    levels = torch.empty((B, 4), dtype=torch.int32, device=dev)
    out = torch.empty(dst, dtype=torch.uint8, device=dev)
    npx = dst                                    # pixels
    c2_src, c2_dst = px[:npx], torch.empty(npx, dtype=torch.uint8, device=dev)
    n3 = 3 * npx // 2
    c3_src = torch.empty(n3, dtype=torch.uint8, device=dev)
    c3_dst = torch.empty(n3, dtype=torch.uint8, device=dev)
    hd = descs.ctypes.data

    def levels_pass():
        call("mmdx_window_levels", ptr(px), src, hd, ptr(d_desc), B, ptr(ws), ws.numel(),
             ptr(levels), stream())

    def apply_pass():
        call("mmdx_window_apply", ptr(px), src, hd, ptr(d_desc), B, ptr(levels), ptr(out), dst,
             stream())

    def both():
        levels_pass()
        apply_pass()

    def copy_both():
        c2_dst.copy_(c2_src)
        c3_dst.copy_(c3_src)

    both()
    torch.cuda.synchronize()
    for b in range(min(B, 2)):      # the timed launches compute the definition
        want, win = W.reference(planes[b], setting, return_window=True)
        o = int(descs[b]["dst_off"])
        if not np.array_equal(out[o:o + want.size].cpu().numpy(), want.reshape(-1)) or \
                tuple(levels[b, :2].cpu().tolist()) != win:
            raise SystemExit(f"{kind} {B} x [{H}, {W_}]: the kernels and the reference disagree")
    gb_lev, gb_apply = 2 * npx / 1e9, 3 * npx / 1e9
    ops = [("levels pass (mmdx_window_levels)", levels_pass, gb_lev),
           ("copy of 2 B/px in all (half read, half written)", lambda: c2_dst.copy_(c2_src),
            gb_lev),
           ("apply pass (mmdx_window_apply)", apply_pass, gb_apply),
           ("copy of 3 B/px in all (half read, half written)", lambda: c3_dst.copy_(c3_src),
            gb_apply),
           ("both passes", both, gb_lev + gb_apply),
           ("both copies", copy_both, gb_lev + gb_apply)]
    inner = 5 if npx >= (1 << 26) else 20
    for _, fn, _ in ops:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in ops]
    for _ in range(samples):
        for k, (_, fn, _) in enumerate(ops):
            ts[k].append(one(fn, inner))
    med = [float(np.median(t)) for t in ts]
    lines.append(f"{kind} pixels, {B} x [{H}, {W_}]: {2 * npx / 1e6:.2f} MB of 16-bit pixels; "
                 f"{inner} calls per sample")
    for k, (name, _, gb) in enumerate(ops):
        lines.append(line(name, np.array(ts[k]), gb))
    lines.append(f"  levels pass / its copy = {med[0] / med[1]:.2f};   apply pass / its copy = "
                 f"{med[2] / med[3]:.2f};   both passes / both copies = {med[4] / med[5]:.2f}")
    return planes, med[0]


def bench_preprocess(dev, planes, samples, lines):
    setting = mmdx.Window()

    def host_route():
        return mmdx.preprocess_batch([W.reference(a, setting) for a in planes], dev)

    fns = [("preprocess_batch(imgs16, window=Window())",
            lambda: mmdx.preprocess_batch(planes, dev, window=setting)),
           ("numpy window.reference, then preprocess_batch", host_route)]
    if not torch.equal(fns[0][1](), fns[1][1]()):
        raise SystemExit("preprocess_batch(window=...) and the host route disagree")
    ts = [[] for _ in fns]
    for _ in range(samples):
        for k, (_, fn) in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    h, w = planes[0].shape
    lines.append(f"whole preprocess_batch, {len(planes)} x [{h}, {w}] uint16 arrays, host clock "
                 "around the call (packing, upload, launches, synchronise):")
    for k, (name, _) in enumerate(fns):
        t = np.array(ts[k])
        lines.append(f"  {name:<46s} median {np.median(t):9.2f} ms   min {t.min():9.2f}   "
                     f"max {t.max():9.2f}   ({len(t)} samples)")
    lines.append(f"  host route / windowed on the GPU = "
                 f"{np.median(ts[1]) / np.median(ts[0]):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"window passes vs copies of the same algorithmic bytes, percentile window "
             f"(0.5, 99.5), {torch.cuda.get_device_name(0)}"]
    first = None
    hist = {}
    with torch.cuda.device(dev):
        for kind in ("uniform", "radiograph-like"):
            for B, H, W_ in SHAPES:
                planes, t_levels = bench_case(dev, kind, B, H, W_, a.samples, lines)
                hist[(kind, B, H, W_)] = t_levels
                if kind == "radiograph-like" and first is None:
                    first = planes
        for B, H, W_ in SHAPES:
            r = hist[("radiograph-like", B, H, W_)] / hist[("uniform", B, H, W_)]
            lines.append(f"levels pass, radiograph-like / uniform, {B} x [{H}, {W_}]: {r:.2f}")
        bench_preprocess(dev, first, max(3, a.samples // 6), lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
