"""Time the two CLAHE passes (mmdx_clahe_luts, mmdx_clahe_apply; csrc/clahe.hip) against plain
device copies of the same algorithmic bytes, and the whole preprocess_batch with and without
`clahe`.

    python tools/clahe_bench.py [--samples 30] [--out profiles/clahe_kernels.txt]

Shapes: 128 x [1024, 1024, 1] (a training batch of full-resolution radiographs),
1 x [2048, 2048, 1] (one image at inference: only tiles_x * tiles_y LUT blocks) and
128 x [256, 256, 1] (small images: the LUT tables are a quarter of the pixel bytes), with the
default setting (clip_limit 2, 8 x 8 tiles).  Two kinds of pixels per shape, because the LUT
pass's LDS atomics depend on the data: uniform random bytes (no two lanes agree on a bin), and
a radiograph-like field (a smooth 8-bit ramp with noise, a saturated flat margin of a quarter of
the width and a black collimator band: whole waves hit one bin).

Method: device events around back-to-back launches through the C entry points (descriptor
table and buffers on the device before the clock starts), after a warm-up of every op; the ops
alternate sample by sample so that a drift of the shared machine hits all of them; per op the
median with min / p10 / p90 / max.  GB/s is against the algorithmic bytes: the LUT pass reads
every pixel once (1 B/px; the LUT bytes it writes are counted too), the apply pass reads and
writes every pixel once (2 B/px).  The copies are tensor.copy_ of that many bytes in total
(half read, half written), the bandwidth ceiling of those bytes.  The outputs are checked
against mmdx.clahe.reference on the first images of every case before anything is timed.
preprocess_batch is timed with a host clock around the call (it ends in a synchronise) and
includes the host's packing of the pixels into the pinned staging buffer.  Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmdx  # noqa: E402
from mmdx import clahe as K  # noqa: E402
from mmdx._lib import call, ptr, stream  # noqa: E402

SHAPES = [(128, 1024, 1024), (1, 2048, 2048), (128, 256, 256)]


def make_images(kind, B, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return [rng.integers(0, 256, (H, W, 1), dtype=np.uint8) for _ in range(B)]
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = 40 + 150 * (0.5 + 0.5 * np.sin(x * (6.0 / W)) * np.cos(y * (4.0 / H)))
    out = []
    for _ in range(B):
        a = base + rng.normal(0, 3, (H, W)).astype(np.float32)
        a[:, : W // 4] = 255                    # burnt-out margin
        a[H - H // 8:, :] = 0                   # collimator shadow
        out.append(np.clip(np.rint(a), 0, 255).astype(np.uint8)[:, :, None])
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


def bench_case(dev, kind, B, H, W, samples, lines):
    setting = mmdx.Clahe()
    arrays = make_images(kind, B, H, W, seed=H + B)
    descs, total, lut_bytes = K.plan(arrays, setting)
    px = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays])).to(dev)
    d_desc = torch.from_numpy(descs.view(np.uint8).copy()).to(dev)
    luts = torch.empty(lut_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty_like(px)
    half_src, half_dst = px[: total // 2], torch.empty(total // 2, dtype=torch.uint8, device=dev)
    full_dst = torch.empty_like(px)
    hd = descs.ctypes.data

    def lut_pass():
        call("mmdx_clahe_luts", ptr(px), total, hd, ptr(d_desc), B, ptr(luts), lut_bytes,
             stream())

    def apply_pass():
        call("mmdx_clahe_apply", ptr(px), total, hd, ptr(d_desc), B, ptr(luts), lut_bytes,
             ptr(out), total, stream())

    def both():
        lut_pass()
        apply_pass()

    def copy_both():
        half_dst.copy_(half_src)
        full_dst.copy_(px)

    both()
    torch.cuda.synchronize()
    for b in range(min(B, 2)):      # the timed launches compute the definition
        want, want_luts = K.reference(arrays[b], setting.clip_limit, setting.tiles,
                                      return_luts=True)
        o, lo = int(descs[b]["dst_off"]), int(descs[b]["lut_off"])
        if not np.array_equal(out[o:o + want.size].cpu().numpy(), want.reshape(-1)) or \
                not np.array_equal(luts[lo:lo + want_luts.size].cpu().numpy(),
                                   want_luts.reshape(-1)):
            raise SystemExit(f"{kind} {B} x [{H}, {W}]: the kernels and the reference disagree")
    gb_lut, gb_apply = (total + lut_bytes) / 1e9, 2 * total / 1e9
    ops = [("LUT pass (mmdx_clahe_luts)", lut_pass, gb_lut),
           ("copy of 1 B/px in all (half read, half written)", lambda: half_dst.copy_(half_src),
            total / 1e9),
           ("apply pass (mmdx_clahe_apply)", apply_pass, gb_apply),
           ("copy of 2 B/px in all (1 B read + 1 B written)", lambda: full_dst.copy_(px),
            gb_apply),
           ("both passes", both, gb_lut + gb_apply),
           ("both copies", copy_both, 3 * total / 1e9)]
    inner = 5 if total >= (1 << 26) else 20
    for _, fn, _ in ops:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in ops]
    for _ in range(samples):
        for k, (_, fn, _) in enumerate(ops):
            ts[k].append(one(fn, inner))
    med = [float(np.median(t)) for t in ts]
    lines.append(f"{kind} pixels, {B} x [{H}, {W}, 1]: {total / 1e6:.2f} MB of pixels, "
                 f"{lut_bytes / 1e6:.3f} MB of LUTs; {inner} calls per sample")
    for k, (name, _, gb) in enumerate(ops):
        lines.append(line(name, np.array(ts[k]), gb))
    lines.append(f"  LUT pass / its copy = {med[0] / med[1]:.2f};   apply pass / its copy = "
                 f"{med[2] / med[3]:.2f};   both passes / both copies = {med[4] / med[5]:.2f}")
    return arrays


def bench_preprocess(dev, arrays, samples, lines):
    setting = mmdx.Clahe()
    imgs = [a[:, :, 0] for a in arrays]
    fns = [("preprocess_batch(imgs)", lambda: mmdx.preprocess_batch(imgs, dev)),
           ("preprocess_batch(imgs, clahe=Clahe())",
            lambda: mmdx.preprocess_batch(imgs, dev, clahe=setting))]
    for _, fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(samples):
        for k, (_, fn) in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    h, w = imgs[0].shape
    lines.append(f"whole preprocess_batch, {len(imgs)} x [{h}, {w}] grey arrays, host clock "
                 "around the call (packing, upload, launches, synchronise):")
    for k, (name, _) in enumerate(fns):
        t = np.array(ts[k])
        lines.append(f"  {name:<46s} median {np.median(t):9.2f} ms   min {t.min():9.2f}   "
                     f"max {t.max():9.2f}   ({len(t)} samples)")
    lines.append(f"  with / without = {np.median(ts[1]) / np.median(ts[0]):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clahe_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"CLAHE passes vs copies of the same algorithmic bytes, clip_limit 2, 8 x 8 tiles, "
             f"{torch.cuda.get_device_name(0)}"]
    first = None
    for kind in ("random", "radiograph-like"):
        for B, H, W in SHAPES:
            arrays = bench_case(dev, kind, B, H, W, a.samples, lines)
            if first is None:
                first = arrays
    bench_preprocess(dev, first, max(3, a.samples // 6), lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
