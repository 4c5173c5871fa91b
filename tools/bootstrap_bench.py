"""Time the bootstrap kernels (functional.bootstrap_weights, functional.bootstrap_counts)
against the same bootstrap composed from torch ops on the same GPU, with one all-pairs
auroc_counts call for scale.

    python tools/bootstrap_bench.py [--samples 20] [--out profiles/bootstrap_kernels.txt]

Shapes: [4096, 13] with R = 1000 and [65536, 13] with R = 200.  Device events around
back-to-back launches after a warm-up of every shape; per op the median of the samples with
min / max and the 10th / 90th percentile as the spread.  The torch composition shares the
kernel's plan (one sort): per replicate batch it gathers weights[:, row], takes an int64 cumsum
of the negative weights and sums the products, for both tie orders, per class and micro; it is
checked against the kernel's integers before anything is timed.  Needs a GPU."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmdx.functional as F  # noqa: E402

CASES = [(4096, 13, 1000, 250), (65536, 13, 200, 50)]   # N, C, R, torch replicate batch


def _scan(items, w):
    """items int32 [2, cols, L] (or [2, L]); w int32 [Rb, N].  int64 [Rb, cols, 3] =
    (u2, w_pos, w_neg)."""
    if items.dim() == 2:
        items = items[:, None]
    out = None
    for o in range(2):
        it = items[o].to(torch.int64)                       # [cols, L]
        live, pos = (it & 2) != 0, (it & 1) != 0
        x = w[:, it >> 3].to(torch.int64) * live            # [Rb, cols, L]
        xp, xn = x * pos, x * ~pos
        t = (xp * (torch.cumsum(xn, -1) - xn)).sum(-1)
        if o == 0:
            out = torch.stack([t, xp.sum(-1), xn.sum(-1)], -1)
        else:
            out[..., 0] += t
    return out


def torch_bootstrap(plan, weights, batch):
    class_items, micro_items = plan[0], plan[1]
    parts = []
    for r0 in range(0, weights.shape[0], batch):
        w = weights[r0:r0 + batch]
        parts.append(torch.cat([_scan(class_items, w), _scan(micro_items, w)], 1))
    return torch.cat(parts)


def timed(fn, samples, inner):
    out = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return np.array(out)


def line(name, t):
    return (f"  {name:<38s} median {np.median(t):9.4f} ms   min {t.min():9.4f}   "
            f"p10 {np.percentile(t, 10):9.4f}   p90 {np.percentile(t, 90):9.4f}   "
            f"max {t.max():9.4f}   ({len(t)} samples)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bootstrap_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"bootstrap kernels vs the same bootstrap in torch ops, "
             f"{torch.cuda.get_device_name(0)}",
             "scores: randn logits rounded to 1/64 (fp32, ties common); labels Bernoulli(0.2); "
             "pred = score >= 0; seed 1"]
    for N, C, R, tb in CASES:
        g = torch.Generator(device="cpu").manual_seed(N)
        s = (torch.round(torch.randn(N, C, generator=g) * 64) / 64).to(dev)
        y = (torch.rand(N, C, generator=g) < 0.2).float().to(dev)
        plan = F.bootstrap_plan(s, y, s >= 0)
        w = F.bootstrap_weights(R, N, 1, device=dev)
        boot = F.bootstrap_counts(plan, w)
        base = torch_bootstrap(plan, w, tb)
        torch.cuda.synchronize()
        if not torch.equal(boot[..., :3], base):
            raise SystemExit(f"N = {N}: the kernel and the torch composition disagree")
        path = f"{-(-N // 16384)} LDS window(s)" if N <= 131072 else "global integer atomics"
        ops = [(f"bootstrap_weights ({path})", lambda: F.bootstrap_weights(R, N, 1, device=dev),
                5),
               ("bootstrap_plan (sorts, once)", lambda: F.bootstrap_plan(s, y, s >= 0), 1),
               ("bootstrap_counts (weighted scan)", lambda: F.bootstrap_counts(plan, w), 2),
               ("torch gather + cumsum composition", lambda: torch_bootstrap(plan, w, tb), 1),
               ("auroc_counts (all pairs), ONE call", lambda: F.auroc_counts(s, y), 1)]
        for _, fn, inner in ops:            # warm-up
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        visits = 2 * R * 2 * N * C
        lines.append(f"[N, C] = [{N}, {C}], R = {R}: {visits:.3e} element visits (2 orders x R x "
                     f"(N C class + N C micro)); u2, w_pos, w_neg equal to the torch "
                     f"composition's (torch replicate batch {tb})")
        med = {}
        for name, fn, inner in ops:
            t = timed(fn, a.samples, inner)
            med[name] = float(np.median(t))
            lines.append(line(name, t))
        k, tc = med["bootstrap_counts (weighted scan)"], med["torch gather + cumsum composition"]
        lines.append(f"  counts kernel: {visits / k / 1e6:.1f} G element visits / s; torch / "
                     f"kernel = {tc / k:.2f}x; draws: "
                     f"{R * N / med[ops[0][0]] / 1e6:.2f} G / s; R replicates cost "
                     f"{k / med[ops[4][0]]:.2f}x one all-pairs call")
    # the weight kernels side by side at the row counts where one path hands over to the next
    lines.append("bootstrap_weights at the hand-overs: N = 16384 is one LDS window per row, 16385 "
                 "two (every block makes all N draws); N = 131072 is eight windows, 131073 the "
                 "first row on global integer atomics (memset included)")
    for N, R in ((16384, 1000), (16385, 1000), (131072, 256), (131073, 256)):
        fn = lambda: F.bootstrap_weights(R, N, 1, device=dev)  # noqa: E731
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        lines.append(line(f"bootstrap_weights N = {N}, R = {R}", timed(fn, a.samples, 5)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
