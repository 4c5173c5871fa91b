"""Time the validation-metric kernels (functional.auroc_counts, functional.confusion_grid)
against a torch-on-GPU sort-and-rank AUROC on the same inputs.

    python tools/metrics_bench.py [--n 2048 16384 65536] [--c 13] [--samples 30] [--out FILE]

Device events around back-to-back launches (the entry points' own memsets included), after a
warm-up of every shape; per op the median of the samples with min / max and the 10th / 90th
percentile as the spread.  The baseline computes the same integer statistic (midranks from a
sort, group sizes from unique_consecutive-style flags, all classes batched plus the micro
problem) and is checked against the kernel's counts before anything is timed.  Needs a GPU."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mmdx.functional as F  # noqa: E402
from mmdx.metrics import default_grid, grid_logits  # noqa: E402


def _u2_sorted(x, pos):
    """x, pos: [G, n] (one problem per row, no NaN).  int64 [G]: 2 * rank-sum of the positives
    - n_pos (n_pos + 1), ranks being midranks."""
    G, n = x.shape
    xs, idx = torch.sort(x, dim=1)
    new = torch.ones((G, n), dtype=torch.bool, device=x.device)
    new[:, 1:] = xs[:, 1:] != xs[:, :-1]
    gid = torch.cumsum(new.reshape(-1).to(torch.int64), 0) - 1          # global group id
    cnt = torch.bincount(gid)
    cum = torch.cumsum(cnt, 0)
    row_start = (torch.arange(G, device=x.device, dtype=torch.int64) * n).repeat_interleave(n)
    rank2 = 2 * (cum[gid] - row_start) - cnt[gid] + 1                   # twice the midrank
    ps = torch.gather(pos, 1, idx).reshape(-1)
    rs = (rank2 * ps).reshape(G, n).sum(1)
    npos = pos.sum(1)
    return rs - npos * (npos + 1)


def torch_auroc_u2(scores, target):
    """[C + 1] u2 values: per class and micro, by sort and rank."""
    pos = (target > 0.5).to(torch.int64)
    per = _u2_sorted(scores.t().contiguous(), pos.t().contiguous())
    mic = _u2_sorted(scores.reshape(1, -1), pos.reshape(1, -1))
    return torch.cat([per, mic])


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
    return (f"  {name:<34s} median {np.median(t):9.4f} ms   min {t.min():9.4f}   "
            f"p10 {np.percentile(t, 10):9.4f}   p90 {np.percentile(t, 90):9.4f}   "
            f"max {t.max():9.4f}   ({len(t)} samples)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2048, 16384, 65536])
    ap.add_argument("--c", type=int, default=13)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"validation-metric kernels vs torch sort-and-rank, C = {a.c}, "
             f"{torch.cuda.get_device_name(0)}",
             "scores: randn logits (fp32, ties rare); labels Bernoulli(0.2); thresholds: the "
             "default 99-point grid"]
    thr = torch.from_numpy(grid_logits(default_grid())).to(dev)
    for N in a.n:
        g = torch.Generator(device="cpu").manual_seed(N)
        s = torch.randn(N, a.c, generator=g).to(dev)
        y = (torch.rand(N, a.c, generator=g) < 0.2).float().to(dev)
        k = F.auroc_counts(s, y)
        base = torch_auroc_u2(s, y)
        torch.cuda.synchronize()
        if not torch.equal(k[:, 0], base):
            raise SystemExit(f"N = {N}: the kernel and the sort-and-rank baseline disagree")
        pairs = a.c * N * N + (N * a.c) ** 2
        ops = [("auroc_counts (all pairs)", lambda: F.auroc_counts(s, y), 1),
               ("torch sort-and-rank AUROC", lambda: torch_auroc_u2(s, y), 1),
               ("confusion_grid (T = 99)", lambda: F.confusion_grid(s, y, thr), 20)]
        for _, fn, inner in ops:            # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        lines.append(f"N = {N}: {pairs:.3e} ordered pairs in the problem (C N^2 + (N C)^2; the "
                     f"kernel visits those with a positive i), u2 equal to the baseline's")
        n_s = a.samples if pairs < 1e11 else max(5, a.samples // 3)
        for name, fn, inner in ops:
            lines.append(line(name, timed(fn, n_s, inner)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
