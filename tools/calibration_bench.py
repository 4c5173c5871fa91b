"""Time the calibration kernels (mmdx_calib_fit_step, mmdx_reliability_bins) against the same
Platt fit written with torch's own ROCm ops, and beside the disease-loss forward.

    python tools/calibration_bench.py [--samples 20] [--out FILE]

Shapes [128, 13], [4096, 13] and [2^20, 13] fp32 logits, hard labels with 10 % NaN.  Per shape:
- one fit pass (one launch: the seven sums and the solver step), through the C entry point;
- a whole fit, 33 passes back to back, through the C entry point (every buffer allocated first);
- functional.calib_fit (the same plus the label counts, the allocations and the checks);
- the reliability-bins kernel (15 bins, with scale and bias);
- the same damped Newton fit from torch elementwise ops on the device (33 passes, no sync,
  torch.where for the accept / reject);
- torch.optim.LBFGS as a user would write it (max_iter 33, strong Wolfe; syncs per step);
- mmdx_disease_loss_fwd (default settings, no gradient) at the same shape: a fit pass reads the
  same 8 bytes per element and does the same expf + log1pf, plus seven fp64 sums.

Device events around back-to-back calls after a warm-up; the ops alternate sample by sample, so
a drift of the shared machine hits all of them; per op the median with min / p10 / p90 / max.
At the two small shapes a pass is a few microseconds of device work: those rows measure
launches.  Before anything is timed, the kernel fit, the torch Newton fit and LBFGS are checked
to agree on the calibrated probabilities.  No gate; the numbers are a record.  Needs a GPU."""
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
from mmdx.calibration import bin_edges  # noqa: E402

ITERS = 32


def _targets(y):
    m = ~torch.isnan(y)
    y0 = torch.where(m, y, torch.zeros_like(y))
    n_pos, n_neg = y0.sum(0), (m.float() - y0).sum(0)
    t_pos, t_neg = (n_pos + 1) / (n_pos + 2), 1 / (n_neg + 2)
    return m, t_neg + y0 * (t_pos - t_neg)


def torch_newton(z, y, iters=ITERS):
    """The solver of mmdx.calibration (mode "platt") from elementwise ops: fp32 terms, fp64 sums,
    accept / reject through torch.where, no host sync."""
    m, t = _targets(y)
    C = z.shape[1]
    dd = dict(dtype=torch.float64, device=z.device)
    a_t, b_t = torch.ones(C, **dd), torch.zeros(C, **dd)
    a, b = a_t.clone(), b_t.clone()
    lam = torch.full((C,), 1e-3, **dd)
    f_acc = torch.full((C,), float("inf"), **dd)
    g = [torch.zeros(C, **dd) for _ in range(5)]
    zero = torch.zeros_like(z)
    for it in range(iters + 1):
        u = z * a_t.float() + b_t.float()
        e = torch.exp(-u.abs())
        l1p = torch.log1p(e)
        hi, lo = 1 / (1 + e), e / (1 + e)
        p, q = torch.where(u >= 0, hi, lo), torch.where(u >= 0, lo, hi)
        d, w = p - t, p * q

        def s(x):
            return torch.where(m, x, zero).sum(0, dtype=torch.float64)
        cur = [s(u.clamp(min=0) + l1p - t * u), s(d * z), s(d), s(w * z * z), s(w * z), s(w)]
        ok = cur[0] <= f_acc + 1e-9 * f_acc.abs()
        a, b = torch.where(ok, a_t, a), torch.where(ok, b_t, b)
        f_acc = torch.where(ok, cur[0], f_acc)
        g = [torch.where(ok, c, o) for c, o in zip(cur[1:], g)]
        lam = torch.where(ok, (lam / 10).clamp(min=1e-9), (lam * 10).clamp(max=1e12))
        if it == iters:
            break
        ga, gb, haa, hab, hbb = g
        A, D = haa * (1 + lam), hbb * (1 + lam)
        det = A * D - hab * hab
        good = det > 0
        det = torch.where(good, det, torch.ones_like(det))
        none = torch.zeros_like(det)
        a_t = (a - torch.where(good, (D * ga - hab * gb) / det, none)).float().double()
        b_t = (b - torch.where(good, (A * gb - hab * ga) / det, none)).float().double()
    return a.float(), b.float()


def torch_lbfgs(z, y, iters=ITERS + 1):
    """Platt scaling as a user would write it: two parameter vectors, BCE on soft targets,
    torch.optim.LBFGS with a strong-Wolfe line search."""
    m, t = _targets(y)
    t = torch.where(m, t, torch.zeros_like(t))
    a = torch.ones(z.shape[1], device=z.device, requires_grad=True)
    b = torch.zeros(z.shape[1], device=z.device, requires_grad=True)
    opt = torch.optim.LBFGS([a, b], lr=1.0, max_iter=iters, line_search_fn="strong_wolfe")

    def closure():
        opt.zero_grad()
        u = z * a + b
        e = torch.nn.functional.softplus(u) - t * u
        loss = torch.where(m, e, torch.zeros_like(e)).sum() / m.sum()
        loss.backward()
        return loss
    opt.step(closure)
    return a.detach(), b.detach()


def one(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def line(name, t):
    return (f"  {name:<46s} median {np.median(t) * 1e3:10.2f} us   min {t.min() * 1e3:10.2f}   "
            f"p10 {np.percentile(t, 10) * 1e3:10.2f}   p90 {np.percentile(t, 90) * 1e3:10.2f}   "
            f"max {t.max() * 1e3:10.2f}   ({len(t)} samples)")


def bench(dev, N, C, samples, lines):
    g = torch.Generator().manual_seed(N)
    y = (torch.rand(N, C, generator=g) < 0.15).float()
    z = (2.0 * (torch.randn(N, C, generator=g) + (2 * y - 1)) + 1.0).to(dev)
    y[torch.rand(N, C, generator=g) < 0.1] = float("nan")
    y = y.to(dev)
    lab = ~torch.isnan(y)
    y0 = torch.where(lab, y, torch.zeros_like(y)).double()
    counts = torch.stack([y0.sum(0), (lab.double() - y0).sum(0)], dim=1).contiguous()
    scale = torch.empty(C, dtype=torch.float32, device=dev)
    bias = torch.empty(C, dtype=torch.float32, device=dev)
    status = torch.empty(C, dtype=torch.int32, device=dev)
    info = torch.empty((C, 4), dtype=torch.float64, device=dev)
    nws = L.lib().mmdx_calib_fit_workspace_size(N, C)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    n_bins = 15
    edges = torch.from_numpy(bin_edges(n_bins)).to(dev)
    bins = torch.empty((C + 1) * n_bins * 4 + C + 1, dtype=torch.int64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    norm = torch.empty(1, dtype=torch.float32, device=dev)
    stats = torch.empty((C, 2), dtype=torch.float32, device=dev)
    nwl = L.lib().mmdx_disease_loss_workspace_size(N, C)
    wl = torch.empty(nwl, dtype=torch.uint8, device=dev)

    def step(k, last):
        call("mmdx_calib_fit_step", ptr(z), ptr(y), N, C, ptr(counts), 1, 1, k, int(last), 1, 1e-7,
             ptr(scale), ptr(bias), ptr(status), ptr(info), ptr(ws), nws, stream())

    def fit():
        for k in range(ITERS + 1):
            step(k, k == ITERS)

    def rel():
        call("mmdx_reliability_bins", ptr(z), ptr(y), N, C, ptr(scale), ptr(bias), ptr(edges),
             n_bins, ptr(bins), stream())

    def dloss():
        call("mmdx_disease_loss_fwd", L.F32, ptr(z), ptr(y), N, C, None, None, 0.0, 0.0, 1,
             ptr(loss), ptr(stats), ptr(norm), None, ptr(wl), nwl, stream())

    fit()
    a_n, b_n = torch_newton(z, y)
    a_l, b_l = torch_lbfgs(z, y)
    torch.cuda.synchronize()
    if status.any().item():
        raise SystemExit(f"[{N}, {C}]: the kernel fit ended with status {status.tolist()}")
    gap_n = (torch.sigmoid(z * scale + bias) - torch.sigmoid(z * a_n + b_n)).abs().max().item()
    gap_l = (torch.sigmoid(z * scale + bias) - torch.sigmoid(z * a_l + b_l)).abs().max().item()
    if not gap_n <= 1e-4:
        raise SystemExit(f"[{N}, {C}]: kernel fit and torch Newton fit differ by {gap_n}")

    small = N * C <= (1 << 16)
    ops = [("one fit pass (1 launch), C entry point", lambda: step(1, False), 50 if small else 5),
           ("whole fit, 33 passes, C entry points", fit, 2 if small else 1),
           ("functional.calib_fit (33 passes)", lambda: F.calib_fit(z, y), 2 if small else 1),
           ("reliability_bins, 15 bins, C entry point", rel, 50 if small else 5),
           ("torch elementwise Newton fit, 33 passes", lambda: torch_newton(z, y), 1),
           ("torch.optim.LBFGS, max_iter 33", lambda: torch_lbfgs(z, y), 1),
           ("disease_loss forward, C entry point", dloss, 50 if small else 5)]
    for _, fn, _ in ops:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in ops]
    for _ in range(samples):       # alternate the ops sample by sample
        for k, (_, fn, inner) in enumerate(ops):
            ts[k].append(one(fn, inner))
    grid = (nws - 16 - C * 16 * 8) // (7 * C * 8)
    lines.append(f"[{N}, {C}] fp32, platt; fit grid {grid} block(s); {N * C * 8 / 1e6:.2f} MB of "
                 f"logits + targets; max probability gap kernel fit vs torch Newton {gap_n:.1e}, "
                 f"vs LBFGS {gap_l:.1e}")
    for k, (name, _, _) in enumerate(ops):
        lines.append(line(name, np.array(ts[k])))
    med = [float(np.median(t)) for t in ts]
    lines.append(f"  fit pass / disease_loss forward = {med[0] / med[6]:.2f} (expectation: about 2 "
                 f"or less);   whole fit / torch Newton = {med[1] / med[4]:.3f};   whole fit / "
                 f"LBFGS = {med[1] / med[5]:.3f}")
    lines.append(f"  fit pass: {N * C * 8 / 1e9 / (med[0] * 1e-3):.1f} GB/s of algorithmic bytes; "
                 f"bins: {N * C * 8 / 1e9 / (med[3] * 1e-3):.1f} GB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("calibration_bench needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"Calibration kernels vs torch's own ops vs the disease-loss forward, "
             f"{torch.cuda.get_device_name(0)}"]
    for N in (128, 4096, 1 << 20):
        bench(dev, N, 13, a.samples, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
