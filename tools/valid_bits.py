"""Pin the bits of the validation-path kernels: disease_loss (forward and backward), calib_fit,
reliability_bins and confusion_grid, run through mmdx.functional on seeded inputs.

    python tools/valid_bits.py --write tests/golden/valid_bits.json [--commit SHA]
    python tools/valid_bits.py --check tests/golden/valid_bits.json

One SHA-256 per output tensor over its raw bytes; for the loss and the bins the raw values of the
cases of at most 64 elements too, so that a mismatch can be read.  tests/test_valid_bits_gpu.py
runs the same cases through the same functions and compares with the committed file.

All four kernels are bit-reproducible by construction (fixed-order sums, integer atomics), so the
digests are a function of the inputs, the kernels and the compiler.  The file is rewritten only
after a compiler or ROCm change, and only from a tree whose kernels are unchanged: never to make
a kernel edit pass.

Shapes: the smallest at which each part of the class-aligned reduction (csrc/class_reduce.h: 256
threads, the largest multiple TB of C among them in R = TB / C rows, 8 elements per thread before
the grid grows, at most 1024 blocks) can go wrong:
  [1, 1], [3, 13], [5, 64]  one block; TB = 256 / 247 / 256, R = 256 / 19 / 4 (19: the row tree
                            off a power of two)
  [153, 13]                 2 blocks, the second ragged: the hand-off
  [129, 64]                 5 blocks > R = 4: the gather's second trip
  [2889, 13]                20 blocks > R = 19: the same with the odd tree
  [524289, 1]               257 blocks > R = 256
  [160001, 13]              the 1024-block grid cap (loss and fit only: the bins and the grid stop
                            at 2^24 items and take the shapes above)
Needs a GPU."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import mmdx  # noqa: E402,F401
import mmdx.functional as F  # noqa: E402

BIG = (160001, 13)
SHAPES = [(1, 1), (3, 13), (5, 64), (153, 13), (129, 64), (2889, 13), (524289, 1)]
RAW_MAX = 64          # raw values are kept for cases of at most this many elements
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:8], "little")


def make_inputs(name, shape, labelled):
    """float32 logits 2 (randn + 2 y - 1) and targets: ~20 % exact 1, the rest exact 0.  A few
    logits are +-0 and +-30 and +-inf.  labelled (the loss and the fit): ~15 % of the targets are
    NaN ("no label"), and the infinite logits sit only there: on a labelled element they make a
    class sum inf or NaN, which would hide the order of the additions.  Otherwise (the bins and
    the grid): the infinite logits sit anywhere and NaN logits join them."""
    rng = np.random.default_rng(_seed(name))
    n = shape[0] * shape[1]
    y = (rng.random(shape) < 0.2).astype(np.float32)
    z = (2.0 * (rng.standard_normal(shape) + 2.0 * y - 1.0)).astype(np.float32)
    zf, yf = z.reshape(-1), y.reshape(-1)
    if labelled:
        yf[rng.random(n) < 0.15] = np.nan
    k = min(n // 4, 12)
    spots = rng.choice(n, size=k, replace=False)
    zf[spots] = np.array([0.0, -0.0, 30.0, -30.0], np.float32)[np.arange(k) % 4]
    free = np.flatnonzero(np.isnan(yf)) if labelled else np.arange(n)
    free = np.setdiff1d(free, spots)
    k = min(len(free) // 4, 6)
    odd = [np.inf, -np.inf] if labelled else [np.inf, -np.inf, np.nan]
    zf[rng.choice(free, size=k, replace=False)] = np.array(odd, np.float32)[np.arange(k) % len(odd)]
    return z, y


def _tag(shape):
    return f"{shape[0]}x{shape[1]}"


def cases():
    """[(name, kind, settings)] in a fixed order."""
    out = []
    for s in SHAPES + [BIG]:
        out.append((f"loss/{_tag(s)}/g0/f32", "loss", dict(shape=s)))
    for s in ((153, 13), (129, 64), (2889, 13)):
        for gamma in (2.0, 3.5):
            out.append((f"loss/{_tag(s)}/g{gamma:g}/f32", "loss", dict(shape=s, gamma=gamma)))
    out.append(("loss/153x13/g2/f32/weights", "loss",
                dict(shape=(153, 13), gamma=2.0, weights=True, eps=0.1)))
    for dt in ("bf16", "f16"):
        out.append((f"loss/153x13/g0/{dt}", "loss", dict(shape=(153, 13), dtype=dt)))
    for s in SHAPES + [BIG]:
        for mode in ("platt", "temperature"):
            out.append((f"fit/{_tag(s)}/{mode}/it6", "fit", dict(shape=s, mode=mode, iters=6)))
    out.append(("fit/153x13/platt/it0", "fit", dict(shape=(153, 13), mode="platt", iters=0)))
    for s in SHAPES:
        for sb in (False, True):
            out.append((f"bins/{_tag(s)}/b15/{'map' if sb else 'raw'}", "bins",
                        dict(shape=s, n_bins=15, sb=sb)))
    for s in ((153, 13), (129, 64)):   # [129, 64] with 64 bins: the class-chunk path
        for nb in (1, 64):
            for sb in (False, True):
                out.append((f"bins/{_tag(s)}/b{nb}/{'map' if sb else 'raw'}", "bins",
                            dict(shape=s, n_bins=nb, sb=sb)))
    for s in SHAPES:
        out.append((f"grid/{_tag(s)}/t99", "grid", dict(shape=s, T=99)))
    for s in ((153, 13), (129, 64)):
        for T in (1, 256):
            out.append((f"grid/{_tag(s)}/t{T}", "grid", dict(shape=s, T=T)))
    return out


CASES = {name: (kind, kw) for name, kind, kw in cases()}


def _loss(name, dev, shape, gamma=0.0, dtype="f32", weights=False, eps=0.0):
    z, y = make_inputs(name, shape, True)
    C = shape[1]
    pw = cw = None
    if weights:
        rng = np.random.default_rng(_seed(name + "/w"))
        pw = torch.from_numpy((0.5 + 5.0 * rng.random(C)).astype(np.float32)).to(dev)
        cw = torch.from_numpy((0.5 + rng.random(C)).astype(np.float32)).to(dev)
    zd = torch.from_numpy(z).to(dev).to(DTYPES[dtype])
    yd = torch.from_numpy(y).to(dev)
    out = {}
    for red in ("mean", "sum"):
        zg = zd.clone().requires_grad_(True)
        loss, stats = F.disease_loss(zg, yd, pw, cw, gamma, eps, red)
        loss.backward()
        out[f"loss_{red}"], out[f"dz_{red}"] = loss.detach(), zg.grad
        if red == "mean":
            out["stats"] = stats
    # the normaliser the kernel divided by: the "sum" loss is the same sum over 1
    out["normaliser"] = out["loss_sum"].cpu() / out["loss_mean"].cpu()
    return out


def _fit(name, dev, shape, mode, iters):
    z, y = make_inputs(name, shape, True)
    res = F.calib_fit(torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev), mode=mode,
                      iters=iters)
    return dict(zip(("scale", "bias", "status", "info"), res))


def _bins(name, dev, shape, n_bins, sb):
    z, y = make_inputs(name, shape, False)
    scale = bias = None
    if sb:
        rng = np.random.default_rng(_seed(name + "/map"))
        scale = torch.from_numpy((0.25 + 2.0 * rng.random(shape[1])).astype(np.float32)).to(dev)
        bias = torch.from_numpy(rng.standard_normal(shape[1]).astype(np.float32)).to(dev)
    bins, n_nan = F.reliability_bins(torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev),
                                     scale, bias, n_bins)
    return {"bins": bins, "n_nan": n_nan}


def _grid(name, dev, shape, T):
    z, y = make_inputs(name, shape, False)
    thr = torch.from_numpy(np.linspace(-6.0, 6.0, T).astype(np.float32) if T > 1
                           else np.zeros(1, np.float32)).to(dev)
    tp, fp = F.confusion_grid(torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev), thr)
    return {"tp": tp, "fp": fp}


_RUN = {"loss": _loss, "fit": _fit, "bins": _bins, "grid": _grid}


def run_case(name, dev):
    """({output: sha256 of its bytes}, {output: values} for the small loss and bins cases)."""
    kind, kw = CASES[name]
    outs = _RUN[kind](name, dev, **kw)
    digests, raw = {}, {}
    small = kind in ("loss", "bins") and kw["shape"][0] * kw["shape"][1] <= RAW_MAX
    for k, t in outs.items():
        t = t.detach().cpu().contiguous().reshape(-1)
        digests[k] = hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()
        if small:
            raw[k] = t.tolist() if t.dtype == torch.int64 else t.double().tolist()
    return digests, raw


def compare(name, digests, raw, want):
    """Lines that describe every mismatch of one case against the stored file (none: equal)."""
    exp = want["digests"].get(name)
    if exp is None:
        return [f"{name}: not in the stored file"]
    lines = []
    for k in sorted(set(exp) | set(digests)):
        if exp.get(k) != digests.get(k):
            lines.append(f"{name}: {k}: stored {exp.get(k)}, computed {digests.get(k)}")
            if name in want.get("raw", {}) and k in raw:
                lines.append(f"  stored   {want['raw'][name].get(k)}")
                lines.append(f"  computed {raw[k]}")
    return lines


def _commit(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True,
                              text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--write", metavar="PATH")
    g.add_argument("--check", metavar="PATH")
    ap.add_argument("--commit", default=None, help="the commit the kernels were built from "
                    "(default: git rev-parse HEAD)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("valid_bits needs a GPU")
    dev = torch.device("cuda:0")
    if a.write:
        doc = {"rocm": torch.version.hip, "device": torch.cuda.get_device_name(0),
               "commit": _commit(a.commit), "digests": {}, "raw": {}}
        for name in CASES:
            doc["digests"][name], raw = run_case(name, dev)
            if raw:
                doc["raw"][name] = raw
        os.makedirs(os.path.dirname(os.path.abspath(a.write)), exist_ok=True)
        with open(a.write, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {len(CASES)} cases to {a.write}")
        return
    with open(a.check) as f:
        want = json.load(f)
    bad = []
    for name in CASES:
        bad += compare(name, *run_case(name, dev), want)
    bad += [f"{name}: stored, but no such case" for name in want["digests"] if name not in CASES]
    print("\n".join(bad) if bad else f"{len(CASES)} cases match {a.check} "
          f"(written at {want.get('commit')}, ROCm {want.get('rocm')})")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
