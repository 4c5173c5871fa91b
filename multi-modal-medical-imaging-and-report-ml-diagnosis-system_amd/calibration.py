"""Probability calibration of the multi-label disease head: definitions and host-side math.

A calibration is a monotone per-class map of the logits, z' = a_c z + b_c, p = sigmoid(z'):

- mode "temperature": one scalar a for all classes, b = 0;
- mode "platt":       a free (a_c, b_c) per class (Platt scaling).  The bias is the term that
  undoes the log(pos_weight) shift a weighted loss puts into the logits.

As a value it is the JSON-safe dict {"mode": str, "scale": [C floats], "bias": [C floats]}
(`to_dict` / `from_dict` / `check_calibration`); the identity is scale = 1, bias = 0.

Objective.  A NaN target is "no label" (m = 0); any other target is a label y in [0, 1].  With
smooth=True (default) the targets are Platt's, t = t_neg_c + y (t_pos_c - t_neg_c) with
t_pos_c = (n_pos_c + 1) / (n_pos_c + 2), t_neg_c = 1 / (n_neg_c + 2), n_pos_c = sum m y,
n_neg_c = sum m (1 - y), which keep the optimum finite on separable data; smooth=False uses
t = y.  Minimised is NLL_c = sum_i m (softplus(z') - t z').

Solver: damped Newton (Levenberg-Marquardt), deterministic and free of host syncs on the device.
Start at (1, 0) with lambda = 1e-3.  Every pass evaluates NLL, gradient (ga, gb) and Hessian
(haa, hab, hbb) at the trial point.  If NLL <= NLL_accepted (1 + 1e-9) the point is accepted and
lambda /= 10 (floor 1e-9); otherwise it is rejected and lambda *= 10 (cap 1e12).  The next trial
point is theta_acc - (H_acc with its diagonal scaled by (1 + lambda))^-1 g_acc, rounded to
float32 (the device evaluates in float32 logit arithmetic, so the accepted point is exactly the
one that was evaluated).  `iters` such passes are followed by one more that evaluates the last
trial point; the result is the accepted point after it.  In temperature mode ga, haa and the NLL
are summed over the classes in class order and b stays 0.

Status per class (temperature mode: one status for all classes, from the pooled sums), decided
in the last pass; anything but 0 returns the identity:
  0 fitted;
  1 inactive: fewer than `min_count` positives (sum m y) or negatives (sum m (1 - y));
  2 not converged: the Newton decrement g^T H^-1 g per labelled element exceeds `tol`, or a
    value is not finite;
  3 non-positive slope a <= 0 (the map would reverse the ranking).

`reference_fit` is this text in float64 numpy, the yardstick of functional.calib_fit (one HIP
launch per pass, csrc/calibration.hip).  `calibration_from_bins` turns the integer sums of
functional.reliability_bins into ECE / MCE / Brier and the reliability curve, in float64 from
exact integers, on the host.
"""
from __future__ import annotations

import math

import numpy as np

__all__ = ["MODES", "STATUS_FITTED", "STATUS_INACTIVE", "STATUS_NOT_CONVERGED",
           "STATUS_BAD_SLOPE", "FIXED_ONE", "reference_fit", "apply", "bin_edges",
           "calibration_from_bins", "check_calibration", "to_dict", "from_dict", "identity"]

MODES = ("temperature", "platt")
STATUS_FITTED, STATUS_INACTIVE, STATUS_NOT_CONVERGED, STATUS_BAD_SLOPE = 0, 1, 2, 3
FIXED_ONE = 1 << 30           # reliability_bins sums probabilities as round(p * 2^30)
MAX_BINS = 64
MAX_CLASSES = 64              # as the metrics kernels

LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-9, 1e12
ACCEPT_SLACK = 1e-9


def check_fit_args(mode, iters, min_count, tol):
    """The host-side checks functional.calib_fit and reference_fit share."""
    if mode not in MODES:
        raise ValueError(f"calibration mode must be one of {MODES}, got {mode!r}")
    if not isinstance(iters, int) or isinstance(iters, bool) or not 0 <= iters <= 1000:
        raise ValueError(f"iters must be an int in [0, 1000], got {iters!r}")
    if not isinstance(min_count, int) or isinstance(min_count, bool) or min_count < 0:
        raise ValueError(f"min_count must be an int >= 0, got {min_count!r}")
    tol = float(tol)
    if not tol > 0.0 or not math.isfinite(tol):
        raise ValueError(f"tol must be a finite value > 0, got {tol!r}")
    return tol


def _np(x, dtype):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


def _sums(z, t, m, a, b, elem):
    """The seven per-class sums at (a, b): element terms in `elem`, sums in float64."""
    with np.errstate(all="ignore"):
        u = z.astype(elem) * a.astype(elem)[None, :]
        u = u + b.astype(elem)[None, :]
        e = np.exp(-np.abs(u))
        l1p = np.log1p(e)
        hi, lo = 1.0 / (1.0 + e), e / (1.0 + e)
        p = np.where(u >= 0, hi, lo).astype(np.float64)
        q = np.where(u >= 0, lo, hi).astype(np.float64)
        u = u.astype(np.float64)
        zz = z.astype(np.float64)
        nll = np.maximum(u, 0.0) + l1p.astype(np.float64) - t * u
        d, w = p - t, p * q

        def s(x):
            return np.where(m, x, 0.0).sum(0)
        return (s(nll), s(d * zz), s(d), s(w * zz * zz), s(w * zz), s(w),
                m.sum(0).astype(np.float64))


def _fit(z, y, mode, iters, smooth, min_count, tol, elem):
    N, C = z.shape
    m = ~np.isnan(y)
    y0 = np.where(m, y, 0.0).astype(np.float64)
    n_pos = y0.sum(0)
    n_neg = np.where(m, 1.0 - y0, 0.0).sum(0)
    if smooth:
        t_pos, t_neg = (n_pos + 1.0) / (n_pos + 2.0), 1.0 / (n_neg + 2.0)
    else:
        t_pos, t_neg = np.ones(C), np.zeros(C)
    t = t_neg[None, :] + y0 * (t_pos - t_neg)[None, :]
    temp = mode == "temperature"

    a_t, b_t = np.ones(C), np.zeros(C)
    a_acc, b_acc = np.ones(C), np.zeros(C)
    lam = np.full(C, LAMBDA0)
    f_acc = np.full(C, np.inf)
    acc = [np.zeros(C) for _ in range(7)]   # nll, ga, gb, haa, hab, hbb, n at the accepted point
    f0 = None
    with np.errstate(all="ignore"):
        for it in range(iters + 1):
            cur = list(_sums(z, t, m, a_t, b_t, elem))
            if temp:   # pooled over the classes, in class order
                cur = [np.full(C, math.fsum(v) if elem is np.float64 else float(np.sum(v)))
                       for v in cur]
            if it == 0:
                f0 = cur[0].copy()
                acc[6] = cur[6].copy()
            ok = cur[0] <= f_acc + ACCEPT_SLACK * np.abs(f_acc)
            a_acc, b_acc = np.where(ok, a_t, a_acc), np.where(ok, b_t, b_acc)
            acc = [np.where(ok, c, o) for c, o in zip(cur, acc)]
            f_acc = np.where(ok, cur[0], f_acc)
            lam = np.where(ok, np.maximum(lam / 10.0, LAMBDA_MIN),
                           np.minimum(lam * 10.0, LAMBDA_MAX))
            if it == iters:
                break
            _, ga, gb, haa, hab, hbb, _ = acc
            if temp:
                den = haa * (1.0 + lam)
                good = np.isfinite(den) & (den > 0) & np.isfinite(ga)
                da, db = np.where(good, ga / np.where(good, den, 1.0), 0.0), np.zeros(C)
            else:
                A, D = haa * (1.0 + lam), hbb * (1.0 + lam)
                det = A * D - hab * hab
                good = np.isfinite(det) & (det > 0) & np.isfinite(ga) & np.isfinite(gb)
                dd = np.where(good, det, 1.0)
                da = np.where(good, (D * ga - hab * gb) / dd, 0.0)
                db = np.where(good, (A * gb - hab * ga) / dd, 0.0)
            # the device evaluates at the float32 rounding of the trial point
            a_t = (a_acc - da).astype(np.float32).astype(np.float64)
            b_t = (b_acc - db).astype(np.float32).astype(np.float64)

        f, ga, gb, haa, hab, hbb, n = acc
        if temp:
            dec = ga * ga / haa
            pos, neg = np.full(C, n_pos.sum()), np.full(C, n_neg.sum())
        else:
            dec = (hbb * ga * ga - 2.0 * hab * ga * gb + haa * gb * gb) / (haa * hbb - hab * hab)
            pos, neg = n_pos, n_neg
        dec = dec / np.maximum(n, 1.0)
        finite = np.isfinite(f) & np.isfinite(dec) & np.isfinite(a_acc) & np.isfinite(b_acc)
        status = np.where((pos < min_count) | (neg < min_count) | (n < 1), STATUS_INACTIVE,
                          np.where(~finite | ~(dec <= tol), STATUS_NOT_CONVERGED,
                                   np.where(a_acc <= 0, STATUS_BAD_SLOPE, STATUS_FITTED)))
    fitted = status == STATUS_FITTED
    return {"mode": mode,
            "scale": np.where(fitted, a_acc, 1.0).astype(np.float32),
            "bias": np.where(fitted, b_acc, 0.0).astype(np.float32),
            "status": status.astype(np.int32),
            "info": np.stack([f0, f, dec, acc[6]], axis=1),
            "raw_scale": a_acc, "raw_bias": b_acc}


def reference_fit(logits, target, mode="platt", iters=32, smooth=True, min_count=1, tol=1e-7):
    """The module docstring in float64 numpy.  logits, target: [N, C] arrays or tensors (the
    logits are read as float32 values, as the device sees them).  Returns a dict: mode, scale
    and bias (float32 [C], the identity where status != 0), status (int32 [C]), info (float64
    [C, 4]: NLL at the identity, NLL at the result, Newton decrement per labelled element,
    labelled count) and raw_scale / raw_bias (float64 [C], the accepted point whatever the
    status)."""
    tol = check_fit_args(mode, iters, min_count, tol)
    z, y = _np(logits, np.float32), _np(target, np.float64)
    if z.ndim != 2 or z.shape != y.shape or z.shape[0] < 1 or not 1 <= z.shape[1] <= MAX_CLASSES:
        raise ValueError(f"reference_fit takes logits and targets of one shape [N, C <= "
                         f"{MAX_CLASSES}], got {z.shape} and {y.shape}")
    return _fit(z, y, mode, iters, bool(smooth), min_count, tol, np.float64)


# ------------------------------------------------------------------------------ the map
def identity(C, mode="platt"):
    return {"mode": mode, "scale": [1.0] * C, "bias": [0.0] * C}


def check_calibration(calibration, C):
    """Raise ValueError unless `calibration` is a calibration dict for C classes: a known mode,
    scale and bias of C finite numbers each, every scale > 0; temperature mode additionally
    needs one common scale and zero biases.  Returns (scale, bias) as lists of floats."""
    if not isinstance(calibration, dict):
        raise ValueError(f"a calibration is a dict, got {type(calibration).__name__}")
    miss = [k for k in ("mode", "scale", "bias") if k not in calibration]
    if miss:
        raise ValueError(f"calibration lacks {miss}")
    mode = calibration["mode"]
    if mode not in MODES:
        raise ValueError(f"calibration mode must be one of {MODES}, got {mode!r}")
    out = []
    for k in ("scale", "bias"):
        v = calibration[k]
        v = v.tolist() if hasattr(v, "tolist") else v
        if not isinstance(v, (list, tuple)) or len(v) != C:
            raise ValueError(f"calibration[{k!r}] must list {C} numbers")
        try:
            v = [float(x) for x in v]
        except (TypeError, ValueError):
            raise ValueError(f"calibration[{k!r}] must list {C} numbers") from None
        if not all(math.isfinite(x) for x in v):
            raise ValueError(f"calibration[{k!r}] is not finite: {v}")
        out.append(v)
    scale, bias = out
    if not all(s > 0.0 for s in scale):
        raise ValueError(f"calibration scale must be > 0 (a monotone map), got {scale}")
    if mode == "temperature" and (len(set(scale)) != 1 or any(b != 0.0 for b in bias)):
        raise ValueError("a temperature calibration has one common scale and zero biases")
    return scale, bias


def to_dict(mode, scale, bias, status=None):
    """The JSON-safe dict from a mode and per-class scale / bias (tensors, arrays or lists);
    `status` (optional, the fit's status codes) is stored as a list of ints."""
    def lst(v, conv):
        if hasattr(v, "detach"):
            v = v.detach().cpu()
        return [conv(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]
    d = {"mode": str(mode), "scale": lst(scale, float), "bias": lst(bias, float)}
    if status is not None:
        d["status"] = lst(status, int)
    check_calibration(d, len(d["scale"]))
    return d


def from_dict(calibration, C=None, device=None):
    """(scale, bias) as float32 torch tensors [C] on `device`, after check_calibration."""
    import torch
    if C is None:
        C = len(calibration.get("scale", ())) if isinstance(calibration, dict) else 0
    scale, bias = check_calibration(calibration, C)
    return (torch.tensor(scale, dtype=torch.float32, device=device),
            torch.tensor(bias, dtype=torch.float32, device=device))


def apply(logits, calibration):
    """z' = z * scale + bias in float32, one multiply and one add as the kernels do it (so the
    calibrated logits are the same bits on the host, on the device and in the kernels).  logits:
    a [..., C] torch tensor (the result stays on its device) or numpy array."""
    C = logits.shape[-1]
    scale, bias = check_calibration(calibration, C)
    if hasattr(logits, "detach"):
        import torch
        s = torch.tensor(scale, dtype=torch.float32, device=logits.device)
        b = torch.tensor(bias, dtype=torch.float32, device=logits.device)
        return logits.float() * s + b
    z = np.asarray(logits, dtype=np.float32)
    return z * np.asarray(scale, np.float32) + np.asarray(bias, np.float32)


# ------------------------------------------------------------------------------ reliability
def bin_edges(n_bins):
    """The n_bins - 1 interior edges k / n_bins in logit space (metrics.grid_logits: float64
    log-odds rounded to float32, 0.5 -> 0.0 exactly).  Bin index of a logit = #{edges <= z}."""
    from .metrics import grid_logits
    if not isinstance(n_bins, int) or isinstance(n_bins, bool) or not 1 <= n_bins <= MAX_BINS:
        raise ValueError(f"n_bins must be an int in [1, {MAX_BINS}], got {n_bins!r}")
    if n_bins == 1:
        return np.zeros(0, dtype=np.float32)
    return grid_logits([k / n_bins for k in range(1, n_bins)])


def calibration_from_bins(bins, n_nan):
    """ECE, MCE, Brier score and the reliability curve from functional.reliability_bins.

    bins: integer [(C + 1), n_bins, 4] = (count, positives, sum round(p 2^30),
    sum round((p - y)^2 2^30)) per probability bin, row C = micro (all classes pooled); n_nan:
    integer [(C + 1)], the dropped NaN logits.  In float64 from the integers, with n = the
    row's total count:
      ECE   = (1 / n) sum_k |sum p_k - pos_k|
      MCE   = max over non-empty bins of |mean p_k - pos_k / n_k|
      Brier = sum (p - y)^2 / n
    A row without elements gives nan for all three.  Returns {"n_bins", "per_class": [row dict
    per class], "micro": row dict}; a row dict has ece, mce, brier, n, n_nan and the per-bin
    lists mean_p, frac_pos (None in an empty bin) and count."""
    if hasattr(bins, "detach"):
        bins = bins.detach().cpu().numpy()
    if hasattr(n_nan, "detach"):
        n_nan = n_nan.detach().cpu().numpy()
    k = np.asarray(bins, dtype=np.int64)
    nn = np.asarray(n_nan, dtype=np.int64)
    if k.ndim != 3 or k.shape[2] != 4 or k.shape[0] < 2 or k.shape[1] < 1 or \
            nn.shape != (k.shape[0],):
        raise ValueError(f"bins must be [(C + 1), n_bins, 4] and n_nan [(C + 1)], got "
                         f"{k.shape} and {nn.shape}")

    def row(r):
        cnt = [int(v) for v in k[r, :, 0]]
        pos = [int(v) for v in k[r, :, 1]]
        sp = [int(v) / FIXED_ONE for v in k[r, :, 2]]
        n = sum(cnt)
        out = {"n": n, "n_nan": int(nn[r]), "count": cnt,
               "mean_p": [s / c if c else None for s, c in zip(sp, cnt)],
               "frac_pos": [p / c if c else None for p, c in zip(pos, cnt)]}
        if n == 0:
            out.update(ece=math.nan, mce=math.nan, brier=math.nan)
            return out
        out["ece"] = math.fsum(abs(s - p) for s, p in zip(sp, pos)) / n
        out["mce"] = max(abs(s / c - p / c) for s, p, c in zip(sp, pos, cnt) if c)
        out["brier"] = sum(int(v) for v in k[r, :, 3]) / FIXED_ONE / n
        return out

    C = k.shape[0] - 1
    return {"n_bins": int(k.shape[1]), "per_class": [row(c) for c in range(C)], "micro": row(C)}
