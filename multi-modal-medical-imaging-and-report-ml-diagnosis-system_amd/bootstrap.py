"""Bootstrap confidence intervals for the validation metrics: AUROC, sensitivity, specificity, F1.

The non-parametric bootstrap over ROWS (patients): replicate r draws N row indices with
replacement, and a row is resampled with all of its labels, so the correlation between classes
is kept.  The device part (functional.bootstrap_weights / bootstrap_plan / bootstrap_counts,
include/mmdx.h "bootstrap") produces exact integers per replicate,

    boot int64 [R, C + 1, 5] = (u2, w_pos, w_neg, tp, fp),   row C = the flattened (micro) problem,

and everything that turns them into numbers is a pure host function here, in float64 from the
integers, testable without a GPU:

- `intervals`: percentile intervals and standard errors of AUROC (per class, macro, micro) and
  of sensitivity, specificity and F1 (per class, micro);
- `paired_delta`: the interval and a two-sided p-value of the AUROC difference of two models
  scored on the same rows with the same seed;
- `reference_weights`, `reference_counts`: the numpy statement of the two kernels, on another
  algorithm (weighted midranks from np.unique), which the GPU tests match with zero tolerance.

The thresholds behind tp / fp are FIXED: evaluate() picks them once on the full split and every
replicate reuses them (re-picking per replicate is out of scope).  Limits: 1 <= C <= 64,
N * C <= 2^24, R * N <= 2^26 per launch.
"""
from __future__ import annotations

import math

import numpy as np

__all__ = ["GOLDEN", "MAX_CLASSES", "MAX_ITEMS", "MAX_WEIGHTS", "batch_size", "check_args",
           "reference_weights", "reference_counts", "replicate_stats", "intervals",
           "paired_delta"]

GOLDEN = 0x9E3779B97F4A7C15
MAX_CLASSES = 64
MAX_ITEMS = 2 ** 24      # N * C
MAX_WEIGHTS = 2 ** 26    # R * N per launch
_M64 = 0xFFFFFFFFFFFFFFFF


def check_args(bootstrap, ci_level=0.95, seed=0, who="evaluate"):
    """(R, level, seed) of evaluate(bootstrap=, ci_level=, bootstrap_seed=): ValueError for a
    non-integer or negative replicate count, a level outside (0, 1) or a non-integer seed."""
    if isinstance(bootstrap, bool) or not isinstance(bootstrap, (int, np.integer)) \
            or bootstrap < 0:
        raise ValueError(f"{who}: bootstrap must be a non-negative integer (replicates), got "
                         f"{bootstrap!r}")
    if isinstance(ci_level, bool) or not isinstance(ci_level, (int, float, np.floating)) \
            or not 0.0 < float(ci_level) < 1.0:
        raise ValueError(f"{who}: ci_level must lie in (0, 1), got {ci_level!r}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"{who}: bootstrap_seed must be an integer, got {seed!r}")
    return int(bootstrap), float(ci_level), int(seed) & _M64


def batch_size(R, N):
    """Replicates per launch of evaluate(): the int32 weights workspace stays <= 64 MiB."""
    return max(1, min(int(R), 2 ** 24 // int(N)))


# ----------------------------------------------------------------------------- yardsticks
def _mix64(z):
    """SplitMix64's output function on uint64 arrays (arithmetic wraps mod 2^64)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def reference_weights(R, N, seed, r0=0):
    """int32 [R, N]: the resampling weights of replicates r0 ... r0 + R - 1, the numpy
    restatement of csrc/bootstrap_rng.h.  Draw k of replicate r is
    idx = mulhi64(mix64(key_r + (k + 1) G), N) with key_r = mix64(seed ^ ((r + 1) G)), and
    w[r, i] counts the draws that hit row i: every row sums to N."""
    R, N, r0 = int(R), int(N), int(r0)
    if R < 1 or N < 1 or r0 < 0 or N >= 2 ** 32:
        raise ValueError(f"reference_weights: R = {R}, N = {N}, r0 = {r0}")
    g = np.uint64(GOLDEN)
    with np.errstate(over="ignore"):
        r = np.arange(r0 + 1, r0 + R + 1, dtype=np.uint64)
        key = _mix64(np.uint64(int(seed) & _M64) ^ (r * g))
        k = np.arange(1, N + 1, dtype=np.uint64)
        h = _mix64(key[:, None] + k[None, :] * g)
        # mulhi64(h, N) for N < 2^32 from 32-bit halves: hi * N + ((lo * N) >> 32) < 2^64
        n = np.uint64(N)
        lo, hi = h & np.uint64(0xFFFFFFFF), h >> np.uint64(32)
        idx = (hi * n + ((lo * n) >> np.uint64(32))) >> np.uint64(32)
    idx = idx.astype(np.int64)
    return np.stack([np.bincount(row, minlength=N) for row in idx]).astype(np.int32)


def _ref_column(s, pos, w, pred):
    """[R, 5] of one column: s [n] scores, pos / pred [n] bool, w int64 [R, n]."""
    live = ~np.isnan(s)
    s, pos, pred, w = s[live], pos[live], pred[live], w[:, live]
    R = w.shape[0]
    out = np.zeros((R, 5), dtype=np.int64)
    if s.size == 0:
        return out
    wp, wn = w * pos, w * ~pos
    out[:, 1], out[:, 2] = wp.sum(1), wn.sum(1)
    out[:, 3], out[:, 4] = (wp * pred).sum(1), (wn * pred).sum(1)
    vals, inv = np.unique(s, return_inverse=True)   # -0.0 == +0.0: one value
    inv = inv.reshape(-1)
    V = vals.size
    for r in range(R):
        # weight per distinct value (float64 sums of integers < 2^53 are exact)
        p_v = np.bincount(inv, weights=wp[r], minlength=V).astype(np.int64)
        n_v = np.bincount(inv, weights=wn[r], minlength=V).astype(np.int64)
        below = np.cumsum(n_v) - n_v
        # a positive beats the negatives below twice and the tied ones once: twice its weighted
        # midrank among the negatives
        out[r, 0] = int((p_v * (2 * below + n_v)).sum())
    return out


def reference_counts(scores, target, weights, pred=None):
    """int64 [R, C + 1, 5] = (u2, w_pos, w_neg, tp, fp), the numpy statement of
    functional.bootstrap_counts by weighted midranks: fp32 [N, C] scores and targets (positive
    iff > 0.5; a NaN score drops the element), integer [R, N] weights, optional bool [N, C]
    pred (tp = fp = 0 without it).  Row C is the flattened problem, element (i, c) weighing
    w[r, i]."""
    s = np.asarray(scores, dtype=np.float32)
    y = np.asarray(target, dtype=np.float32)
    w = np.asarray(weights).astype(np.int64)
    if s.ndim != 2 or y.shape != s.shape or w.ndim != 2 or w.shape[1] != s.shape[0]:
        raise ValueError(f"reference_counts: scores {s.shape}, target {y.shape}, weights "
                         f"{w.shape}")
    N, C = s.shape
    p = np.zeros((N, C), dtype=bool) if pred is None else np.asarray(pred, dtype=bool)
    if p.shape != s.shape:
        raise ValueError(f"reference_counts: pred {p.shape} for scores {s.shape}")
    pos = y > 0.5
    cols = [_ref_column(s[:, c], pos[:, c], w, p[:, c]) for c in range(C)]
    cols.append(_ref_column(s.reshape(-1), pos.reshape(-1), np.repeat(w, C, axis=1),
                            p.reshape(-1)))
    return np.stack(cols, axis=1)


# ----------------------------------------------------------------------------- statistics
def _boot_array(boot):
    if hasattr(boot, "detach"):
        boot = boot.detach().cpu().numpy()
    b = np.asarray(boot)
    if b.ndim != 3 or b.shape[2] != 5 or b.shape[1] < 2 or b.shape[0] < 1 \
            or not np.issubdtype(b.dtype, np.integer):
        raise ValueError(f"boot must be integer [R, C + 1, 5], got {b.dtype} {b.shape}")
    return b.astype(np.int64)


def _ratio(num, den):
    """num / den in float64, nan where den == 0."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(den.shape, math.nan)
    np.divide(num, den, out=out, where=den != 0)
    return out


def replicate_stats(boot):
    """The per-replicate statistics, float64 from the integers; nan = undefined there.
    "auroc" [R, C + 1] (column C micro), "auroc_macro" [R], "sensitivity", "specificity",
    "f1" [R, C + 1].

    AUROC = u2 / (2 w_pos w_neg), nan where w_pos or w_neg is 0; macro is the mean over the
    classes defined IN THAT REPLICATE (auroc_from_counts' rule), nan if none is.  Sensitivity
    = tp / w_pos and F1 = 2tp / (2tp + fp + fn) are nan where w_pos == 0, specificity
    = 1 - fp / w_neg where w_neg == 0."""
    b = _boot_array(boot)
    u2, wp, wn, tp, fp = (b[..., k] for k in range(5))
    # 2 w_pos w_neg <= 2^49: exact in int64, and in float64 after the conversion
    auroc = _ratio(u2, 2 * wp * wn)
    cls = auroc[:, :-1]
    ok = ~np.isnan(cls)
    macro = _ratio(np.where(ok, cls, 0.0).sum(1), ok.sum(1))
    f1 = _ratio(2 * tp, tp + fp + wp)       # 2tp + fp + (w_pos - tp)
    f1[wp == 0] = math.nan
    return {"auroc": auroc, "auroc_macro": macro, "sensitivity": _ratio(tp, wp),
            "specificity": 1.0 - _ratio(fp, wn), "f1": f1}


def _check_level(level):
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"level must lie in (0, 1), got {level!r}")
    return float(level)


def _leaf(x, level):
    """{"lo", "hi", "se", "n_valid"} of the replicate values x (nan = invalid replicate)."""
    v = np.asarray(x, dtype=np.float64)
    v = v[~np.isnan(v)]
    n = int(v.size)
    if n < 2:
        return {"lo": math.nan, "hi": math.nan, "se": math.nan, "n_valid": n}
    a = (1.0 - level) / 2.0
    lo, hi = np.quantile(v, [a, 1.0 - a], method="linear")
    return {"lo": float(lo), "hi": float(hi), "se": float(np.std(v, ddof=1)), "n_valid": n}


def intervals(boot, level=0.95):
    """Percentile bootstrap intervals from boot [R, C + 1, 5].  Returns "level",
    "n_replicates", and for name in (auroc, sensitivity, specificity, f1) the entries
    name_per_class (a list of C) and name_micro, plus auroc_macro; each leaf is
    {"lo", "hi", "se", "n_valid"}: np.quantile (linear) at (1 - level) / 2 and its complement
    over the valid replicates (replicate_stats: which are), their standard deviation with
    ddof = 1, and how many there were.  With n_valid < 2, lo, hi and se are nan."""
    level = _check_level(level)
    st = replicate_stats(boot)
    C = st["auroc"].shape[1] - 1
    out = {"level": level, "n_replicates": int(st["auroc"].shape[0]),
           "auroc_macro": _leaf(st["auroc_macro"], level)}
    for name in ("auroc", "sensitivity", "specificity", "f1"):
        out[f"{name}_per_class"] = [_leaf(st[name][:, c], level) for c in range(C)]
        out[f"{name}_micro"] = _leaf(st[name][:, C], level)
    return out


def paired_delta(boot_a, boot_b, level=0.95):
    """The bootstrap of AUROC(a) - AUROC(b) for two models scored on the SAME rows with the SAME
    seed: replicate r of both is the same resample, so the difference is taken per replicate.
    Identical w_pos and w_neg columns are required (ValueError otherwise: other rows, labels,
    masks or seeds).  Returns "level", "n_replicates", "per_class" (a list of C), "macro" and
    "micro"; each is an intervals() leaf of the differences plus
    p_two_sided = min(1, 2 min(#(d <= 0) + 1, #(d >= 0) + 1) / (n_valid + 1))."""
    level = _check_level(level)
    a, b = _boot_array(boot_a), _boot_array(boot_b)
    if a.shape != b.shape or not np.array_equal(a[..., 1:3], b[..., 1:3]):
        raise ValueError("paired_delta: the two bootstraps differ in shape or in their w_pos / "
                         "w_neg columns: not the same rows, labels and seed")
    sa, sb = replicate_stats(a), replicate_stats(b)

    def leaf(d):
        out = _leaf(d, level)
        v = d[~np.isnan(d)]
        tail = min(int((v <= 0).sum()) + 1, int((v >= 0).sum()) + 1)
        out["p_two_sided"] = min(1.0, 2.0 * tail / (out["n_valid"] + 1))
        return out

    d = sa["auroc"] - sb["auroc"]
    C = d.shape[1] - 1
    return {"level": level, "n_replicates": int(d.shape[0]),
            "per_class": [leaf(d[:, c]) for c in range(C)],
            "macro": leaf(sa["auroc_macro"] - sb["auroc_macro"]), "micro": leaf(d[:, C])}
