"""Validation metrics of the multi-label disease head and the report head.

The device part is two integer-count kernels (functional.auroc_counts / confusion_grid, see
include/mmdx.h "validation metrics"); everything that turns counts into numbers is a pure host
function here, in float64 from exact integers, so it can be tested without a GPU:

- `auroc_from_counts`: Mann-Whitney AUROC (midranks for ties) per class, macro and micro;
- `pick_thresholds`: per-class F1-optimal probability thresholds from a threshold sweep;
- `rouge_l`: token-id ROUGE-L F1 of generated reports;
- `evaluate`: the loop that feeds them from held-out batches (and, with `calibrate`, fits and
  measures a probability calibration: mmdx.calibration; with `bootstrap`, adds row-bootstrap
  confidence intervals: mmdx.bootstrap).

`evaluate()` runs in ONE process: pair counts need every score on one rank, so data-parallel
evaluation is out of scope (gather the logits to one rank first).  The AUROC kernel counts all
pairs, which bounds a validation set at N * 13 <= 2^24 scores (N <= 1,290,555 rows).
"""
from __future__ import annotations

import math

import numpy as np
import torch

__all__ = ["default_grid", "grid_logits", "auroc_from_counts", "pick_thresholds", "rouge_l",
           "evaluate"]


def default_grid():
    """0.01 ... 0.99 in steps of 0.01; 0.5 is in it exactly once (50 / 100 == 0.5)."""
    return [k / 100.0 for k in range(1, 100)]


def grid_logits(grid_probs):
    """The probability grid in logit space: log(p / (1 - p)) in float64, rounded to float32;
    0.5 is passed as logit 0.0 exactly.  Monotone, so a sorted grid stays sorted."""
    g = np.asarray(grid_probs, dtype=np.float64)
    if g.ndim != 1 or g.size < 1 or not np.all((g > 0.0) & (g < 1.0)):
        raise ValueError("grid_probs must be a non-empty 1-D list of probabilities in (0, 1)")
    if np.any(np.diff(g) <= 0.0):
        raise ValueError("grid_probs must be strictly increasing")
    z = np.log(g / (1.0 - g))
    z[g == 0.5] = 0.0
    return z.astype(np.float32)


def _int_array(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.int64)


def auroc_from_counts(counts):
    """(per_class, macro, micro) from the int64 [(C + 1), 4] rows (u2, n_pos, n_neg, n_nan) of
    functional.auroc_counts: AUROC = u2 / (2 n_pos n_neg), the integers divided in float64.
    A class without positives or without negatives is nan and left out of the macro mean
    (nan if no class is defined); micro is nan only if the flattened set has one label.
    Raises ValueError naming the classes if any score was NaN."""
    k = _int_array(counts)
    if k.ndim != 2 or k.shape[1] != 4 or k.shape[0] < 2:
        raise ValueError(f"counts must be [(C + 1), 4], got {k.shape}")
    C = k.shape[0] - 1
    bad = [c for c in range(C) if k[c, 3] > 0]
    if bad or k[C, 3] > 0:
        raise ValueError(f"NaN scores in class(es) {bad} ({int(k[C, 3])} in all): AUROC is "
                         "undefined")

    def one(u2, n_pos, n_neg):
        if n_pos == 0 or n_neg == 0:
            return math.nan
        return float(int(u2)) / float(2 * int(n_pos) * int(n_neg))

    per_class = [one(*k[c, :3]) for c in range(C)]
    defined = [v for v in per_class if not math.isnan(v)]
    macro = math.fsum(defined) / len(defined) if defined else math.nan
    return per_class, macro, one(*k[C, :3])


def _prf(tp, fp, n_pos):
    """precision, recall, F1 in float64 from integer counts (0 where a denominator is 0);
    F1 = 2tp / (2tp + fp + fn)."""
    tp, fp, n_pos = int(tp), int(fp), int(n_pos)
    fn = n_pos - tp
    p = tp / (tp + fp) if tp + fp else 0.0
    r = tp / n_pos if n_pos else 0.0
    d = 2 * tp + fp + fn
    return p, r, (2 * tp / d if d else 0.0)


def pick_thresholds(tp, fp, n_pos, grid_probs, min_pos=1):
    """Per-class probability thresholds that maximise F1 on a threshold sweep.

    tp, fp: integer [C][T] counts of positives / negatives at or above grid point t
    (functional.confusion_grid on grid_logits(grid_probs)); n_pos: [C] positives per class.
    The winner of a class is the grid point of maximal F1 (float64 from the integers); ties go
    to the point nearest 0.5, then to the lower one.  A class with fewer than `min_pos`
    positives keeps 0.5.  grid_probs must contain 0.5.

    Returns a dict: "thresholds" (the chosen grid PROBABILITIES), "per_class" (a dict per class:
    precision, recall, f1, n_pos at the chosen threshold, and *_at_0p5), "micro" and
    "micro_at_0p5" (precision, recall, f1 over all classes' summed counts).

    The sweep compares logits with the float32 logit of each grid point, while inference()
    compares float32 sigmoid outputs with the stored probability: a logit within rounding of a
    threshold can land on the other side there."""
    tp, fp, n_pos = _int_array(tp), _int_array(fp), _int_array(n_pos)
    g = [float(p) for p in grid_probs]
    C, T = tp.shape
    if fp.shape != (C, T) or n_pos.shape != (C,) or len(g) != T:
        raise ValueError("pick_thresholds: tp, fp [C][T], n_pos [C] and grid_probs [T] disagree")
    if 0.5 not in g:
        raise ValueError("pick_thresholds: grid_probs must contain 0.5")
    i_half = g.index(0.5)
    chosen = []
    for c in range(C):
        if n_pos[c] < min_pos:
            chosen.append(i_half)
            continue
        f1 = [_prf(tp[c, t], fp[c, t], n_pos[c])[2] for t in range(T)]
        chosen.append(min(range(T), key=lambda t: (-f1[t], round(abs(g[t] - 0.5), 12), g[t])))
    per_class = []
    for c, t in enumerate(chosen):
        p, r, f = _prf(tp[c, t], fp[c, t], n_pos[c])
        p5, r5, f5 = _prf(tp[c, i_half], fp[c, i_half], n_pos[c])
        per_class.append({"precision": p, "recall": r, "f1": f, "n_pos": int(n_pos[c]),
                          "precision_at_0p5": p5, "recall_at_0p5": r5, "f1_at_0p5": f5})

    def micro(idx):
        p, r, f = _prf(sum(int(tp[c, t]) for c, t in enumerate(idx)),
                       sum(int(fp[c, t]) for c, t in enumerate(idx)), int(n_pos.sum()))
        return {"precision": p, "recall": r, "f1": f}

    return {"thresholds": [g[t] for t in chosen], "per_class": per_class,
            "micro": micro(chosen), "micro_at_0p5": micro([i_half] * C)}


def _lcs(a, b):
    if not a or not b:
        return 0
    b = np.asarray(b)
    row = np.zeros(len(b) + 1, dtype=np.int64)
    for x in a:
        hit = row[:-1] + (b == x)          # diagonal + 1 where the tokens match
        new = np.maximum(row[1:], hit)     # max(up, diagonal)
        row[1:] = np.maximum.accumulate(new)  # max with left (hits raise a cell by <= 1)
    return int(row[-1])


def rouge_l(pred_ids, ref_ids, ignore=(0, 1, -100)):
    """Mean token-level ROUGE-L F1 over a batch: F = 2PR / (P + R), P = LCS / len(pred),
    R = LCS / len(ref), 0 where either side is empty (after dropping the `ignore` ids: pad,
    eos and the loss mask).  Computed on the host over token IDS, not words: no SentencePiece
    model exists offline, so the ids are whatever tokenizer produced the references."""
    def rows(x):
        return x.tolist() if torch.is_tensor(x) or isinstance(x, np.ndarray) else list(x)
    P, Rf = rows(pred_ids), rows(ref_ids)
    if len(P) != len(Rf):
        raise ValueError(f"rouge_l: {len(P)} predictions for {len(Rf)} references")
    if not P:
        return 0.0
    drop = set(ignore)
    total = 0.0
    for p, r in zip(P, Rf):
        p = [int(t) for t in p if int(t) not in drop]
        r = [int(t) for t in r if int(t) not in drop]
        n = _lcs(p, r)
        if n:
            pr, rc = n / len(p), n / len(r)
            total += 2 * pr * rc / (pr + rc)
    return total / len(P)


def _append_rows(buf, n, rows):
    """buf[n : n + len(rows)] = rows on the device, growing buf (x2) when it is full."""
    need = n + rows.shape[0]
    if need > buf.shape[0]:
        grown = torch.empty((max(need, 2 * buf.shape[0]),) + tuple(buf.shape[1:]),
                            dtype=buf.dtype, device=buf.device)
        grown[:n].copy_(buf[:n])
        buf = grown
    buf[n:need].copy_(rows)
    return buf, need


def _calibration_report(x, C, n_bins, ignored, mode):
    """The "calibration" entry of evaluate() from the int64 words of the one host copy, in the
    order evaluate() packed them."""
    from . import calibration as K
    nb = (C + 1) * n_bins * 4
    sides, o = [], 0
    for _ in range(2):
        bins = x[o:o + nb].reshape(C + 1, n_bins, 4)
        n_nan = x[o + nb:o + nb + C + 1].copy()
        n_nan[:C] -= ignored        # what is left is a NaN the model produced
        n_nan[C] -= ignored.sum()
        sides.append(K.calibration_from_bins(bins, n_nan))
        o += nb + C + 1

    def f32(w):
        return np.ascontiguousarray(w).astype(np.int32).view(np.float32)

    scale, bias = f32(x[o:o + C]), f32(x[o + C:o + 2 * C])
    status = [int(v) for v in x[o + 2 * C:o + 3 * C]]
    o += 3 * C
    nll = [np.ascontiguousarray(x[o + i * C:o + (i + 1) * C]).view(np.float64) for i in range(3)]
    n_lab = nll[2]  # labelled elements per class (the evaluation passes run per class)

    def side(rel, s):
        tot = float(n_lab.sum())
        d = {"val_nll_per_class": [float(v) / float(m) if m > 0 else math.nan
                                   for v, m in zip(s, n_lab)],
             "val_nll_micro": math.fsum(float(v) for v in s) / tot if tot > 0 else math.nan}
        for k in ("ece", "mce", "brier"):
            d[f"val_{k}_micro"] = rel["micro"][k]
            d[f"val_{k}_per_class"] = [r[k] for r in rel["per_class"]]
        keep = ("mean_p", "frac_pos", "count")
        d["reliability"] = {"micro": {k: rel["micro"][k] for k in keep},
                            "per_class": [{k: r[k] for k in keep} for r in rel["per_class"]]}
        return d

    out = K.to_dict(mode, scale, bias, status)
    out.update(n_bins=n_bins, before=side(sides[0], nll[0]), after=side(sides[1], nll[1]))
    return out


def evaluate(image_encoder, text_encoder, fusion_model, batches, *, tokenize=None,
             grid_probs=None, generate=False, gen_kwargs=None, report_labels=None,
             compute_dtype=None, criterion=None, calibrate=None, n_bins=15, bootstrap=0,
             ci_level=0.95, bootstrap_seed=0):
    """Validation metrics of the three modules over `batches`, an iterable of
    (images, patient_details, labels) as data.LocalCXRBatches yields them.

    The modules run in eval mode under no_grad (every submodule's `training` flag is put back
    on exit, also on an exception).  Each batch's fp32 disease logits and its labels are
    written into device buffers [N, n_disease] (sized from len(batches) when it has one, grown
    on the device otherwise) with no host sync inside the loop; afterwards the validation BCE
    (mmdx_bce_logits_fwd over the whole buffer), the AUROC pair counts and the confusion grid
    are computed on the device and reach the host in ONE copy.  `tokenize` maps a list of
    patient_details strings to the text encoder's inputs (default tokenize_patient_details,
    max_len 96); `compute_dtype` casts the embeddings handed to the fusion model (None: as the
    encoders produce them); `grid_probs` defaults to default_grid() and gets 0.5 added if absent.

    `criterion` (an mmdx.DiseaseLoss) computes val_loss instead of the plain BCE; None keeps the
    plain BCE, which is NaN if a label is.  Independently of it, an ignored label (NaN, see
    data.apply_uncertain) is left out of AUROC, the threshold sweep and n_pos: its score is
    masked on the device and the per-class counts of masked elements travel in the same copy.
    A NaN the model produced at a labelled element still raises (auroc_from_counts).

    generate=True (needs the report head and `report_labels`, int64 [N, L] token ids in batch
    order, -100 / pad ignored) beam-generates a report per row with `gen_kwargs` and scores
    token-id ROUGE-L; generation syncs with the host per batch, the metric path does not.

    `calibrate` (default None: today's launches, bits and keys) measures and repairs the
    probabilities (mmdx.calibration).  "temperature" or "platt" fits that map on the collected
    rows (functional.calib_fit); a calibration dict is applied without fitting, so a map fitted
    on one split can be measured on another.  The result then gains "calibration": the dict
    (mode, scale, bias) plus status, n_bins and, under "before" and "after", val_ece_micro /
    _per_class, val_mce_*, val_brier_*, val_nll_* (the plain BCE of the labelled elements) and
    "reliability" (per class and micro: mean_p, frac_pos and count per bin, `n_bins`
    equal-width bins).  The threshold sweep then runs on the CALIBRATED logits, so `thresholds`
    refer to the probabilities inference() reports from a bundle that carries the map; AUROC
    stays on the raw logits (the map is monotone, and the identity where a class was not
    fitted, so it is the uncalibrated number exactly).  Ignored labels are left out of the fit
    and of the bins.  Everything new travels in the same single copy.  "after" numbers of a
    map fitted on the same rows are IN-SAMPLE: they show what the map can do, not what it will
    do on new data.

    `bootstrap` = R > 0 (default 0: today's launches, copies, keys and bits) adds R bootstrap
    replicates over ROWS (mmdx.bootstrap) after that copy.  The thresholds are picked on the host
    as always, go back to the device, and stay FIXED: pred = (the swept logits >= the chosen
    threshold's grid logit), so a replicate re-weights the confusion counts of the chosen grid
    points but never re-picks a threshold.  The sort plan is built from the raw masked logits
    (AUROC stays the uncalibrated number); the replicates run in batches of
    mmdx.bootstrap.batch_size(R, n) (weights workspace <= 64 MiB) and all of them reach the host
    in ONE further copy: two copies with bootstrap, one without.  The result gains "boot", the
    int64 [R, C + 1, 5] array itself (for mmdx.bootstrap.paired_delta), and "ci": level,
    n_replicates, seed, and an mmdx.bootstrap.intervals leaf {lo, hi, se, n_valid} for
    val_auroc_micro, val_auroc_macro, each of val_auroc_per_class, val_f1_micro and, under
    per_class, each class's sensitivity, specificity and f1 at its threshold.  `ci_level` is the
    coverage, `bootstrap_seed` the stream (same seed and rows = same resamples, which is what
    paired_delta needs).

    Returns n, val_loss, val_auroc_micro, val_auroc_macro, val_auroc_per_class, thresholds,
    val_f1_micro (at the chosen thresholds), val_f1_micro_at_0p5, per_class (precision, recall,
    f1, n_pos, ...) and, with generate, val_rougeL.  Single process only (module docstring)."""
    from . import functional as F
    from .training_pipeline import tokenize_patient_details

    if tokenize is None:
        def tokenize(texts):
            return tokenize_patient_details(texts, max_len=96)
    from . import bootstrap as B
    n_boot, ci_level, bootstrap_seed = B.check_args(bootstrap, ci_level, bootstrap_seed)
    grid = sorted(set(float(p) for p in (grid_probs if grid_probs is not None
                                         else default_grid())) | {0.5})
    thr_host = grid_logits(grid)
    has_head = getattr(fusion_model, "report_model", None) is not None
    if generate and has_head and report_labels is None:
        raise ValueError("evaluate(generate=True) needs report_labels")
    if calibrate is not None:
        from . import calibration as K
        if isinstance(calibrate, str):
            if calibrate not in K.MODES:
                raise ValueError(f"evaluate: calibrate must be None, one of {K.MODES} or a "
                                 f"calibration dict, got {calibrate!r}")
        elif not isinstance(calibrate, dict):
            raise TypeError(f"evaluate: calibrate must be None, one of {K.MODES} or a "
                            f"calibration dict, got {type(calibrate).__name__}")
        K.bin_edges(n_bins)
    modules = (image_encoder, text_encoder, fusion_model)
    flags = [(m, m.training) for top in modules for m in top.modules()]
    logits_buf = labels_buf = None
    n = 0
    gen_ids = []
    try:
        for top in modules:
            top.eval()
        with torch.no_grad():
            for images, details, labels in batches:
                tok = tokenize(list(details))
                tok = {k: v.to(images.device) for k, v in tok.items()}
                z_img = image_encoder(images)["embeddings"]
                z_txt = text_encoder(**tok)["embeddings"]
                if compute_dtype is not None:
                    z_img, z_txt = z_img.to(compute_dtype), z_txt.to(compute_dtype)
                logits = fusion_model(z_img=z_img, z_txt=z_txt,
                                      report_labels=None)["disease_logits"]
                if logits_buf is None:
                    try:
                        cap = len(batches) * labels.shape[0]
                    except TypeError:
                        cap = 4 * labels.shape[0]
                    cap = max(cap, labels.shape[0])
                    logits_buf = torch.empty((cap, logits.shape[1]), dtype=torch.float32,
                                             device=logits.device)
                    labels_buf = torch.empty_like(logits_buf)
                logits_buf, _ = _append_rows(logits_buf, n, logits.float())
                labels_buf, n = _append_rows(labels_buf, n, labels.float())
                if generate and has_head:
                    gen_ids.append(fusion_model.generate(z_img, z_txt, **(gen_kwargs or {})))
            if n == 0:
                raise ValueError("evaluate: no validation rows")
            z, y = logits_buf[:n], labels_buf[:n]
            loss = F.bce_with_logits(z, y) if criterion is None else criterion(z, y)
            # an ignored (NaN) label becomes a NaN score with target 0: the metrics kernels
            # drop NaN scores and count them in n_nan, from which `ignored` is taken off below
            ign = torch.isnan(y)
            ignored = ign.sum(0)
            zm = torch.where(ign, torch.full_like(z, math.nan), z)
            ym = torch.where(ign, torch.zeros_like(y), y)
            counts = F.auroc_counts(zm, ym)
            thr = torch.from_numpy(thr_host).to(z.device)
            extra = []
            z_sweep = zm
            if calibrate is not None:
                if isinstance(calibrate, str):
                    scale, bias, status, _ = F.calib_fit(z, y, mode=calibrate)
                    cal_mode = calibrate
                else:
                    scale, bias = K.from_dict(calibrate, z.shape[1], z.device)
                    status = torch.tensor([int(v) for v in calibrate.get(
                        "status", [0] * z.shape[1])], dtype=torch.int32, device=z.device)
                    cal_mode = calibrate["mode"]
                z_cal = z * scale + bias  # a multiply and an add, as the kernels compute z'
                z_sweep = torch.where(ign, torch.full_like(z, math.nan), z_cal)
                bins0, nan0 = F.reliability_bins(zm, ym, n_bins=n_bins)
                bins1, nan1 = F.reliability_bins(zm, ym, scale, bias, n_bins=n_bins)
                # the plain NLL of the labelled elements: one evaluation pass at the identity
                info0 = F.calib_fit(z, y, iters=0, smooth=False)[3]
                info1 = F.calib_fit(z_cal, y, iters=0, smooth=False)[3]
                extra = [bins0.reshape(-1), nan0, bins1.reshape(-1), nan1,
                         scale.view(torch.int32).to(torch.int64),
                         bias.view(torch.int32).to(torch.int64), status.to(torch.int64),
                         info0[:, 0].contiguous().view(torch.int64),
                         info1[:, 0].contiguous().view(torch.int64),
                         info0[:, 3].contiguous().view(torch.int64)]
            tp, fp = F.confusion_grid(z_sweep, ym, thr)
            packed = torch.cat([counts.reshape(-1), tp.reshape(-1), fp.reshape(-1),
                                ignored.reshape(-1).to(torch.int64)] + extra +
                               [loss.reshape(1).view(torch.int32).to(torch.int64)])
            host = packed.cpu().numpy()  # the one device-to-host copy
    finally:
        for m, was in flags:
            m.training = was

    C, T = z.shape[1], len(grid)
    k = host[:(C + 1) * 4].reshape(C + 1, 4).copy()
    tp_h = host[(C + 1) * 4:(C + 1) * 4 + C * T].reshape(C, T)
    fp_h = host[(C + 1) * 4 + C * T:(C + 1) * 4 + 2 * C * T].reshape(C, T)
    ign_h = host[(C + 1) * 4 + 2 * C * T:(C + 1) * 4 + 2 * C * T + C]
    k[:C, 3] -= ign_h            # what is left in n_nan is a NaN the model produced
    k[C, 3] -= ign_h.sum()
    val_loss = float(np.array([host[-1]], dtype=np.int64).astype(np.int32).view(np.float32)[0])
    per_class, macro, micro = auroc_from_counts(k)
    # labels per class from the sweep-independent pair counts (no NaN got past the line above)
    picked = pick_thresholds(tp_h, fp_h, k[:C, 1], grid)
    out = {"n": n, "val_loss": val_loss, "val_auroc_micro": micro, "val_auroc_macro": macro,
           "val_auroc_per_class": per_class, "thresholds": picked["thresholds"],
           "val_f1_micro": picked["micro"]["f1"],
           "val_f1_micro_at_0p5": picked["micro_at_0p5"]["f1"],
           "per_class": picked["per_class"]}
    if calibrate is not None:
        out["calibration"] = _calibration_report(
            host[(C + 1) * 4 + 2 * C * T + C:-1], C, n_bins, ign_h, cal_mode)
    if n_boot:
        if n * C > B.MAX_ITEMS:
            raise ValueError(f"evaluate(bootstrap=...): n * C = {n * C} exceeds 2^24")
        with torch.no_grad():
            # the chosen thresholds as the sweep compared them: the grid's own fp32 logits
            thr_c = torch.from_numpy(np.array([thr_host[grid.index(p)] for p in
                                               picked["thresholds"]], np.float32)).to(z.device)
            plan = F.bootstrap_plan(zm.contiguous(), ym.contiguous(), z_sweep >= thr_c)
            boot = torch.empty((n_boot, C + 1, 5), dtype=torch.int64, device=z.device)
            step = B.batch_size(n_boot, n)
            for r0 in range(0, n_boot, step):
                rb = min(step, n_boot - r0)
                w = F.bootstrap_weights(rb, n, bootstrap_seed, r0=r0, device=z.device)
                F.bootstrap_counts(plan, w, out=boot[r0:r0 + rb])
            boot_h = boot.cpu().numpy()  # the second (and last) device-to-host copy
        iv = B.intervals(boot_h, ci_level)
        out["boot"] = boot_h
        out["ci"] = {"level": ci_level, "n_replicates": n_boot, "seed": bootstrap_seed,
                     "val_auroc_micro": iv["auroc_micro"], "val_auroc_macro": iv["auroc_macro"],
                     "val_auroc_per_class": iv["auroc_per_class"],
                     "val_f1_micro": iv["f1_micro"],
                     "per_class": [{k: iv[f"{k}_per_class"][c] for k in
                                    ("sensitivity", "specificity", "f1")} for c in range(C)]}
    if generate and has_head:
        width = max(g.shape[1] for g in gen_ids)
        pred = [row + [0] * (width - len(row)) for g in gen_ids for row in g.tolist()]
        ref = report_labels.tolist() if torch.is_tensor(report_labels) else list(report_labels)
        if len(ref) != n:
            raise ValueError(f"evaluate: {len(ref)} report_labels rows for {n} validation rows")
        out["val_rougeL"] = rouge_l(pred, ref)
    return out
