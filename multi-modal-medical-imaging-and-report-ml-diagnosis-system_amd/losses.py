"""Disease loss for imbalanced, partly labelled chest-X-ray targets.

One criterion covers `pos_weight`, class weights, ignored labels, label smoothing and focal
modulation; on the GPU it is one fused HIP kernel (csrc/loss.hip, functional.disease_loss).  This
module holds the definition and everything that needs no device:

- `reference`: the CPU statement of the loss in plain torch (run it in float64), the yardstick of
  the tests, as mmdx.augment.reference is for the warp;
- `reference_grad`: the closed-form element gradient the kernel computes;
- `check_loss_args`: the argument checks, made on the host before any launch;
- `DiseaseLoss`: the criterion object of the training loops and of metrics.evaluate().

Definition.  logits z [B, C]; targets y [B, C] where NaN means "no label: ignore" (mask m = 0)
and any other value is a (possibly soft) label in [0, 1]; pos_weight pw [C] and class_weight
cw [C] default to 1; gamma is 0 or >= 1; label_smoothing eps is in [0, 1).  Per element

    y' = y (1 - eps) + eps / 2                              (0 where ignored)
    p  = sigmoid(z)
    bce = pw_c y' softplus(-z) + (1 - y') softplus(z)
    e   = m cw_c |y' - p|^gamma bce                         (gamma = 0: the factor is exactly 1)

"mean" is sum e / max(sum m, 1), the mean over LABELLED elements (an all-ignored batch gives
loss 0 and gradient 0, never NaN); "sum" is sum e.  stats [C, 2] holds sum_b e and sum_b m per
class.  With gamma = 0 this is binary_cross_entropy_with_logits(weight = cw m, pos_weight = pw);
with hard labels, cw = 1 - alpha and pw = alpha / (1 - alpha) it is the sigmoid focal loss
alpha_t (1 - p_t)^gamma CE.  For 0 < gamma < 1 the gradient is unbounded at p = y', so that
range is rejected.

Data parallelism: the "mean" normaliser is per rank.  Ranks whose batches hold different numbers
of labelled elements are averaged as ranks by the gradient all-reduce, not as one pooled batch; a
global label count is not exchanged.
"""
from __future__ import annotations

import math

import numpy as np
import torch

__all__ = ["MAX_CLASSES", "reference", "reference_grad", "check_loss_args", "DiseaseLoss"]

MAX_CLASSES = 64  # as the metrics kernels
_REDUCTIONS = ("mean", "sum")


def _terms(z, y, pos_weight, class_weight, gamma, label_smoothing):
    """m, y', p, bce, cw of the definition, in z's dtype."""
    dt = z.dtype
    m = ~torch.isnan(y)
    ys = torch.where(m, y, torch.zeros_like(y)).to(dt)
    ys = torch.where(m, ys * (1.0 - label_smoothing) + 0.5 * label_smoothing,
                     torch.zeros_like(ys))
    C = z.shape[1]
    pw = torch.ones(C, dtype=dt) if pos_weight is None else torch.as_tensor(pos_weight).to(dt)
    cw = torch.ones(C, dtype=dt) if class_weight is None else torch.as_tensor(class_weight).to(dt)
    l1p = torch.log1p(torch.exp(-z.abs()))  # softplus(x) = max(x, 0) + log1p(exp(-|x|))
    bce = pw * ys * ((-z).clamp(min=0.0) + l1p) + (1.0 - ys) * (z.clamp(min=0.0) + l1p)
    return m, ys, torch.sigmoid(z), bce, pw, cw


def reference(z, y, pos_weight=None, class_weight=None, gamma=0.0, label_smoothing=0.0,
              reduction="mean"):
    """(loss, stats [C, 2]) of the module docstring in plain torch, in z's dtype (pass float64
    logits for the yardstick; y keeps its NaNs).  Differentiable in z."""
    check_loss_args(gamma, label_smoothing, reduction)
    m, ys, p, bce, pw, cw = _terms(z, y, pos_weight, class_weight, gamma, label_smoothing)
    e = cw * bce
    if gamma != 0.0:
        e = (ys - p).abs() ** gamma * e
    e = torch.where(m, e, torch.zeros_like(e))
    mf = m.to(z.dtype)
    stats = torch.stack([e.sum(0), mf.sum(0)], dim=1)
    total = e.sum()
    if reduction == "mean":
        total = total / mf.sum().clamp(min=1.0)
    return total, stats


def reference_grad(z, y, pos_weight=None, class_weight=None, gamma=0.0, label_smoothing=0.0):
    """The closed-form UN-normalised element gradient de/dz (what the kernel stores):
    d = p - y';  cw m [gamma |d|^(gamma-1) sign(d) p (1-p) bce
                       + |d|^gamma ((1 - y') p - pw y' (1 - p))]."""
    check_loss_args(gamma, label_smoothing, "sum")
    m, ys, p, bce, pw, cw = _terms(z, y, pos_weight, class_weight, gamma, label_smoothing)
    dbce = (1.0 - ys) * p - pw * ys * (1.0 - p)
    if gamma == 0.0:
        g = cw * dbce
    else:
        d = p - ys
        g = cw * (gamma * d.abs() ** (gamma - 1.0) * torch.sign(d) * p * (1.0 - p) * bce
                  + d.abs() ** gamma * dbce)
    return torch.where(m, g, torch.zeros_like(g))


def _check_weight_values(name, w):
    a = np.asarray(w, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"{name} must be a 1-D vector of per-class weights, got shape {a.shape}")
    if not np.all(np.isfinite(a)) or np.any(a < 0.0):
        raise ValueError(f"{name} must be finite and >= 0, got {a.tolist()}")


def check_loss_args(gamma, label_smoothing, reduction):
    """The scalar settings of the loss; ValueError on the host, before any launch."""
    g = float(gamma)
    if not (g == 0.0 or (g >= 1.0 and math.isfinite(g))):
        raise ValueError(f"gamma must be 0 or >= 1 (the focal gradient is unbounded at p = y' "
                         f"for 0 < gamma < 1), got {gamma}")
    e = float(label_smoothing)
    if not (0.0 <= e < 1.0):
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
    if reduction not in _REDUCTIONS:
        raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
    return g, e


def check_weight(name, w, C=None):
    """A per-class weight tensor as functional.disease_loss takes it: fp32, 1-D, C long.  A host
    tensor also has its values checked (finite, >= 0); a device tensor is trusted, since looking
    at it would sync - DiseaseLoss checks its weights on the host before it moves them."""
    if w is None:
        return
    if not torch.is_tensor(w):
        raise TypeError(f"{name} must be a float32 tensor, got {type(w).__name__}")
    if w.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {w.dtype}")
    if w.dim() != 1 or (C is not None and w.shape[0] != C):
        raise ValueError(f"{name} must have shape [{C}], got {tuple(w.shape)}")
    if not w.is_cuda:
        _check_weight_values(name, w.detach().numpy())


class DiseaseLoss:
    """The disease-head criterion: `crit(logits, target)` returns the scalar loss of the module
    docstring, computed by functional.disease_loss (one HIP launch, no host sync; the backward
    takes a device-scalar upstream gradient, so GradScaler.scale(loss).backward() works).

    pos_weight / class_weight: None or C host values (list, numpy array or CPU tensor; see
    mmdx.data.pos_weight_from_stats), checked here and moved to the logits' device once.
    logits may be fp32, bf16 or fp16; targets are fp32 with NaN = ignore.  After a call,
    `stats` is that call's [C, 2] device tensor (per-class loss sum and labelled count; never
    synced here).  With every default it computes what mmdx.BCEWithLogitsLoss() computes."""

    def __init__(self, pos_weight=None, class_weight=None, gamma=0.0, label_smoothing=0.0,
                 reduction="mean"):
        self.gamma, self.label_smoothing = check_loss_args(gamma, label_smoothing, reduction)
        self.reduction = reduction
        self.pos_weight = self._host_weight("pos_weight", pos_weight)
        self.class_weight = self._host_weight("class_weight", class_weight)
        if (self.pos_weight is not None and self.class_weight is not None
                and self.pos_weight.shape != self.class_weight.shape):
            raise ValueError(f"pos_weight has {self.pos_weight.shape[0]} classes, class_weight "
                             f"{self.class_weight.shape[0]}")
        self.stats = None
        self._on_device = {}

    @staticmethod
    def _host_weight(name, w):
        if w is None:
            return None
        if torch.is_tensor(w):
            if w.is_cuda:
                raise ValueError(f"{name}: pass host values; DiseaseLoss checks them and moves "
                                 "them to the logits' device itself")
            w = w.detach().numpy()
        _check_weight_values(name, w)
        a = np.asarray(w, dtype=np.float32)
        if a.shape[0] < 1 or a.shape[0] > MAX_CLASSES:
            raise ValueError(f"{name} has {a.shape[0]} classes; 1 to {MAX_CLASSES} are supported")
        return torch.from_numpy(a.copy())

    def _weights_on(self, device):
        key = (device.type, device.index)
        got = self._on_device.get(key)
        if got is None:
            got = tuple(None if w is None else w.to(device)
                        for w in (self.pos_weight, self.class_weight))
            self._on_device[key] = got
        return got

    def config(self):
        """The settings as a plain (JSON-safe) dict, stored with a saved bundle."""
        def lst(w):
            return None if w is None else [float(v) for v in w.tolist()]
        return {"name": "DiseaseLoss", "pos_weight": lst(self.pos_weight),
                "class_weight": lst(self.class_weight), "gamma": self.gamma,
                "label_smoothing": self.label_smoothing, "reduction": self.reduction}

    def __call__(self, logits, target):
        from . import functional as F
        for name, w in (("pos_weight", self.pos_weight), ("class_weight", self.class_weight)):
            if w is not None and logits.dim() == 2 and w.shape[0] != logits.shape[1]:
                raise ValueError(f"{name} has {w.shape[0]} classes, the logits have "
                                 f"{logits.shape[1]}")
        pw, cw = self._weights_on(logits.device)
        loss, self.stats = F.disease_loss(logits, target, pos_weight=pw, class_weight=cw,
                                          gamma=self.gamma,
                                          label_smoothing=self.label_smoothing,
                                          reduction=self.reduction)
        return loss
