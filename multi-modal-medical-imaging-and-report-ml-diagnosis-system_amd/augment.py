"""Training augmentation on the GPU: small random rotations, zooms, shifts, optional flips and
contrast / brightness changes of the normalised [B, C, H, W] batch `preprocess_batch` leaves on
the device, in one HIP launch (`mmdx_augment_affine`, functional.augment_affine).

Semantics (kernel, `reference` below and the tests agree on these):

  * a parameter row is (a00, a01, ox, a10, a11, oy, gain, delta), fp32;
  * with cx = (W-1)/2, cy = (H-1)/2, dx = j - cx, dy = i - cy, output pixel (i, j) samples
    sx = a00 dx + a01 dy + (cx + ox), sy = a10 dx + a11 dy + (cy + oy) in pixel-index
    coordinates: the bilinear blend of the taps (floor(sy) | +1, floor(sx) | +1), a tap outside
    the image reading fill_c = (0 - mean_c) / std_c (black) - torch's
    grid_sample(x - fill, padding_mode="zeros", align_corners=False) + fill on the grid
    ((2 sx + 1) / W - 1, (2 sy + 1) / H - 1);
  * the warp runs in normalised space with weights exactly 1 and 0 at integer positions, so the
    identity, a flip, a quarter turn and a whole-pixel shift return input bits;
  * then, in pixel terms, p' = clamp(gain (p - 0.5) + 0.5 + delta, 0, 1), computed as
    v' = gain v + ((gain - 1)(mean_c - 0.5) + delta) / std_c clamped to
    [(0 - mean_c) / std_c, (1 - mean_c) / std_c] (fp32, the values `preprocess_batch` writes for
    the pixel values 0 and 255, so the clamp is the identity on its output).

`Augment` draws the rows from its own numpy Generator.  Under data parallelism every rank
builds its own `Augment` with a different seed (for example `seed + rank`), or all ranks would
apply the same warps.
"""
from __future__ import annotations

import math

import numpy as np
import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)   # as csrc/preprocess.hip
IMAGENET_STD = (0.229, 0.224, 0.225)
MAX_A, MAX_O = 1e3, 1e6                 # check_params: |a| and |o| limits
MAX_C, MAX_HW, MAX_B = 4, 4096, 65535   # as csrc/augment.hip
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0)


def check_params(params, B=None) -> np.ndarray:
    """Host validation of parameter rows: [B, 8], every value finite, |a| <= 1e3, |o| <= 1e6;
    ValueError otherwise.  Returns them as a C-contiguous float32 array."""
    if isinstance(params, torch.Tensor):
        if params.device.type != "cpu":
            raise ValueError("augment parameters are validated on the host: pass a CPU tensor")
        params = params.detach().numpy()
    p = np.asarray(params)
    if p.ndim != 2 or p.shape[1] != 8 or p.shape[0] < 1 or (B is not None and p.shape[0] != B):
        raise ValueError(f"augment parameters must be [{'B' if B is None else B}, 8], got "
                         f"{tuple(p.shape)}")
    if p.dtype.kind not in "fiu":
        raise ValueError(f"augment parameters must be numeric, got {p.dtype}")
    p = np.ascontiguousarray(p, dtype=np.float32)
    if not np.isfinite(p).all():
        raise ValueError("augment parameters must be finite")
    if np.abs(p[:, [0, 1, 3, 4]]).max() > MAX_A:
        raise ValueError(f"augment matrix entries must be at most {MAX_A:g} in magnitude")
    if np.abs(p[:, [2, 5]]).max() > MAX_O:
        raise ValueError(f"augment offsets must be at most {MAX_O:g} in magnitude")
    return p


def norm_constants(C, mean=None, std=None):
    """(mean, std) as float32 arrays of C values; the defaults are preprocess.hip's ImageNet
    constants (C <= 3)."""
    if mean is None or std is None:
        if C > 3:
            raise ValueError(f"no default mean / std for C = {C}")
        mean = IMAGENET_MEAN[:C] if mean is None else mean
        std = IMAGENET_STD[:C] if std is None else std
    m = np.asarray(mean, dtype=np.float32).reshape(-1)
    s = np.asarray(std, dtype=np.float32).reshape(-1)
    if m.size != C or s.size != C:
        raise ValueError(f"mean and std need {C} values each, got {m.size} and {s.size}")
    if not (np.isfinite(m).all() and np.isfinite(s).all() and (s > 0).all()):
        raise ValueError("mean must be finite and std positive")
    return m, s


def clamp_bounds(mean, std):
    """(lo, hi) fp32: (0 - mean) / std and (1 - mean) / std in float32 arithmetic, as
    preprocess.hip normalises the pixel values 0 and 255.  lo is also the fill value."""
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    return (np.float32(0) - m) / s, (np.float32(1) - m) / s


def reference(x, params, mean=None, std=None, clamp=True, dtype=torch.float64):
    """The semantics of the module docstring in plain torch on the CPU, computed in `dtype`.
    x [B, C, H, W] (any device; taken to the CPU), params [B, 8].  Returns a CPU tensor."""
    x = x.detach().cpu().to(dtype)
    if x.dim() != 4:
        raise ValueError(f"reference takes [B, C, H, W], got {tuple(x.shape)}")
    B, C, H, W = x.shape
    p = torch.from_numpy(check_params(params, B)).to(dtype)
    m32, s32 = norm_constants(C, mean, std)
    lo32, hi32 = clamp_bounds(m32, s32)
    m, s = torch.from_numpy(m32).to(dtype), torch.from_numpy(s32).to(dtype)
    lo = torch.from_numpy(lo32).to(dtype).view(1, C, 1, 1)
    hi = torch.from_numpy(hi32).to(dtype).view(1, C, 1, 1)
    a00, a01, ox, a10, a11, oy, gain, delta = (p[:, k].view(B, 1, 1) for k in range(8))
    cx, cy = (W - 1) / 2, (H - 1) / 2
    dx = (torch.arange(W, dtype=dtype) - cx).view(1, 1, W)
    dy = (torch.arange(H, dtype=dtype) - cy).view(1, H, 1)
    sx = (a00 * dx + a01 * dy + (cx + ox)).clamp(-1.5, W + 0.5)
    sy = (a10 * dx + a11 * dy + (cy + oy)).clamp(-1.5, H + 0.5)
    fx, fy = sx.floor(), sy.floor()
    wx, wy = (sx - fx).unsqueeze(1), (sy - fy).unsqueeze(1)
    x0, y0 = fx.long(), fy.long()
    flat = x.reshape(B, C, H * W)
    fill = lo.expand(B, C, H, W)

    def tap(yy, xx):
        inside = ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).unsqueeze(1).expand(B, C, H, W)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(B, 1, H * W).expand(B, C, H * W)
        return torch.where(inside, flat.gather(2, idx).view(B, C, H, W), fill)

    top = tap(y0, x0) * (1 - wx) + tap(y0, x0 + 1) * wx
    bot = tap(y0 + 1, x0) * (1 - wx) + tap(y0 + 1, x0 + 1) * wx
    v = top * (1 - wy) + bot * wy
    g, d = gain.view(B, 1, 1, 1), delta.view(B, 1, 1, 1)
    v = g * v + ((g - 1) * (m.view(1, C, 1, 1) - 0.5) + d) / s.view(1, C, 1, 1)
    if clamp:
        v = torch.minimum(torch.maximum(v, lo), hi)
    return v


def affine_rows(theta, s, tx, ty, flip, gain, delta) -> np.ndarray:
    """Parameter rows [B, 8] (fp64) of the forward map q = s R(theta) F (p - c) + c + (tx, ty),
    R = [[cos, -sin], [sin, cos]], F = diag(flip, 1) with flip = +-1, theta in radians: the row
    holds the inverse the kernel samples with, A = F^-1 R^-1 / s and o = -A t."""
    theta, s, tx, ty, flip, gain, delta = np.broadcast_arrays(
        *(np.asarray(v, dtype=np.float64) for v in (theta, s, tx, ty, flip, gain, delta)))
    cos, sin = np.cos(theta), np.sin(theta)
    a00, a01, a10, a11 = flip * cos / s, flip * sin / s, -sin / s, cos / s
    ox, oy = -(a00 * tx + a01 * ty), -(a10 * tx + a11 * ty)
    return np.stack([a00, a01, ox, a10, a11, oy, gain, delta], axis=-1) + 0.0  # no -0.0


class Augment:
    """Random affine + photometric augmentation of a normalised GPU batch.

    rotate: degrees, theta ~ U(-rotate, rotate); scale: (lo, hi), s ~ U(lo, hi); translate:
    fraction of the side, t ~ U(-translate, translate) * (W, H); hflip: probability of a
    horizontal flip (0 by default: laterality matters in a radiograph); contrast:
    gain ~ 1 + U(-contrast, contrast); brightness: delta ~ U(-brightness, brightness), in pixel
    units of [0, 1].  The forward map from source to output is q = s R(theta) F (p - c) + c + t
    with R = [[cos, -sin], [sin, cos]] and F = diag(+-1, 1); a row stores its inverse,
    A = F^-1 R^-1 / s and o = -A t.  All magnitudes 0 give identity rows.  The object owns its
    numpy Generator (`seed`): the same seed gives the same rows in the same order."""

    def __init__(self, rotate=10.0, scale=(0.9, 1.1), translate=0.05, hflip=0.0, contrast=0.2,
                 brightness=0.1, seed=0):
        lo, hi = (float(v) for v in scale)
        if not (0.0 < lo <= hi):
            raise ValueError(f"scale must be 0 < lo <= hi, got {scale}")
        if not (0.0 <= hflip <= 1.0):
            raise ValueError(f"hflip is a probability, got {hflip}")
        for name, v in (("rotate", rotate), ("translate", translate), ("contrast", contrast),
                        ("brightness", brightness)):
            if not (v >= 0.0 and math.isfinite(v)):
                raise ValueError(f"{name} must be a finite magnitude >= 0, got {v}")
        self.rotate, self.scale, self.translate = float(rotate), (lo, hi), float(translate)
        self.hflip, self.contrast, self.brightness = float(hflip), float(contrast), \
            float(brightness)
        self.seed = seed
        self.rng = np.random.default_rng(seed)

    def draw(self, B, H, W) -> np.ndarray:
        """[B, 8] fp32 parameter rows for B images of H x W, from the object's Generator."""
        r = self.rng
        theta = np.deg2rad(r.uniform(-self.rotate, self.rotate, B))
        s = r.uniform(self.scale[0], self.scale[1], B)
        tx = r.uniform(-self.translate, self.translate, B) * W
        ty = r.uniform(-self.translate, self.translate, B) * H
        f = np.where(r.random(B) < self.hflip, -1.0, 1.0)
        gain = 1.0 + r.uniform(-self.contrast, self.contrast, B)
        delta = r.uniform(-self.brightness, self.brightness, B)
        return affine_rows(theta, s, tx, ty, f, gain, delta).astype(np.float32)

    def __call__(self, x, mean=None, std=None, clamp=True):
        from .functional import augment_affine
        B, _, H, W = x.shape
        return augment_affine(x, self.draw(B, H, W), mean=mean, std=std, clamp=clamp)
