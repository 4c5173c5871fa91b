"""Contrast-limited adaptive histogram equalisation (CLAHE) of 8-bit radiographs: the
definition, its numpy statement and the descriptor table of the GPU passes
(csrc/clahe.hip: `mmdx_clahe_luts`, `mmdx_clahe_apply`; functional.clahe;
preprocess_batch(clahe=...)).

The algorithm is the one of OpenCV's CLAHE_Impl for 8-bit images
(`cv2.createCLAHE(clip_limit, tiles).apply(img)`), restated so that every step is integer
arithmetic or ONE correctly-rounded fp32 operation; `reference` below is the definition, and
the kernels equal it byte for byte.  For one uint8 plane [H, W], `clip_limit` and
`tiles = (tx, ty)` (columns, rows of tiles):

  1. Extension.  If W % tx == 0 and H % ty == 0 the plane is used as it is.  Otherwise it is
     extended on the right by tx - W % tx columns AND at the bottom by ty - H % ty rows with
     reflect-101 (np.pad(mode="reflect")): an axis that was already divisible gets a whole
     extra tx or ty, as in OpenCV.  tw = W_ext / tx, th = H_ext / ty, area = tw * th.
  2. Per-tile constants (host, Python): clip = 0 when clip_limit <= 0 (no clipping), else
     max(int(clip_limit * area / 256), 1) in double arithmetic, truncated;
     lut_scale = float32(255) / float32(area).
  3. Per-tile LUT.  h = the 256-bin histogram of the extended tile.  With clip > 0:
     clipped = sum(max(h - clip, 0)), h = min(h, clip), batch = clipped // 256,
     res = clipped - 256 * batch; every bin gains batch; with res > 0 and
     step = max(256 // res, 1), bin i gains 1 more iff i % step == 0 and i // step < res (the
     closed form of OpenCV's serial loop).  sum(h) == area.
     lut[i] = clamp(rint(float32(cumsum(h)[i]) * lut_scale), 0, 255): one fp32 multiply,
     rounding half to even; the int -> float conversion is exact because area <= 2^24.
  4. Interpolation over the original H x W pixels.  Per column x: inv = float32(1) /
     float32(tw), f = float32(x) * inv - 0.5f, x1 = floor(f), xa = f - float32(x1),
     xa1 = 1.0f - xa, tile columns max(x1, 0) and min(x1 + 1, tx - 1); rows alike with th, ty,
     ya, ya1.  With v the source pixel and L.. the four tiles' lut[v] as fp32,
     r = (L11 * xa1 + L12 * xa) * ya1 + (L21 * xa1 + L22 * xa) * ya, every * and + its own
     correctly-rounded fp32 operation (no fused multiply-add); the output is
     clamp(rint(r), 0, 255).

A three-channel image is three independent planes: a grey radiograph stored as RGB comes out
with three equal channels, identical to the grey treatment.  That is not a colour-faithful
method (no LAB conversion).  Equality with cv2 itself is not checked anywhere (cv2 is not a
dependency): `reference` is the definition.

Limits (ValueError / TypeError before any launch): uint8 only, C in {1, 3},
1 <= tx, ty <= 16, W >= 2 tx and H >= 2 ty (the reflection stays inside the image),
tile area <= 2^24, H, W <= 65535, clip_limit finite.

CLAHE is part of a model's input definition, not an augmentation: a model trained on
equalised pixels must be served equalised pixels.  `Clahe.config()` is the JSON-safe dict
that travels in a bundle's artifacts["clahe"]; inference() rebuilds the `Clahe` from it.
"""
from __future__ import annotations

import math

import numpy as np

MAX_TILES = 16           # per axis, as csrc/clahe.hip
MAX_AREA = 1 << 24       # float32(count) stays exact
MAX_SIDE = 65535

# mirrors mmdx_clahe_desc (include/mmdx.h)
DESC = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("lut_off", "<i8"),
                 ("w", "<i4"), ("h", "<i4"), ("c", "<i4"), ("tiles_x", "<i4"),
                 ("tiles_y", "<i4"), ("tile_w", "<i4"), ("tile_h", "<i4"), ("clip", "<i4"),
                 ("lut_scale", "<f4")], align=True)
assert DESC.itemsize == 64


def check_params(clip_limit, tiles):
    """(clip_limit as float, (tx, ty) as ints) after validation: TypeError for a wrong type,
    ValueError for a value outside the limits."""
    if isinstance(clip_limit, bool) or not isinstance(clip_limit, (int, float, np.integer,
                                                                   np.floating)):
        raise TypeError(f"clip_limit must be a number, got {type(clip_limit).__name__}")
    clip_limit = float(clip_limit)
    if not math.isfinite(clip_limit):
        raise ValueError(f"clip_limit must be finite, got {clip_limit}")
    try:
        tx, ty = tiles
    except (TypeError, ValueError):
        raise TypeError(f"tiles must be a pair (columns, rows), got {tiles!r}") from None
    for v in (tx, ty):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"tiles must be integers, got {tiles!r}")
    tx, ty = int(tx), int(ty)
    if not (1 <= tx <= MAX_TILES and 1 <= ty <= MAX_TILES):
        raise ValueError(f"tiles must be in [1, {MAX_TILES}] per axis, got {(tx, ty)}")
    return clip_limit, (tx, ty)


def geometry(h, w, clip_limit, tiles):
    """(tile_w, tile_h, clip, lut_scale) of an H x W plane (steps 1 and 2 of the definition),
    after checking the image limits."""
    tx, ty = tiles
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"image {h} x {w}: sides must be in [1, {MAX_SIDE}]")
    if w < 2 * tx or h < 2 * ty:
        raise ValueError(f"image {h} x {w} is too small for {tx} x {ty} tiles: CLAHE needs "
                         "W >= 2 tx and H >= 2 ty (the reflected border stays inside the image)")
    if w % tx == 0 and h % ty == 0:
        w_ext, h_ext = w, h
    else:
        w_ext, h_ext = w + (tx - w % tx), h + (ty - h % ty)
    tw, th = w_ext // tx, h_ext // ty
    area = tw * th
    if area > MAX_AREA:
        raise ValueError(f"tile area {tw} x {th} exceeds 2^24 pixels")
    if clip_limit > 0:
        c = clip_limit * area / 256
        # no bin exceeds area, so a clip of area or more clips nothing: capping it there keeps
        # the value an int32 for any finite clip_limit without changing a result
        clip = area if c >= area else max(int(c), 1)
    else:
        clip = 0
    return tw, th, clip, np.float32(255) / np.float32(area)


def as_planes(img):
    """uint8 HxW / HxWx{1,3} array or PIL L / RGB image -> contiguous (H, W, C) array."""
    if hasattr(img, "mode") and hasattr(img, "size"):
        if img.mode not in ("L", "RGB"):
            raise ValueError(f"image mode {img.mode!r}: CLAHE takes L or RGB images")
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise TypeError(f"CLAHE takes uint8 pixels, got {a.dtype}")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3):
        raise ValueError(f"expected HxW or HxWx{{1,3}} pixels, got {a.shape}")
    return np.ascontiguousarray(a)


def tile_histograms(plane, tiles, tw, th):
    """[ty, tx, 256] int64 histograms of the extended plane's tiles (step 1 + the count)."""
    tx, ty = tiles
    h, w = plane.shape
    ext = np.pad(plane, ((0, th * ty - h), (0, tw * tx - w)), mode="reflect")
    t = ext.reshape(ty, th, tx, tw).transpose(0, 2, 1, 3).reshape(ty * tx, th * tw)
    idx = t.astype(np.int64) + 256 * np.arange(ty * tx, dtype=np.int64)[:, None]
    return np.bincount(idx.ravel(), minlength=256 * ty * tx).reshape(ty, tx, 256)


def redistribute(hist, clip):
    """Step 3's clipping and redistribution of [..., 256] histograms (int64); clip = 0: none."""
    h = np.asarray(hist, dtype=np.int64)
    if clip <= 0:
        return h.copy()
    clipped = np.maximum(h - clip, 0).sum(-1, keepdims=True)
    batch = clipped // 256
    res = clipped - 256 * batch
    step = np.maximum(256 // np.maximum(res, 1), 1)
    i = np.arange(256, dtype=np.int64)
    extra = (res > 0) & (i % step == 0) & (i // step < res)
    return np.minimum(h, clip) + batch + extra


def luts_from_histograms(hist, lut_scale):
    """lut = clamp(rint(float32(cumsum) * lut_scale), 0, 255) as uint8 (one fp32 multiply)."""
    cdf = np.cumsum(hist, axis=-1).astype(np.float32)
    return np.clip(np.rint(cdf * np.float32(lut_scale)), 0, 255).astype(np.uint8)


def _axis(n, t, nt):
    """Step 4's per-coordinate (first tile, second tile, a, 1 - a), fp32 operation by operation."""
    inv = np.float32(1) / np.float32(t)
    f = np.arange(n, dtype=np.float32) * inv - np.float32(0.5)
    i1 = np.floor(f)
    a = f - i1
    a1 = np.float32(1) - a
    i1 = i1.astype(np.int64)
    return np.maximum(i1, 0), np.minimum(i1 + 1, nt - 1), a, a1


def interpolate(plane, luts, tw, th):
    """Step 4 for one plane and its [ty, tx, 256] LUTs."""
    ty, tx = luts.shape[:2]
    h, w = plane.shape
    x1, x2, xa, xa1 = _axis(w, tw, tx)
    y1, y2, ya, ya1 = _axis(h, th, ty)
    lf = luts.astype(np.float32)
    v = plane.astype(np.int64)
    y1c, y2c = y1[:, None], y2[:, None]
    x1r, x2r = x1[None, :], x2[None, :]
    xa, xa1 = xa[None, :], xa1[None, :]
    ya, ya1 = ya[:, None], ya1[:, None]
    top = lf[y1c, x1r, v] * xa1 + lf[y1c, x2r, v] * xa
    bot = lf[y2c, x1r, v] * xa1 + lf[y2c, x2r, v] * xa
    r = top * ya1 + bot * ya
    assert r.dtype == np.float32
    return np.clip(np.rint(r), 0, 255).astype(np.uint8)


def reference(img, clip_limit=2.0, tiles=(8, 8), return_luts=False):
    """The definition in numpy.  img: uint8 HxW or HxWx{1,3} (array or PIL L / RGB); returns an
    array of the same shape, and with return_luts the uint8 LUTs [ty, tx, 256] (HxW input) or
    [C, ty, tx, 256]."""
    clip_limit, tiles = check_params(clip_limit, tiles)
    flat = np.asarray(img).ndim == 2
    a = as_planes(img)
    h, w, c = a.shape
    tw, th, clip, lut_scale = geometry(h, w, clip_limit, tiles)
    out = np.empty_like(a)
    luts = np.empty((c, tiles[1], tiles[0], 256), dtype=np.uint8)
    for ch in range(c):
        hist = redistribute(tile_histograms(a[:, :, ch], tiles, tw, th), clip)
        luts[ch] = luts_from_histograms(hist, lut_scale)
        out[:, :, ch] = interpolate(a[:, :, ch], luts[ch], tw, th)
    if flat:
        out, luts = out[:, :, 0], luts[0]
    return (out, luts) if return_luts else out


class Clahe:
    """The CLAHE setting of a model's input: clip_limit and tiles = (columns, rows).  Hand it
    to preprocess_batch / LocalCXRBatches / training_tests; `config()` is what a bundle stores
    under artifacts["clahe"] and `from_config` what inference() rebuilds it with."""

    def __init__(self, clip_limit=2.0, tiles=(8, 8)):
        self.clip_limit, self.tiles = clip_limit, tiles
        self.check()

    def check(self):
        """Validate (and normalise) the setting: TypeError / ValueError as check_params."""
        self.clip_limit, self.tiles = check_params(self.clip_limit, self.tiles)
        return self

    def config(self) -> dict:
        self.check()
        return {"clip_limit": self.clip_limit, "tiles": [self.tiles[0], self.tiles[1]]}

    @classmethod
    def from_config(cls, cfg):
        if isinstance(cfg, Clahe):
            return cfg.check()
        if not isinstance(cfg, dict):
            raise TypeError(f"a CLAHE config is a dict, got {type(cfg).__name__}")
        miss = [k for k in ("clip_limit", "tiles") if k not in cfg]
        if miss:
            raise ValueError(f"CLAHE config lacks {miss}")
        tiles = cfg["tiles"]
        return cls(cfg["clip_limit"], tuple(tiles) if isinstance(tiles, list) else tiles)

    def __call__(self, img):
        """`reference` with this setting (the host path: inference() on a CPU device)."""
        return reference(img, self.clip_limit, self.tiles)

    def __eq__(self, other):
        return isinstance(other, Clahe) and self.config() == other.config()

    def __hash__(self):
        return hash((self.clip_limit, self.tiles))

    def __repr__(self):
        return f"Clahe(clip_limit={self.clip_limit}, tiles={self.tiles})"


def plan(arrays, clahe):
    """Descriptor table of the two GPU passes for a list of (H, W, C) uint8 arrays packed back
    to back: (descs [B] of DESC, pixel bytes, LUT bytes).  Source and destination share the
    packed layout (dst_off == src_off); an image's LUTs are [c][tiles_y][tiles_x][256] bytes at
    lut_off.  Raises the documented errors before anything is uploaded."""
    if not isinstance(clahe, Clahe):
        raise TypeError(f"clahe must be an mmdx.Clahe, got {type(clahe).__name__}")
    clahe.check()
    tx, ty = clahe.tiles
    if not len(arrays):
        raise ValueError("empty batch")
    descs = np.zeros(len(arrays), dtype=DESC)
    off = lut_off = 0
    for b, a in enumerate(arrays):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
            raise TypeError("CLAHE takes uint8 arrays")
        if a.ndim != 3 or a.shape[2] not in (1, 3):
            raise ValueError(f"expected (H, W, {{1,3}}) pixels, got {a.shape}")
        h, w, c = a.shape
        tw, th, clip, lut_scale = geometry(h, w, clahe.clip_limit, clahe.tiles)
        d = descs[b]
        d["src_off"] = d["dst_off"] = off
        d["lut_off"] = lut_off
        d["w"], d["h"], d["c"] = w, h, c
        d["tiles_x"], d["tiles_y"], d["tile_w"], d["tile_h"] = tx, ty, tw, th
        d["clip"], d["lut_scale"] = clip, lut_scale
        off += h * w * c
        lut_off += c * ty * tx * 256
    return descs, off, lut_off
