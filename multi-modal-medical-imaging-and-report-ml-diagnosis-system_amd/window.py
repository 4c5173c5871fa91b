"""Grey-level windowing of 16-bit radiographs to 8 bits: the definition, its numpy statement
and the descriptor table of the GPU passes (csrc/window.hip: `mmdx_window_levels`,
`mmdx_window_apply`; functional.window16; preprocess_batch(window=...)).

Detectors deliver 12 to 16 bits per pixel (DICOM pixel data, 16-bit PNGs); everything
downstream here (CLAHE, the transform, the towers) takes 8.  Which window of grey levels is
mapped to those 8 bits is part of a model's input definition, exactly as CLAHE is.  For one
uint16 plane [H, W] with n = H * W pixels and a `Window`:

  1. The window (lo, hi).
     percentile mode (0 <= low < high <= 100): k_lo = min(n - 1, floor(low * n / 100)),
     k_hi = min(n - 1, floor(high * n / 100)) in Python arithmetic (`ranks`, the one place
     they are computed); lo is the k_lo-th and hi the k_hi-th order statistic (0-based) of the
     plane's pixels; a flat image (hi == lo) gets hi = lo + 1.  low = 0, high = 100 is min-max.
     fixed mode: lo and hi are given, multiples of 0.5 with -65536 <= lo < hi <= 131072, so
     float32(v) - lo and hi - lo are exact.  `Window.from_center_width(c, w)` (integer c,
     integer w >= 2) is DICOM's linear VOI function: lo = c - 0.5 - (w - 1) / 2,
     hi = lo + (w - 1).
  2. The mapping.  scale = float32(255) / float32(hi - lo), one correctly-rounded fp32
     division; y = clamp(rint((float32(v) - float32(lo)) * scale), 0, 255): one exact
     subtraction, one multiply, rounding half to even.  invert (MONOCHROME1) gives 255 - y.

`reference` below is the definition and the kernels equal it byte for byte.

Limits (TypeError / ValueError before any launch): uint16 only, one channel (HxW or HxWx1,
PIL mode I;16), 1 <= H, W <= 65535, H * W <= 2^30, percentiles and lo / hi finite and in
range, mode one of "percentile" / "fixed".

`Window.config()` is the JSON-safe dict that travels in a bundle's artifacts["window"];
inference() rebuilds the `Window` from it.
"""
from __future__ import annotations

import math

import numpy as np

MAX_SIDE = 65535
MAX_PIXELS = 1 << 30
FIXED_MIN, FIXED_MAX = -65536.0, 131072.0
MODES = ("percentile", "fixed")

# mirrors mmdx_window_desc (include/mmdx.h)
DESC = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("w", "<i4"), ("h", "<i4"),
                 ("mode", "<i4"), ("invert", "<i4"), ("k_lo", "<i4"), ("k_hi", "<i4"),
                 ("lo", "<f4"), ("hi", "<f4"), ("scale", "<f4")], align=True)
assert DESC.itemsize == 56


def _number(v, what):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise TypeError(f"{what} must be a number, got {type(v).__name__}")
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{what} must be finite, got {v}")
    return v


def ranks(n, low, high):
    """(k_lo, k_hi), the 0-based ranks of the two order statistics of an n-pixel plane."""
    n = int(n)
    if n < 1:
        raise ValueError(f"ranks: n = {n} pixels")
    return (min(n - 1, int(math.floor(low * n / 100))),
            min(n - 1, int(math.floor(high * n / 100))))


def check_shape(h, w):
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"image {h} x {w}: sides must be in [1, {MAX_SIDE}]")
    if h * w > MAX_PIXELS:
        raise ValueError(f"image {h} x {w} exceeds 2^30 pixels")


def as_plane(img):
    """uint16 HxW / HxWx1 array or PIL I;16 image -> contiguous (H, W) uint16 array."""
    if hasattr(img, "mode") and hasattr(img, "size"):
        if img.mode != "I;16":
            raise TypeError(f"image mode {img.mode!r}: windowing takes 16-bit images "
                            "(PIL mode I;16)")
    a = np.asarray(img)
    if a.dtype != np.uint16:
        raise TypeError(f"windowing takes uint16 pixels, got {a.dtype}")
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if a.ndim != 2:
        raise ValueError(f"expected HxW or HxWx1 pixels (one channel), got {a.shape}")
    check_shape(*a.shape)
    return np.ascontiguousarray(a)


class Window:
    """The grey-level window of a model's 16-bit input.  Hand it to preprocess_batch /
    LocalCXRBatches / training_tests; `config()` is what a bundle stores under
    artifacts["window"] and `from_config` what inference() rebuilds it with."""

    def __init__(self, mode="percentile", low=0.5, high=99.5, lo=None, hi=None, invert=False):
        self.mode, self.low, self.high = mode, low, high
        self.lo, self.hi, self.invert = lo, hi, invert
        self.check()

    @classmethod
    def from_center_width(cls, center, width, invert=False):
        """DICOM's linear VOI function for WindowCenter c, WindowWidth w (integers, w >= 2)."""
        for v, what in ((center, "center"), (width, "width")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{what} must be an integer, got {type(v).__name__}")
        c, w = int(center), int(width)
        if w < 2:
            raise ValueError(f"width must be >= 2, got {w}")
        lo = c - 0.5 - (w - 1) / 2
        return cls("fixed", lo=lo, hi=lo + (w - 1), invert=invert)

    def check(self):
        """Validate (and normalise) the setting: TypeError for a wrong type, ValueError for a
        value outside the limits."""
        if not isinstance(self.mode, str):
            raise TypeError(f"mode must be a string, got {type(self.mode).__name__}")
        if self.mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {self.mode!r}")
        if not isinstance(self.invert, (bool, np.bool_)):
            raise TypeError(f"invert must be a bool, got {type(self.invert).__name__}")
        self.invert = bool(self.invert)
        if self.mode == "percentile":
            self.low, self.high = _number(self.low, "low"), _number(self.high, "high")
            if not (0 <= self.low < self.high <= 100):
                raise ValueError(f"percentiles need 0 <= low < high <= 100, got "
                                 f"{(self.low, self.high)}")
            if self.lo is not None or self.hi is not None:
                raise ValueError("lo / hi belong to mode 'fixed'")
        else:
            if self.lo is None or self.hi is None:
                raise ValueError("mode 'fixed' needs lo and hi")
            self.lo, self.hi = _number(self.lo, "lo"), _number(self.hi, "hi")
            if not (FIXED_MIN <= self.lo < self.hi <= FIXED_MAX):
                raise ValueError(f"fixed window needs {FIXED_MIN:g} <= lo < hi <= "
                                 f"{FIXED_MAX:g}, got {(self.lo, self.hi)}")
            if (2 * self.lo) % 1 or (2 * self.hi) % 1:
                raise ValueError(f"lo and hi must be multiples of 0.5, got "
                                 f"{(self.lo, self.hi)}")
        return self

    def config(self) -> dict:
        self.check()
        if self.mode == "percentile":
            return {"mode": "percentile", "low": self.low, "high": self.high,
                    "invert": self.invert}
        return {"mode": "fixed", "lo": self.lo, "hi": self.hi, "invert": self.invert}

    @classmethod
    def from_config(cls, cfg):
        if isinstance(cfg, Window):
            return cfg.check()
        if not isinstance(cfg, dict):
            raise TypeError(f"a window config is a dict, got {type(cfg).__name__}")
        if "mode" not in cfg:
            raise ValueError("window config lacks ['mode']")
        keys = ("lo", "hi") if cfg["mode"] == "fixed" else ("low", "high")
        miss = [k for k in keys if k not in cfg]
        if miss:
            raise ValueError(f"window config lacks {miss}")
        return cls(cfg["mode"], invert=cfg.get("invert", False), **{k: cfg[k] for k in keys})

    def levels(self, plane):
        """(lo, hi) of step 1 for one (H, W) uint16 plane: ints in percentile mode, the given
        floats in fixed mode."""
        if self.mode == "fixed":
            return self.lo, self.hi
        k_lo, k_hi = ranks(plane.size, self.low, self.high)
        part = np.partition(plane.reshape(-1), sorted({k_lo, k_hi}))
        lo, hi = int(part[k_lo]), int(part[k_hi])
        return lo, (lo + 1 if hi == lo else hi)

    def __call__(self, img):
        """`reference` with this setting (the host path: inference() on a CPU device)."""
        return reference(img, self)

    def __eq__(self, other):
        return isinstance(other, Window) and self.config() == other.config()

    def __hash__(self):
        return hash(tuple(sorted(self.config().items())))

    def __repr__(self):
        if self.mode == "percentile":
            return f"Window(mode='percentile', low={self.low}, high={self.high}, " \
                   f"invert={self.invert})"
        return f"Window(mode='fixed', lo={self.lo}, hi={self.hi}, invert={self.invert})"


def scale_of(lo, hi):
    """float32(255) / float32(hi - lo): one correctly-rounded fp32 division."""
    return np.float32(255) / np.float32(hi - lo)


def reference(img, window, return_window=False):
    """The definition in numpy.  img: uint16 HxW or HxWx1 (array or PIL I;16); returns the
    uint8 plane [H, W], and with return_window also (lo, hi)."""
    if not isinstance(window, Window):
        raise TypeError(f"window must be an mmdx.Window, got {type(window).__name__}")
    window.check()
    a = as_plane(img)
    lo, hi = window.levels(a)
    d = a.astype(np.float32) - np.float32(lo)
    y = np.clip(np.rint(d * scale_of(lo, hi)), 0, 255)
    assert y.dtype == np.float32
    y = y.astype(np.uint8)
    if window.invert:
        y = 255 - y
    return (y, (lo, hi)) if return_window else y


def plan(planes, window):
    """Descriptor table of the GPU passes for a list of (H, W) uint16 planes: (descs [B] of
    DESC, source bytes, destination bytes).  The source packs the 16-bit pixels with every
    image starting at a 16-byte boundary (and the buffer ending at one); the destination is
    the back-to-back (H, W, 1) uint8 layout of preprocess.plan_batch and clahe.plan.  Raises
    the documented errors before anything is uploaded."""
    if not isinstance(window, Window):
        raise TypeError(f"window must be an mmdx.Window, got {type(window).__name__}")
    window.check()
    if not len(planes):
        raise ValueError("empty batch")
    descs = np.zeros(len(planes), dtype=DESC)
    src = dst = 0
    for b, a in enumerate(planes):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint16:
            raise TypeError("windowing takes uint16 arrays")
        if a.ndim != 2:
            raise ValueError(f"expected (H, W) pixels, got {a.shape}")
        h, w = a.shape
        check_shape(h, w)
        d = descs[b]
        d["src_off"], d["dst_off"], d["w"], d["h"] = src, dst, w, h
        d["invert"] = int(window.invert)
        if window.mode == "percentile":
            d["mode"] = 0
            d["k_lo"], d["k_hi"] = ranks(h * w, window.low, window.high)
        else:
            d["mode"] = 1
            d["lo"], d["hi"] = window.lo, window.hi
            d["scale"] = scale_of(window.lo, window.hi)
        src += (2 * h * w + 15) // 16 * 16
        dst += h * w
    return descs, src, dst


def pack(planes, descs, out):
    """Copy the planes into the flat uint8 host view `out` at their descriptors' offsets."""
    for a, d in zip(planes, descs):
        o = int(d["src_off"])
        out[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
