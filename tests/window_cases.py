"""Inputs shared by tests/test_window_cpu.py and tests/test_window_gpu.py: seeded 16-bit images
(every pixel class of the issue at the smallest shapes the passes can go wrong at), the window
settings, and the references, computed once per (image, setting)."""
import functools

import numpy as np

# tails of the 16-byte loads (8 pixels) and of the 8-byte stores, odd row lengths, one pixel
SHAPES = [(1, 1), (1, 7), (3, 5), (37, 53), (64, 64), (257, 129)]
BIG = (1024, 1024)   # several histogram blocks


def uniform(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 65536, shape, dtype=np.uint16)


def flat(shape, value):
    return np.full(shape, value, np.uint16)


def two_valued(shape, seed=0):
    return (np.random.default_rng(seed).integers(0, 2, shape) * 65535).astype(np.uint16)


def gauss12(shape, seed=0):
    """12-bit detector values piled around 1800: a few hundred neighbouring levels."""
    a = np.random.default_rng(seed).normal(1800, 150, shape)
    return np.clip(np.rint(a), 0, 4095).astype(np.uint16)


def radiograph(shape, seed=0):
    """The field of tools/clahe_bench.py in 12 bits: a smooth ramp with noise, a saturated flat
    margin of a quarter of the width and a black collimator band."""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = 640 + 2400 * (0.5 + 0.5 * np.sin(x * (6.0 / w)) * np.cos(y * (4.0 / h)))
    a = a + np.random.default_rng(seed).normal(0, 12, shape).astype(np.float32)
    a[:, : w // 4] = 4095
    a[h - h // 8:, :] = 0
    return np.clip(np.rint(a), 0, 4095).astype(np.uint16)


def boundary(shape):
    """A quarter of the pixels at 100, half at 2000, a quarter at 60000 (n a multiple of 4), in
    scattered order: with low = 25, high = 75 both ranks are the first pixel of the NEXT
    populated level (k_lo = n / 4 -> 2000, k_hi = 3 n / 4 -> 60000)."""
    n = shape[0] * shape[1]
    assert n % 4 == 0
    a = np.concatenate([np.full(n // 4, 100), np.full(n // 2, 2000), np.full(n // 4, 60000)])
    return np.random.default_rng(3).permutation(a).astype(np.uint16).reshape(shape)


def with_65535(shape, seed=0):
    a = uniform(shape, seed)
    a.reshape(-1)[a.size // 3] = 65535
    a.reshape(-1)[a.size // 2] = 0
    return a


# name -> image factory: the kernel cases of tests/test_window_gpu.py
IMAGES = {f"uniform_{h}x{w}": functools.partial(uniform, (h, w), 10 + i)
          for i, (h, w) in enumerate(SHAPES)}
IMAGES.update({
    "uniform_big": lambda: uniform(BIG, 20),
    "all0_37x53": lambda: flat((37, 53), 0),
    "all40000_37x53": lambda: flat((37, 53), 40000),
    "all65535_37x53": lambda: flat((37, 53), 65535),
    "all40000_1x1": lambda: flat((1, 1), 40000),
    "all40000_big": lambda: flat(BIG, 40000),
    "two_valued_257x129": lambda: two_valued((257, 129), 21),
    "two_valued_3x5": lambda: two_valued((3, 5), 22),
    "gauss12_37x53": lambda: gauss12((37, 53), 23),
    "gauss12_257x129": lambda: gauss12((257, 129), 24),
    "gauss12_big": lambda: gauss12(BIG, 25),
    "radiograph_257x129": lambda: radiograph((257, 129), 26),
    "radiograph_big": lambda: radiograph(BIG, 27),
    "boundary_2x2": lambda: boundary((2, 2)),
    "boundary_64x64": lambda: boundary((64, 64)),
    "with65535_37x53": lambda: with_65535((37, 53), 28),
    "with65535_257x129": lambda: with_65535((257, 129), 29),
})


def windows():
    """name -> Window: every mode of the issue, each also inverted."""
    from mmdx.window import Window
    base = {
        "percentile": dict(mode="percentile", low=0.5, high=99.5),
        "quartiles": dict(mode="percentile", low=25, high=75),   # the `boundary` ranks
        "minmax": dict(mode="percentile", low=0, high=100),
        "fixed_half": dict(mode="fixed", lo=1023.5, hi=3071.5),
        "fixed_wide": dict(mode="fixed", lo=-1000.5, hi=70000.0),
    }
    out = {}
    for name, kw in base.items():
        out[name] = Window(**kw)
        out[name + "_inv"] = Window(invert=True, **kw)
    return out


@functools.lru_cache(maxsize=None)
def image(name):
    a = IMAGES[name]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected(name, wname):
    """(reference output, (lo, hi)) of image `name` under window `wname`, computed once."""
    from mmdx.window import reference
    out, win = reference(image(name), windows()[wname], return_window=True)
    out.setflags(write=False)
    return out, win


def mixed_batch():
    """Every small shape in one batch (offsets, the 16-byte padding between sources, every
    destination alignment), pixel classes mixed."""
    return [image(f"uniform_{h}x{w}") for h, w in SHAPES] + \
           [image("gauss12_37x53"), image("all65535_37x53"), image("boundary_2x2")]
