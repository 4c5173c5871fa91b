"""Inputs shared by tests/test_clahe_cpu.py and tests/test_clahe_gpu.py: seeded images, and the
step-3 redistribution written as OpenCV's serial loop (independent of mmdx.clahe's closed
form)."""
import functools

import numpy as np


def random_image(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def smooth_image(h=224, w=224):
    """128 + 100 sin(x / 37) cos(y / 29): few grey levels per tile, so the clipped excess is
    large and the residual step is 1."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.rint(128 + 100 * np.sin(x / 37) * np.cos(y / 29)).astype(np.uint8)


def two_level_image(h=64, w=96):
    a = np.full((h, w), 40, np.uint8)
    a[:, w // 3:] = 200
    a[h // 2:, : w // 2] = 200
    return a


def serial_redistribute(hist, clip):
    """One tile: clip, then hand the excess out as OpenCV's loop does."""
    h = [int(v) for v in hist]
    if clip <= 0:
        return h
    clipped = 0
    for i in range(256):
        if h[i] > clip:
            clipped += h[i] - clip
            h[i] = clip
    batch = clipped // 256
    residual = clipped - batch * 256
    for i in range(256):
        h[i] += batch
    if residual != 0:
        step = max(256 // residual, 1)
        i = 0
        while i < 256 and residual > 0:
            h[i] += 1
            i += step
            residual -= 1
    return h


# name -> (image factory, clip_limit, tiles): the kernel cases of tests/test_clahe_gpu.py
KERNEL_CASES = {
    "clip1_16x16": (lambda: random_image((16, 16), 1), 2.0, (2, 2)),
    "reflect_29x37": (lambda: random_image((29, 37), 2), 2.0, (4, 3)),
    "reflect_30x32": (lambda: random_image((30, 32), 3), 2.0, (8, 8)),
    "rgb_20x24": (lambda: random_image((20, 24, 3), 4), 2.0, (2, 2)),
    "random_224": (lambda: random_image((224, 224), 5), 2.0, (8, 8)),
    "smooth_224": (smooth_image, 2.0, (8, 8)),
    "clip0_96x80": (lambda: random_image((96, 80), 6), 0, (8, 8)),
    "clip0p5_96x80": (lambda: random_image((96, 80), 6), 0.5, (8, 8)),
    "clip40_96x80": (lambda: random_image((96, 80), 6), 40, (8, 8)),
    "clip0_256": (lambda: random_image((256, 256), 7), 0, (2, 2)),
    "clip0p5_256": (lambda: random_image((256, 256), 7), 0.5, (2, 2)),
    "clip40_256": (lambda: random_image((256, 256), 7), 40, (2, 2)),
    "all0": (lambda: np.zeros((48, 40), np.uint8), 2.0, (4, 4)),
    "all255": (lambda: np.full((48, 40), 255, np.uint8), 2.0, (4, 4)),
    "two_level": (two_level_image, 2.0, (4, 4)),
    "constant_1024": (lambda: np.full((1024, 1024), 77, np.uint8), 2.0, (2, 2)),
    "random_1024": (lambda: random_image((1024, 1024), 8), 2.0, (8, 8)),
    "tiles16_64x64": (lambda: random_image((64, 64), 9), 2.0, (16, 16)),
}

MIXED_SHAPES = [(16, 16, 1), (29, 37, 1), (64, 48, 3), (224, 224, 1)]


def mixed_batch():
    return [random_image(s, 20 + i) for i, s in enumerate(MIXED_SHAPES)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(image, clip_limit, tiles, reference output, reference LUTs), computed once."""
    from mmdx.clahe import reference
    make, clip_limit, tiles = KERNEL_CASES[name]
    img = make()
    out, luts = reference(img, clip_limit, tiles, return_luts=True)
    for a in (img, out, luts):
        a.setflags(write=False)
    return img, clip_limit, tiles, out, luts
