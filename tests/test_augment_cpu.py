"""CPU: the semantics of the training augmentation (mmdx.augment) without a GPU: `reference`
against torch's grid_sample formulation, the exact cases, what `Augment.draw` draws, the host
validation, and the opt-in arguments of the loader and the driver."""
import inspect
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from mmdx import augment as A
from mmdx import data as D

MEAN = torch.tensor(A.IMAGENET_MEAN, dtype=torch.float32)
STD = torch.tensor(A.IMAGENET_STD, dtype=torch.float32)


def pixels(shape, seed=0):
    """Uniform 8-bit pixels, normalised in fp32 as preprocess_batch does."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(0, 256, shape, generator=g).float() / 255.0
    C = shape[1]
    return (p - MEAN[:C].view(1, C, 1, 1)) / STD[:C].view(1, C, 1, 1)


def fill32(C=3):
    return ((0.0 - MEAN[:C]) / STD[:C]).view(1, C, 1, 1)


def rows(B, **kw):
    r = np.tile(np.asarray(A.IDENTITY, np.float32), (B, 1))
    for k, v in kw.items():
        r[:, "a00 a01 ox a10 a11 oy gain delta".split().index(k)] = v
    return r


def test_reference_matches_grid_sample():
    B, C, H, W = 3, 3, 20, 28
    x = pixels((B, C, H, W)).double()
    p = A.Augment(hflip=0.5, seed=3).draw(B, H, W)
    got = A.reference(x, p, clamp=False, dtype=torch.float64)
    q = torch.from_numpy(p).double()
    a00, a01, ox, a10, a11, oy, gain, delta = (q[:, k].view(B, 1, 1) for k in range(8))
    cx, cy = (W - 1) / 2, (H - 1) / 2
    dx = (torch.arange(W, dtype=torch.float64) - cx).view(1, 1, W)
    dy = (torch.arange(H, dtype=torch.float64) - cy).view(1, H, 1)
    sx = a00 * dx + a01 * dy + (cx + ox)
    sy = a10 * dx + a11 * dy + (cy + oy)
    grid = torch.stack([(2 * sx + 1) / W - 1, (2 * sy + 1) / H - 1], dim=-1)
    fill = fill32().double()
    warped = TF.grid_sample(x - fill, grid, mode="bilinear", padding_mode="zeros",
                            align_corners=False) + fill
    m, s = MEAN.double().view(1, C, 1, 1), STD.double().view(1, C, 1, 1)
    g, d = gain.view(B, 1, 1, 1), delta.view(B, 1, 1, 1)
    want = g * warped + ((g - 1) * (m - 0.5) + d) / s
    assert (got - want).abs().max().item() <= 1e-10
    lo, hi = (0 - MEAN.double().view(1, C, 1, 1)) / s, (1 - MEAN.double().view(1, C, 1, 1)) / s
    lo32, hi32 = A.clamp_bounds(MEAN.numpy(), STD.numpy())
    clamped = A.reference(x, p, clamp=True, dtype=torch.float64)
    assert (clamped - torch.minimum(torch.maximum(want, lo), hi)).abs().max().item() <= 1e-6
    assert (clamped >= torch.from_numpy(lo32).double().view(1, C, 1, 1)).all()
    assert (clamped <= torch.from_numpy(hi32).double().view(1, C, 1, 1)).all()


def test_draw_is_deterministic_per_seed():
    a, b, c = A.Augment(seed=7), A.Augment(seed=7), A.Augment(seed=8)
    r1, r2 = a.draw(5, 224, 224), a.draw(5, 224, 224)
    assert r1.shape == (5, 8) and r1.dtype == np.float32
    assert np.array_equal(r1, b.draw(5, 224, 224)) and np.array_equal(r2, b.draw(5, 224, 224))
    assert not np.array_equal(r1, r2)
    assert not np.array_equal(r1, c.draw(5, 224, 224))


def test_zero_magnitudes_give_identity_rows():
    z = A.Augment(rotate=0.0, scale=(1.0, 1.0), translate=0.0, hflip=0.0, contrast=0.0,
                  brightness=0.0, seed=1)
    r = z.draw(4, 20, 28)
    assert np.array_equal(r, np.tile(np.asarray(A.IDENTITY, np.float32), (4, 1)))
    assert not np.signbit(r).any()


def test_drawn_rows_decompose_into_the_ranges():
    H, W = 200, 300
    aug = A.Augment(rotate=10.0, scale=(0.9, 1.1), translate=0.05, hflip=0.5, contrast=0.2,
                    brightness=0.1, seed=11)
    r = aug.draw(512, H, W).astype(np.float64)
    a00, a01, ox, a10, a11, oy, gain, delta = r.T
    det = a00 * a11 - a01 * a10
    s = np.abs(det) ** -0.5
    eps = 1e-5
    assert (s >= 0.9 - eps).all() and (s <= 1.1 + eps).all()
    assert s.max() - s.min() > 0.1
    theta = np.degrees(np.arctan2(-a10, a11))   # A's second row is (-sin, cos) / s
    assert (np.abs(theta) <= 10.0 + 1e-3).all() and np.abs(theta).max() > 5.0
    flips = det < 0
    assert 0.3 < flips.mean() < 0.7
    # t = -A^-1 o is the forward translation
    Ainv = np.linalg.inv(np.stack([np.stack([a00, a01], -1), np.stack([a10, a11], -1)], -2))
    t = -np.einsum("bij,bj->bi", Ainv, np.stack([ox, oy], -1))
    assert (np.abs(t[:, 0]) <= 0.05 * W + 1e-3).all() and (np.abs(t[:, 1]) <= 0.05 * H + 1e-3).all()
    assert np.abs(t[:, 0]).max() > 0.03 * W and np.abs(t[:, 1]).max() > 0.03 * H
    assert (np.abs(gain - 1) <= 0.2 + eps).all() and (np.abs(delta) <= 0.1 + eps).all()
    assert np.abs(gain - 1).max() > 0.1 and np.abs(delta).max() > 0.05


def test_forward_map_composed_with_stored_inverse_is_identity():
    """q = s R F (p - c) + c + t, then A (q - c) + c + o = p, in fp64 (affine_rows, which
    draw() rounds to fp32); and draw() is affine_rows of the documented Generator stream."""
    H, W, B = 60, 80, 64
    aug = A.Augment(hflip=0.5, seed=2)
    r = np.random.default_rng(2)
    theta = np.deg2rad(r.uniform(-aug.rotate, aug.rotate, B))
    s = r.uniform(aug.scale[0], aug.scale[1], B)
    tx = r.uniform(-aug.translate, aug.translate, B) * W
    ty = r.uniform(-aug.translate, aug.translate, B) * H
    f = np.where(r.random(B) < aug.hflip, -1.0, 1.0)
    gain = 1.0 + r.uniform(-aug.contrast, aug.contrast, B)
    delta = r.uniform(-aug.brightness, aug.brightness, B)
    rows64 = A.affine_rows(theta, s, tx, ty, f, gain, delta)
    assert rows64.dtype == np.float64
    assert np.array_equal(aug.draw(B, H, W), rows64.astype(np.float32))
    cos, sin = np.cos(theta), np.sin(theta)
    M = s[:, None, None] * np.stack([np.stack([cos * f, -sin], -1), np.stack([sin * f, cos], -1)],
                                    -2)   # s R F
    Am = np.stack([rows64[:, [0, 1]], rows64[:, [3, 4]]], -2)
    o = rows64[:, [2, 5]]
    c = np.array([(W - 1) / 2, (H - 1) / 2])
    p = np.random.default_rng(0).uniform(0, 60, size=(B, 2))
    q = np.einsum("bij,bj->bi", M, p - c) + c + np.stack([tx, ty], -1)
    back = np.einsum("bij,bj->bi", Am, q - c) + c + o
    assert np.abs(back - p).max() <= 1e-12


def test_hflip_one_gives_negative_determinant():
    r = A.Augment(hflip=1.0, seed=4).draw(32, 224, 224)
    assert (r[:, 0] * r[:, 4] - r[:, 1] * r[:, 3] < 0).all()
    r = A.Augment(hflip=0.0, seed=4).draw(32, 224, 224)
    assert (r[:, 0] * r[:, 4] - r[:, 1] * r[:, 3] > 0).all()


def test_check_params_rejects_bad_rows():
    ok = rows(2)
    assert np.array_equal(A.check_params(ok), ok)
    assert np.array_equal(A.check_params(torch.from_numpy(ok), B=2), ok)
    for k, v in ((0, np.nan), (2, np.inf), (6, -np.inf), (7, np.nan)):
        bad = ok.copy()
        bad[1, k] = v
        with pytest.raises(ValueError):
            A.check_params(bad)
    for shape in ((2, 7), (8,), (1, 2, 8), (0, 8)):
        with pytest.raises(ValueError):
            A.check_params(np.zeros(shape, np.float32))
    with pytest.raises(ValueError):
        A.check_params(ok, B=3)
    for k, v in ((0, 1.5e3), (1, -1.5e3), (3, 2e3), (4, -1e4), (2, 2e6), (5, -2e6)):
        bad = ok.copy()
        bad[0, k] = v
        with pytest.raises(ValueError):
            A.check_params(bad)
    edge = ok.copy()
    edge[0, 0], edge[0, 2] = 1e3, -1e6   # the limits themselves are legal
    A.check_params(edge)


@pytest.mark.parametrize("shape", [(2, 3, 224, 224), (3, 3, 20, 28)])
def test_exact_cases_identity_flip_shift(shape):
    x = pixels(shape)
    B, C, H, W = shape

    def same(a, b):
        return torch.equal(a.view(torch.int32), b.view(torch.int32))

    assert same(A.reference(x, rows(B), dtype=torch.float32), x)
    assert same(A.reference(x, rows(B, a00=-1.0), dtype=torch.float32), x.flip(-1))
    got = A.reference(x, rows(B, ox=3.0, oy=-2.0), dtype=torch.float32)
    want = fill32().expand(B, C, H, W).clone()
    want[:, :, 2:, :W - 3] = x[:, :, :H - 2, 3:]
    assert same(got, want)


def test_exact_case_quarter_turn():
    x = pixels((2, 3, 32, 32), seed=1)
    got = A.reference(x, rows(2, a00=0.0, a01=1.0, a10=-1.0, a11=0.0), dtype=torch.float32)
    assert torch.equal(got.view(torch.int32),
                       torch.rot90(x, -1, (2, 3)).contiguous().view(torch.int32))


def _frame(n):
    import pandas as pd
    vecs = [np.eye(13)[i % 13].tolist() for i in range(n)]
    df = pd.DataFrame(dict(image_url=[f"img{i}.png" for i in range(n)],
                           patient_details=[f"p{i}" for i in range(n)],
                           disease_classification_vector=vecs, report=["r"] * n))
    return D.enforce_raw_data_columns(df)


def test_loader_order_is_the_same_with_and_without_augment():
    df = _frame(11)
    plain = D.LocalCXRBatches(df, "", batch_size=3, shuffle=True, seed=4)
    aug = D.LocalCXRBatches(df, "", batch_size=3, shuffle=True, seed=4,
                            augment=A.Augment(seed=9))
    for _ in range(3):   # epochs
        assert np.array_equal(plain.order(), aug.order())


def test_loader_and_driver_take_augment_defaulting_to_none():
    from mmdx.training_driver import training_tests
    import mmdx
    assert mmdx.Augment is A.Augment
    for fn in (D.LocalCXRBatches.__init__, training_tests):
        p = inspect.signature(fn).parameters["augment"]
        assert p.default is None
    assert D.LocalCXRBatches(_frame(3), "").augment is None
    sig = inspect.signature(A.Augment.__init__).parameters
    assert [(k, v.default) for k, v in sig.items() if k != "self"] == [
        ("rotate", 10.0), ("scale", (0.9, 1.1)), ("translate", 0.05), ("hflip", 0.0),
        ("contrast", 0.2), ("brightness", 0.1), ("seed", 0)]


def test_augment_affine_rejects_bad_tensors_on_the_host():
    """dtype, layout and aliasing are refused before anything touches a device."""
    import mmdx.functional as F
    x = torch.zeros(2, 3, 8, 8)
    p = rows(2)
    with pytest.raises(ValueError):
        F.augment_affine(x.double(), p)
    with pytest.raises(ValueError):
        F.augment_affine(x.permute(0, 1, 3, 2), p)
    with pytest.raises(ValueError):
        F.augment_affine(x, p, out=x)
    with pytest.raises(ValueError):
        F.augment_affine(x, p, out=x.view(-1)[:].view_as(x))
    with pytest.raises(ValueError):
        F.augment_affine(torch.zeros(2, 5, 8, 8), rows(2), mean=[0.5] * 5, std=[0.5] * 5)
    with pytest.raises(ValueError):
        F.augment_affine(x, rows(3))
    bad = p.copy()
    bad[0, 0] = math.nan
    with pytest.raises(ValueError):
        F.augment_affine(x, bad)
    with pytest.raises(RuntimeError):   # a valid call on the CPU: there is no CPU path
        F.augment_affine(x, p)
