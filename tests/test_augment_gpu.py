"""GPU: the augmentation kernel (mmdx_augment_affine) against mmdx.augment.reference: the exact
cases bit for bit, parity with the fp64 reference on random draws, the photometry's closed form,
safety of far-out rows, reproducibility, the loader and one training step."""
import numpy as np
import pytest
import torch

import mmdx
import mmdx.functional as F
from mmdx import augment as A
from test_augment_cpu import MEAN, STD, fill32, pixels, rows

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32),
                       b.cpu().contiguous().view(torch.int32))


@pytest.mark.parametrize("shape", [(2, 3, 224, 224), (3, 3, 20, 28)])
def test_exact_identity_flip_shift(dev, shape):
    B, C, H, W = shape
    x = pixels(shape)
    xd = x.to(dev)
    assert same_bits(F.augment_affine(xd, rows(B)), x)
    assert same_bits(F.augment_affine(xd, rows(B, a00=-1.0)), x.flip(-1))
    want = fill32().expand(B, C, H, W).clone()
    want[:, :, 2:, :W - 3] = x[:, :, :H - 2, 3:]
    assert same_bits(F.augment_affine(xd, rows(B, ox=3.0, oy=-2.0)), want)
    assert same_bits(xd, x)   # the input is left alone


def test_exact_quarter_turn(dev):
    x = pixels((2, 3, 32, 32), seed=1)
    got = F.augment_affine(x.to(dev), rows(2, a00=0.0, a01=1.0, a10=-1.0, a11=0.0))
    assert same_bits(got, torch.rot90(x, -1, (2, 3)))


@pytest.mark.parametrize("shape", [(3, 3, 20, 28), (1, 3, 5, 300), (4, 3, 224, 224)])
def test_parity_with_fp64_reference(dev, shape):
    """Bound 1e-3, derived: source coordinates up to ~400 carry at most ~3e-5 of fp32 rounding,
    times two axes, a neighbour slope of at most 1 / std = 4.47 (uniform 8-bit pixels) and a
    gain of at most 1.3: ~3.6e-4.  A half-pixel or row / column mistake gives errors of
    order 1."""
    B, C, H, W = shape
    x = pixels(shape, seed=H)
    p = A.Augment(hflip=0.5, seed=W).draw(B, H, W)
    for clamp in (True, False):
        got = F.augment_affine(x.to(dev), p, clamp=clamp).cpu().double()
        want = A.reference(x, p, clamp=clamp, dtype=torch.float64)
        err = (got - want).abs().max().item()
        print(f"augment parity {shape} clamp={clamp}: max abs err {err:.3e}")
        assert err <= 1e-3
    assert (got - x.double()).abs().max().item() > 0.5   # the draw did move pixels


def test_photometry_closed_form_and_clamp(dev):
    B, C, H, W = 3, 3, 20, 28
    x = pixels((B, C, H, W), seed=2)
    gain = np.array([1.3, 0.7, 1.0], np.float32)
    delta = np.array([0.1, -0.1, 0.25], np.float32)
    p = rows(B, gain=gain, delta=delta)
    g = torch.from_numpy(gain).double().view(B, 1, 1, 1)
    d = torch.from_numpy(delta).double().view(B, 1, 1, 1)
    m, s = MEAN.double().view(1, C, 1, 1), STD.double().view(1, C, 1, 1)
    want = g * x.double() + ((g - 1) * (m - 0.5) + d) / s
    got = F.augment_affine(x.to(dev), p, clamp=False).cpu()
    assert (got.double() - want).abs().max().item() <= 1e-6
    # the same in pixel terms: p' = gain (p - 0.5) + 0.5 + delta
    px = x.double() * s + m
    assert ((got.double() * s + m) - (g * (px - 0.5) + 0.5 + d)).abs().max().item() <= 1e-6
    lo32, hi32 = (torch.from_numpy(v).view(1, C, 1, 1)
                  for v in A.clamp_bounds(MEAN.numpy(), STD.numpy()))
    got_c = F.augment_affine(x.to(dev), p, clamp=True).cpu()
    assert (got_c >= lo32).all() and (got_c <= hi32).all()
    assert (got_c == lo32).any() and (got_c == hi32).any()   # both ends are reached
    want_c = torch.minimum(torch.maximum(want, lo32.double()), hi32.double())
    assert (got_c.double() - want_c).abs().max().item() <= 1e-6
    # the clamp is the identity on normalised pixels, and clamp=False passes anything through
    assert same_bits(F.augment_affine(x.to(dev), rows(B), clamp=True), x)
    wild = torch.linspace(-50.0, 50.0, B * C * H * W).view(B, C, H, W).contiguous()
    assert same_bits(F.augment_affine(wild.to(dev), rows(B), clamp=False), wild)


def test_row_far_outside_gives_fill_everywhere(dev):
    B, C, H, W = 2, 3, 20, 28
    x = pixels((B, C, H, W), seed=3).to(dev)
    fill = fill32().expand(B, C, H, W)
    assert same_bits(F.augment_affine(x, rows(B, ox=2.0 * W)), fill)
    # the largest rows the host validation lets through are safe too
    far = rows(B, a00=1e3, a01=-1e3, a10=1e3, a11=1e3, ox=-1e6, oy=1e6)
    got = F.augment_affine(x, far)
    assert torch.isfinite(got).all()
    assert (got.cpu() - fill).abs().max().item() <= 1e-6


def test_rows_are_independent_and_calls_reproducible(dev):
    B, C, H, W = 3, 3, 37, 300
    x = pixels((B, C, H, W), seed=4).to(dev)
    p = A.Augment(hflip=0.5, seed=6).draw(B, H, W)
    a, b = F.augment_affine(x, p), F.augment_affine(x, p)
    assert same_bits(a, b)
    for k in range(B):
        assert same_bits(F.augment_affine(x[k:k + 1].contiguous(), p[k:k + 1]), a[k:k + 1])
    out = torch.full_like(x, float("nan"))
    assert F.augment_affine(x, p, out=out) is out and same_bits(out, a)
    with pytest.raises(ValueError):
        F.augment_affine(x, p, out=x)
    with pytest.raises(ValueError):
        F.augment_affine(x.transpose(2, 3), p)


def test_other_channel_counts_and_constants(dev):
    """C = 1, 2, 4 (each its own kernel instance) with the caller's mean / std."""
    for C in (1, 2, 4):
        mean, std = [0.5, 0.4, 0.3, 0.2][:C], [0.25, 0.2, 0.3, 0.5][:C]
        g = torch.Generator().manual_seed(C)
        x = torch.randn((2, C, 9, 70), generator=g)
        p = A.Augment(hflip=0.5, seed=C).draw(2, 9, 70)
        got = F.augment_affine(x.to(dev), p, mean=mean, std=std).cpu().double()
        want = A.reference(x, p, mean=mean, std=std, dtype=torch.float64)
        assert (got - want).abs().max().item() <= 1e-3


def test_loader_applies_the_augmentation(dev, tmp_path):
    import pandas as pd
    from mmdx import data as D
    from test_preprocess_cpu import images
    ims = images()[2:7]
    keys = []
    for i, im in enumerate(ims):
        im.save(tmp_path / f"img{i}.png")
        keys.append(f"img{i}.png")
    vecs = [np.eye(13)[i % 13].tolist() for i in range(len(keys))]
    df = pd.DataFrame(dict(image_url=keys, patient_details=[f"p{i}" for i in range(len(keys))],
                           disease_classification_vector=vecs, report=["r"] * len(keys)))
    df = D.enforce_raw_data_columns(df)
    kw = dict(batch_size=2, shuffle=True, seed=1, device=dev)
    order = D.LocalCXRBatches(df, str(tmp_path), **kw).order()
    twin = A.Augment(seed=5)   # the same rows, in the same order
    seen = 0
    for (x, details, y), (x0, details0, y0) in zip(
            D.LocalCXRBatches(df, str(tmp_path), augment=A.Augment(seed=5), **kw),
            D.LocalCXRBatches(df, str(tmp_path), augment=None, **kw)):
        idx = order[seen:seen + x.shape[0]]
        plain = mmdx.preprocess_batch([ims[i] for i in idx], dev)
        assert same_bits(x0, plain)                      # augment=None: today's output
        want = F.augment_affine(plain, twin.draw(len(idx), 224, 224))
        assert same_bits(x, want) and not same_bits(x, plain)
        assert details == details0 == [f"p{i}" for i in idx]
        assert torch.equal(y, y0)
        assert torch.equal(y.cpu(), torch.tensor([vecs[i] for i in idx], dtype=torch.float32))
        seen += x.shape[0]
    assert seen == len(ims)


def test_training_step_on_an_augmented_batch(dev):
    torch.manual_seed(0)
    x = pixels((2, 3, 224, 224), seed=5).to(dev)
    y = torch.tensor(np.eye(13)[[1, 4]], dtype=torch.float32, device=dev)
    xa = A.Augment(seed=3)(x)
    assert xa.shape == x.shape and not same_bits(xa, x)
    model = mmdx.ImageEncoderCNN("resnet18", 1024, 13).to(dev)
    model.unfreeze_backbone()
    loss = mmdx.BCEWithLogitsLoss()(model(xa)["logits"], y)
    loss.backward()
    assert torch.isfinite(loss).item()
    g = model.proj.weight.grad
    assert g is not None and torch.isfinite(g).all()
