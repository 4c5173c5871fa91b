"""GPU: the Grad-CAM kernels (mmdx_cam_fwd, mmdx_cam_resize) against fp64 references, and
mmdx.explain.grad_cam / inference(explain=...) against autograd on the CPU oracle.

Kernel level
- exact: integer-valued inputs whose every partial sum is exact in fp32 in any order, so raw must
  equal the fp64 reference bit for bit, for fp32 / bf16 / fp16 feature maps;
- random floats: |raw - ref64| <= (K + 2) 2^-24 sum_k |alpha fmap| elementwise, the fp32
  summation bound of any order (the reference uses the same dtype-rounded inputs; ReLU is
  1-Lipschitz, so the bound survives it);
- resize: fp64 F.interpolate(bilinear, align_corners=False) of raw / max on the CPU, 1e-5
  absolute (values in [0, 1]; the fp32 source coordinate (d + 0.5) H / Ho - 0.5 with H <= 32
  carries <= ~4e-6 into a lerp weight, two axes, one rounding of the division); the 7 -> 224 and
  2 -> 64 cases have weights that are multiples of 1/64, exact in fp32, and must meet 1e-6.

Model level: the oracle map is relu(sum_k mean_hw(d logit_c / d A) A) with A the output of
ref.image.backbone[7] (layer4), by torch.autograd on the CPU, eval mode.  raw is compared per
sample over all 13 classes flattened together (some 2 x 2 oracle maps are identically zero, a
per-class cosine would be ill-posed there): cosine >= 0.9999, |norm ratio - 1| <= 1e-3 (the
project's gradient criteria) and rel_err <= 1e-4 (its fp32 criterion).

bf16 (resnet18, 64 x 64 input, 2 samples), measured on an MI355X against the same oracle maps
(profiles/cam_parity.txt, written by tools/cam_bench.py --parity over the model seeds 0..3):
worst 1 - cos 1.634e-4, worst rel_err 2.101e-2 (BF16_MEASURED_* below); the test asserts 4x
those, the margin covering run-to-run differences of the bf16 trunk across seeds.  A wrong
alpha scale or a transposed map gives 1 - cos >> 1e-2.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF
from PIL import Image

import mmdx
import mmdx.functional as F
from parity_util import build_pair, cosine, mmdx_forward, norm_ratio, rel_err, synth_batch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (B, H, W, K, C)
SHAPES = [
    (1, 7, 7, 2048, 13),   # the real resnet50 geometry
    (2, 2, 2, 512, 13),    # resnet18 at 64 x 64 input
    (2, 3, 5, 520, 3),     # H != W, K no multiple of 64 or 512
    (1, 1, 1, 8, 1),       # the smallest legal shape
    (3, 4, 4, 64, 64),     # C at its limit
    (1, 32, 32, 8, 2),     # H * W at its limit
]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]

# measured on an MI355X (profiles/cam_parity.txt); the bf16 test asserts 4x these
BF16_MEASURED_1MCOS = 1.634e-4   # worst of 8 (4 model seeds x 2 samples); seed 0: 1.483e-4
BF16_MEASURED_REL = 2.101e-2     # seed 0: 1.550e-2


def _ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v).split(".")[-1]


def _ref_raw(fmap, alpha):
    """fp64 on the CPU from the (already dtype-rounded) inputs: (relu'd sums, sums of |terms|)."""
    f, a = fmap.double().cpu(), alpha.double().cpu()
    s = torch.einsum("bck,bhwk->bchw", a, f)
    mag = torch.einsum("bck,bhwk->bchw", a.abs(), f.abs())
    return s.clamp(min=0), mag


# ----------------------------------------------------------------------------- cam_raw
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_cam_raw_exact_on_integer_inputs(dev, shape, dtype):
    B, H, W, K, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    fmap = torch.randint(-4, 5, (B, H, W, K), generator=g).to(dtype)
    alpha = torch.randint(-128, 129, (B, C, K), generator=g).float() / 64.0
    # |term| <= 8 = 2^9 units of 2^-6, K <= 2048 terms: every partial sum < 2^20 units
    want, _ = _ref_raw(fmap, alpha)
    got = F.cam_raw(fmap.to(dev), alpha.to(dev))
    assert got.shape == (B, C, H, W) and got.dtype == torch.float32
    assert (want > 0).any() or want.numel() < 8
    assert torch.equal(got.cpu(), want.float())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_cam_raw_random_within_the_fp32_summation_bound(dev, shape, dtype):
    B, H, W, K, C = shape
    g = torch.Generator().manual_seed(1 + sum(shape))
    fmap = torch.randn(B, H, W, K, generator=g).clamp(min=0).to(dtype)  # post-ReLU activations
    alpha = torch.randn(B, C, K, generator=g)
    alpha[B - 1] = -alpha[B - 1].abs() - 1e-3    # one sample all negative: its raw is exactly 0
    if B == 1:                                   # (the only sample: keep the others' signs
        alpha = torch.randn(B, C, K, generator=g)   # and make its last class the negative one)
        alpha[0, C - 1] = -alpha[0, C - 1].abs() - 1e-3
    want, mag = _ref_raw(fmap, alpha)
    got = F.cam_raw(fmap.to(dev), alpha.to(dev)).cpu().double()
    err = (got - want).abs()
    bound = (K + 2) * 2.0 ** -24 * mag
    worst = (err - bound).max().item()
    print(f"cam_raw {shape} {dtype}: max err {err.max().item():.3e}, "
          f"max err / bound {(err / bound.clamp(min=1e-300)).max().item():.3e}")
    assert worst <= 0.0, f"error exceeds the summation bound by {worst:.3e}"
    if B > 1:
        assert (got[B - 1] == 0).all()
    else:
        assert (got[0, C - 1] == 0).all()
    if C > 1:
        assert (got > 0).any()


def test_cam_raw_bit_reproducible(dev):
    g = torch.Generator().manual_seed(7)
    fmap = torch.randn(4, 7, 7, 2048, generator=g).to(torch.bfloat16).to(dev)
    alpha = torch.randn(4, 13, 2048, generator=g).to(dev)
    a = F.cam_raw(fmap, alpha).cpu().numpy().tobytes()
    b = F.cam_raw(fmap, alpha).cpu().numpy().tobytes()
    assert a == b


def test_cam_raw_every_pixels_per_wave_variant_agrees(dev):
    """The launch picks 1, 2 or 4 pixels per wave from the batch size: the same sample must
    come out bit-identical whichever variant computed it (49 pixels: uneven last tiles)."""
    g = torch.Generator().manual_seed(11)
    fmap = torch.randint(-4, 5, (160, 7, 7, 64), generator=g).to(torch.bfloat16)
    alpha = torch.randint(-128, 129, (160, 13, 64), generator=g).float() / 64.0
    want, _ = _ref_raw(fmap, alpha)
    for nb in (1, 80, 160):   # 13 blocks -> 1 pixel per wave, 560 -> 2, 640 -> 4
        got = F.cam_raw(fmap[:nb].contiguous().to(dev), alpha[:nb].contiguous().to(dev))
        assert torch.equal(got.cpu(), want[:nb].float()), nb


def test_cam_wrappers_check_their_inputs(dev):
    f = torch.zeros(2, 2, 2, 16, device=dev)
    a = torch.zeros(2, 3, 16, device=dev)
    with pytest.raises(RuntimeError, match="contiguous"):
        F.cam_raw(f.transpose(1, 2), a)
    with pytest.raises(TypeError):
        F.cam_raw(f, a.half())
    with pytest.raises(TypeError):
        F.cam_raw(f.double(), a)
    with pytest.raises(ValueError):
        F.cam_raw(f, a[:, :, :8].contiguous())
    with pytest.raises(ValueError):
        F.cam_raw(f[0], a)
    with pytest.raises(RuntimeError, match="K = 12"):
        F.cam_raw(torch.zeros(1, 2, 2, 12, device=dev), torch.zeros(1, 3, 12, device=dev))
    with pytest.raises(RuntimeError, match="C = 65"):
        F.cam_raw(f, torch.zeros(2, 65, 16, device=dev))
    with pytest.raises(RuntimeError, match="Ho = 4097"):
        F.cam_resize(torch.zeros(1, 2, 2, device=dev), (4097, 4))
    with pytest.raises(TypeError):
        F.cam_resize(torch.zeros(1, 2, 2, device=dev).half(), (4, 4))
    with pytest.raises(RuntimeError, match="contiguous"):
        F.cam_resize(torch.zeros(1, 2, 3, device=dev).transpose(1, 2), (4, 4))


# ----------------------------------------------------------------------------- cam_resize
RESIZES = [((7, 7), (224, 224), 1e-6), ((2, 2), (64, 64), 1e-6), ((1, 1), (5, 3), 1e-5),
           ((3, 5), (17, 40), 1e-5), ((16, 16), (512, 512), 1e-5)]


def _maps(hw, seed):
    """[2, 3, H, W] in [0, 1], one map all zero."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.rand(2, 3, *hw, generator=g)
    raw[1, 1] = 0.0
    return raw


@pytest.mark.parametrize("hw,out,tol", RESIZES, ids=lambda v: _ids(v) if isinstance(v, tuple)
                         else None)
def test_cam_resize_matches_fp64_interpolate(dev, hw, out, tol):
    raw = _maps(hw, 3 + hw[0] * hw[1])
    r64 = raw.double()
    peak = r64.amax(dim=(2, 3), keepdim=True)
    norm = torch.where(peak > 0, r64 / peak.clamp(min=1e-300), torch.zeros_like(r64))
    want = TF.interpolate(norm, size=out, mode="bilinear", align_corners=False)
    got = F.cam_resize(raw.to(dev), out).cpu()
    assert got.shape == (2, 3, *out) and got.dtype == torch.float32
    assert torch.isfinite(got).all()
    err = (got.double() - want).abs().max().item()
    print(f"cam_resize {hw} -> {out}: max abs err {err:.3e}")
    assert err <= tol
    assert (got[1, 1] == 0).all()                     # the all-zero map: zeros, no NaN
    # normalize=False is the plain interpolation
    want0 = TF.interpolate(r64, size=out, mode="bilinear", align_corners=False)
    got0 = F.cam_resize(raw.to(dev), out, normalize=False).cpu()
    err0 = (got0.double() - want0).abs().max().item()
    print(f"cam_resize {hw} -> {out}, normalize off: max abs err {err0:.3e}")
    assert err0 <= tol


def test_cam_resize_bit_reproducible(dev):
    raw = _maps((7, 7), 5).to(dev)
    a = F.cam_resize(raw, (224, 224)).cpu().numpy().tobytes()
    b = F.cam_resize(raw, (224, 224)).cpu().numpy().tobytes()
    assert a == b


# ----------------------------------------------------------------------------- model level
_CASES = {}


def _case(arch, hw):
    """(x, ids, mask, oracle maps [B, 13, H, W], oracle logits) of the fp32 CPU oracle, computed
    once.  (Its own distance from an fp64 run of itself on these inputs: 1 - cos <= 2.1e-12,
    norm ratio <= 7.1e-7, rel_err <= 2.1e-6, 50x inside the tightest criterion below.)"""
    key = (arch, hw)
    if key not in _CASES:
        ref = build_pair(arch, "embed-mean")[0].eval()
        x, ids, mask, _ = synth_batch(2, 16, hw=hw)
        keep = {}
        h = ref.image.backbone[7].register_forward_hook(lambda m, i, o: keep.update(A=o))
        logits = ref(x, ids, mask)
        h.remove()
        A = keep["A"]                                       # [B, K, H, W]
        maps = []
        for c in range(13):
            (gA,) = torch.autograd.grad(logits[:, c].sum(), A, retain_graph=True)
            w = gA.mean(dim=(2, 3), keepdim=True)
            maps.append((w * A).sum(1).clamp(min=0))
        _CASES[key] = (x, ids, mask, torch.stack(maps, 1).detach(), logits.detach())
    return _CASES[key]


def _mine(arch, dtype, dev):
    _, img, txt, fus = build_pair(arch, "embed-mean", dtype=dtype)
    return img.to(dev).eval(), txt.to(dev).eval(), fus.to(dev).eval()


@pytest.mark.parametrize("arch,hw", [("resnet18", 64), ("resnet50", 64), ("resnet18", 224)])
def test_grad_cam_matches_oracle_autograd_fp32(dev, arch, hw):
    from mmdx.explain import grad_cam
    x, ids, mask, want, _ = _case(arch, hw)
    img, txt, fus = _mine(arch, torch.float32, dev)
    xd, idd, md = x.to(dev), ids.to(dev), mask.to(dev)
    out = grad_cam(img, txt, fus, xd, idd, md)
    raw = out["raw"].cpu()
    assert raw.shape == want.shape and out["classes"] == list(range(13))
    assert out["cam"].shape == (2, 13, 224, 224)
    for b in range(2):
        cos, nr, re = cosine(raw[b], want[b]), norm_ratio(raw[b], want[b]), rel_err(raw[b], want[b])
        print(f"grad_cam {arch} {hw} sample {b}: 1-cos {1 - cos:.2e}, |norm ratio - 1| "
              f"{abs(nr - 1):.2e}, rel_err {re:.2e}")
        assert cos >= 0.9999
        assert abs(nr - 1.0) <= 1e-3
        assert re <= 1e-4
    with torch.no_grad():
        plain = mmdx_forward(img, txt, fus, xd, idd, md)
    assert (out["logits"] - plain).abs().max().item() <= 1e-5
    # a class subset is the same maps, in the order asked for
    sub = grad_cam(img, txt, fus, xd, idd, md, classes=[5, 0], out_size=None)
    assert "cam" not in sub and sub["classes"] == [5, 0]
    tol = 1e-5 * out["raw"].abs().max().item()   # (another row count in the head GEMMs)
    assert (sub["raw"][:, 0] - out["raw"][:, 5]).abs().max().item() <= tol
    assert (sub["raw"][:, 1] - out["raw"][:, 0]).abs().max().item() <= tol
    cam = out["cam"]
    assert cam.min().item() >= 0.0 and cam.max().item() <= 1.0 + 1e-6


def test_grad_cam_bf16_within_4x_of_the_measured_error(dev):
    from mmdx.explain import grad_cam
    x, ids, mask, want, _ = _case("resnet18", 64)
    img, txt, fus = _mine("resnet18", torch.bfloat16, dev)
    raw = grad_cam(img, txt, fus, x.to(dev), ids.to(dev), mask.to(dev), out_size=None)["raw"]
    raw = raw.cpu()
    omc = max(1.0 - cosine(raw[b], want[b]) for b in range(2))
    rel = max(rel_err(raw[b], want[b]) for b in range(2))
    print(f"grad_cam bf16 resnet18 64: worst 1-cos {omc:.3e}, worst rel_err {rel:.3e}")
    assert omc <= 4 * BF16_MEASURED_1MCOS
    assert rel <= 4 * BF16_MEASURED_REL


def test_grad_cam_has_no_side_effects(dev):
    from mmdx.explain import grad_cam
    x, ids, mask, _, _ = _case("resnet18", 64)
    img, txt, fus = _mine("resnet18", torch.float32, dev)
    mods = (img, txt, fus)
    xd, idd, md = x.to(dev), ids.to(dev), mask.to(dev)
    base = grad_cam(img, txt, fus, xd, idd, md, out_size=None)["raw"]
    assert all(not m.training for top in mods for m in top.modules())
    assert all(p.grad is None for top in mods for p in top.parameters())
    # train mode on entry (the backbone frozen in eval, the heads in train, as phase 1 leaves
    # them): same maps, flags back as they were, running statistics untouched
    img.train()
    img.freeze_backbone()
    txt.train()
    fus.train()
    flags = [(m, m.training) for top in mods for m in top.modules()]
    assert any(f for _, f in flags) and not all(f for _, f in flags)
    bn = [b.clone() for b in img.backbone.buffers()]
    with torch.no_grad():
        again = grad_cam(img, txt, fus, xd, idd, md, out_size=None)["raw"]
    assert torch.equal(again, base)
    assert all(m.training == f for m, f in flags)
    assert all(p.grad is None for top in mods for p in top.parameters())
    assert all(torch.equal(a, b) for a, b in zip(bn, img.backbone.buffers()))


# ----------------------------------------------------------------------------- inference()
def test_inference_explain(dev):
    from mmdx.inference_pipeline import inference
    _, img, txt, fus = build_pair("resnet18", "embed-mean")
    pil = Image.open(os.path.join(GOLD, "e1.jpg")).convert("RGB")
    with open(os.path.join(GOLD, "patient_details.json")) as f:
        text = json.load(f)["e1.jpg"]
    bundle = {"fusion_model": fus, "image_encoder": img, "text_encoder": txt,
              "class_names": mmdx.DISEASES, "thresholds": [0.5] * 13, "version": 999,
              "t5_tok": None}
    plain = inference(bundle, pil, text, device="cuda")
    assert set(plain) == {"report_text", "disease_probs", "disease_vector", "model_version",
                          "report_generated", "report_ids"}
    out = inference(bundle, pil, text, device="cuda", explain=3)
    assert set(out) == set(plain) | {"heatmaps"}
    assert out["disease_probs"] == plain["disease_probs"]          # bit-identical floats
    assert out["disease_vector"] == plain["disease_vector"]
    top3 = sorted(mmdx.DISEASES, key=lambda c: -plain["disease_probs"][c])[:3]
    assert list(out["heatmaps"]) == top3
    for name, m in out["heatmaps"].items():
        assert isinstance(m, np.ndarray) and m.shape == (224, 224) and m.dtype == np.float32
        assert np.isfinite(m).all() and m.min() >= 0.0 and m.max() <= 1.0
        assert m.max() == 1.0 or not m.any(), name
    # by name, and by threshold (thresholds of 2: no class reaches one, so the top-1 class)
    named = inference(bundle, pil, text, device="cuda", explain=[top3[1]])
    assert list(named["heatmaps"]) == [top3[1]]
    assert np.abs(named["heatmaps"][top3[1]] - out["heatmaps"][top3[1]]).max() <= 1e-4
    hi = inference(dict(bundle, thresholds=[2.0] * 13), pil, text, device="cuda", explain=True)
    assert list(hi["heatmaps"]) == [top3[0]]
