"""GPU: the ViT explanation kernels (mmdx_attention_relevance, mmdx_rollout_step) against
float64 references, and mmdx.explain.attention_rollout / transformer_attribution /
inference(explain=...) on a two-layer ViT bundle against the float64 CPU references.

Kernel level: the error bound of attention_relevance is derived in vit_explain_cases (a logit's
fp32 dot error through the softmax, the dP dot error through relu(P dP), the head mean) and
evaluated elementwise in float64 from the same dtype-rounded inputs; nothing in it is tuned.
rollout_step with non-negative inputs: Ls fused multiply-adds and the final alpha r + beta s
round Ls + 2 times, every partial sum <= the result, so |r' - ref| <= (Ls + 3) u ref, u = 2^-24.

Model level (VitTrunk(layers=2) in an ImageEncoderCNN("vit_b_16"), weights shared with the
oracle pair, B = 2, three classes): fp32 meets the project's criteria, rel_err <= 1e-4 for the
rollout row and the logits, 1 - cos <= 1e-4 and |norm ratio - 1| <= 1e-3 for the class maps
(per sample over its classes' patch maps flattened).

fp16 / bf16, measured on an MI355X against the same float64 maps over the model seeds 0..3
(profiles/vit_explain_parity.txt, written by tools/vit_explain_bench.py --parity): the worst
values are the *_MEASURED constants below; the tests assert 4x those, the margin
tests/test_cam_gpu.py uses for the run-to-run differences of a 16-bit trunk across seeds.
"""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import mmdx
import mmdx.explain
import mmdx.functional as F
import vit_explain_cases as C

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = C.U

# (B, Ls, H): the real geometry, one token, one past each tile edge (16 keys, 32 queries), a
# full tile, the limit
SHAPES = [(1, 197, 12), (2, 1, 1), (1, 2, 3), (1, 16, 1), (2, 17, 2), (1, 33, 12), (3, 64, 12),
          (1, 256, 2)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]

# measured on an MI355X (profiles/vit_explain_parity.txt): worst over the model seeds 0..3
FP16_MEASURED_1MCOS = 1.327e-7   # seed 0: 1.210e-7
FP16_MEASURED_NORM = 2.577e-4    # seed 0: 8.731e-5
FP16_MEASURED_LOGITS = 2.670e-3  # seed 0: 3.595e-4
FP16_MEASURED_ROLLOUT = 4.004e-6  # seed 0: 3.244e-6
BF16_MEASURED_1MCOS = 9.222e-6   # seed 0: 8.833e-6
BF16_MEASURED_NORM = 1.259e-3    # seed 0: 1.259e-3
BF16_MEASURED_LOGITS = 1.195e-2  # seed 0: 6.823e-3
BF16_MEASURED_ROLLOUT = 2.765e-5  # seed 0: 2.765e-5
MEASURED = {torch.float16: (FP16_MEASURED_1MCOS, FP16_MEASURED_NORM, FP16_MEASURED_LOGITS,
                            FP16_MEASURED_ROLLOUT),
            torch.bfloat16: (BF16_MEASURED_1MCOS, BF16_MEASURED_NORM, BF16_MEASURED_LOGITS,
                             BF16_MEASURED_ROLLOUT)}


def _ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v).split(".")[-1]


def _operands(shape, dtype, seed=0):
    """qkv [B * Ls, 3 * H * 64] ~ N(0, 1) (logits ~ N(0, 1)) and dout on a grid of 1/64 (exact in
    every dtype, no subnormals, so 4 * dout is exact too), both rounded to dtype."""
    B, Ls, H = shape
    g = torch.Generator().manual_seed(seed + 7 * sum(shape))
    qkv = torch.randn(B * Ls, 3 * H * 64, generator=g).to(dtype)
    dout = ((torch.randn(B * Ls, H * 64, generator=g) * 16).round() / 64).to(dtype)
    return qkv, dout


def _check(got, ref, bound, what):
    got = got.cpu().double()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = (got - ref).abs()
    ratio = (err / bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, max err / bound {ratio:.3e}")
    assert ratio <= 1.0, f"{what}: the error exceeds the bound {ratio:.3f} times"


# ----------------------------------------------------------------------------- attention_relevance
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("mode", ["plain", "weighted"])
def test_attention_relevance_within_the_derived_bound(dev, mode, shape, dtype):
    B, Ls, H = shape
    qkv, dout = _operands(shape, dtype)
    dout = dout if mode == "weighted" else None
    ref, bound = C.relevance_reference(qkv, dout, B, Ls, H, 0.125)
    got = F.attention_relevance(qkv.to(dev), B, Ls, H, 0.125,
                                dout=None if dout is None else dout.to(dev))
    assert got.dtype == torch.float32 and got.shape == (B, Ls, Ls)
    _check(got, ref, bound, f"attention_relevance {mode} {shape} {dtype}")
    if mode == "plain":
        assert (got.sum(-1).cpu().double() - 1).abs().max().item() <= (Ls + 70) * U
    else:
        assert (got >= 0).all() and (Ls == 1 or (got > 0).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("mode", ["plain", "weighted"])
def test_attention_relevance_with_logits_of_100(dev, mode, dtype):
    """Queries scaled until the unshifted logits reach +-100: exp(100) would overflow an
    unshifted softmax's sum; with the maximum subtracted the result stays inside the bound."""
    shape = (2, 65, 3)
    B, Ls, H = shape
    qkv, dout = _operands(shape, dtype, seed=1)
    t = qkv.double().view(B, Ls, 3, H, 64)
    peak = (0.125 * torch.einsum("bqhd,bkhd->bhqk", t[:, :, 0], t[:, :, 1])).abs().max().item()
    t = t.clone()
    t[:, :, 0] *= 100.0 / peak
    qkv = t.view(B * Ls, -1).to(dtype)
    dout = dout if mode == "weighted" else None
    ref, bound = C.relevance_reference(qkv, dout, B, Ls, H, 0.125)
    t = qkv.double().view(B, Ls, 3, H, 64)
    logits = 0.125 * torch.einsum("bqhd,bkhd->bhqk", t[:, :, 0], t[:, :, 1])
    assert logits.abs().max().item() >= 95          # (the rounding to dtype moves it a little)
    assert logits.max().item() >= 60 and logits.min().item() <= -60
    got = F.attention_relevance(qkv.to(dev), B, Ls, H, 0.125,
                                dout=None if dout is None else dout.to(dev))
    _check(got, ref, bound, f"attention_relevance {mode} logits +-100 {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_attention_relevance_special_values(dev, dtype):
    shape = (2, 37, 5)
    B, Ls, H = shape
    qkv, dout = _operands(shape, dtype, seed=2)
    qd, dd = qkv.to(dev), dout.to(dev)
    # all-zero queries: uniform rows
    zq = qkv.clone().view(B * Ls, 3, H * 64)
    zq[:, 0] = 0
    flat = F.attention_relevance(zq.view(B * Ls, -1).to(dev), B, Ls, H, 0.125)
    assert (flat.cpu().double() - 1.0 / Ls).abs().max().item() <= 4 * U
    # dout = 0: exactly zero; dout * 4: exactly 4 x
    assert not F.attention_relevance(qd, B, Ls, H, 0.125, dout=torch.zeros_like(dd)).any()
    one = F.attention_relevance(qd, B, Ls, H, 0.125, dout=dd)
    four = F.attention_relevance(qd, B, Ls, H, 0.125, dout=dd * 4)
    assert one.any() and torch.equal(four, one * 4)
    # into the caller's buffer
    out = torch.full((B, Ls, Ls), -1.0, device=dev)
    assert F.attention_relevance(qd, B, Ls, H, 0.125, dout=dd, out=out) is out
    assert torch.equal(out, one)


def test_attention_relevance_reproducible_and_independent_of_the_batch(dev):
    shape = (3, 64, 12)
    B, Ls, H = shape
    qkv, dout = _operands(shape, torch.float16, seed=3)
    qd, dd = qkv.to(dev), dout.to(dev)
    for d in (None, dd):
        a = F.attention_relevance(qd, B, Ls, H, 0.125, dout=d)
        b = F.attention_relevance(qd, B, Ls, H, 0.125, dout=d)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        # the last sample alone (another grid) gives the same bits
        solo = F.attention_relevance(qd[2 * Ls:].contiguous(), 1, Ls, H, 0.125,
                                     dout=None if d is None else d[2 * Ls:].contiguous())
        assert torch.equal(solo[0], a[2])


def test_wrappers_refuse_aliasing_and_limits_on_the_device(dev):
    qkv = torch.zeros(2 * 5, 3 * 2 * 64, device=dev)
    with pytest.raises(ValueError, match="shares memory"):
        F.attention_relevance(qkv, 2, 5, 2, 0.125, out=qkv.view(-1)[:50].view(2, 5, 5))
    with pytest.raises(ValueError, match="outside"):
        F.attention_relevance(torch.zeros(257, 192, device=dev), 1, 257, 1, 0.125)
    with pytest.raises(ValueError, match="outside"):
        F.attention_relevance(torch.zeros(4, 3 * 17 * 64, device=dev), 1, 4, 17, 0.125)
    with pytest.raises(ValueError, match="GPU"):
        F.attention_relevance(qkv, 2, 5, 2, 0.125, dout=torch.zeros(2 * 5, 2 * 64))
    r, abar = torch.rand(2, 5, device=dev), torch.rand(2, 5, 5, device=dev)
    with pytest.raises(ValueError, match="shares memory"):
        F.rollout_step(r, abar, 1.0, 1.0, out=r)
    with pytest.raises(ValueError, match="shares memory"):
        F.rollout_step(r, abar, 1.0, 1.0, out=abar[1, 2:4])
    with pytest.raises(ValueError, match="GPU"):
        F.rollout_step(r, abar.cpu(), 1.0, 1.0)


# ----------------------------------------------------------------------------- rollout_step
@pytest.mark.parametrize("shape", [(1, 1), (2, 17), (3, 64), (2, 65), (64, 197), (1, 256)],
                         ids=_ids)
@pytest.mark.parametrize("ab", [(0.5, 0.5), (1.0, 1.0), (0.0, 1.0)], ids=_ids)
def test_rollout_step_within_the_summation_bound(dev, shape, ab):
    B, Ls = shape
    alpha, beta = ab
    g = torch.Generator().manual_seed(B + Ls)
    r = torch.rand(B, Ls, generator=g)
    abar = torch.rand(B, Ls, Ls, generator=g) / Ls
    want = alpha * r.double() + beta * torch.einsum("bi,bij->bj", r.double(), abar.double())
    got = F.rollout_step(r.to(dev), abar.to(dev), alpha, beta)
    assert got.shape == (B, Ls) and got.dtype == torch.float32
    err = (got.cpu().double() - want).abs()
    ratio = (err / ((Ls + 3) * U * want)).max().item()
    print(f"rollout_step {shape} {ab}: max err / bound {ratio:.3e}")
    assert ratio <= 1.0
    again = F.rollout_step(r.to(dev), abar.to(dev), alpha, beta)
    assert torch.equal(got, again)
    # abar = 0: alpha r exactly; into the caller's buffer
    out = torch.empty(B, Ls, device=dev)
    z = F.rollout_step(r.to(dev), torch.zeros(B, Ls, Ls, device=dev), alpha, beta, out=out)
    assert z is out and torch.equal(z.cpu(), torch.tensor(alpha, dtype=torch.float32) * r)


# ----------------------------------------------------------------------------- model level
def test_forward_attention_features_are_forward_bit_for_bit(dev):
    for dtype in DTYPES:
        img, _, _ = C.mine(0, dtype, dev)
        x = C.inputs()[0].to(dev)
        with torch.no_grad():
            want = img.backbone(x)
        feats, abar = img.backbone.forward_attention(x)
        assert torch.equal(feats, want) and feats.dtype == dtype
        assert abar.shape == (C.LAYERS, 2, 197, 197) and abar.dtype == torch.float32
        assert not hasattr(img.backbone, "forward_features")


def test_attention_rollout_matches_the_reference_fp32(dev):
    err, out = C.rollout_errors(0, torch.float32, dev)
    want = C.oracle(0)["rollout"]
    print(f"attention_rollout fp32: rel_err {err:.3e}")
    assert err <= 1e-4
    assert out["rollout"].shape == (2, 197) and out["raw"].shape == (2, 14, 14)
    assert out["cam"].shape == (2, 224, 224) and out["attention"].shape == (2, 2, 197, 197)
    assert (out["rollout"].double().sum(-1).cpu() - 1).abs().max().item() <= C.LAYERS * 200 * U
    a_err = (out["attention"].double().cpu() - want["attention"]).abs().max().item()
    assert a_err <= 1e-4 * want["attention"].max().item()
    assert torch.equal(out["raw"].reshape(2, 196), out["rollout"][:, 1:])
    cam = out["cam"]
    assert cam.min().item() >= 0.0 and 0.9 <= cam.max().item() <= 1.0 + 1e-6
    # the last layer alone, another residual: one step from e_0
    img, _, _ = C.mine(0, torch.float32, dev)
    one = C.inputs()[0][:1].to(dev)
    last = mmdx.explain.attention_rollout(img, one, residual=0.25, start_layer=1, out_size=None)
    assert "cam" not in last and "attention" not in last
    w = 0.75 * want["attention"][1, 0, 0]
    w[0] += 0.25
    assert ((last["rollout"][0].double().cpu() - w).abs().max() / w.max()).item() <= 1e-4


def test_transformer_attribution_matches_the_reference_fp32(dev):
    per, lerr, out = C.attribution_errors(0, torch.float32, dev)
    want = C.oracle(0)["attr"]
    assert out["classes"] == C.CLASSES
    assert out["logits"].shape == (2, 13) and out["relevance"].shape == (2, 3, 197)
    assert out["raw"].shape == (2, 3, 14, 14) and out["cam"].shape == (2, 3, 224, 224)
    print(f"transformer_attribution fp32: logits rel_err {lerr:.3e}")
    assert lerr <= 1e-4
    for b, (omc, nr) in enumerate(per):
        print(f"transformer_attribution fp32 sample {b}: 1-cos {omc:.3e}, |norm ratio - 1| "
              f"{nr:.3e}")
        assert omc <= 1e-4
        assert nr <= 1e-3
    rel = out["relevance"].double().cpu()
    assert ((rel - want["relevance"]).abs().max() / want["relevance"].max()).item() <= 1e-4
    assert (out["relevance"][:, :, 0] >= 1).all() and (out["relevance"] >= 0).all()
    assert torch.equal(out["raw"].reshape(2, 3, 196), out["relevance"][:, :, 1:])
    cam = out["cam"]
    assert cam.min().item() >= 0.0 and cam.max().item() <= 1.0 + 1e-6
    # a class subset under no_grad: the same maps in the order asked for
    img, txt, fus = C.mine(0, torch.float32, dev)
    x, ids, mask = (t.to(dev) for t in C.inputs())
    with torch.no_grad():
        sub = mmdx.explain.transformer_attribution(img, txt, fus, x, ids, mask, classes=[11],
                                                   out_size=None)
    assert "cam" not in sub and sub["classes"] == [11]
    tol = 1e-4 * out["raw"].abs().max().item()   # (another row count in every GEMM)
    assert (sub["raw"][:, 0] - out["raw"][:, 2]).abs().max().item() <= tol


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=_ids)
def test_16_bit_explanations_within_4x_of_the_measured_error(dev, dtype):
    m_cos, m_norm, m_logits, m_roll = MEASURED[dtype]
    per, lerr, _ = C.attribution_errors(0, dtype, dev)
    rerr, _ = C.rollout_errors(0, dtype, dev)
    omc, nr = max(p[0] for p in per), max(p[1] for p in per)
    print(f"{dtype} seed 0: worst 1-cos {omc:.3e}, worst |norm ratio - 1| {nr:.3e}, logits "
          f"rel_err {lerr:.3e}, rollout rel_err {rerr:.3e}")
    assert omc <= 4 * m_cos
    assert nr <= 4 * m_norm
    assert lerr <= 4 * m_logits
    assert rerr <= 4 * m_roll


def test_transformer_attribution_has_no_side_effects(dev):
    img, txt, fus = C.mine(0, torch.float32, dev)
    mods = (img, txt, fus)
    x, ids, mask = (t.to(dev) for t in C.inputs())
    tr = mmdx.explain.transformer_attribution
    base = tr(img, txt, fus, x, ids, mask, classes=[0, 5], out_size=None)["raw"]
    assert all(not m.training for top in mods for m in top.modules())
    assert all(p.grad is None for top in mods for p in top.parameters())
    try:
        img.train()
        img.freeze_backbone()
        txt.train()
        fus.train()
        flags = [(m, m.training) for top in mods for m in top.modules()]
        assert any(f for _, f in flags) and not all(f for _, f in flags)
        with torch.no_grad():
            again = tr(img, txt, fus, x, ids, mask, classes=[0, 5], out_size=None)["raw"]
        roll = mmdx.explain.attention_rollout(img, x, out_size=None)["rollout"]
        assert torch.equal(again, base) and torch.isfinite(roll).all()
        assert all(m.training == f for m, f in flags)
        assert all(p.grad is None for top in mods for p in top.parameters())
    finally:
        img.unfreeze_backbone()
        for top in mods:
            top.eval()


# ----------------------------------------------------------------------------- inference()
def test_inference_explain_on_a_vit_bundle(dev):
    from mmdx.inference_pipeline import inference
    img, txt, fus = C.mine(0, torch.float32, dev)
    pil = Image.open(os.path.join(GOLD, "e1.jpg")).convert("RGB")
    with open(os.path.join(GOLD, "patient_details.json")) as f:
        text = json.load(f)["e1.jpg"]
    bundle = {"fusion_model": fus, "image_encoder": img, "text_encoder": txt,
              "class_names": mmdx.DISEASES, "thresholds": [0.5] * 13, "version": 999,
              "t5_tok": None}
    plain = inference(bundle, pil, text, device="cuda")
    out = inference(bundle, pil, text, device="cuda", explain=2)
    assert set(out) == set(plain) | {"heatmaps"}
    for k in plain:                                   # bit-identical floats
        assert out[k] == plain[k], k
    top2 = sorted(mmdx.DISEASES, key=lambda c: -plain["disease_probs"][c])[:2]
    assert list(out["heatmaps"]) == top2
    for name, m in out["heatmaps"].items():
        assert isinstance(m, np.ndarray) and m.shape == (224, 224) and m.dtype == np.float32
        assert np.isfinite(m).all() and m.min() >= 0.0 and m.max() == 1.0, name
        on_image = mmdx.explain.cam_to_image(m, pil.size)
        assert mmdx.explain.overlay(pil, on_image).size == pil.size
    named = inference(bundle, pil, text, device="cuda", explain=[top2[1]])
    assert list(named["heatmaps"]) == [top2[1]]
    assert np.abs(named["heatmaps"][top2[1]] - out["heatmaps"][top2[1]]).max() <= 1e-3
