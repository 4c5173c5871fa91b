"""GPU: the fused text-explanation kernel (mmdx_token_relevance_step) against a float64
reference, and mmdx.explain.text_attribution / text_rollout and inference_explained(explain_text=
...) on a two-layer BERT tower against the float64 CPU references.

Kernel level: the error bound of one step is derived in text_explain_cases (the bound of abar
under the key mask, weighted by the row vector, plus the fused sum's own roundings) and
evaluated elementwise in float64 from the same dtype-rounded inputs; nothing in it is tuned.

Model level (bert_base_config(num_hidden_layers=2, dropout=0) in a TextEncoderTransformer and a
resnet18 image tower, weights shared with the oracle pair, B = 2 with 16 and 9 real tokens,
three classes): fp32 meets the project's criteria, rel_err <= 1e-4 for the rollout rows and the
logits, 1 - cos <= 1e-4 and |norm ratio - 1| <= 1e-3 for the relevance (per sample over its
classes' rows flattened).

fp16 / bf16, measured on an MI355X against the same float64 references over the model seeds 0..3
(profiles/text_explain_parity.txt, written by tools/text_explain_bench.py --parity): the worst
values are the *_MEASURED constants below; the tests assert 4x those, the margin
tests/test_vit_explain_gpu.py uses for the seed-to-seed spread of a 16-bit trunk.
"""
import copy
import os

import pytest
import torch
from PIL import Image

import mmdx
import mmdx.explain
import mmdx.functional as F
import text_explain_cases as C
import vit_explain_cases as V

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = C.U

# (B, Ls, H), the samples' real key counts (None: all real): the tokenizer's geometry with a
# short text; one token; a full key tile; one past it with a single real key; a mask that ends
# on a key-tile edge; three query tiles with lengths on and off the tile edges; the limit
CASES = [((2, 96, 12), (96, 7)), ((1, 1, 1), None), ((1, 16, 1), (16,)), ((2, 17, 2), (17, 1)),
         ((1, 33, 12), (16,)), ((3, 64, 12), (64, 33, 2)), ((1, 256, 2), (255,))]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MODES = ["plain", "weighted"]

# measured on an MI355X (profiles/text_explain_parity.txt): worst over the model seeds 0..3
FP16_MEASURED_1MCOS = 1.324e-13   # seed 0: 1.324e-13
FP16_MEASURED_NORM = 2.969e-7     # seed 0: 1.491e-7
FP16_MEASURED_LOGITS = 9.659e-4   # seed 0: 9.659e-4
FP16_MEASURED_ROLLOUT = 3.179e-5  # seed 0: 3.179e-5
BF16_MEASURED_1MCOS = 1.130e-11   # seed 0: 1.130e-11
BF16_MEASURED_NORM = 2.006e-6     # seed 0: 4.861e-7
BF16_MEASURED_LOGITS = 1.594e-2   # seed 0: 1.594e-2
BF16_MEASURED_ROLLOUT = 2.164e-4  # seed 0: 1.842e-4
MEASURED = {torch.float16: (FP16_MEASURED_1MCOS, FP16_MEASURED_NORM, FP16_MEASURED_LOGITS,
                            FP16_MEASURED_ROLLOUT),
            torch.bfloat16: (BF16_MEASURED_1MCOS, BF16_MEASURED_NORM, BF16_MEASURED_LOGITS,
                             BF16_MEASURED_ROLLOUT)}


def _ids(v):
    if isinstance(v, tuple) and v and isinstance(v[0], tuple):
        return "x".join(str(i) for i in v[0])
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v).split(".")[-1]


def _operands(shape, dtype, seed=0):
    """qkv [B * Ls, 3 * H * 64] ~ N(0, 1), dout and r on a grid of 1/64 (exact in every dtype),
    r of mixed sign; qkv and dout rounded to dtype, r fp32."""
    B, Ls, H = shape
    g = torch.Generator().manual_seed(seed + 7 * sum(shape))
    qkv = torch.randn(B * Ls, 3 * H * 64, generator=g).to(dtype)
    dout = ((torch.randn(B * Ls, H * 64, generator=g) * 16).round() / 64).to(dtype)
    r = (torch.randn(B, Ls, generator=g) * 16).round() / 64
    return qkv, dout, r


def _step(dev, r, qkv, shape, alpha, beta, mask, dout):
    B, Ls, H = shape
    return F.token_relevance_step(r.to(dev), qkv.to(dev), B, Ls, H, 0.125, alpha, beta,
                                  mask=None if mask is None else mask.to(dev),
                                  dout=None if dout is None else dout.to(dev))


def _check(got, ref, bound, what):
    got = got.cpu().double()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = (got - ref).abs()
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, max err / bound {ratio:.3e}")
    assert (err <= bound).all(), f"{what}: the error exceeds the bound {ratio:.3f} times"


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", CASES, ids=_ids)
@pytest.mark.parametrize("mode", MODES)
def test_token_relevance_step_within_the_derived_bound(dev, mode, case, dtype):
    shape, lengths = case
    B, Ls, H = shape
    qkv, dout, r = _operands(shape, dtype)
    dout = dout if mode == "weighted" else None
    mask = None if lengths is None else C.key_mask(B, Ls, lengths)
    for alpha, beta in ((1.0, 1.0), (0.5, 0.5)):
        ref, bound = C.step_reference(r, qkv, dout, mask, B, Ls, H, 0.125, alpha, beta)
        got = _step(dev, r, qkv, shape, alpha, beta, mask, dout)
        assert got.dtype == torch.float32 and got.shape == (B, Ls)
        _check(got, ref, bound, f"token_relevance_step {mode} {shape} {lengths} {dtype}")
        if mask is not None:   # a masked column: alpha r exactly
            want = torch.tensor(alpha, dtype=torch.float32) * r
            assert torch.equal(got.cpu()[mask == 0], want[mask == 0])


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("mode", MODES)
def test_a_mask_with_a_hole_is_no_length(dev, mode, dtype):
    """Keys 5..9 of 20 masked, real keys on both sides: a kernel that reduced the mask to a
    length would count them in or drop the tail."""
    shape = (1, 20, 3)
    qkv, dout, r = _operands(shape, dtype, seed=4)
    dout = dout if mode == "weighted" else None
    mask = torch.ones(1, 20, dtype=torch.long)
    mask[0, 5:10] = 0
    ref, bound = C.step_reference(r, qkv, dout, mask, 1, 20, 3, 0.125, 1.0, 1.0)
    got = _step(dev, r, qkv, shape, 1.0, 1.0, mask, dout)
    _check(got, ref, bound, f"token_relevance_step {mode} hole {dtype}")
    assert torch.equal(got.cpu()[0, 5:10], r[0, 5:10])
    prefix, _ = C.step_reference(r, qkv, dout, C.key_mask(1, 20, (15,)), 1, 20, 3, 0.125, 1.0, 1.0)
    assert ((prefix - ref).abs() > 8 * bound).any()     # (the check can tell the two apart)


@pytest.mark.parametrize("mode", MODES)
def test_a_sample_without_a_real_key_next_to_a_normal_one(dev, mode):
    shape = (2, 40, 4)
    qkv, dout, r = _operands(shape, torch.float16, seed=5)
    dout = dout if mode == "weighted" else None
    mask = C.key_mask(2, 40, (0, 23))
    got = _step(dev, r, qkv, shape, 0.75, 0.5, mask, dout).cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(got[0], torch.tensor(0.75, dtype=torch.float32) * r[0])
    ref, bound = C.step_reference(r, qkv, dout, mask, 2, 40, 4, 0.125, 0.75, 0.5)
    _check(got, ref, bound, f"token_relevance_step {mode} next to an empty sample")
    # the normal sample's row does not know its neighbour
    solo = _step(dev, r[1:], qkv[40:], (1, 40, 4), 0.75, 0.5, mask[1:],
                 None if dout is None else dout[40:])
    assert torch.equal(solo.cpu()[0], got[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_plain_mode_keeps_the_mass(dev, dtype):
    """abar's rows sum to 1 over the real keys, so sum_j r' = (alpha + beta) sum_j r for an r that
    is 0 on the pads; non-negative r, within (Ls + 70) u sum |r|."""
    shape = (3, 64, 12)
    B, Ls, H = shape
    qkv, _, r = _operands(shape, dtype, seed=6)
    mask = C.key_mask(B, Ls, (64, 33, 2))
    r = r.abs() * mask
    for alpha, beta in ((0.5, 0.5), (1.0, 1.0), (0.0, 1.0)):
        got = _step(dev, r, qkv, shape, alpha, beta, mask, None).cpu().double()
        want = (alpha + beta) * r.double().sum(1)
        tol = (Ls + 70) * U * r.double().sum(1)
        assert ((got.sum(1) - want).abs() <= tol).all(), (alpha, beta)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("mode", MODES)
def test_token_relevance_step_with_logits_of_100(dev, mode, dtype):
    """Queries scaled until the unshifted logits reach +-100 (as the sibling kernel's test)."""
    shape = (2, 65, 3)
    B, Ls, H = shape
    qkv, dout, r = _operands(shape, dtype, seed=1)
    t = qkv.double().view(B, Ls, 3, H, 64)
    peak = (0.125 * torch.einsum("bqhd,bkhd->bhqk", t[:, :, 0], t[:, :, 1])).abs().max().item()
    t = t.clone()
    t[:, :, 0] *= 100.0 / peak
    qkv = t.view(B * Ls, -1).to(dtype)
    t = qkv.double().view(B, Ls, 3, H, 64)
    logits = 0.125 * torch.einsum("bqhd,bkhd->bhqk", t[:, :, 0], t[:, :, 1])
    assert logits.abs().max().item() >= 95
    dout = dout if mode == "weighted" else None
    mask = C.key_mask(B, Ls, (65, 40))
    ref, bound = C.step_reference(r, qkv, dout, mask, B, Ls, H, 0.125, 1.0, 1.0)
    got = _step(dev, r, qkv, shape, 1.0, 1.0, mask, dout)
    _check(got, ref, bound, f"token_relevance_step {mode} logits +-100 {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("mode", MODES)
def test_all_ones_mask_agrees_with_the_two_kernel_pair(dev, mode, dtype):
    """alpha = beta = 1 and no pad: rollout_step(r, attention_relevance(...)) computes the same
    thing; the two agree within the sum of their bounds."""
    shape = (2, 96, 12)
    B, Ls, H = shape
    qkv, dout, r = _operands(shape, dtype, seed=2)
    dout = dout if mode == "weighted" else None
    _, mine = C.step_reference(r, qkv, dout, None, B, Ls, H, 0.125, 1.0, 1.0)
    abar, a_err = V.relevance_reference(qkv, dout, B, Ls, H, 0.125)
    mag = r.double().abs() + torch.einsum("bi,bij->bj", r.double().abs(), abar)
    pair = torch.einsum("bi,bij->bj", r.double().abs(), a_err) + (Ls + 3) * U * mag
    qd, dd = qkv.to(dev), None if dout is None else dout.to(dev)
    two = F.rollout_step(r.to(dev), F.attention_relevance(qd, B, Ls, H, 0.125, dout=dd), 1.0, 1.0)
    ones = torch.ones(B, Ls, dtype=torch.long)
    for mask in (None, ones):
        got = _step(dev, r, qkv, shape, 1.0, 1.0, mask, dout)
        diff = (got.double() - two.double()).abs().cpu()
        print(f"fused vs pair {mode} {dtype}: max diff / bound {(diff / (mine + pair)).max():.3e}")
        assert (diff <= mine + pair).all()
    assert torch.equal(_step(dev, r, qkv, shape, 1.0, 1.0, None, dout),
                       _step(dev, r, qkv, shape, 1.0, 1.0, ones, dout))


def test_token_relevance_step_reproducible_and_independent_of_the_batch(dev):
    shape = (3, 64, 12)
    B, Ls, H = shape
    qkv, dout, r = _operands(shape, torch.float16, seed=3)
    mask = C.key_mask(B, Ls, (64, 33, 2))
    for d in (None, dout):
        a = _step(dev, r, qkv, shape, 1.0, 1.0, mask, d)
        b = _step(dev, r, qkv, shape, 1.0, 1.0, mask, d)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        for s in range(B):     # each sample alone (another grid) gives the same bits
            rows = slice(s * Ls, (s + 1) * Ls)
            solo = _step(dev, r[s:s + 1], qkv[rows], (1, Ls, H), 1.0, 1.0, mask[s:s + 1],
                         None if d is None else d[rows])
            assert torch.equal(solo[0], a[s]), s
    # into the caller's buffer
    out = torch.full((B, Ls), -1.0, device=dev)
    got = F.token_relevance_step(r.to(dev), qkv.to(dev), B, Ls, H, 0.125, 1.0, 1.0,
                                 mask=mask.to(dev), out=out)
    assert got is out and torch.equal(out, _step(dev, r, qkv, shape, 1.0, 1.0, mask, None))


def test_calls_of_other_batch_sizes_and_lengths_do_not_disturb_each_other(dev):
    """The tiles of a sample meet through a workspace the wrapper keeps between calls; its
    counters sit in front of the partial rows, and how many there are depends on B."""
    shapes = [(1, 64, 2), (13, 96, 2), (2, 33, 2), (13, 40, 2), (1, 64, 2)]
    first = {}
    for shape in shapes:
        B, Ls, H = shape
        qkv, dout, r = _operands(shape, torch.float32, seed=8)
        mask = C.key_mask(B, Ls, [Ls - (3 * b) % Ls for b in range(B)])
        ref, bound = C.step_reference(r, qkv, dout, mask, B, Ls, H, 0.125, 1.0, 1.0)
        for _ in range(2):
            got = _step(dev, r, qkv, shape, 1.0, 1.0, mask, dout)
            _check(got, ref, bound, f"token_relevance_step after other shapes {shape}")
            assert torch.equal(first.setdefault(shape, got), got)


def test_wrapper_refuses_aliasing_and_other_devices(dev):
    qkv = torch.zeros(2 * 5, 3 * 2 * 64, device=dev)
    r = torch.zeros(2, 5, device=dev)
    with pytest.raises(ValueError, match="shares memory"):
        F.token_relevance_step(r, qkv, 2, 5, 2, 0.125, 1.0, 1.0, out=r)
    with pytest.raises(ValueError, match="shares memory"):
        F.token_relevance_step(r, qkv, 2, 5, 2, 0.125, 1.0, 1.0, out=qkv.view(-1)[:10].view(2, 5))
    with pytest.raises(ValueError, match="GPU"):
        F.token_relevance_step(r, qkv, 2, 5, 2, 0.125, 1.0, 1.0,
                               mask=torch.ones(2, 5, dtype=torch.long))


# ----------------------------------------------------------------------------- model level
def test_forward_layers_is_forward_bit_for_bit(dev):
    _, ids, mask = (t.to(dev) for t in C.inputs())
    for dtype in DTYPES:
        _, txt, _ = C.mine(0, dtype, dev)
        with torch.no_grad():
            want = txt.encoder(input_ids=ids, attention_mask=mask).last_hidden_state
        h, c, kept = txt.encoder.forward_layers(ids, mask, None, False)
        assert torch.equal(h, want) and h.dtype == dtype and not h.requires_grad
        assert kept == [] and (c.B, c.Ls, c.H, c.p, c.pa) == (2, 16, 12, 0.0, 0.0)
        # keep=True: what bert_bwd needs of every layer (a 16-bit tower then runs the attention
        # forward that saves the row log-sum-exp: the same values, not the same bits)
        h2, _, kept = txt.encoder.forward_layers(ids, mask, None, True)
        assert len(kept) == C.LAYERS and all("qkv" in s for s in kept)
        tol = 1e-6 if dtype == torch.float32 else 4e-2
        assert (h2.float() - want.float()).abs().max().item() <= tol * want.float().abs().max()


def test_text_attribution_matches_the_reference_fp32(dev):
    per, lerr, out = C.attribution_errors(0, torch.float32, dev)
    want = C.oracle(0)["attr"]
    assert out["classes"] == C.CLASSES
    assert out["logits"].shape == (2, 13) and out["relevance"].shape == (2, 3, 16)
    assert out["relevance"].dtype == torch.float32
    print(f"text_attribution fp32: logits rel_err {lerr:.3e}")
    assert lerr <= 1e-4
    for b, (omc, nr) in enumerate(per):
        print(f"text_attribution fp32 sample {b}: 1-cos {omc:.3e}, |norm ratio - 1| {nr:.3e}")
        assert omc <= 1e-4
        assert nr <= 1e-3
    rel = out["relevance"].double().cpu()
    assert ((rel - want["relevance"]).abs().max() / want["relevance"].max()).item() <= 1e-4
    _, _, mask = C.inputs()
    # what the layers added to the start vector mask / n (a randomly initialised tower: little)
    start = (mask.double() / mask.sum(1, keepdim=True))[:, None, :]
    omc = 1 - C.cosine(rel - start, want["relevance"] - start)
    print(f"text_attribution fp32: above the start vector {(rel - start).abs().max():.3e} (start "
          f"{start.max():.3e}), 1-cos of that part {omc:.3e}")
    pads = (mask == 0)[:, None, :].expand(2, 3, 16)
    assert pads.any() and not out["relevance"].cpu()[pads].any()       # exactly 0
    assert (out["relevance"].cpu()[~pads] > 0).all()
    # a class subset under no_grad, the last layer alone: the same rows in the order asked for
    img, txt, fus = C.mine(0, torch.float32, dev)
    x, ids, mask = (t.to(dev) for t in C.inputs())
    with torch.no_grad():
        sub = mmdx.explain.text_attribution(img, txt, fus, x, ids, mask, classes=[11])
    assert sub["classes"] == [11]
    tol = 1e-4 * out["relevance"].abs().max().item()   # (another row count in every GEMM)
    assert (sub["relevance"][:, 0] - out["relevance"][:, 2]).abs().max().item() <= tol


def test_text_rollout_matches_the_reference_fp32(dev):
    err, out = C.rollout_errors(0, torch.float32, dev)
    print(f"text_rollout fp32: rel_err {err:.3e}")
    assert err <= 1e-4
    roll = out["rollout"]
    assert roll.shape == (2, 16) and roll.dtype == torch.float32
    assert (roll.double().sum(-1).cpu() - 1).abs().max().item() <= C.LAYERS * 100 * U
    _, _, mask = C.inputs()
    assert not roll.cpu()[mask == 0].any()
    # the last layer alone, another residual: one step from mask / n
    _, txt, _ = C.mine(0, torch.float32, dev)
    _, ids, m = (t.to(dev) for t in C.inputs())
    last = mmdx.explain.text_rollout(txt, ids, m, residual=0.25, start_layer=1)["rollout"]
    att = C.oracle(0)["rollout"]["attention"][1]
    start = mask.double() / mask.sum(1, keepdim=True)
    w = 0.25 * start + 0.75 * torch.einsum("bi,bij->bj", start, att)
    assert ((last.double().cpu() - w).abs().max() / w.max()).item() <= 1e-4


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


def test_text_explanations_have_no_side_effects(dev):
    img, txt, fus = C.mine(0, torch.float32, dev)
    mods = (img, txt, fus)
    x, ids, mask = (t.to(dev) for t in C.inputs())
    ta = mmdx.explain.text_attribution
    base = ta(img, txt, fus, x, ids, mask, classes=[0, 5])["relevance"]
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
            again = ta(img, txt, fus, x, ids, mask, classes=[0, 5])["relevance"]
        roll = mmdx.explain.text_rollout(txt, ids, mask)["rollout"]
        assert torch.equal(again, base) and torch.isfinite(roll).all()
        assert all(m.training == f for m, f in flags)
        assert all(p.grad is None for top in mods for p in top.parameters())
    finally:
        img.unfreeze_backbone()
        for top in mods:
            top.eval()
    empty = mask.clone()
    empty[1] = 0
    with pytest.raises(ValueError, match="no real token"):
        ta(img, txt, fus, x, ids, empty, classes=[0])
    with pytest.raises(ValueError, match="no real token"):
        mmdx.explain.text_rollout(txt, ids, empty)


# ----------------------------------------------------------------------------- inference()
def _saved_bundle(dev, tmp_path, txt):
    from mmdx.inference_pipeline import load_model_bundle, save_model_bundle
    img, _, fus = C.mine(0, torch.float32, dev)
    arts = {"class_names": list(mmdx.DISEASES), "thresholds": [0.5] * 13}
    path = save_model_bundle(fus, img, txt, str(tmp_path), timestamped_copy=False,
                             artifacts=arts)
    return load_model_bundle(path, with_report_head=False)


def test_inference_explain_text_on_a_saved_bert_bundle(dev, tmp_path):
    import re
    from mmdx.inference_pipeline import inference, inference_explained
    _, txt, _ = C.mine(0, torch.float32, dev)
    bundle = _saved_bundle(dev, tmp_path, txt)
    assert len(bundle["text_encoder"].encoder.encoder.layer) == C.LAYERS
    pil = Image.open(os.path.join(GOLD, "e1.jpg")).convert("RGB")
    text = "44 year old female PA view , hypertension , cough"
    plain = inference(bundle, pil, text)
    again = inference_explained(bundle, pil, text, explain_text=None)
    assert again == plain and "token_relevance" not in plain
    out = inference_explained(bundle, pil, text, explain_text=2)
    assert set(out) == set(plain) | {"token_relevance"}
    for k in plain:                                   # bit-identical floats
        assert out[k] == plain[k], k
    top2 = sorted(mmdx.DISEASES, key=lambda c: -plain["disease_probs"][c])[:2]
    assert list(out["token_relevance"]) == top2
    words = re.findall(r"\w+|[^\w\s]", text.lower())      # (the hash tokenizer: whole words)
    # the float64 reference of the same call
    tok = mmdx.tokenize_patient_details([text], max_len=96)
    x = mmdx.preprocess_batch([pil], dev)
    ref = C.oracle(0)["ref"]
    m64 = copy.deepcopy(ref).double()
    with torch.no_grad():
        z_img = m64.image(x.double().cpu())["embeddings"]
    picked = [mmdx.DISEASES.index(c) for c in top2]
    want = mmdx.explain.text_attribution_reference(
        ref.text.state_dict(), tok["input_ids"], tok["attention_mask"],
        lambda pooled: m64.fusion(z_img, m64.text.proj(pooled))["disease_logits"],
        classes=picked)["relevance"][0]
    for i, name in enumerate(top2):
        item = out["token_relevance"][name]
        assert item["tokens"] == words and len(item["scores"]) == len(words)
        assert all(0.0 <= v <= 1.0 for v in item["scores"]) and max(item["scores"]) == 1.0
        best = max(range(len(words)), key=lambda j: item["scores"][j])
        assert best == int(want[i, 1:1 + len(words)].argmax()), name
    both = inference_explained(bundle, pil, text, explain=1, explain_text=[top2[1]])
    assert set(both) == set(plain) | {"heatmaps", "token_relevance"}
    assert list(both["token_relevance"]) == [top2[1]]


def test_inference_explain_text_refuses_an_embed_mean_tower(dev, tmp_path):
    from mmdx.inference_pipeline import inference_explained
    txt = mmdx.TextEncoderTransformer("embed-mean", 512, 13).to(dev).eval()
    bundle = _saved_bundle(dev, tmp_path, txt)
    pil = Image.open(os.path.join(GOLD, "e1.jpg")).convert("RGB")
    with pytest.raises(NotImplementedError, match="BERT"):
        inference_explained(bundle, pil, "44 year old female PA view", explain_text=True)
