"""What tests/test_vit_explain_gpu.py and tools/vit_explain_bench.py --parity share: the fp64
reference and error bound of the attention-relevance kernel, and the two-layer ViT model pair
(oracle weights -> mmdx modules) with its float64 explanations.

The bound (u = 2^-24, evaluated elementwise in float64; the reference is computed from the same
dtype-rounded inputs the kernel reads):
- an fp32 dot of 64 products in any order, then the scale, errs by <= 65 u sum_d |x_d y_d|, so a
  logit errs by e_ij = 65 u scale sum_d |q_d k_d|;
- |dP_ij| <= (2 max_j e_ij + (S + 64) u) P_ij + 4 u: the logit's own error and the row
  maximum's, the row sum of S terms, the rounding of the exponential's argument for |x| <= 16,
  the exponential and the division; 4 u is the floor for what lies below (P < 4 u means
  |x| > 15.2; there a relative error of a few hundred u is an absolute one far below u);
- weighted: |d(dP)_ij| <= 65 u sum_d |dO_d v_d| and
  |d relu(P dP)| <= |dP_err| |dP| + (P + |dP_err|) |d(dP)| + u |P dP| (ReLU is 1-Lipschitz);
- the head mean (H - 1 additions, one division) adds (H + 1) u of the result.
"""
import copy

import torch

import mmdx
from oracle import ref_cpu as R
from parity_util import synth_batch

U = 2.0 ** -24
CLASSES = [5, 0, 11]      # three classes, not in index order
LAYERS = 2


def relevance_reference(qkv, dout, B, Ls, H, scale):
    """(abar [B, Ls, Ls], its error bound) in float64 on the CPU; dout=None: the plain mode."""
    t = qkv.detach().cpu().double().reshape(B, Ls, 3, H, 64)
    q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))          # [B, H, Ls, 64]
    P = torch.softmax(scale * (q @ k.transpose(-1, -2)), dim=-1)
    e = 65 * U * scale * (q.abs() @ k.abs().transpose(-1, -2))
    p_err = (2 * e.amax(-1, keepdim=True) + (Ls + 64) * U) * P + 4 * U
    if dout is None:
        ref = P.mean(1)
        return ref, p_err.mean(1) + (H + 1) * U * ref
    d = dout.detach().cpu().double().reshape(B, Ls, H, 64).permute(0, 2, 1, 3)
    dP = d @ v.transpose(-1, -2)
    dp_err = 65 * U * (d.abs() @ v.abs().transpose(-1, -2))
    ref = (P * dP).clamp(min=0).mean(1)
    err = p_err * dP.abs() + (P + p_err) * dp_err + U * (P * dP).abs()
    return ref, err.mean(1) + (H + 1) * U * ref


# ----------------------------------------------------------------------------- model level
_ORACLE = {}
_MINE = {}


def inputs():
    x, ids, mask, _ = synth_batch(2, 16, hw=224)
    return x, ids, mask


def oracle(seed=0):
    """The CPU oracle pair of one model seed: a two-layer RefVitTrunk, proj, the embed-mean text
    tower and the fusion head (fp32 masters), and the float64 explanations of inputs():
    {"rollout": rollout_reference, "attr": attribution_reference for CLASSES}.  Computed once."""
    if seed not in _ORACLE:
        from mmdx.explain import attribution_reference, rollout_reference
        torch.manual_seed(seed)
        trunk = R.RefVitTrunk(layers=LAYERS)
        with torch.no_grad():
            trunk.class_token.normal_(std=0.02)
        proj = torch.nn.Linear(768, 1024)
        text = R.RefTextEncoderTransformer("embed-mean", 512, 13, bert_layers=2, dropout=0.0)
        fusion = R.RefFusion(1024, 512, 1024, 13, 0.0)
        mods = dict(trunk=trunk.eval(), proj=proj.eval(), text=text.eval(), fusion=fusion.eval())
        x, ids, mask = inputs()
        p64, t64, f64 = (copy.deepcopy(m).double() for m in (proj, text, fusion))
        with torch.no_grad():
            z_txt = t64(input_ids=ids, attention_mask=mask)["embeddings"]

        def head(feats):
            return f64(p64(feats), z_txt)["disease_logits"]

        sd = trunk.state_dict()
        mods["rollout"] = rollout_reference(sd, x)
        mods["attr"] = attribution_reference(sd, x, head, classes=CLASSES)
        _ORACLE[seed] = mods
    return _ORACLE[seed]


def mine(seed, dtype, dev):
    """The mmdx modules with the oracle's weights: an ImageEncoderCNN("vit_b_16") whose backbone
    is a two-layer VitTrunk, the text tower, the fusion head; on `dev`, eval mode."""
    from mmdx.vit import VitTrunk
    o = oracle(seed)
    if seed not in _MINE:     # (the 12-layer trunk the constructor builds is replaced)
        img = mmdx.ImageEncoderCNN("vit_b_16", 1024, 13)
        img.backbone = VitTrunk(layers=LAYERS)
        img.backbone.load_state_dict(o["trunk"].state_dict())
        img.proj.load_state_dict(o["proj"].state_dict())
        fus = mmdx.FusionTransformerModel(1024, 512, 1024, 13, dropout=0.0)
        fus.load_state_dict(o["fusion"].state_dict())
        _MINE[seed] = (img.to(dev).eval(), fus.to(dev).eval())
    img, fus = _MINE[seed]
    img.set_compute_dtype(dtype)
    txt = mmdx.TextEncoderTransformer("embed-mean", 512, 13, compute_dtype=dtype)
    txt.load_state_dict(o["text"].state_dict(), strict=True)
    return img, txt.to(dev).eval(), fus


def cosine(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm()).clamp(min=1e-300)).item()


def attribution_errors(seed, dtype, dev):
    """transformer_attribution of the mmdx pair against the float64 oracle maps: per sample,
    over its classes' patch maps flattened, (1 - cos, |norm ratio - 1|); and the logits'
    rel_err.  -> ([(1 - cos, nr)] per sample, logits rel_err, the function's output)."""
    from mmdx.explain import transformer_attribution
    img, txt, fus = mine(seed, dtype, dev)
    x, ids, mask = inputs()
    out = transformer_attribution(img, txt, fus, x.to(dev), ids.to(dev), mask.to(dev),
                                  classes=CLASSES)
    want = oracle(seed)["attr"]
    raw = out["raw"].double().cpu()
    per = []
    for b in range(raw.shape[0]):
        nr = (raw[b].norm() / want["raw"][b].norm().clamp(min=1e-300)).item()
        per.append((1.0 - cosine(raw[b], want["raw"][b]), abs(nr - 1.0)))
    wl = want["logits"]
    lerr = ((out["logits"].double().cpu() - wl).abs().max() / wl.abs().max()).item()
    return per, lerr, out


def rollout_errors(seed, dtype, dev):
    """attention_rollout against rollout_reference: (rel_err of the rollout rows, the output)."""
    from mmdx.explain import attention_rollout
    img, _, _ = mine(seed, dtype, dev)
    x, _, _ = inputs()
    out = attention_rollout(img, x.to(dev), return_attention=True)
    want = oracle(seed)["rollout"]["rollout"]
    err = ((out["rollout"].double().cpu() - want).abs().max() / want.abs().max()).item()
    return err, out
