"""What tests/test_text_explain_gpu.py, tests/test_text_explain_cpu.py and
tools/text_explain_bench.py share: the float64 reference and the error bound of one
token_relevance_step, and the two-layer BERT model pair (oracle weights -> mmdx modules) with its
float64 explanations.

One step computes r'[j] = alpha r[j] + beta sum_i r[i] abar[i][j] with abar recomputed under the
key mask.  The bound (u = 2^-24, evaluated elementwise in float64 from the same dtype-rounded
inputs the kernel reads) has three parts:
- the bound of abar[i][j] is vit_explain_cases.relevance_reference's, with the softmax taken
  over the real keys: a logit errs by e_ij = 65 u scale sum_d |q_d k_d|;
  |dP_ij| <= (2 max_{j real} e_ij + (n_real + 64) u) P_ij + 4 u (the row sum now has n_real
  terms); the weighted form and the head mean as there.  A masked key has P = 0 exactly in the
  kernel and in the reference: its bound is 0, and so is every entry of a sample without a real
  key;
- these enter the sum weighted by the row vector: |beta| sum_i |r_i| bound_ij;
- the fused sum itself: Ls products accumulated in some fixed order (at most Ls - 1 additions on
  the path of any term), the scaling by beta and the final fused multiply-add round at most
  Ls + 3 times, each relative to a partial sum of absolute values:
  (Ls + 3) u (|alpha r_j| + |beta| sum_i |r_i| abar_ij).
"""
import copy

import torch

import mmdx
from oracle import ref_cpu as R
from parity_util import synth_batch

U = 2.0 ** -24
CLASSES = [5, 0, 11]      # three classes, not in index order
LAYERS = 2
LENGTHS = (16, 9)         # real tokens of the two samples, Ls = 16


def key_mask(B, Ls, lengths):
    """int64 [B, Ls]: sample b's first lengths[b] keys are real (None: all)."""
    mask = torch.ones(B, Ls, dtype=torch.long)
    for b, n in enumerate(lengths or ()):
        mask[b, n:] = 0
    return mask


def abar_reference(qkv, dout, mask, B, Ls, H, scale):
    """(abar [B, Ls, Ls], its error bound) in float64 on the CPU under the key mask [B, Ls]
    (None: all real); dout=None: the plain mode."""
    t = qkv.detach().cpu().double().reshape(B, Ls, 3, H, 64)
    q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))          # [B, H, Ls, 64]
    real = torch.ones(B, Ls, dtype=torch.bool) if mask is None else mask.cpu() != 0
    keys = real[:, None, None, :]                                         # [B, 1, 1, Ls]
    some = real.any(1)[:, None, None, None]
    logits = (scale * (q @ k.transpose(-1, -2))).masked_fill(~keys, -float("inf"))
    logits = torch.where(some, logits, torch.zeros_like(logits))   # (no real key: P = 0 below)
    P = torch.softmax(logits, dim=-1) * (keys & some)
    e = 65 * U * scale * (q.abs() @ k.abs().transpose(-1, -2)) * keys
    n_real = real.sum(1).double()[:, None, None, None]
    p_err = ((2 * e.amax(-1, keepdim=True) + (n_real + 64) * U) * P + 4 * U) * (keys & some)
    if dout is None:
        ref = P.mean(1)
        return ref, p_err.mean(1) + (H + 1) * U * ref
    d = dout.detach().cpu().double().reshape(B, Ls, H, 64).permute(0, 2, 1, 3)
    dP = d @ v.transpose(-1, -2)
    dp_err = 65 * U * (d.abs() @ v.abs().transpose(-1, -2))
    ref = (P * dP).clamp(min=0).mean(1)
    err = p_err * dP.abs() + (P + p_err) * dp_err * (keys & some) + U * (P * dP).abs()
    return ref, err.mean(1) + (H + 1) * U * ref


def step_reference(r, qkv, dout, mask, B, Ls, H, scale, alpha, beta):
    """(r' [B, Ls], its error bound) of one token_relevance_step in float64 on the CPU."""
    abar, a_err = abar_reference(qkv, dout, mask, B, Ls, H, scale)
    r = r.detach().cpu().double()
    moved = torch.einsum("bi,bij->bj", r, abar)
    ref = alpha * r + beta * moved
    mag = abs(alpha) * r.abs() + abs(beta) * torch.einsum("bi,bij->bj", r.abs(), abar)
    bound = abs(beta) * torch.einsum("bi,bij->bj", r.abs(), a_err) + (Ls + 3) * U * mag
    return ref, bound


# ----------------------------------------------------------------------------- model level
_ORACLE = {}
_MINE = {}


def inputs():
    """B = 2, Ls = 16, texts of LENGTHS real tokens ([CLS] ... [SEP], then [PAD] = 0)."""
    x, ids, _, _ = synth_batch(2, 16, hw=64)
    mask = key_mask(2, 16, LENGTHS)
    for b, n in enumerate(LENGTHS):
        ids[b, n - 1] = 102
        ids[b, n:] = 0
    return x, ids, mask


def oracle(seed=0):
    """The CPU oracle of one model seed: RefMultimodal(resnet18, two-layer transformers BERT)
    (fp32 masters) and the float64 explanations of inputs(): {"rollout":
    text_rollout_reference, "attr": text_attribution_reference for CLASSES}.  Computed once."""
    if seed not in _ORACLE:
        from mmdx.explain import text_attribution_reference, text_rollout_reference
        torch.manual_seed(seed)
        ref = R.RefMultimodal("resnet18", "bert-base-uncased", bert_layers=LAYERS,
                              dropout=0.0).eval()
        x, ids, mask = inputs()
        m64 = copy.deepcopy(ref).double()
        with torch.no_grad():
            z_img = m64.image(x.double())["embeddings"]

        def head(pooled):
            return m64.fusion(z_img, m64.text.proj(pooled))["disease_logits"]

        sd = ref.text.state_dict()
        _ORACLE[seed] = dict(ref=ref, rollout=text_rollout_reference(sd, ids, mask),
                             attr=text_attribution_reference(sd, ids, mask, head,
                                                             classes=CLASSES))
    return _ORACLE[seed]


def mine(seed, dtype, dev):
    """The mmdx modules with the oracle's weights, on `dev`, eval mode, the text tower computing
    in dtype; the image tower too, but for fp16, which a ResNet trunk has no kernels for: it
    stays in fp32 then (text_attribution casts its embedding)."""
    ref = oracle(seed)["ref"]
    if seed not in _MINE:
        img = mmdx.ImageEncoderCNN("resnet18", 1024, 13)
        txt = mmdx.TextEncoderTransformer(f"bert-base-uncased@{LAYERS}", 512, 13)
        fus = mmdx.FusionTransformerModel(1024, 512, 1024, 13, dropout=0.0)
        img.load_state_dict(ref.image.state_dict())
        txt.load_state_dict(ref.text.state_dict(), strict=True)
        fus.load_state_dict(ref.fusion.state_dict())
        _MINE[seed] = tuple(m.to(dev).eval() for m in (img, txt, fus))
    img, txt, fus = _MINE[seed]
    img.set_compute_dtype(torch.float32 if dtype == torch.float16 else dtype)
    txt.set_compute_dtype(dtype)
    return img, txt, fus


def cosine(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm()).clamp(min=1e-300)).item()


def attribution_errors(seed, dtype, dev):
    """text_attribution of the mmdx pair against the float64 oracle: per sample, over its
    classes' token rows flattened, (1 - cos, |norm ratio - 1|); and the logits' rel_err.
    -> ([(1 - cos, nr)] per sample, logits rel_err, the function's output)."""
    from mmdx.explain import text_attribution
    img, txt, fus = mine(seed, dtype, dev)
    x, ids, mask = inputs()
    out = text_attribution(img, txt, fus, x.to(dev), ids.to(dev), mask.to(dev), classes=CLASSES)
    want = oracle(seed)["attr"]
    rel = out["relevance"].double().cpu()
    per = []
    for b in range(rel.shape[0]):
        nr = (rel[b].norm() / want["relevance"][b].norm().clamp(min=1e-300)).item()
        per.append((1.0 - cosine(rel[b], want["relevance"][b]), abs(nr - 1.0)))
    wl = want["logits"]
    lerr = ((out["logits"].double().cpu() - wl).abs().max() / wl.abs().max()).item()
    return per, lerr, out


def rollout_errors(seed, dtype, dev):
    """text_rollout against text_rollout_reference: (rel_err of the rows, the output)."""
    from mmdx.explain import text_rollout
    _, txt, _ = mine(seed, dtype, dev)
    _, ids, mask = inputs()
    out = text_rollout(txt, ids.to(dev), mask.to(dev))
    want = oracle(seed)["rollout"]["rollout"]
    err = ((out["rollout"].double().cpu() - want).abs().max() / want.abs().max()).item()
    return err, out
