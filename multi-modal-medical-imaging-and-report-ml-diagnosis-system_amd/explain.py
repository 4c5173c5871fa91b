"""Grad-CAM heatmaps of the disease head: where on the radiograph the image tower found its
evidence for a class.

Between the trunk's last conv activation A [B, H, W, K] and the disease logits there is only
the global average pool, `proj`, the fusion MLP and `disease_head`, so

    d logit_c / d A[b, h, w, k] = g[b, c, k] / (H W),      g = d logit_c / d feats,

the same for every pixel: no trunk backward is needed.  With eval mode everywhere
(running-statistics BatchNorm, dropout off) and the LOGIT (before the sigmoid) as the target:

    alpha[b, c, k] = g[b, c, k] / (H W)
    raw[b, c, h, w] = max(0, sum_k alpha[b, c, k] A[b, h, w, k])            (functional.cam_raw)
    cam[b, c]       = bilinear(raw[b, c] / max_hw raw[b, c]) -> [Ho, Wo]    (functional.cam_resize)

`g` runs through the heads' own autograd Functions (Linear, fusion_linear, LayerNorm): one
pass over B * Cs rows and one torch.autograd.grad with one-hot grad_outputs.  Only ResNet
trunks have such a conv stage; on a vit_b_16 encoder grad_cam raises NotImplementedError.

The ViT tower is explained from its attention probabilities instead.  With S = 197 tokens (the
class token, then 14 x 14 patches), P_h = softmax(Q_h K_h^T / 8) of head h in layer l and
dP_h = dO_h V_h^T = d logit_c / d P_h (dO: the gradient at the attention core's output):

    plain     abar_l = mean_h P_h                      rows sum to 1
    weighted  abar_l = mean_h relu(P_h * dP_h)         per (sample, class)

    attention_rollout        R = A_{Lyr-1} ... A_s,  A_l = a I + (1 - a) abar_l   (Abnar & Zuidema)
    transformer_attribution  R = (I + abar_{Lyr-1}) ... (I + abar_s)           (Chefer, Gur & Wolf)

Only the class-token row of R is wanted: r = e_0, then r <- alpha r + beta (r abar_l) from the
last layer down to s (functional.rollout_step), with (alpha, beta) = (a, 1 - a) or (1, 1).  The
attention core stores no P; functional.attention_relevance recomputes abar_l from the block's
qkv buffer.  The weighted form meets each layer's (qkv, dO) pair where the block backward
(xlayers.vit_bwd) hands it to the attention backward.  r[1:] as [14, 14] is the map.
`rollout_reference` / `attribution_reference` restate all of it in float64 torch on the CPU with
explicit attention matrices: the tests' yardstick.

The BERT text tower gets the same two explanations per token (text_rollout, text_attribution).
Two things differ.  Its attention has a key mask: P_h is the softmax over the REAL keys, a pad's
probability is exactly 0.  And it pools by the mean over the real tokens, not by a class token,
so the recursion starts at r = mask / n_real and yields (1 / n) sum_{i real} R[i, :].  One
launch per layer (functional.token_relevance_step) recomputes P under the mask and applies
r <- alpha r + beta (r abar_l) without ever writing abar_l.  `text_rollout_reference` /
`text_attribution_reference` are the float64 yardsticks; `merge_wordpieces` folds "##" pieces
back into words for display.

`cam_to_image` and `overlay` are the host half (numpy / PIL): put a 224 x 224 map back on the
original radiograph and blend it in.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import functional as F
from .training_pipeline import IMG_SIZE

__all__ = ["grad_cam", "attention_rollout", "transformer_attribution", "rollout_reference",
           "attribution_reference", "select_classes", "cam_to_image", "overlay",
           "text_attribution", "text_rollout", "text_attribution_reference",
           "text_rollout_reference", "merge_wordpieces"]

RESIZE_SIZE = 256  # the shorter side before the centre crop (image_transfom_into_tensor)
MAX_ATTRIBUTION_ROWS = 64  # B * Cs of one transformer_attribution call


def _backbone_name(image_encoder):
    trunk = getattr(image_encoder, "backbone", None)
    return getattr(image_encoder, "backbone_name", type(trunk).__name__)


def _trunk_of(image_encoder):
    trunk = getattr(image_encoder, "backbone", None)
    if not hasattr(trunk, "forward_features"):
        raise NotImplementedError(
            f"Grad-CAM needs a convolutional last stage: the {_backbone_name(image_encoder)} "
            f"image encoder has none (ResNet backbones only; a ViT encoder is explained by "
            f"attention_rollout / transformer_attribution)")
    return trunk


def _vit_trunk_of(image_encoder):
    trunk = getattr(image_encoder, "backbone", None)
    if not hasattr(trunk, "forward_attention"):
        raise NotImplementedError(
            f"attention rollout and transformer attribution need a transformer image tower: "
            f"the {_backbone_name(image_encoder)} image encoder has none (vit_b_16 only; a "
            f"ResNet encoder is explained by grad_cam)")
    return trunk


def grad_cam(image_encoder, text_encoder, fusion_model, images, input_ids, attention_mask,
             token_type_ids=None, classes=None, out_size=(IMG_SIZE, IMG_SIZE), normalize=True):
    """Grad-CAM maps of the disease logits at layer4 for a batch.

    images: what the image encoder takes ([B, 3, H, W] fp32); input_ids / attention_mask /
    token_type_ids: what the text encoder takes.  classes: class indices (default: all).
    Returns {"logits": [B, n_disease] fp32, "classes": the indices, "raw": [B, Cs, H, W] fp32
    (ReLU'd, unnormalised), "cam": [B, Cs, Ho, Wo] fp32}; out_size=None leaves "cam" out.

    Runs in eval mode whatever the modules' mode (restored on return), works under
    torch.no_grad(), and leaves every parameter's .grad untouched."""
    trunk = _trunk_of(image_encoder)
    n_cls = fusion_model.disease_head.out_features
    classes = list(range(n_cls)) if classes is None else [int(c) for c in classes]
    if not classes or any(c < 0 or c >= n_cls for c in classes):
        raise ValueError(f"classes must be indices in [0, {n_cls}), got {classes}")
    Cs = len(classes)
    mods = (image_encoder, text_encoder, fusion_model)
    was = [(m, m.training) for top in mods for m in top.modules()]
    try:
        for top in mods:
            top.eval()
        with torch.no_grad():
            feats, fmap = trunk.forward_features(images)
            z_txt = text_encoder(input_ids=input_ids, attention_mask=attention_mask,
                                 token_type_ids=token_type_ids)["embeddings"]
        B, H, W, K = fmap.shape
        with torch.enable_grad():
            # row b * Cs + j carries sample b and is differentiated for classes[j]
            f_rep = feats.repeat_interleave(Cs, dim=0).requires_grad_(True)
            t_rep = z_txt.detach().repeat_interleave(Cs, dim=0)
            logits = fusion_model(image_encoder.proj(f_rep), t_rep)["disease_logits"]
            pick = torch.zeros_like(logits)
            pick[torch.arange(B * Cs, device=logits.device),
                 torch.tensor(classes, device=logits.device).repeat(B)] = 1.0
            (g,) = torch.autograd.grad(logits, f_rep, grad_outputs=pick)
        with torch.no_grad():
            alpha = (g.float() / float(H * W)).view(B, Cs, K).contiguous()
            raw = F.cam_raw(fmap, alpha)
            out = {"logits": logits.detach().view(B, Cs, n_cls)[:, 0].float().contiguous(),
                   "classes": classes, "raw": raw}
            if out_size is not None:
                out["cam"] = F.cam_resize(raw, out_size, normalize)
        return out
    finally:
        for m, flag in was:
            m.training = flag


# ----------------------------------------------------------------------------- ViT explanations
def _check_vit_call(trunk, images, start_layer, rows):
    layers = len(trunk.encoder.layers)
    if not torch.is_tensor(images) or images.dim() != 4 or \
            tuple(images.shape[1:]) != (3, IMG_SIZE, IMG_SIZE) or images.shape[0] < 1:
        raise ValueError(f"the ViT tower takes images [B, 3, {IMG_SIZE}, {IMG_SIZE}], got "
                         f"{tuple(images.shape) if torch.is_tensor(images) else type(images)}")
    if isinstance(start_layer, bool) or not isinstance(start_layer, int) or \
            not 0 <= start_layer < layers:
        raise ValueError(f"start_layer must be an int in [0, {layers}), got {start_layer!r}")
    if images.shape[0] * rows > MAX_ATTRIBUTION_ROWS:
        raise ValueError(f"B * Cs = {images.shape[0]} * {rows} > {MAX_ATTRIBUTION_ROWS}: split "
                         f"the batch or the classes")
    return layers


def _token_maps(r, lead, out_size, normalize, out):
    """r [..., S] -> out["raw"] [..., g, g] (the patch tokens) and out["cam"]."""
    g = math.isqrt(r.shape[-1] - 1)
    out["raw"] = r[:, 1:].reshape(*lead, g, g).contiguous()
    if out_size is not None:
        out["cam"] = F.cam_resize(out["raw"], out_size, normalize)
    return out


def attention_rollout(image_encoder, images, residual=0.5, start_layer=0,
                      out_size=(IMG_SIZE, IMG_SIZE), normalize=True, return_attention=False):
    """Attention rollout (Abnar & Zuidema 2020) of a vit_b_16 image encoder: where the class
    token's information came from.  Class-agnostic, forward only, no text tower, no heads.

    images [B, 3, 224, 224] fp32.  residual a in [0, 1): the identity's share of every layer,
    A_l = a I + (1 - a) mean_h P_h.  The layers start_layer .. last are multiplied up.
    Returns {"rollout": [B, S] fp32 (the class-token row of the product; sums to 1),
    "raw": [B, 14, 14] (its patch part), "cam": [B, Ho, Wo] (raw / max, bilinear;
    out_size=None leaves it out)} and, return_attention=True, "attention": [layers, B, S, S],
    the head-averaged maps.  Eval mode whatever the encoder's mode (restored on return); a
    ResNet encoder raises NotImplementedError."""
    trunk = _vit_trunk_of(image_encoder)
    layers = _check_vit_call(trunk, images, start_layer, 1)
    a = float(residual)
    if not 0.0 <= a < 1.0:
        raise ValueError(f"residual must be in [0, 1), got {residual!r}")
    was = [(m, m.training) for m in image_encoder.modules()]
    try:
        image_encoder.eval()
        with torch.no_grad():
            _, abar = trunk.forward_attention(images)
            B, S = abar.shape[1], abar.shape[2]
            r = torch.zeros((B, S), dtype=torch.float32, device=abar.device)
            r[:, 0] = 1.0
            for li in range(layers - 1, start_layer - 1, -1):
                r = F.rollout_step(r, abar[li], a, 1.0 - a)
            out = _token_maps(r, (B,), out_size, normalize, {"rollout": r})
            if return_attention:
                out["attention"] = abar
        return out
    finally:
        for m, flag in was:
            m.training = flag


def _relevance_walk(T, dev, r, fused=False):
    """The eager backend of xlayers.vit_bwd / bert_bwd with the relevance recursion hooked in
    where the layer backward holds (qkv, dO, mask); the parameter gradients are not formed.
    fused (the text tower): one token_relevance_step launch that honours the key mask and
    writes no map, instead of the attention_relevance + rollout_step pair."""
    from . import xlayers as XL

    class Walk(XL.Eager):
        def __init__(self):
            super().__init__(T, dev, True)
            self.r = r

        @staticmethod
        def gemm_wgrad_bias(*args, **kwargs):
            return None

        def attn_bwd(self, qkv, saved, att, datt, mask, B, Ls, H, scale, p_drop, dqkv):
            if fused:
                self.r = F.token_relevance_step(self.r, qkv, B, Ls, H, scale, 1.0, 1.0, mask,
                                                dout=datt)
            else:
                abar = F.attention_relevance(qkv, B, Ls, H, scale, dout=datt)
                self.r = F.rollout_step(self.r, abar, 1.0, 1.0)
            F.attention_bwd(qkv, saved, att, datt, mask, B, Ls, H, scale, p_drop, dqkv)

    return Walk()


def transformer_attribution(image_encoder, text_encoder, fusion_model, images, input_ids,
                            attention_mask, token_type_ids=None, classes=None, start_layer=0,
                            out_size=(IMG_SIZE, IMG_SIZE), normalize=True):
    """Gradient-weighted attention relevance (Chefer, Gur & Wolf 2021, the self-attention rule)
    of the disease logits for a vit_b_16 image encoder: one map per sample and class.

    Arguments as grad_cam; images [B, 3, 224, 224], B * len(classes) <= 64; the layers
    start_layer .. last take part.  Returns grad_cam's keys, {"logits": [B, n_disease] fp32,
    "classes", "raw": [B, Cs, 14, 14] fp32, "cam": [B, Cs, Ho, Wo] (out_size=None leaves it
    out)}, and "relevance": [B, Cs, S], the class-token row of (I + abar_last) ... (I + abar_s).

    The trunk runs eagerly, outside autograd, on B * Cs replicated rows (row b * Cs + j: sample
    b, classes[j]); only the class-token LayerNorm, `proj` and the fusion head are differentiated
    (one torch.autograd.grad with one-hot grad_outputs), then xlayers.vit_bwd carries the
    gradient down the blocks.  Eval mode whatever the modules' mode (restored on return), works
    under torch.no_grad(), leaves every parameter's .grad untouched."""
    from . import xlayers as XL
    from .vit import _ClassTokenLNFn
    trunk = _vit_trunk_of(image_encoder)
    n_cls = fusion_model.disease_head.out_features
    classes = list(range(n_cls)) if classes is None else [int(c) for c in classes]
    if not classes or any(c < 0 or c >= n_cls for c in classes):
        raise ValueError(f"classes must be indices in [0, {n_cls}), got {classes}")
    Cs = len(classes)
    layers = _check_vit_call(trunk, images, start_layer, Cs)
    B = images.shape[0]
    mods = (image_encoder, text_encoder, fusion_model)
    was = [(m, m.training) for top in mods for m in top.modules()]
    try:
        for top in mods:
            top.eval()
        with torch.no_grad():
            # row b * Cs + j carries sample b and is differentiated for classes[j]
            h, c, kept = trunk.forward_blocks(images.repeat_interleave(Cs, dim=0), True)
            z_txt = text_encoder(input_ids=input_ids, attention_mask=attention_mask,
                                 token_type_ids=token_type_ids)["embeddings"]
        with torch.enable_grad():
            h = h.requires_grad_(True)
            feats = _ClassTokenLNFn.apply(h, trunk.encoder.ln.weight, trunk.encoder.ln.bias)
            t_rep = z_txt.detach().repeat_interleave(Cs, dim=0)
            logits = fusion_model(image_encoder.proj(feats), t_rep)["disease_logits"]
            pick = torch.zeros_like(logits)
            pick[torch.arange(B * Cs, device=logits.device),
                 torch.tensor(classes, device=logits.device).repeat(B)] = 1.0
            (dh,) = torch.autograd.grad(logits, h, grad_outputs=pick)
        with torch.no_grad():
            S, M = c.Ls, B * Cs * c.Ls
            r = torch.zeros((B * Cs, S), dtype=torch.float32, device=h.device)
            r[:, 0] = 1.0
            be = _relevance_walk(h.dtype, h.device, r)
            gd = be.grad_bufs(XL.vit_grads(c.D, c.I))   # only the LayerNorm entries are written
            dO = F.cast(dh.contiguous().reshape(M, c.D), h.dtype)
            for li in range(layers - 1, start_layer - 1, -1):
                dO = XL.vit_bwd(be, kept[li], dO, None, gd, c)
                kept[li] = None
            out = {"logits": logits.detach().view(B, Cs, n_cls)[:, 0].float().contiguous(),
                   "classes": classes, "relevance": be.r.view(B, Cs, S)}
            _token_maps(be.r, (B, Cs), out_size, normalize, out)
        return out
    finally:
        for m, flag in was:
            m.training = flag


# ----------------------------------------------------------------------------- text explanations
def _bert_of(text_encoder):
    enc = getattr(text_encoder, "encoder", None)
    if not hasattr(enc, "forward_layers"):
        raise NotImplementedError(
            f"token relevance needs a transformer text tower: the "
            f"{getattr(text_encoder, 'model_name', type(enc).__name__)} text encoder has no "
            f"attention (BERT towers only)")
    return enc


def _check_text_call(enc, input_ids, attention_mask, start_layer, rows):
    layers = len(enc.encoder.layer)
    if not torch.is_tensor(input_ids) or input_ids.dim() != 2 or input_ids.shape[0] < 1 or \
            not torch.is_tensor(attention_mask) or attention_mask.shape != input_ids.shape:
        raise ValueError("the text tower takes input_ids and attention_mask [B, Ls]")
    if not 1 <= input_ids.shape[1] <= F.ATTN_REL_MAX_L:
        raise ValueError(f"Ls = {input_ids.shape[1]} outside [1, {F.ATTN_REL_MAX_L}]")
    if isinstance(start_layer, bool) or not isinstance(start_layer, int) or \
            not 0 <= start_layer < layers:
        raise ValueError(f"start_layer must be an int in [0, {layers}), got {start_layer!r}")
    if input_ids.shape[0] * rows > MAX_ATTRIBUTION_ROWS:
        raise ValueError(f"B * Cs = {input_ids.shape[0]} * {rows} > {MAX_ATTRIBUTION_ROWS}: "
                         f"split the batch or the classes")
    if int((attention_mask != 0).sum(1).min()) == 0:
        raise ValueError("a row of attention_mask has no real token: its mean pool is undefined")
    return layers


def _mean_pool_start(mask):
    """The recursion's start vector for a tower pooled by the mean over the real tokens:
    mask / n_real, fp32 [B, Ls] (the class-token towers start at e_0)."""
    m = (mask != 0).float()
    return (m / m.sum(1, keepdim=True)).contiguous()


def text_attribution(image_encoder, text_encoder, fusion_model, images, input_ids,
                     attention_mask, token_type_ids=None, classes=None, start_layer=0):
    """Gradient-weighted attention relevance (Chefer, Gur & Wolf 2021, the self-attention rule)
    of the disease logits for the tokens of a BERT text tower: one score per sample, class and
    token.  Arguments as grad_cam; B * len(classes) <= 64, Ls <= 256; the layers start_layer ..
    last take part.  Returns {"logits": [B, n_disease] fp32, "classes", "relevance":
    [B, Cs, Ls] fp32}.

    The tower pools by the mean over the real tokens, so the recursion starts at r = mask /
    n_real and "relevance" is (1 / n) sum_{i real} R[i, :] with R = (I + abar_last) ... (I +
    abar_s); the attention probabilities are those over the real keys, and a pad's relevance is
    exactly 0.  The layers run eagerly, outside autograd, on B * Cs replicated rows (row
    b * Cs + j: sample b, classes[j]); only the mean pool, `proj` and the fusion head are
    differentiated (one torch.autograd.grad with one-hot grad_outputs; the image embedding is
    computed once), then xlayers.bert_bwd carries the gradient down the layers, with one
    functional.token_relevance_step per layer where it holds (qkv, dO, mask).  Eval mode whatever
    the modules' mode (restored on return), works under torch.no_grad(), leaves every parameter's
    .grad untouched.  A row without a real token is a ValueError; an embed-mean or BiLSTM tower
    raises NotImplementedError."""
    from . import xlayers as XL
    enc = _bert_of(text_encoder)
    n_cls = fusion_model.disease_head.out_features
    classes = list(range(n_cls)) if classes is None else [int(c) for c in classes]
    if not classes or any(c < 0 or c >= n_cls for c in classes):
        raise ValueError(f"classes must be indices in [0, {n_cls}), got {classes}")
    Cs = len(classes)
    layers = _check_text_call(enc, input_ids, attention_mask, start_layer, Cs)
    B, Ls = input_ids.shape
    mods = (image_encoder, text_encoder, fusion_model)
    was = [(m, m.training) for top in mods for m in top.modules()]
    try:
        for top in mods:
            top.eval()
        with torch.no_grad():
            z_img = image_encoder(images)["embeddings"]
            # row b * Cs + j carries sample b and is differentiated for classes[j]
            mask = attention_mask.long().repeat_interleave(Cs, dim=0).contiguous()
            tt = None if token_type_ids is None else token_type_ids.repeat_interleave(Cs, dim=0)
            h, c, kept = enc.forward_layers(input_ids.repeat_interleave(Cs, dim=0), mask, tt,
                                            True)
        with torch.enable_grad():
            h = h.requires_grad_(True)
            z_txt = text_encoder.proj(text_encoder.mean_pool(h, mask))
            # (the image tower may compute in another dtype: a ResNet has no fp16 path)
            z_rep = F.cast(z_img.detach().repeat_interleave(Cs, dim=0).contiguous(), z_txt.dtype)
            logits = fusion_model(z_rep, z_txt)["disease_logits"]
            pick = torch.zeros_like(logits)
            pick[torch.arange(B * Cs, device=logits.device),
                 torch.tensor(classes, device=logits.device).repeat(B)] = 1.0
            (dh,) = torch.autograd.grad(logits, h, grad_outputs=pick)
        with torch.no_grad():
            be = _relevance_walk(h.dtype, h.device, _mean_pool_start(mask), fused=True)
            gd = be.grad_bufs(XL.bert_grads(c.D, c.I))   # only the LayerNorm entries are written
            dO = F.cast(dh.contiguous().reshape(B * Cs * Ls, c.D), h.dtype)
            for li in range(layers - 1, start_layer - 1, -1):
                dO = XL.bert_bwd(be, kept[li], dO, mask, gd, c)
                kept[li] = None
        return {"logits": logits.detach().view(B, Cs, n_cls)[:, 0].float().contiguous(),
                "classes": classes, "relevance": be.r.view(B, Cs, Ls)}
    finally:
        for m, flag in was:
            m.training = flag


def text_rollout(text_encoder, input_ids, attention_mask, token_type_ids=None, residual=0.5,
                 start_layer=0):
    """Attention rollout (Abnar & Zuidema 2020) of a BERT text tower with the key mask: where
    the mean-pooled embedding's information came from.  Class-agnostic, forward only.
    A_l = a I + (1 - a) mean_h P_h with the residual a in [0, 1); the start vector is mask /
    n_real as in text_attribution.  Returns {"rollout": [B, Ls] fp32}: each row sums to 1, pads
    are exactly 0.  Eval mode whatever the encoder's mode (restored on return)."""
    enc = _bert_of(text_encoder)
    layers = _check_text_call(enc, input_ids, attention_mask, start_layer, 1)
    a = float(residual)
    if not 0.0 <= a < 1.0:
        raise ValueError(f"residual must be in [0, 1), got {residual!r}")
    was = [(m, m.training) for m in text_encoder.modules()]
    try:
        text_encoder.eval()
        qkvs = []
        mask = attention_mask.long().contiguous()
        _, c, _ = enc.forward_layers(input_ids, mask, token_type_ids, False,
                                     lambda li, saved: qkvs.append(saved["qkv"]))
        with torch.no_grad():
            r = _mean_pool_start(mask)
            scale = 1.0 / math.sqrt(c.D // c.H)
            for li in range(layers - 1, start_layer - 1, -1):
                r = F.token_relevance_step(r, qkvs[li], c.B, c.Ls, c.H, scale, a, 1.0 - a, mask)
        return {"rollout": r}
    finally:
        for m, flag in was:
            m.training = flag


def merge_wordpieces(tokens, scores):
    """WordPiece tokens and their scores -> (words, scores): a "##" continuation piece is
    appended to the word before it and its score added to that word's."""
    if len(tokens) != len(scores):
        raise ValueError(f"{len(tokens)} tokens, {len(scores)} scores")
    words, sums = [], []
    for tok, sc in zip(tokens, scores):
        if tok.startswith("##") and len(tok) > 2 and words:
            words[-1] += tok[2:]
            sums[-1] += float(sc)
        else:
            words.append(tok)
            sums.append(float(sc))
    return words, sums


# ----------------------------------------------------------------------------- fp64 references
def _ref_ln(x, w, b, eps=1e-6):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def reference_vit(state_dict, images, heads=12, track=False):
    """A VitTrunk / RefVitTrunk state dict restated in float64 on the CPU with the attention
    probabilities as explicit tensors of the graph: -> (feats [B, 768], [P_l [B, H, S, S]]).
    track=True makes the token embeddings a leaf that requires grad, so that autograd can
    differentiate a function of feats with respect to every P_l.
    (nn.MultiheadAttention cannot serve: the weights it returns are not the tensor its output
    was computed from, so they carry no gradient of the output.)"""
    sd = {k: v.detach().double().cpu() for k, v in state_dict.items()}
    x = images.detach().double().cpu()
    B = x.shape[0]
    w = sd["conv_proj.weight"]
    D, _, p, _ = w.shape
    tok = torch.nn.functional.conv2d(x, w, sd["conv_proj.bias"], stride=p)
    tok = tok.reshape(B, D, -1).permute(0, 2, 1)
    h = torch.cat([sd["class_token"].expand(B, -1, -1), tok], dim=1) + sd["encoder.pos_embedding"]
    if track:
        h.requires_grad_(True)
    S, hd = h.shape[1], D // heads
    probs = []
    li = 0
    while f"encoder.layers.encoder_layer_{li}.ln_1.weight" in sd:
        k = f"encoder.layers.encoder_layer_{li}."
        u = _ref_ln(h, sd[k + "ln_1.weight"], sd[k + "ln_1.bias"])
        qkv = u @ sd[k + "self_attention.in_proj_weight"].T + sd[k + "self_attention.in_proj_bias"]
        q, kk, v = (t.reshape(B, S, heads, hd).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
        P = torch.softmax(q @ kk.transpose(-1, -2) / math.sqrt(hd), dim=-1)
        probs.append(P)
        att = (P @ v).transpose(1, 2).reshape(B, S, D)
        h = h + att @ sd[k + "self_attention.out_proj.weight"].T + \
            sd[k + "self_attention.out_proj.bias"]
        u = _ref_ln(h, sd[k + "ln_2.weight"], sd[k + "ln_2.bias"])
        f = torch.nn.functional.gelu(u @ sd[k + "mlp.0.weight"].T + sd[k + "mlp.0.bias"])
        h = h + f @ sd[k + "mlp.3.weight"].T + sd[k + "mlp.3.bias"]
        li += 1
    feats = _ref_ln(h[:, 0], sd["encoder.ln.weight"], sd["encoder.ln.bias"])
    return feats, probs


def _class_token_row(abars, alpha, beta, start_layer):
    """e_0^T (alpha I + beta abar_last) ... (alpha I + beta abar_s) by vector steps."""
    B, S = abars[0].shape[0], abars[0].shape[1]
    r = torch.zeros(B, S, dtype=torch.float64)
    r[:, 0] = 1.0
    for A in reversed(abars[start_layer:]):
        r = alpha * r + beta * torch.einsum("bi,bij->bj", r, A)
    return r


def rollout_reference(state_dict, images, residual=0.5, start_layer=0):
    """attention_rollout in float64 torch on the CPU from a trunk's state dict:
    {"feats": [B, 768], "attention": [layers, B, S, S], "rollout": [B, S], "raw": [B, 14, 14]}."""
    with torch.no_grad():
        feats, probs = reference_vit(state_dict, images)
        abars = [P.mean(1) for P in probs]
        r = _class_token_row(abars, float(residual), 1.0 - float(residual), start_layer)
    g = math.isqrt(r.shape[1] - 1)
    return {"feats": feats, "attention": torch.stack(abars), "rollout": r,
            "raw": r[:, 1:].reshape(-1, g, g)}


def attribution_reference(state_dict, images, head, classes=None, start_layer=0):
    """transformer_attribution in float64 torch on the CPU.  head: feats [B, 768] float64 ->
    logits [B, C], differentiable (proj, the fusion head with the text embeddings closed over).
    d logit_c / d P comes from autograd through the explicit attention; the relevance is the
    matrix recursion R <- R + abar R from the identity, of which row 0 is returned:
    {"logits": [B, C], "classes", "relevance": [B, Cs, S], "raw": [B, Cs, 14, 14]}."""
    with torch.enable_grad():
        feats, probs = reference_vit(state_dict, images, track=True)
        logits = head(feats)
        classes = list(range(logits.shape[1])) if classes is None else [int(c) for c in classes]
        rows = []
        for cls in classes:
            # (a head that does not depend on feats has a zero gradient everywhere)
            grads = torch.autograd.grad(logits[:, cls].sum(), probs, retain_graph=True,
                                        allow_unused=True) if logits.requires_grad \
                else [None] * len(probs)
            B, _, S, _ = probs[0].shape
            R = torch.eye(S, dtype=torch.float64).expand(B, S, S).clone()
            for P, dP in list(zip(probs, grads))[start_layer:]:
                dP = torch.zeros_like(P) if dP is None else dP
                abar = (P.detach() * dP).clamp(min=0).mean(1)
                R = R + abar @ R
            rows.append(R[:, 0])
    rel = torch.stack(rows, 1)
    g = math.isqrt(rel.shape[2] - 1)
    return {"logits": logits.detach(), "classes": classes, "relevance": rel,
            "raw": rel[:, :, 1:].reshape(rel.shape[0], len(classes), g, g)}


def reference_bert(state_dict, input_ids, attention_mask, token_type_ids=None, heads=12,
                   track=False):
    """A BertModel state dict (transformers' keys; a text tower's "encoder." prefix is accepted)
    restated in float64 on the CPU with the attention probabilities as explicit tensors of the
    graph: -> (last hidden state [B, Ls, D], [P_l [B, H, Ls, Ls]]).  BERT's embedding sum and
    LayerNorm (eps 1e-12), post-LN layers, exact-erf GELU; the softmax runs over the real keys
    (a masked key's probability is exactly 0), every query row is computed.  track=True makes
    the embeddings a leaf that requires grad (see reference_vit)."""
    pre = "encoder." if "encoder.embeddings.word_embeddings.weight" in state_dict else ""
    sd = {k[len(pre):]: v.detach().double().cpu() for k, v in state_dict.items()
          if k.startswith(pre) and v.is_floating_point()}
    ids = input_ids.detach().long().cpu()
    B, Ls = ids.shape
    real = attention_mask.detach().cpu() != 0
    if not real.any(1).all():
        raise ValueError("a row of attention_mask has no real token")
    tt = torch.zeros_like(ids) if token_type_ids is None else token_type_ids.detach().long().cpu()
    eps = 1e-12
    e = "embeddings."
    h = sd[e + "word_embeddings.weight"][ids] + sd[e + "position_embeddings.weight"][:Ls] + \
        sd[e + "token_type_embeddings.weight"][tt]
    h = _ref_ln(h, sd[e + "LayerNorm.weight"], sd[e + "LayerNorm.bias"], eps)
    if track:
        h.requires_grad_(True)
    D = h.shape[-1]
    hd = D // heads
    neg = torch.zeros(B, 1, 1, Ls, dtype=torch.float64).masked_fill(~real[:, None, None, :],
                                                                    -math.inf)
    probs = []
    li = 0
    while f"encoder.layer.{li}.attention.self.query.weight" in sd:
        k = f"encoder.layer.{li}."

        def lin(x, name):
            return x @ sd[k + name + ".weight"].T + sd[k + name + ".bias"]

        q, kk, v = (lin(h, "attention.self." + n).reshape(B, Ls, heads, hd).transpose(1, 2)
                    for n in ("query", "key", "value"))
        P = torch.softmax(q @ kk.transpose(-1, -2) / math.sqrt(hd) + neg, dim=-1)
        probs.append(P)
        att = (P @ v).transpose(1, 2).reshape(B, Ls, D)
        h1 = _ref_ln(lin(att, "attention.output.dense") + h,
                     sd[k + "attention.output.LayerNorm.weight"],
                     sd[k + "attention.output.LayerNorm.bias"], eps)
        f = torch.nn.functional.gelu(lin(h1, "intermediate.dense"))
        h = _ref_ln(lin(f, "output.dense") + h1, sd[k + "output.LayerNorm.weight"],
                    sd[k + "output.LayerNorm.bias"], eps)
        li += 1
    return h, probs


def _masked_mean(x, real):
    """The mean over the real positions of dim 1: x [B, Ls, ...], real [B, Ls] bool."""
    w = real.double() / real.sum(1, keepdim=True)
    return torch.einsum("bi,bi...->b...", w, x)


def _mean_pool_row(abars, real, alpha, beta, start_layer):
    """(mask / n)^T (alpha I + beta abar_last) ... (alpha I + beta abar_s) by vector steps."""
    r = real.double() / real.sum(1, keepdim=True)
    for A in reversed(abars[start_layer:]):
        r = alpha * r + beta * torch.einsum("bi,bij->bj", r, A)
    return r


def text_rollout_reference(state_dict, input_ids, attention_mask, token_type_ids=None,
                           residual=0.5, start_layer=0, heads=12):
    """text_rollout in float64 torch on the CPU from a text tower's (or BertModel's) state dict:
    {"hidden": [B, Ls, D], "attention": [layers, B, Ls, Ls], "rollout": [B, Ls]}."""
    with torch.no_grad():
        h, probs = reference_bert(state_dict, input_ids, attention_mask, token_type_ids, heads)
        abars = [P.mean(1) for P in probs]
        real = attention_mask.detach().cpu() != 0
        r = _mean_pool_row(abars, real, float(residual), 1.0 - float(residual), start_layer)
    return {"hidden": h, "attention": torch.stack(abars), "rollout": r}


def text_attribution_reference(state_dict, input_ids, attention_mask, head, token_type_ids=None,
                               classes=None, start_layer=0, heads=12):
    """text_attribution in float64 torch on the CPU.  head: the mean-pooled hidden state
    [B, D] float64 -> logits [B, C], differentiable (the tower's proj, the fusion head with the
    image embeddings closed over).  d logit_c / d P comes from autograd through the explicit
    attention; the relevance is the matrix recursion R <- R + abar R from the identity, of which
    the mean over the real rows is returned: {"logits": [B, C], "classes", "relevance":
    [B, Cs, Ls], "matrix": [B, Cs, Ls, Ls], "abar": per class the layers' [B, Ls, Ls]}."""
    real = attention_mask.detach().cpu() != 0
    with torch.enable_grad():
        h, probs = reference_bert(state_dict, input_ids, attention_mask, token_type_ids, heads,
                                  track=True)
        logits = head(_masked_mean(h, real))
        classes = list(range(logits.shape[1])) if classes is None else [int(c) for c in classes]
        rows, mats, maps = [], [], []
        for cls in classes:
            grads = torch.autograd.grad(logits[:, cls].sum(), probs, retain_graph=True,
                                        allow_unused=True) if logits.requires_grad \
                else [None] * len(probs)
            B, _, S, _ = probs[0].shape
            R = torch.eye(S, dtype=torch.float64).expand(B, S, S).clone()
            abars = []
            for P, dP in zip(probs, grads):
                dP = torch.zeros_like(P) if dP is None else dP
                abars.append((P.detach() * dP).clamp(min=0).mean(1))
            for abar in abars[start_layer:]:
                R = R + abar @ R
            rows.append(_masked_mean(R, real))
            mats.append(R)
            maps.append(abars)
    return {"logits": logits.detach(), "classes": classes, "relevance": torch.stack(rows, 1),
            "matrix": torch.stack(mats, 1), "abar": maps}


def select_classes(probs, thresholds, class_names, explain):
    """The class indices inference(explain=...) draws heatmaps for.  True: the classes at or
    above their threshold, or the top-1 class if there is none; an int k: the top-k classes
    by probability; a list of class names: those."""
    n = len(class_names)
    order = sorted(range(n), key=lambda j: (-float(probs[j]), j))
    if explain is True:
        hit = [j for j in range(n) if float(probs[j]) >= float(thresholds[j])]
        return hit or order[:1]
    if isinstance(explain, int) and not isinstance(explain, bool):
        if not 1 <= explain <= n:
            raise ValueError(f"explain={explain}: the top-k count must be in [1, {n}]")
        return order[:explain]
    if isinstance(explain, (list, tuple)) and explain and \
            all(isinstance(c, str) for c in explain):
        names = list(class_names)
        unknown = [c for c in explain if c not in names]
        if unknown:
            raise ValueError(f"explain: unknown class names {unknown}")
        return [names.index(c) for c in explain]
    raise TypeError("explain must be None, True, a top-k count or a list of class names, got "
                    f"{explain!r}")


# ----------------------------------------------------------------------------- host helpers
def _crop_geometry(image_size):
    """Resize-256 (shorter side) + CenterCrop-224 of a (W, H) image, as
    image_transfom_into_tensor does it: the resized size and the crop's left / top in it."""
    w, h = (int(v) for v in image_size)
    if w <= h:
        nw, nh = RESIZE_SIZE, int(RESIZE_SIZE * h / w)
    else:
        nw, nh = int(RESIZE_SIZE * w / h), RESIZE_SIZE
    left = int(round((nw - IMG_SIZE) / 2.0))
    top = int(round((nh - IMG_SIZE) / 2.0))
    return nw, nh, left, top


def cam_to_image(cam224, image_size):
    """Undo Resize-256 + CenterCrop-224: the [224, 224] map placed on the original image of
    `image_size` = (W, H) (PIL's order).  Returns float32 [H, W], zero outside the crop."""
    from PIL import Image
    cam = np.asarray(cam224, dtype=np.float32)
    if cam.shape != (IMG_SIZE, IMG_SIZE):
        raise ValueError(f"cam_to_image takes a [{IMG_SIZE}, {IMG_SIZE}] map, got {cam.shape}")
    w, h = (int(v) for v in image_size)
    nw, nh, left, top = _crop_geometry((w, h))
    sx, sy = w / nw, h / nh
    # the crop rectangle in original pixels
    x0, x1 = int(round(left * sx)), int(round((left + IMG_SIZE) * sx))
    y0, y1 = int(round(top * sy)), int(round((top + IMG_SIZE) * sy))
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
    out = np.zeros((h, w), dtype=np.float32)
    if x1 > x0 and y1 > y0:
        patch = Image.fromarray(cam).resize((x1 - x0, y1 - y0), Image.BILINEAR)
        out[y0:y1, x0:x1] = np.asarray(patch, dtype=np.float32)
    return out


def _jet(v):
    """Jet-style ramp of v in [0, 1] -> float32 [..., 3] in [0, 1] (blue, cyan, yellow, red)."""
    v = np.clip(np.asarray(v, dtype=np.float32), 0.0, 1.0)
    r = np.clip(1.5 - np.abs(4.0 * v - 3.0), 0.0, 1.0)
    g = np.clip(1.5 - np.abs(4.0 * v - 2.0), 0.0, 1.0)
    b = np.clip(1.5 - np.abs(4.0 * v - 1.0), 0.0, 1.0)
    return np.stack([r, g, b], axis=-1)


def overlay(image_pil, cam, alpha=0.4):
    """The image with the heatmap blended in: PIL RGB, same size.  `cam` is a float map in
    [0, 1] at the image's size ([H, W], e.g. from cam_to_image).  The blend weight of a pixel is
    alpha * cam, so a zero map leaves the image unchanged."""
    from PIL import Image
    rgb = np.asarray(image_pil.convert("RGB"), dtype=np.float32)
    cam = np.clip(np.asarray(cam, dtype=np.float32), 0.0, 1.0)
    if cam.shape != rgb.shape[:2]:
        raise ValueError(f"overlay: the map is {cam.shape}, the image {rgb.shape[:2]} (H, W)")
    wgt = (float(alpha) * cam)[..., None]
    mix = rgb * (1.0 - wgt) + 255.0 * _jet(cam) * wgt
    return Image.fromarray(np.clip(np.rint(mix), 0, 255).astype(np.uint8))
