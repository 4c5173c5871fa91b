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
trunks have such a conv stage; a vit_b_16 encoder raises NotImplementedError.

`cam_to_image` and `overlay` are the host half (numpy / PIL): put a 224 x 224 map back on the
original radiograph and blend it in.
"""
from __future__ import annotations

import numpy as np
import torch

from . import functional as F
from .training_pipeline import IMG_SIZE

__all__ = ["grad_cam", "select_classes", "cam_to_image", "overlay"]

RESIZE_SIZE = 256  # the shorter side before the centre crop (image_transfom_into_tensor)


def _trunk_of(image_encoder):
    trunk = getattr(image_encoder, "backbone", None)
    if not hasattr(trunk, "forward_features"):
        raise NotImplementedError(
            f"Grad-CAM needs a convolutional last stage: the "
            f"{getattr(image_encoder, 'backbone_name', type(trunk).__name__)} image encoder has "
            f"none (ResNet backbones only; ViT attention rollout is not implemented)")
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
