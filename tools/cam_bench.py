"""Time the Grad-CAM kernels (functional.cam_raw + functional.cam_resize) against the same
computation from torch's own ROCm ops (einsum, relu, amax, F.interpolate) on the same tensors,
and the cost explain=True adds to one inference() call.

    python tools/cam_bench.py [--batch 1 128] [--samples 30] [--out FILE] [--parity FILE]

The resnet50 geometry: a 7 x 7 x 2048 bf16 feature map, 13 classes, 224 x 224 output.  Device
events around back-to-back launches, after a warm-up of every shape; the two sides alternate
sample by sample, so a drift of the shared machine hits both; per op the median with min / p10 /
p90 / max.  GB/s is against the algorithmic bytes: fmap and alpha read once, the output written
once (the fp32 intermediate `raw` is not counted).  The torch side is checked against the
kernels before anything is timed.  inference(): a randomly initialised resnet50 + embed-mean
bundle on tests/golden/e1.jpg, host clock around calls that end in a device-to-host copy.

--parity FILE: grad_cam of the bf16 resnet18 towers against autograd on the fp32 CPU oracle
(the figures tests/test_cam_gpu.py bounds), over the model seeds 0..3.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmdx  # noqa: E402
import mmdx.functional as F  # noqa: E402

H = W = 7
K = 2048
C = 13
OUT = (224, 224)


def ours(fmap, alpha):
    return F.cam_resize(F.cam_raw(fmap, alpha), OUT)


def torch_ops(fmap, alpha):
    raw = torch.relu(torch.einsum("bck,bhwk->bchw", alpha, fmap.float()))
    peak = raw.amax(dim=(2, 3), keepdim=True)
    norm = torch.where(peak > 0, raw / peak, torch.zeros_like(raw))
    return TF.interpolate(norm, size=OUT, mode="bilinear", align_corners=False)


def torch_ops_bf16(fmap, alpha):
    """The same with the contraction in the map's own dtype (no fp32 copy of the map; a bf16
    GEMM whose result is rounded to bf16): cheaper for torch, less accurate."""
    raw = torch.relu(torch.einsum("bck,bhwk->bchw", alpha.to(fmap.dtype), fmap)).float()
    peak = raw.amax(dim=(2, 3), keepdim=True)
    norm = torch.where(peak > 0, raw / peak, torch.zeros_like(raw))
    return TF.interpolate(norm, size=OUT, mode="bilinear", align_corners=False)


def one(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def line(name, t, gbytes=None):
    s = (f"  {name:<40s} median {np.median(t) * 1e3:9.2f} us   min {t.min() * 1e3:9.2f}   "
         f"p10 {np.percentile(t, 10) * 1e3:9.2f}   p90 {np.percentile(t, 90) * 1e3:9.2f}   "
         f"max {t.max() * 1e3:9.2f}   ({len(t)} samples)")
    if gbytes is not None:
        s += f"   {gbytes / (np.median(t) * 1e-3):8.1f} GB/s"
    return s


def bench_kernels(dev, batches, samples, lines):
    for B in batches:
        g = torch.Generator().manual_seed(B)
        fmap = torch.randn(B, H, W, K, generator=g).clamp(min=0).to(torch.bfloat16).to(dev)
        alpha = (torch.randn(B, C, K, generator=g) / (H * W)).to(dev)
        a, b = ours(fmap, alpha), torch_ops(fmap, alpha)
        torch.cuda.synchronize()
        err = (a - b).abs().max().item()
        if not err <= 1e-4:
            raise SystemExit(f"B = {B}: the kernels and the torch composition disagree ({err})")
        gb = (fmap.numel() * 2 + alpha.numel() * 4 + B * C * OUT[0] * OUT[1] * 4) / 1e9
        inner = 50 if B <= 8 else 10
        ops = [("cam_raw + cam_resize (2 launches)", lambda: ours(fmap, alpha)),
               ("torch einsum/relu/amax/interpolate", lambda: torch_ops(fmap, alpha)),
               ("torch, contraction in bf16", lambda: torch_ops_bf16(fmap, alpha)),
               ("cam_raw alone", lambda: F.cam_raw(fmap, alpha)),
               ("cam_resize alone", lambda: F.cam_resize(a[:, :, :H, :W].contiguous(), OUT))]
        for _, fn in ops:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ts = [[] for _ in ops]
        for _ in range(samples):       # alternate the ops sample by sample
            for k, (_, fn) in enumerate(ops):
                ts[k].append(one(fn, inner))
        lines.append(f"B = {B}: fmap [{B}, 7, 7, 2048] bf16, alpha [{B}, 13, 2048] fp32 -> "
                     f"[{B}, 13, 224, 224] fp32; {gb * 1e3:.2f} MB algorithmic; "
                     f"kernels vs torch max abs diff {err:.1e}; {inner} calls per sample")
        for k, (name, _) in enumerate(ops):
            lines.append(line(name, np.array(ts[k]), gb if k < 3 else None))


def bench_inference(dev, samples, lines):
    from PIL import Image
    from mmdx.inference_pipeline import inference
    torch.manual_seed(0)
    bundle = {"image_encoder": mmdx.ImageEncoderCNN("resnet50", 1024, 13,
                                                    compute_dtype=torch.bfloat16),
              "text_encoder": mmdx.TextEncoderTransformer("embed-mean", 512, 13,
                                                          compute_dtype=torch.bfloat16),
              "fusion_model": mmdx.FusionTransformerModel(1024, 512, 1024, 13),
              "class_names": mmdx.DISEASES, "thresholds": [0.5] * 13, "version": 0,
              "t5_tok": None}
    for k in ("image_encoder", "text_encoder", "fusion_model"):
        bundle[k] = bundle[k].to(dev).eval()
    gold = os.path.join(ROOT, "tests", "golden")
    pil = Image.open(os.path.join(gold, "e1.jpg")).convert("RGB")
    with open(os.path.join(gold, "patient_details.json")) as f:
        text = json.load(f)["e1.jpg"]
    modes = [("inference()", None), ("inference(explain=True)", True),
             ("inference(explain=13)", 13)]
    n_maps = {}
    for name, ex in modes:
        for _ in range(3):
            out = inference(bundle, pil, text, device=dev, explain=ex)
        n_maps[name] = len(out.get("heatmaps", {}))
    ts = {name: [] for name, _ in modes}
    for _ in range(samples):
        for name, ex in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inference(bundle, pil, text, device=dev, explain=ex)
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    lines.append("inference() end to end, resnet50 + embed-mean in bf16, no report head, "
                 "tests/golden/e1.jpg (host clock around calls that end synchronised):")
    for name, _ in modes:
        lines.append(line(f"{name} [{n_maps[name]} maps]", np.array(ts[name])))
    base = np.median(ts["inference()"])
    for name, _ in modes[1:]:
        lines.append(f"  {name} adds {(np.median(ts[name]) - base) * 1e3:.0f} us (medians)")


def parity(dev, path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from parity_util import build_pair, cosine, rel_err, synth_batch
    from mmdx.explain import grad_cam
    lines = ["grad_cam raw maps, bf16 towers vs torch.autograd on the fp32 CPU oracle: resnet18 + "
             "embed-mean, synth_batch(2, 16, hw=64) (2 x 2 maps), per sample over the 13 classes "
             "flattened", torch.cuda.get_device_name(0)]
    x, ids, mask, _ = synth_batch(2, 16, hw=64)
    worst = [0.0, 0.0]
    for seed in range(4):
        ref, img, txt, fus = build_pair("resnet18", "embed-mean", seed=seed,
                                        dtype=torch.bfloat16)
        ref.eval()
        keep = {}
        h = ref.image.backbone[7].register_forward_hook(lambda m, i, o: keep.update(A=o))
        logits = ref(x, ids, mask)
        h.remove()
        A = keep["A"]
        maps = []
        for c in range(13):
            (gA,) = torch.autograd.grad(logits[:, c].sum(), A, retain_graph=True)
            maps.append((gA.mean(dim=(2, 3), keepdim=True) * A).sum(1).clamp(min=0))
        want = torch.stack(maps, 1).detach()
        raw = grad_cam(img.to(dev), txt.to(dev), fus.to(dev), x.to(dev), ids.to(dev),
                       mask.to(dev), out_size=None)["raw"].cpu()
        for b in range(2):
            omc, rel = 1.0 - cosine(raw[b], want[b]), rel_err(raw[b], want[b])
            worst = [max(worst[0], omc), max(worst[1], rel)]
            lines.append(f"  seed {seed} sample {b}: 1-cos {omc:.3e}   rel_err {rel:.3e}")
    lines.append(f"worst over the seeds: 1-cos {worst[0]:.3e}   rel_err {worst[1]:.3e}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 128])
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parity", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cam_bench needs a GPU")
    dev = torch.device("cuda:0")
    if a.parity:
        parity(dev, a.parity)
    lines = [f"Grad-CAM kernels vs torch's own ops, resnet50 geometry (7 x 7 x 2048 bf16, 13 "
             f"classes, 224 x 224 out), {torch.cuda.get_device_name(0)}"]
    bench_kernels(dev, a.batch, a.samples, lines)
    bench_inference(dev, a.samples, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
