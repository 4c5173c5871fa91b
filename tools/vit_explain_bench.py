"""Time the ViT explanation kernels (functional.attention_relevance, functional.rollout_step)
against two yardsticks on the same GPU, and the explanations end to end.

    python tools/vit_explain_bench.py [--batch 1 13 64] [--samples 20] [--out FILE]
                                       [--parity FILE [--parity-only]]

The vit_b_16 geometry: Ls = 197 tokens, H = 12 heads of 64, fp16 and fp32.  Yardsticks:
the same quantity from torch's own ROCm ops (einsum, softmax, mean over the heads; the weighted
mode adds the dO V^T einsum, the product, relu), checked against the kernel before anything is
timed; and the project's attention forward (mmdx_attention_fwd, inference form, nothing saved) on
the same qkv buffer: a kernel that also forms softmax(Q K^T) per head, and P V on top.  Device
events around back-to-back launches after a warm-up of every op; the ops alternate sample by
sample, so a drift of the shared machine hits all of them; per op the median with min / p10 /
p90 / max.

End to end: a randomly initialised vit_b_16 + embed-mean bundle in fp16 on tests/golden/e1.jpg:
transformer_attribution for one image and all 13 classes, attention_rollout, and inference()
plain and with explain=13 (host clock around calls that end synchronised).

--parity FILE: transformer_attribution and attention_rollout of the fp32, fp16 and bf16
two-layer towers against the float64 CPU references (the figures tests/test_vit_explain_gpu.py
bounds), over the model seeds 0..3; --parity-only stops after it.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmdx  # noqa: E402
import mmdx.functional as F  # noqa: E402

LS, H, HD = 197, 12, 64
SCALE = 0.125


def torch_ops(qkv, dout, B):
    t = qkv.view(B, LS, 3, H, HD)
    q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    P = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k).float() * SCALE, dim=-1)
    if dout is None:
        return P.mean(1)
    dP = torch.einsum("bqhd,bkhd->bhqk", dout.view(B, LS, H, HD), v).float()
    return torch.relu(P * dP).mean(1)


def one(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def line(name, t):
    return (f"  {name:<44s} median {np.median(t) * 1e3:9.2f} us   min {t.min() * 1e3:9.2f}   "
            f"p10 {np.percentile(t, 10) * 1e3:9.2f}   p90 {np.percentile(t, 90) * 1e3:9.2f}   "
            f"max {t.max() * 1e3:9.2f}   ({len(t)} samples)")


def timed(ops, samples, inner, lines):
    for _, fn in ops:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in ops]
    for _ in range(samples):       # alternate the ops sample by sample
        for k, (_, fn) in enumerate(ops):
            ts[k].append(one(fn, inner))
    for k, (name, _) in enumerate(ops):
        lines.append(line(name, np.array(ts[k])))
    return [float(np.median(t)) for t in ts]


def bench_kernels(dev, batches, samples, lines):
    for dtype in (torch.float16, torch.float32):
        for B in batches:
            g = torch.Generator().manual_seed(B)
            qkv = torch.randn(B * LS, 3 * H * HD, generator=g).to(dtype).to(dev)
            dout = (torch.randn(B * LS, H * HD, generator=g) / 64).to(dtype).to(dev)
            att = torch.empty(B * LS, H * HD, dtype=dtype, device=dev)
            for d in (None, dout):
                a, b = F.attention_relevance(qkv, B, LS, H, SCALE, dout=d), torch_ops(qkv, d, B)
                torch.cuda.synchronize()
                err = (a - b).abs().max().item()
                # (torch's fp16 einsum rounds the logits to fp16 before the softmax)
                tol = 1e-4 if dtype == torch.float32 else 2e-2
                if not err <= tol * max(b.abs().max().item(), 1e-30):
                    raise SystemExit(f"B = {B} {dtype}: kernel and torch ops disagree ({err})")
            r = torch.rand(B, LS, device=dev)
            abar = F.attention_relevance(qkv, B, LS, H, SCALE)
            inner = 20 if B <= 13 else 5
            ops = [("attention_relevance plain", lambda: F.attention_relevance(qkv, B, LS, H,
                                                                                SCALE)),
                   ("torch einsum/softmax/mean", lambda: torch_ops(qkv, None, B)),
                   ("attention_relevance weighted",
                    lambda: F.attention_relevance(qkv, B, LS, H, SCALE, dout=dout)),
                   ("torch, weighted (two einsums, relu, mean)",
                    lambda: torch_ops(qkv, dout, B)),
                   ("attention forward (mmdx_attention_fwd)",
                    lambda: F.attention_fwd(qkv, None, B, LS, H, SCALE, 0.0, 0, None, att,
                                            False)),
                   ("rollout_step", lambda: F.rollout_step(r, abar, 0.5, 0.5))]
            lines.append(f"B = {B}, {str(dtype).split('.')[-1]}: qkv [{B * LS}, 3, 12, 64] -> abar "
                         f"[{B}, 197, 197] fp32; {inner} calls per sample")
            m = timed(ops, samples, inner, lines)
            lines.append(f"  plain: {m[1] / m[0]:.2f}x torch, {m[0] / m[4]:.2f}x the attention "
                         f"forward's time; weighted: {m[3] / m[2]:.2f}x torch")


def bench_end_to_end(dev, samples, lines):
    from PIL import Image
    from mmdx.explain import attention_rollout, transformer_attribution
    from mmdx.inference_pipeline import inference
    torch.manual_seed(0)
    T = torch.float16
    bundle = {"image_encoder": mmdx.ImageEncoderCNN("vit_b_16", 1024, 13, compute_dtype=T),
              "text_encoder": mmdx.TextEncoderTransformer("embed-mean", 512, 13, compute_dtype=T),
              "fusion_model": mmdx.FusionTransformerModel(1024, 512, 1024, 13),
              "class_names": mmdx.DISEASES, "thresholds": [0.5] * 13, "version": 0,
              "t5_tok": None}
    for k in ("image_encoder", "text_encoder", "fusion_model"):
        bundle[k] = bundle[k].to(dev).eval()
    img, txt, fus = (bundle[k] for k in ("image_encoder", "text_encoder", "fusion_model"))
    gold = os.path.join(ROOT, "tests", "golden")
    pil = Image.open(os.path.join(gold, "e1.jpg")).convert("RGB")
    with open(os.path.join(gold, "patient_details.json")) as f:
        text = json.load(f)["e1.jpg"]
    x = torch.randn(1, 3, 224, 224, device=dev)
    ids = torch.randint(1000, 30000, (1, 16), device=dev)
    mask = torch.ones_like(ids)
    calls = [("inference()", lambda: inference(bundle, pil, text, device=dev)),
             ("inference(explain=13)", lambda: inference(bundle, pil, text, device=dev,
                                                         explain=13)),
             ("inference(explain=1)", lambda: inference(bundle, pil, text, device=dev,
                                                        explain=1)),
             ("transformer_attribution, 1 image x 13 classes",
              lambda: transformer_attribution(img, txt, fus, x, ids, mask)),
             ("attention_rollout, 1 image", lambda: attention_rollout(img, x))]
    for _, fn in calls:
        for _ in range(3):
            fn()
    ts = {name: [] for name, _ in calls}
    for _ in range(samples):
        for name, fn in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    lines.append("end to end, vit_b_16 (12 layers) + embed-mean in fp16, no report head, "
                 "tests/golden/e1.jpg (host clock around calls that end synchronised):")
    for name, _ in calls:
        lines.append(line(name, np.array(ts[name])))
    base = np.median(ts["inference()"])
    for name in ("inference(explain=13)", "inference(explain=1)"):
        lines.append(f"  {name} adds {(np.median(ts[name]) - base):.2f} ms (medians)")


def parity(dev, path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vit_explain_cases as C
    lines = ["transformer_attribution raw maps (per sample over the classes " + str(C.CLASSES) +
             " flattened), its logits, and the attention_rollout row, fp32 / fp16 / bf16 towers "
             "vs the float64 CPU references: VitTrunk(layers=2) + embed-mean, "
             "synth_batch(2, 16, hw=224)",
             torch.cuda.get_device_name(0)]
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        name = str(dtype).split(".")[-1]
        worst = [0.0, 0.0, 0.0, 0.0]
        for seed in range(4):
            per, lerr, _ = C.attribution_errors(seed, dtype, dev)
            rerr, _ = C.rollout_errors(seed, dtype, dev)
            for b, (omc, nr) in enumerate(per):
                lines.append(f"  {name} seed {seed} sample {b}: 1-cos {omc:.3e}   |norm ratio - 1| "
                             f"{nr:.3e}")
                worst[0], worst[1] = max(worst[0], omc), max(worst[1], nr)
            lines.append(f"  {name} seed {seed}: logits rel_err {lerr:.3e}   rollout rel_err "
                         f"{rerr:.3e}")
            worst[2], worst[3] = max(worst[2], lerr), max(worst[3], rerr)
        lines.append(f"{name} worst over the seeds: 1-cos {worst[0]:.3e}   |norm ratio - 1| "
                     f"{worst[1]:.3e}   logits rel_err {worst[2]:.3e}   rollout rel_err "
                     f"{worst[3]:.3e}")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 13, 64])
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parity", default=None)
    ap.add_argument("--parity-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vit_explain_bench needs a GPU")
    dev = torch.device("cuda:0")
    if a.parity:
        parity(dev, a.parity)
    if a.parity_only:
        return
    lines = [f"ViT explanation kernels vs torch's own ops and the attention forward, vit_b_16 "
             f"geometry (Ls = 197, H = 12, head dim 64), {torch.cuda.get_device_name(0)}"]
    bench_kernels(dev, a.batch, a.samples, lines)
    bench_end_to_end(dev, a.samples, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
