"""Time the fused text-explanation kernel (functional.token_relevance_step) against two
yardsticks on the same GPU, and the text explanations end to end.

    python tools/text_explain_bench.py [--batch 1 13 64] [--samples 20] [--out FILE]
                                        [--parity FILE [--parity-only]]

The tokenizer's geometry: Ls = 96 tokens, H = 12 heads of 64, fp16 and fp32, plain and
weighted, an all-ones key mask (so that the yardsticks compute the same thing).  Yardsticks: the
pair functional.attention_relevance + functional.rollout_step, which writes the [Ls, Ls] map and
reads it back in a second launch; and the same quantity from torch's own ROCm ops (einsum,
masked softmax, mean over the heads, the row-vector product; the weighted mode adds the dO V^T
einsum, the product, relu).  Both are checked against the fused launch before anything is timed.
Device events around back-to-back launches after a warm-up of every op; the ops alternate sample
by sample, so a drift of the shared machine hits all of them; per op the median of the samples
with min / p10 / p90 / max.

End to end: a randomly initialised vit_b_16 + 12-layer BERT bundle in fp16 on tests/golden/e1.jpg:
text_attribution for one sample and all 13 classes, text_rollout, and inference() against
inference_explained(explain_text=13) (host clock around calls that end synchronised).

--parity FILE: text_attribution and text_rollout of the fp32, fp16 and bf16 two-layer towers
against the float64 CPU references (the figures tests/test_text_explain_gpu.py bounds), over the
model seeds 0..3; --parity-only stops after it.  Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mmdx  # noqa: E402
import mmdx.functional as F  # noqa: E402

LS, H, HD = 96, 12, 64
SCALE = 0.125


def torch_ops(r, qkv, dout, mask, B):
    t = qkv.view(B, LS, 3, H, HD)
    q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    logits = torch.einsum("bqhd,bkhd->bhqk", q, k).float() * SCALE
    P = torch.softmax(logits.masked_fill(mask[:, None, None, :] == 0, -float("inf")), dim=-1)
    if dout is None:
        abar = P.mean(1)
    else:
        dP = torch.einsum("bqhd,bkhd->bhqk", dout.view(B, LS, H, HD), v).float()
        abar = torch.relu(P * dP).mean(1)
    return r + torch.einsum("bi,bij->bj", r, abar)


def pair(r, qkv, dout, B):
    return F.rollout_step(r, F.attention_relevance(qkv, B, LS, H, SCALE, dout=dout), 1.0, 1.0)


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
            r = torch.rand(B, LS, generator=g).to(dev)
            mask = torch.ones(B, LS, dtype=torch.long, device=dev)

            def fused(d):
                return F.token_relevance_step(r, qkv, B, LS, H, SCALE, 1.0, 1.0, mask, dout=d)

            for d in (None, dout):
                a, b, c = fused(d), pair(r, qkv, d, B), torch_ops(r, qkv, d, mask, B)
                torch.cuda.synchronize()
                # (torch's fp16 einsum rounds the logits to fp16 before the softmax)
                tol = 1e-4 if dtype == torch.float32 else 2e-2
                for name, other in (("the pair", b), ("torch ops", c)):
                    err = (a - other).abs().max().item()
                    if not err <= tol * max(other.abs().max().item(), 1e-30):
                        raise SystemExit(f"B = {B} {dtype}: the fused launch and {name} disagree "
                                         f"({err})")
            inner = 20 if B <= 13 else 5
            ops = [("token_relevance_step plain", lambda: fused(None)),
                   ("attention_relevance + rollout_step", lambda: pair(r, qkv, None, B)),
                   ("torch einsum/masked softmax/mean/einsum",
                    lambda: torch_ops(r, qkv, None, mask, B)),
                   ("token_relevance_step weighted", lambda: fused(dout)),
                   ("attention_relevance + rollout_step, weighted",
                    lambda: pair(r, qkv, dout, B)),
                   ("torch, weighted", lambda: torch_ops(r, qkv, dout, mask, B))]
            lines.append(f"B = {B}, {str(dtype).split('.')[-1]}: qkv [{B * LS}, 3, 12, 64], r "
                         f"[{B}, {LS}] fp32; {inner} calls per sample")
            m = timed(ops, samples, inner, lines)
            lines.append(f"  fused / pair: plain {m[0] / m[1]:.2f}, weighted {m[3] / m[4]:.2f}; "
                         f"fused / torch: plain {m[0] / m[2]:.2f}, weighted {m[3] / m[5]:.2f}")


def bench_end_to_end(dev, samples, lines):
    from PIL import Image
    from mmdx.explain import text_attribution, text_rollout
    from mmdx.inference_pipeline import inference, inference_explained
    torch.manual_seed(0)
    T = torch.float16
    bundle = {"image_encoder": mmdx.ImageEncoderCNN("vit_b_16", 1024, 13, compute_dtype=T),
              "text_encoder": mmdx.TextEncoderTransformer("bert-base-uncased", 512, 13,
                                                          compute_dtype=T),
              "fusion_model": mmdx.FusionTransformerModel(1024, 512, 1024, 13),
              "class_names": mmdx.DISEASES, "thresholds": [0.5] * 13, "version": 0,
              "t5_tok": None}
    for k in ("image_encoder", "text_encoder", "fusion_model"):
        bundle[k] = bundle[k].to(dev).eval()
    img, txt, fus = (bundle[k] for k in ("image_encoder", "text_encoder", "fusion_model"))
    pil = Image.open(os.path.join(ROOT, "tests", "golden", "e1.jpg")).convert("RGB")
    text = "44 year old female PA view , hypertension , cough"
    x = torch.randn(1, 3, 224, 224, device=dev)
    tok = {k: v.to(dev) for k, v in mmdx.tokenize_patient_details([text], max_len=96).items()}
    ids, mask = tok["input_ids"], tok["attention_mask"]
    calls = [("inference()", lambda: inference(bundle, pil, text, device=dev)),
             ("inference_explained(explain_text=13)",
              lambda: inference_explained(bundle, pil, text, device=dev, explain_text=13)),
             ("inference_explained(explain_text=1)",
              lambda: inference_explained(bundle, pil, text, device=dev, explain_text=1)),
             ("text_attribution, 1 sample x 13 classes",
              lambda: text_attribution(img, txt, fus, x, ids, mask)),
             ("text_rollout, 1 sample", lambda: text_rollout(txt, ids, mask))]
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
    lines.append("end to end, vit_b_16 + BERT (12 layers, Ls = 96) in fp16, no report head, "
                 "tests/golden/e1.jpg; milliseconds (host clock around calls that end "
                 "synchronised):")
    for name, _ in calls:
        t = np.array(ts[name])
        lines.append(f"  {name:<44s} median {np.median(t):9.2f} ms   min {t.min():9.2f}   p90 "
                     f"{np.percentile(t, 90):9.2f}   max {t.max():9.2f}   ({len(t)} samples)")
    base = np.median(ts["inference()"])
    for name in ("inference_explained(explain_text=13)", "inference_explained(explain_text=1)"):
        lines.append(f"  {name} adds {(np.median(ts[name]) - base):.2f} ms (medians)")


def parity(dev, path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import text_explain_cases as C
    lines = ["text_attribution relevance (per sample over the classes " + str(C.CLASSES) +
             " flattened), its logits, and the text_rollout rows, fp32 / fp16 / bf16 towers vs the "
             "float64 CPU references: resnet18 + BERT(layers=2), B = 2, Ls = 16, " +
             str(C.LENGTHS) + " real tokens",
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
        raise SystemExit("text_explain_bench needs a GPU")
    dev = torch.device("cuda:0")
    if a.parity:
        parity(dev, a.parity)
    if a.parity_only:
        return
    lines = [f"The fused text-explanation launch vs the two-kernel pair and torch's own ops, the "
             f"tokenizer's geometry (Ls = {LS}, H = {H}, head dim {HD}, all-ones mask), "
             f"{torch.cuda.get_device_name(0)}"]
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
