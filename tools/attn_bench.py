#!/usr/bin/env python3
"""Isolated timing of the attention kernels at the C5 shapes, ViT-B/16 (B 64, L 197, H 12) and
BERT-base (B 64, L 128, H 12, masked; also with the dropout p = 0.1 C5 trains with), fp16:
the P-saving entry points (mmdx_attention_fwd / _bwd) and the flash-style ones the C5 path
runs (mmdx_attention_fwd_lse / _bwd_lse).
    python tools/attn_bench.py [--reps 20]
--digest times nothing: it runs every attention entry point, and the other consumers of the
dropout stream (mmdx_xattn_fwd, mmdx_dropout_fwd, mmdx_layernorm_fwd_dropout / _bwd_dropout),
on seeded inputs at small edge shapes and prints one sha256 per output tensor.  These kernels
have no atomics and fixed reduction orders, so two builds that compute the same thing print the
same lines.
    python tools/attn_bench.py --digest > new.txt
    MMDX_LIB_PATH=/path/to/other/libmmdx_hip.so python tools/attn_bench.py --digest > old.txt
Both modes load the library MMDX_LIB_PATH names, if set (mmdx._lib).
"""
import argparse
import hashlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def bench(L, dev, reps):
    dt = torch.float16
    dc = L.dtype_code(dt)
    for name, B, Ls, H, masked, pd in (("vit", 64, 197, 12, False, 0.0),
                                       ("bert", 64, 128, 12, True, 0.0),
                                       ("bert", 64, 128, 12, True, 0.1)):
        D = 64 * H
        qkv = (torch.randn(B * Ls, 3 * D, device=dev) * 0.5).to(dt)
        mask = torch.ones(B, Ls, dtype=torch.long, device=dev) if masked else None
        out = torch.empty(B * Ls, D, dtype=dt, device=dev)
        probs = torch.empty(B, H, Ls, Ls, device=dev)
        lse = torch.empty(B, H, Ls, device=dev)
        rng = torch.zeros(1, dtype=torch.int64, device=dev)
        ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        dout = (torch.randn(B * Ls, D, device=dev) * 0.5).to(dt)
        dqkv = torch.empty_like(qkv)
        n = L.lib().mmdx_attention_workspace_size(dc, B, Ls, H)
        ws = torch.empty(max(1, n), dtype=torch.uint8, device=dev)
        nl = L.lib().mmdx_attention_lse_workspace_size(dc, B, Ls, H)
        wl = torch.empty(max(1, nl), dtype=torch.uint8, device=dev)
        scale = 1.0 / math.sqrt(64)
        mp = mask.data_ptr() if mask is not None else None

        def fwd():
            L.call("mmdx_attention_fwd", dc, qkv.data_ptr(), mp, B, Ls, H, scale, pd, 0,
                   ctr.data_ptr(), out.data_ptr(), probs.data_ptr(), L.stream())

        def bwd():
            L.call("mmdx_attention_bwd", dc, qkv.data_ptr(), probs.data_ptr(), dout.data_ptr(),
                   mp, B, Ls, H, scale, pd, dqkv.data_ptr(), ws.data_ptr(), n, L.stream())

        def fwd_np():  # inference form: probabilities not saved
            L.call("mmdx_attention_fwd", dc, qkv.data_ptr(), mp, B, Ls, H, scale, 0.0, 0, None,
                   out.data_ptr(), None, L.stream())

        def fwd_lse():
            L.call("mmdx_attention_fwd_lse", dc, qkv.data_ptr(), mp, B, Ls, H, scale, pd, 0,
                   ctr.data_ptr(), out.data_ptr(), lse.data_ptr(), rng.data_ptr(), L.stream())

        def bwd_lse():
            L.call("mmdx_attention_bwd_lse", dc, qkv.data_ptr(), out.data_ptr(), lse.data_ptr(),
                   rng.data_ptr(), dout.data_ptr(), mp, B, Ls, H, scale, pd, dqkv.data_ptr(),
                   wl.data_ptr(), nl, L.stream())
        tf, tb, tn = timeit(fwd, reps), timeit(bwd, reps), timeit(fwd_np, reps)
        tfl, tbl = timeit(fwd_lse, reps), timeit(bwd_lse, reps)
        fl = 4.0 * B * H * Ls * Ls * 64
        pbytes = B * H * Ls * Ls * 4
        print(f"{name:5s} B{B} L{Ls} H{H} p{pd}: fwd {tf:7.1f} us ({fl / tf / 1e6:6.1f} TF, P "
              f"{pbytes / tf / 1e3:6.1f} GB/s)  bwd {tb:7.1f} us ({2 * fl / tb / 1e6:6.1f} TF)  "
              f"fwd w/o P {tn:7.1f} us  fwd_lse {tfl:7.1f} us  bwd_lse {tbl:7.1f} us",
              flush=True)


DIGEST_SHAPES = ((3, 37, 2), (4, 129, 6), (1, 256, 1), (1, 1, 3), (2, 197, 4))
DT_NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
SEED, COUNTER = 77, 3   # a non-zero launch counter: the high half of the stream base is live


def digest(L, dev):
    st = L.stream()

    def show(tag, **tensors):
        torch.cuda.synchronize()
        for k, t in tensors.items():
            h = hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
            print(f"{tag} {k} {h.hexdigest()}", flush=True)

    def counter():
        return torch.full((1,), COUNTER, dtype=torch.int64, device=dev)

    def attention(dt, B, Ls, H, masked, pd, bias_causal=False):
        g = torch.Generator().manual_seed(B * Ls + H + int(pd * 100))
        dc = L.dtype_code(dt)
        qkv = torch.randn(B, Ls, 3, H, 64, generator=g).to(dev, dt)
        mask = None
        if masked:
            lens = torch.randint(1, Ls + 1, (B,), generator=g)
            mask = (torch.arange(Ls)[None] < lens[:, None]).long().to(dev)
        dout = torch.randn(B, Ls, H, 64, generator=g).to(dev, dt)
        bias = torch.randn(H, Ls, Ls, generator=g).to(dev) if bias_causal else None
        mp = mask.data_ptr() if mask is not None else None
        tag = (f"{DT_NAME[dt]} B{B} L{Ls} H{H} mask{int(masked)} p{pd}"
               f"{' bias+causal' if bias_causal else ''}")
        # P-saving
        ctr = counter()
        out = torch.zeros(B, Ls, H, 64, dtype=dt, device=dev)
        probs = torch.zeros(B, H, Ls, Ls, device=dev)
        if bias_causal:
            L.call("mmdx_attention_fwd_ex", dc, qkv.data_ptr(), mp, bias.data_ptr(), 1, B, Ls, H,
                   0.125, pd, SEED, ctr.data_ptr(), out.data_ptr(), probs.data_ptr(), st)
        else:
            L.call("mmdx_attention_fwd", dc, qkv.data_ptr(), mp, B, Ls, H, 0.125, pd, SEED,
                   ctr.data_ptr(), out.data_ptr(), probs.data_ptr(), st)
        dqkv = torch.zeros_like(qkv)
        n = L.lib().mmdx_attention_workspace_size(dc, B, Ls, H)
        ws = torch.zeros(n, dtype=torch.uint8, device=dev)
        L.call("mmdx_attention_bwd", dc, qkv.data_ptr(), probs.data_ptr(), dout.data_ptr(), mp, B,
               Ls, H, 0.125, pd, dqkv.data_ptr(), ws.data_ptr(), n, st)
        show("attn " + tag, out=out, probs=probs, dqkv=dqkv, counter=ctr)
        if pd == 0.0 and not bias_causal:   # inference form: probabilities not saved
            out_np = torch.zeros_like(out)
            L.call("mmdx_attention_fwd", dc, qkv.data_ptr(), mp, B, Ls, H, 0.125, 0.0, SEED, None,
                   out_np.data_ptr(), None, st)
            show("attn_np " + tag, out=out_np)
        if dt == torch.float32 or bias_causal:
            return
        # flash-style
        ctr = counter()
        out = torch.zeros(B, Ls, H, 64, dtype=dt, device=dev)
        lse = torch.zeros(B, H, Ls, device=dev)
        rng = torch.zeros(1, dtype=torch.int64, device=dev)
        L.call("mmdx_attention_fwd_lse", dc, qkv.data_ptr(), mp, B, Ls, H, 0.125, pd, SEED,
               ctr.data_ptr(), out.data_ptr(), lse.data_ptr(), rng.data_ptr(), st)
        dqkv = torch.zeros_like(qkv)
        n = L.lib().mmdx_attention_lse_workspace_size(dc, B, Ls, H)
        ws = torch.zeros(n, dtype=torch.uint8, device=dev)
        L.call("mmdx_attention_bwd_lse", dc, qkv.data_ptr(), out.data_ptr(), lse.data_ptr(),
               rng.data_ptr(), dout.data_ptr(), mp, B, Ls, H, 0.125, pd, dqkv.data_ptr(),
               ws.data_ptr(), n, st)
        show("attn_lse " + tag, out=out, lse=lse, rng=rng, dqkv=dqkv, D=ws, counter=ctr)

    def dropout_stream(dt):
        g = torch.Generator().manual_seed(5)
        dc = L.dtype_code(dt)
        tag = DT_NAME[dt]
        # cross-attention as T5 uses it: 16 condition tokens
        B, Lq, Lk, H = 3, 37, 16, 2
        q = torch.randn(B, Lq, H * 64, generator=g).to(dev, dt)
        kv = torch.randn(B, Lk, 2, H, 64, generator=g).to(dev, dt)
        for pd in (0.0, 0.1):
            ctr = counter()
            out = torch.zeros(B, Lq, H, 64, dtype=dt, device=dev)
            probs = torch.zeros(B, H, Lq, Lk, device=dev)
            L.call("mmdx_xattn_fwd", dc, q.data_ptr(), H * 64, kv.data_ptr(), B, Lq, Lk, H, 0.125,
                   pd, SEED, ctr.data_ptr(), out.data_ptr(), probs.data_ptr(), st)
            show(f"xattn {tag} p{pd}", out=out, probs=probs, counter=ctr)
        # plain dropout and LayerNorm(dropout(x) + residual)
        rows, D, p = 37, 768, 0.1
        x = torch.randn(rows, D, generator=g).to(dev, dt)
        res = torch.randn(rows, D, generator=g).to(dev, dt)
        dy = torch.randn(rows, D, generator=g).to(dev, dt)
        gam = torch.randn(D, generator=g).to(dev)
        bet = torch.randn(D, generator=g).to(dev)
        ctr = counter()
        y = torch.zeros_like(x)
        keep = torch.zeros(rows, D, dtype=torch.uint8, device=dev)
        L.call("mmdx_dropout_fwd", dc, x.data_ptr(), x.numel(), p, SEED, 11, ctr.data_ptr(),
               y.data_ptr(), keep.data_ptr(), st)
        show(f"dropout {tag}", y=y, mask=keep, counter=ctr)
        ctr = counter()
        y, xs = torch.zeros_like(x), torch.zeros_like(x)
        mean, rstd = torch.zeros(rows, device=dev), torch.zeros(rows, device=dev)
        rng = torch.zeros(1, dtype=torch.int64, device=dev)
        L.call("mmdx_layernorm_fwd_dropout", dc, x.data_ptr(), res.data_ptr(), rows, D,
               gam.data_ptr(), bet.data_ptr(), 1e-12, p, SEED, ctr.data_ptr(), y.data_ptr(),
               xs.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rng.data_ptr(), st)
        n = L.lib().mmdx_layernorm_workspace_size(rows, D)
        ws = torch.zeros(n, dtype=torch.uint8, device=dev)
        dx, dxd = torch.zeros_like(x), torch.zeros_like(x)
        dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        L.call("mmdx_layernorm_bwd_dropout", dc, xs.data_ptr(), dy.data_ptr(), rows, D,
               gam.data_ptr(), mean.data_ptr(), rstd.data_ptr(), p, rng.data_ptr(), dx.data_ptr(),
               dxd.data_ptr(), dg.data_ptr(), db.data_ptr(), 0.0, ws.data_ptr(), n, st)
        show(f"ln_dropout {tag}", y=y, xsum=xs, mean=mean, rstd=rstd, rng=rng, dx=dx,
             dx_drop=dxd, dgamma=dg, dbeta=db, counter=ctr)

    for dt in (torch.bfloat16, torch.float16, torch.float32):
        for B, Ls, H in DIGEST_SHAPES:
            for masked, pd in ((False, 0.0), (True, 0.0), (False, 0.1), (True, 0.1)):
                attention(dt, B, Ls, H, masked, pd)
        attention(dt, 3, 37, 2, False, 0.1, bias_causal=True)
        dropout_stream(dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--digest", action="store_true",
                    help="print a sha256 per output tensor at small seeded shapes; no timing")
    a = ap.parse_args()
    import mmdx  # noqa: F401
    from mmdx import _lib as L
    dev = torch.device("cuda", 0)
    print(f"library: {L.LIB_PATH}", file=sys.stderr, flush=True)
    if a.digest:
        digest(L, dev)
    else:
        bench(L, dev, a.reps)


if __name__ == "__main__":
    main()
