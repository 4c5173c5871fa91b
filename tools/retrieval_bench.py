"""Time the similar-case search (functional.topk_similar: two launches, select + merge) against
(a) torch's own matmul + topk on the same tensors and (b) a device-to-device copy that moves as
many bytes as the index read.

    python tools/retrieval_bench.py [--n 262144] [--d 1024] [--out FILE] [--parity FILE]

Default shape: N = 2^18, d = 1024 (512 MB in 16-bit, past the 256 MiB Infinity Cache), k in
{5, 64}, nq in {1, 16, 64}, fp16 and bf16; unit gaussian rows.  Device events around one call
each, after a warm-up of every shape; the three sides alternate sample by sample, so a drift of
the shared machine hits all of them; medians of 20 with min and max.  The kernel is timed
through the C entry point with its workspace allocated beforehand (device work on both sides).
The copy moves N * d * size bytes once (read + write): the index is read once per group of 16
queries, so at nq = 64 the kernel reads four times the copy's bytes.  The ids are checked
against torch's before anything is timed (equal where torch's scores are separated).
Expectations, each marked met or missed: kernel faster than (a) at every shape; at nq <= 16
within a small multiple (3x) of (b).

--parity FILE: worst |score - float64 reference| / derived bound on the gaussian cases that
tests/test_retrieval_gpu.py asserts.  Needs a GPU."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mmdx  # noqa: E402,F401
import mmdx.functional as F  # noqa: E402
from mmdx import _lib as L  # noqa: E402

SAMPLES, COPY_MULTIPLE = 20, 3.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3   # us


def bench(N, d, out):
    dev = torch.device("cuda:0")
    lines = [f"Similar-case search vs torch matmul + topk vs a copy of the index bytes; "
             f"N = {N}, d = {d}, {torch.cuda.get_device_name(0)}; medians of {SAMPLES} (us)"]
    met_all = True
    for dtype in (torch.float16, torch.bfloat16):
        g = torch.Generator().manual_seed(0)
        x = torch.empty((N, d), dtype=dtype, device=dev)
        for s in range(0, N, 1 << 16):   # filled in pieces: no fp32 copy of the whole index
            e = min(N, s + (1 << 16))
            r = torch.randn(e - s, d, generator=g)
            x[s:e] = (r / torch.linalg.vector_norm(r, dim=1, keepdim=True)).to(dtype).to(dev)
        dst = torch.empty_like(x)
        index_mb = x.numel() * x.element_size() / 1e6
        for nq in (1, 16, 64):
            r = torch.randn(nq, d, generator=g)
            q = (r / torch.linalg.vector_norm(r, dim=1, keepdim=True)).to(dtype).to(dev)
            for k in (5, 64):
                need = int(L.lib().mmdx_topk_similar_workspace_size(N, d, nq, k))
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
                sc = torch.empty((nq, k), dtype=torch.float32, device=dev)
                ids = torch.empty((nq, k), dtype=torch.int32, device=dev)
                st, dt = L.stream(), L.dtype_code(dtype)

                def kern():
                    L.call("mmdx_topk_similar", st, dt, q.data_ptr(), x.data_ptr(), N, d, nq, k,
                           None, sc.data_ptr(), ids.data_ptr(), ws.data_ptr(), need)

                def torch_side():
                    return torch.topk(q @ x.T, k, dim=1)

                def copy():
                    dst.copy_(x)

                kern()
                ts, ti = torch_side()
                same = (ti == ids.long()).all(dim=1).float().mean().item()
                worst = (ts.float() - sc).abs().max().item()
                for fn in (kern, torch_side, copy):   # warm-up of every shape
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                t = {"kernel": [], "torch": [], "copy": []}
                for _ in range(SAMPLES):
                    t["kernel"].append(timed(kern))
                    t["torch"].append(timed(torch_side))
                    t["copy"].append(timed(copy))
                med = {n: float(np.median(v)) for n, v in t.items()}
                a_met = med["kernel"] < med["torch"]
                b_met = nq > 16 or med["kernel"] <= COPY_MULTIPLE * med["copy"]
                met_all &= a_met and b_met
                reads = -(-nq // 16)
                name = str(dtype).replace("torch.", "")
                lines.append(
                    f"{name:8s} nq {nq:2d} k {k:2d}: kernel {med['kernel']:8.1f} (min "
                    f"{min(t['kernel']):8.1f} max {max(t['kernel']):8.1f})  torch "
                    f"{med['torch']:8.1f}  copy {med['copy']:8.1f} | kernel / torch "
                    f"{med['kernel'] / med['torch']:5.2f} ({'met' if a_met else 'MISSED'}: < 1)  "
                    f"kernel / copy {med['kernel'] / med['copy']:5.2f} ("
                    f"{'met' if b_met else 'MISSED'}"
                    + (": <= 3 at nq <= 16)" if nq <= 16 else
                       f": no expectation, {reads} index reads)") +
                    f"  index read {reads * index_mb / med['kernel']:6.2f} TB/s | rows "
                    f"with torch's ids {same:4.2f}, max |score - torch| {worst:.1e}")
                print(lines[-1], flush=True)
        del x, dst
    text = "\n".join(lines) + "\n"
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    return met_all


def parity(out):
    import retrieval_cases as RC
    FLOAT_SEEDS = RC.FLOAT_SEEDS
    dev = torch.device("cuda:0")
    lines = ["Similar-case search against the float64 reference: unit gaussian rows, N = 5000, "
             "d = 1024, nq = 17; bound b = gamma_d sum |q x|, gamma_d = d 2^-24 / (1 - d 2^-24) "
             f"(derived); {torch.cuda.get_device_name(0)}"]
    for name, dtype in RC.DTYPES.items():
        for seed in FLOAT_SEEDS[name]:
            q, x = RC.gaussian_inputs(5000, 1024, 17, dtype, seed)
            S, B = RC.score_matrix(q, x), RC.accumulation_bound(q, x)
            sep = sum(RC.separated_queries(S, B, 5))
            for k in (5, 64):
                s, i = F.topk_similar(q.to(dev), x.to(dev), k)
                s, i = s.cpu().numpy().astype(np.float64), i.cpu().numpy().astype(np.int64)
                rows = np.arange(17)[:, None]
                err, bound = np.abs(s - S[rows, i]), B[rows, i]
                lines.append(f"{name} seed {seed} k {k:2d}: worst error / bound "
                             f"{(err / bound).max():.4f}  worst error {err.max():.2e}  largest "
                             f"bound {B.max():.2e}  separated queries {sep} of 17")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_kernels.txt"))
    ap.add_argument("--parity", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("retrieval_bench needs a GPU")
    if a.parity:
        parity(a.parity)
        return 0
    bench(a.n, a.d, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
