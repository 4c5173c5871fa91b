"""Shared cases of the retrieval tests: exact integer inputs, unit gaussian inputs with the
derived fp32 accumulation bound, and the host merge of sliced searches."""
import functools

import numpy as np
import torch

from mmdx.retrieval import reference_search

R = 128   # index rows per block step of the select kernel (mmdx_topk_rows_per_block)
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}

# (N, d, nq, k, with_exclude): every N in {1, 2, 15, 16, 17, 63, 64, 65, R-1, R, R+1, 2R+1, 5000},
# d in {32, 96, 1024}, nq in {1, 2, 16, 17, 64}, k in {1, 5, 64} appears, the corners together;
# k > N with and without exclude.  Two more paths of the kernel: d = 2048 (the queries are
# staged in more than one segment; the largest d at which integer dots stay below 2^24) and
# N = 512 R + R + 1 (more chunks than select blocks: a block walks several chunks).
EXACT = [
    (1, 32, 1, 1, False), (1, 32, 64, 64, True), (2, 96, 2, 5, False), (15, 32, 16, 64, True),
    (16, 96, 17, 1, False), (17, 1024, 1, 5, True), (63, 32, 64, 5, False),
    (64, 1024, 2, 64, True), (65, 96, 16, 1, True), (R - 1, 32, 17, 64, False),
    (R, 1024, 64, 1, True), (R + 1, 96, 1, 64, False), (2 * R + 1, 1024, 17, 5, True),
    (5000, 32, 1, 1, False), (5000, 96, 16, 5, True), (5000, 1024, 64, 64, True),
    (300, 2048, 17, 5, True), (512 * R + R + 1, 32, 2, 5, True),
]

# Seeds of the gaussian cases: the first three of 0, 1, 2, ... at which at least 14 of the 17
# queries have their first six REFERENCE scores separated by more than the bounds (counted on
# the CPU from the reference alone: fp16 17 / 16 / 15, fp32 16 / 16 / 15 of 17 at seeds 0, 1, 2;
# bf16 15 / 13 / 15 / 14 / 15 / 16 at seeds 0 .. 5, so 1 is left out there).
FLOAT_SEEDS = {"fp16": (0, 1, 2), "bf16": (0, 2, 3), "fp32": (0, 1, 2)}


def int_inputs(N, d, nq, seed=0):
    """Integer values in [-3, 3] as fp32 CPU tensors (exact in fp16 and bf16 as well) and an
    exclude vector that mixes -1 with real rows, the first and the last among them."""
    g = np.random.default_rng(seed + 1000 * N + d + nq)
    x = g.integers(-3, 4, (N, d)).astype(np.float32)
    q = g.integers(-3, 4, (nq, d)).astype(np.float32)
    ex = g.integers(-1, N, nq).astype(np.int32)
    ex[0] = N - 1
    if nq > 1:
        ex[1] = 0
    if nq > 2:
        ex[2] = -1
    return torch.from_numpy(q), torch.from_numpy(x), torch.from_numpy(ex)


@functools.lru_cache(maxsize=None)
def exact_case(i):
    """(q, x, exclude or None, k, reference scores, reference ids) of EXACT[i], computed once."""
    N, d, nq, k, with_ex = EXACT[i]
    q, x, ex = int_inputs(N, d, nq)
    ex = ex if with_ex else None
    s, ids = reference_search(q, x, k, ex)
    return q, x, ex, k, s, ids


def gaussian_inputs(N, d, nq, dtype, seed):
    """Gaussian rows of unit length (normalised in fp32), rounded to `dtype` (CPU tensors)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, d, generator=g)
    q = torch.randn(nq, d, generator=g)
    x = x / torch.linalg.vector_norm(x, dim=1, keepdim=True)
    q = q / torch.linalg.vector_norm(q, dim=1, keepdim=True)
    return q.to(dtype), x.to(dtype)


def accumulation_bound(q, x):
    """b[i, j] = gamma_d sum_t |q_t x_jt| with gamma_d = d 2^-24 / (1 - d 2^-24): the bound of a
    length-d fp32 accumulation in any order (products of 16-bit inputs are exact in fp32; fp32
    inputs go through fused multiply-adds: d roundings as well).  Derived, not measured."""
    d = q.shape[1]
    u = 2.0 ** -24
    gamma = d * u / (1.0 - d * u)
    a = q.float().numpy().astype(np.float64)
    b = x.float().numpy().astype(np.float64)
    return gamma * (np.abs(a) @ np.abs(b).T)


def score_matrix(q, x):
    """The float64 scores of every (query, row) pair on the stored values."""
    return q.float().numpy().astype(np.float64) @ x.float().numpy().astype(np.float64).T


def separated_queries(S, B, k):
    """The queries whose first k + 1 reference scores are pairwise separated by more than the
    sum of the two rows' bounds (consecutive ones suffice: the scores are sorted)."""
    ok = []
    for i in range(S.shape[0]):
        order = np.argsort(-S[i], kind="stable")[:k + 1]
        gaps = S[i, order[:-1]] - S[i, order[1:]]
        ok.append(bool(np.all(gaps > B[i, order[:-1]] + B[i, order[1:]])))
    return ok


def merge_host(parts, k):
    """parts: list of (scores [nq, k'] fp32 numpy, global ids [nq, k'] int64 numpy, -1 = empty).
    The first k under (score descending, id ascending) per query, padded with (-inf, -1)."""
    s = np.concatenate([p[0] for p in parts], axis=1)
    ids = np.concatenate([p[1] for p in parts], axis=1)
    nq = s.shape[0]
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        keep = np.flatnonzero(ids[i] >= 0)
        order = keep[np.lexsort((ids[i, keep], -s[i, keep].astype(np.float64)))][:k]
        out_s[i, :order.size] = s[i, order]
        out_i[i, :order.size] = ids[i, order]
    return out_s, out_i
