"""fp64 CPU reference for the attention kernels of csrc/attention.hip (mmdx_attention_fwd,
_fwd_ex, _bwd, _fwd_lse, _bwd_lse) and csrc/t5.hip (mmdx_xattn_fwd / _bwd, mmdx_t5_decode_attn,
mmdx_t5_position_bias / _bwd): torch and numpy only.  Inputs are the tensors the kernel sees,
already rounded to the compute dtype; all arithmetic is in double; every backward is
torch.autograd through this file's forward.

The contract of the self-attention kernels, as this reference states it:
  * S = scale Q K^T + bias[h, q, k].  A masked key's score IS MASK_NEG = -1e30f: the kernels
    add -1e30f in fp32, which absorbs every finite score (and the bias).  causal REPLACES the
    score of key > q by MASK_NEG.  Keys beyond L do not exist (-inf).
  * A row whose allowed keys are all masked therefore has L equal scores and P = 1 / L over ALL
    L keys, the causal-hidden ones included (a fully padded batch row: every query of it).
  * The backward treats both masks as additive constants: dS = P o (dP - rowsum(P o dP)) flows
    into dQ and dK for masked cells too (they have P = 0 unless the whole row is masked).  The
    reference reproduces that by giving a blocked score the value MASK_NEG and the derivative 1.
  * P' = P keep / (1 - p), O = P' V; the saved probabilities carry the keep bit in their sign.
  * lse = log sum exp S (in fp32 a fully masked row's lse is MASK_NEG itself: log L is
    absorbed; the bound h_T |lse| covers that), D = rowsum(dO o O).
mmdx_t5_position_bias_bwd sums dS over the batch and the cells k <= q of each bucket; cells
k > q are never read (the decoder's self-attention is causal, their dS is zero; the GPU test
fills them with NaN).

Each result carries the sums of |terms| of the fp32 accumulations that produce it, and
bounds() turns them into per-element error bounds built from the reference alone: h_T |ref|
for the store, ACC sum |terms| per accumulation (conv_ref's constants), the unit roundoff of
the 16-bit P' and dS operands times the same sums, the device's __expf / __logf error as
EXPF_C / LOGF_C times 2^-24 (1 + |argument|), and the softmax's first-order sensitivity to the
score error, and FLOOR, the absolute error of a rounding that underflows.

keep_mask() mirrors csrc/dropout_rng.h on the host; attn_lp(), blocks_per_head(),
block_order() and the constants mirror the launch geometry, and edges() names from them the
tile / block / mask edges a self-attention case reaches."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from conv_ref import ACC, BF16, F16, F32, H_T, assert_exact, bound_ratio  # noqa: F401

DT_NAME = {BF16: "bf16", F16: "f16", F32: "f32"}
NAN = float("nan")
MASK_NEG = float(np.float32(-1e30))
U24 = 2.0 ** -24
# absolute floor of one rounding: half the subnormal spacing of fp16; fp32 and bf16 values below
# the smallest normal may be flushed to zero
FLOOR = {F32: 2.0 ** -126, BF16: 2.0 ** -126, F16: 2.0 ** -25}

# the device's __expf / __logf against fp64, in units of 2^-24 (1 + |argument|): twice the
# largest value measured on an MI355X (tests/test_attention_reference_gpu.py records them)
EXPF_C = 2 * 1.19
LOGF_C = 2 * 0.375

# ------------------------------------------------------------------ launch-geometry mirrors
HD = 64
MAXKT = 16          # 16-key tiles: L <= 256
NW32 = 2            # waves of an fp32 block
BLOCK32 = NW32 * 16  # query (key) rows of an fp32 block
QC = 32             # query chunk of attn_bwd_kv_kernel
XA_MAXK = 16        # cross-attention keys
DEC_MAXL = 512      # decode positions


def attn_lp(L):
    return (L + 31) & ~31


def blocks_per_head(L, nw):
    return (L + nw * 16 - 1) // (nw * 16)


def workspace_size(dt, B, L, H):
    return B * H * L * attn_lp(L) * (4 if dt == F32 else 2)


def lse_workspace_size(dt, B, L, H):
    return B * H * L * 4


def xattn_workspace_size(B, Lq, Lk, H):
    return 2 * B * H * Lq * Lk * 4


def xcd_grouped(B, H):
    """attn_block takes the XCD-grouped block order when B * H is a multiple of 8."""
    return (B * H) % 8 == 0


def block_order(B, H, L, nw):
    """attn_block: (blk, h, b) of linear block id n."""
    nb = blocks_per_head(L, nw)
    out = []
    for n in range(nb * B * H):
        if xcd_grouped(B, H):
            k = n >> 3
            blk, hl = k % nb, (k // nb) * 8 + (n & 7)
        else:
            blk, hl = n % nb, n // nb
        out.append((blk, hl % H, hl // H))
    return out


def fwd_nw(dt, entry, knobs):
    """Waves of the forward block: fp32 2; P-saving 16-bit 8 (knob 4); flash-style 8 (4 | 16)."""
    if dt == F32:
        return NW32
    v = int(knobs.get("MMDX_ATTN_FWD_NW", 8))
    if entry == "lse":
        return v if v in (4, 16) else 8
    return 4 if v == 4 else 8


def bwd_q_nw(dt, entry, knobs):
    if dt == F32:
        return NW32
    if entry == "lse":
        return 8
    return 4 if int(knobs.get("MMDX_ATTN_BWD_NW", 8)) == 4 else 8


def edges(dt, B, L, H, mask_kind, knobs=None):
    """Names of the edges a self-attention case reaches."""
    knobs = knobs or {}
    e = set()
    LP = attn_lp(L)
    if L < LP:
        e.add("lp-pad")
    if LP - L >= 16:
        e.add("dead-key-tile")
    if L % 16:
        e.add("ragged-key-tile")
    if L in (32, 33):
        e.add("lp-step")
    if L % 4:
        e.add("prob-transpose")
    if LP // 16 == MAXKT:
        e.add("all-key-tiles")
    for nw, name in ((2, "block32"), (4, "block64"), (8, "block128"), (16, "block256")):
        if L % (nw * 16) in (0, 1, nw * 16 - 1):
            e.add(name + "-edge")
    if L > QC and L % QC:
        e.add("ragged-chunk")
    for entry in ("psave", "lse"):
        nw = fwd_nw(dt, entry, knobs)
        if dt != F32 and blocks_per_head(L, nw) * nw * 16 - L >= 16:
            e.add("idle-waves")
        if dt != F32 and blocks_per_head(L, nw) > 1:
            e.add("multi-block")
    e.add("xcd-grouped" if xcd_grouped(B, H) else "linear-order")
    e.add("mask-" + mask_kind)
    return e


# ------------------------------------------------------------------------ the dropout stream
_M64 = (1 << 64) - 1


def dropout_mix(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xff51afd7ed558ccd)
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xc4ceb9fe1a85ec53)
        x = x ^ (x >> np.uint64(33))
    return (x & np.uint64(0xffffffff)).astype(np.uint32)


def dropout_stream_base(seed, counter):
    """seed * golden ratio + (counter << 32) mod 2^64; counter None: the seed alone."""
    base = (int(seed) * 0x9E3779B97F4A7C15) & _M64
    if counter is not None:
        base = (base + ((int(counter) << 32) & _M64)) & _M64
    return base


def keep_from_base(base, idx, p):
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        bits = dropout_mix(np.uint64(base) + idx)
    u = (bits >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(p)


def keep_mask(seed, counter, idx, p):
    """dropout_keep(dropout_stream_base(seed, &counter), idx, p) for an array of indices."""
    return keep_from_base(dropout_stream_base(seed, counter), idx, p)


def self_keep(seed, counter, B, H, L, p, base=None):
    """[B, H, L, L] bool: element ((b*H + h)*L + q)*L + key of the launch's stream."""
    if not p > 0:
        return torch.ones(B, H, L, L, dtype=torch.bool)
    idx = np.arange(B * H * L * L, dtype=np.uint64)
    k = keep_from_base(dropout_stream_base(seed, counter) if base is None else base, idx, p)
    return torch.from_numpy(k.reshape(B, H, L, L))


def cross_keep(seed, counter, B, H, Lq, Lk, p):
    """[B, H, Lq, Lk] bool: element ((b*H + h)*Lq + q)*Lk + key."""
    if not p > 0:
        return torch.ones(B, H, Lq, Lk, dtype=torch.bool)
    idx = np.arange(B * H * Lq * Lk, dtype=np.uint64)
    return torch.from_numpy(keep_mask(seed, counter, idx, p).reshape(B, H, Lq, Lk))


# ---------------------------------------------------------------------------- the reference
def _core(q, k, v, dout, scale, bias, blocked, keep, p):
    """q, dout [B, Lq, H, 64]; k, v [B, Lk, H, 64]; bias broadcastable to [B, H, Lq, Lk] or
    None; blocked bool, broadcastable, or None; keep [B, H, Lq, Lk] bool or None."""
    q, k, v = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    do = dout.double()
    B, Lq, H, _ = q.shape
    Lk = k.shape[1]
    S0 = scale * torch.einsum("bqhd,bkhd->bhqk", q, k)
    if bias is not None:
        S0 = S0 + bias.double()
    S0.retain_grad()
    if blocked is not None:
        blocked = blocked.expand(B, H, Lq, Lk)
        # value MASK_NEG exactly, derivative 1: the kernels' additive constant
        S = torch.where(blocked, MASK_NEG + (S0 - S0.detach()), S0)
    else:
        blocked = torch.zeros(B, H, Lq, Lk, dtype=torch.bool)
        S = S0
    P = torch.softmax(S, -1)
    lse = torch.logsumexp(S, -1)
    ks = 1.0 / (1.0 - p)
    kf = torch.ones_like(P) if keep is None else keep.double()
    Pp = P * kf * ks
    O = torch.einsum("bhqk,bkhd->bqhd", Pp, v)
    O.backward(do)
    r = SimpleNamespace(B=B, Lq=Lq, Lk=Lk, H=H, scale=scale, p=p, ks=ks, keep=kf, blocked=blocked)
    r.q, r.k, r.v, r.do = q.detach(), k.detach(), v.detach(), do
    r.S, r.P, r.Pp, r.lse, r.O = S.detach(), P.detach(), Pp.detach(), lse.detach(), O.detach()
    r.dq, r.dk, r.dv, r.dS = q.grad, k.grad, v.grad, S0.grad
    r.D = (do * r.O).sum(-1).permute(0, 2, 1)                       # [B, H, Lq]
    r.dP = ks * kf * torch.einsum("bqhd,bkhd->bhqk", do, r.v)       # keep * dP' / (1 - p)
    # sums of |terms|
    aq, ak, av, ad = r.q.abs(), r.k.abs(), r.v.abs(), do.abs()
    r.s_terms = scale * torch.einsum("bqhd,bkhd->bhqk", aq, ak)
    if bias is not None:
        r.s_terms = r.s_terms + bias.double().abs()
    r.s_terms = torch.where(blocked, torch.zeros_like(r.s_terms), r.s_terms)
    r.o_terms = torch.einsum("bhqk,bkhd->bqhd", r.Pp.abs(), av)
    r.dp_terms = ks * kf * torch.einsum("bqhd,bkhd->bhqk", ad, av)
    r.dq_terms = scale * torch.einsum("bhqk,bkhd->bqhd", r.dS.abs(), ak)
    r.dk_terms = scale * torch.einsum("bhqk,bqhd->bkhd", r.dS.abs(), aq)
    r.dv_terms = torch.einsum("bhqk,bqhd->bkhd", r.Pp.abs(), ad)
    r.d_terms = (ad * r.O.abs()).sum(-1).permute(0, 2, 1)
    return r


def blocked_mask(B, L, mask, causal):
    """[B, 1, L, L] bool: key masked out, or hidden by causal."""
    blk = torch.zeros(B, 1, L, L, dtype=torch.bool)
    if mask is not None:
        blk = blk | (mask == 0)[:, None, None, :]
    if causal:
        ar = torch.arange(L)
        blk = blk | (ar[None, :] > ar[:, None])[None, None]
    return blk


def self_attention(qkv, dout, scale, mask=None, bias=None, causal=False, keep=None, p=0.0):
    """qkv [B, L, 3, H, 64], dout [B, L, H, 64], mask [B, L] (0 = pad) or None, bias
    [H, L, L] or None.  Returns the _core() namespace plus dqkv [B, L, 3, H, 64] and dS_ws
    [B, H, L, LP] (the workspace of mmdx_attention_bwd: zero in columns [L, LP))."""
    B, L = qkv.shape[:2]
    blk = blocked_mask(B, L, mask, causal) if (mask is not None or causal) else None
    r = _core(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], dout, scale,
              None if bias is None else bias[None], blk, keep, p)
    r.dqkv = torch.stack([r.dq, r.dk, r.dv], 2)
    r.L, r.LP = L, attn_lp(L)
    r.row_blocked = r.blocked.all(-1)                               # [B, H, L]
    return r


def pad_ws(t, LP):
    """[B, H, L, L] -> [B, H, L, LP] with zeros behind."""
    return torch.nn.functional.pad(t, (0, LP - t.shape[-1]))


def cross_attention(q, kv, dout, scale, keep=None, p=0.0):
    """q [B, Lq, H, 64] (the head slices of ldq-wide rows), kv [B, Lk, 2, H, 64]."""
    r = _core(q, kv[:, :, 0], kv[:, :, 1], dout, scale, None, None, keep, p)
    r.dkv = torch.stack([r.dk, r.dv], 2)
    return r


def decode_step(qkv, kc, vc, slots, bias, pos):
    """qkv [R, 3, H, 64] (this step's q, k, v), kc / vc [R, Lmax, H, 64], slots [R, Lmax],
    bias [H, Lmax, Lmax]: key j < pos of row r is cache row slots[r, j], position j; key pos is
    this step's.  Returns the _core() namespace (Lq = 1) plus the caches after the append."""
    R = qkv.shape[0]
    ar = torch.arange(R)
    ks, vs = [], []
    for j in range(pos):
        ks.append(kc[slots[:, j].long(), j])
        vs.append(vc[slots[:, j].long(), j])
    ks.append(qkv[:, 1])
    vs.append(qkv[:, 2])
    k, v = torch.stack(ks, 1), torch.stack(vs, 1)                   # [R, pos + 1, H, 64]
    b = bias[:, pos, :pos + 1][None, :, None, :]
    r = _core(qkv[:, 0][:, None], k, v, torch.zeros(R, 1, *qkv.shape[2:]), 1.0, b, None, None,
              0.0)
    r.kc, r.vc = kc.clone(), vc.clone()
    r.kc[ar, pos], r.vc[ar, pos] = qkv[:, 1], qkv[:, 2]
    return r


def t5_bucket_causal(n, nb, maxd, dtype=torch.float32):
    """transformers' T5Attention._relative_position_bucket (bidirectional = False) of the
    relative positions n >= 0 (a long tensor), its logarithm evaluated in `dtype`."""
    exact = nb // 2
    nf = n.to(dtype).clamp(min=1)
    large = exact + (torch.log(nf / exact) / math.log(maxd / exact) * (nb - exact)).to(torch.long)
    large = torch.minimum(large, torch.full_like(large, nb - 1))
    return torch.where(n < exact, n, large)


def bucket_matrix(L, nb, maxd, dtype=torch.float32):
    ar = torch.arange(L)
    return t5_bucket_causal((ar[:, None] - ar[None, :]).clamp(min=0), nb, maxd, dtype)   # [q, k]


def position_bias(table, L, nb, maxd):
    """table [nb, H] -> bias [H, L, L] = table[bucket(max(q - k, 0))][h]."""
    return table[bucket_matrix(L, nb, maxd)].permute(2, 0, 1).contiguous()


def position_bias_bwd(dS, nb, maxd, dtable0=None, beta=0.0):
    """dS [B, H, L, >= L] -> (dtable [nb, H], sum of |terms|): beta dtable0 + the sum of dS over
    the batch and the cells k <= q of each bucket."""
    B, H, L = dS.shape[:3]
    bk = bucket_matrix(L, nb, maxd)
    ar = torch.arange(L)
    live = (ar[None, :] <= ar[:, None])
    d = dS[..., :L].double()
    d = torch.where(live, d, torch.zeros_like(d)).sum(0)            # [H, L, L]
    out = torch.zeros(nb, H, dtype=torch.float64)
    terms = torch.zeros(nb, H, dtype=torch.float64)
    a = torch.where(live, dS[..., :L].double().abs(), torch.zeros_like(d)).sum(0)
    for b in range(nb):
        sel = (bk == b) & live
        out[b] = d[:, sel].sum(-1)
        terms[b] = a[:, sel].sum(-1)
    if beta != 0.0:
        out = out + beta * dtable0.double()
        terms = terms + abs(beta) * dtable0.double().abs()
    return out, terms


# -------------------------------------------------------------------------------- the bounds
def bounds(r, dt, lse_path=False, fixed_rows=None, round_ops=True):
    """Per-element error bounds of a _core() result for kernels that compute in dt: fp32
    accumulation, P' and dS rounded to dt (16-bit) before their products, outputs stored in dt
    (probabilities, lse, D in fp32).  lse_path: the flash-style backward, which recomputes P
    from the saved lse and takes the row term as D = rowsum(dO o O) of the stored output.
    fixed_rows [B, H, Lq] bool: rows whose P that backward sets to 1 / L itself (all keys
    masked), instead of trusting an lse that absorbed log L.  round_ops = False: P' and dS stay
    in fp32 (the cross-attention and decode kernels)."""
    hT = H_T[dt]
    u16 = 0.0 if dt == F32 or not round_ops else H_T[dt]
    fl, fl32 = FLOOR[dt], FLOOR[F32]
    b = SimpleNamespace()
    mx = r.S.max(-1, keepdim=True).values
    arg = (r.S - mx).clamp(min=-200.0)
    # score error: the accumulation, the scale and bias roundings; a blocked score is exact
    dS_ = ACC * r.s_terms + torch.where(r.blocked, torch.zeros_like(r.S), 3 * U24 * r.S.abs())
    ex = EXPF_C * U24 * (1 + arg.abs()) + U24 * arg.abs()
    rel = dS_ + ex
    avg = (r.P * rel).sum(-1, keepdim=True)
    # |error| of the forward's probabilities
    ep = r.P * (rel + avg + ACC + 4 * U24) + fl32
    epp = ep * r.ks * r.keep + fl                   # ... of P' before its rounding's u16 |P'|
    av, ad = r.v.abs(), r.do.abs()
    b.P = U24 * r.P + ep
    b.out = hT * r.O.abs() + (ACC + u16) * r.o_terms + \
        torch.einsum("bhqk,bkhd->bqhd", epp, av) + fl
    sum_ref = torch.exp(r.lse[..., None] - mx)[..., 0]
    b.lse = U24 * r.lse.abs() + (r.P * dS_).sum(-1) + (r.P * ex).sum(-1) + ACC + \
        LOGF_C * U24 * (1 + sum_ref) + U24 * mx[..., 0].abs()
    ddP = ACC * r.dp_terms + 2 * U24 * r.dP.abs()
    if not lse_path:
        dot = (r.P * r.dP).sum(-1, keepdim=True)
        ddot = (ep * r.dP.abs() + r.P * ddP).sum(-1, keepdim=True) + \
            ACC * (r.P * r.dP.abs()).sum(-1, keepdim=True)
        eds = ep * (r.dP - dot).abs() + r.P * (ddP + ddot) + (2 * U24 + u16) * r.dS.abs() + fl
        b.dv = hT * r.dv.abs() + (ACC + u16) * r.dv_terms + \
            torch.einsum("bhqk,bqhd->bkhd", epp, ad) + fl
    else:
        dl = b.lse
        if fixed_rows is not None:
            fx = (EXPF_C + 1) * U24 * (1 + math.log(r.Lk)) + LOGF_C * U24 * (1 + r.Lk)
            dl = torch.where(fixed_rows, torch.full_like(dl, fx), dl)
        a2 = (r.S - r.lse[..., None]).clamp(min=-200.0).abs()
        rel2 = dS_ + dl[..., None] + (EXPF_C + 1) * U24 * (1 + a2) + 4 * U24
        ep2 = r.P * rel2 + fl32
        dD = (ad * b.out).sum(-1).permute(0, 2, 1) + ACC * r.d_terms
        b.D = U24 * r.D.abs() + dD
        eds = ep2 * (r.dP - r.D[..., None]).abs() + r.P * (ddP + dD[..., None]) + \
            (2 * U24 + u16) * r.dS.abs() + fl
        ep2p = ep2 * r.ks * r.keep + fl
        b.dv = hT * r.dv.abs() + (ACC + u16) * r.dv_terms + \
            torch.einsum("bhqk,bqhd->bkhd", ep2p, ad) + fl
    b.dS = eds
    b.dq = hT * r.dq.abs() + ACC * r.dq_terms + \
        r.scale * torch.einsum("bhqk,bkhd->bqhd", eds, r.k.abs()) + fl
    b.dk = hT * r.dk.abs() + ACC * r.dk_terms + \
        r.scale * torch.einsum("bhqk,bqhd->bkhd", eds, r.q.abs()) + fl
    return b


def check_bounded(kind, got, ref, bound, what):
    """|got - ref| <= bound, element by element; prints 'attnref <kind> <error / bound>
    <case>' first and returns the ratio."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: {kind} shape {tuple(got.shape)} != {tuple(ref.shape)}"
    ratio = bound_ratio(got, ref, bound)
    print(f"attnref {kind} {ratio:.4f} {what}")
    assert ratio <= 1.0, f"{what}: {kind} error / bound = {ratio:.3f}"
    return ratio


def ratio_only(got, ref, bound):
    """check_bounded's ratio without its assertions: inf for a non-finite value or an error
    where the bound is zero."""
    got = got.detach().double().cpu()
    if got.shape != ref.shape or not torch.isfinite(got).all():
        return float("inf")
    err = (got - ref).abs()
    zero = bound == 0
    if (err[zero] != 0).any():
        return float("inf")
    return (err[~zero] / bound[~zero]).max().item() if (~zero).any() else 0.0
