"""CPU checks of tests/attention_ref.py and tests/attention_cases.py: the reference against a
triple-loop definition and finite differences, the case table against the launch-geometry
mirrors, the exactness preconditions of every exact case, the dropout mirror, and the
well-posedness of the Gaussian bounds: a plain fp32 torch emulation of each kernel's
arithmetic (same order of roundings, P' and dS rounded to 16 bits where the kernels round)
passes every bound, and five emulations that change arithmetic only fail exactly the cases
that reach the changed code."""
import functools
import math

import numpy as np
import pytest
import torch

import attention_cases as C
import attention_ref as R
from attention_ref import F32

GAUSS_SELF = [c.id for c in C.CASES if c.kind == "self" and "gauss" in c.families and not c.knobs]
MASK32 = torch.tensor(-1e30, dtype=torch.float32)


# ------------------------------------------------------------------- reference vs definition
def _loops(qkv, dout, scale, mask, bias, causal, keep, p):
    """O, P, lse by the definition, one (b, h, q) at a time, in Python floats."""
    B, L, _, H, D = qkv.shape
    O = torch.zeros(B, L, H, D, dtype=torch.float64)
    P = torch.zeros(B, H, L, L, dtype=torch.float64)
    lse = torch.zeros(B, H, L, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            for q in range(L):
                s = []
                for k in range(L):
                    v = scale * sum(qkv[b, q, 0, h, d].item() * qkv[b, k, 1, h, d].item()
                                    for d in range(D))
                    if bias is not None:
                        v += bias[h, q, k].item()
                    if (mask is not None and mask[b, k] == 0) or (causal and k > q):
                        v = R.MASK_NEG
                    s.append(v)
                m = max(s)
                e = [math.exp(v - m) for v in s]
                z = sum(e)
                lse[b, h, q] = m + math.log(z)
                for k in range(L):
                    P[b, h, q, k] = e[k] / z
                    pe = P[b, h, q, k] * (1.0 if keep[b, h, q, k] else 0.0) / (1 - p)
                    O[b, q, h] += pe * qkv[b, k, 2, h]
    return O, P, lse


@pytest.mark.parametrize("mask,bias,causal,p", [(None, False, False, 0.0),
                                                ("holes", True, True, 0.5),
                                                ("padded", False, True, 0.0)])
def test_reference_is_the_definition(mask, bias, causal, p):
    g = torch.Generator().manual_seed(3)
    B, L, H = 3, 5, 2
    qkv = torch.randn(B, L, 3, H, 64, generator=g, dtype=torch.float64)
    dout = torch.randn(B, L, H, 64, generator=g, dtype=torch.float64)
    m = C.make_mask(mask, B, L) if mask else None
    bs = torch.randn(H, L, L, generator=g, dtype=torch.float64) if bias else None
    keep = torch.rand(B, H, L, L, generator=g) >= p
    r = R.self_attention(qkv, dout, 0.125, m, bs, causal, keep, p)
    O, P, lse = _loops(qkv, dout, 0.125, m, bs, causal, keep, p)
    assert (r.O - O).abs().max() < 1e-12 and (r.P - P).abs().max() < 1e-14
    assert (r.lse - lse).abs().max() <= 1e-12 * lse.abs().max()
    if mask == "padded":
        # the contract: a row with every allowed key masked is uniform over all L keys
        assert torch.equal(r.P[1], torch.full_like(r.P[1], 1.0 / L))
        assert (r.lse[1] == R.MASK_NEG + math.log(L)).all()
    assert torch.allclose(r.D, (dout * r.O).sum(-1).permute(0, 2, 1))
    dot = (r.P * r.dP).sum(-1, keepdim=True)
    assert (r.dS - r.P * (r.dP - dot)).abs().max() < 1e-12


def test_gradients_are_finite_differences():
    g = torch.Generator().manual_seed(5)
    B, L, H = 2, 6, 1
    qkv = torch.randn(B, L, 3, H, 64, generator=g, dtype=torch.float64) * 0.5
    dout = torch.randn(B, L, H, 64, generator=g, dtype=torch.float64)
    # no row has all of its allowed keys masked: there the kernels' derivative (1, an additive
    # constant) is not the value's (0), see attention_ref's docstring; elsewhere P = 0 on
    # every masked cell and the two agree
    m = C.make_mask("prefix", B, L)
    bs = torch.randn(H, L, L, generator=g, dtype=torch.float64)
    keep = torch.rand(B, H, L, L, generator=g) >= 0.5
    f = lambda x: (R.self_attention(x, dout, 0.125, m, bs, True, keep, 0.5).O * dout).sum()  # noqa
    r = R.self_attention(qkv, dout, 0.125, m, bs, True, keep, 0.5)
    gi = torch.Generator().manual_seed(6)
    for _ in range(24):
        idx = tuple(int(torch.randint(0, n, (1,), generator=gi)) for n in qkv.shape)
        e = torch.zeros_like(qkv)
        e[idx] = 1e-5
        fd = (f(qkv + e) - f(qkv - e)).item() / 2e-5
        assert abs(fd - r.dqkv[idx].item()) <= 1e-7 * max(1.0, abs(fd)), (idx, fd, r.dqkv[idx])
    # the bias gradient is the score gradient
    e = torch.zeros_like(bs)
    e[0, 3, 1] = 1e-5
    fb = lambda b_: (R.self_attention(qkv, dout, 0.125, m, b_, True, keep, 0.5).O * dout).sum()  # noqa
    fd = (fb(bs + e) - fb(bs - e)).item() / 2e-5
    assert abs(fd - r.dS[:, 0, 3, 1].sum().item()) <= 1e-7 * max(1.0, abs(fd))


def test_cross_and_decode_reduce_to_self_attention():
    g = torch.Generator().manual_seed(8)
    B, L, H = 2, 7, 2
    qkv = torch.randn(B, L, 3, H, 64, generator=g, dtype=torch.float64)
    dout = torch.randn(B, L, H, 64, generator=g, dtype=torch.float64)
    r = R.self_attention(qkv, dout, 0.125)
    x = R.cross_attention(qkv[:, :, 0], qkv[:, :, 1:], dout, 0.125)
    assert torch.equal(x.O, r.O) and torch.equal(x.dq, r.dq) and torch.equal(x.dkv, r.dqkv[:, :, 1:])
    # decode at position L - 1 of a causal run: the last row of causal self-attention
    bias = torch.randn(H, L, L, generator=g, dtype=torch.float64)
    rc = R.self_attention(qkv, dout, 1.0, None, bias, True)
    slots = torch.arange(B)[:, None].expand(B, L).to(torch.int32)
    d = R.decode_step(qkv[:, L - 1], qkv[:, :, 1].clone(), qkv[:, :, 2].clone(), slots, bias,
                      L - 1)
    assert (d.O[:, 0] - rc.O[:, L - 1]).abs().max() < 1e-13
    assert torch.equal(d.kc[:, L - 1], qkv[:, L - 1, 1])


@pytest.mark.parametrize("nb,maxd,L", sorted({(c.nb, c.maxd, c.L) for c in C.CASES
                                              if c.kind == "posbias"}))
def test_bucket_fp32_is_fp64(nb, maxd, L):
    b32, b64 = R.bucket_matrix(L, nb, maxd), R.bucket_matrix(L, nb, maxd, torch.float64)
    assert torch.equal(b32, b64)
    assert b32.max() == nb - 1 and b32[0, L - 1] == 0 and (b32.diff(dim=0) >= 0).all()
    dS = torch.randn(2, 3, L, L + 5, dtype=torch.float64)
    got, terms = R.position_bias_bwd(dS, nb, maxd)
    want = torch.zeros(nb, 3, dtype=torch.float64)
    for q in range(L):
        for k in range(q + 1):
            want[b32[q, k]] += dS[:, :, q, k].sum(0)
    assert (got - want).abs().max() < 1e-11 and (terms >= got.abs() - 1e-11).all()


# ---------------------------------------------------------------------------- dropout mirror
def _mix_scalar(x):
    m = (1 << 64) - 1
    x ^= x >> 33
    x = x * 0xff51afd7ed558ccd & m
    x ^= x >> 33
    x = x * 0xc4ceb9fe1a85ec53 & m
    x ^= x >> 33
    return x & 0xffffffff


def test_keep_mask_is_self_consistent():
    seed, ctr, p = C.SEED, C.COUNTER0, 0.5
    base = R.dropout_stream_base(seed, ctr)
    assert base == (seed * 0x9E3779B97F4A7C15 + (ctr << 32)) % 2 ** 64
    assert R.dropout_stream_base(seed, None) == seed * 0x9E3779B97F4A7C15 % 2 ** 64
    idx = np.array([0, 1, 2, 255, 2 ** 31, 2 ** 40 + 3], dtype=np.uint64)
    want = [(_mix_scalar((base + int(i)) % 2 ** 64) >> 8) * 2.0 ** -24 >= p for i in idx]
    assert R.keep_mask(seed, ctr, idx, p).tolist() == want
    k = R.self_keep(seed, ctr, 2, 2, 64, p)
    assert abs(k.double().mean().item() - 0.5) < 0.02
    assert not torch.equal(k, R.self_keep(seed, ctr + 1, 2, 2, 64, p))
    # element ((b*H + h)*L + q)*L + key; cross: ((b*H + h)*Lq + q)*Lk + key
    assert k[1, 0, 3, 5] == bool(R.keep_mask(seed, ctr, np.array([((1 * 2 + 0) * 64 + 3) * 64 + 5]), p))
    x = R.cross_keep(seed, ctr, 2, 2, 5, 4, p)
    assert x[1, 1, 2, 3] == bool(R.keep_mask(seed, ctr, np.array([((1 * 2 + 1) * 5 + 2) * 4 + 3]), p))
    assert R.self_keep(seed, ctr, 1, 1, 4, 0.0).all()
    assert torch.equal(k, R.self_keep(0, None, 2, 2, 64, p, base=base))


# -------------------------------------------------------------------------- the case table
def test_case_table_reaches_the_edges():
    assert all(c.B * c.H <= 16 and c.L <= 256 for c in C.CASES if c.kind == "self")
    e = {c.id: C.case_edges(c) for c in C.CASES if c.kind == "self"}
    assert {c.L for c in C.CASES if c.kind == "self"} >= set(C.LS)
    for dt in ("f32", "bf16", "f16"):
        for L in C.LS:
            assert any(i.startswith(f"{dt}-L{L}-") for i in e), (dt, L)
        assert "dead-key-tile" in e[[i for i in e if i.startswith(f"{dt}-L15-")][0]]
        assert "lp-step" in e[[i for i in e if i.startswith(f"{dt}-L33-")][0]]
        assert "prob-transpose" in e[f"{dt}-uni-L37"]
        assert "all-key-tiles" in e[[i for i in e if i.startswith(f"{dt}-L255-")][0]]
        assert {"xcd-grouped", "ragged-chunk", "block128-edge"} <= e[f"{dt}-xcd-L129"]
        assert "linear-order" in e[f"{dt}-g-L256-padded"]
    assert {"idle-waves", "multi-block"} <= e["bf16-xcd-L129"]
    assert R.blocks_per_head(129, 8) == 2 and R.blocks_per_head(129, 16) == 1
    assert R.blocks_per_head(129, 4) == 3 and R.blocks_per_head(256, 16) == 1
    kinds = {c.mask for c in C.CASES if c.kind == "self"}
    assert kinds >= {"none", "prefix", "holes", "suffix", "single", "padded"}
    # every fully-padded-row case is a Gaussian case
    assert all("gauss" in c.families for c in C.CASES if c.kind == "self" and c.mask == "padded")
    assert {c.scale for c in C.CASES if c.kind == "self"} == {0.125, 1.0}
    assert {(c.Lq, c.Lk) for c in C.CASES if c.kind == "cross"} == \
        {(a, b) for a in (1, 5, 70) for b in (1, 4, 16)}
    assert all(c.ldq > 64 * c.H and c.lddq > 64 * c.H and c.B * c.Lq * c.H > 256 or c.Lq < 70
               for c in C.CASES if c.kind == "cross")
    assert {(c.pos, c.Lmax) for c in C.CASES if c.kind == "decode"} == \
        {(p, m) for p in (0, 1, 63, 64, 65, 511) for m in (p + 1, 512)}
    assert all(c.Lmax <= R.DEC_MAXL and c.R == 3 and c.H == 2 for c in C.CASES if c.kind == "decode")
    assert all(c.Lk <= R.XA_MAXK for c in C.CASES if c.kind == "cross")


@pytest.mark.parametrize("B,H,L,nw", [(2, 8, 129, 8), (2, 8, 129, 4), (3, 2, 129, 8), (1, 3, 256, 16),
                                      (2, 8, 129, 2)])
def test_block_order_is_a_permutation(B, H, L, nw):
    order = R.block_order(B, H, L, nw)
    nb = R.blocks_per_head(L, nw)
    assert sorted(order) == sorted((k, h, b) for k in range(nb) for h in range(H) for b in range(B))
    if R.xcd_grouped(B, H):     # the blocks of one head have ids congruent mod 8
        for h in range(H):
            for b in range(B):
                assert len({n % 8 for n, o in enumerate(order) if o[1:] == (h, b)}) == 1


def test_masks_are_what_their_names_say():
    for L in C.LS:
        for kind in C.MASKS[1:]:
            m = C.make_mask(kind, 4, L)
            assert (m.sum(-1) >= 1).all(), (kind, L)
        if L > 17:
            h = C.make_mask("holes", 4, L)
            assert h[0, 0] == 0 and h[0, 15] == 0 and h[0, 16] == 0 and h[0, L - 1] == 0
            assert (C.make_mask("single", 4, L).sum(-1) == 1).all()
            assert C.make_mask("suffix", 4, L)[:, 0].sum() == 0
    p = C.make_mask("padded", 3, 33)
    assert p[1].sum() == 0 and p[0].all() and 0 < p[2].sum() < 33


@pytest.mark.parametrize("cid", C.ids("self", "sel"))
def test_selector_preconditions(cid):
    c = C.BY_ID[cid]
    h = C.host_self(c, "sel")
    C.check_selector_preconditions(h, C.reference_self(h))
    assert torch.equal(h.qkv.to(c.dt).double(), h.qkv)
    if c.L > 1:
        assert h.targets.min() == 0 or c.mask in ("suffix", "single", "holes")
    if c.causal:
        assert (h.targets <= torch.arange(c.L)).all()
        assert (h.targets == torch.arange(c.L)).sum() > c.L // 3


@pytest.mark.parametrize("cid", C.ids("self", "uni"))
def test_uniform_preconditions(cid):
    h = C.host_self(C.BY_ID[cid], "uni")
    C.check_uniform_preconditions(h, C.reference_self(h))


def test_softmax_of_the_selector_is_one_hot_in_fp32():
    c = C.BY_ID["f32-L256-" + [x.mask for x in C.CASES if x.id.startswith("f32-L256-")][0]]
    h = C.host_self(c, "sel")
    r = C.reference_self(h)
    p = torch.softmax(r.S.float(), -1)
    assert torch.equal(p.double(), r.P.round())


# ------------------------------------------------------------------------- the emulations
def _rd(t, dt):
    return t if dt == F32 else t.to(dt).float()


def emulate(h, keep, mut=None):
    """fp32 torch emulation of the kernels on host data h.  Returns a dict of the P-saving
    flow's results and, for the cases that run it, the flash-style flow's under 'lse:'."""
    c, dt = h.c, h.c.dt
    B, L, H = c.B, c.L, c.H
    x = h.qkv.float()
    q, k, v, do = x[:, :, 0], x[:, :, 1], x[:, :, 2], h.dout.float()
    p, ks = h.p, np.float32(1.0) / (np.float32(1.0) - np.float32(h.p))
    ks = float(ks)
    mask = h.mask
    if mask is not None and mut == "hole-as-prefix":
        mask = (torch.arange(L)[None] < mask.sum(-1, keepdim=True)).long()
    madd = torch.zeros(B, 1, 1, L)
    if mask is not None:
        madd = torch.where(mask == 0, MASK32, torch.tensor(0.0))[:, None, None, :]
    ar = torch.arange(L)
    raw = torch.einsum("bqhd,bkhd->bhqk", q, k)
    S = raw * np.float32(c.scale) + madd
    if h.bias is not None:
        S = S + h.bias.float()[None]
    if c.causal:
        hid = ar[None, :] >= ar[:, None] if mut == "causal-ge" else ar[None, :] > ar[:, None]
        S = torch.where(hid[None, None], MASK32, S)
    dead = torch.zeros(L, dtype=torch.bool)
    if mut == "skip-last-tile":
        dead[(L - 1) // 16 * 16:] = True
    S = torch.where(dead, torch.tensor(-float("inf")), S)
    mx = S.max(-1, keepdim=True).values
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.exp(S - mx)
    z = e.sum(-1, keepdim=True)
    P = e * (1.0 / z)
    lse = (mx + torch.log(z))[..., 0]
    Pp = _rd(torch.where(keep, P * ks, torch.zeros_like(P)), dt)
    O = _rd(torch.einsum("bhqk,bkhd->bqhd", Pp, v), dt)
    out = {"out": O, "P": P, "lse": lse}
    dPr = torch.einsum("bqhd,bkhd->bhqk", do, v)
    dP = torch.where(keep, dPr if mut == "no-keep-scale" else dPr * ks, torch.zeros_like(P))
    dot = (P * dP).sum(-1, keepdim=True)
    dS = _rd(P * (dP - dot), dt)
    out["dS"] = dS
    out["dq"] = _rd(torch.einsum("bhqk,bkhd->bqhd", dS, k) * np.float32(c.scale), dt)
    out["dk"] = _rd(torch.einsum("bhqk,bqhd->bkhd", dS, q) * np.float32(c.scale), dt)
    out["dv"] = _rd(torch.einsum("bhqk,bqhd->bkhd", Pp, do), dt)
    if c.lse:
        D = (do * O).sum(-1).permute(0, 2, 1)
        S2 = raw * np.float32(c.scale) + madd
        S2 = torch.where(dead, torch.tensor(-float("inf")), S2)
        P2 = torch.exp(S2 - lse[..., None])
        padded = lse <= 0.5 * MASK32
        if mut != "padded-exp0":
            fixed = torch.exp(-torch.log(torch.tensor(float(L)))).expand_as(P2)
            P2 = torch.where(padded[..., None] & ~dead, fixed, P2)
        dS2 = _rd(P2 * (dP - D[..., None]), dt)
        Pp2 = _rd(torch.where(keep, P2 * ks, torch.zeros_like(P2)), dt)
        out["lse:D"] = D
        out["lse:dq"] = _rd(torch.einsum("bhqk,bkhd->bqhd", dS2, k) * np.float32(c.scale), dt)
        out["lse:dk"] = _rd(torch.einsum("bhqk,bqhd->bkhd", dS2, q) * np.float32(c.scale), dt)
        out["lse:dv"] = _rd(torch.einsum("bhqk,bqhd->bkhd", Pp2, do), dt)
    return out


@functools.lru_cache(maxsize=None)
def _gauss(cid):
    c = C.BY_ID[cid]
    h = C.host_self(c, "gauss")
    keep = R.self_keep(C.SEED, C.COUNTER0, c.B, c.H, c.L, h.p)
    r = C.reference_self(h, keep)
    b = R.bounds(r, c.dt)
    b2 = R.bounds(r, c.dt, lse_path=True, fixed_rows=r.row_blocked) if c.lse else None
    return h, keep, r, b, b2


def ratios(cid, mut=None):
    """{kind: error / bound} of the emulation of case cid against the reference."""
    h, keep, r, b, b2 = _gauss(cid)
    e = emulate(h, keep, mut)
    out = {}
    for name, ref, bd in (("out", r.O, b.out), ("P", r.P, b.P), ("lse", r.lse, b.lse),
                          ("dS", r.dS, b.dS), ("dq", r.dq, b.dq), ("dk", r.dk, b.dk),
                          ("dv", r.dv, b.dv)):
        out[name] = R.ratio_only(e[name], ref, bd)
    if b2 is not None:
        for name, ref, bd in (("lse:D", r.D, b2.D), ("lse:dq", r.dq, b2.dq),
                              ("lse:dk", r.dk, b2.dk), ("lse:dv", r.dv, b2.dv)):
            out[name] = R.ratio_only(e[name], ref, bd)
    return out


@pytest.mark.parametrize("cid", GAUSS_SELF)
def test_bounds_are_well_posed(cid):
    """The fp32 emulation passes every Gaussian bound with a ratio below 1."""
    rt = ratios(cid)
    print("attnref-cpu", cid, {k: round(v, 3) for k, v in rt.items()})
    assert max(rt.values()) < 1.0, rt


def _prefix_form(m):
    return (torch.arange(m.shape[1])[None] < m.sum(-1, keepdim=True)).long()


def _expected_to_fail(c, mut):
    h, keep, r, _, _ = _gauss(c.id)
    if mut == "causal-ge":
        return c.causal
    if mut == "hole-as-prefix":
        return h.mask is not None and not torch.equal(h.mask, _prefix_form(h.mask))
    if mut == "no-keep-scale":      # one allowed key: dS = 0 whatever dP is
        return h.p > 0 and c.mask != "single"
    if mut == "skip-last-tile":     # some row puts weight on a key of the last tile
        return bool((r.P[..., (c.L - 1) // 16 * 16:] > 1e-30).any())
    if mut == "padded-exp0":
        return c.lse and bool(r.row_blocked.any())
    raise ValueError(mut)


@pytest.mark.parametrize("mut", ["causal-ge", "hole-as-prefix", "no-keep-scale", "skip-last-tile",
                                 "padded-exp0"])
def test_the_checks_bite(mut):
    """Each emulation that changes arithmetic only fails exactly the cases that run the changed
    code: causal as key >= q; a hole mask read as a prefix mask; keep_scale dropped from dP;
    the last key tile skipped; p = exp(0) for a fully padded row in the flash-style backward."""
    wrong = []
    for cid in GAUSS_SELF:
        c = C.BY_ID[cid]
        rt = ratios(cid, mut)
        fails = max(rt.values()) > 1.0
        if mut == "padded-exp0" and fails:
            assert all(v <= 1.0 for k, v in rt.items() if not k.startswith("lse:")), (cid, rt)
        if fails != _expected_to_fail(c, mut):
            wrong.append((cid, fails, {k: round(v, 3) for k, v in rt.items()}))
    assert not wrong, wrong
    assert any(_expected_to_fail(C.BY_ID[i], mut) for i in GAUSS_SELF)
    assert not all(_expected_to_fail(C.BY_ID[i], mut) for i in GAUSS_SELF)
