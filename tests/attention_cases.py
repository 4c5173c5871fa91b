"""Case table and operand families of tests/test_attention_reference_gpu.py (and of the CPU
checks of tests/test_attention_ref_cpu.py): the smallest shapes at which each path of the
attention kernels can go wrong, B * H <= 16 and L <= 256 throughout.

Self-attention cases run both flows where the entry points accept them: the P-saving one
(mmdx_attention_fwd / _fwd_ex with and without probs, mmdx_attention_bwd with its dS workspace)
and, for 16-bit cases without bias / causal, the flash-style one (mmdx_attention_fwd_lse,
mmdx_attention_bwd_lse with its D workspace and rng[0]).

Operand families (host(c, family)):
  * "sel"  selector, exact: key j carries the +-c code of j's bits in head dims 0..7, query q
    the code of target(q) (c = 32 at scale 0.125, c = 16 at scale 1), so the target's score
    beats every other allowed key's by >= 256, every other __expf argument is <= -256 (0 in
    fp32) and P is exactly one-hot.  The other Q dims hold small integers (K is zero there), V
    small integers with the key's bits in dims 0..7 (distinct rows), dO in {-1, 0, 1}, the bias
    integers in [-3, 0] (in [0, 3] at the target).  Dropout p = 0.5: 1 / (1 - p) = 2.
    out, saved P with its sign, lse, dV, dQ = dK = 0, the dS workspace = 0 and D must EQUAL
    the reference (rounded to the integers it differs from by < 1e-90: fp64 keeps exp(-256)).
  * "uni"  uniform, exact forward: Q = 0, K, V, dO in {-1, 0, 1}, a power-of-two number n of
    allowed keys per row: P = 1 / n, out and dV are exact; lse, dQ, dK, dS are bounded.
  * "gauss"  bounded: unit Gaussians on the compute dtype's grid (Q times 12 in the "hot"
    cases: |s - max| reaches about 60); every check is attention_ref.bounds()."""
from types import SimpleNamespace

import torch

import attention_ref as R
from attention_ref import BF16, F16, F32

DTS = (F32, BF16, F16)
LS = (1, 15, 16, 17, 31, 32, 33, 37, 63, 64, 65, 127, 128, 129, 197, 255, 256)
MASKS = ("none", "prefix", "holes", "suffix", "single")
KNOB_NAMES = ("MMDX_ATTN_FWD_NW", "MMDX_ATTN_BWD_NW")
SEED, COUNTER0 = 0x5EED1234, 7


def make_mask(kind, B, L):
    """[B, L] int64 (0 = pad) or None."""
    if kind == "none":
        return None
    m = torch.ones(B, L, dtype=torch.int64)
    for b in range(B):
        if kind == "prefix":
            m[b, max(1, (L * (b + 1)) // (B + 1)):] = 0
        elif kind == "holes":
            for k in ((0, 15, 16, L - 1), (0,), (15, 16), (L - 1, 16))[b % 4]:
                if 0 <= k < L and m[b].sum() > 1:
                    m[b, k] = 0
        elif kind == "suffix":
            m[b, :min(L - 1, L // 2 + b)] = 0
        elif kind == "single":
            m[b] = 0
            m[b, (L - 1, 0, 16 % L, 15 % L)[b % 4]] = 1
        elif kind == "padded":          # one fully padded batch row beside normal ones
            if b == 1:
                m[b] = 0
            elif b == 2:
                m[b, max(1, L // 3):] = 0
        elif kind == "uni-holes":       # 5 holes: 32 of 37 keys
            for k in (0, 15, 16, 31, L - 1):
                m[b, k] = 0
        elif kind == "uni-padded":
            if b == 1:
                m[b] = 0
        else:
            raise ValueError(kind)
    return m


def _self(cid, dt, B, L, H, mask="none", p=0.0, scale=0.125, bias=False, causal=False,
          knobs=None, fam=("sel",), hot=False):
    return SimpleNamespace(id=cid, kind="self", dt=dt, B=B, L=L, H=H, mask=mask, p=p, scale=scale,
                           bias=bias, causal=causal, knobs=dict(knobs or {}), families=tuple(fam),
                           hot=hot, lse=dt != F32 and not bias and not causal)


def _build_self():
    cs = []
    n = R.DT_NAME
    # every L with every dtype, the mask kind and dropout rotating
    for i, L in enumerate(LS):
        for j, dt in enumerate(DTS):
            mk = MASKS[(i + j) % len(MASKS)]
            if L == 1 and mk in ("holes", "suffix"):
                mk = "none"
            cs.append(_self(f"{n[dt]}-L{L}-{mk}", dt, 2, L, 2, mk, 0.5 if (i + j) % 2 else 0.0))
    # one Gaussian case per kernel path and mask kind; a fully padded batch row in every dtype
    for j, dt in enumerate(DTS):
        for i, mk in enumerate(MASKS + ("padded",)):
            L = (37, 65, 129, 33, 197, 17)[(i + j) % 6]
            fam = ("gauss",) if mk == "padded" else ("sel", "gauss")
            cs.append(_self(f"{n[dt]}-g-L{L}-{mk}", dt, 3, L, 2, mk, 0.5 if i % 2 else 0.0,
                            fam=fam))
        cs.append(_self(f"{n[dt]}-g-L256-padded", dt, 3, 256, 1, "padded", 0.0, fam=("gauss",)))
        cs.append(_self(f"{n[dt]}-g-L129-hot", dt, 2, 129, 2, "prefix", 0.0, fam=("gauss",),
                        hot=True))
        # B * H = 16 at L = 129: the XCD-grouped order, two blocks per head, two groups
        cs.append(_self(f"{n[dt]}-xcd-L129", dt, 2, 129, 8, "prefix", 0.5, fam=("sel", "gauss")))
        # T5: unscaled, bias and causal through mmdx_attention_fwd_ex
        for L in (33, 129):
            cs.append(_self(f"{n[dt]}-t5-L{L}-bias", dt, 2, L, 2, "none", 0.0, 1.0, bias=True,
                            fam=("sel", "gauss")))
            cs.append(_self(f"{n[dt]}-t5-L{L}-causal", dt, 2, L, 2, "prefix", 0.5, 1.0,
                            causal=True, fam=("sel", "gauss")))
            cs.append(_self(f"{n[dt]}-t5-L{L}-bias-causal", dt, 3, L, 2, "none", 0.5, 1.0,
                            bias=True, causal=True, fam=("sel", "gauss")))
        # causal with a hole at key 0: query 0 has no allowed key (uniform over all L)
        cs.append(_self(f"{n[dt]}-t5-L17-causal-hole0", dt, 2, 17, 2, "holes", 0.0, 1.0,
                        causal=True, fam=("gauss",)))
        cs.append(_self(f"{n[dt]}-s1-L65", dt, 2, 65, 2, "holes", 0.5, 1.0, fam=("sel", "gauss")))
        # uniform
        cs.append(_self(f"{n[dt]}-uni-L37", dt, 2, 37, 2, "uni-holes", fam=("uni",)))
        for L in (32, 64):
            cs.append(_self(f"{n[dt]}-uni-L{L}-padded", dt, 3, L, 2, "uni-padded", fam=("uni",)))
    # knob runs where block edges differ between the sizes
    for dt in (BF16, F16):
        for kn, v in (("MMDX_ATTN_FWD_NW", 4), ("MMDX_ATTN_FWD_NW", 16), ("MMDX_ATTN_BWD_NW", 4)):
            tag = f"{'f' if 'FWD' in kn else 'b'}{v}"
            cs.append(_self(f"{n[dt]}-xcd-L129-{tag}", dt, 2, 129, 8, "prefix", 0.5,
                            knobs={kn: v}, fam=("sel", "gauss")))
            cs.append(_self(f"{n[dt]}-L37-{tag}", dt, 3, 37, 2, "holes", 0.5, knobs={kn: v},
                            fam=("sel", "gauss")))
            for L in (65, 256):
                cs.append(_self(f"{n[dt]}-L{L}-{tag}", dt, 1, L, 3, "suffix", 0.0, knobs={kn: v}))
            cs.append(_self(f"{n[dt]}-L64-padded-{tag}", dt, 3, 64, 2, "padded", 0.0,
                            knobs={kn: v}, fam=("gauss",)))
    return cs


def _build_cross():
    cs = []
    i = 0
    for Lk in (1, 4, 16):
        for Lq in (1, 5, 70):       # B * Lq * H = 280: past one 256-thread block
            for dt in DTS:
                i += 1
                cs.append(SimpleNamespace(
                    id=f"x-{R.DT_NAME[dt]}-q{Lq}-k{Lk}", kind="cross", dt=dt, B=2, Lq=Lq, Lk=Lk,
                    H=2, scale=(0.125, 1.0)[i % 2], p=0.5 if i % 3 else 0.0, ldq=128 + 16,
                    lddq=128 + 8, knobs={}, families=("gauss",)))
    return cs


def _build_decode():
    cs = []
    for pos in (0, 1, 63, 64, 65, 511):
        for Lmax in sorted({pos + 1, 512}):
            for dt in DTS:
                cs.append(SimpleNamespace(
                    id=f"d-{R.DT_NAME[dt]}-p{pos}-m{Lmax}", kind="decode", dt=dt, R=3, H=2, pos=pos,
                    Lmax=Lmax, knobs={}, families=("gauss",)))
    return cs


def _build_posbias():
    cs = []
    for nb, maxd, L in ((32, 128, 130), (8, 16, 20)):
        for beta in (0.0, 1.0):
            for dt in DTS:
                cs.append(SimpleNamespace(
                    id=f"pb-{R.DT_NAME[dt]}-nb{nb}-L{L}-beta{int(beta)}", kind="posbias", dt=dt, B=2,
                    H=2, L=L, nb=nb, maxd=maxd, beta=beta, knobs={}, families=("int", "gauss")))
    return cs


CASES = _build_self() + _build_cross() + _build_decode() + _build_posbias()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "duplicate case ids"


def ids(kind, family):
    return [c.id for c in CASES if c.kind == kind and family in c.families]


def case_edges(c):
    return R.edges(c.dt, c.B, c.L, c.H, c.mask, c.knobs)


# ---------------------------------------------------------------------------------- operands
def _gen(c, family):
    return torch.Generator().manual_seed(sum(map(ord, c.id)) * 7 + len(family))


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _code(idx, c):
    """[..., 8]: +c where bit d of idx is set, -c elsewhere."""
    bits = (idx[..., None] >> torch.arange(8)) & 1
    return (2 * bits - 1).double() * c


TARGET_KEYS = (0, 255, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 196, 197)


def selector_targets(c, mask):
    """[B, H, L] long: an allowed key per query.  They cycle through key 0, the last key and
    both sides of every tile boundary; under causal every other query takes the diagonal."""
    B, L, H = c.B, c.L, c.H
    cand = sorted({min(k, L - 1) for k in TARGET_KEYS})
    blk = R.blocked_mask(B, L, mask, c.causal).expand(B, 1, L, L)
    t = torch.zeros(B, H, L, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            for q in range(L):
                k = cand[(q + h + (0 if c.bias else 2 * b)) % len(cand)]
                if c.causal:
                    k = q if (q + h) % 2 else min(k, q)
                if blk[b, 0, q, k]:
                    ok = (~blk[b, 0, q]).nonzero().flatten().tolist()
                    assert ok, f"{c.id}: query {q} of batch {b} has no allowed key"
                    k = ok[(q * 7 + h) % len(ok)]
                t[b, h, q] = k
    return t


def host_self(c, family):
    """qkv [B, L, 3, H, 64], dout [B, L, H, 64], mask, bias [H, L, L] (fp64 values the compute
    dtype holds; the bias fp32's), plus targets for the selector family."""
    g = _gen(c, family)
    B, L, H = c.B, c.L, c.H
    h = SimpleNamespace(c=c, family=family, mask=make_mask(c.mask, B, L), bias=None, targets=None)
    h.p = c.p if family != "uni" else 0.0
    if family == "sel":
        cc = 32.0 if c.scale == 0.125 else 16.0
        assert c.scale in (0.125, 1.0)
        h.targets = selector_targets(c, h.mask)
        ar = torch.arange(L)
        q = _ints((B, L, H, 64), -3, 3, g)
        q[..., :8] = _code(h.targets.permute(0, 2, 1), cc)
        k = torch.zeros(B, L, H, 64, dtype=torch.float64)
        k[..., :8] = _code(ar, cc)[None, :, None, :]
        v = _ints((B, L, H, 64), -1, 1, g)
        v[..., :8] = ((ar[:, None] >> torch.arange(8)) & 1).double()[None, :, None, :] * \
            _ints((1, 1, H, 8), 1, 3, g)
        h.dout = _ints((B, L, H, 64), -1, 1, g)
        if c.bias:
            h.bias = _ints((H, L, L), -3, 0, g)
            at = _ints((B, H, L), 0, 3, g)
            for b in range(B):     # the same target per (h, q) in every batch row when biased
                assert torch.equal(h.targets[b], h.targets[0]), "biased selector: targets"
            h.bias.scatter_(2, h.targets[0][..., None], at[0][..., None])
    elif family == "uni":
        q = torch.zeros(B, L, H, 64, dtype=torch.float64)
        k, v = _ints((B, L, H, 64), -1, 1, g), _ints((B, L, H, 64), -1, 1, g)
        h.dout = _ints((B, L, H, 64), -1, 1, g)
    else:
        rn = lambda *s: torch.randn(*s, generator=g).to(c.dt).double()   # noqa: E731
        q, k, v = rn(B, L, H, 64), rn(B, L, H, 64), rn(B, L, H, 64)
        if c.hot:
            q = (q * 12).to(c.dt).double()
        h.dout = rn(B, L, H, 64)
        if c.bias:
            h.bias = torch.randn(H, L, L, generator=g).float().double()
    h.qkv = torch.stack([q, k, v], 2)
    return h


def reference_self(h, keep=None):
    c = h.c
    if keep is None:
        keep = R.self_keep(SEED, COUNTER0, c.B, c.H, c.L, h.p)
    return R.self_attention(h.qkv, h.dout, c.scale, h.mask, h.bias, c.causal, keep, h.p)


def check_selector_preconditions(h, r):
    """From the reference alone: the target's score beats every other key's by >= 256 (so the
    fp32 softmax is exactly one-hot), every compared value is within 1e-90 of an integer the
    stored dtype holds, and the sums stay far below 2^24."""
    c = h.c
    S = r.S
    top = S.gather(-1, h.targets[..., None])
    assert (~r.blocked.gather(-1, h.targets[..., None])).all(), f"{c.id}: a target is masked"
    rest = S.clone()
    rest.scatter_(-1, h.targets[..., None], -float("inf"))
    gap = (top - rest.max(-1, keepdim=True).values).min().item()
    assert gap >= 256, f"{c.id}: score gap {gap} < 256"
    assert torch.equal(top, top.round()) and top.abs().max() < 2 ** 20
    lim = {BF16: 256.0, F16: 2048.0, F32: 2.0 ** 24}[c.dt]
    for name, step in (("O", 1.0), ("dv", 1.0), ("P", 1.0), ("D", 1.0)):
        t = getattr(r, name)
        assert (t - t.round()).abs().max() < 1e-90, f"{c.id}: {name} is not integer-valued"
    # even integers up to twice the limit are held too (dropout doubles every term)
    for name in ("O", "dv"):
        t = getattr(r, name).round()
        assert torch.equal(t.to(c.dt).double(), t), f"{c.id}: {name} not storable in {c.dt}"
        assert t.abs().max() <= 2 * lim
    for name in ("dq", "dk", "dS"):
        assert getattr(r, name).abs().max() < 1e-90, f"{c.id}: {name} is not zero"
    assert r.dv_terms.max() < 2 ** 20 and r.o_terms.max() < 2 ** 20


def check_uniform_preconditions(h, r):
    c = h.c
    n = (~r.blocked).sum(-1)
    n = torch.where(n == 0, torch.full_like(n, c.L), n)
    assert ((n & (n - 1)) == 0).all(), f"{c.id}: allowed keys per row not a power of two"
    assert torch.equal(r.P * n[..., None], (r.P > 0).double()), f"{c.id}: P is not 1 / n"
    for name in ("O", "dv"):
        t = getattr(r, name)
        assert torch.equal(t.to(c.dt).double(), t), f"{c.id}: {name} not storable in {c.dt}"
    assert (r.dk == 0).all()


def host_cross(c, family="gauss"):
    g = _gen(c, family)
    rn = lambda *s: torch.randn(*s, generator=g).to(c.dt).double()   # noqa: E731
    h = SimpleNamespace(c=c, q=rn(c.B, c.Lq, c.H, 64), kv=rn(c.B, c.Lk, 2, c.H, 64),
                        dout=rn(c.B, c.Lq, c.H, 64), p=c.p)
    return h


def reference_cross(h):
    c = h.c
    keep = R.cross_keep(SEED, COUNTER0, c.B, c.H, c.Lq, c.Lk, c.p)
    return R.cross_attention(h.q, h.kv, h.dout, c.scale, keep, c.p)


def host_decode(c, family="gauss"):
    g = _gen(c, family)
    rn = lambda *s: torch.randn(*s, generator=g).to(c.dt).double()   # noqa: E731
    h = SimpleNamespace(c=c, qkv=rn(c.R, 3, c.H, 64), kc=rn(c.R, c.Lmax, c.H, 64),
                        vc=rn(c.R, c.Lmax, c.H, 64))
    h.kc[:, c.pos:] = R.NAN         # nothing at or behind pos is read
    h.vc[:, c.pos:] = R.NAN
    # permuted: key j of row r lives in another row's cache
    r, j = torch.arange(c.R)[:, None], torch.arange(c.Lmax)[None, :]
    h.slots = ((r + j + 1) % c.R).to(torch.int32)
    h.bias = torch.randn(c.H, c.Lmax, c.Lmax, generator=g).float().double()
    return h


def host_posbias(c, family):
    g = _gen(c, family)
    LP = R.attn_lp(c.L)
    assert LP > c.L
    h = SimpleNamespace(c=c, LP=LP)
    h.table = torch.randn(c.nb, c.H, generator=g).float().double()
    if family == "int":
        ds = _ints((c.B, c.H, c.L, c.L), -1, 1, g)
        h.dtable0 = _ints((c.nb, c.H), -3, 3, g)
    else:
        ds = torch.randn(c.B, c.H, c.L, c.L, generator=g).to(c.dt).double()
        h.dtable0 = torch.randn(c.nb, c.H, generator=g).float().double()
    h.ds = torch.full((c.B, c.H, c.L, LP), R.NAN, dtype=torch.float64)
    h.ds[..., :c.L] = ds
    ar = torch.arange(c.L)
    h.ds[..., :c.L][..., ar[None, :] > ar[:, None]] = R.NAN     # cells k > q are never read
    return h
