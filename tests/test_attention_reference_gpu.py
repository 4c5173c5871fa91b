"""The attention entry points against the fp64 reference of tests/attention_ref.py, element by
element, through raw-pointer calls, at the cases of tests/attention_cases.py (the smallest
shapes that reach each tile, block, chunk and mask edge; tests/test_attention_ref_cpu.py
asserts which case reaches which edge and that the bounds are well posed and bite).

Entry points covered: mmdx_attention_fwd (with probs and with probs = NULL, bit-identical
outputs), mmdx_attention_fwd_ex (bias, causal, both), mmdx_attention_bwd with its dS workspace
(columns [L, LP) of live rows included: zero), mmdx_attention_fwd_lse and mmdx_attention_bwd_lse
with the D workspace and rng[0], both workspace-size functions (equal to their mirrors),
mmdx_xattn_fwd / _bwd, mmdx_t5_decode_attn, mmdx_t5_position_bias and _bias_bwd; fp32, bf16 and
fp16 wherever the entry point accepts them; MMDX_ATTN_FWD_NW in {4, 16} and MMDX_ATTN_BWD_NW = 4.

Guards: every output sits between sentinel guard elements and is preset to NaN where it must be
fully written (to the sentinel where it must not be: dq's ldq padding columns); workspaces are
exactly the queried size with a sentinel behind; qkv, dout, q, kv, the bias and the caches live
inside NaN-filled buffers, ldq padding and the dS padding columns / upper triangle fed to the
bias backward are NaN, the decode bias is NaN outside row pos; every input is bit-identical
afterwards.  Dropout: the keep bits read from the saved probabilities' signs equal
attention_ref.keep_mask at the documented element index (self- and cross-attention), the launch
counter advances by exactly one, rng[0] is the stream base, and the flash-style backward is held
to the reference computed with keep_mask's bits.

Measured on an MI355X.  test_expf_logf_allowance: __expf 1.187 x 2^-24 (1 + |argument|) in
fp32, bf16 and fp16 alike (arguments down to -33), __logf 0.375 x 2^-24 (1 + sum) (sums 1 to
9); attention_ref.EXPF_C and LOGF_C are twice these.  Equalities: every selector case (out, the
saved P and its sign, lse, dV, dQ = dK = 0, the dS workspace = 0, D, in both flows), out / P / dV
of every uniform case, the position bias and the integer-family dtable, the decode caches, and
every bit-identity above.  Largest error / bound per kind over the Gaussian and uniform cases
(with EXPF_C = 3, LOGF_C = 1, the values before the measurement): out 0.76, P 0.52, lse 0.007,
dS 0.997 (the half-ulp of the 16-bit store), dQ 0.65, dK 0.82, dV 0.77, D 0.15, flash-style dQ
0.48, dK 0.31, dV 0.71, cross-attention out 0.93, P 0.007, dQ 0.84, dK 0.96, dV 0.94, decode
0.68, dtable 0.003.
The fully padded batch row (a finding of these tests): before the fix
attn_bwd_q16_lse_kernel / attn_bwd_kv16_lse_kernel recomputed P = exp(MASK_NEG - lse) = 1 for
such a row, whose saved lse = MASK_NEG + log L is MASK_NEG in fp32: the flash-style dV of
bf16-uni-L32-padded was exactly L = 32 times the reference (4.0 for 0.125), and lse-dV error /
bound was 4.5e3 to 8.4e4 in all ten padded Gaussian cases (both 16-bit dtypes, L 37 to 256, all
three knob settings) while the P-saving flow passed them.  After the fix (the block of such a
head takes scale = 0, lse = 0 and -log L as its key mask) every case passes and the forward's
bits are unchanged.
"""
import pytest
import torch

import attention_cases as C
import attention_ref as R
import mmdx._lib as L
from attention_ref import F32, NAN, U24

pytestmark = pytest.mark.gpu

SENT = -7.0
GUARD = 64
RAN = set()


# ----------------------------------------------------------------------------------- buffers
def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


class _Buf:
    """A flat device buffer: GUARD elements, the body, GUARD elements.  Inputs: NaN guards
    around the data, bit-identical afterwards.  Outputs: sentinel guards around a preset body."""

    def __init__(self, dev, shape, dt, data=None, fill=NAN, guard=SENT):
        self.shape = tuple(shape)
        n = 1
        for s in self.shape:
            n *= s
        self.n = n
        host = torch.full((GUARD + n + GUARD,), guard, dtype=dt)
        host[GUARD:GUARD + n] = fill
        if data is not None:
            host[GUARD:GUARD + n] = data.reshape(-1).to(dt)
        self.before = host
        self.dev = host.to(dev)
        self.ptr = self.dev.data_ptr() + GUARD * host.element_size()

    def body(self):
        return self.dev[GUARD:GUARD + self.n].view(self.shape)

    def f64(self):
        return self.body().cpu().double()

    def check_guards(self, what):
        g = self.dev.cpu()
        ok = _same_bits(g[:GUARD], self.before[:GUARD]) and \
            _same_bits(g[GUARD + self.n:], self.before[GUARD + self.n:])
        assert ok, f"{what}: written outside the buffer"

    def check_unchanged(self, what):
        assert _same_bits(self.dev, self.before), f"{what}: changed"


def _in(dev, data, dt):
    return _Buf(dev, data.shape, dt, data=data, guard=NAN)


def _i64(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def _set_knobs(knobs, c):
    for name in C.KNOB_NAMES:
        knobs(name, c.knobs.get(name))


# --------------------------------------------------------------------------- self-attention
def _run_self(dev, c, h):
    """Both flows of case c on host data h.  Checks guards, inputs, counter, rng, the
    workspace sizes and the keep bits; returns the results as fp64 CPU tensors."""
    lib = L.lib()
    dc = L.dtype_code(c.dt)
    B, Ls, H, p = c.B, c.L, c.H, h.p
    LP = R.attn_lp(Ls)
    st = L.stream()
    qkv, do = _in(dev, h.qkv, c.dt), _in(dev, h.dout, c.dt)
    mask = h.mask.to(dev) if h.mask is not None else None
    mp = mask.data_ptr() if mask is not None else None
    bias = _in(dev, h.bias, F32) if h.bias is not None else None
    ctr = torch.tensor([C.COUNTER0], dtype=torch.int64, device=dev)
    keep = R.self_keep(C.SEED, C.COUNTER0, B, H, Ls, p)
    g = {"keep": keep}

    def fwd(out, probs):
        pp = probs.ptr if probs is not None else None
        if c.bias or c.causal:
            L.call("mmdx_attention_fwd_ex", dc, qkv.ptr, mp, bias.ptr if bias else None,
                   int(c.causal), B, Ls, H, c.scale, p, C.SEED, ctr.data_ptr(), out.ptr, pp, st)
        else:
            L.call("mmdx_attention_fwd", dc, qkv.ptr, mp, B, Ls, H, c.scale, p, C.SEED,
                   ctr.data_ptr(), out.ptr, pp, st)
        torch.cuda.synchronize()
        out.check_guards(f"{c.id}: out")

    out = _Buf(dev, (B, Ls, H, 64), c.dt)
    probs = _Buf(dev, (B, H, Ls, Ls), F32)
    fwd(out, probs)
    probs.check_guards(f"{c.id}: probs")
    assert int(ctr.item()) == C.COUNTER0 + (1 if p > 0 else 0), f"{c.id}: launch counter"
    pr = probs.body().cpu()
    assert torch.equal(~torch.signbit(pr), keep), f"{c.id}: keep bits differ from keep_mask"
    g["out"], g["P"] = out.f64(), pr.double().abs()
    if p == 0:      # probs = NULL: the same output, bit for bit
        out2 = _Buf(dev, (B, Ls, H, 64), c.dt)
        fwd(out2, None)
        assert _same_bits(out2.dev, out.dev), f"{c.id}: out differs without probs"
    n = lib.mmdx_attention_workspace_size(dc, B, Ls, H)
    assert n == R.workspace_size(c.dt, B, Ls, H)
    ws = _Buf(dev, (B, H, Ls, LP), c.dt)
    assert ws.n * ws.dev.element_size() == n
    dqkv = _Buf(dev, (B, Ls, 3, H, 64), c.dt)
    pb = probs.dev.cpu().clone()
    L.call("mmdx_attention_bwd", dc, qkv.ptr, probs.ptr, do.ptr, mp, B, Ls, H, c.scale, p,
           dqkv.ptr, ws.ptr, n, st)
    torch.cuda.synchronize()
    ws.check_guards(f"{c.id}: dS workspace")
    dqkv.check_guards(f"{c.id}: dqkv")
    assert _same_bits(probs.dev, pb), f"{c.id}: probs changed in the backward"
    g["dqkv"], g["ws"] = dqkv.f64(), ws.f64()
    if c.lse:
        ctr.fill_(C.COUNTER0)
        out_l = _Buf(dev, (B, Ls, H, 64), c.dt)
        lse = _Buf(dev, (B, H, Ls), F32)
        rng = _Buf(dev, (1,), torch.int64, fill=0, guard=-7)
        L.call("mmdx_attention_fwd_lse", dc, qkv.ptr, mp, B, Ls, H, c.scale, p, C.SEED,
               ctr.data_ptr(), out_l.ptr, lse.ptr, rng.ptr, st)
        torch.cuda.synchronize()
        for t, name in ((out_l, "out"), (lse, "lse"), (rng, "rng")):
            t.check_guards(f"{c.id}: {name} (lse)")
        assert int(ctr.item()) == C.COUNTER0 + (1 if p > 0 else 0), f"{c.id}: counter (lse)"
        assert int(rng.body().item()) == _i64(R.dropout_stream_base(C.SEED, C.COUNTER0)), \
            f"{c.id}: rng[0] is not the stream base"
        assert _same_bits(out_l.dev, out.dev), f"{c.id}: the flash-style forward's output differs"
        n2 = lib.mmdx_attention_lse_workspace_size(dc, B, Ls, H)
        assert n2 == R.lse_workspace_size(c.dt, B, Ls, H)
        wd = _Buf(dev, (B, H, Ls), F32)
        dq_l = _Buf(dev, (B, Ls, 3, H, 64), c.dt)
        befo = [t.dev.cpu().clone() for t in (out_l, lse, rng)]
        L.call("mmdx_attention_bwd_lse", dc, qkv.ptr, out_l.ptr, lse.ptr, rng.ptr, do.ptr, mp, B,
               Ls, H, c.scale, p, dq_l.ptr, wd.ptr, n2, st)
        torch.cuda.synchronize()
        wd.check_guards(f"{c.id}: D workspace")
        dq_l.check_guards(f"{c.id}: dqkv (lse)")
        for t, b0, name in zip((out_l, lse, rng), befo, ("out", "lse", "rng")):
            assert _same_bits(t.dev, b0), f"{c.id}: {name} changed in the flash-style backward"
        g["lse"], g["D"], g["dqkv_l"] = lse.f64(), wd.f64(), dq_l.f64()
    qkv.check_unchanged(f"{c.id}: qkv")
    do.check_unchanged(f"{c.id}: dout")
    if bias:
        bias.check_unchanged(f"{c.id}: bias")
    if mask is not None:
        assert torch.equal(mask.cpu(), h.mask), f"{c.id}: mask changed"
    return g


@pytest.mark.parametrize("cid", C.ids("self", "sel"))
def test_self_attention_selector(dev, knobs, cid):
    """Selector operands: out, the saved P with its sign, lse, dV, dQ = dK = 0, the dS
    workspace = 0 and D equal the reference."""
    c = C.BY_ID[cid]
    h = C.host_self(c, "sel")
    r = C.reference_self(h)
    C.check_selector_preconditions(h, r)
    _set_knobs(knobs, c)
    g = _run_self(dev, c, h)
    R.assert_exact(g["out"], r.O.round(), f"{cid}: out")
    R.assert_exact(g["P"], r.P.round(), f"{cid}: P")
    R.assert_exact(g["dqkv"], r.dqkv.round(), f"{cid}: dqkv")
    R.assert_exact(g["ws"], torch.zeros_like(g["ws"]), f"{cid}: dS workspace")
    if c.lse:
        R.assert_exact(g["lse"], r.lse, f"{cid}: lse")
        R.assert_exact(g["D"], r.D.round(), f"{cid}: D")
        R.assert_exact(g["dqkv_l"], r.dqkv.round(), f"{cid}: dqkv (lse)")
    RAN.add((cid, "sel"))


def _bounded_self(cid, c, r, g, exact_fwd):
    b = R.bounds(r, c.dt)
    if exact_fwd:
        R.assert_exact(g["out"], r.O, f"{cid}: out")
        R.assert_exact(g["P"], r.P, f"{cid}: P")
        R.assert_exact(g["dqkv"][:, :, 2], r.dv, f"{cid}: dV")
    else:
        R.check_bounded("out", g["out"], r.O, b.out, cid)
        R.check_bounded("P", g["P"], r.P, b.P, cid)
        R.check_bounded("dV", g["dqkv"][:, :, 2], r.dv, b.dv, cid)
    R.check_bounded("dS", g["ws"], R.pad_ws(r.dS, r.LP), R.pad_ws(b.dS, r.LP), cid)
    R.check_bounded("dQ", g["dqkv"][:, :, 0], r.dq, b.dq, cid)
    R.check_bounded("dK", g["dqkv"][:, :, 1], r.dk, b.dk, cid)
    if c.lse:
        b2 = R.bounds(r, c.dt, lse_path=True, fixed_rows=r.row_blocked)
        R.check_bounded("lse", g["lse"], r.lse, b.lse, cid)
        R.check_bounded("D", g["D"], r.D, b2.D, cid)
        if exact_fwd:
            R.assert_exact(g["dqkv_l"][:, :, 2], r.dv, f"{cid}: dV (lse)")
        else:
            R.check_bounded("lse-dV", g["dqkv_l"][:, :, 2], r.dv, b2.dv, cid)
        R.check_bounded("lse-dQ", g["dqkv_l"][:, :, 0], r.dq, b2.dq, cid)
        R.check_bounded("lse-dK", g["dqkv_l"][:, :, 1], r.dk, b2.dk, cid)


@pytest.mark.parametrize("cid", C.ids("self", "uni"))
def test_self_attention_uniform(dev, knobs, cid):
    """Q = 0 and a power-of-two number of allowed keys: P = 1 / n, out and dV are exact; lse,
    dS, dQ and dK are bounded (a fully padded batch row is such a row: n = L)."""
    c = C.BY_ID[cid]
    h = C.host_self(c, "uni")
    r = C.reference_self(h)
    C.check_uniform_preconditions(h, r)
    _set_knobs(knobs, c)
    _bounded_self(cid, c, r, _run_self(dev, c, h), True)
    RAN.add((cid, "uni"))


@pytest.mark.parametrize("cid", C.ids("self", "gauss"))
def test_self_attention_gaussian(dev, knobs, cid):
    """Gaussian operands: every output within attention_ref.bounds() of the reference."""
    c = C.BY_ID[cid]
    h = C.host_self(c, "gauss")
    r = C.reference_self(h)
    _set_knobs(knobs, c)
    _bounded_self(cid, c, r, _run_self(dev, c, h), False)
    RAN.add((cid, "gauss"))


@pytest.mark.parametrize("dt", C.DTS, ids=lambda d: R.DT_NAME[d])
def test_expf_logf_allowance(dev, knobs, dt):
    """The device's __expf and __logf against fp64: integer Q and K in [-3, 3] at scale 0.125
    make every score an exact multiple of 1 / 8, so s - max is exact, the row maximum's
    probability is __expf(0) / sum = 1 / sum, and a saved probability over the row maximum's is
    __expf(s - max) with one product rounding: its error in units of 2^-24 (1 + |s - max|) is
    __expf's.  lse - max is __logf(sum) with the sum's own error and one addition: its error
    beyond h_T |lse|, in units of 2^-24 (1 + sum), is __logf's.  Prints the largest of each
    and pins EXPF_C and LOGF_C: both stay within the constants (twice the largest seen)."""
    c = C._self(f"ulps-{R.DT_NAME[dt]}", dt, 1, 256, 2)
    _set_knobs(knobs, c)
    g = torch.Generator().manual_seed(11)
    h = C.host_self(c, "gauss")
    h.qkv[:, :, :2] = torch.randint(-3, 4, h.qkv[:, :, :2].shape, generator=g).double()
    r = C.reference_self(h)
    assert torch.equal(r.S * 8, (r.S * 8).round()) and r.S.abs().max() < 2 ** 20
    got = _run_self(dev, c, h)
    arg = r.S - r.S.max(-1, keepdim=True).values
    e = torch.exp(arg)
    live = e > 1e-30
    ratio = got["P"] / got["P"].max(-1, keepdim=True).values
    m = ((ratio - e).abs()[live] / (U24 * (1 + arg.abs()) * e)[live]).max().item()
    print(f"attnref expf-ulps {m:.3f} {c.id} (max |arg| {arg[live].abs().max().item():.1f})")
    ml = 0.0
    if c.lse:
        s = torch.exp(r.lse - r.S.max(-1).values)
        over = ((got["lse"] - r.lse).abs() - U24 * r.lse.abs()).clamp(min=0)
        ml = (over / (U24 * (1 + s))).max().item()
        print(f"attnref logf-ulps {ml:.3f} {c.id} (sums {s.min().item():.2f} .. {s.max().item():.1f})")
    assert m <= R.EXPF_C, f"__expf error {m:.2f} x 2^-24 (1 + |arg|)"
    assert ml <= R.LOGF_C, f"__logf error {ml:.2f} x 2^-24 (1 + sum)"


# --------------------------------------------------------------------------- cross-attention
@pytest.mark.parametrize("cid", C.ids("cross", "gauss"))
def test_cross_attention(dev, knobs, cid):
    c = C.BY_ID[cid]
    h = C.host_cross(c)
    r = C.reference_cross(h)
    lib = L.lib()
    dc = L.dtype_code(c.dt)
    B, Lq, Lk, H = c.B, c.Lq, c.Lk, c.H
    st = L.stream()
    qrows = torch.full((B * Lq, c.ldq), NAN, dtype=torch.float64)      # ldq padding is NaN
    qrows[:, :64 * H] = h.q.reshape(B * Lq, 64 * H)
    q, kv, do = _in(dev, qrows, c.dt), _in(dev, h.kv, c.dt), _in(dev, h.dout, c.dt)
    ctr = torch.tensor([C.COUNTER0], dtype=torch.int64, device=dev)
    out = _Buf(dev, (B, Lq, H, 64), c.dt)
    probs = _Buf(dev, (B, H, Lq, Lk), F32)
    L.call("mmdx_xattn_fwd", dc, q.ptr, c.ldq, kv.ptr, B, Lq, Lk, H, c.scale, c.p, C.SEED,
           ctr.data_ptr(), out.ptr, probs.ptr, st)
    torch.cuda.synchronize()
    out.check_guards(f"{cid}: out")
    probs.check_guards(f"{cid}: probs")
    assert int(ctr.item()) == C.COUNTER0 + (1 if c.p > 0 else 0), f"{cid}: launch counter"
    pr = probs.body().cpu()
    assert torch.equal(~torch.signbit(pr), r.keep.bool()), f"{cid}: keep bits differ from keep_mask"
    n = lib.mmdx_xattn_workspace_size(B, Lq, Lk, H)
    assert n == R.xattn_workspace_size(B, Lq, Lk, H)
    ws = _Buf(dev, (n // 4,), F32)
    dq0 = torch.full((B * Lq, c.lddq), SENT, dtype=torch.float64)      # lddq padding: untouched
    dq0[:, :64 * H] = NAN
    dq = _Buf(dev, dq0.shape, c.dt, data=dq0)
    dkv = _Buf(dev, (B, Lk, 2, H, 64), c.dt)
    pb = probs.dev.cpu().clone()
    L.call("mmdx_xattn_bwd", dc, q.ptr, c.ldq, kv.ptr, probs.ptr, do.ptr, B, Lq, Lk, H, c.scale,
           c.p, dq.ptr, c.lddq, dkv.ptr, ws.ptr, n, st)
    torch.cuda.synchronize()
    for t, name in ((ws, "workspace"), (dq, "dq"), (dkv, "dkv")):
        t.check_guards(f"{cid}: {name}")
    assert _same_bits(probs.dev, pb), f"{cid}: probs changed in the backward"
    for t, name in ((q, "q"), (kv, "kv"), (do, "dout")):
        t.check_unchanged(f"{cid}: {name}")
    dqg = dq.f64()
    assert (dqg[:, 64 * H:] == SENT).all(), f"{cid}: dq's padding columns written"
    b = R.bounds(r, c.dt, round_ops=False)
    R.check_bounded("x-out", out.f64(), r.O, b.out, cid)
    R.check_bounded("x-P", pr.double().abs(), r.P, b.P, cid)
    R.check_bounded("x-dQ", dqg[:, :64 * H].reshape(B, Lq, H, 64), r.dq, b.dq, cid)
    R.check_bounded("x-dK", dkv.f64()[:, :, 0], r.dk, b.dk, cid)
    R.check_bounded("x-dV", dkv.f64()[:, :, 1], r.dv, b.dv, cid)
    RAN.add((cid, "gauss"))


# ------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("cid", C.ids("decode", "gauss"))
def test_decode_step(dev, knobs, cid):
    """out against the reference; cache row (r, pos) equals this step's K / V bit for bit and
    every other cache element is untouched."""
    c = C.BY_ID[cid]
    h = C.host_decode(c)
    r = R.decode_step(h.qkv, h.kc, h.vc, h.slots, h.bias, c.pos)
    qkv = _in(dev, h.qkv, c.dt)
    kc, vc = _in(dev, h.kc, c.dt), _in(dev, h.vc, c.dt)
    b0 = torch.full_like(h.bias, NAN)                # nothing but row pos, keys <= pos, is read
    b0[:, c.pos, :c.pos + 1] = h.bias[:, c.pos, :c.pos + 1]
    bias = _in(dev, b0, F32)
    slots = h.slots.to(dev)
    out = _Buf(dev, (c.R, c.H, 64), c.dt)
    L.call("mmdx_t5_decode_attn", L.dtype_code(c.dt), qkv.ptr, c.R, c.H, c.pos, c.Lmax, kc.ptr,
           vc.ptr, slots.data_ptr(), bias.ptr, out.ptr, L.stream())
    torch.cuda.synchronize()
    out.check_guards(f"{cid}: out")
    for t, want, name in ((kc, r.kc, "k cache"), (vc, r.vc, "v cache")):
        t.check_guards(f"{cid}: {name}")
        assert _same_bits(t.body(), want.to(c.dt)), \
            f"{cid}: {name} is not the old cache with this step's row at pos"
    qkv.check_unchanged(f"{cid}: qkv")
    bias.check_unchanged(f"{cid}: bias")
    assert torch.equal(slots.cpu(), h.slots)
    b = R.bounds(r, c.dt, round_ops=False)
    R.check_bounded("decode", out.f64()[:, None], r.O, b.out, cid)
    RAN.add((cid, "gauss"))


# ----------------------------------------------------------------------------- position bias
@pytest.mark.parametrize("family", ["int", "gauss"])
@pytest.mark.parametrize("cid", C.ids("posbias", "int"))
def test_position_bias(dev, knobs, cid, family):
    """bias = table[bucket] exactly; dtable = beta dtable + the bucket sums of dS over cells
    k <= q: equal to the reference for integer dS, within ACC sum |terms| for Gaussian dS.  The
    dS rows are LP wide with NaN padding columns, as mmdx_attention_bwd's workspace is."""
    c = C.BY_ID[cid]
    h = C.host_posbias(c, family)
    dev_t = _in(dev, h.table, F32)
    bias = _Buf(dev, (c.H, c.L, c.L), F32)
    L.call("mmdx_t5_position_bias", dev_t.ptr, c.H, c.L, c.nb, c.maxd, bias.ptr, L.stream())
    torch.cuda.synchronize()
    bias.check_guards(f"{cid}: bias")
    R.assert_exact(bias.f64(), R.position_bias(h.table, c.L, c.nb, c.maxd), f"{cid}: bias")
    ds = _in(dev, h.ds, c.dt)
    dt0 = torch.full((c.nb, c.H), NAN, dtype=torch.float64) if c.beta == 0.0 else h.dtable0
    dtab = _Buf(dev, (c.nb, c.H), F32, data=dt0)
    L.call("mmdx_t5_position_bias_bwd", L.dtype_code(c.dt), ds.ptr, c.B, c.H, c.L, h.LP, c.nb,
           c.maxd, dtab.ptr, c.beta, L.stream())
    torch.cuda.synchronize()
    dtab.check_guards(f"{cid}: dtable")
    ds.check_unchanged(f"{cid}: dS")
    dev_t.check_unchanged(f"{cid}: table")
    ref, terms = R.position_bias_bwd(h.ds, c.nb, c.maxd, h.dtable0, c.beta)
    if family == "int":
        assert terms.max() < 2 ** 24 and torch.equal(ref, ref.round())
        R.assert_exact(dtab.f64(), ref, f"{cid}: dtable")
    else:
        R.check_bounded("dtable", dtab.f64(), ref, U24 * ref.abs() + R.ACC * terms, cid)
    RAN.add((cid, family))


# --------------------------------------------------------------------------------- coverage
def test_every_case_ran():
    """Every case of the table ran in every family it lists (this file run whole, unfiltered)."""
    want = {(c.id, f) for c in C.CASES for f in c.families}
    assert want - RAN == set(), sorted(want - RAN)
