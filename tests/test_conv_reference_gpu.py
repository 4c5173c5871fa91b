"""The implicit-GEMM conv entry points of csrc/conv.hip against the fp64 reference of
tests/conv_ref.py, element by element, at the smallest shapes that reach each path of the
dispatcher (ragged M / N tiles, ragged K tails, odd-sized and unreached dgrad phases, every
split-K tile and both split reductions, the fp32 kernels; tests/test_conv_ref_cpu.py asserts
which case reaches which path).

Two operand families:
  * integer: x, w, dy in {-1, 0, 1}.  Every product and partial sum is a small integer that an
    fp32 accumulator holds exactly in any summation order, K-tile order or split-K grouping, so
    pack, fwd, dgrad (beta 0, beta 1, accmask) and wgrad (beta 0, beta 1) must EQUAL the
    reference.  The preconditions (integer reference, |ref| <= 256 where stored in bf16, fewer
    than 2^24 terms) are asserted from the reference before any launch.  The forward's
    BatchNorm slabs (mean, M2 per 128 rows) are no integers: every slab and channel within
    TOL[fp32] of the statistic's largest magnitude, in a buffer preset to NaN.
  * Gaussian (a subset): fp32 accumulation, one rounding on store, per element
    |got - ref| <= h_T |ref| + 2e-5 sum |terms|, h_T = 2^-8 (bf16) or 2^-24 (fp32, and every
    dW), the reference on operands already rounded to the compute dtype.
    mmdx_conv_fwd_bn_eval: h_T |ref| + 2e-5 (|scale| sum |terms| + |shift| + |res|).  Its
    epilogue (igemm.h EpiBnEval) applies scale and shift to the fp32 accumulators: the conv
    result is NOT rounded before the BatchNorm, so the bound has no |scale| h_T |conv| term.
Every bounded check prints "convref <kind> <error / bound>" before it asserts.

Measured on an MI355X: every integer-family comparison is an equality, and the largest error /
bound per kind is fwd 0.978, dgrad 0.975, wgrad 0.012, bn-eval 0.983, stats 0.014 (the bf16
ratios are the store's rounding: half an ulp just above a power of two is 2^-8 |ref|; the fp32
case's are 0.008 / 0.009 / 0.012 / 0.010).  The kernels needed no fix.  The checks do bite: a
library whose wgrad_reduce_kernel skips its tail splits fails exactly the cases with more than
8 splits and a tail (11, 12, 18, 24, 25).
"""
import functools
from types import SimpleNamespace

import pytest
import torch

import bn_ref
import conv_ref as R
import mmdx._lib as L
from conv_ref import F32
from test_kernels_gpu import TOL

pytestmark = pytest.mark.gpu

TOL32 = TOL[torch.float32]
EPS = 1e-3   # visible in rstd at TOL[fp32] (1e-5 is not: tests/test_bn_reference_gpu.py)
KNOB_NAMES = sorted({k for _, kn in R.KNOB_RUNS for k in kn})

EXACT_RUNS = [(cid, None) for cid in list(R.CASES_BF16) + list(R.CASES_F32)] + R.KNOB_RUNS


def _id(run):
    cid, kn = run
    tag = f"c{cid:02d}" if isinstance(cid, int) else cid
    return tag + "".join(f"-{k[5:]}={v}" for k, v in (kn or {}).items())


def _desc(cfg):
    N, C, H, W, K, Rr, S, sh, sw, ph, pw = cfg
    P, Q = R.out_size(cfg)
    return L.ConvDesc(N, H, W, C, K, Rr, S, sh, sw, ph, pw, P, Q)


# ------------------------------------------------------------------------------- host data
@functools.lru_cache(maxsize=None)
def _host(cid, family):
    """Operands and fp64 references of one case.  Shared by the tests; never modified."""
    cfg, cm, dt = R.case(cid)
    N, C, H, W, K, Rr, S = cfg[:7]
    P, Q = R.out_size(cfg)
    h = SimpleNamespace(cfg=cfg, cm=cm, dt=dt, P=P, Q=Q)
    h.x, h.w, h.dy, g = R.operands(cid, family)
    h.wgrad_only = cid in R.WGRAD_ONLY
    wp = R.pad_c(h.w, C)
    if not h.wgrad_only:
        h.y = R.ref_fwd(h.x, h.w, cfg)
        h.dx = R.ref_dgrad(h.dy, wp, cfg)              # [N, C, H, W]: padded lanes are 0
        assert (h.dx[:, cm:] == 0).all()
    h.dw = R.ref_wgrad(h.x, h.dy, cfg)                 # master shape [K, cm, R, S]
    if family == "int":
        h.dw0 = R.gen_integer((K, cm, Rr, S), g)
        if not h.wgrad_only:
            h.dx0 = R.pad_c(R.gen_integer((N, cm, H, W), g), C)
            h.src = R.pad_c(R.gen_integer((N, cm, H, W), g), C)
            h.bits = torch.rand(N, H, W, C, generator=g) > 0.5
    else:
        if not h.wgrad_only:
            h.y_abs = R.ref_abs_fwd(h.x, h.w, cfg)
            h.dx_abs = R.ref_abs_dgrad(h.dy, wp, cfg)
        h.dw_abs = R.ref_abs_wgrad(h.x, h.dy, cfg)
        h.gam = torch.rand(K, generator=g) + 0.5
        h.gam[::5] *= -1.0
        h.bet = torch.randn(K, generator=g) * 0.3
        h.rm = torch.randn(K, generator=g) * 0.3
        h.rv = torch.rand(K, generator=g) + 0.5
        h.res = R.gen_gaussian((N, K, P, Q), g, dt)
    return h


def _exact_preconditions(h):
    """From the reference alone, before any launch."""
    cfg, cm, dt = h.cfg, h.cm, h.dt
    N, C, H, W, K, Rr, S = cfg[:7]
    for t in (h.x, h.w, h.dy, h.dw0):
        assert set(t.unique().tolist()) <= {-1.0, 0.0, 1.0}
    if not h.wgrad_only:
        assert set(h.dx0.unique().tolist()) | set(h.src.unique().tolist()) <= {-1.0, 0.0, 1.0}
        R.check_exact_preconditions(h.y, cm * Rr * S, dt, "y")
        R.check_exact_preconditions(h.dx, K * Rr * S, dt, "dx")
        R.check_exact_preconditions(h.dx + h.dx0, K * Rr * S + 1, dt, "dx0 + dgrad")
        masked = torch.where(h.bits.permute(0, 3, 1, 2), h.src, torch.zeros_like(h.src))
        R.check_exact_preconditions(h.dx + masked, K * Rr * S + 1, dt, "dgrad + masked source")
    R.check_exact_preconditions(h.dw, N * h.P * h.Q, F32, "dw")
    R.check_exact_preconditions(h.dw + h.dw0, N * h.P * h.Q + 1, F32, "dw0 + wgrad")


# ------------------------------------------------------------------------------ device calls
def _nan(shape, dt, dev):
    return torch.full(shape, float("nan"), dtype=dt, device=dev)


def _pack(dev, h):
    cfg, dt = h.cfg, h.dt
    N, C, H, W, K, Rr, S = cfg[:7]
    wm = h.w.float().contiguous().to(dev)
    wk, wc = _nan((K, Rr, S, C), dt, dev), _nan((C, Rr, S, K), dt, dev)
    L.call("mmdx_conv_pack_weight", L.dtype_code(dt), _desc(cfg), h.cm, wm.data_ptr(),
           wk.data_ptr(), wc.data_ptr(), L.stream())
    torch.cuda.synchronize()
    return wk, wc


def _fwd(dev, h, xd, wk, stats):
    cfg, dt = h.cfg, h.dt
    d = _desc(cfg)
    y = _nan((cfg[0], h.P, h.Q, cfg[4]), dt, dev)
    part = None
    if stats:
        part = _nan((cfg[4], L.lib().mmdx_conv_fwd_stat_blocks(d), 2), F32, dev)
    L.call("mmdx_conv_fwd", L.dtype_code(dt), d, xd.data_ptr(), wk.data_ptr(), y.data_ptr(),
           L.ptr(part), L.stream())
    torch.cuda.synchronize()
    return y, part


def _dgrad(dev, h, dyd, wc, beta, dx0=None):
    cfg, dt = h.cfg, h.dt
    N, C, H, W = cfg[:4]
    dx = _nan((N, H, W, C), dt, dev) if dx0 is None else R.to_nhwc(dx0, C, dt).to(dev)
    L.call("mmdx_conv_dgrad", L.dtype_code(dt), _desc(cfg), dyd.data_ptr(), wc.data_ptr(),
           dx.data_ptr(), beta, L.stream())
    torch.cuda.synchronize()
    return dx


def _wgrad(dev, h, xd, dyd, beta, dw0=None):
    """Returns dW [K, c_master, R, S] (the master shape) after checking that nothing was written
    behind it."""
    cfg, dt = h.cfg, h.dt
    K, Rr, S = cfg[4:7]
    n, guard = K * h.cm * Rr * S, 64
    buf = torch.full((n + guard,), -7.0, device=dev)
    buf[:n] = float("nan") if dw0 is None else dw0.float().reshape(-1).to(dev)
    ws_n = L.lib().mmdx_conv_wgrad_workspace_size(L.dtype_code(dt), _desc(cfg))
    ws = torch.full((ws_n // 4,), float("nan"), device=dev)
    L.call("mmdx_conv_wgrad", L.dtype_code(dt), _desc(cfg), h.cm, xd.data_ptr(), dyd.data_ptr(),
           buf.data_ptr(), beta, ws.data_ptr(), ws_n, L.stream())
    torch.cuda.synchronize()
    assert (buf[n:] == -7.0).all(), "wgrad wrote past the master-shaped dW"
    return buf[:n].view(K, h.cm, Rr, S)


def _check_stats(part, y_ref, rows, what):
    """Every slab and channel of the epilogue's (mean, M2) against the fp64 slab values."""
    ref = R.slab_stats(y_ref, rows).double()
    got = part.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: slabs {tuple(got.shape)} != {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: a statistics slab was not written"
    worst = 0.0
    for j, name in enumerate(("mean", "M2")):
        bound = (TOL32 * ref[..., j].abs().max()).expand_as(ref[..., j])
        worst = max(worst, R.bound_ratio(got[..., j], ref[..., j], bound))
    print(f"convref stats {worst:.4f} {what}")
    assert worst <= 1.0, f"{what}: stats error / bound = {worst:.3f}"


# ============================================================================ integer family
@pytest.mark.parametrize("run", EXACT_RUNS, ids=_id)
def test_conv_exact(dev, knobs, run):
    """pack, fwd (+ statistics slabs), dgrad at beta 0 / beta 1 / accmask and wgrad at beta 0 /
    beta 1 with integer operands: equal to the fp64 reference, element for element."""
    cid, kn = run
    h = _host(cid, "int")
    _exact_preconditions(h)
    for name in KNOB_NAMES:
        knobs(name, (kn or {}).get(name))
    cfg, cm, dt = h.cfg, h.cm, h.dt
    N, C, H, W, K, Rr, S, sh, sw, ph, pw = cfg
    what, dc, d = _id(run), L.dtype_code(dt), _desc(cfg)
    path = R.expected_path(cfg, dt, kn)

    # what the library exposes about its path
    ws_n = L.lib().mmdx_conv_wgrad_workspace_size(dc, d)
    assert ws_n == path.plan.splits * 4 * K * Rr * S * C, f"{what}: wgrad splits"
    if cid == 19:
        assert ws_n >= 128 * 4 * K * Rr * S * C
    rows = L.lib().mmdx_conv_fwd_stat_rows(d)
    M = N * h.P * h.Q
    assert rows == 128 and L.lib().mmdx_conv_fwd_stat_blocks(d) == (M + rows - 1) // rows
    assert L.lib().mmdx_conv_dgrad_stat_blocks(dc, d) == R.dgrad_stat_blocks(cfg, dt)

    wk, wc = _pack(dev, h)
    R.assert_exact(wk, R.pack_krsc(h.w, C, dt).double(), f"{what}: packed KRSC")
    R.assert_exact(wc, R.pack_crsk(h.w, C, dt).double(), f"{what}: packed CRSK")
    xd = R.to_nhwc(h.x, C, dt).to(dev)
    dyd = R.to_nhwc(h.dy, K, dt).to(dev)

    if not h.wgrad_only:
        y, part = _fwd(dev, h, xd, wk, True)
        R.assert_exact(R.from_nhwc(y), h.y, f"{what}: fwd")
        _check_stats(part, h.y, rows, what)

        reach = R.reached(cfg)
        dx = R.from_nhwc(_dgrad(dev, h, dyd, wc, 0.0))
        R.assert_exact(dx, h.dx, f"{what}: dgrad beta 0")
        assert (dx[:, :, ~reach] == 0).all(), f"{what}: dx where no tap reaches, beta 0"
        assert (dx[:, cm:] == 0).all(), f"{what}: padded channels of dx"
        dx = R.from_nhwc(_dgrad(dev, h, dyd, wc, 1.0, h.dx0))
        R.assert_exact(dx, h.dx + h.dx0, f"{what}: dgrad beta 1")
        assert torch.equal(dx[:, :, ~reach], h.dx0[:, :, ~reach]), \
            f"{what}: dx where no tap reaches, beta 1"
        assert (dx[:, cm:] == 0).all(), f"{what}: padded channels of dx, beta 1"
        if sh == 1 and sw == 1:
            src = R.to_nhwc(h.src, C, dt).to(dev)
            mask = bn_ref.pack_mask(h.bits.view(-1, C), R.vec(dt)).to(dev)
            got = _nan((N, H, W, C), dt, dev)
            L.call("mmdx_conv_dgrad_accmask", dc, d, dyd.data_ptr(), wc.data_ptr(),
                   got.data_ptr(), src.data_ptr(), mask.data_ptr(), L.stream())
            torch.cuda.synchronize()
            want = h.dx + torch.where(h.bits.permute(0, 3, 1, 2), h.src, torch.zeros_like(h.src))
            R.assert_exact(R.from_nhwc(got), want, f"{what}: dgrad accmask")

    dw = _wgrad(dev, h, xd, dyd, 0.0)
    R.assert_exact(dw, h.dw, f"{what}: wgrad beta 0")
    dw = _wgrad(dev, h, xd, dyd, 1.0, h.dw0)
    R.assert_exact(dw, h.dw + h.dw0, f"{what}: wgrad beta 1")


# =========================================================================== Gaussian family
@pytest.mark.parametrize("cid", R.GAUSSIAN, ids=lambda c: _id((c, None)))
def test_conv_gaussian(dev, knobs, cid):
    """fwd, dgrad and wgrad with Gaussian operands: fp32 accumulation and one rounding."""
    h = _host(cid, "gauss")
    for name in KNOB_NAMES:
        knobs(name, None)
    cfg, cm, dt = h.cfg, h.cm, h.dt
    C, K = cfg[1], cfg[4]
    what = _id((cid, None))
    wk, wc = _pack(dev, h)
    R.assert_exact(wk, R.pack_krsc(h.w, C, dt).double(), f"{what}: packed KRSC")
    xd = R.to_nhwc(h.x, C, dt).to(dev)
    dyd = R.to_nhwc(h.dy, K, dt).to(dev)
    y, _ = _fwd(dev, h, xd, wk, False)
    R.assert_bounded("fwd", R.from_nhwc(y), h.y, h.y_abs, dt, what)
    dx = R.from_nhwc(_dgrad(dev, h, dyd, wc, 0.0))
    R.assert_bounded("dgrad", dx, h.dx, h.dx_abs, dt, what)
    assert (dx[:, :, ~R.reached(cfg)] == 0).all() and (dx[:, cm:] == 0).all()
    dw = _wgrad(dev, h, xd, dyd, 0.0)
    R.assert_bounded("wgrad", dw, h.dw, h.dw_abs, F32, what)


@pytest.mark.parametrize("cid", R.GAUSSIAN, ids=lambda c: _id((c, None)))
def test_conv_fwd_bn_eval_gaussian(dev, knobs, cid):
    """mmdx_conv_fwd_bn_eval = act(conv * scale + shift (+ residual)) for residual + ReLU, ReLU
    only and neither; scale and shift in fp64 from the fp32 vectors the kernel reads."""
    h = _host(cid, "gauss")
    for name in KNOB_NAMES:
        knobs(name, None)
    cfg, dt = h.cfg, h.dt
    N, C, K = cfg[0], cfg[1], cfg[4]
    wk, _ = _pack(dev, h)
    xd = R.to_nhwc(h.x, C, dt).to(dev)
    resd = R.to_nhwc(h.res, K, dt).to(dev)
    bn = [t.to(dev) for t in (h.gam, h.bet, h.rm, h.rv)]
    scale = h.gam.double() / torch.sqrt(h.rv.double() + EPS)
    shift = h.bet.double() - h.rm.double() * scale
    sc, sf = scale.view(1, K, 1, 1), shift.view(1, K, 1, 1)
    for use_res, relu in ((1, 1), (0, 1), (0, 0)):
        what = f"{_id((cid, None))} res={use_res} relu={relu}"
        ref = h.y * sc + sf
        fp32_terms = sc.abs() * h.y_abs + sf.abs()
        if use_res:
            ref = ref + h.res
            fp32_terms = fp32_terms + h.res.abs()
        if relu:
            ref = ref.clamp(min=0.0)
        out = _nan((N, h.P, h.Q, K), dt, dev)
        L.call("mmdx_conv_fwd_bn_eval", L.dtype_code(dt), _desc(cfg), xd.data_ptr(),
               wk.data_ptr(), out.data_ptr(), *[t.data_ptr() for t in bn], EPS,
               resd.data_ptr() if use_res else None, relu, L.stream())
        torch.cuda.synchronize()
        R.assert_bounded("bn-eval", R.from_nhwc(out), ref, fp32_terms, dt, what)
