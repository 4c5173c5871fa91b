"""The BatchNorm entry points of csrc/norm.hip against the fp64 reference of tests/bn_ref.py, at
the smallest shapes that reach each layout and code path of the kernels.

Tolerances are derived, not tuned.  The reference sees the same dtype-rounded inputs as the
kernels, which compute in fp32 and round once on store (TOL is test_kernels_gpu's table):
  * tensors stored in dtype T (y, dx, d_residual), per element:
    |out - ref| <= h_T |ref| + TOL[fp32] max|ref|, h_T one rounding (2^-8 bf16, 2^-24 fp32);
  * per-channel fp32 vectors (mean, rstd, running stats, scale, shift): TOL[fp32] times the
    vector's largest magnitude;
  * dgamma / dbeta, per channel: TOL[fp32] sum_r |term| (the worst case of an fp32 summation
    chain of about 300 additions; no shape here has a longer one) + |beta_acc preload| 2^-23.
Every check prints "bnref <kind> <error / bound>" before it asserts."""
import functools
from types import SimpleNamespace

import pytest
import torch

import bn_ref
import mmdx._lib as L
from bn_ref import _wide_rows
from test_kernels_gpu import TOL

pytestmark = pytest.mark.gpu

TOL32 = TOL[torch.float32]
H_T = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
# eps = 1e-3 (the Keras default), not torch's 1e-5: with inputs of unit scale 1e-5 moves rstd by
# a few 1e-6, below TOL[fp32], so a kernel that dropped eps would pass; 1e-3 moves it by about
# 1e-4.  It also keeps the 2-row case meaningful: there the train-mode dx is gamma g O(eps / var)
# (it is identically 0 without eps), which at 1e-5 is below the rounding of any fp32 evaluation.
EPS, MOM = 1e-3, 0.1
BF16, F32 = torch.bfloat16, torch.float32

# (rows, C): one bf16 vector (ct = 1) | cv does not divide 256 (fp32: 12 channel threads x 21
# row threads, 4 idle threads alias the next row) | the pair test's smallest | cgroups > 1 and
# 256 vectors in bf16 | ragged last channel group, the apply's j loop runs twice | bf16 cv = 257:
# the second j iteration has one live thread | more than fin_wide() slabs | fp32 only: C < 8
SHAPES = [(2, 8), (37, 48), (98, 64), (37, 2048), (5, 2304), (3, 2056), (None, 64), (21, 4)]
# Every shape above gives a reduce thread ONE row of its slab (bn_layout keeps rows_per_block at
# the row-thread count until rows exceed 2048 * rt / cgroups).  This one is just past that for
# both dtypes: fp32 12-row slabs over 4 row threads (3 rows each; the last slab holds 1 row, so
# three of its row threads have none), bf16 8-row slabs (2 rows each; the last holds 5: 2, 1, 1,
# 1).  2048 * 256 * (4 | 8) elements is the least that reaches it, so it has a test of its own
# with fewer mode combinations (test_bn_threads_with_several_rows), not the full crosses.
SEVERAL = len(SHAPES)
SHAPES.append((2101, 2048))
CASES = [(s, dt) for s in range(SEVERAL) for dt in (BF16, F32)
         if SHAPES[s][1] % (8 if dt == BF16 else 4) == 0]
IDS = [f"{SHAPES[s][0] or 'wide'}x{SHAPES[s][1]}-{'bf16' if dt == BF16 else 'fp32'}"
       for s, dt in CASES]


def _vec(dt):
    return 8 if dt == BF16 else 4


def _round(t, dt):
    """The values of t on the compute dtype's grid, as fp64."""
    return t.to(dt).double()


def _report(kind, err, bound, what):
    exact = bound == 0     # (e.g. a channel whose mask is all zeros: every term is 0)
    assert (err[exact] == 0).all(), f"{what}: {kind} must be exact where every term is zero"
    ratio = (err[~exact] / bound[~exact]).max().item() if (~exact).any() else 0.0
    print(f"bnref {kind} {ratio:.4f} {what}")
    assert ratio <= 1.0, f"{what}: {kind} error / bound = {ratio:.3f}"


def _check_tensor(out, ref, dt, kind, what):
    """A tensor stored in dtype dt, elementwise."""
    out = out.detach().double().cpu()
    assert torch.isfinite(out).all(), what
    _report(kind, (out - ref).abs(), H_T[dt] * ref.abs() + TOL32 * ref.abs().max(), what)


def _check_vector(out, ref, kind, what):
    """A per-channel fp32 vector."""
    out = out.detach().double().cpu()
    assert torch.isfinite(out).all(), what
    _report(kind, (out - ref).abs(), (TOL32 * ref.abs().max()).expand_as(ref), what)


def _check_sum(out, ref, sum_abs, preload, kind, what):
    """dgamma / dbeta: fp32 sums over the rows of terms whose magnitudes add up to sum_abs."""
    out = out.detach().double().cpu()
    assert torch.isfinite(out).all(), what
    _report(kind, (out - ref).abs(), TOL32 * sum_abs + preload.abs() * 2.0 ** -23, what)


def _ws(rows, C, dev):
    n = L.lib().mmdx_bn_workspace_size(rows, C)
    assert n == bn_ref.workspace_size(rows, C) > 0
    return torch.empty(n, dtype=torch.uint8, device=dev), n


@functools.lru_cache(maxsize=None)
def _host_case(s, dt):
    """Host inputs of one (shape, dtype) case, the tensors on the dtype's grid (fp64), the
    per-channel vectors fp32 as the kernels read them.  Shared by the tests; never modified."""
    rows, C = SHAPES[s]
    if rows is None:
        rows = _wide_rows(C)
    g = torch.Generator().manual_seed(1000 + s)
    d = SimpleNamespace(rows=rows, C=C)
    # Two rows have xhat = +-sqrt(var / (var + eps)), and the train-mode dx is gamma * g times
    # O(eps / var): its terms cancel to that fraction, so its condition number is var / eps and
    # a bound relative to max|dx| is well posed for fp32 (2^-24 per term against TOL[fp32])
    # only while var / eps stays below about 100.  Hence a spread of 0.2 (var ~ 0.02 = 20 eps)
    # for the 2-row case; 2 elsewhere.
    spread = 0.2 if rows == 2 else 2.0
    d.x = _round(torch.randn(rows, C, generator=g) * spread + torch.linspace(-1.5, 1.5, C), dt)
    d.res = _round(torch.randn(rows, C, generator=g), dt)
    d.dy = _round(torch.randn(rows, C, generator=g), dt)
    d.gam = torch.rand(C, generator=g) + 0.5
    d.gam[::7] *= -1.0
    d.bet = torch.randn(C, generator=g) * 0.3
    d.rm = torch.randn(C, generator=g) * 0.2
    d.rv = torch.rand(C, generator=g) + 0.5
    d.bits = torch.rand(rows, C, generator=g) > 0.4          # a ReLU mask unrelated to y
    d.acc = [torch.randn(C, generator=g) for _ in range(2)]  # dgamma / dbeta preloads
    return d


# =============================================================================== forward
# (residual, relu, mask): a mask needs relu
FWD_COMBOS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1)]


def _fwd_ex(dev, dt, train, x, rows, C, gam, bet, rm, rv, res, relu, want_y, want_mask, ws, ws_n,
            stat=None):
    """mmdx_bn_fwd_ex; returns mean, rstd, y, mask (device tensors or None)."""
    mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    y = torch.empty(rows, C, dtype=dt, device=dev) if want_y else None
    mask = (torch.full((rows, C // _vec(dt)), 0xA5, dtype=torch.uint8, device=dev)
            if want_mask else None)
    part, nblk, stat_rows = stat if stat else (None, 0, 0)
    L.call("mmdx_bn_fwd_ex", L.dtype_code(dt), train, x.data_ptr(), rows, C, L.ptr(part), nblk,
           stat_rows, L.ptr(gam), L.ptr(bet), L.ptr(rm), L.ptr(rv), MOM, EPS, mean.data_ptr(),
           rstd.data_ptr(), L.ptr(res), relu, L.ptr(y), L.ptr(mask), ws.data_ptr(), ws_n,
           L.stream())
    torch.cuda.synchronize()
    return mean, rstd, y, mask


def _check_mask(mask, y, dt, what):
    """The mask bytes against the bits of the device's own stored y."""
    want = bn_ref.pack_mask(y.cpu().float() > 0, _vec(dt))
    assert torch.equal(mask.cpu(), want), f"{what}: mask bytes"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bn_fwd_ex(dev, case):
    s, dt = case
    d = _host_case(s, dt)
    rows, C = d.rows, d.C
    x, res = d.x.to(dev, dt), d.res.to(dev, dt)
    gam, bet = d.gam.to(dev), d.bet.to(dev)
    ws, ws_n = _ws(rows, C, dev)
    for train in (1, 0):
        for use_res, relu, use_mask in FWD_COMBOS:
            what = f"train={train} res={use_res} relu={relu} mask={use_mask}"
            ref = bn_ref.bn_forward(d.x, d.gam, d.bet, d.rm, d.rv, MOM, EPS,
                                    d.res if use_res else None, bool(relu), bool(train))
            rm, rv = d.rm.to(dev), d.rv.to(dev)
            mean, rstd, y, mask = _fwd_ex(dev, dt, train, x, rows, C, gam, bet, rm, rv,
                                          res if use_res else None, relu, True, use_mask, ws, ws_n)
            _check_tensor(y, ref.y, dt, "y", what)
            _check_vector(rstd, ref.rstd, "rstd", what)
            if train:
                _check_vector(mean, ref.mean, "mean", what)
                _check_vector(rm, ref.running_mean, "running_mean", what)
                _check_vector(rv, ref.running_var, "running_var", what)
            else:  # eval: the running statistics normalise and stay as they are
                assert torch.equal(mean.cpu(), d.rm) and torch.equal(rm.cpu(), d.rm), what
                assert torch.equal(rv.cpu(), d.rv), what
            if use_mask:
                _check_mask(mask, y, dt, what)


@pytest.mark.parametrize("dt", [BF16, F32])
def test_bn_fwd_ex_null_affine_and_statistics_only(dev, dt):
    """gamma == NULL and beta == NULL (1 and 0), no running statistics; and y == NULL: the
    statistics and the running update alone."""
    s = 1
    d = _host_case(s, dt)
    rows, C = d.rows, d.C
    x = d.x.to(dev, dt)
    ws, ws_n = _ws(rows, C, dev)
    ref = bn_ref.bn_forward(d.x, None, None, None, None, MOM, EPS, None, True, True)
    mean, rstd, y, mask = _fwd_ex(dev, dt, 1, x, rows, C, None, None, None, None, None, 1, True,
                                  True, ws, ws_n)
    _check_tensor(y, ref.y, dt, "y", "null affine")
    _check_vector(mean, ref.mean, "mean", "null affine")
    _check_vector(rstd, ref.rstd, "rstd", "null affine")
    _check_mask(mask, y, dt, "null affine")

    s = 2
    d = _host_case(s, dt)
    rows, C = d.rows, d.C
    ws, ws_n = _ws(rows, C, dev)
    ref = bn_ref.bn_forward(d.x, d.gam, d.bet, d.rm, d.rv, MOM, EPS, None, True, True)
    rm, rv = d.rm.to(dev), d.rv.to(dev)
    mean, rstd, y, _ = _fwd_ex(dev, dt, 1, d.x.to(dev, dt), rows, C, d.gam.to(dev),
                               d.bet.to(dev), rm, rv, None, 1, False, False, ws, ws_n)
    assert y is None
    _check_vector(mean, ref.mean, "mean", "statistics only")
    _check_vector(rstd, ref.rstd, "rstd", "statistics only")
    _check_vector(rm, ref.running_mean, "running_mean", "statistics only")
    _check_vector(rv, ref.running_var, "running_var", "statistics only")


# ================================================================= finalize from partials
STAT_ROWS = 3
# slabs: 1 | 2 | the last count of the one-wave finalize | the first of the 256-thread one | the
# last it holds in registers (256 x FIN_PER) | the first it re-reads from memory | the direct
# stem's slab count at batch 128 (one slab per 2 of 112 output rows)
NBLK = [1, 2, bn_ref.FIN_WIDE, bn_ref.FIN_WIDE + 1, bn_ref.FIN_REGS, bn_ref.FIN_REGS + 1, 7168]


@functools.lru_cache(maxsize=None)
def _slab_case(nblk, C, dt):
    """[rows, C] whose 3-row slabs have means several standard deviations apart and whose
    1-row last slab is an outlier, with its fp32 (mean, M2) slabs: a wrong weight of the last
    slab or a dropped n_b (mean_b - mean)^2 term moves the statistics far outside tolerance."""
    rows = (nblk - 1) * STAT_ROWS + 1
    g = torch.Generator().manual_seed(2000 + nblk)
    d = SimpleNamespace(rows=rows, C=C, nblk=nblk)
    off = (torch.randn(nblk, C, generator=g) * 5).repeat_interleave(STAT_ROWS, dim=0)[:rows]
    x = torch.randn(rows, C, generator=g) + off + torch.linspace(-3, 3, C)
    x[-1] += 40.0
    d.x = _round(x, dt)
    d.part = bn_ref.slab_stats(d.x, STAT_ROWS)
    assert d.part.shape == (C, nblk, 2)
    d.gam = torch.rand(C, generator=g) + 0.5
    d.gam[::3] *= -1.0
    d.bet = torch.randn(C, generator=g) * 0.3
    d.rm = torch.randn(C, generator=g) * 0.2
    d.rv = torch.rand(C, generator=g) + 0.5
    d.res = _round(torch.randn(rows, C, generator=g), dt)
    return d


@pytest.mark.parametrize("nblk", NBLK)
def test_bn_finalize_from_slabs(dev, nblk):
    """mmdx_bn_finalize alone (no x on the device).  C = 10 is no multiple of FIN_W, so the last
    one-wave block runs the c >= C guard: the outputs' tails must stay untouched."""
    C, pad = 10, 6
    d = _slab_case(nblk, C, F32)
    ref = bn_ref.bn_forward(d.x, d.gam, d.bet, d.rm, d.rv, MOM, EPS)
    part, gam, bet = d.part.to(dev), d.gam.to(dev), d.bet.to(dev)
    names = ("running_mean", "running_var", "mean", "rstd", "scale", "shift")
    out = {n: torch.full((C + pad,), -7.0, device=dev) for n in names}
    out["running_mean"][:C] = d.rm.to(dev)
    out["running_var"][:C] = d.rv.to(dev)
    L.call("mmdx_bn_finalize", part.data_ptr(), nblk, STAT_ROWS, d.rows, C,
           gam.data_ptr(), bet.data_ptr(), out["running_mean"].data_ptr(),
           out["running_var"].data_ptr(), MOM, EPS, out["mean"].data_ptr(),
           out["rstd"].data_ptr(), out["scale"].data_ptr(), out["shift"].data_ptr(), L.stream())
    torch.cuda.synchronize()
    for n in names:
        assert (out[n][C:] == -7.0).all(), f"{n}: written past C"
        _check_vector(out[n][:C], getattr(ref, n), n, f"finalize nblk={nblk}")


@pytest.mark.parametrize("nblk", [bn_ref.FIN_WIDE + 1, bn_ref.FIN_REGS + 1])
def test_bn_fwd_ex_from_slabs(dev, nblk):
    """The same slab construction through mmdx_bn_fwd_ex(stat_part=...) with a bf16 x (C = 16:
    bf16 needs whole 8-channel vectors), residual and ReLU: y."""
    C, dt = 16, BF16
    d = _slab_case(nblk, C, dt)
    ref = bn_ref.bn_forward(d.x, d.gam, d.bet, d.rm, d.rv, MOM, EPS, d.res, True, True)
    ws, ws_n = _ws(d.rows, C, dev)
    rm, rv = d.rm.to(dev), d.rv.to(dev)
    mean, rstd, y, mask = _fwd_ex(dev, dt, 1, d.x.to(dev, dt), d.rows, C, d.gam.to(dev),
                                  d.bet.to(dev), rm, rv, d.res.to(dev, dt), 1, True, True, ws,
                                  ws_n, stat=(d.part.to(dev), nblk, STAT_ROWS))
    what = f"fwd_ex from {nblk} slabs"
    _check_tensor(y, ref.y, dt, "y", what)
    _check_vector(mean, ref.mean, "mean", what)
    _check_vector(rstd, ref.rstd, "rstd", what)
    _check_vector(rm, ref.running_mean, "running_mean", what)
    _check_vector(rv, ref.running_var, "running_var", what)
    _check_mask(mask, y, dt, what)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bn_apply(dev, case):
    """mmdx_bn_apply alone: y = act(x * scale + shift (+ residual)) for given coefficients."""
    s, dt = case
    d = _host_case(s, dt)
    rows, C = d.rows, d.C
    x, res = d.x.to(dev, dt), d.res.to(dev, dt)
    scale, shift = d.gam, d.bet * 3
    scale_d, shift_d = scale.to(dev), shift.to(dev)
    for use_res, relu, use_mask in [(0, 0, 0), (1, 1, 1), (0, 1, 1), (1, 1, 0)]:
        what = f"apply res={use_res} relu={relu} mask={use_mask}"
        ref = d.x * scale.double() + shift.double()
        if use_res:
            ref = ref + d.res
        if relu:
            ref = torch.clamp(ref, min=0.0)
        y = torch.empty_like(x)
        mask = torch.full((rows, C // _vec(dt)), 0xA5, dtype=torch.uint8, device=dev)
        L.call("mmdx_bn_apply", L.dtype_code(dt), x.data_ptr(), res.data_ptr() if use_res else None,
               rows, C, scale_d.data_ptr(), shift_d.data_ptr(), relu, y.data_ptr(),
               mask.data_ptr() if use_mask else None, L.stream())
        torch.cuda.synchronize()
        _check_tensor(y, ref, dt, "y", what)
        if use_mask:
            _check_mask(mask, y, dt, what)


def test_stat_part_layout_preconditions(dev):
    """Slabs that do not cover the rows exactly are refused: too few (rows missing) and too many
    ((stat_blocks - 1) * stat_rows >= rows: the last slab's weight would be <= 0)."""
    C, rows = 8, 7
    f = torch.zeros(8 * C * 2, device=dev)
    v = [torch.zeros(C, device=dev) for _ in range(4)]
    x = torch.zeros(rows, C, dtype=BF16, device=dev)
    y = torch.empty_like(x)
    ws, ws_n = _ws(rows, C, dev)

    def finalize(nblk, stat_rows):
        L.call("mmdx_bn_finalize", f.data_ptr(), nblk, stat_rows, rows, C, None, None, None, None,
               MOM, EPS, *[t.data_ptr() for t in v], L.stream())

    def fwd(nblk, stat_rows):
        L.call("mmdx_bn_fwd_ex", L.BF16, 1, x.data_ptr(), rows, C, f.data_ptr(), nblk, stat_rows,
               None, None, None, None, MOM, EPS, v[0].data_ptr(), v[1].data_ptr(), None, 0,
               y.data_ptr(), None, ws.data_ptr(), ws_n, L.stream())

    for call in (finalize, fwd):
        for nblk, stat_rows in [(3, 3), (1, 7), (1, 100), (7, 1)]:   # exact covers
            call(nblk, stat_rows)
        for nblk, stat_rows in [(2, 3), (4, 3), (2, 7), (8, 1), (0, 3), (3, 0)]:
            with pytest.raises(RuntimeError, match="statistics layout"):
                call(nblk, stat_rows)
    torch.cuda.synchronize()


# =============================================================================== backward
@functools.lru_cache(maxsize=None)
def _bwd_case(s, dt):
    """_host_case with x moved off the ReLU decision boundary of the recomputing mode, the
    statistics the backward is handed, and the four ReLU decisions.  Host only.

    MODE 3 and mmdx_bn_bwd_pool recompute x * scale + shift > 0 in fp32; so that no check
    depends on that rounding, every element whose fp64 pre-activation (from the fp32 gamma,
    beta, mean and rstd actually passed) has |pre| <= 2^-16 (|x scale| + |shift|) is replaced
    by a value one standard deviation above the mean and the statistics are recomputed."""
    d = _host_case(s, dt)
    b = SimpleNamespace(rows=d.rows, C=d.C, dy=d.dy, gam=d.gam, bet=d.bet, acc=d.acc)
    b.x, b.mean32, b.rstd32, b.var, b.pre = _off_the_boundary(d.x, d.gam, d.bet, dt)
    b.pos_x = b.pre > 0                                     # MODE 3: recomputed from x
    b.mask = bn_ref.pack_mask(d.bits, _vec(dt))             # MODE 1: given mask bytes
    b.pos_mask = bn_ref.unpack_mask(b.mask, _vec(dt))
    assert torch.equal(b.pos_mask, d.bits)
    b.y = _round(torch.clamp(b.pre + d.res, min=0.0), dt)   # MODE 2: the unit's stored output
    b.pos_y = b.y > 0
    assert 0.2 < b.pos_y.double().mean() < 0.8 and 0.2 < b.pos_x.double().mean() < 0.8
    return b


def _off_the_boundary(x, gam, bet, dt):
    x = x.clone()
    replaced = torch.zeros_like(x, dtype=torch.bool)
    for _ in range(4):
        f = bn_ref.bn_forward(x, eps=EPS)
        mean32, rstd32 = f.mean.float(), f.rstd.float()
        scale = gam.double() * rstd32.double()
        shift = bet.double() - mean32.double() * scale
        pre = x * scale + shift
        near = pre.abs() <= 2.0 ** -16 * ((x * scale).abs() + shift.abs())
        if not near.any():
            break
        x[near] = _round(f.mean + torch.sqrt(f.var), dt).expand_as(x)[near]
        replaced |= near
    assert not near.any()
    assert replaced.double().mean() < 1e-3
    return x, mean32, rstd32, f.var, pre


def _bwd_ref(s, dt, mode, train):
    """The reference backward of one case for one ReLU decision source (0 none, 1 the mask
    bytes, 2 y, 3 recomputed from x), train or eval."""
    b = _bwd_case(s, dt)
    pos = (None, b.pos_mask, b.pos_y, b.pos_x)[mode]
    # (eval: the statistics handed over are constants; the batch ones serve for both)
    return bn_ref.bn_backward(b.x, b.dy, b.gam, pos, bool(train), EPS, b.mean32.double(),
                              1.0 / b.rstd32.double() ** 2 - EPS, b.mean32, b.rstd32)


def _check_bwd(ref, dt, dx, dres, dg, db, beta_acc, acc, what):
    _check_tensor(dx, ref.dx, dt, "dx", what)
    if dres is not None:
        _check_tensor(dres, ref.d_residual, dt, "d_residual", what)
    pre = [a.double() * beta_acc for a in acc]
    _check_sum(dg, ref.dgamma + pre[0], ref.sum_abs_gx, pre[0], "dgamma", what)
    _check_sum(db, ref.dbeta + pre[1], ref.sum_abs_g, pre[1], "dbeta", what)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bn_bwd_ex_and_masked_dy(dev, case):
    """mmdx_bn_bwd_ex in its four ReLU modes (0 none, 1 mask bytes, 2 the device y, 3 y == NULL:
    recomputed from x), train / eval, beta_acc 0 / 1, and mmdx_bn_bwd_masked_dy — the two halves
    of mmdx_bn_bwd_pair, which tests/test_bn_bwd_pair_gpu.py holds bit-equal to them."""
    s, dt = case
    b = _bwd_case(s, dt)    # (its host-side assertions run before any GPU call)
    rows, C, dc = b.rows, b.C, L.dtype_code(dt)
    x, dy, y = b.x.to(dev, dt), b.dy.to(dev, dt), b.y.to(dev, dt)
    gam, bet, mask = b.gam.to(dev), b.bet.to(dev), b.mask.to(dev)
    mean, rstd = b.mean32.to(dev), b.rstd32.to(dev)
    ws, ws_n = _ws(rows, C, dev)
    for mode in (0, 1, 2, 3):
        for train in (1, 0):
            ref = _bwd_ref(s, dt, mode, train)
            for beta_acc in (0.0, 1.0):
                what = f"mode={mode} train={train} beta_acc={beta_acc}"
                dx = torch.empty_like(x)
                dres = torch.empty_like(x) if mode in (1, 2) else None
                dg, db = b.acc[0].to(dev), b.acc[1].to(dev)
                L.call("mmdx_bn_bwd_ex", dc, train, x.data_ptr(),
                       y.data_ptr() if mode == 2 else None, dy.data_ptr(), rows, C,
                       gam.data_ptr(), bet.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                       int(mode != 0), None, 0, dx.data_ptr(), L.ptr(dres), dg.data_ptr(),
                       db.data_ptr(), beta_acc, mask.data_ptr() if mode == 1 else None,
                       ws.data_ptr(), ws_n, L.stream())
                torch.cuda.synchronize()
                _check_bwd(ref, dt, dx, dres, dg, db, beta_acc, b.acc, what)
                if mode != 1:
                    continue
                what = f"masked_dy train={train} beta_acc={beta_acc}"
                dx = torch.empty_like(x)
                dg, db = b.acc[0].to(dev), b.acc[1].to(dev)
                L.call("mmdx_bn_bwd_masked_dy", dc, train, x.data_ptr(), dy.data_ptr(),
                       mask.data_ptr(), rows, C, gam.data_ptr(), bet.data_ptr(), mean.data_ptr(),
                       rstd.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), beta_acc,
                       ws.data_ptr(), ws_n, L.stream())
                torch.cuda.synchronize()
                _check_bwd(ref, dt, dx, None, dg, db, beta_acc, b.acc, what)


@pytest.mark.parametrize("dt", [BF16, F32])
def test_bn_bwd_null_affine(dev, dt):
    """gamma == NULL and bn_beta == NULL are 1 and 0, in the mode that reads them most (3)."""
    d = _host_case(1, dt)
    rows, C = d.rows, d.C
    one, zero = torch.ones(C), torch.zeros(C)
    xh, mean32, rstd32, _, pre = _off_the_boundary(d.x, one, zero, dt)
    ref = bn_ref.bn_backward(xh, d.dy, None, pre > 0, True, EPS, save_mean=mean32,
                             save_rstd=rstd32)
    x, dy = xh.to(dev, dt), d.dy.to(dev, dt)
    mean, rstd = mean32.to(dev), rstd32.to(dev)
    dx = torch.empty_like(x)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    ws, ws_n = _ws(rows, C, dev)
    L.call("mmdx_bn_bwd_ex", L.dtype_code(dt), 1, x.data_ptr(), None, dy.data_ptr(), rows, C,
           None, None, mean.data_ptr(), rstd.data_ptr(), 1, None, 0,
           dx.data_ptr(), None, dg.data_ptr(), db.data_ptr(), 0.0, None, ws.data_ptr(), ws_n,
           L.stream())
    torch.cuda.synchronize()
    _check_bwd(ref, dt, dx, None, dg, db, 0.0, [zero, zero], "null affine")


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("nblk", [1, bn_ref.FIN_WIDE + 1, bn_ref.FIN_REGS + 1])
def test_bn_bwd_from_partials(dev, dt, nblk):
    """mmdx_bn_bwd with stat_part: the reference's (sum g, sum g*xhat) split into nblk fp32
    pieces per channel replaces the reduce pass (one-wave finalize | the 256-thread one from
    registers | from memory); ReLU from y (mode 2) and recomputed from x (mode 3)."""
    rows, C = 64, 64
    g = torch.Generator().manual_seed(3000)
    gam = torch.rand(C, generator=g) + 0.5
    gam[::7] *= -1.0
    bet = torch.randn(C, generator=g) * 0.3
    x0 = _round(torch.randn(rows, C, generator=g) * 2 + torch.linspace(-1.5, 1.5, C), dt)
    xh, mean32, rstd32, _, pre = _off_the_boundary(x0, gam, bet, dt)
    dyh = _round(torch.randn(rows, C, generator=g), dt)
    yh = _round(torch.clamp(pre + _round(torch.randn(rows, C, generator=g), dt), min=0.0), dt)
    acc = [torch.randn(C, generator=g) for _ in range(2)]
    x, dy, y = xh.to(dev, dt), dyh.to(dev, dt), yh.to(dev, dt)
    gamd, betd, mean, rstd = gam.to(dev), bet.to(dev), mean32.to(dev), rstd32.to(dev)
    ws, ws_n = _ws(rows, C, dev)
    for mode, pos in ((2, yh > 0), (3, pre > 0)):
        ref = bn_ref.bn_backward(xh, dyh, gam, pos, True, EPS, save_mean=mean32,
                                 save_rstd=rstd32)
        part = bn_ref.split_totals(ref.dbeta, ref.dgamma, nblk, g).to(dev)
        for beta_acc in (0.0, 1.0):
            what = f"stat_part nblk={nblk} mode={mode} beta_acc={beta_acc}"
            dx = torch.empty_like(x)
            dres = torch.empty_like(x) if mode == 2 else None
            dg, db = acc[0].to(dev), acc[1].to(dev)
            L.call("mmdx_bn_bwd", L.dtype_code(dt), 1, x.data_ptr(),
                   y.data_ptr() if mode == 2 else None, dy.data_ptr(), rows, C,
                   gamd.data_ptr(), betd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), 1,
                   part.data_ptr(), nblk, dx.data_ptr(),
                   L.ptr(dres), dg.data_ptr(), db.data_ptr(), beta_acc, ws.data_ptr(), ws_n,
                   L.stream())
            torch.cuda.synchronize()
            _check_bwd(ref, dt, dx, dres, dg, db, beta_acc, acc, what)


@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("cfg", [(2, 7, 9, 16, 1), (2, 8, 6, 16, 0)])
def test_bn_bwd_pool(dev, dt, cfg):
    """mmdx_bn_bwd_pool against its documented contract: the BN + ReLU backward of the pooled
    gradient scattered through the argmax bytes (the library's own forward wrote them) and
    rounded to the compute dtype.  Odd sizes with padding; an uncovered last row without."""
    N, H, W, C, pad = cfg
    rows = N * H * W
    P, Q = (H + 2 * pad - 3) // 2 + 1, (W + 2 * pad - 3) // 2 + 1
    g = torch.Generator().manual_seed(4000 + H)
    gam = torch.rand(C, generator=g) + 0.5
    gam[::5] *= -1.0
    bet = torch.randn(C, generator=g) * 0.3
    x0 = _round(torch.randn(rows, C, generator=g) * 2 + torch.linspace(-1, 1, C), dt)
    xh, mean32, rstd32, _, pre = _off_the_boundary(x0, gam, bet, dt)
    dyp = _round(torch.randn(N, P, Q, C, generator=g), dt)
    acc = [torch.randn(C, generator=g) for _ in range(2)]

    dc = L.dtype_code(dt)
    x, dypd = xh.to(dev, dt), dyp.to(dev, dt)
    gamd, betd, mean, rstd = gam.to(dev), bet.to(dev), mean32.to(dev), rstd32.to(dev)
    pooled = torch.empty(N, P, Q, C, dtype=dt, device=dev)
    am = torch.empty(N, P, Q, C, dtype=torch.uint8, device=dev)
    L.call("mmdx_maxpool_bn_fwd", dc, x.data_ptr(), N, H, W, C, 3, 2, pad, gamd.data_ptr(),
           betd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), 1, pooled.data_ptr(),
           am.data_ptr(), P, Q, L.stream())
    torch.cuda.synchronize()
    gin = bn_ref.pool_scatter(dyp, am.cpu(), H, W, pad, dt).view(rows, C)
    ws, ws_n = _ws(rows, C, dev)
    for train in (1, 0):
        ref = bn_ref.bn_backward(xh, gin, gam, pre > 0, bool(train), EPS, mean32.double(),
                                 1.0 / rstd32.double() ** 2 - EPS, mean32, rstd32)
        for beta_acc in (0.0, 1.0):
            dx = torch.empty_like(x)
            dg, db = acc[0].to(dev), acc[1].to(dev)
            L.call("mmdx_bn_bwd_pool", dc, train, x.data_ptr(), am.data_ptr(),
                   dypd.data_ptr(), N, H, W, C, 3, 2, pad, P, Q, gamd.data_ptr(),
                   betd.data_ptr(), mean.data_ptr(), rstd.data_ptr(), 1, dx.data_ptr(),
                   dg.data_ptr(), db.data_ptr(), beta_acc, ws.data_ptr(), ws_n, L.stream())
            torch.cuda.synchronize()
            _check_bwd(ref, dt, dx, None, dg, db, beta_acc, acc,
                       f"bwd_pool {cfg} train={train} beta_acc={beta_acc}")


# ============================================================== several rows per reduce thread
@pytest.mark.parametrize("dt", [BF16, F32])
def test_bn_threads_with_several_rows(dev, dt):
    """The accumulation loops of bn_stats_kernel and bn_bwd_reduce_kernel (a thread's second and
    later rows, the pivot's add-back, the divisor cnt > 1, a ragged last slab with row threads
    that have fewer rows or none): forward (train: plain, and residual + ReLU + mask) and
    backward (train, every ReLU mode, and mmdx_bn_bwd_masked_dy) at SHAPES[SEVERAL]."""
    d = _host_case(SEVERAL, dt)
    rows, C, dc = d.rows, d.C, L.dtype_code(dt)
    rt, rpb, nblk = bn_ref._layout(rows, C, _vec(dt))
    assert rpb // rt >= 2 and 0 < rows - (nblk - 1) * rpb < rpb    # several rows; ragged tail
    b = _bwd_case(SEVERAL, dt)    # (its host-side assertions run before any GPU call)
    ws, ws_n = _ws(rows, C, dev)
    gam, bet = d.gam.to(dev), d.bet.to(dev)

    x, res = d.x.to(dev, dt), d.res.to(dev, dt)
    for use_res, relu, use_mask in [(0, 0, 0), (1, 1, 1)]:
        what = f"several rows: fwd res={use_res} relu={relu} mask={use_mask}"
        ref = bn_ref.bn_forward(d.x, d.gam, d.bet, d.rm, d.rv, MOM, EPS,
                                d.res if use_res else None, bool(relu), True)
        rm, rv = d.rm.to(dev), d.rv.to(dev)
        mean, rstd, y, mask = _fwd_ex(dev, dt, 1, x, rows, C, gam, bet, rm, rv,
                                      res if use_res else None, relu, True, use_mask, ws, ws_n)
        _check_tensor(y, ref.y, dt, "y", what)
        _check_vector(mean, ref.mean, "mean", what)
        _check_vector(rstd, ref.rstd, "rstd", what)
        _check_vector(rm, ref.running_mean, "running_mean", what)
        _check_vector(rv, ref.running_var, "running_var", what)
        if use_mask:
            _check_mask(mask, y, dt, what)
    del res, y, mask

    x, dy, y = b.x.to(dev, dt), b.dy.to(dev, dt), b.y.to(dev, dt)
    mask = b.mask.to(dev)
    mean, rstd = b.mean32.to(dev), b.rstd32.to(dev)
    for mode in (0, 1, 2, 3):
        ref = _bwd_ref(SEVERAL, dt, mode, 1)
        what = f"several rows: bwd mode={mode}"
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if mode in (1, 2) else None
        dg, db = b.acc[0].to(dev), b.acc[1].to(dev)
        L.call("mmdx_bn_bwd_ex", dc, 1, x.data_ptr(), y.data_ptr() if mode == 2 else None,
               dy.data_ptr(), rows, C, gam.data_ptr(), bet.data_ptr(), mean.data_ptr(),
               rstd.data_ptr(), int(mode != 0), None, 0, dx.data_ptr(), L.ptr(dres),
               dg.data_ptr(), db.data_ptr(), 1.0, mask.data_ptr() if mode == 1 else None,
               ws.data_ptr(), ws_n, L.stream())
        torch.cuda.synchronize()
        _check_bwd(ref, dt, dx, dres, dg, db, 1.0, b.acc, what)
        if mode != 1:
            continue
        dx = torch.empty_like(x)
        dg, db = b.acc[0].to(dev), b.acc[1].to(dev)
        L.call("mmdx_bn_bwd_masked_dy", dc, 1, x.data_ptr(), dy.data_ptr(), mask.data_ptr(),
               rows, C, gam.data_ptr(), bet.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
               dx.data_ptr(), dg.data_ptr(), db.data_ptr(), 1.0, ws.data_ptr(), ws_n, L.stream())
        torch.cuda.synchronize()
        _check_bwd(ref, dt, dx, None, dg, db, 1.0, b.acc, "several rows: masked_dy")


# =============================================================================== numerics
@pytest.mark.parametrize("C,per_thread", [(64, 1), (2048, 4)])
def test_bn_statistics_with_a_large_mean(dev, C, per_thread):
    """fp32, 4096 rows, channel c drawn as N(r_c, 1) with r_c cycling through 0, 4, 16, 64:
    a one-pass sum x^2 - (sum x)^2 / n in fp32 loses M2 bits as |mean| / std grows.  Up to
    r = 16 save_mean and save_rstd must meet the per-channel-vector tolerance; at r = 64 only
    finiteness is asserted and the relative error of rstd is printed.

    C = 64 is the issue's case: its layout gives every reduce thread ONE row, so it measures
    only what a single-row thread hands on as M2 (0 now; fl(x^2) - x*x under fma contraction
    before the pivot).  C = 2048 (8 channel groups: 16-row slabs, 4 row threads) gives every
    thread 4 rows, so bn_stats_kernel's accumulation over d = x - first row is what it measures.

    Measured on an MI355X, largest relative rstd error at r = 4 / 16 / 64:
      C = 64,   sums of x (before the pivot):  2.0e-7 / 1.5e-6 / 2.5e-5
      C = 64,   sums of x - first row (now):   9.1e-8 / 9.7e-8 / 3.2e-7
      C = 2048, sums of x (before the pivot):  1.3e-7 / 1.1e-6 / 1.8e-5
      C = 2048, sums of x - first row (now):   1.2e-7 / 1.1e-7 / 2.1e-7"""
    rows = 4096
    rt, rpb, _ = bn_ref._layout(rows, C, 4)
    assert rpb // rt == per_thread and rows % rpb == 0
    g = torch.Generator().manual_seed(5000)
    r = torch.tensor([0.0, 4.0, 16.0, 64.0]).repeat(C // 4)
    xh = (torch.randn(rows, C, generator=g) + r).double()     # (fp32 values)
    ref = bn_ref.bn_forward(xh, eps=EPS)
    ws, ws_n = _ws(rows, C, dev)
    mean, rstd, _, _ = _fwd_ex(dev, F32, 1, xh.to(dev, F32), rows, C, None, None, None, None,
                               None, 0, False, False, ws, ws_n)
    mean, rstd = mean.double().cpu(), rstd.double().cpu()
    assert torch.isfinite(mean).all() and torch.isfinite(rstd).all()
    for rc in (0.0, 4.0, 16.0, 64.0):
        sel = r == rc
        rel = ((rstd[sel] - ref.rstd[sel]).abs() / ref.rstd[sel]).max().item()
        print(f"bnref numerics C={C} r={rc:g}: max relative rstd error {rel:.3e}, "
              f"max mean error {(mean[sel] - ref.mean[sel]).abs().max().item():.3e}")
    ok = r <= 16.0
    _check_vector(mean[ok], ref.mean[ok], "mean", f"numerics C={C} r <= 16")
    _check_vector(rstd[ok], ref.rstd[ok], "rstd", f"numerics C={C} r <= 16")
