"""CPU: tests/bn_ref.py (the fp64 reference the BatchNorm kernels are checked against) against
torch.nn.BatchNorm2d and torch.nn.functional.max_pool2d in double, and its layout helpers
against the definitions they mirror."""
import pytest
import torch
import torch.nn.functional as tF

import bn_ref

EPS = 1e-5
MOM = 0.1


def _case(rows=45, C=12, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = dict(dtype=torch.float64, generator=g)
    x = torch.randn(rows, C, **d) * 2 + 0.5
    res = torch.randn(rows, C, **d)
    dy = torch.randn(rows, C, **d)
    gam = torch.rand(C, **d) + 0.5
    gam[::5] *= -1.0
    bet = torch.randn(C, **d) * 0.3
    rm = torch.randn(C, **d) * 0.2
    rv = torch.rand(C, **d) + 0.5
    return x, res, dy, gam, bet, rm, rv


def _torch_bn(x, res, gam, bet, rm, rv, train, use_res, relu):
    """nn.BatchNorm2d in double on [rows, C] viewed as [rows, C, 1, 1]; returns the module, the
    leaf tensors and the output."""
    C = x.shape[1]
    bn = torch.nn.BatchNorm2d(C, eps=EPS, momentum=MOM).double()
    with torch.no_grad():
        bn.weight.copy_(gam)
        bn.bias.copy_(bet)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    bn.train(train)
    xr = x.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True)
    out = bn(xr[:, :, None, None])[:, :, 0, 0]
    if use_res:
        out = out + rr
    pre = out
    if relu:
        out = torch.relu(out)
    return bn, xr, rr, pre, out


def _same(a, b, what):
    err = (a - b).abs().max().item()
    assert err <= 1e-12 * max(1.0, b.abs().max().item()), f"{what}: {err}"


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("use_res,relu", [(False, False), (False, True), (True, False),
                                          (True, True)])
def test_forward_and_backward_match_torch_batchnorm(train, use_res, relu):
    x, res, dy, gam, bet, rm, rv = _case()
    bn, xr, rr, pre, out = _torch_bn(x, res, gam, bet, rm, rv, train, use_res, relu)
    out.backward(dy)
    f = bn_ref.bn_forward(x, gam, bet, rm, rv, MOM, EPS, res if use_res else None, relu, train)
    _same(f.y, out.detach(), "y")
    _same(f.pre, pre.detach(), "pre")
    if train:
        _same(f.mean, x.mean(0), "mean")
        _same(f.var, x.var(0, unbiased=False), "var")
        _same(f.running_mean, bn.running_mean, "running_mean")
        _same(f.running_var, bn.running_var, "running_var")
    else:
        _same(f.running_mean, rm, "running_mean (eval: unchanged)")
        _same(f.running_var, rv, "running_var (eval: unchanged)")
    _same(f.rstd, 1 / torch.sqrt(f.var + EPS), "rstd")
    _same(x * f.scale + f.shift, (x - f.mean) * f.rstd * gam + bet, "scale / shift")

    pos = (pre.detach() > 0) if relu else None
    b = bn_ref.bn_backward(x, dy, gam, pos, train, EPS, rm, rv)
    _same(b.dx, xr.grad, "dx")
    _same(b.dgamma, bn.weight.grad, "dgamma")
    _same(b.dbeta, bn.bias.grad, "dbeta")
    if use_res:
        _same(b.d_residual, rr.grad, "d_residual")
    g = dy if pos is None else dy * pos
    xhat = (x - f.mean) * f.rstd
    _same(b.sum_abs_g, g.abs().sum(0), "sum |g|")
    _same(b.sum_abs_gx, (g * xhat).abs().sum(0), "sum |g xhat|")


def test_backward_at_the_rounded_statistics_a_kernel_is_handed():
    """save_mean / save_rstd replace the values of the batch statistics, not the derivative:
    the exact ones change nothing; rounded ones give the closed form evaluated at them."""
    x, _, dy, gam, _, _, _ = _case(rows=9)
    pos = torch.rand(x.shape, generator=torch.Generator().manual_seed(1)) > 0.3
    f = bn_ref.bn_forward(x, eps=EPS)
    a = bn_ref.bn_backward(x, dy, gam, pos, True, EPS)
    b = bn_ref.bn_backward(x, dy, gam, pos, True, EPS, save_mean=f.mean, save_rstd=f.rstd)
    for k in ("dx", "d_residual", "dgamma", "dbeta", "sum_abs_g", "sum_abs_gx"):
        _same(getattr(b, k), getattr(a, k), k)
    m, r = f.mean.bfloat16().double(), f.rstd.bfloat16().double()   # coarse: a visible change
    c = bn_ref.bn_backward(x, dy, gam, pos, True, EPS, save_mean=m, save_rstd=r)
    g, xhat = dy * pos, (x - m) * r
    _same(c.dgamma, (g * xhat).sum(0), "dgamma")
    _same(c.sum_abs_gx, (g * xhat).abs().sum(0), "sum |g xhat|")
    _same(c.dx, gam * r * (g - g.mean(0)) + _dx_k_term(x, g, gam, f, m, r), "dx")


def _dx_k_term(x, g, gam, f, m, r):
    """-(gamma / n) * sum_r(g * (x - m)) * (r / rstd) * rstd^3 * (x - mean): the derivative of
    rstd flows through the batch statistics, scaled by the substituted value's ratio."""
    s = (g * (x - m)).sum(0)
    return -gam * s * (r / f.rstd) * f.rstd ** 3 * (x - f.mean) / x.shape[0]


def test_forward_defaults_one_row_and_statistics_only():
    """gamma / beta None are 1 / 0; a single row has variance 0 and keeps it as the unbiased
    one; without running statistics none are returned."""
    x = torch.tensor([[1.0, -2.0, 3.0, 0.5]], dtype=torch.float64)
    f = bn_ref.bn_forward(x, running_mean=torch.zeros(4), running_var=torch.ones(4))
    _same(f.var, torch.zeros(4, dtype=torch.float64), "var")
    _same(f.running_var, torch.full((4,), 0.9, dtype=torch.float64), "running_var")
    _same(f.y, torch.zeros(1, 4, dtype=torch.float64), "y")
    _same(f.scale, f.rstd, "scale")
    assert bn_ref.bn_forward(x).running_mean is None


@pytest.mark.parametrize("rows,stat_rows", [(1, 3), (3, 3), (4, 3), (100, 7), (64, 128)])
def test_slabs_remerge_to_the_direct_statistics(rows, stat_rows):
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, 6, generator=g) * 2 + 1).double()   # fp32 values: slabs round little
    part = bn_ref.slab_stats(x, stat_rows)
    nblk = (rows + stat_rows - 1) // stat_rows
    assert part.shape == (6, nblk, 2) and part.dtype == torch.float32 and part.is_contiguous()
    last = x[(nblk - 1) * stat_rows:]
    assert torch.allclose(part[:, -1, 0].double(), last.mean(0), rtol=1e-6, atol=1e-7)
    mean, m2 = bn_ref.merge_slabs(part, stat_rows, rows)
    f = bn_ref.bn_forward(x)
    assert torch.allclose(mean, f.mean, rtol=1e-6, atol=1e-6)
    assert torch.allclose(m2, f.var * rows, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("nblk", [1, 2, 513])
def test_split_totals_add_up(nblk):
    g = torch.Generator().manual_seed(nblk)
    sg = torch.randn(5, generator=g, dtype=torch.float64) * 10
    sgx = torch.randn(5, generator=g, dtype=torch.float64) * 10
    part = bn_ref.split_totals(sg, sgx, nblk, g)
    assert part.shape == (5, nblk, 2) and part.dtype == torch.float32
    tot = part.double().sum(1)
    assert torch.allclose(tot[:, 0], sg, rtol=1e-6) and torch.allclose(tot[:, 1], sgx, rtol=1e-6)
    # shares of one sign: the sum of magnitudes is the total's magnitude
    assert torch.allclose(part.double().abs().sum(1), tot.abs(), rtol=1e-12)


@pytest.mark.parametrize("vec", [4, 8])
def test_mask_pack_unpack(vec):
    g = torch.Generator().manual_seed(vec)
    pos = torch.rand(7, 3 * vec, generator=g) > 0.5
    mask = bn_ref.pack_mask(pos, vec)
    assert mask.shape == (7, 3) and mask.dtype == torch.uint8
    assert torch.equal(bn_ref.unpack_mask(mask, vec), pos)
    one = torch.zeros(1, vec, dtype=torch.bool)
    one[0, 2] = True            # bit e = element e
    assert bn_ref.pack_mask(one, vec).item() == 4
    assert bn_ref.pack_mask(torch.ones(1, vec, dtype=torch.bool), vec).item() == (1 << vec) - 1


@pytest.mark.parametrize("N,H,W,C,pad", [(2, 7, 9, 3, 1), (2, 8, 6, 3, 0), (1, 3, 3, 1, 0)])
def test_pool_scatter_matches_max_pool2d_autograd(N, H, W, C, pad):
    g = torch.Generator().manual_seed(H * W)
    n = N * C * H * W
    x = (torch.randperm(n, generator=g).double() - n / 2).view(N, C, H, W)   # no ties
    xr = x.clone().requires_grad_(True)
    y, idx = tF.max_pool2d(xr, 3, 2, pad, return_indices=True)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    P, Q = y.shape[2:]
    # flat h * W + w of the maximum -> tap inside the window whose corner is (2i - pad, 2j - pad)
    h, w = idx // W, idx % W
    i = torch.arange(P).view(1, 1, P, 1)
    j = torch.arange(Q).view(1, 1, 1, Q)
    tap = (h - (2 * i - pad)) * 3 + (w - (2 * j - pad))
    am = tap.permute(0, 2, 3, 1).to(torch.uint8)
    got = bn_ref.pool_scatter(dy.permute(0, 2, 3, 1), am, H, W, pad, torch.float64)
    _same(got, xr.grad.permute(0, 2, 3, 1), "scatter")
    # rounded to the compute dtype after the sum
    got16 = bn_ref.pool_scatter(dy.permute(0, 2, 3, 1), am, H, W, pad, torch.bfloat16)
    assert torch.equal(got16, xr.grad.permute(0, 2, 3, 1).bfloat16().double())


def test_layout_mirror():
    """_rblocks against hand-worked bn_layout cases (BN_NT = 256, target 2048 slabs)."""
    assert bn_ref._rblocks(252, 64, 8) == 8          # ct 8, rt 32: 32-row slabs
    assert bn_ref._rblocks(252, 64, 4) == 16         # ct 16, rt 16
    assert bn_ref._rblocks(37, 48, 4) == 2           # ct 12, rt 21 (252 live threads)
    assert bn_ref._rblocks(21, 4, 4) == 1            # ct 1, rt 256
    assert bn_ref._rblocks(5, 2304, 8) == 2          # 5 channel groups, rt 4
    assert bn_ref._rblocks(128 * 56 * 56, 64, 8) == 1792    # 196 -> 224-row slabs
    # (row threads, rows per slab, slabs): past 2048 * rt / cgroups rows a thread gets several
    assert bn_ref._layout(2101, 2048, 4) == (4, 12, 176)    # 8 groups: target 256 slabs
    assert bn_ref._layout(2101, 2048, 8) == (4, 8, 263)     # 4 groups: target 512 slabs
    assert bn_ref._layout(4096, 2048, 4) == (4, 16, 256) and bn_ref._layout(4096, 64, 4)[:2] == (16, 16)
    assert bn_ref.workspace_size(21, 4) == 1 * 4 * 8 + 5 * 4 * 4
    assert bn_ref.workspace_size(21, 12) == bn_ref._rblocks(21, 12, 4) * 12 * 8 + 5 * 12 * 4
    assert bn_ref.workspace_size(21, 6) == 0 and bn_ref.workspace_size(21, 0) == 0
