"""mmdx_bn_bwd_pair (the two BatchNorm backwards of a downsample block over one pass of their
shared masked gradient) against the two separate calls it replaces, on the same inputs:
mmdx_bn_bwd_ex(relu=1, relu_mask=...) for side a and mmdx_bn_bwd_masked_dy for side b.
dconv_a, dconv_b and both dgamma / dbeta must be equal bit for bit: the paired kernels keep
the separate kernels' grid, row order, merge order and arithmetic."""
import ctypes

import pytest
import torch

import mmdx._lib as L
from bn_ref import _wide_rows  # the mirror of csrc/norm.hip bn_layout lives in tests/bn_ref.py

pytestmark = pytest.mark.gpu


# (rows, C): < 256 channel vectors, several rows per block, ragged tail | 256 vectors (bf16) |
# the apply's j loop runs twice | more than fin_wide() slabs (rows from bn_layout)
CASES = [(98, 64), (37, 2048), (5, 2304), (None, 64)]


def _side(x, gam, bet, mean, rstd, dx, dgm, dbt):
    return L.BnSide(x.data_ptr(), gam.data_ptr(), bet.data_ptr(), mean.data_ptr(),
                    rstd.data_ptr(), dx.data_ptr(), dgm.data_ptr(), dbt.data_ptr())


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_bn_bwd_pair_matches_separate_calls(dev, dt, case):
    rows, C = CASES[case]
    if rows is None:
        rows = _wide_rows(C)
    vec = 4 if dt == torch.float32 else 8
    dc = L.dtype_code(dt)
    g = torch.Generator().manual_seed(100 + case)
    dy = torch.randn(rows, C, generator=g).to(dev, dt)
    xs = [torch.randn(rows, C, generator=g).to(dev, dt) for _ in range(2)]
    gam = [(torch.rand(C, generator=g) + 0.5).to(dev) for _ in range(2)]
    bet = [(torch.randn(C, generator=g) * 0.1).to(dev) for _ in range(2)]
    mean = [(torch.randn(C, generator=g) * 0.1).to(dev) for _ in range(2)]
    rstd = [(torch.rand(C, generator=g) + 0.5).to(dev) for _ in range(2)]
    acc0 = [torch.randn(C, generator=g).to(dev) for _ in range(4)]
    masks = {
        "random": torch.randint(0, 256, (rows, C // vec), generator=g).to(torch.uint8).to(dev),
        "zeros": torch.zeros(rows, C // vec, dtype=torch.uint8, device=dev),
        "ones": torch.full((rows, C // vec), 0xFF, dtype=torch.uint8, device=dev),
    }
    ws_n = L.lib().mmdx_bn_workspace_size(rows, C)
    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
    wp_n = L.lib().mmdx_bn_pair_workspace_size(rows, C)
    wp = torch.empty(wp_n, dtype=torch.uint8, device=dev)
    for density, mask in masks.items():
        for beta_acc in (0.0, 1.0):
            for train in (1, 0):
                tag = f"{density} beta_acc={beta_acc} train={train}"
                ref_dx = [torch.empty_like(dy) for _ in range(2)]
                ref_g = [t.clone() for t in acc0]   # dgamma_a, dbeta_a, dgamma_b, dbeta_b
                L.call("mmdx_bn_bwd_ex", dc, train, xs[0].data_ptr(), None, dy.data_ptr(), rows,
                       C, gam[0].data_ptr(), bet[0].data_ptr(), mean[0].data_ptr(),
                       rstd[0].data_ptr(), 1, None, 0, ref_dx[0].data_ptr(), None,
                       ref_g[0].data_ptr(), ref_g[1].data_ptr(), beta_acc, mask.data_ptr(),
                       ws.data_ptr(), ws_n, L.stream())
                L.call("mmdx_bn_bwd_masked_dy", dc, train, xs[1].data_ptr(), dy.data_ptr(),
                       mask.data_ptr(), rows, C, gam[1].data_ptr(), bet[1].data_ptr(),
                       mean[1].data_ptr(), rstd[1].data_ptr(), ref_dx[1].data_ptr(),
                       ref_g[2].data_ptr(), ref_g[3].data_ptr(), beta_acc, ws.data_ptr(), ws_n,
                       L.stream())
                got_dx = [torch.empty_like(dy) for _ in range(2)]
                got_g = [t.clone() for t in acc0]
                a = _side(xs[0], gam[0], bet[0], mean[0], rstd[0], got_dx[0], got_g[0], got_g[1])
                b = _side(xs[1], gam[1], bet[1], mean[1], rstd[1], got_dx[1], got_g[2], got_g[3])
                L.call("mmdx_bn_bwd_pair", dc, train, dy.data_ptr(), mask.data_ptr(), rows, C,
                       ctypes.byref(a), ctypes.byref(b), beta_acc, wp.data_ptr(), wp_n,
                       L.stream())
                torch.cuda.synchronize()
                for name, u, v in zip(("dconv_a", "dconv_b"), got_dx, ref_dx):
                    assert torch.equal(u, v), f"{name} ({tag})"
                for name, u, v in zip(("dgamma_a", "dbeta_a", "dgamma_b", "dbeta_b"), got_g,
                                      ref_g):
                    assert torch.equal(u, v), f"{name} ({tag})"


def test_bn_bwd_pair_refuses_fp16_and_a_short_workspace(dev):
    rows, C = 16, 64
    t = torch.zeros(rows, C, dtype=torch.float16, device=dev)
    f = torch.ones(C, device=dev)
    m = torch.zeros(rows, C // 8, dtype=torch.uint8, device=dev)
    d1, d2 = torch.empty_like(t), torch.empty_like(t)
    a = _side(t, f, f, f, f, d1, f.clone(), f.clone())
    b = _side(t, f, f, f, f, d2, f.clone(), f.clone())
    n = L.lib().mmdx_bn_pair_workspace_size(rows, C)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="fp16"):
        L.call("mmdx_bn_bwd_pair", L.F16, 1, t.data_ptr(), m.data_ptr(), rows, C,
               ctypes.byref(a), ctypes.byref(b), 0.0, ws.data_ptr(), n, L.stream())
    with pytest.raises(RuntimeError, match="workspace"):
        L.call("mmdx_bn_bwd_pair", L.BF16, 1, t.data_ptr(), m.data_ptr(), rows, C,
               ctypes.byref(a), ctypes.byref(b), 0.0, ws.data_ptr(), 64, L.stream())
