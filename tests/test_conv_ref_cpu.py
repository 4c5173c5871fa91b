"""CPU: tests/conv_ref.py (the fp64 reference the conv kernels are checked against) against a
seven-loop convolution written from the definition and torch's fp32 conv2d autograd; its layout
helpers against the definitions; the dispatcher mirror expected_path() against an explicit list
of the paths the case table must reach and against the library's own host-side planning calls;
and the sensitivity of the two comparisons to one missing term."""
import os

import pytest
import torch
import torch.nn.functional as tF

import conv_ref as R
from conv_ref import BF16, F32

ALL = list(R.CASES_BF16) + list(R.CASES_F32)


# ------------------------------------------------------------------- the reference itself
def _seven_loops(x, w, dy, cfg):
    """y, dx, dw straight from y[n,k,p,q] = sum_{c,r,s} x[n,c,p sh - ph + r,q sw - pw + s]
    w[k,c,r,s] and its two derivatives of sum(dy * y)."""
    N, C, H, W, K, Rr, S, sh, sw, ph, pw = cfg
    P, Q = R.out_size(cfg)
    y = torch.zeros(N, K, P, Q, dtype=torch.float64)
    dx = torch.zeros(N, C, H, W, dtype=torch.float64)
    dw = torch.zeros(K, C, Rr, S, dtype=torch.float64)
    for n in range(N):
        for k in range(K):
            for p in range(P):
                for q in range(Q):
                    for c in range(C):
                        for r in range(Rr):
                            for s in range(S):
                                ih, iw = p * sh - ph + r, q * sw - pw + s
                                if not (0 <= ih < H and 0 <= iw < W):
                                    continue
                                y[n, k, p, q] += x[n, c, ih, iw] * w[k, c, r, s]
                                dx[n, c, ih, iw] += dy[n, k, p, q] * w[k, c, r, s]
                                dw[k, c, r, s] += dy[n, k, p, q] * x[n, c, ih, iw]
    return y, dx, dw


@pytest.mark.parametrize("cfg", [(1, 2, 4, 4, 3, 3, 3, 1, 1, 1, 1),
                                 (2, 2, 6, 5, 3, 3, 2, 2, 1, 0, 1)])   # the second: asymmetric
def test_reference_matches_the_definition(cfg):
    """Also with |operands|: the ref_abs_* sums.  The asymmetric descriptor leaves an input row
    no tap reaches ((6 - 3) % 2 = 1), which reached() must name."""
    N, C, H, W, K, Rr, S = cfg[:7]
    P, Q = R.out_size(cfg)
    g = torch.Generator().manual_seed(sum(cfg))
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(K, C, Rr, S, generator=g, dtype=torch.float64)
    dy = torch.randn(N, K, P, Q, generator=g, dtype=torch.float64)
    y, dx, dw = _seven_loops(x, w, dy, cfg)
    for got, want in ((R.ref_fwd(x, w, cfg), y), (R.ref_dgrad(dy, w, cfg), dx),
                      (R.ref_wgrad(x, dy, cfg), dw)):
        assert got.shape == want.shape and (got - want).abs().max() <= 1e-12 * want.abs().max()
    ya, dxa, dwa = _seven_loops(x.abs(), w.abs(), dy.abs(), cfg)
    for got, want in ((R.ref_abs_fwd(x, w, cfg), ya), (R.ref_abs_dgrad(dy, w, cfg), dxa),
                      (R.ref_abs_wgrad(x, dy, cfg), dwa)):
        assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    assert torch.equal(R.reached(cfg), dxa[0, 0] > 0)
    if cfg[7] == 2:
        assert not R.reached(cfg)[-1].any() and R.reached(cfg)[:-1].all()


@pytest.mark.parametrize("cid", ALL)
def test_reference_matches_torch_autograd(cid):
    """Every case of the table, integer operands: torch's fp32 conv2d and its autograd are then
    exact as well, so the fp64 reference must equal them element for element."""
    cfg, cm, dt = R.case(cid)
    x, w, dy, _ = R.operands(cid, "int")
    xr, wr = x.float().requires_grad_(True), w.float().requires_grad_(True)
    y = tF.conv2d(xr, wr, stride=cfg[7:9], padding=cfg[9:11])
    assert y.shape[2:] == R.out_size(cfg)
    y.backward(dy.float())
    assert torch.equal(R.ref_fwd(x, w, cfg), y.detach().double())
    assert torch.equal(R.ref_dgrad(dy, w, cfg), xr.grad.double())
    assert torch.equal(R.ref_wgrad(x, dy, cfg), wr.grad.double())


def test_exact_preconditions_hold_for_the_table_and_reject_violations():
    """The integer family of the small cases (the GPU test asserts every case's before its
    launches), and the three ways a precondition can break."""
    for cid in (2, 10, 22, "f2"):
        cfg, cm, dt = R.case(cid)
        x, w, dy, _ = R.operands(cid, "int")
        assert set(x.unique().tolist()) <= {-1.0, 0.0, 1.0} and 0.4 < (x == 0).double().mean() < 0.6
        R.check_exact_preconditions(R.ref_fwd(x, w, cfg), cm * cfg[5] * cfg[6], dt, "y")
    ok = torch.tensor([3.0, -256.0])
    R.check_exact_preconditions(ok, 10, BF16, "ok")
    with pytest.raises(AssertionError, match="not integer"):
        R.check_exact_preconditions(torch.tensor([0.5]), 10, F32, "half")
    with pytest.raises(AssertionError, match="max"):
        R.check_exact_preconditions(torch.tensor([257.0]), 10, BF16, "257")
    R.check_exact_preconditions(torch.tensor([257.0]), 10, F32, "257 in fp32")
    with pytest.raises(AssertionError, match="terms"):
        R.check_exact_preconditions(ok, 1 << 24, F32, "many terms")


# ---------------------------------------------------------------------------------- layouts
def test_layout_helpers():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64)
    assert R.pad_channels(3, BF16) == 8 and R.pad_channels(3, F32) == 4 and R.pad_channels(8, BF16) == 8
    xn = R.to_nhwc(x, 8, BF16)
    assert xn.shape == (2, 4, 5, 8) and xn.dtype == BF16 and (xn[..., 3:] == 0).all()
    assert xn[1, 2, 3, 1] == x[1, 1, 2, 3].to(BF16)
    assert torch.equal(R.from_nhwc(xn)[:, :3], x.to(BF16).double())
    w = torch.randn(6, 3, 2, 3, generator=g, dtype=torch.float64)     # [K, c_master, R, S]
    wk, wc = R.pack_krsc(w, 4, F32), R.pack_crsk(w, 4, F32)
    assert wk.shape == (6, 2, 3, 4) and wc.shape == (4, 2, 3, 6)
    assert wk[5, 1, 2, 0] == w[5, 0, 1, 2].float() and wc[2, 1, 0, 4] == w[4, 2, 1, 0].float()
    assert (wk[..., 3] == 0).all() and (wc[3] == 0).all()
    # slabs of the forward output: rows are the pixels (n, p, q); the last slab is ragged
    y = torch.randn(2, 5, 3, 3, generator=g).double()
    part = R.slab_stats(y, 4)                                           # 18 rows: 4 x 4 + 2
    assert part.shape == (5, 5, 2) and part.dtype == torch.float32
    rows = y.permute(0, 2, 3, 1).reshape(18, 5)
    assert torch.allclose(part[:, 1, 0].double(), rows[4:8].mean(0), rtol=1e-6, atol=1e-7)
    assert torch.allclose(part[:, 4, 0].double(), rows[16:].mean(0), rtol=1e-6, atol=1e-7)
    assert torch.allclose(part[:, 4, 1].double(), ((rows[16:] - rows[16:].mean(0)) ** 2).sum(0),
                          rtol=1e-6, atol=1e-7)
    assert R.slab_stats(y[:1, :, :1], 128).shape == (5, 1, 2)          # fewer rows than a slab


# --------------------------------------------------------------------- the dispatcher mirror
# Every path of conv.hip's dispatcher the case table must keep reaching (expected_path's names).
FWD_PATHS = {
    "point/dma/128x64/ns2", "point/dma/128x128-8w", "fast/dma/128x64/ns2", "fast/dma/128x64/ns3",
    "fast/dma/128x128-8w", "fast/dma/256x64", "generic/dma-lanetap/128x64/ns2",
    "generic/dma-lanetap/128x64/ns3", "generic/kload/128x64", "generic/kload/128x128",
    "point/kload/128x64", "fast/kload/128x64", "fast/kload/128x128",   # fp32
    "stem-direct",                                                     # the pixel-pair stem
}
DGRAD_PATHS = {
    "point/dma/128x64/ns2", "point/dma/128x128-8w", "fast/dma/128x64/ns3", "fast/dma/256x64",
    "fast/dma/128x128-8w", "generic/kload/128x64", "phases-merged/dma/128x64",
    "phases-merged/dma/128x128", "phases-each/kload/128x64",
    "point/kload/128x64", "phases-each/kload/128x128",               # fp32
}
WGRAD_PATHS = {
    "64x64/DmaR-point/ns3/reduce", "64x64/DmaR-point/ns3/reduce-z", "128x64/DmaR-point/ns3/reduce",
    "128x128/DmaR-point/ns2/reduce", "128x128/DmaR-point/ns3/reduce", "64x128/DmaRq/ns2/reduce",
    "64x128/DmaRq/ns3/reduce", "128x64/DmaRq/ns2/reduce", "128x128/DmaRq/ns2/reduce",
    "128x128/DmaRq/ns3/reduce", "128x128/DmaR/ns3/reduce",
    "64x64/RLoad/reduce", "64x128/RLoad/reduce", "128x128/RLoad/reduce",   # fp32
    "stem-direct/reduce",                                                  # the pixel-pair stem
}
RUNS = [(cid, None) for cid in ALL] + R.KNOB_RUNS
# The pixel-pair stem (mmdx_stem_pair_desc of a 2 x 3 x 224 x 224 batch, 7x7 / 2 / pad 3): its
# direct kernels by default, the implicit GEMM with MMDX_STEM_DIRECT=0.  Mirror only: on the GPU
# tests/test_stem_pair_gpu.py and the trunk tests run it.
STEM_PAIR = (2, 8, 230, 115, 64, 7, 4, 2, 1, 0, 0)
STEM_RUNS = [(STEM_PAIR, None), (STEM_PAIR, {"MMDX_STEM_DIRECT": 0})]


def _reached():
    fwd, dgrad, wgrad = set(), set(), set()
    for cid, kn in RUNS:
        cfg, cm, dt = R.case(cid)
        p = R.expected_path(cfg, dt, kn)
        wgrad.add(p.wgrad)
        if cid not in R.WGRAD_ONLY:
            fwd.add(p.fwd)
            dgrad.add(p.dgrad)
    for cfg, kn in STEM_RUNS:               # the stem has no data gradient
        p = R.expected_path(cfg, BF16, kn)
        fwd.add(p.fwd)
        wgrad.add(p.wgrad)
    dgrad.add(R.expected_path(R.case(5)[0], BF16, None, beta=1.0).dgrad)
    return fwd, dgrad, wgrad


def test_case_table_reaches_every_dispatcher_path():
    fwd, dgrad, wgrad = _reached()
    assert fwd == FWD_PATHS, (sorted(FWD_PATHS - fwd), sorted(fwd - FWD_PATHS))
    assert dgrad == DGRAD_PATHS, (sorted(DGRAD_PATHS - dgrad), sorted(dgrad - DGRAD_PATHS))
    assert wgrad == WGRAD_PATHS, (sorted(WGRAD_PATHS - wgrad), sorted(wgrad - WGRAD_PATHS))


def _path(cid, knobs=None):
    cfg, cm, dt = R.case(cid)
    return R.expected_path(cfg, dt, knobs)


def test_each_case_reaches_the_edge_it_is_in_the_table_for():
    """The table's comments as assertions: dropping or changing a case fails here."""
    def rows(cid, dgrad=False):
        cfg = R.case(cid)[0]
        P, Q = R.out_size(cfg)
        return cfg[0] * (cfg[2] * cfg[3] if dgrad else P * Q)

    assert rows(1) == 35 and _path(1).fwd.startswith("fast/dma/128x64")
    assert rows(2) == 162 and R.case(2)[0][4] % 64 == 8 and _path(2).dgrad == "generic/kload/128x64"
    assert _path(3).fwd == "point/dma/128x64/ns2" and R.case(3)[0][1] == 2 * 64
    assert sorted(p["M"] // 2 for p in _path(4).phases) == [42, 48, 49, 56]
    assert _path(4).dgrad == _path(5).dgrad == _path(6).dgrad == "phases-merged/dma/128x64"
    assert [p["K"] for p in _path(5).phases] == [128, 0, 0, 0]
    assert all(p["K"] for p in _path(6).phases) and not R.reached(R.case(6)[0])[-1].any() \
        and not R.reached(R.case(6)[0])[:, -1].any()
    assert _path(7).fwd == "generic/kload/128x64" and (9 * 24) % 64 != 0
    assert _path(8).fwd == "generic/dma-lanetap/128x64/ns2" and (9 * 16) % 64 != 0
    assert _path(9).fwd.startswith("generic/dma-lanetap") and _path(9).dgrad.startswith("fast/dma")
    assert _path(10).fwd.startswith("generic/dma-lanetap") and _path(10).dgrad.startswith("phases-each")
    assert R.case(10)[1] == 3
    assert rows(11) == 194 * 128 + 116
    assert _path(11).fwd == _path(11).dgrad == "point/dma/128x128-8w"
    assert _path(12).fwd == "fast/dma/128x128-8w"
    assert rows(13) == 256 + 41 and _path(13, R.KNOB_RUNS[0][1]).fwd == "fast/dma/256x64" \
        and _path(13, R.KNOB_RUNS[0][1]).dgrad == "fast/dma/256x64" and "256" not in _path(13).fwd
    p = _path(14).plan
    assert (p.bm, p.bn, p.splits) == (64, 64, 2) and rows(14) == 2205 and 2205 - p.kper == 1053 \
        and 1053 % 64 != 0
    assert _path(15).wgrad == "128x128/DmaRq/ns3/reduce" \
        and _path(15, R.KNOB_RUNS[1][1]).wgrad == "128x128/DmaR/ns3/reduce"
    assert _path(16).wgrad.startswith("64x128/") and _path(17).wgrad.startswith("128x64/")
    assert _path(18).plan.splits == 9
    assert _path(19).plan.splits >= 128 and _path(19).wgrad.endswith("reduce-z")
    assert R.case(20)[0][2:4] == (1, 1) and R.out_size(R.case(20)[0]) == (1, 1)   # 8 of 9 taps out
    c = R.case(21)[0]
    assert c[5] != c[6] and c[7] != c[8] and c[9] != c[10] and c[2] != c[3]
    assert R.case(22)[0][1] * 9 == 4608
    assert _path(23).fwd == "generic/kload/128x128"
    assert _path(24).dgrad == "phases-merged/dma/128x128" \
        and sum((p["M"] + 127) // 128 for p in _path(24).phases) == 392 \
        and all(p["M"] % 128 for p in _path(24).phases)
    assert _path(25).dgrad == "fast/dma/128x128-8w"
    assert _path("f1").fwd == _path("f1").dgrad == "generic/kload/128x64"
    assert _path("f2").dgrad == "generic/kload/128x64" and R.case("f2")[0][7] == 2
    assert _path("f3").dgrad == _path("f5").dgrad == "phases-each/kload/128x64"
    assert len(_path("f3").phases) == 2 and len(_path("f5").phases) == 4
    assert _path("f4").wgrad == "64x64/RLoad/reduce" and _path("f4").plan.splits > 1
    assert _path("f6").fwd == "fast/kload/128x128" and _path("f6").wgrad == "128x128/RLoad/reduce"
    assert _path("f7").dgrad == "phases-each/kload/128x128"


def test_mirror_predicates():
    """Hand-worked values of the mirrored predicates at their thresholds."""
    assert R.is_pointwise((1, 8, 4, 4, 8, 1, 1, 1, 1, 0, 0))
    assert not R.is_pointwise((1, 8, 4, 4, 8, 1, 1, 2, 2, 0, 0))
    assert not R.is_pointwise((1, 8, 4, 4, 8, 1, 1, 1, 1, 1, 1))
    c = (2, 8, 12, 12, 64, 5, 5, 1, 1, 2, 2)
    assert R.dma_geom_ok(c, False) and R.dma_geom_ok(c, True) and not R.dma_geom_ok(c, False, 24)
    assert not R.dma_geom_ok((2, 8, 12, 12, 64, 5, 5, 2, 1, 2, 2), True)
    assert not R.dma_geom_ok(c, False, 32, (1 << 22) - 256) and R.dma_geom_ok(c, False, 32, (1 << 22) - 257)
    # kNarrowBelow: 383 tiles of 128x128 stay narrow, 384 do not
    k1 = (1, 64, 1, 191 * 128, 256, 1, 1, 1, 1, 0, 0)
    k2 = (1, 64, 1, 192 * 128, 256, 1, 1, 1, 1, 0, 0)
    assert R.expected_path(k1, BF16).fwd.startswith("point/dma/128x64")
    assert R.expected_path(k2, BF16).fwd == "point/dma/128x128-8w"
    assert R.expected_path(k2, BF16, {"MMDX_CONV_8W128": 0}).fwd == "point/dma/128x128/ns2"
    # conv_n64_wide on its own: from 1024 blocks of 256 rows
    n1 = (1, 64, 1, 1023 * 256, 64, 1, 1, 1, 1, 0, 0)
    n2 = (1, 64, 1, 1023 * 256 + 1, 64, 1, 1, 1, 1, 0, 0)
    assert R.expected_path(n1, BF16).fwd.startswith("point/dma/128x64")
    assert R.expected_path(n2, BF16).fwd == "point/dma/256x64"
    assert R.expected_path(n2, BF16, {"MMDX_CONV_N64_WIDE": 0}).fwd.startswith("point/dma/128x64")
    # the benched layer1 3x3 weight gradient: 128 x 56 x 56 pixels over 5 tiles of 64 x 128
    p = R.plan_wgrad((128, 64, 56, 56, 64, 3, 3, 1, 1, 1, 1), BF16)
    assert (p.bm, p.bn, p.splits, p.kper) == (64, 128, 52, 7744)


def test_plan_mirror_matches_the_library():
    """plan_wgrad's splits against mmdx_conv_wgrad_workspace_size / (4 K R S C), and the slab
    counts, through the library's host-side calls (no GPU needed)."""
    from mmdx import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libmmdx_hip.so is not built")
    for cid in ALL:
        cfg, cm, dt = R.case(cid)
        N, C, H, W, K, Rr, S, sh, sw, ph, pw = cfg
        P, Q = R.out_size(cfg)
        d = L.ConvDesc(N, H, W, C, K, Rr, S, sh, sw, ph, pw, P, Q)
        ws = L.lib().mmdx_conv_wgrad_workspace_size(L.dtype_code(dt), d)
        assert ws == R.expected_path(cfg, dt).plan.splits * 4 * K * Rr * S * C, cid
        assert L.lib().mmdx_conv_dgrad_stat_blocks(L.dtype_code(dt), d) == R.dgrad_stat_blocks(cfg, dt)
        assert L.lib().mmdx_conv_fwd_stat_rows(d) == 128
        assert L.lib().mmdx_conv_fwd_stat_blocks(d) == (N * P * Q + 127) // 128


# ------------------------------------------------------- the mirror against mmdx_conv_describe
K1 = (1, 64, 1, 191 * 128, 256, 1, 1, 1, 1, 0, 0)       # test_mirror_predicates' thresholds
K2 = (1, 64, 1, 192 * 128, 256, 1, 1, 1, 1, 0, 0)
N1 = (1, 64, 1, 1023 * 256, 64, 1, 1, 1, 1, 0, 0)
N2 = (1, 64, 1, 1023 * 256 + 1, 64, 1, 1, 1, 1, 0, 0)
# 1x1 / stride 2 over four phases of 104 tiles of 128 x 128 each, one of them reached: 416 tiles
# at beta 0 (all launched), 104 at beta 1, on the two sides of kNarrowBelow
B1 = (13, 128, 64, 64, 64, 1, 1, 2, 2, 0, 0)
KNOB_NAMES = ["MMDX_CONV_N64_WIDE", "MMDX_CONV_8W128", "MMDX_WGRAD_RQ", "MMDX_STEM_DIRECT"]


def _resnet_convs():
    """Every distinct conv of ResNet-18 and ResNet-50 at 224 x 224 (enumerated from the modules
    by tools/conv_bench.py) at three batches, as descriptors with the channels the kernels see;
    the stems both channel-padded and as the pixel-pair conv of mmdx_stem_pair_desc."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "tools"))
    import conv_bench
    from mmdx import _lib as L
    cfgs, pairs = set(), set()
    for arch in ("resnet18", "resnet50"):
        for (H, W, C, K, k, s, p), info in conv_bench.shapes(arch, 224).items():
            for B in (64, 128, 256):
                cfgs.add((B, R.pad_channels(C, BF16), H, W, K, k, k, s, s, p, p))
                if info["tag"] == "stem":
                    d = L.ConvDesc()
                    L.call("mmdx_stem_pair_desc", B, C, H, W, K, k, k, s, p, d)
                    pairs.add((d.N, d.C, d.H, d.W, d.K, d.R, d.S, d.stride_h, d.stride_w,
                               d.pad_h, d.pad_w))
    return sorted(cfgs), sorted(pairs)


def _assert_mirror_is_describe(lib, cfg, dt, kn, what, beta=0.0):
    e = R.expected_path(cfg, dt, kn, beta)
    for pas in ((1,) if beta else (0, 1, 2)):
        assert e.desc(pas) == R.describe(lib, cfg, dt, pas, beta), (what, pas, kn, beta)
    return e


def test_mirror_equals_describe(knobs):
    """expected_path() == mmdx_conv_describe() (which prints what the launches consult) for fwd,
    dgrad at beta 0 and wgrad: the case table and its knob runs, the threshold shapes, the
    ResNet-18 / -50 trunks at batch 64 / 128 / 256, the pixel-pair stem with and without its
    direct kernels, and the strided dgrad at beta 1, where unreached phases leave the grid."""
    from mmdx import _lib as L
    lib = L.lib()

    def set_knobs(kn):
        for name in KNOB_NAMES:
            knobs(name, (kn or {}).get(name))

    for cid, kn in RUNS:
        cfg, cm, dt = R.case(cid)
        set_knobs(kn)
        _assert_mirror_is_describe(lib, cfg, dt, kn, cid)
    for cfg, kn in [(K1, None), (K2, None), (N1, None), (N2, None), (B1, None),
                    (K2, {"MMDX_CONV_8W128": 0}), (N2, {"MMDX_CONV_N64_WIDE": 0})] + STEM_RUNS:
        set_knobs(kn)
        _assert_mirror_is_describe(lib, cfg, BF16, kn, cfg)
    d = L.ConvDesc()
    L.call("mmdx_stem_pair_desc", 2, 3, 224, 224, 64, 7, 7, 2, 3, d)
    assert STEM_PAIR == (d.N, d.C, d.H, d.W, d.K, d.R, d.S, d.stride_h, d.stride_w, d.pad_h,
                         d.pad_w)
    cfgs, pairs = _resnet_convs()
    assert len(cfgs) == 3 * 29 and len(pairs) == 3     # 29 distinct convs over the two trunks
    for direct in (1, 0):
        kn = {"MMDX_STEM_DIRECT": direct}
        set_knobs(kn)
        for cfg in cfgs + pairs:
            _assert_mirror_is_describe(lib, cfg, BF16, kn, cfg)
    # dgrad at beta 1: case 5 launches one phase of its four; B1 changes tile with it
    set_knobs(None)
    for cfg in (R.case(5)[0], B1):
        _assert_mirror_is_describe(lib, cfg, BF16, None, cfg, beta=1.0)
    assert R.expected_path(B1, BF16).dgrad == "phases-merged/dma/128x128"
    assert R.expected_path(B1, BF16, None, 1.0).dgrad == "phases-merged/dma/128x64"
    e = R.expected_path(pairs[0], BF16)
    assert (e.fwd, e.wgrad) == ("stem-direct", "stem-direct/reduce-z") and e.plan.splits == 256


def test_describe_rejects_bad_arguments():
    import ctypes
    from mmdx import _lib as L
    lib = L.lib()
    cfg = R.case(1)[0]
    N, C, H, W, K, Rr, S, sh, sw, ph, pw = cfg
    d = L.ConvDesc(N, H, W, C, K, Rr, S, sh, sw, ph, pw, *R.out_size(cfg))
    buf = ctypes.create_string_buffer(96)
    assert lib.mmdx_conv_describe(L.BF16, 0, d, 0.0, buf, 96) == 0
    assert buf.value.decode() == R.expected_path(cfg, BF16).fwd
    assert lib.mmdx_conv_describe(L.BF16, 0, d, 0.0, buf, 4) != 0          # short buffer
    assert lib.mmdx_conv_describe(L.BF16, 0, d, 0.0, None, 96) != 0
    assert lib.mmdx_conv_describe(7, 0, d, 0.0, buf, 96) != 0 and buf.value == b""
    assert lib.mmdx_conv_describe(L.F16, 0, d, 0.0, buf, 96) != 0          # fp16: no conv path
    assert lib.mmdx_conv_describe(L.BF16, 3, d, 0.0, buf, 96) != 0
    assert lib.mmdx_conv_describe(L.BF16, -1, d, 0.0, buf, 96) != 0
    assert lib.mmdx_conv_describe(L.BF16, 0, None, 0.0, buf, 96) != 0
    d.P += 1                                                                # inconsistent
    assert lib.mmdx_conv_describe(L.BF16, 0, d, 0.0, buf, 96) != 0


# ------------------------------------------------------------------------------ sensitivity
def test_one_missing_term_is_rejected_where_the_old_bar_accepts_it():
    """Case 2's forward with one x * w term removed from a border pixel (the corner (0, 0): its
    centre tap, the median-magnitude channel of that tap): the exact comparison and the Gaussian
    bound reject it; test_kernels_gpu._close at TOL[bf16] accepts it."""
    from test_kernels_gpu import _close
    cfg, cm, dt = R.case(2)
    n, k, p, q, r, s = 0, 5, 0, 0, 1, 1

    x, w, dy, _ = R.operands(2, "int")
    ref = R.ref_fwd(x, w, cfg)
    terms = x[n, :, p, q] * w[k, :, r, s]          # ih = p - 1 + r = 0, iw = 0
    c = terms.abs().argmax().item()
    assert terms[c].abs() == 1
    bad = ref.clone()
    bad[n, k, p, q] -= terms[c]
    R.assert_exact(ref.to(dt), ref, "unchanged")
    with pytest.raises(AssertionError, match="1 of"):
        R.assert_exact(bad.to(dt), ref, "one term missing")

    x, w, dy, _ = R.operands(2, "gauss")
    ref, abs_terms = R.ref_fwd(x, w, cfg), R.ref_abs_fwd(x, w, cfg)
    terms = x[n, :, p, q] * w[k, :, r, s]
    c = terms.abs().argsort()[len(terms) // 2].item()
    bad = ref.clone()
    bad[n, k, p, q] -= terms[c]
    assert R.assert_bounded("fwd", ref.to(dt), ref, abs_terms, dt, "rounded once") <= 1.0
    with pytest.raises(AssertionError, match="error / bound"):
        R.assert_bounded("fwd", bad.to(dt), ref, abs_terms, dt, "one term missing")
    _close(bad.to(dt), ref, dt, "one term missing")     # does not raise
