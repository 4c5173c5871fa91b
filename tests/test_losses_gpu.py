"""GPU: the fused disease loss (csrc/loss.hip, functional.disease_loss, mmdx.DiseaseLoss) against
mmdx.losses.reference in float64, masked evaluate(), the loader's label policies and the driver.

Tolerance: the project's own for fp32 kernels, rtol 1e-5 / atol 1e-6 (test_kernels_gpu.py),
applied after dividing both sides by max(cw) * max(pw, 1) * (1 + gamma), the factor by which the
weights and the focal derivative scale a term.

Shapes are the smallest at which the reduction can go wrong for the kernel's constants (256
threads, of which TB = (256 / C) * C work: 247 for C = 13; 8 elements per thread before the grid
grows; at most 1024 blocks):
  [1, 1]; [3, 13] (less than one wave); [65, 1] and [5, 13] (just over one wave); [257, 1] and
  [20, 13] (just over one pass of a block: the thread loop iterates); [2049, 1] and [153, 13]
  (just over one block's 8 passes: two blocks, the ticket hand-off); [1031, 13] (7 blocks, ragged
  tail); [5, 64] (maximum C); [160001, 13] (2,080,013 elements > 1024 * 247 * 8 = 2,023,424: the
  grid is capped and the stride loop runs a ninth pass).
"""
import io
import json
import math
import os

import numpy as np
import pytest
import torch

import mmdx
import mmdx.functional as F
from mmdx import data as D
from mmdx import losses as LS
from mmdx import metrics as M

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BUCKET = "medical-ml-proj-bucket"
NAN = float("nan")
RTOL, ATOL = 1e-5, 1e-6

BIG = (160001, 13)
SHAPES = [(1, 1), (3, 13), (65, 1), (5, 13), (257, 1), (20, 13), (2049, 1), (153, 13),
          (1031, 13), (5, 64), BIG]
GAMMAS = [0.0, 2.0, 3.5]
EPSS = [0.0, 0.1]


# ----------------------------------------------------------------------------- inputs, reference
_INPUTS = {}
_REFS = {}


def inputs(B, C):
    """4 randn logits; targets ~20 % positives, ~10 % soft values, ~15 % NaN; pw in [0.5, 5.5],
    cw in [0.5, 1.5].  Made once per shape and never written to."""
    key = (B, C)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * B + C)
        z = 4.0 * torch.randn(B, C, generator=g)
        y = (torch.rand(B, C, generator=g) < 0.2).float()
        y = torch.where(torch.rand(B, C, generator=g) < 0.1, torch.rand(B, C, generator=g), y)
        y = torch.where(torch.rand(B, C, generator=g) < 0.15, torch.full_like(y, NAN), y)
        pw = 0.5 + 5.0 * torch.rand(C, generator=g)
        cw = 0.5 + torch.rand(C, generator=g)
        _INPUTS[key] = (z, y, pw, cw)
    return _INPUTS[key]


def ref64(z, y, pw, cw, gamma, eps):
    """float64: (sum e, stats [C, 2], un-normalised gradient g, labelled count)."""
    z64 = z.double()
    pw64 = None if pw is None else pw.double()
    cw64 = None if cw is None else cw.double()
    total, stats = LS.reference(z64, y, pw64, cw64, gamma, eps, "sum")
    g = LS.reference_grad(z64, y, pw64, cw64, gamma, eps)
    return total.item(), stats, g, float(stats[:, 1].sum().item())


def shared_ref(B, C, gamma, eps):
    key = (B, C, gamma, eps)
    if key not in _REFS:
        _REFS[key] = ref64(*inputs(B, C), gamma, eps)
    return _REFS[key]


def scale_of(pw, cw, gamma):
    s = 1.0 + gamma
    if cw is not None:
        s *= float(cw.max())
    if pw is not None:
        s *= max(float(pw.max()), 1.0)
    return s


def excess(got, want, s):
    """max of |got - want| / s - (ATOL + RTOL |want| / s): <= 0 passes.  Also the raw maximum
    error, for the record."""
    got = torch.as_tensor(got, dtype=torch.float64).cpu().reshape(-1)
    want = torch.as_tensor(want, dtype=torch.float64).reshape(-1)
    assert torch.isfinite(got).all()
    err = (got - want).abs()
    return ((err - RTOL * want.abs()) / s - ATOL).max().item(), err.max().item()


def run(dev, z, y, pw, cw, gamma, eps, reduction, upstream=None, dtype=torch.float32):
    """loss, stats, dz of one call on the device (dz from loss.backward(), or from
    (loss * upstream).backward() with a device scalar, as GradScaler supplies it)."""
    zd = z.to(dev).to(dtype).requires_grad_(True)
    yd = y.to(dev)
    pwd = None if pw is None else pw.to(dev)
    cwd = None if cw is None else cw.to(dev)
    loss, stats = F.disease_loss(zd, yd, pwd, cwd, gamma, eps, reduction)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
    assert stats.shape == (z.shape[1], 2) and not stats.requires_grad and stats.is_cuda
    if upstream is None:
        loss.backward()
    else:
        (loss * upstream).backward()
    assert zd.grad.dtype == dtype and zd.grad.shape == z.shape
    return loss.detach(), stats.detach(), zd.grad


# ----------------------------------------------------------------------------- parity
@pytest.mark.parametrize("eps", EPSS)
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity_with_the_float64_reference(dev, shape, gamma, eps):
    B, C = shape
    z, y, pw, cw = inputs(B, C)
    total, stats64, g64, count = shared_ref(B, C, gamma, eps)
    s = scale_of(pw, cw, gamma)
    up = torch.full((), 65536.0, device=dev)
    worst = {}
    for reduction in ("mean", "sum"):
        norm = max(count, 1.0) if reduction == "mean" else 1.0
        for upstream in (None, up):
            loss, stats, dz = run(dev, z, y, pw, cw, gamma, eps, reduction, upstream)
            k = 1.0 if upstream is None else 65536.0
            for name, got, want in (("loss", loss, total / norm), ("stats_e", stats[:, 0],
                                                                   stats64[:, 0]),
                                    ("dz", dz, g64 * (k / norm))):
                # an upstream factor scales dz and its error alike: compare in loss units
                ex, err = excess(got.double() / (k if name == "dz" else 1.0),
                                 torch.as_tensor(want, dtype=torch.float64)
                                 / (k if name == "dz" else 1.0), s)
                worst[name] = max(worst.get(name, 0.0), err)
                assert ex <= 0.0, (name, reduction, upstream is not None, err)
            assert torch.equal(stats[:, 1].cpu().double(), stats64[:, 1])   # counts are exact
    print(f"loss_parity [{B}, {C}] gamma={gamma} eps={eps}: max abs err loss "
          f"{worst['loss']:.3e} stats {worst['stats_e']:.3e} dz {worst['dz']:.3e} "
          f"(|loss sum| {abs(total):.3e}, scale {s:.2f})")


@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(3, 13), (1031, 13), (5, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_low_precision_logits(dev, shape, dtype, gamma):
    """bf16 / fp16 logits: the reference is evaluated on the rounded logits.  The loss keeps the
    fp32 bound.  dz is rounded once from fp32, so it lies within one unit roundoff (2^-8 relative
    for bf16, 2^-11 for fp16) of the float64 value - plus half the subnormal spacing where fp16
    underflows - and at most one ulp away from that value rounded to the dtype."""
    B, C = shape
    z, y, pw, cw = inputs(B, C)
    zr = z.to(dtype).float()
    total, stats64, g64, count = ref64(zr, y, pw, cw, gamma, 0.1)
    s = scale_of(pw, cw, gamma)
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    tiny = 2.0 ** -24 if dtype == torch.float16 else 0.0    # fp16's subnormal spacing
    up = torch.full((), 65536.0, device=dev)
    for reduction, upstream, k in (("sum", None, 1.0), ("mean", up, 65536.0 / max(count, 1.0))):
        loss, stats, dz = run(dev, z, y, pw, cw, gamma, 0.1, reduction, upstream, dtype)
        norm = max(count, 1.0) if reduction == "mean" else 1.0
        ex, err = excess(loss, total / norm, s)
        assert ex <= 0.0, ("loss", reduction, err)
        assert excess(stats[:, 0], stats64[:, 0], s)[0] <= 0.0
        want = g64 * k
        got = dz.cpu().double()
        assert torch.isfinite(got).all()
        d = (got - want).abs()
        # fp32 arithmetic error (RTOL of the scaled term) on top of the one rounding
        fp32_room = RTOL * want.abs() + ATOL * s * k
        room = u * want.abs() + 0.5 * tiny + fp32_room
        assert (d <= room).all(), (reduction, (d - room).max().item())
        rounded = want.to(dtype).double()
        ulp = torch.maximum(2.0 ** (torch.floor(torch.log2(rounded.abs().clamp(min=1e-300)))
                                    - (7 if dtype == torch.bfloat16 else 10)),
                            torch.full_like(rounded, tiny))
        assert ((got - rounded).abs() <= ulp + fp32_room).all()
        print(f"loss_parity {dtype} [{B}, {C}] gamma={gamma} {reduction}: dz max rel err "
              f"{(d / want.abs().clamp(min=1e-30))[want.abs() > 1e-3 * k].max().item():.3e} "
              f"(unit roundoff {u:.3e}), not bit-equal to the rounded reference: "
              f"{int((got != rounded).sum())} of {got.numel()}")


def test_defaults_agree_with_bce_with_logits(dev):
    """DiseaseLoss() on NaN-free hard labels and mmdx.BCEWithLogitsLoss(): both within the fp32
    tolerance of the float64 reference (not bit for bit: the reduction order differs)."""
    g = torch.Generator().manual_seed(5)
    z = 4.0 * torch.randn(128, 13, generator=g)
    y = (torch.rand(128, 13, generator=g) < 0.2).float()
    zr = z.double().requires_grad_(True)
    want = torch.nn.functional.binary_cross_entropy_with_logits(zr, y.double())
    want.backward()
    assert abs(LS.reference(z.double(), y)[0].item() - want.item()) <= 1e-14
    for crit in (mmdx.DiseaseLoss(), mmdx.BCEWithLogitsLoss()):
        zd = z.to(dev).requires_grad_(True)
        loss = crit(zd, y.to(dev))
        loss.backward()
        assert excess(loss.detach(), want.item(), 1.0)[0] <= 0.0
        assert excess(zd.grad, zr.grad, 1.0)[0] <= 0.0


# ----------------------------------------------------------------------------- extremes
EXTREME = [20.0, -20.0, 88.0, -88.0, 1e4, -1e4, 3e38, -3e38, 0.0]


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_extreme_logits_are_finite_and_match(dev, gamma):
    """Every logit x label in ONE launch: class c of a [1, 36] problem is one combination, so
    stats[c] is that element's loss term (the whole sum would overflow fp32: four terms of 3e38).
    Default weights: a weighted term cw pw 3e38 is beyond fp32 by definition."""
    labels = [0.0, 1.0, 0.3, NAN]
    z = torch.tensor([[v for v in EXTREME for _ in labels]])
    y = torch.tensor([[lab for _ in EXTREME for lab in labels]])
    assert z.shape == (1, 36)
    zd = z.to(dev).requires_grad_(True)
    loss, stats = F.disease_loss(zd, y.to(dev), gamma=gamma, reduction="sum")
    loss.backward()
    e = stats[:, 0].cpu()
    dz = zd.grad.cpu()
    assert torch.isfinite(e).all() and torch.isfinite(dz).all()
    assert dz.abs().max().item() <= (1.0 + gamma)              # bounded: cw (gamma + 1) max(pw, 1)
    ignored = torch.isnan(y[0])
    assert torch.equal(dz[0][ignored].view(torch.int32),
                       torch.zeros(int(ignored.sum()), dtype=torch.int32))   # exactly +0
    assert not e[ignored].any()
    assert torch.equal(stats[:, 1].cpu(), (~ignored).float())
    # per element against float64 (every one of these is finite there)
    z64 = z.double()
    e64 = torch.stack([LS.reference(z64[:, c:c + 1], y[:, c:c + 1], None, None, gamma, 0.0,
                                    "sum")[0] for c in range(36)])
    g64 = LS.reference_grad(z64, y, None, None, gamma)
    assert torch.isfinite(e64).all() and torch.isfinite(g64).all()
    s = 1.0 + gamma
    assert excess(e, e64, s)[0] <= 0.0
    assert excess(dz, g64, s)[0] <= 0.0
    # the sum itself: finite where it is representable (leave the four 3e38 columns out)
    keep = z[0].abs() < 1e38
    zk = z[:, keep].contiguous().to(dev)
    loss_k, _ = F.disease_loss(zk, y[:, keep].contiguous().to(dev), gamma=gamma)
    want = e64[keep].sum().item() / float((~ignored & keep).sum())
    assert math.isfinite(loss_k.item()) and excess(loss_k, want, s)[0] <= 0.0


def test_large_weighted_logits_stay_finite(dev):
    """+-1e4 with pos_weight 5.5 and class weight 1.5, and a gradient that stays finite even
    where the weighted loss term itself leaves fp32 (3e38 x 5.5)."""
    z = torch.tensor([[1e4, -1e4, 3e38, -3e38]])
    y = torch.tensor([[0.0, 1.0, 0.3, 1.0]])
    pw, cw = torch.full((4,), 5.5), torch.full((4,), 1.5)
    for gamma in (0.0, 2.0, 3.5):
        zd = z.to(dev).requires_grad_(True)
        loss, stats = F.disease_loss(zd, y.to(dev), pw.to(dev), cw.to(dev), gamma,
                                     reduction="sum")
        loss.backward()
        assert torch.isfinite(zd.grad).all()
        assert zd.grad.abs().max().item() <= 1.5 * 5.5 * (1.0 + gamma)
        e = stats[:2, 0].cpu()
        want = torch.stack([LS.reference(z[:, c:c + 1].double(), y[:, c:c + 1], pw[c:c + 1].double(),
                                         cw[c:c + 1].double(), gamma, 0.0, "sum")[0]
                            for c in range(2)])
        assert torch.isfinite(e).all()
        assert excess(e, want, 1.5 * 5.5 * (1.0 + gamma))[0] <= 0.0


# ----------------------------------------------------------------------------- masking
@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_all_ignored_batch(dev, gamma):
    z = torch.randn(40, 13)
    y = torch.full((40, 13), NAN)
    for reduction in ("mean", "sum"):
        loss, stats, dz = run(dev, z, y, None, None, gamma, 0.1, reduction,
                              torch.full((), 65536.0, device=dev))
        assert loss.item() == 0.0
        assert not stats.cpu().any()
        assert torch.equal(dz.cpu().view(torch.int32), torch.zeros(40, 13, dtype=torch.int32))


def test_one_ignored_column_leaves_the_others_alone(dev):
    B, C = 1031, 13
    z, y, pw, cw = inputs(B, C)
    y = y.clone()
    y[:, 4] = NAN
    keep = [c for c in range(C) if c != 4]
    a = run(dev, z, y, pw, cw, 2.0, 0.1, "sum")
    b = run(dev, z[:, keep].contiguous(), y[:, keep].contiguous(), pw[keep], cw[keep], 2.0, 0.1,
            "sum")
    assert a[1][4].tolist() == [0.0, 0.0]
    assert not a[2][:, 4].cpu().any()
    # a thread keeps its class, but rows land on other threads at C = 12: sums to rounding,
    # element gradients bit for bit
    assert torch.equal(a[1][keep, 1], b[1][:, 1])
    s = scale_of(pw, cw, 2.0)
    assert excess(a[1][keep, 0], b[1][:, 0].cpu().double(), s)[0] <= 0.0
    assert excess(a[0], b[0].cpu().double(), s)[0] <= 0.0
    assert torch.equal(a[2][:, keep], b[2])


# ----------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("gamma", [0.0, 3.5])
def test_two_calls_give_the_same_bits_and_leave_the_inputs_alone(dev, gamma):
    B, C = BIG
    z, y, pw, cw = inputs(B, C)
    zd, yd, pwd, cwd = z.to(dev), y.to(dev), pw.to(dev), cw.to(dev)
    before = [t.clone() for t in (zd, yd, pwd, cwd)]
    outs = []
    for _ in range(2):
        zg = zd.detach().requires_grad_(True)
        loss, stats = F.disease_loss(zg, yd, pwd, cwd, gamma, 0.1)
        loss.backward()
        outs.append((loss.detach().clone(), stats.clone(), zg.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for t, was in zip((zd, yd, pwd, cwd), before):
        assert torch.equal(t.view(torch.int32), was.view(torch.int32))


# ----------------------------------------------------------------------------- autograd
def test_autograd_through_a_linear_head_and_no_grad(dev):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(64, 32, generator=g)
    w = 0.3 * torch.randn(13, 32, generator=g)
    b = 0.1 * torch.randn(13, generator=g)
    y = (torch.rand(64, 13, generator=g) < 0.2).float()
    y[::7, 3] = NAN
    pw = 0.5 + 5.0 * torch.rand(13, generator=g)
    crit = mmdx.DiseaseLoss(pos_weight=pw, gamma=2.0, label_smoothing=0.1)

    w64 = w.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    want, stats64 = LS.reference(x.double() @ w64.t() + b64, y, pw.double(), None, 2.0, 0.1)
    want.backward()

    wd = w.to(dev).requires_grad_(True)
    bd = b.to(dev).requires_grad_(True)
    xd, yd = x.to(dev), y.to(dev)
    loss = crit(F.linear(xd, wd, bd), yd)
    loss.backward()
    s = scale_of(pw, None, 2.0)
    assert excess(loss.detach(), want.item(), s)[0] <= 0.0
    # a weight gradient sums 64 rows of dz x: its rounding grows with that sum of magnitudes
    rows = x.abs().sum(0).max().item()
    assert excess(wd.grad, w64.grad, s * max(rows / 64.0, 1.0))[0] <= 0.0
    assert excess(bd.grad, b64.grad, s)[0] <= 0.0
    assert crit.stats.shape == (13, 2) and crit.stats.is_cuda
    assert torch.equal(crit.stats[:, 1].cpu().double(), stats64[:, 1])

    with torch.no_grad():
        quiet = crit(F.linear(xd, wd, bd), yd)
    assert not quiet.requires_grad and quiet.grad_fn is None
    assert torch.equal(quiet.view(torch.int32), loss.detach().view(torch.int32))
    # weights are moved once and cached per device
    assert crit._weights_on(dev)[0] is crit._weights_on(dev)[0]


def test_wrapper_errors_are_raised_before_a_launch(dev):
    z = torch.zeros(8, 13, device=dev)
    y = torch.zeros(8, 13, device=dev)
    with pytest.raises((ValueError, TypeError)):
        F.disease_loss(torch.zeros(13, 8, device=dev).t(), y)           # not contiguous
    with pytest.raises((ValueError, TypeError)):
        F.disease_loss(z.double(), y)
    with pytest.raises((ValueError, TypeError)):
        F.disease_loss(z, y[:7])
    with pytest.raises((ValueError, TypeError)):
        F.disease_loss(torch.zeros(2, 65, device=dev), torch.zeros(2, 65, device=dev))
    with pytest.raises((ValueError, TypeError)):
        F.disease_loss(z, y, pos_weight=torch.ones(13))                 # weights on the host
    with pytest.raises((ValueError, TypeError)):
        F.disease_loss(z, y, class_weight=torch.ones(12, device=dev))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- evaluate()
def _ref_row(s, pos):
    """(u2, n_pos, n_neg) of one class from midranks (np.unique), in int64."""
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    _, inv, cnt = np.unique(s, return_inverse=True, return_counts=True)
    cum = np.cumsum(cnt).astype(np.int64)
    rank2 = 2 * cum - cnt + 1
    return int(rank2[inv.reshape(-1)][pos].sum()) - n_pos * (n_pos + 1), n_pos, n_neg


def _ref_sweep(s, pos, thr):
    k = np.searchsorted(thr, s, side="right")
    tp = np.array([(k[pos] > t).sum() for t in range(len(thr))], dtype=np.int64)
    fp = np.array([(k[~pos] > t).sum() for t in range(len(thr))], dtype=np.int64)
    return tp, fp


def _ref_threshold(tp, fp, n_pos, grid):
    best = None
    for t, p in enumerate(grid):
        d = int(tp[t]) + int(fp[t]) + n_pos
        key = (-(2 * int(tp[t]) / d if d else 0.0), round(abs(p - 0.5), 12), p)
        if best is None or key < best:
            best = key
    return best[2]


@pytest.fixture(scope="module")
def eval_model(dev):
    torch.manual_seed(0)
    img = mmdx.ImageEncoderCNN("resnet18", 1024, 13).to(dev)
    txt = mmdx.TextEncoderTransformer("bert-base-uncased@2", 512, 13).to(dev)
    fus = mmdx.FusionTransformerModel(1024, 512, 1024, 13).to(dev)
    g = torch.Generator().manual_seed(21)
    N = 200
    x = torch.randn(N, 3, 64, 64, generator=g)
    y = (torch.rand(N, 13, generator=g) < 0.3).float()
    hole = torch.rand(N, 13, generator=g) < 0.2
    details = [f"{30 + i % 50} year old {'male' if i % 2 else 'female'} PA view, "
               f"{'cough' if i % 3 else 'fever'}, case {i}" for i in range(N)]
    for top in (img, txt, fus):
        top.eval()
    zs = []
    with torch.no_grad():
        for s0 in range(0, N, 48):
            tok = {k: v.to(dev) for k, v in
                   mmdx.tokenize_patient_details(details[s0:s0 + 48], max_len=96).items()}
            zs.append(fus(z_img=img(x[s0:s0 + 48].to(dev))["embeddings"],
                          z_txt=txt(**tok)["embeddings"])["disease_logits"].float())
    z = torch.cat(zs)

    def batches(labels, images=x):
        return [(images[s0:s0 + 48].to(dev), details[s0:s0 + 48], labels[s0:s0 + 48].to(dev))
                for s0 in range(0, N, 48)]            # 48 x 4 + 8: the last batch is ragged
    return img, txt, fus, batches, x, y, hole, z


def test_evaluate_leaves_ignored_labels_out(dev, eval_model):
    img, txt, fus, batches, x, y, hole, z = eval_model
    ym = torch.where(hole, torch.full_like(y, NAN), y)
    lab = ~hole.numpy()
    yn, zn = y.numpy(), z.cpu().numpy()
    for c in range(13):      # never vacuous: both kinds among the labelled rows of every class
        assert (yn[lab[:, c], c] > 0.5).any() and (yn[lab[:, c], c] < 0.5).any()
    assert hole.any(0).all()

    pw = torch.from_numpy(D.pos_weight_from_stats(D.label_stats(ym.numpy())))
    crit = mmdx.DiseaseLoss(pos_weight=pw)
    res = M.evaluate(img, txt, fus, batches(ym), criterion=crit)
    assert res["n"] == 200

    grid = M.default_grid()
    thr = M.grid_logits(grid)
    i_half = grid.index(0.5)
    rows, want_thr, tp5, fp5, tpc, fpc = [], [], 0, 0, 0, 0
    for c in range(13):
        s, pos = zn[lab[:, c], c], yn[lab[:, c], c] > 0.5
        rows.append(_ref_row(s, pos))
        tp, fp = _ref_sweep(s, pos, thr)
        p = _ref_threshold(tp, fp, rows[-1][1], grid)
        want_thr.append(p)
        tp5, fp5 = tp5 + int(tp[i_half]), fp5 + int(fp[i_half])
        tpc, fpc = tpc + int(tp[grid.index(p)]), fpc + int(fp[grid.index(p)])
    want_pc = [u2 / (2 * n_pos * n_neg) for u2, n_pos, n_neg in rows]
    assert res["val_auroc_per_class"] == want_pc
    assert res["val_auroc_macro"] == math.fsum(want_pc) / 13
    u2, n_pos, n_neg = _ref_row(zn[lab], yn[lab] > 0.5)
    assert res["val_auroc_micro"] == u2 / (2 * n_pos * n_neg)
    assert res["thresholds"] == want_thr
    assert [p["n_pos"] for p in res["per_class"]] == [r[1] for r in rows]
    assert n_pos == sum(r[1] for r in rows)
    assert res["val_f1_micro_at_0p5"] == 2 * tp5 / (tp5 + fp5 + n_pos)
    assert res["val_f1_micro"] == 2 * tpc / (tpc + fpc + n_pos)

    want_loss = LS.reference(z.cpu().double(), ym, pw.double())[0].item()
    assert excess(res["val_loss"], want_loss, scale_of(pw, None, 0.0))[0] <= 0.0
    # without a criterion the plain BCE meets the NaN labels; the metrics are the same
    plain = M.evaluate(img, txt, fus, batches(ym))
    assert math.isnan(plain["val_loss"])
    assert {k: v for k, v in plain.items() if k != "val_loss"} == \
           {k: v for k, v in res.items() if k != "val_loss"}


def test_evaluate_is_unchanged_for_complete_labels(dev, eval_model):
    """NaN-free labels, no criterion: every value equals the recomputation from the public pieces
    evaluate() was made of before masking existed."""
    img, txt, fus, batches, x, y, hole, z = eval_model
    res = M.evaluate(img, txt, fus, batches(y))
    yd = y.to(dev)
    grid = M.default_grid()
    loss = F.bce_with_logits(z, yd)
    k = F.auroc_counts(z, yd).cpu().numpy()
    tp, fp = F.confusion_grid(z, yd, torch.from_numpy(M.grid_logits(grid)).to(dev))
    per_class, macro, micro = M.auroc_from_counts(k)
    picked = M.pick_thresholds(tp.cpu().numpy(), fp.cpu().numpy(), k[:13, 1], grid)
    want = {"n": 200, "val_loss": float(loss.item()), "val_auroc_micro": micro,
            "val_auroc_macro": macro, "val_auroc_per_class": per_class,
            "thresholds": picked["thresholds"], "val_f1_micro": picked["micro"]["f1"],
            "val_f1_micro_at_0p5": picked["micro_at_0p5"]["f1"],
            "per_class": picked["per_class"]}
    assert res == want
    assert np.float32(res["val_loss"]).view(np.int32) == loss.cpu().numpy().view(np.int32)


def test_evaluate_still_reports_a_nan_the_model_produced(dev, eval_model):
    img, txt, fus, batches, x, y, hole, z = eval_model
    ym = torch.where(hole, torch.full_like(y, NAN), y)
    assert not hole[:, 3].all()
    bias = [p for p in fus.disease_head.parameters() if tuple(p.shape) == (13,)][-1]
    was = bias.detach().clone()
    try:
        with torch.no_grad():
            bias[3] = NAN                      # every logit of class 3 is NaN, labelled or not
        with pytest.raises(ValueError, match="NaN scores"):
            M.evaluate(img, txt, fus, batches(ym), criterion=mmdx.DiseaseLoss())
    finally:
        with torch.no_grad():
            bias.copy_(was)


# ----------------------------------------------------------------------------- loader, driver
@pytest.fixture(scope="module")
def feature_group(tmp_path_factory):
    """16 generated images with CheXpert-style labels: 0 / 1 with -1 (uncertain) and NaN (not
    mentioned) scattered in."""
    import pandas as pd
    from PIL import Image
    root = tmp_path_factory.mktemp("loss_driver")
    mirror = root / "s3"
    (mirror / BUCKET / "chest-x-ray-images").mkdir(parents=True)
    rng = np.random.default_rng(23)
    rows = []
    for i in range(16):
        key = f"chest-x-ray-images/img{i:02d}.jpg"
        if i == 0:
            data = open(os.path.join(GOLD, "e1.jpg"), "rb").read()
        else:
            h, w = int(rng.integers(240, 320)), int(rng.integers(240, 320))
            arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            buf = io.BytesIO()
            Image.fromarray(arr, "RGB").save(buf, format="JPEG", quality=90)
            data = buf.getvalue()
        (mirror / BUCKET / key).write_bytes(data)
        vec = (rng.random(13) < 0.3).astype(float)
        kind = rng.random(13)
        vec[kind < 0.15] = -1.0
        vec[kind > 0.9] = np.nan
        rows.append({"image_url": f"s3://{BUCKET}/{key}",
                     "patient_details": f"{40 + i} year old {'male' if i % 2 else 'female'} "
                                        f"PA view, cough, case {i}",
                     "disease_classification_vector": json.dumps(vec.tolist()),
                     "report": f"Findings: case {i}. The lungs are clear. No effusion."})
    pq = root / "features.parquet"
    pd.DataFrame(rows).to_parquet(pq)
    # the same rows with complete 0 / 1 labels, for the default run
    for r in rows:
        v = np.asarray(json.loads(r["disease_classification_vector"]), dtype=float)
        r["disease_classification_vector"] = json.dumps((v > 0.5).astype(float).tolist())
    pd.DataFrame(rows).to_parquet(root / "features_complete.parquet")
    return root, mirror, pq


def test_loader_applies_the_uncertain_policy(dev, feature_group):
    root, mirror, pq = feature_group
    df = D.load_features_labels_local(str(pq))
    stored = np.stack([np.asarray(v, dtype=np.float32)
                       for v in df["disease_classification_vector"]])
    assert (stored == -1).any() and np.isnan(stored).any()
    image_root = str(mirror / BUCKET)
    kw = dict(batch_size=8, shuffle=False, device=dev)
    got = torch.cat([b[2] for b in D.LocalCXRBatches(df, image_root, **kw)]).cpu().numpy()
    assert np.array_equal(got.view(np.int32), stored.view(np.int32))       # bit for bit
    ign = torch.cat([b[2] for b in D.LocalCXRBatches(df, image_root, uncertain="ignore",
                                                     **kw)]).cpu().numpy()
    assert np.isnan(ign[stored == -1]).all()
    same = stored != -1
    assert np.array_equal(ign[same].view(np.int32), stored[same].view(np.int32))
    soft = torch.cat([b[2] for b in D.LocalCXRBatches(df, image_root, uncertain=0.25,
                                                      **kw)]).cpu().numpy()
    assert (soft[stored == -1] == 0.25).all() and np.isnan(soft[np.isnan(stored)]).all()


def _drive(feature_group, sub, complete=False, **kw):
    root, mirror, pq = feature_group
    if complete:
        pq = root / "features_complete.parquet"
    old = dict(os.environ)
    os.environ.update(MMDX_FEATURES_PARQUET=str(pq), MMDX_S3_MIRROR=str(mirror),
                      AWS_S3_BUCKET_NAME=BUCKET, MMDX_MODEL_REGISTRY=str(root / sub / "registry"),
                      MMDX_MODEL_DIR=str(root / sub / "model"))
    try:
        torch.manual_seed(0)
        out = mmdx.training_pipeline.training_tests(
            num_steps=2, b_fusion=2, batch_size=4, image_backbone="resnet18",
            text_model="bert-base-uncased@2", save=True,
            gen_kwargs=dict(max_new_tokens=4, min_new_tokens=1, num_beams=2), verbose=False,
            **kw)
        torch.cuda.synchronize()
    finally:
        os.environ.clear()
        os.environ.update(old)
    return out, str(root / sub / "model" / "model_bundle.pt")


def test_driver_trains_with_the_criterion_and_stores_its_config(dev, feature_group):
    from PIL import Image
    from mmdx.inference_pipeline import inference, load_model_bundle
    df = D.load_features_labels_local(str(feature_group[2]))
    crit = mmdx.DiseaseLoss(pos_weight=D.pos_weight_from_stats(D.label_stats(df)), gamma=2.0)
    out, path = _drive(feature_group, "with", criterion=crit, uncertain="ignore", val_rows=6)
    losses = out["image_loss"] + out["text_loss"] + [v for row in out["fusion_loss"]
                                                     for v in row[1:]]
    assert len(out["image_loss"]) == 2 and len(out["text_loss"]) == 6
    assert all(math.isfinite(v) for v in losses)
    assert out["val"]["n"] == 6 and math.isfinite(out["val"]["val_loss"])
    bundle = load_model_bundle(path)
    assert bundle["cfg"]["artifacts"]["loss"] == crit.config()
    assert bundle["cfg"]["artifacts"]["loss"]["gamma"] == 2.0
    pil = Image.open(os.path.join(GOLD, "e1.jpg")).convert("RGB")
    res = inference(bundle, pil, "44 year old female PA view , hypertension , cough",
                    gen_kwargs={"max_new_tokens": 4, "min_new_tokens": 1})
    assert len(res["disease_vector"]) == 13
    assert all(math.isfinite(res["disease_probs"][c]) for c in mmdx.DISEASES)


def test_driver_without_a_criterion_stores_no_loss_artifact(dev, feature_group):
    """The same call without criterion and uncertain, on the frame with complete labels (the
    plain loss has no way to leave a NaN label out)."""
    from mmdx.inference_pipeline import load_model_bundle
    out, path = _drive(feature_group, "without", complete=True)
    assert all(math.isfinite(v) for v in out["image_loss"] + out["text_loss"])
    arts = load_model_bundle(path)["cfg"]["artifacts"]
    assert "loss" not in arts
    assert sorted(arts) == ["class_names", "thresholds"]
