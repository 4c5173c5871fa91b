"""CPU: the definition of the disease loss (mmdx.losses.reference, float64) against torch's own
losses and autograd, the label helpers of mmdx.data, and the argument checks, which are all made
on the host before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import mmdx
import mmdx.functional as F
from mmdx import data as D
from mmdx import losses as LS

NAN = float("nan")


def _case(B=37, C=13, seed=0, soft=True, nan=True):
    g = torch.Generator().manual_seed(seed)
    z = (4.0 * torch.randn(B, C, generator=g)).double()
    y = (torch.rand(B, C, generator=g) < 0.2).float()
    if soft:
        s = torch.rand(B, C, generator=g)
        y = torch.where(torch.rand(B, C, generator=g) < 0.1, s, y)
    if nan:
        y = torch.where(torch.rand(B, C, generator=g) < 0.15, torch.full_like(y, NAN), y)
    pw = (0.5 + 5.0 * torch.rand(C, generator=g)).double()
    cw = (0.5 + torch.rand(C, generator=g)).double()
    return z, y, pw, cw


# ----------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_reference_is_weighted_bce_at_gamma_zero(reduction):
    z, y, pw, cw = _case()
    m = ~torch.isnan(y)
    y0 = torch.where(m, y, torch.zeros_like(y)).double()
    w = cw * m.double()
    want = torch.nn.functional.binary_cross_entropy_with_logits(
        z, y0, weight=w.expand_as(z), pos_weight=pw, reduction="sum")
    if reduction == "mean":
        want = want / m.sum()
    got, stats = LS.reference(z, y, pw, cw, 0.0, 0.0, reduction)
    assert got.dtype == torch.float64
    assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())
    assert torch.equal(stats[:, 1], m.double().sum(0))
    assert abs(stats[:, 0].sum().item() - (want * (m.sum() if reduction == "mean" else 1)).item()) \
        <= 1e-9


@pytest.mark.parametrize("gamma", [1.0, 2.0, 3.5])
def test_reference_is_alpha_focal_loss_for_hard_labels(gamma):
    z, y, _, _ = _case(soft=False, nan=False)
    alpha = 0.25
    C = z.shape[1]
    cw = torch.full((C,), 1.0 - alpha, dtype=torch.float64)
    pw = torch.full((C,), alpha / (1.0 - alpha), dtype=torch.float64)
    yd = y.double()
    p = torch.sigmoid(z)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(z, yd, reduction="none")
    p_t = p * yd + (1 - p) * (1 - yd)
    a_t = alpha * yd + (1 - alpha) * (1 - yd)
    want = (a_t * (1 - p_t) ** gamma * ce).sum()
    got, _ = LS.reference(z, y, pw, cw, gamma, 0.0, "sum")
    assert abs(got.item() - want.item()) <= 1e-12 * abs(want.item())


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0, 3.5])
def test_closed_form_gradient_is_autograd(gamma, eps):
    z, y, pw, cw = _case(seed=3)
    z = z.clone().requires_grad_(True)
    loss, _ = LS.reference(z, y, pw, cw, gamma, eps, "sum")
    loss.backward()
    g = LS.reference_grad(z.detach(), y, pw, cw, gamma, eps)
    assert (g - z.grad).abs().max().item() <= 1e-13
    assert torch.equal(g[torch.isnan(y)], torch.zeros_like(g[torch.isnan(y)]))


def test_label_smoothing_and_nan_masking_as_defined():
    z = torch.tensor([[0.3, -1.2, 2.0]], dtype=torch.float64)
    y = torch.tensor([[1.0, NAN, 0.0]])
    eps = 0.1
    got, stats = LS.reference(z, y, None, None, 0.0, eps, "mean")
    sp = torch.nn.functional.softplus
    e0 = 0.95 * sp(-z[0, 0]) + 0.05 * sp(z[0, 0])          # y' = 1 * 0.9 + 0.05
    e2 = 0.05 * sp(-z[0, 2]) + 0.95 * sp(z[0, 2])          # y' = 0.05
    assert abs(got.item() - ((e0 + e2) / 2).item()) <= 1e-15
    assert stats[1].tolist() == [0.0, 0.0]
    assert stats[:, 1].tolist() == [1.0, 0.0, 1.0]
    # the ignored logit does not matter
    z2 = z.clone()
    z2[0, 1] = 1e4
    assert LS.reference(z2, y, None, None, 2.0, eps)[0] == LS.reference(z, y, None, None, 2.0,
                                                                       eps)[0]


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_all_ignored_batch_is_zero_loss_and_zero_gradient(gamma):
    z = torch.randn(4, 5, dtype=torch.float64, requires_grad=True)
    y = torch.full((4, 5), NAN)
    for reduction in ("mean", "sum"):
        loss, stats = LS.reference(z, y, None, None, gamma, 0.0, reduction)
        assert loss.item() == 0.0 and not stats.any()
        (g,) = torch.autograd.grad(loss, z)
        assert not g.any() and not torch.isnan(g).any()


def test_reference_is_finite_at_extreme_logits():
    z = torch.tensor([[20.0, -88.0, 1e4, -1e4, 3e38, -3e38, 0.0]], dtype=torch.float64)
    for lab in (0.0, 1.0, 0.3):
        y = torch.full((1, 7), lab)
        for gamma in (0.0, 2.0):
            loss, _ = LS.reference(z, y, None, None, gamma)
            assert torch.isfinite(loss)
            assert torch.isfinite(LS.reference_grad(z, y, None, None, gamma)).all()


# ----------------------------------------------------------------------------- label helpers
def test_apply_uncertain_policies():
    a = np.array([[1.0, -1.0, NAN, 0.0], [0.25, 1.0, -1.0, -1.0]], dtype=np.float32)
    keep = a.copy()
    assert D.apply_uncertain(a, None) is a
    lst = [[1.0, -1.0]]
    assert D.apply_uncertain(lst, None) is lst
    for policy, fill in (("ignore", NAN), ("zeros", 0.0), ("ones", 1.0), (0.3, 0.3)):
        got = D.apply_uncertain(a, policy)
        want = keep.copy()
        want[keep == -1.0] = fill
        assert got.dtype == np.float32 and got is not a
        assert np.array_equal(got, want.astype(np.float32), equal_nan=True)
        assert np.isnan(got[0, 2])                      # NaN stays NaN under every policy
    assert np.array_equal(a, keep, equal_nan=True)      # the input is left alone


def test_apply_uncertain_errors():
    a = np.zeros((3, 4), dtype=np.float32)
    a[2, 1] = 2.0
    with pytest.raises(ValueError, match=r"row 2, class 1"):
        D.apply_uncertain(a, "ignore")
    a[2, 1] = -0.5
    with pytest.raises(ValueError, match=r"row 2, class 1"):
        D.apply_uncertain(a, "zeros")
    a[2, 1] = np.inf
    with pytest.raises(ValueError, match=r"row 2, class 1"):
        D.apply_uncertain(a, 0.5)
    ok = np.zeros((2, 2), dtype=np.float32)
    for policy in ("drop", 0.0, 1.0, 1.5, True, [0.5]):
        with pytest.raises(ValueError):
            D.apply_uncertain(ok, policy)
    assert D.apply_uncertain(a, None) is a              # None checks nothing


def test_label_stats_and_pos_weight_on_a_hand_written_frame():
    import pandas as pd
    rows = [[1, 0, 0, -1], [0, 0, NAN, 1], [1, 0, -1, 0], [0, 0, 0, 0], [0, 0, 0, 0],
            [0, 0, 1, 0]]
    df = pd.DataFrame({"disease_classification_vector": [np.asarray(r, dtype=float)
                                                         for r in rows]})
    for src in (df, np.asarray(rows, dtype=np.float32), rows):
        st = D.label_stats(src)
        assert st["n"] == 6
        assert st["n_pos"].tolist() == [2, 0, 1, 1]
        assert st["n_neg"].tolist() == [4, 6, 3, 4]
        assert st["n_uncertain"].tolist() == [0, 0, 1, 1]
        assert st["n_missing"].tolist() == [0, 0, 1, 0]
        assert all(st[k].dtype == np.int64 for k in ("n_pos", "n_neg", "n_uncertain",
                                                      "n_missing"))
    pw = D.pos_weight_from_stats(st, cap=3.5)
    assert pw.dtype == np.float32
    assert pw.tolist() == [2.0, 1.0, 3.0, 3.5]          # no positives -> 1; 4 / 1 capped
    assert D.pos_weight_from_stats(st, cap=100.0).tolist() == [2.0, 1.0, 3.0, 4.0]
    with pytest.raises(ValueError):
        D.pos_weight_from_stats(st, cap=0.0)


# ----------------------------------------------------------------------------- argument checks
BAD = [
    (dict(gamma=0.5), ValueError),
    (dict(gamma=-1.0), ValueError),
    (dict(gamma=float("inf")), ValueError),
    (dict(label_smoothing=1.0), ValueError),
    (dict(label_smoothing=-0.1), ValueError),
    (dict(reduction="none"), ValueError),
    (dict(pos_weight=[1.0] * 12 + [-0.5]), ValueError),
    (dict(class_weight=[1.0] * 12 + [float("inf")]), ValueError),
    (dict(pos_weight=[1.0] * 12 + [NAN]), ValueError),
]


@pytest.mark.parametrize("kw,exc", BAD)
def test_criterion_rejects_bad_arguments_on_the_host(kw, exc):
    with pytest.raises(exc):
        mmdx.DiseaseLoss(**kw)


@pytest.mark.parametrize("kw,exc", BAD + [(dict(pos_weight=[1.0] * 12), ValueError),
                                          (dict(class_weight=[1.0] * 14), ValueError)])
def test_functional_rejects_bad_arguments_without_a_device(kw, exc):
    """CPU tensors throughout: every one of these is raised before the device is looked at."""
    kw = {k: (torch.tensor(v, dtype=torch.float32) if isinstance(v, list) else v)
          for k, v in kw.items()}
    z, y = torch.zeros(4, 13), torch.zeros(4, 13)
    with pytest.raises(exc):
        F.disease_loss(z, y, **kw)


def test_functional_rejects_bad_tensors_without_a_device():
    z, y = torch.zeros(4, 13), torch.zeros(4, 13)
    with pytest.raises(TypeError):
        F.disease_loss(z, y, pos_weight=[1.0] * 13)                 # not a tensor
    with pytest.raises(TypeError):
        F.disease_loss(z, y, pos_weight=torch.ones(13, dtype=torch.float64))
    with pytest.raises(TypeError):
        F.disease_loss(z.double(), y)
    with pytest.raises(TypeError):
        F.disease_loss(z, y.double())
    with pytest.raises(ValueError):
        F.disease_loss(z, y[:3])
    with pytest.raises(ValueError):
        F.disease_loss(torch.zeros(2, 65), torch.zeros(2, 65))
    with pytest.raises(ValueError):
        F.disease_loss(torch.zeros(13, 4).t(), y)                   # not contiguous
    with pytest.raises(ValueError, match="GPU"):
        F.disease_loss(z, y)                                        # a host tensor: no CPU path


def test_criterion_length_mismatch_and_config():
    crit = mmdx.DiseaseLoss(pos_weight=np.full(13, 2.0, dtype=np.float32),
                            class_weight=[0.5] * 13, gamma=2.0, label_smoothing=0.1)
    cfg = crit.config()
    assert cfg == {"name": "DiseaseLoss", "pos_weight": [2.0] * 13, "class_weight": [0.5] * 13,
                   "gamma": 2.0, "label_smoothing": 0.1, "reduction": "mean"}
    import json
    assert json.loads(json.dumps(cfg)) == cfg
    assert mmdx.DiseaseLoss().config()["pos_weight"] is None
    with pytest.raises(ValueError):
        mmdx.DiseaseLoss(pos_weight=[1.0] * 13, class_weight=[1.0] * 12)
    with pytest.raises(ValueError):
        crit(torch.zeros(4, 12), torch.zeros(4, 12))                # 13 weights, 12 classes
    with pytest.raises(ValueError):
        mmdx.DiseaseLoss(pos_weight=[1.0] * 65)


# ----------------------------------------------------------------------------- the C ABI
def test_entry_points_reject_bad_arguments_before_any_launch():
    """Argument errors are decided on the host: fake, never dereferenced pointers."""
    import mmdx._lib as L
    lib = L.lib()
    ws = lib.mmdx_disease_loss_workspace_size
    assert ws(128, 13) == 16 + 1 * 13 * 8                 # one block: 247 threads x 8 elements
    assert ws(153, 13) == 16 + 2 * 13 * 8                 # 1989 elements > 1976
    assert ws(2048, 1) == 16 + 8 and ws(2049, 1) == 16 + 2 * 8
    assert ws(1 << 24, 13) == 16 + 1024 * 13 * 8          # the grid is capped
    for B, C in ((0, 13), (4, 0), (4, 65), ((1 << 31) // 13 + 1, 13)):
        assert ws(B, C) == 0
    p = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]

    def fwd(B=4, C=13, gamma=0.0, eps=0.0, logits=p[0], target=p[1], loss=p[2], stats=p[3],
            norm=p[4], g=p[5], wsp=p[6], nbytes=1 << 20, dtype=L.F32):
        return lib.mmdx_disease_loss_fwd(dtype, logits, target, B, C, None, None, gamma, eps, 1,
                                         loss, stats, norm, g, wsp, nbytes, None)
    for kw in (dict(C=65), dict(B=(1 << 31) // 13 + 1), dict(B=0), dict(gamma=0.5),
               dict(eps=1.0), dict(logits=None), dict(target=None), dict(loss=None),
               dict(stats=None), dict(norm=None), dict(wsp=None), dict(nbytes=8),
               dict(g=p[0]), dict(loss=p[1]), dict(stats=p[4]), dict(dtype=7),
               dict(wsp=ctypes.c_void_p(0x7004))):
        assert fwd(**kw) == -22, kw
        assert b"disease_loss" in lib.mmdx_last_error()
    assert lib.mmdx_disease_loss_bwd(L.F32, None, 4, None, p[1], p[2], None) == -22
    assert lib.mmdx_disease_loss_bwd(L.F32, p[0], 0, None, p[1], p[2], None) == -22
    assert lib.mmdx_disease_loss_bwd(L.F32, p[0], 4, None, p[1], p[0], None) == -22
