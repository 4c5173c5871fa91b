"""CPU: the float64 calibration reference (mmdx.calibration.reference_fit), the host math that
turns reliability bins into ECE / MCE / Brier, the calibration dict and its bundle round trip."""
import json
import math

import numpy as np
import pytest
import torch

from mmdx import calibration as K

from calibration_cases import FIT_CASES, make_case, sigmoid64


# ----------------------------------------------------------------------------- reference_fit
def test_reference_fit_recovers_a_known_map():
    """Logits (true_logit - b) / a with labels drawn from sigmoid(true_logit): the maximum
    likelihood estimate of (a, b) is asymptotically normal around the truth with covariance
    H^-1, H = sum p (1 - p) [[z^2, z], [z, 1]] at the truth.  Tolerance: 5 standard errors
    (a 5-sigma miss has probability < 1e-6 per parameter); Platt's target smoothing moves the
    optimum by O(1 / N), two orders below that."""
    rng = np.random.default_rng(5)
    N = 20000
    a = np.array([0.5, 1.0, 2.5])
    b = np.array([-2.0, 0.0, 1.5])
    true = rng.standard_normal((N, 3)) * 2.0 + np.array([-1.0, 0.0, 0.5])
    z = ((true - b) / a).astype(np.float32)
    y = (rng.random((N, 3)) < sigmoid64(true)).astype(np.float32)
    fit = K.reference_fit(z, y, "platt")
    assert fit["status"].tolist() == [0, 0, 0]
    for c in range(3):
        zc = z[:, c].astype(np.float64)
        p = sigmoid64(a[c] * zc + b[c])
        w = p * (1 - p)
        H = np.array([[np.sum(w * zc * zc), np.sum(w * zc)], [np.sum(w * zc), np.sum(w)]])
        se = np.sqrt(np.diag(np.linalg.inv(H)))
        assert abs(fit["scale"][c] - a[c]) <= 5 * se[0], (c, fit["scale"][c], se)
        assert abs(fit["bias"][c] - b[c]) <= 5 * se[1], (c, fit["bias"][c], se)
    # temperature: one slope, no bias
    z1 = (true / 1.7).astype(np.float32)
    y1 = (rng.random((N, 3)) < sigmoid64(true)).astype(np.float32)
    t = K.reference_fit(z1, y1, "temperature")
    assert t["status"].tolist() == [0, 0, 0] and t["bias"].tolist() == [0, 0, 0]
    assert len(set(t["scale"].tolist())) == 1
    zc = z1.astype(np.float64)
    p = sigmoid64(1.7 * zc)
    se = 1.0 / math.sqrt(np.sum(p * (1 - p) * zc * zc))
    assert abs(t["scale"][0] - 1.7) <= 5 * se


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_reference_fit_converges_on_every_fit_case(name, mode):
    """Status 0 within the default 32 iterations, at a stationary point: the gradient of the
    float64 objective, recomputed here, vanishes against its own scale."""
    z, y = make_case(*FIT_CASES[name])
    fit = K.reference_fit(z, y, mode)
    assert fit["status"].tolist() == [0] * z.shape[1]
    assert np.all(fit["scale"] > 0) and np.all(fit["info"][:, 1] <= fit["info"][:, 0])
    assert np.all(fit["info"][:, 2] <= 1e-7)
    m = ~np.isnan(y)
    y0 = np.where(m, y, 0).astype(np.float64)
    n_pos, n_neg = y0.sum(0), np.where(m, 1 - y0, 0).sum(0)
    t = 1 / (n_neg + 2) + y0 * ((n_pos + 1) / (n_pos + 2) - 1 / (n_neg + 2))
    z64 = z.astype(np.float64)
    d = np.where(m, sigmoid64(z64 * fit["raw_scale"] + fit["raw_bias"]) - t, 0.0)
    ga, gb = (d * z64).sum(0), d.sum(0)
    sa = np.abs(d * z64).sum(0)
    if mode == "temperature":
        assert abs(ga.sum()) <= 1e-6 * sa.sum()
    else:
        assert np.all(np.abs(ga) <= 1e-6 * sa) and np.all(np.abs(gb) <= 1e-6 * np.abs(d).sum(0))


def test_reference_fit_status_codes():
    z, y = make_case(*FIT_CASES["easy"])
    y[:, 3] = np.where(np.isnan(y[:, 3]), np.nan, 0.0)   # no positives
    y[:, 5] = np.nan                                      # nothing labelled
    y[:, 7] = np.where(np.isnan(y[:, 7]), np.nan, 1.0)   # no negatives
    fit = K.reference_fit(z, y)
    want = [0] * 13
    want[3] = want[5] = want[7] = K.STATUS_INACTIVE
    assert fit["status"].tolist() == want
    for c in (3, 5, 7):
        assert fit["scale"][c] == 1.0 and fit["bias"][c] == 0.0
    assert fit["info"][5, 3] == 0
    # min_count: a class with fewer positives than asked for is inactive
    n_pos = np.nansum(y, 0)
    fit = K.reference_fit(z, y, min_count=int(n_pos[0]) + 1)
    assert fit["status"][0] == K.STATUS_INACTIVE

    z, y = make_case(*FIT_CASES["far"])
    for mode in K.MODES:
        fit = K.reference_fit(z, y, mode, iters=2)
        assert fit["status"].tolist() == [K.STATUS_NOT_CONVERGED] * 13
        assert fit["scale"].tolist() == [1.0] * 13 and fit["bias"].tolist() == [0.0] * 13

    z, y = make_case((300, 13), 1.0, 0.0, 0.2, -1.0)     # anti-correlated
    for mode in K.MODES:
        fit = K.reference_fit(z, y, mode)
        assert fit["status"].tolist() == [K.STATUS_BAD_SLOPE] * 13
        assert np.all(fit["raw_scale"] < 0) and fit["scale"].tolist() == [1.0] * 13

    z, y = make_case(*FIT_CASES["easy"])
    z[0, 2] = np.nan                                      # a NaN logit under a label
    assert K.reference_fit(z, y)["status"][2] == K.STATUS_NOT_CONVERGED


def test_reference_fit_argument_errors():
    z, y = make_case((8, 3), 1, 0, 0.5, 1)
    with pytest.raises(ValueError):
        K.reference_fit(z, y, mode="isotonic")
    with pytest.raises(ValueError):
        K.reference_fit(z, y, iters=-1)
    with pytest.raises(ValueError):
        K.reference_fit(z, y, tol=0.0)
    with pytest.raises(ValueError):
        K.reference_fit(z, y[:, :2])
    with pytest.raises(ValueError):
        K.reference_fit(np.zeros((4, 65), np.float32), np.zeros((4, 65), np.float32))


# ----------------------------------------------------------------------------- bins -> numbers
def _direct(bins_row):
    cnt = bins_row[:, 0].astype(np.float64)
    pos = bins_row[:, 1].astype(np.float64)
    sp = bins_row[:, 2].astype(np.float64) / 2.0 ** 30
    sb = bins_row[:, 3].astype(np.float64) / 2.0 ** 30
    n = cnt.sum()
    ece = np.abs(sp - pos).sum() / n
    ne = cnt > 0
    mce = np.abs(sp[ne] / cnt[ne] - pos[ne] / cnt[ne]).max()
    return ece, mce, sb.sum() / n


def test_calibration_from_bins_against_direct_float64():
    one = K.FIXED_ONE
    bins = np.zeros((3, 4, 4), np.int64)
    # class 0: bins 0 and 2 filled, 1 and 3 empty
    bins[0, 0] = (10, 1, int(0.12 * one) * 10, int(0.05 * one) * 10)
    bins[0, 2] = (4, 3, int(0.6 * one) * 4, int(0.2 * one) * 4)
    # class 1: one element, a positive with p = 1
    bins[1, 3] = (1, 1, one, 0)
    bins[2] = bins[0] + bins[1]
    n_nan = np.array([2, 0, 2], np.int64)
    out = K.calibration_from_bins(bins, n_nan)
    assert out["n_bins"] == 4 and len(out["per_class"]) == 2
    for r, row in enumerate(out["per_class"] + [out["micro"]]):
        ece, mce, brier = _direct(bins[r])
        assert row["ece"] == pytest.approx(ece, rel=1e-15, abs=0)
        assert row["mce"] == pytest.approx(mce, rel=1e-15, abs=0)
        assert row["brier"] == pytest.approx(brier, rel=1e-15, abs=0)
        assert row["n"] == int(bins[r, :, 0].sum()) and row["n_nan"] == int(n_nan[r])
        assert row["count"] == bins[r, :, 0].tolist()
    c0 = out["per_class"][0]
    assert c0["mean_p"][1] is None and c0["frac_pos"][3] is None
    assert c0["frac_pos"][2] == 0.75 and c0["mean_p"][2] == int(0.6 * one) / one
    assert out["per_class"][1]["ece"] == 0.0 and out["per_class"][1]["brier"] == 0.0
    # hand value: |1.2 - 1| + |2.4 - 3| over 14 elements
    assert c0["ece"] == pytest.approx((abs(10 * int(0.12 * one) / one - 1)
                                       + abs(4 * int(0.6 * one) / one - 3)) / 14, rel=1e-14)

    # a single bin
    one_bin = np.array([[[5, 2, 3 * one, one]], [[5, 2, 3 * one, one]]], np.int64)
    out = K.calibration_from_bins(torch.from_numpy(one_bin), torch.zeros(2, dtype=torch.int64))
    assert out["micro"]["ece"] == pytest.approx(0.2, rel=1e-15)   # |3 - 2| / 5
    assert out["micro"]["mce"] == pytest.approx(0.2, rel=1e-15)   # |3 / 5 - 2 / 5|
    assert out["micro"]["brier"] == pytest.approx(0.2)

    # all NaN: nothing counted
    out = K.calibration_from_bins(np.zeros((2, 15, 4), np.int64), np.array([7, 7]))
    for row in (out["per_class"][0], out["micro"]):
        assert row["n"] == 0 and row["n_nan"] == 7
        assert all(math.isnan(row[k]) for k in ("ece", "mce", "brier"))
        assert row["mean_p"] == [None] * 15

    with pytest.raises(ValueError):
        K.calibration_from_bins(np.zeros((2, 15, 3), np.int64), np.zeros(2, np.int64))
    with pytest.raises(ValueError):
        K.calibration_from_bins(np.zeros((2, 15, 4), np.int64), np.zeros(3, np.int64))


def test_bin_edges():
    assert K.bin_edges(1).shape == (0,)
    e = K.bin_edges(4)
    assert e.dtype == np.float32 and e[1] == 0.0
    assert np.allclose(e, np.log(np.array([0.25, 0.5, 0.75]) / np.array([0.75, 0.5, 0.25])))
    assert len(K.bin_edges(64)) == 63 and np.all(np.diff(K.bin_edges(64)) > 0)
    for bad in (0, 65, 2.0, True, None):
        with pytest.raises(ValueError):
            K.bin_edges(bad)


def test_training_tests_calibrate_needs_held_out_rows():
    """Checked before anything is loaded or launched."""
    from mmdx.training_driver import training_tests
    with pytest.raises(ValueError, match="val_rows"):
        training_tests(calibrate="platt")
    with pytest.raises(ValueError, match="calibrate"):
        training_tests(calibrate="isotonic", val_rows=4)


# ----------------------------------------------------------------------------- the dict
def test_check_calibration_errors():
    good = {"mode": "platt", "scale": [1.0, 2.0], "bias": [0.0, -1.0]}
    assert K.check_calibration(good, 2) == ([1.0, 2.0], [0.0, -1.0])
    assert K.check_calibration(K.identity(3, "temperature"), 3) == ([1.0] * 3, [0.0] * 3)
    bad = [
        ["not", "a", "dict"],
        {"mode": "platt", "scale": [1.0, 2.0]},                              # no bias
        dict(good, mode="isotonic"),
        dict(good, scale=[1.0]),                                             # wrong length
        dict(good, bias=[0.0, 0.0, 0.0]),
        dict(good, scale=[1.0, float("nan")]),
        dict(good, bias=[0.0, float("inf")]),
        dict(good, scale=[1.0, 0.0]),                                        # not monotone
        dict(good, scale=[1.0, -2.0]),
        dict(good, scale=["a", "b"]),
        dict(good, scale=3.0),
        dict(good, mode="temperature"),                                      # two slopes, a bias
    ]
    for d in bad:
        with pytest.raises(ValueError):
            K.check_calibration(d, 2)
    with pytest.raises(ValueError):
        K.check_calibration(good, 3)


def test_apply_is_a_multiply_and_an_add_in_float32():
    rng = np.random.default_rng(2)
    z = rng.standard_normal((7, 3)).astype(np.float32) * 5
    cal = {"mode": "platt", "scale": [0.3, 1.7, 1.0], "bias": [-2.2, 0.4, 0.0]}
    s, b = np.array(cal["scale"], np.float32), np.array(cal["bias"], np.float32)
    want = (z * s).astype(np.float32) + b
    assert np.array_equal(K.apply(z, cal), want)
    got = K.apply(torch.from_numpy(z), cal)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert np.array_equal(K.apply(z, K.identity(3)), z)


def test_dict_round_trip_through_bundle_config_and_json():
    from mmdx.inference_pipeline import bundle_config
    scale = torch.tensor([0.1, 1.25, 3.0000002], dtype=torch.float32)
    bias = torch.tensor([-2.5, 0.0, 1e-3], dtype=torch.float32)
    d = K.to_dict("platt", scale, bias, status=torch.tensor([0, 0, 1], dtype=torch.int32))
    assert d["status"] == [0, 0, 1] and d["mode"] == "platt"
    cfg = bundle_config(object(), object(), object(),
                        artifacts={"thresholds": [0.5] * 3, "calibration": d})
    back = json.loads(json.dumps(cfg))["artifacts"]["calibration"]
    assert back == d
    s2, b2 = K.from_dict(back, 3)
    assert s2.dtype == torch.float32 and torch.equal(s2, scale) and torch.equal(b2, bias)
    with pytest.raises(ValueError):
        K.to_dict("platt", [1.0, -1.0], [0.0, 0.0])
    with pytest.raises(ValueError):
        K.from_dict(back, 4)
