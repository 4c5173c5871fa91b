"""GPU: the calibration kernels against their CPU statements, evaluate(calibrate=...) on a small
model and the bundle round trip through inference().

- reliability bins (mmdx_reliability_bins) vs np.searchsorted on float32 z' (multiply, then
  add): zero tolerance on the counts; the fixed-point sums vs float64 within the bound derived
  below.
- the fit (mmdx_calib_fit_step x (iters + 1)) vs mmdx.calibration.reference_fit (float64):
  calibrated probabilities within 1e-4 on the case's own logits.

The measured figures go to profiles/calibration_parity.txt.
"""
import math
import os

import numpy as np
import pytest
import torch

import mmdx
import mmdx.functional as F
from mmdx import calibration as K
from mmdx import metrics as M

from calibration_cases import FIT_CASES, make_case, ref_bins, sigmoid64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

SHAPES = [(n, c) for n in (1, 2, 63, 257, 1000) for c in (1, 13, 64)] + [(4099, 13)]


@pytest.fixture(scope="module")
def parity():
    """Collects the measured figures; written to profiles/calibration_parity.txt at the end."""
    rows = {}
    yield rows
    if not rows:
        return
    lines = ["# measured by tests/test_calibration_gpu.py on the GPU (gfx950); bounds in the tests",
             f"# device: {torch.cuda.get_device_name(0)}"]
    lines += [f"{k}: {rows[k]}" for k in sorted(rows)]
    try:
        with open(os.path.join(ROOT, "profiles", "calibration_parity.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:   # a read-only checkout still runs the assertions
        pass


def _bin_inputs(N, C, n_bins, seed):
    """randn rounded to 1 / 8, with +-inf, NaN, +-0 and the fp32 bin edges themselves mixed in."""
    rng = np.random.default_rng(seed)
    z = (np.round(rng.standard_normal((N, C)) * 8 * 2) / 8).astype(np.float32)
    special = np.concatenate([np.array([np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32),
                              K.bin_edges(n_bins)])
    hit = rng.random((N, C)) < 0.25
    z[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    y = (rng.random((N, C)) < 0.3).astype(np.float32)
    return z, y


# ----------------------------------------------------------------------------- reliability bins
@pytest.mark.parametrize("n_bins", [1, 15, 64])
def test_reliability_bins_match_numpy(dev, parity, n_bins):
    """count, positives and n_nan: exact.  sum p within count * 2^-20 and sum (p - y)^2 within
    count * 2^-19 of float64: expf is within 1 ulp, then one add and one correctly rounded
    divide, so p <= 1 carries at most 3 ulp = 3 * 2^-24 < 2^-22, plus 2^-31 of the fixed-point
    rounding: under half of 2^-20; the square has derivative <= 2."""
    edges = K.bin_edges(n_bins)
    worst_p = worst_b = 0.0
    for i, (N, C) in enumerate(SHAPES):
        z, y = _bin_inputs(N, C, n_bins, 100 * n_bins + i)
        zd, yd = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
        rng = np.random.default_rng(i)
        scale = (0.25 + rng.random(C) * 2).astype(np.float32)
        bias = rng.standard_normal(C).astype(np.float32)
        for sb in (None, (scale, bias)):
            if sb is None:
                bins, n_nan = F.reliability_bins(zd, yd, n_bins=n_bins)
                cnt, pos, nn, sp, sq = ref_bins(z, y, edges)
            else:
                bins, n_nan = F.reliability_bins(zd, yd, torch.from_numpy(scale).to(dev),
                                                 torch.from_numpy(bias).to(dev), n_bins=n_bins)
                cnt, pos, nn, sp, sq = ref_bins(z, y, edges, scale, bias)
            bins, n_nan = bins.cpu().numpy(), n_nan.cpu().numpy()
            tag = (N, C, n_bins, sb is not None)
            assert bins.shape == (C + 1, n_bins, 4) and n_nan.shape == (C + 1,)
            assert np.array_equal(bins[:, :, 0], cnt), tag
            assert np.array_equal(bins[:, :, 1], pos), tag
            assert np.array_equal(n_nan, nn), tag
            ep = np.abs(bins[:, :, 2] / 2.0 ** 30 - sp)
            eb = np.abs(bins[:, :, 3] / 2.0 ** 30 - sq)
            ne = cnt > 0
            if ne.any():
                worst_p = max(worst_p, float((ep[ne] / cnt[ne]).max()))
                worst_b = max(worst_b, float((eb[ne] / cnt[ne]).max()))
            assert np.all(ep <= cnt * 2.0 ** -20), tag
            assert np.all(eb <= cnt * 2.0 ** -19), tag
    parity[f"reliability_bins n_bins={n_bins:2d} max |sum p - f64| / count"] = \
        f"{worst_p:.3e} (bound {2.0 ** -20:.3e})"
    parity[f"reliability_bins n_bins={n_bins:2d} max |sum (p-y)^2 - f64| / count"] = \
        f"{worst_b:.3e} (bound {2.0 ** -19:.3e})"


def test_reliability_bins_are_reproducible(dev):
    z, y = _bin_inputs(4099, 13, 15, 7)
    zd, yd = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
    a = [t.cpu().numpy().tobytes() for t in F.reliability_bins(zd, yd)]
    b = [t.cpu().numpy().tobytes() for t in F.reliability_bins(zd, yd)]
    assert a == b


# ----------------------------------------------------------------------------- the fit
@pytest.fixture(scope="module")
def fit_refs():
    """reference_fit of every case and mode, computed once."""
    out = {}
    for name, spec in FIT_CASES.items():
        z, y = make_case(*spec)
        for mode in K.MODES:
            out[name, mode] = (z, y, K.reference_fit(z, y, mode))
    return out


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_calib_fit_matches_the_float64_reference(dev, parity, fit_refs, name, mode):
    """Status 0 and calibrated probabilities within 1e-4 of the float64 optimum over the case's
    logits (a user reads four decimals; the CPU emulation of the kernel's arithmetic, fp32
    element terms and fp64 sums, is within 1.6e-5)."""
    z, y, ref = fit_refs[name, mode]
    assert ref["status"].tolist() == [0] * z.shape[1]
    scale, bias, status, info = F.calib_fit(torch.from_numpy(z).to(dev),
                                            torch.from_numpy(y).to(dev), mode=mode)
    scale, bias = scale.cpu().numpy(), bias.cpu().numpy()
    status, info = status.cpu().numpy(), info.cpu().numpy()
    z64 = z.astype(np.float64)
    gap = np.abs(sigmoid64(z64 * scale.astype(np.float64) + bias.astype(np.float64))
                 - sigmoid64(z64 * ref["raw_scale"] + ref["raw_bias"])).max()
    da = np.abs(scale - ref["raw_scale"]).max()
    db = np.abs(bias - ref["raw_bias"]).max()
    excess = (info[:, 1] - ref["info"][:, 1]).max()
    parity[f"calib_fit {name:5s} {mode:11s}"] = (
        f"|da| {da:.3e} |db| {db:.3e} prob gap {gap:.3e} NLL excess {excess:.3e} "
        f"decrement {info[:, 2].max():.3e} status {sorted(set(status.tolist()))}")
    print(name, mode, parity[f"calib_fit {name:5s} {mode:11s}"])
    assert status.tolist() == [0] * z.shape[1]
    assert gap <= 1e-4
    assert np.array_equal(info[:, 3], ref["info"][:, 3])       # labelled counts: exact
    assert np.allclose(info[:, 0], ref["info"][:, 0], rtol=1e-6)  # NLL at the identity
    if mode == "temperature":
        assert len(set(scale.tolist())) == 1 and not bias.any()


def _fit_host(dev, z, y, **kw):
    return [t.cpu().numpy() for t in F.calib_fit(torch.from_numpy(z).to(dev),
                                                 torch.from_numpy(y).to(dev), **kw)]


def test_calib_fit_statuses_and_identity(dev):
    z, y = make_case(*FIT_CASES["easy"])
    y[:, 3] = np.where(np.isnan(y[:, 3]), np.nan, 0.0)   # no positives
    y[:, 5] = np.nan                                      # nothing labelled
    scale, bias, status, info = _fit_host(dev, z, y)
    want = [0] * 13
    want[3] = want[5] = K.STATUS_INACTIVE
    assert status.tolist() == want == K.reference_fit(z, y)["status"].tolist()
    assert scale[3] == scale[5] == 1.0 and bias[3] == bias[5] == 0.0 and info[5, 3] == 0

    z, y = make_case(*FIT_CASES["far"])
    for mode in K.MODES:
        scale, bias, status, _ = _fit_host(dev, z, y, mode=mode, iters=2)
        assert status.tolist() == [K.STATUS_NOT_CONVERGED] * 13
        assert scale.tolist() == [1.0] * 13 and bias.tolist() == [0.0] * 13

    z, y = make_case((300, 13), 1.0, 0.0, 0.2, -1.0)     # anti-correlated
    for mode in K.MODES:
        scale, bias, status, _ = _fit_host(dev, z, y, mode=mode)
        assert status.tolist() == [K.STATUS_BAD_SLOPE] * 13
        assert scale.tolist() == [1.0] * 13 and bias.tolist() == [0.0] * 13


def test_calib_fit_is_bit_reproducible(dev):
    """More than one block (4096 x 13 elements: 27 blocks), both modes: identical bytes."""
    z, y = make_case(*FIT_CASES["big"])
    for mode in K.MODES:
        a = [t.tobytes() for t in _fit_host(dev, z, y, mode=mode)]
        b = [t.tobytes() for t in _fit_host(dev, z, y, mode=mode)]
        assert a == b


def test_calib_fit_evaluation_pass_is_the_plain_nll(dev):
    """iters = 0, smooth = False: info[:, 0] is the BCE sum of the labelled elements."""
    z, y = make_case(*FIT_CASES["big"])
    _, _, _, info = _fit_host(dev, z, y, iters=0, smooth=False)
    m = ~np.isnan(y)
    z64 = z.astype(np.float64)
    nll = np.where(m, np.maximum(z64, 0) + np.log1p(np.exp(-np.abs(z64)))
                   - np.where(m, y, 0) * z64, 0.0).sum(0)
    assert np.allclose(info[:, 0], nll, rtol=1e-6) and np.array_equal(info[:, 0], info[:, 1])
    assert np.array_equal(info[:, 3], m.sum(0).astype(np.float64))


def test_argument_errors_come_before_any_launch(dev):
    z = torch.zeros(8, 3, device=dev)
    y = torch.zeros(8, 3, device=dev)
    for fn in (F.calib_fit, F.reliability_bins):
        with pytest.raises(TypeError):
            fn(z.double(), y)
        with pytest.raises(TypeError):
            fn(z, y.half())
        with pytest.raises(TypeError):
            fn(z.cpu().numpy(), y)
        with pytest.raises(ValueError):
            fn(z, y[:, :2])
        with pytest.raises(ValueError):
            fn(z.reshape(-1), y.reshape(-1))
        with pytest.raises(ValueError):
            fn(z.cpu(), y.cpu())
        with pytest.raises(ValueError):
            fn(z, y.cpu())
        with pytest.raises(ValueError):
            fn(z.t(), y.t())                                   # not contiguous
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 65, device=dev), torch.zeros(2, 65, device=dev))
    for bad in (0, 65, 15.0, None):
        with pytest.raises(ValueError):
            F.reliability_bins(z, y, n_bins=bad)
    with pytest.raises(ValueError):
        F.reliability_bins(z, y, scale=torch.ones(3, device=dev))          # no bias
    with pytest.raises(ValueError):
        F.reliability_bins(z, y, torch.ones(4, device=dev), torch.zeros(4, device=dev))
    with pytest.raises(TypeError):
        F.reliability_bins(z, y, torch.ones(3, device=dev).double(), torch.zeros(3, device=dev))
    with pytest.raises(ValueError):
        F.reliability_bins(z, y, torch.ones(3), torch.zeros(3))           # on the host
    for kw in (dict(mode="isotonic"), dict(iters=-1), dict(iters=1.5), dict(min_count=-1),
               dict(tol=0.0), dict(tol=float("nan"))):
        with pytest.raises(ValueError):
            F.calib_fit(z, y, **kw)
    # the C entry points reject what the wrappers cannot express
    with pytest.raises(RuntimeError, match="mode"):
        mmdx._lib.call("mmdx_calib_fit_step", z.data_ptr(), y.data_ptr(), 8, 3, z.data_ptr(), 1,
                       7, 0, 1, 1, 1e-7, None, None, None, None, None, 0, 0)
    with pytest.raises(RuntimeError, match="workspace"):
        mmdx._lib.call("mmdx_calib_fit_step", z.data_ptr(), y.data_ptr(), 8, 3, z.data_ptr(), 1,
                       1, 0, 0, 1, 1e-7, None, None, None, None, None, 0, 0)
    assert mmdx._lib.lib().mmdx_calib_fit_workspace_size(8, 65) == 0


# ----------------------------------------------------------------------------- evaluate()
KEYS = {"n", "val_loss", "val_auroc_micro", "val_auroc_macro", "val_auroc_per_class",
        "thresholds", "val_f1_micro", "val_f1_micro_at_0p5", "per_class"}


@pytest.fixture(scope="module")
def small_model(dev):
    """The small model of tests/test_metrics_gpu.py with 48 rows; the labels are drawn from a
    shifted and rescaled copy of the model's own logits z, with a few labels ignored (NaN), so
    the raw probabilities are wrong by construction and a Platt map can repair them."""
    torch.manual_seed(0)
    img = mmdx.ImageEncoderCNN("resnet18", 1024, 13).to(dev).eval()
    txt = mmdx.TextEncoderTransformer("bert-base-uncased@2", 512, 13).to(dev).eval()
    fus = mmdx.FusionTransformerModel(1024, 512, 1024, 13).to(dev).eval()
    g = torch.Generator().manual_seed(11)
    n = 48
    x = torch.randn(n, 3, 64, 64, generator=g)
    details = [f"{30 + i} year old {'male' if i % 2 else 'female'} PA view, "
               f"{'cough' if i % 3 else 'fever'}, case {i}" for i in range(n)]
    zs = []
    with torch.no_grad():
        for s in range(0, n, 16):
            tok = {k: v.to(dev) for k, v in
                   mmdx.tokenize_patient_details(details[s:s + 16], max_len=96).items()}
            z_img = img(x[s:s + 16].to(dev))["embeddings"]
            z_txt = txt(**tok)["embeddings"]
            zs.append(fus(z_img=z_img, z_txt=z_txt)["disease_logits"].float())
    z = torch.cat(zs)
    # an untrained head's logits barely move from row to row: standardise them per class so
    # that the labels depend on them (a true map with a large positive slope and a shift)
    zc = z.cpu()
    true = 2.0 * (zc - zc.mean(0)) / zc.std(0) - 1.5
    y = (torch.rand(n, 13, generator=g) < torch.sigmoid(true)).float()
    y[torch.rand(n, 13, generator=g) < 0.05] = math.nan
    batches = [(x[s:s + 16].to(dev), details[s:s + 16], y[s:s + 16].to(dev))
               for s in range(0, n, 16)]
    return img, txt, fus, batches, z, y.to(dev)


def test_evaluate_without_calibrate_is_unchanged(dev, small_model):
    img, txt, fus, batches, _, _ = small_model
    crit = mmdx.DiseaseLoss()
    a = M.evaluate(img, txt, fus, batches, criterion=crit)
    b = M.evaluate(img, txt, fus, batches, criterion=crit, calibrate=None)
    assert set(a) == set(b) == KEYS
    assert repr(a) == repr(b)      # equal values, NaN included


def test_evaluate_calibrate_platt(dev, small_model):
    img, txt, fus, batches, z, y = small_model
    crit = mmdx.DiseaseLoss()
    raw = M.evaluate(img, txt, fus, batches, criterion=crit)
    res = M.evaluate(img, txt, fus, batches, criterion=crit, calibrate="platt")
    assert set(res) == KEYS | {"calibration"}
    cal = res["calibration"]

    # the fitted dict is functional.calib_fit on the same buffers
    scale, bias, status, _ = F.calib_fit(z.contiguous(), y.contiguous(), mode="platt")
    assert cal["mode"] == "platt" and cal["n_bins"] == 15
    assert cal["scale"] == scale.cpu().tolist() and cal["bias"] == bias.cpu().tolist()
    assert cal["status"] == status.cpu().tolist() == [0] * 13

    # ranking is untouched; the loss is the raw logits'
    for k in ("val_auroc_micro", "val_auroc_macro", "val_auroc_per_class", "val_loss", "n"):
        assert repr(res[k]) == repr(raw[k]), k

    # the bins are the kernel's on the same buffers, ignored labels left out
    ign = torch.isnan(y)
    zm = torch.where(ign, torch.full_like(z, math.nan), z)
    ym = torch.where(ign, torch.zeros_like(y), y)
    bins, _ = F.reliability_bins(zm, ym, scale, bias)
    want = K.calibration_from_bins(bins.cpu().numpy(), np.zeros(14, np.int64))
    assert cal["after"]["val_ece_micro"] == want["micro"]["ece"]
    assert cal["after"]["val_brier_per_class"] == [r["brier"] for r in want["per_class"]]
    assert cal["after"]["reliability"]["micro"]["count"] == want["micro"]["count"]
    assert sum(want["micro"]["count"]) == int((~ign).sum())

    # labels drawn from shifted logits: the map repairs the probabilities (in-sample)
    before, after = cal["before"], cal["after"]
    assert after["val_ece_micro"] < before["val_ece_micro"]
    assert after["val_nll_micro"] <= before["val_nll_micro"]
    assert after["val_brier_micro"] < before["val_brier_micro"]
    for side in (before, after):
        assert len(side["val_ece_per_class"]) == len(side["val_nll_per_class"]) == 13
        assert len(side["reliability"]["per_class"]) == 13
        assert len(side["reliability"]["micro"]["mean_p"]) == 15
    z64, y64 = z.double().cpu().numpy(), y.double().cpu().numpy()
    lab = ~np.isnan(y64)
    nll = (np.maximum(z64, 0) + np.log1p(np.exp(-np.abs(z64))) - np.where(lab, y64, 0) * z64)
    assert before["val_nll_micro"] == pytest.approx(nll[lab].sum() / lab.sum(), rel=1e-6)

    # the thresholds are those of the calibrated probabilities
    thr = torch.from_numpy(M.grid_logits(sorted(set(M.default_grid()) | {0.5}))).to(dev)
    z_cal = torch.where(ign, torch.full_like(z, math.nan), z * scale + bias)
    tp, fp = F.confusion_grid(z_cal, ym, thr)
    n_pos = torch.where(ign, torch.zeros_like(y), y).sum(0).long()
    picked = M.pick_thresholds(tp, fp, n_pos, sorted(set(M.default_grid()) | {0.5}))
    assert res["thresholds"] == picked["thresholds"]

    # the returned dict, passed back in, reproduces the "after" numbers bit for bit
    again = M.evaluate(img, txt, fus, batches, criterion=crit, calibrate=cal)
    assert repr(again["calibration"]["after"]) == repr(cal["after"])
    assert repr(again["calibration"]["before"]) == repr(cal["before"])
    assert again["thresholds"] == res["thresholds"]
    assert again["calibration"]["scale"] == cal["scale"]

    temp = M.evaluate(img, txt, fus, batches, criterion=crit, calibrate="temperature")
    assert len(set(temp["calibration"]["scale"])) == 1
    assert temp["calibration"]["bias"] == [0.0] * 13

    with pytest.raises(ValueError):
        M.evaluate(img, txt, fus, batches, calibrate="isotonic")
    with pytest.raises(ValueError):
        M.evaluate(img, txt, fus, batches, calibrate="platt", n_bins=0)
    with pytest.raises(ValueError):
        M.evaluate(img, txt, fus, batches, criterion=crit,
                   calibrate={"mode": "platt", "scale": [1.0], "bias": [0.0]})


# ----------------------------------------------------------------------------- the driver
def test_driver_stores_the_calibration_and_registers_ece(dev, tmp_path):
    """training_tests(calibrate="temperature", val_rows=6) on the 16-row feature group of
    tests/test_metrics_gpu.py: the bundle and the registry config carry the fitted dict, the
    registry metrics gain val_ece_micro, and inference() reports the calibrated probabilities."""
    import io
    import json
    import pandas as pd
    from PIL import Image
    from mmdx.inference_pipeline import inference, load_model_bundle
    bucket = "medical-ml-proj-bucket"
    mirror = tmp_path / "s3"
    (mirror / bucket / "chest-x-ray-images").mkdir(parents=True)
    rng = np.random.default_rng(17)
    rows = []
    for i in range(16):
        key = f"chest-x-ray-images/img{i:02d}.jpg"
        arr = rng.integers(0, 256, (250, 260, 3), dtype=np.uint8)
        buf = io.BytesIO()
        Image.fromarray(arr, "RGB").save(buf, format="JPEG", quality=90)
        (mirror / bucket / key).write_bytes(buf.getvalue())
        vec = (rng.random(13) < 0.3).astype(float).tolist()
        rows.append({"image_url": f"s3://{bucket}/{key}",
                     "patient_details": f"{40 + i} year old {'male' if i % 2 else 'female'} "
                                        f"PA view, cough, case {i}",
                     "disease_classification_vector": json.dumps(vec),
                     "report": f"Findings: case {i}. The lungs are clear. No effusion."})
    pq = tmp_path / "features.parquet"
    pd.DataFrame(rows).to_parquet(pq)
    old = dict(os.environ)
    os.environ.update(MMDX_FEATURES_PARQUET=str(pq), MMDX_S3_MIRROR=str(mirror),
                      AWS_S3_BUCKET_NAME=bucket, MMDX_MODEL_REGISTRY=str(tmp_path / "registry"),
                      MMDX_MODEL_DIR=str(tmp_path / "model"))
    try:
        torch.manual_seed(0)
        out = mmdx.training_pipeline.training_tests(
            num_steps=1, b_fusion=2, batch_size=4, image_backbone="resnet18",
            text_model="bert-base-uncased@2", val_rows=6, calibrate="temperature",
            gen_kwargs=dict(max_new_tokens=4, min_new_tokens=1, num_beams=2), verbose=False)
        torch.cuda.synchronize()
    finally:
        os.environ.clear()
        os.environ.update(old)
    cal = out["val"]["calibration"]
    stored = {k: cal[k] for k in ("mode", "scale", "bias", "status")}
    assert cal["mode"] == "temperature" and len(cal["scale"]) == 13
    vdir = tmp_path / "registry" / "fusion_model_T5" / str(out["registry_version"])
    entry = json.load(open(vdir / "model.json"))
    ece = cal["after"]["val_ece_micro"]
    assert entry["metrics"]["val_ece_micro"] == ece and 0.0 <= ece <= 1.0
    assert json.load(open(vdir / "config.json"))["artifacts"]["calibration"] == stored

    bundle = load_model_bundle(str(tmp_path / "model" / "model_bundle.pt"))
    assert bundle["calibration"] == stored and bundle["thresholds"] == out["val"]["thresholds"]
    pil = Image.open(os.path.join(GOLD, "e1.jpg")).convert("RGB")
    text = "44 year old female PA view , hypertension , cough"
    kw = dict(gen_kwargs={"max_new_tokens": 4, "min_new_tokens": 1})
    res = inference(bundle, pil, text, **kw)
    raw = inference(dict(bundle, calibration=None), pil, text, **kw)
    p_cal = np.array([res["disease_probs"][c] for c in mmdx.DISEASES], dtype=np.float64)
    p_raw = np.array([raw["disease_probs"][c] for c in mmdx.DISEASES], dtype=np.float64)
    # the logits back from the raw probabilities: sigmoid(a z) within float32 rounding of p_raw
    z = np.log(p_raw / (1 - p_raw))
    assert np.abs(p_cal - sigmoid64(z * cal["scale"][0])).max() <= 1e-5
    thr = np.array(bundle["thresholds"], dtype=np.float32)
    assert res["disease_vector"] == (p_cal.astype(np.float32) >= thr).astype(int).tolist()


# ----------------------------------------------------------------------------- the bundle
def test_bundle_round_trip_through_inference(dev, small_model, tmp_path):
    from PIL import Image
    from mmdx.inference_pipeline import inference, load_model_bundle, save_model_bundle
    img, txt, fus, _, _, _ = small_model
    rng = np.random.default_rng(3)
    cal = K.to_dict("platt", (0.5 + rng.random(13)).astype(np.float32),
                    rng.standard_normal(13).astype(np.float32), status=[0] * 13)
    thr = [0.3] * 13
    arts = {"class_names": list(mmdx.DISEASES), "thresholds": thr}
    p_cal = save_model_bundle(fus, img, txt, str(tmp_path / "cal"), timestamped_copy=False,
                              artifacts=dict(arts, calibration=cal))
    p_raw = save_model_bundle(fus, img, txt, str(tmp_path / "raw"), timestamped_copy=False,
                              artifacts=arts)
    b_cal = load_model_bundle(p_cal, with_report_head=False)
    b_raw = load_model_bundle(p_raw, with_report_head=False)
    assert b_cal["calibration"] == cal and b_raw["calibration"] is None

    pil = Image.open(os.path.join(GOLD, "e1.jpg")).convert("RGB")
    text = "44 year old female PA view , hypertension , cough"
    r_cal = inference(b_cal, pil, text)
    r_raw = inference(b_raw, pil, text)
    assert set(r_cal) == set(r_raw)

    with torch.no_grad():
        tok = {k: v.to(dev) for k, v in mmdx.tokenize_patient_details([text], max_len=96).items()}
        z_img = b_raw["image_encoder"](mmdx.preprocess_batch([pil], dev))["embeddings"]
        z_txt = b_raw["text_encoder"](**tok)["embeddings"]
        logits = b_raw["fusion_model"](z_img=z_img, z_txt=z_txt)["disease_logits"].float()
        scale, bias = K.from_dict(cal, 13, dev)
        want_cal = torch.sigmoid(logits * scale + bias)[0].cpu().numpy()
        want_raw = torch.sigmoid(logits)[0].cpu().numpy()
    got_cal = np.array([r_cal["disease_probs"][c] for c in mmdx.DISEASES])
    got_raw = np.array([r_raw["disease_probs"][c] for c in mmdx.DISEASES])
    assert np.abs(got_cal - want_cal).max() <= 1e-6
    assert np.array_equal(got_raw.astype(np.float32), want_raw)   # as today: plain sigmoid
    assert np.abs(got_cal - got_raw).max() > 1e-3                  # the map did something
    assert r_cal["disease_vector"] == (got_cal.astype(np.float32)
                                       >= np.float32(0.3)).astype(int).tolist()
    assert r_raw["disease_vector"] == (got_raw.astype(np.float32)
                                       >= np.float32(0.3)).astype(int).tolist()
