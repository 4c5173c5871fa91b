"""GPU: the validation-metric kernels against numpy references built on a different algorithm,
with zero tolerance (both sides are integer counts), evaluate() end to end on a small model,
and the training driver with held-out rows.

- AUROC pair counts (mmdx_auroc_pairs, tiled all-pairs counting) vs midranks from np.unique:
  u2 = 2 * sum(ranks of the positives) - n_pos (n_pos + 1), in int64.
- Confusion grid (mmdx_confusion_grid, LDS histogram + suffix sum) vs np.searchsorted.
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
from mmdx import metrics as M

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BUCKET = "medical-ml-proj-bucket"

SHAPES = [(n, c) for n in (1, 2, 63, 64, 65, 257, 1000) for c in (1, 13, 16)]
# one larger case (14 row tiles, 209 blocks) and the widest class count (3 class chunks of the
# confusion grid at T = 256, 64-row AUROC tiles)
SHAPES += [(4099, 13), (300, 64)]


# ----------------------------------------------------------------------------- references
def _ref_row(s, pos):
    """(u2, n_pos, n_neg, n_nan) of one class from midranks; NaN scores count only in n_nan."""
    nan = np.isnan(s)
    s, pos = s[~nan], pos[~nan]
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    u2 = 0
    if n_pos:
        _, inv, cnt = np.unique(s, return_inverse=True, return_counts=True)  # -0.0 == +0.0
        cum = np.cumsum(cnt).astype(np.int64)
        rank2 = 2 * cum - cnt + 1          # twice the midrank of each distinct value
        u2 = int(rank2[inv.reshape(-1)][pos].sum()) - n_pos * (n_pos + 1)
    return [u2, n_pos, n_neg, int(nan.sum())]


def ref_auroc_counts(scores, target):
    pos = target > 0.5
    rows = [_ref_row(scores[:, c], pos[:, c]) for c in range(scores.shape[1])]
    rows.append(_ref_row(scores.reshape(-1), pos.reshape(-1)))
    return np.array(rows, dtype=np.int64)


def ref_confusion(logits, target, thr):
    pos = target > 0.5
    T = len(thr)
    k = np.searchsorted(thr, logits, side="right")   # number of thresholds <= logit
    k[np.isnan(logits)] = 0
    tp = np.zeros((logits.shape[1], T), dtype=np.int64)
    fp = np.zeros_like(tp)
    for c in range(logits.shape[1]):
        for dst, sel in ((tp, pos[:, c]), (fp, ~pos[:, c])):
            h = np.bincount(k[sel, c], minlength=T + 1)
            dst[c] = h[::-1].cumsum()[::-1][1:]      # sum over k > t
    return tp, fp


def ref_thresholds(tp, fp, n_pos, grid):
    """F1 = 2tp / (2tp + fp + fn) in float64; ties: nearest 0.5, then lower; no positives: 0.5."""
    out = []
    for c in range(tp.shape[0]):
        if n_pos[c] < 1:
            out.append(0.5)
            continue
        best = None
        for t, p in enumerate(grid):
            d = int(tp[c, t]) + int(fp[c, t]) + int(n_pos[c])   # 2tp + fp + (n_pos - tp)
            f1 = 2 * int(tp[c, t]) / d if d else 0.0
            key = (-f1, round(abs(p - 0.5), 12), p)
            if best is None or key < best:
                best = key
        out.append(best[2])
    return out


def synth(N, C, seed=0):
    """randn rounded to multiples of 1/8 (dense ties that cross tile boundaries), the IEEE
    special values, Bernoulli(0.2) labels, one all-positive and one all-negative column."""
    g = np.random.default_rng(seed + 1000 * N + C)
    s = (np.round(g.standard_normal((N, C)) * 8) / 8).astype(np.float32)
    y = (g.random((N, C)) < 0.2).astype(np.float32)
    flat = s.reshape(-1)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 0.0, -0.0, np.inf, -np.inf], np.float32)
    n = min(len(special), flat.size)
    flat[g.choice(flat.size, n, replace=False)] = special[:n]
    if C >= 3:
        y[:, 0] = 1.0
        y[:, C - 1] = 0.0
    return s, y


@pytest.fixture(scope="module")
def cases():
    """Inputs and numpy references, computed once and shared (read-only)."""
    out = {}
    for N, C in SHAPES:
        s, y = synth(N, C)
        out[(N, C)] = (s, y, ref_auroc_counts(s, y))
    return out


# ----------------------------------------------------------------------------- AUROC kernel
@pytest.mark.parametrize("N,C", SHAPES)
def test_auroc_counts_equal_reference(dev, cases, N, C):
    s, y, want = cases[(N, C)]
    got = F.auroc_counts(torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev))
    assert got.dtype == torch.int64 and tuple(got.shape) == (C + 1, 4)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (got - want)
    # floats derived on the host in float64 are equal too
    pc, macro, micro = M.auroc_from_counts(got)
    for c in range(C):
        if want[c, 1] and want[c, 2]:
            assert pc[c] == float(want[c, 0]) / float(2 * want[c, 1] * want[c, 2])
        else:
            assert math.isnan(pc[c])
    if C >= 3:
        assert math.isnan(pc[0]) and math.isnan(pc[C - 1])


@pytest.mark.parametrize("rate", [0.7, 1.0, 0.0])
def test_auroc_counts_at_other_positive_rates(dev, rate):
    """Mostly positive labels (a block then holds more positives than threads and sweeps the
    negatives in several rounds), and the one-label extremes."""
    s, _ = synth(700, 13, seed=3)
    y = (np.random.default_rng(4).random(s.shape) < rate).astype(np.float32)
    want = ref_auroc_counts(s, y)
    got = F.auroc_counts(torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev)).cpu().numpy()
    assert np.array_equal(got, want), (got - want)


def test_auroc_counts_nan_scores(dev):
    s, y = synth(257, 13, seed=5)
    s[3, 2] = s[100, 2] = s[256, 12] = s[0, 0] = np.nan
    y[3, 2], y[100, 2] = 1.0, 0.0          # a NaN positive and a NaN negative in one class
    want = ref_auroc_counts(s, y)
    assert want[2, 3] == 2 and want[12, 3] == 1 and want[0, 3] == 1 and want[13, 3] == 4
    got = F.auroc_counts(torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev)).cpu().numpy()
    assert np.array_equal(got, want), (got - want)
    assert np.array_equal(got[:, 1] + got[:, 2] + got[:, 3], [257] * 13 + [257 * 13])
    with pytest.raises(ValueError, match=r"\[0, 2, 12\]"):
        M.auroc_from_counts(got)


def test_auroc_counts_bit_reproducible(dev, cases):
    s, y, _ = cases[(4099, 13)]
    sd, yd = torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev)
    a = F.auroc_counts(sd, yd).cpu().numpy().tobytes()
    b = F.auroc_counts(sd, yd).cpu().numpy().tobytes()
    assert a == b


def test_metric_wrappers_check_their_inputs(dev):
    z = torch.zeros(8, 4, device=dev)
    with pytest.raises(RuntimeError, match="contiguous"):
        F.auroc_counts(z.t(), z.t())
    with pytest.raises(TypeError):
        F.auroc_counts(z.half(), z)
    with pytest.raises(ValueError):
        F.auroc_counts(z, z[:4])
    with pytest.raises(RuntimeError, match="C = 65"):
        F.auroc_counts(torch.zeros(2, 65, device=dev), torch.zeros(2, 65, device=dev))
    with pytest.raises(RuntimeError, match="T = 257"):
        F.confusion_grid(z, z, torch.zeros(257, device=dev))
    with pytest.raises(TypeError):
        F.confusion_grid(z, z, torch.zeros(3, device=dev, dtype=torch.float64))


# ----------------------------------------------------------------------------- confusion grid
def _thresholds(T, seed):
    """Sorted fp32 thresholds: multiples of 1/8 (equal to many logits), repeated values,
    values between the logits, and the infinities when there is room."""
    g = np.random.default_rng(seed)
    a = np.round(g.standard_normal(T) * 8) / 8
    a[::3] += 1.0 / 16
    if T >= 8:
        a[1] = a[2] = a[3]
        a[4], a[5] = np.inf, -np.inf
        a[6] = 0.0
    return np.sort(a).astype(np.float32)


@pytest.mark.parametrize("N,C", SHAPES)
def test_confusion_grid_equals_reference(dev, cases, N, C):
    s, y, _ = cases[(N, C)]
    sd, yd = torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev)
    for T in (1, 100, 256):
        thr = _thresholds(T, seed=T + N)
        if T >= 8:
            assert len(np.unique(thr)) < T and np.isin(thr, s).any()
        tp, fp = F.confusion_grid(sd, yd, torch.from_numpy(thr).to(dev))
        assert tp.dtype == fp.dtype == torch.int64 and tuple(tp.shape) == (C, T)
        want_tp, want_fp = ref_confusion(s, y, thr)
        assert np.array_equal(tp.cpu().numpy(), want_tp), (N, C, T)
        assert np.array_equal(fp.cpu().numpy(), want_fp), (N, C, T)


def test_confusion_grid_nan_logit_counts_nowhere(dev):
    s, y = synth(65, 13, seed=9)
    s[7, 3] = s[64, 12] = np.nan
    thr = _thresholds(100, seed=3)
    tp, fp = F.confusion_grid(torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev),
                              torch.from_numpy(thr).to(dev))
    want_tp, want_fp = ref_confusion(s, y, thr)
    assert np.array_equal(tp.cpu().numpy(), want_tp)
    assert np.array_equal(fp.cpu().numpy(), want_fp)


# ----------------------------------------------------------------------------- evaluate()
@pytest.fixture(scope="module")
def small_model(dev):
    torch.manual_seed(0)
    img = mmdx.ImageEncoderCNN("resnet18", 1024, 13).to(dev)
    txt = mmdx.TextEncoderTransformer("bert-base-uncased@2", 512, 13).to(dev)
    fus = mmdx.FusionTransformerModel(1024, 512, 1024, 13).to(dev)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(10, 3, 64, 64, generator=g)
    y = (torch.rand(10, 13, generator=g) < 0.3).float()
    details = [f"{30 + 3 * i} year old {'male' if i % 2 else 'female'} PA view, "
               f"{'cough' if i % 3 else 'fever'}, case {i}" for i in range(10)]
    batches = [(x[s:s + 4].to(dev), details[s:s + 4], y[s:s + 4].to(dev))
               for s in range(0, 10, 4)]   # 4 + 4 + 2: the last batch is ragged
    return img, txt, fus, batches


def test_evaluate_end_to_end(dev, small_model):
    img, txt, fus, batches = small_model
    img.train()
    txt.eval()
    fus.train()
    fus.fusion_mlp[2].eval()               # a submodule that differs from its parent
    flags = [[m.training for m in top.modules()] for top in (img, txt, fus)]
    res = M.evaluate(img, txt, fus, batches)
    assert [[m.training for m in top.modules()] for top in (img, txt, fus)] == flags

    for top in (img, txt, fus):
        top.eval()
    zs = []
    with torch.no_grad():
        for xb, db, _ in batches:
            tok = {k: v.to(dev) for k, v in
                   mmdx.tokenize_patient_details(list(db), max_len=96).items()}
            z_img = img(xb)["embeddings"]
            z_txt = txt(**tok)["embeddings"]
            zs.append(fus(z_img=z_img, z_txt=z_txt)["disease_logits"].float())
    z = torch.cat(zs)
    yd = torch.cat([b[2] for b in batches])
    zn, yn = z.cpu().numpy(), yd.cpu().numpy()
    assert zn.shape == (10, 13) and res["n"] == 10

    k = ref_auroc_counts(zn, yn)
    want_pc = [float(r[0]) / float(2 * r[1] * r[2]) if r[1] and r[2] else math.nan
               for r in k[:13]]
    for got, want in zip(res["val_auroc_per_class"], want_pc):
        assert got == want or (math.isnan(got) and math.isnan(want))
    defined = [v for v in want_pc if not math.isnan(v)]
    assert res["val_auroc_macro"] == math.fsum(defined) / len(defined)
    assert res["val_auroc_micro"] == float(k[13, 0]) / float(2 * k[13, 1] * k[13, 2])

    grid = M.default_grid()
    tp, fp = ref_confusion(zn, yn, M.grid_logits(grid))
    want_thr = ref_thresholds(tp, fp, k[:13, 1], grid)
    assert res["thresholds"] == want_thr
    assert [p["n_pos"] for p in res["per_class"]] == k[:13, 1].tolist()
    i_half = grid.index(0.5)
    tp5, fp5 = int(tp[:, i_half].sum()), int(fp[:, i_half].sum())
    assert res["val_f1_micro_at_0p5"] == 2 * tp5 / (tp5 + fp5 + int(k[13, 1]))
    tpc = sum(int(tp[c, grid.index(p)]) for c, p in enumerate(want_thr))
    fpc = sum(int(fp[c, grid.index(p)]) for c, p in enumerate(want_thr))
    assert res["val_f1_micro"] == 2 * tpc / (tpc + fpc + int(k[13, 1]))

    want_loss = torch.nn.functional.binary_cross_entropy_with_logits(z.double(),
                                                                     yd.double()).item()
    assert abs(res["val_loss"] - want_loss) <= 1e-5 * abs(want_loss)
    assert "val_rougeL" not in res


def test_evaluate_restores_training_flags_after_an_exception(dev, small_model):
    img, txt, fus, batches = small_model
    img.eval()
    txt.train()
    fus.train()
    flags = [[m.training for m in top.modules()] for top in (img, txt, fus)]

    def broken():
        yield batches[0]
        raise RuntimeError("loader broke")

    with pytest.raises(RuntimeError, match="loader broke"):
        M.evaluate(img, txt, fus, broken())
    assert [[m.training for m in top.modules()] for top in (img, txt, fus)] == flags


def test_evaluate_from_a_generator_grows_its_buffers(dev, small_model):
    """A loader without len(): the device buffers start at four batches and grow; the result
    is the one the sized loader gives."""
    img, txt, fus, batches = small_model
    small = [(xb[:1], db[:1], yb[:1]) for xb, db, yb in batches] + \
            [(xb[1:], db[1:], yb[1:]) for xb, db, yb in batches]
    a = M.evaluate(img, txt, fus, (b for b in small))
    assert a["n"] == 10 and math.isfinite(a["val_loss"])
    assert len(a["thresholds"]) == 13


# ----------------------------------------------------------------------------- the driver
@pytest.fixture(scope="module")
def feature_group(tmp_path_factory):
    """The local feature group of tests/test_dropin_gpu.py with 16 rows, so that 6 validation
    rows are disjoint from the 2 fusion rows."""
    import pandas as pd
    from PIL import Image
    root = tmp_path_factory.mktemp("metrics_driver")
    mirror = root / "s3"
    (mirror / BUCKET / "chest-x-ray-images").mkdir(parents=True)
    rng = np.random.default_rng(17)
    rows = []
    for i in range(16):
        key = f"chest-x-ray-images/img{i:02d}.jpg"
        if i == 0:
            data = open(os.path.join(GOLD, "e1.jpg"), "rb").read()
        else:
            h, w = int(rng.integers(240, 320)), int(rng.integers(240, 320))
            mode = "L" if i % 3 == 0 else "RGB"
            arr = rng.integers(0, 256, (h, w) if mode == "L" else (h, w, 3), dtype=np.uint8)
            buf = io.BytesIO()
            Image.fromarray(arr, mode).save(buf, format="JPEG", quality=90)
            data = buf.getvalue()
        (mirror / BUCKET / key).write_bytes(data)
        vec = (rng.random(13) < 0.3).astype(float).tolist()
        rows.append({"image_url": f"s3://{BUCKET}/{key}",
                     "patient_details": f"{40 + i} year old {'male' if i % 2 else 'female'} "
                                        f"PA view, cough, case {i}",
                     "disease_classification_vector": json.dumps(vec),
                     "report": f"Findings: case {i}. The lungs are clear. No effusion."})
    pq = root / "features.parquet"
    pd.DataFrame(rows).to_parquet(pq)
    return root, mirror, pq


def test_driver_registers_measured_metrics_and_thresholds(dev, feature_group):
    from PIL import Image
    from mmdx.inference_pipeline import inference, load_model_bundle
    root, mirror, pq = feature_group
    old = dict(os.environ)
    os.environ.update(MMDX_FEATURES_PARQUET=str(pq), MMDX_S3_MIRROR=str(mirror),
                      AWS_S3_BUCKET_NAME=BUCKET, MMDX_MODEL_REGISTRY=str(root / "registry"),
                      MMDX_MODEL_DIR=str(root / "model"))
    try:
        torch.manual_seed(0)
        out = mmdx.training_pipeline.training_tests(
            num_steps=1, b_fusion=2, batch_size=4, image_backbone="resnet18",
            text_model="bert-base-uncased@2", val_rows=6,
            gen_kwargs=dict(max_new_tokens=4, min_new_tokens=1, num_beams=2), verbose=False)
        torch.cuda.synchronize()
    finally:
        os.environ.clear()
        os.environ.update(old)
    val = out["val"]
    assert val["n"] == 6 and len(val["thresholds"]) == 13
    assert 0.0 <= val["val_rougeL"] <= 1.0 and math.isfinite(val["val_loss"])

    with open(root / "registry" / "fusion_model_T5" / str(out["registry_version"]) /
              "model.json") as f:
        entry = json.load(f)
    want = {k: (None if val[k] != val[k] else val[k]) for k in
            ("val_auroc_micro", "val_auroc_macro", "val_loss", "val_f1_micro", "val_rougeL")}
    assert entry["metrics"] == want
    assert entry["metrics"]["val_auroc_micro"] != 0.874
    assert entry["metrics"]["val_rougeL"] != 0.214

    bundle = load_model_bundle(str(root / "model" / "model_bundle.pt"))
    assert bundle["thresholds"] == val["thresholds"]
    assert all(0.0 < t < 1.0 for t in bundle["thresholds"])
    pil = Image.open(os.path.join(GOLD, "e1.jpg")).convert("RGB")
    res = inference(bundle, pil, "44 year old female PA view , hypertension , cough",
                    gen_kwargs={"max_new_tokens": 4, "min_new_tokens": 1})
    probs = np.array([res["disease_probs"][c] for c in mmdx.DISEASES], dtype=np.float32)
    thr = np.array(val["thresholds"], dtype=np.float32)
    assert res["disease_vector"] == (probs >= thr).astype(int).tolist()
