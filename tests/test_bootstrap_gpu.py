"""GPU: the bootstrap kernels against the numpy yardsticks of mmdx.bootstrap with zero tolerance
(both sides are integers), their ties to the two existing metric kernels, evaluate(bootstrap=R)
end to end on a small model, and the training driver.

- mmdx_bootstrap_weights (LDS histograms in windows of 16384 rows, integer atomics beyond 8
  windows) vs
  reference_weights (bincount of the same counter-based draws).
- mmdx_bootstrap_counts (weighted prefix scan over one shared sort, two tie orders) vs
  reference_counts (weighted midranks from np.unique).
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
from mmdx import bootstrap as B
from mmdx import metrics as M

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BUCKET = "medical-ml-proj-bucket"

# 16385: two LDS windows per row (the second holds one row); 131073: past the last LDS window
# count, on global atomics
WEIGHT_N = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 16385, 131073)
REPS = (1, 3, 17)          # 17 is neither a multiple nor a divisor of a replicate group (8)
SHAPES = [(n, c) for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000) for c in (1, 13)]
# (1000, 13): 7 segments of 2048 items in the micro column; (4099, 13): 3 per class column (the
# third holds 3 items) and 27 in the micro column; (300, 64): the widest class count
SHAPES += [(4099, 13), (300, 64)]
KINDS = ("continuous", "quantised", "equal")


# ----------------------------------------------------------------------------- weights
@pytest.mark.parametrize("N", WEIGHT_N)
def test_bootstrap_weights_equal_reference(dev, N):
    for R in REPS:
        for seed, r0 in ((0, 0), (0xDEADBEEFCAFEF00D, 5)):
            w = F.bootstrap_weights(R, N, seed, r0=r0, device=dev)
            assert w.dtype == torch.int32 and tuple(w.shape) == (R, N) and w.is_contiguous()
            got = w.cpu().numpy()
            assert np.array_equal(got, B.reference_weights(R, N, seed, r0=r0)), (N, R, seed)
            again = F.bootstrap_weights(R, N, seed, r0=r0, device=dev).cpu().numpy()
            assert got.tobytes() == again.tobytes()


def test_bootstrap_weights_batches_are_invisible(dev):
    for N in (300, 16385, 131073):
        whole = F.bootstrap_weights(8, N, 11, device=dev)
        parts = torch.cat([F.bootstrap_weights(3, N, 11, r0=0, device=dev),
                           F.bootstrap_weights(5, N, 11, r0=3, device=dev)])
        assert torch.equal(whole, parts)
        assert torch.equal(whole.sum(1), torch.full((8,), N, device=dev))


# ----------------------------------------------------------------------------- counts
def synth(N, C, kind, seed=0):
    """Scores (continuous / on 4 values with both zeros / all equal) with about 5 % NaN,
    Bernoulli(0.2) labels, one class without positives and one without negatives, and a
    random prediction mask."""
    g = np.random.default_rng(seed + 1000 * N + C)
    if kind == "continuous":
        s = g.standard_normal((N, C)).astype(np.float32)
        s.reshape(-1)[g.choice(N * C, min(2, N * C), replace=False)] = [0.0, -0.0][:min(2, N * C)]
    elif kind == "quantised":
        s = g.choice(np.array([-1.5, -0.0, 0.0, 2.0], np.float32), size=(N, C))
    else:
        s = np.full((N, C), 0.25, np.float32)
    s[g.random((N, C)) < 0.05] = np.nan
    y = (g.random((N, C)) < 0.2).astype(np.float32)
    if C >= 3:
        y[:, 0] = 1.0
        y[:, C - 1] = 0.0
    pred = g.random((N, C)) < 0.3
    return s, y, pred


@pytest.fixture(scope="module")
def weights17(dev):
    """Kernel-made weights per row count, 17 replicates (prefixes serve R = 1 and 3: the draw
    of a replicate does not depend on R), with their host copies."""
    out = {}
    for N in sorted({n for n, _ in SHAPES}):
        w = F.bootstrap_weights(17, N, 5, device=dev)
        out[N] = (w, w.cpu().numpy())
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,C", SHAPES)
def test_bootstrap_counts_equal_reference(dev, weights17, N, C, kind):
    s, y, pred = synth(N, C, kind)
    sd, yd = torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev)
    wd, wh = weights17[N]
    assert np.array_equal(wh.sum(1), [N] * 17)
    for use_pred in (True, False):
        plan = F.bootstrap_plan(sd, yd, torch.from_numpy(pred).to(dev) if use_pred else None)
        want = B.reference_counts(s, y, wh, pred if use_pred else None)
        for R in REPS:
            got = F.bootstrap_counts(plan, wd[:R].contiguous())
            assert got.dtype == torch.int64 and tuple(got.shape) == (R, C + 1, 5)
            got = got.cpu().numpy()
            assert np.array_equal(got, want[:R]), (N, C, kind, use_pred, R)
        if not use_pred:
            assert not got[..., 3:].any()
    if C >= 3:
        assert not want[:, 0, 2].any() and not want[:, C - 1, 1].any()
    if kind == "equal":      # every live pair ties: u2 = w_pos * w_neg
        assert np.array_equal(want[..., 0], want[..., 1] * want[..., 2])


def test_bootstrap_counts_adversarial_weights(dev):
    """Hand-made multiplicities: all weight on one row, on the first and the last row, zero
    everywhere, and all ones."""
    N, C = 257, 13
    s, y, pred = synth(N, C, "quantised", seed=3)
    w = np.zeros((5, N), np.int32)
    w[0, 100] = N
    w[1, 0], w[1, N - 1] = N - 1, 1
    w[3] = 1
    w[4, ::2] = 2
    plan = F.bootstrap_plan(torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev),
                            torch.from_numpy(pred).to(dev))
    got = F.bootstrap_counts(plan, torch.from_numpy(w).to(dev)).cpu().numpy()
    assert np.array_equal(got, B.reference_counts(s, y, w, pred))
    assert not got[2].any()
    # one row alone makes no pair within a class, but it does across classes (micro)
    assert not got[0, :C, 0].any()


def test_bootstrap_counts_bit_reproducible_and_out_argument(dev, weights17):
    s, y, pred = synth(4099, 13, "quantised")
    plan = F.bootstrap_plan(torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev),
                            torch.from_numpy(pred).to(dev))
    wd = weights17[4099][0]
    a = F.bootstrap_counts(plan, wd)
    big = torch.full((20, 14, 5), -1, dtype=torch.int64, device=dev)
    b = F.bootstrap_counts(plan, wd, out=big[2:19])
    assert b.data_ptr() == big[2:19].data_ptr()
    assert a.cpu().numpy().tobytes() == big[2:19].cpu().numpy().tobytes()
    assert (big[:2] == -1).all() and (big[19:] == -1).all()


@pytest.mark.parametrize("N,C", [(65, 13), (1000, 13), (300, 64)])
def test_unit_weights_give_the_all_pairs_counts(dev, N, C):
    """Ties the scan to mmdx_auroc_pairs: with every weight 1, (u2, w_pos, w_neg) are its
    (u2, n_pos, n_neg)."""
    s, y, _ = synth(N, C, "quantised", seed=7)
    sd, yd = torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev)
    ones = torch.ones((1, N), dtype=torch.int32, device=dev)
    boot = F.bootstrap_counts(F.bootstrap_plan(sd, yd), ones)
    assert torch.equal(boot[0, :, :3], F.auroc_counts(sd, yd)[:, :3])


def test_pred_from_a_threshold_gives_the_confusion_grid_column(dev):
    """Ties tp / fp to mmdx_confusion_grid: pred = logits >= thr[t] and unit weights."""
    N, C = 1000, 13
    g = np.random.default_rng(21)
    z = (np.round(g.standard_normal((N, C)) * 8) / 8).astype(np.float32)
    z[g.random((N, C)) < 0.05] = np.nan
    y = (g.random((N, C)) < 0.2).astype(np.float32)
    zd, yd = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
    thr = torch.from_numpy(M.grid_logits([0.1, 0.35, 0.5, 0.62, 0.9])).to(dev)
    thr[3] = 0.5                       # a threshold many logits equal
    tp, fp = F.confusion_grid(zd, yd, thr)
    ones = torch.ones((1, N), dtype=torch.int32, device=dev)
    for t in range(5):
        boot = F.bootstrap_counts(F.bootstrap_plan(zd, yd, zd >= thr[t]), ones)
        assert torch.equal(boot[0, :C, 3], tp[:, t]) and torch.equal(boot[0, :C, 4], fp[:, t])
        assert boot[0, C, 3] == tp[:, t].sum() and boot[0, C, 4] == fp[:, t].sum()


def test_bootstrap_wrappers_check_their_inputs(dev):
    z = torch.zeros(8, 4, device=dev)
    w = torch.ones(3, 8, dtype=torch.int32, device=dev)
    plan = F.bootstrap_plan(z, z)
    with pytest.raises(TypeError):
        F.bootstrap_plan(z.half(), z)
    with pytest.raises(ValueError, match="contiguous"):
        F.bootstrap_plan(z.t(), z.t())
    with pytest.raises(ValueError):
        F.bootstrap_plan(z, z[:4])
    with pytest.raises(ValueError, match="GPU"):
        F.bootstrap_plan(z, z.cpu())
    with pytest.raises(ValueError, match="64"):
        F.bootstrap_plan(torch.zeros(2, 65, device=dev), torch.zeros(2, 65, device=dev))
    with pytest.raises(TypeError, match="bool"):
        F.bootstrap_plan(z, z, pred=z)
    with pytest.raises(ValueError, match="pred"):
        F.bootstrap_plan(z, z, pred=torch.zeros(8, 3, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError, match="pred"):
        F.bootstrap_plan(z, z, pred=torch.zeros(8, 4, dtype=torch.bool))
    with pytest.raises(TypeError, match="int32"):
        F.bootstrap_counts(plan, w.long())
    with pytest.raises(ValueError, match=r"\[R, 8\]"):
        F.bootstrap_counts(plan, w[:, :7].contiguous())
    with pytest.raises(ValueError, match=r"\[R, 8\]"):
        F.bootstrap_counts(plan, w[0])
    with pytest.raises(ValueError, match="contiguous"):
        F.bootstrap_counts(plan, torch.ones(8, 3, dtype=torch.int32, device=dev).t())
    with pytest.raises(ValueError, match="plan on"):
        F.bootstrap_counts(plan, w.cpu())
    with pytest.raises(ValueError, match="out must be"):
        F.bootstrap_counts(plan, w, out=torch.zeros(3, 5, 4, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="2\\^26"):
        F.bootstrap_weights(2 ** 13, 2 ** 13 + 1, 0, device=dev)
    with pytest.raises(TypeError):
        F.bootstrap_weights(2, 8, 0.5, device=dev)


# ----------------------------------------------------------------------------- evaluate()
N_EVAL = 300


@pytest.fixture(scope="module")
def eval_run(dev):
    """The small model of tests/test_metrics_gpu.py on 300 rows with label prevalence 0.15
    (the smallest resampled positive count of a class over 64 replicates is then far above 0,
    so every replicate of every class is valid), evaluated once without and once with the
    bootstrap, plus the collected logits."""
    torch.manual_seed(0)
    img = mmdx.ImageEncoderCNN("resnet18", 1024, 13).to(dev)
    txt = mmdx.TextEncoderTransformer("bert-base-uncased@2", 512, 13).to(dev)
    fus = mmdx.FusionTransformerModel(1024, 512, 1024, 13).to(dev)
    for top in (img, txt, fus):
        top.eval()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N_EVAL, 3, 64, 64, generator=g)
    y = (torch.rand(N_EVAL, 13, generator=g) < 0.15).float()
    details = [f"{30 + i % 50} year old {'male' if i % 2 else 'female'} PA view, "
               f"{'cough' if i % 3 else 'fever'}, case {i}" for i in range(N_EVAL)]
    batches = [(x[s:s + 64].to(dev), details[s:s + 64], y[s:s + 64].to(dev))
               for s in range(0, N_EVAL, 64)]       # 4 x 64 + 44: the last batch is ragged
    plain = M.evaluate(img, txt, fus, batches)
    boot = M.evaluate(img, txt, fus, batches, bootstrap=64, bootstrap_seed=9)
    zs = []
    with torch.no_grad():
        for xb, db, _ in batches:
            tok = {k: v.to(dev) for k, v in
                   mmdx.tokenize_patient_details(list(db), max_len=96).items()}
            zs.append(fus(z_img=img(xb)["embeddings"],
                          z_txt=txt(**tok)["embeddings"])["disease_logits"].float())
    return (img, txt, fus, batches), plain, boot, torch.cat(zs).cpu().numpy(), y.numpy()


def _same(a, b):
    """Equality of nested results in which nan == nan."""
    try:
        np.testing.assert_equal(a, b)
    except AssertionError:
        return False
    return True


def test_evaluate_bootstrap_leaves_every_point_estimate_as_it_was(eval_run):
    _, plain, boot, _, _ = eval_run
    assert set(boot) == set(plain) | {"ci", "boot"}
    assert "ci" not in plain and "boot" not in plain
    for k, v in plain.items():
        assert _same(boot[k], v), k
    assert np.float32(boot["val_loss"]).tobytes() == np.float32(plain["val_loss"]).tobytes()


def test_evaluate_bootstrap_equals_the_numpy_statement(eval_run):
    _, _, out, z, y = eval_run
    assert out["n"] == N_EVAL and z.shape == (N_EVAL, 13)
    grid = M.default_grid()
    thr = M.grid_logits(grid)[[grid.index(p) for p in out["thresholds"]]]
    want = B.reference_counts(z, y, B.reference_weights(64, N_EVAL, 9), z >= thr)
    assert out["boot"].dtype == np.int64 and np.array_equal(out["boot"], want)

    ci, iv = out["ci"], B.intervals(out["boot"], 0.95)
    assert (ci["level"], ci["n_replicates"], ci["seed"]) == (0.95, 64, 9)
    assert _same(ci["val_auroc_micro"], iv["auroc_micro"])
    assert _same(ci["val_auroc_macro"], iv["auroc_macro"])
    assert _same(ci["val_auroc_per_class"], iv["auroc_per_class"])
    assert _same(ci["val_f1_micro"], iv["f1_micro"])
    assert len(ci["per_class"]) == 13
    for c, leaf in enumerate(ci["per_class"]):
        assert set(leaf) == {"sensitivity", "specificity", "f1"}
        for k in leaf:
            assert _same(leaf[k], iv[f"{k}_per_class"][c])

    # every replicate of every statistic is valid, and each point estimate lies inside the
    # range of its replicates
    st = B.replicate_stats(out["boot"])
    points = [(ci["val_auroc_micro"], out["val_auroc_micro"], st["auroc"][:, 13]),
              (ci["val_auroc_macro"], out["val_auroc_macro"], st["auroc_macro"]),
              (ci["val_f1_micro"], out["val_f1_micro"], st["f1"][:, 13])]
    for c in range(13):
        pc = out["per_class"][c]
        points += [(ci["val_auroc_per_class"][c], out["val_auroc_per_class"][c],
                    st["auroc"][:, c]),
                   (ci["per_class"][c]["sensitivity"], pc["recall"], st["sensitivity"][:, c]),
                   (ci["per_class"][c]["f1"], pc["f1"], st["f1"][:, c])]
        assert ci["per_class"][c]["specificity"]["n_valid"] == 64
    for leaf, point, reps in points:
        assert leaf["n_valid"] == 64
        assert leaf["lo"] <= leaf["hi"] and leaf["se"] >= 0.0
        assert reps.min() <= point <= reps.max(), (point, reps.min(), reps.max())


def test_evaluate_bootstrap_batching_is_invisible(eval_run, monkeypatch):
    (img, txt, fus, batches), _, out, _, _ = eval_run
    sizes = []

    def seven(R, N):
        sizes.append((R, N))
        return 7

    monkeypatch.setattr(B, "batch_size", seven)
    again = M.evaluate(img, txt, fus, batches, bootstrap=64, bootstrap_seed=9)
    assert sizes == [(64, N_EVAL)]
    assert np.array_equal(again["boot"], out["boot"])
    assert _same(again["ci"], out["ci"])
    other = M.evaluate(img, txt, fus, batches, bootstrap=5, bootstrap_seed=10, ci_level=0.8)
    assert other["boot"].shape == (5, 14, 5) and other["ci"]["level"] == 0.8
    assert not np.array_equal(other["boot"], out["boot"][:5])


def test_evaluate_bootstrap_with_ignored_labels(eval_run, dev):
    """NaN labels are masked exactly as in the point estimates: the elements weigh nothing."""
    (img, txt, fus, batches), _, _, z, y = eval_run
    g = np.random.default_rng(2)
    ign = g.random(y.shape) < 0.1
    yn = y.copy()
    yn[ign] = np.nan
    masked = [(xb, db, torch.from_numpy(yn[s:s + 64]).to(dev))
              for (xb, db, _), s in zip(batches, range(0, N_EVAL, 64))]
    out = M.evaluate(img, txt, fus, masked, bootstrap=16, bootstrap_seed=4)
    zm = np.where(ign, np.nan, z).astype(np.float32)
    ym = np.where(ign, 0.0, y).astype(np.float32)
    grid = M.default_grid()
    thr = M.grid_logits(grid)[[grid.index(p) for p in out["thresholds"]]]
    w = B.reference_weights(16, N_EVAL, 4).astype(np.int64)
    with np.errstate(invalid="ignore"):
        want = B.reference_counts(zm, ym, w, zm >= thr)
    assert np.array_equal(out["boot"], want)
    # an ignored element weighs nothing: w_pos + w_neg is the resampled count of the labelled
    labelled = w @ (~ign).astype(np.int64)
    assert np.array_equal(out["boot"][:, :13, 1] + out["boot"][:, :13, 2], labelled)
    assert np.array_equal(out["boot"][:, 13, 1] + out["boot"][:, 13, 2], labelled.sum(1))
    assert (labelled < N_EVAL).all()


def test_paired_delta_of_a_model_with_itself_and_with_a_noisy_copy(dev, eval_run):
    _, _, out, z, y = eval_run
    zd, yd = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
    w = F.bootstrap_weights(64, N_EVAL, 9, device=dev)
    a = F.bootstrap_counts(F.bootstrap_plan(zd, yd), w).cpu().numpy()
    assert np.array_equal(a[..., :3], out["boot"][..., :3])
    noisy = zd + 3.0 * torch.randn(zd.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    b = F.bootstrap_counts(F.bootstrap_plan(noisy.contiguous(), yd), w).cpu().numpy()
    assert B.paired_delta(a, a)["micro"]["p_two_sided"] == 1.0
    d = B.paired_delta(a, b)
    assert d["micro"]["n_valid"] == 64 and len(d["per_class"]) == 13
    other = F.bootstrap_counts(F.bootstrap_plan(zd, yd),
                               F.bootstrap_weights(64, N_EVAL, 10, device=dev)).cpu().numpy()
    with pytest.raises(ValueError):
        B.paired_delta(a, other)


# ----------------------------------------------------------------------------- the driver
@pytest.fixture(scope="module")
def feature_group(tmp_path_factory):
    """The local feature group of tests/test_metrics_gpu.py with 40 rows, so that 32 validation
    rows are disjoint from the 2 fusion rows."""
    import pandas as pd
    from PIL import Image
    root = tmp_path_factory.mktemp("bootstrap_driver")
    mirror = root / "s3"
    (mirror / BUCKET / "chest-x-ray-images").mkdir(parents=True)
    rng = np.random.default_rng(23)
    rows = []
    for i in range(40):
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


def test_driver_registers_the_interval_ends(dev, feature_group):
    root, mirror, pq = feature_group
    old = dict(os.environ)
    os.environ.update(MMDX_FEATURES_PARQUET=str(pq), MMDX_S3_MIRROR=str(mirror),
                      AWS_S3_BUCKET_NAME=BUCKET, MMDX_MODEL_REGISTRY=str(root / "registry"),
                      MMDX_MODEL_DIR=str(root / "model"))
    try:
        torch.manual_seed(0)
        out = mmdx.training_pipeline.training_tests(
            num_steps=1, b_fusion=2, batch_size=8, image_backbone="resnet18",
            text_model="bert-base-uncased@2", val_rows=32, bootstrap=16,
            gen_kwargs=dict(max_new_tokens=4, min_new_tokens=1, num_beams=2), verbose=False)
        torch.cuda.synchronize()
    finally:
        os.environ.clear()
        os.environ.update(old)
    val = out["val"]
    assert val["n"] == 32 and val["boot"].shape == (16, 14, 5)
    assert val["ci"]["n_replicates"] == 16
    with open(root / "registry" / "fusion_model_T5" / str(out["registry_version"]) /
              "model.json") as f:
        entry = json.load(f)
    for k in ("val_auroc_micro", "val_auroc_macro"):
        lo, hi = entry["metrics"][f"{k}_ci_lo"], entry["metrics"][f"{k}_ci_hi"]
        print(k, lo, entry["metrics"][k], hi)
        assert (lo, hi) == (val["ci"][k]["lo"], val["ci"][k]["hi"])
        assert lo <= entry["metrics"][k] <= hi
    assert math.isfinite(entry["metrics"]["val_loss"])
