"""GPU: the CLAHE kernels (csrc/clahe.hip) against mmdx.clahe.reference, byte for byte, and the
setting's way through preprocess_batch, LocalCXRBatches, training_tests, the bundle loaders and
inference().  No tolerances anywhere: every step of the definition is integer arithmetic or
one correctly-rounded fp32 operation."""
import io
import json
import os

import numpy as np
import pytest
import torch

import mmdx
import mmdx.functional as F
from mmdx import clahe as K

from clahe_cases import KERNEL_CASES, case, mixed_batch, random_image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TEXT = "44 year old female PA view , hypertension , cough"


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} of {want.size} differ, first at {bad[0].tolist()}: " \
           f"got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def _check(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    assert np.array_equal(got, want), f"{what}: {_first_difference(got, want)}"


# ----------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("name", sorted(KERNEL_CASES))
def test_luts_and_output_equal_the_reference(dev, name):
    img, clip_limit, tiles, want, want_luts = case(name)
    (out,), (luts,) = F.clahe([img], clip_limit, tiles, return_luts=True, device=dev)
    _check(luts, want_luts, f"{name} LUTs")
    _check(out, want, f"{name} output")


def test_mixed_batch_in_one_call_and_twice_the_same_bytes(dev):
    imgs = mixed_batch()
    outs, luts = F.clahe(imgs, 2.0, (4, 4), return_luts=True, device=dev)
    assert len(outs) == len(luts) == len(imgs)
    for i, im in enumerate(imgs):
        want, want_luts = K.reference(im, 2.0, (4, 4), return_luts=True)
        _check(luts[i], want_luts, f"mixed[{i}] LUTs")
        _check(outs[i], want, f"mixed[{i}] output")
    again, luts2 = F.clahe(imgs, 2.0, (4, 4), return_luts=True, device=dev)
    for a, b in zip(outs + luts, again + luts2):
        assert torch.equal(a, b)


def test_input_forms(dev):
    """HxW, HxWx1 and PIL inputs come back in their own shapes; the default setting is (2, 8x8)."""
    from PIL import Image
    grey = random_image((70, 90), 50)
    rgb = random_image((70, 90, 3), 51)
    outs = F.clahe([grey, grey[:, :, None], Image.fromarray(grey, "L"),
                    Image.fromarray(rgb, "RGB")], device=dev)
    want = K.reference(grey)
    _check(outs[0], want, "HxW")
    _check(outs[1], want[:, :, None], "HxWx1")
    _check(outs[2], want, "PIL L")
    _check(outs[3], K.reference(rgb), "PIL RGB")


# ----------------------------------------------------------------------------- preprocess
def _golden_images():
    from PIL import Image
    e1 = Image.open(os.path.join(GOLD, "e1.jpg"))
    e1.load()
    e2 = Image.open(os.path.join(GOLD, "e2.jpg"))
    e2.load()
    y, x = np.mgrid[0:301, 0:277]
    grey = Image.fromarray(((x * 3 + y * 2) % 256).astype(np.uint8) // 2 + 60, "L")
    return [e1, e2, grey]


def _host_equalised(img, c):
    from PIL import Image
    return Image.fromarray(K.reference(img, c.clip_limit, c.tiles))


def test_preprocess_batch_with_clahe_equals_host_equalisation_first(dev):
    imgs = _golden_images()
    assert {im.mode for im in imgs} <= {"L", "RGB"}
    for c in (mmdx.Clahe(), mmdx.Clahe(3.5, (4, 6))):
        got = mmdx.preprocess_batch(imgs, dev, clahe=c)
        want = mmdx.preprocess_batch([_host_equalised(im, c) for im in imgs], dev)
        assert got.shape == (3, 3, 224, 224)
        assert torch.equal(got, want)
    plain = mmdx.preprocess_batch(imgs, dev)
    assert torch.equal(mmdx.preprocess_batch(imgs, dev, clahe=None), plain)
    assert not torch.equal(got, plain)
    from PIL import Image
    strip = imgs[:2] + [Image.fromarray(random_image((300, 20), 52), "L")]
    assert mmdx.preprocess_batch(strip, dev).shape == (3, 3, 224, 224)
    with pytest.raises(ValueError):     # W = 20 < 2 * 16: raised before anything is launched
        mmdx.preprocess_batch(strip, dev, clahe=mmdx.Clahe(2.0, (16, 16)))


def test_loader_with_clahe_yields_the_host_equalised_images(dev, tmp_path):
    import pandas as pd
    from mmdx import data as D
    c = mmdx.Clahe(2.0, (8, 8))
    ims = _golden_images()
    keys = []
    for i, im in enumerate(ims):
        im.save(tmp_path / f"img{i}.png")
        keys.append(f"img{i}.png")
    vecs = [np.eye(13)[i % 13].tolist() for i in range(len(keys))]
    df = pd.DataFrame(dict(image_url=keys, patient_details=[f"p{i}" for i in range(len(keys))],
                           disease_classification_vector=vecs, report=["r"] * len(keys)))
    df = D.enforce_raw_data_columns(df)
    kw = dict(batch_size=2, shuffle=False, device=dev)
    got = torch.cat([b[0] for b in D.LocalCXRBatches(df, str(tmp_path), clahe=c, **kw)])
    decoded = [D.open_image(str(tmp_path), k) for k in keys]
    want = mmdx.preprocess_batch([_host_equalised(im, c) for im in decoded], dev)
    assert torch.equal(got, want)
    plain = torch.cat([b[0] for b in D.LocalCXRBatches(df, str(tmp_path), **kw)])
    assert torch.equal(plain, mmdx.preprocess_batch(decoded, dev))
    with pytest.raises(TypeError):
        D.LocalCXRBatches(df, str(tmp_path), clahe=(2.0, (8, 8)), **kw)


# ----------------------------------------------------------------------------- the bundle
@pytest.fixture(scope="module")
def bundles(dev, tmp_path_factory):
    """One small model saved twice: with artifacts["clahe"] and without."""
    from mmdx.inference_pipeline import load_model_bundle, save_model_bundle
    torch.manual_seed(0)
    img = mmdx.ImageEncoderCNN("resnet18", 1024, 13).to(dev).eval()
    txt = mmdx.TextEncoderTransformer("bert-base-uncased@2", 512, 13).to(dev).eval()
    fus = mmdx.FusionTransformerModel(1024, 512, 1024, 13).to(dev).eval()
    c = mmdx.Clahe(2.0, (8, 8))
    arts = {"class_names": list(mmdx.DISEASES), "thresholds": [0.5] * 13}
    d = tmp_path_factory.mktemp("clahe_bundles")
    p_eq = save_model_bundle(fus, img, txt, str(d / "eq"), timestamped_copy=False,
                             artifacts=dict(arts, clahe=c.config()))
    p_raw = save_model_bundle(fus, img, txt, str(d / "raw"), timestamped_copy=False,
                              artifacts=arts)
    return (c, load_model_bundle(p_eq, with_report_head=False),
            load_model_bundle(p_raw, with_report_head=False))


def test_inference_serves_the_bundles_clahe(dev, bundles):
    from PIL import Image
    from mmdx.inference_pipeline import inference
    c, b_eq, b_raw = bundles
    assert b_eq["clahe"] == c.config() and b_raw["clahe"] is None
    pil = Image.open(os.path.join(GOLD, "e1.jpg")).convert("RGB")
    r_eq = inference(b_eq, pil, TEXT)
    r_host = inference(b_raw, _host_equalised(pil, c), TEXT)
    r_raw = inference(b_raw, pil, TEXT)
    assert set(r_eq) == set(r_raw)
    assert r_eq["disease_probs"] == r_host["disease_probs"]
    assert r_eq["disease_vector"] == r_host["disease_vector"]
    assert r_eq["disease_probs"] != r_raw["disease_probs"]


def test_inference_without_the_key_is_unchanged(dev, bundles):
    from PIL import Image
    from mmdx.inference_pipeline import inference
    _, _, b_raw = bundles
    pil = Image.open(os.path.join(GOLD, "e1.jpg")).convert("RGB")
    res = inference(b_raw, pil, TEXT)
    no_key = {k: v for k, v in b_raw.items() if k != "clahe"}   # a bundle dict from before
    assert inference(no_key, pil, TEXT)["disease_probs"] == res["disease_probs"]
    with torch.no_grad():
        tok = {k: v.to(dev) for k, v in mmdx.tokenize_patient_details([TEXT], max_len=96).items()}
        z_img = b_raw["image_encoder"](mmdx.preprocess_batch([pil], dev))["embeddings"]
        z_txt = b_raw["text_encoder"](**tok)["embeddings"]
        logits = b_raw["fusion_model"](z_img=z_img, z_txt=z_txt)["disease_logits"].float()
        want = torch.sigmoid(logits)[0].cpu().tolist()
    assert [res["disease_probs"][n] for n in mmdx.DISEASES] == want


# ----------------------------------------------------------------------------- the driver
def test_driver_stores_the_setting_and_the_loaders_return_it(dev, tmp_path):
    """training_tests(clahe=c) on the 16-row feature group the calibration test drives it with:
    the bundle and the registry config carry c.config(), and both loaders hand it back."""
    import pandas as pd
    from PIL import Image
    from mmdx.inference_pipeline import (load_model_bundle,
                                         load_model_from_hopsworks_model_registry)
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
    c = mmdx.Clahe(2.0, (8, 8))
    old = dict(os.environ)
    os.environ.update(MMDX_FEATURES_PARQUET=str(pq), MMDX_S3_MIRROR=str(mirror),
                      AWS_S3_BUCKET_NAME=bucket, MMDX_MODEL_REGISTRY=str(tmp_path / "registry"),
                      MMDX_MODEL_DIR=str(tmp_path / "model"))
    try:
        torch.manual_seed(0)
        out = mmdx.training_pipeline.training_tests(
            num_steps=1, b_fusion=2, batch_size=4, image_backbone="resnet18",
            text_model="bert-base-uncased@2", val_rows=4, clahe=c,
            gen_kwargs=dict(max_new_tokens=4, min_new_tokens=1, num_beams=2), verbose=False)
        torch.cuda.synchronize()
        reg = load_model_from_hopsworks_model_registry("fusion_model_T5",
                                                       version=out["registry_version"])
    finally:
        os.environ.clear()
        os.environ.update(old)
    vdir = tmp_path / "registry" / "fusion_model_T5" / str(out["registry_version"])
    assert json.load(open(vdir / "config.json"))["artifacts"]["clahe"] == c.config()
    assert reg["clahe"] == c.config()
    bundle = load_model_bundle(str(tmp_path / "model" / "model_bundle.pt"))
    assert bundle["clahe"] == c.config() and mmdx.Clahe.from_config(bundle["clahe"]) == c
    assert out["val"]["n"] == 4
