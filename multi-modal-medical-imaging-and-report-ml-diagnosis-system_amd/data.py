"""Local dataset loader: the reference's Hopsworks feature group + S3
image bucket replaced by a local parquet file and a local image directory, feeding the same
(image, patient_details, disease vector) triples to the GPU train step.

Reference behaviour kept:
  * the raw-data schema and type enforcement of `feature_pipeline.enforce_raw_data_columns`
    (feature_pipeline.py:34-58): image_url / patient_details / report as str, the disease
    vector as 13 floats (a list or its JSON text), ValueError otherwise;
  * the feature-store read's dedupe (TP:86-88): with an `event_time` column, the latest row
    per image_url wins;
  * `construct_input_label_pairs_for_image_encoder_dataset` (TP:122-127): image keys from the
    image_url column (an s3://bucket/key URL keeps its key, TP:99-103; a plain path is used as
    is) and float32 label vectors;
  * `CXR_ImageDataset.__getitem__` (TP:142-152): image bytes -> PIL image -> the transform,
    label as a float32 tensor.

New: `LocalCXRBatches` decodes a batch on the host with PIL (as the reference does) and runs
the transform for the whole batch on the GPU in two HIP launches (`preprocess_batch`,
bit-exact with `image_transfom_into_tensor`), so the host cost per sample is the decode.
With `augment=` one more launch warps and re-exposes the batch there (mmdx.augment).
"""
from __future__ import annotations

import io
import json
import os

import numpy as np
import torch

RAW_DATA_COLUMNS = ["image_url", "patient_details", "disease_classification_vector", "report"]
N_DISEASES = 13


def _to_float_vector(x):
    """feature_pipeline.py:47-54: list/tuple/array or JSON text -> 13 floats."""
    if isinstance(x, (list, tuple, np.ndarray)):
        arr = np.asarray(x, dtype=float)
    else:
        arr = np.asarray(json.loads(str(x)), dtype=float)
    if arr.size != N_DISEASES:
        raise ValueError(f"Expected vector of length {N_DISEASES}, got {arr.size}")
    return arr


def enforce_raw_data_columns(df):
    """feature_pipeline.enforce_raw_data_columns (feature_pipeline.py:41-58)."""
    df["image_url"] = df["image_url"].astype(str)
    df["patient_details"] = df["patient_details"].astype(str)
    df["report"] = df["report"].astype(str)
    df["disease_classification_vector"] = df["disease_classification_vector"].map(
        _to_float_vector)
    return df


def load_features_labels_local(parquet_path: str):
    """Local stand-in for `load_raw_data` + `load_features_labels_from_feature_store`
    (feature_pipeline.py:61-66, TP:72-90): read the raw columns (plus `event_time` when
    present), enforce their types, keep the latest row per image_url."""
    import pandas as pd
    import pyarrow.parquet as pq
    names = set(pq.read_schema(parquet_path).names)
    missing = [c for c in RAW_DATA_COLUMNS if c not in names]
    if missing:
        raise ValueError(f"{parquet_path}: missing columns {missing}")
    cols = RAW_DATA_COLUMNS + (["event_time"] if "event_time" in names else [])
    df = pd.read_parquet(parquet_path, columns=cols, engine="pyarrow")
    df = enforce_raw_data_columns(df)
    if "event_time" in df.columns:  # TP:86-88
        df = (df.sort_values("event_time").groupby("image_url", as_index=False).tail(1)
              .reset_index(drop=True))
    return df


def parse_image_key(url: str) -> str:
    """TP:99-103 for s3:// URLs (the key part); any other string is a local path."""
    if url.startswith("s3://"):
        return url[5:].split("/", 1)[1]
    return url


def construct_input_label_pairs_for_image_encoder_dataset(df):
    """TP:122-127: image keys and float32 disease vectors, in row order."""
    keys = [parse_image_key(u) for u in df["image_url"].tolist()]
    labels = [np.asarray(v, dtype=np.float32) for v in df["disease_classification_vector"]]
    return keys, labels


def _label_matrix(df_or_labels):
    """[N, C] float array from a feature dataframe (its disease_classification_vector column)
    or from the labels themselves (an array or a list of rows)."""
    if hasattr(df_or_labels, "columns"):
        df_or_labels = list(df_or_labels["disease_classification_vector"])
    a = np.asarray(df_or_labels, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"labels must be [N, C], got shape {a.shape}")
    return a


def label_stats(df_or_labels):
    """Per-class label counts of a feature dataframe or an [N, C] label array, as int64 [C]
    arrays in a dict: n_pos (label > 0.5), n_neg (0 <= label <= 0.5), n_uncertain (-1),
    n_missing (NaN), and n (rows).  CheXpert-style frames carry all four kinds."""
    a = _label_matrix(df_or_labels)
    nan = np.isnan(a)
    unc = a == -1.0
    pos = a > 0.5
    neg = ~nan & ~unc & ~pos
    return {"n": int(a.shape[0]),
            "n_pos": pos.sum(0).astype(np.int64), "n_neg": neg.sum(0).astype(np.int64),
            "n_uncertain": unc.sum(0).astype(np.int64), "n_missing": nan.sum(0).astype(np.int64)}


def pos_weight_from_stats(stats, cap=20.0):
    """BCE pos_weight per class from label_stats(): min(n_neg / n_pos, cap), and 1 where a class
    has no positives.  float32 [C], ready for mmdx.DiseaseLoss(pos_weight=...)."""
    if not (cap > 0.0 and np.isfinite(cap)):
        raise ValueError(f"cap must be finite and > 0, got {cap}")
    n_pos = np.asarray(stats["n_pos"], dtype=np.float64)
    n_neg = np.asarray(stats["n_neg"], dtype=np.float64)
    w = np.ones_like(n_pos)
    has = n_pos > 0
    w[has] = np.minimum(n_neg[has] / n_pos[has], cap)
    return w.astype(np.float32)


def apply_uncertain(labels, policy):
    """Map the uncertain (-1) labels of an [N, C] array by `policy`:
    None leaves `labels` untouched (the same object is returned, nothing is checked);
    "ignore" maps -1 to NaN (no label: the disease loss and evaluate() leave it out);
    "zeros" / "ones" map -1 to 0 / 1; a float u in (0, 1) maps -1 to the soft label u.
    NaN (not mentioned) stays NaN under every policy.  Returns a new float32 array.  Any value
    outside {-1, NaN} and [0, 1] is a ValueError naming the row and the class."""
    if policy is None:
        return labels
    if isinstance(policy, str):
        fill = {"ignore": np.nan, "zeros": 0.0, "ones": 1.0}.get(policy)
        if fill is None:
            raise ValueError(f"uncertain policy {policy!r}: None, 'ignore', 'zeros', 'ones' or "
                             "a float in (0, 1)")
    elif isinstance(policy, (int, float, np.floating)) and not isinstance(policy, bool):
        fill = float(policy)
        if not (0.0 < fill < 1.0):
            raise ValueError(f"uncertain policy {policy}: a soft label must be in (0, 1)")
    else:
        raise ValueError(f"uncertain policy {policy!r}: None, 'ignore', 'zeros', 'ones' or a "
                         "float in (0, 1)")
    a = np.array(labels, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError(f"labels must be [N, C], got shape {a.shape}")
    unc = a == -1.0
    bad = ~(np.isnan(a) | unc | ((a >= 0.0) & (a <= 1.0)))
    if bad.any():
        r, c = (int(v) for v in np.argwhere(bad)[0])
        raise ValueError(f"label {a[r, c]!r} at row {r}, class {c} is not -1, NaN or in [0, 1]")
    a[unc] = fill
    return a


def open_image(root, key):
    """Image bytes -> PIL image (TP:144-146), from `root/key` (or `key` if absolute)."""
    from PIL import Image
    path = key if os.path.isabs(key) or not root else os.path.join(root, key)
    with open(path, "rb") as f:
        img = Image.open(io.BytesIO(f.read()))
        img.load()
    return img


class CXR_ImageDataset(torch.utils.data.Dataset):
    """TP:131-152 with the S3 bucket replaced by a local directory `image_root` (image keys
    are paths relative to it).  `image_transform` as in the reference (e.g.
    training_pipeline.image_transfom_into_tensor); None returns the decoded PIL image."""

    def __init__(self, img_keys_input, image_root, labels=None, image_transform=None):
        self.img_keys_input = img_keys_input
        self.image_root = image_root
        self.labels = labels
        self.image_transform = image_transform

    def __len__(self):
        assert len(self.img_keys_input) == len(self.labels)
        return len(self.img_keys_input)

    def __getitem__(self, i):
        img = open_image(self.image_root, self.img_keys_input[i])
        x = self.image_transform(img) if self.image_transform is not None else img
        y = torch.tensor(self.labels[i], dtype=torch.float32)
        return x, y


class LocalCXRBatches:
    """Batches of (images [B,3,224,224] fp32 on the GPU, patient_details list[str],
    labels [B,13] fp32 on the GPU) from a feature dataframe and a local image root.  Images
    are decoded on the host (PIL, TP:146) and transformed on the GPU for the whole batch
    (`preprocess_batch`, identical to stacking `image_transfom_into_tensor` outputs).
    `shuffle` draws a seeded permutation per epoch; the last partial batch is kept unless
    `drop_last`.  `augment` (an mmdx.augment.Augment, training only) is applied to every batch
    on the GPU after the transform; it draws from its own Generator, so the shuffle order is the
    one without it, and None yields the transform's output untouched.  `uncertain` is an
    apply_uncertain() policy for -1 labels, applied once here; None (default) yields the stored
    label values bit for bit.  `clahe` (an mmdx.Clahe) equalises the decoded full-resolution
    pixels on the GPU before the transform, hence before `augment`; it is part of the model's
    input definition, so training and validation loaders of one model carry the same setting.
    None yields the unequalised batches, bit for bit what they were without the argument.
    `window` (an mmdx.Window) is the grey-level window of a 16-bit dataset (16-bit PNGs): the
    decoded I;16 images are windowed to 8 bits on the GPU before `clahe` and the transform; like
    `clahe` it is part of the model's input definition.  None (default) takes 8-bit images."""

    def __init__(self, df, image_root, batch_size=32, shuffle=True, seed=0, drop_last=False,
                 device=None, augment=None, uncertain=None, clahe=None, window=None):
        self.keys, self.labels = construct_input_label_pairs_for_image_encoder_dataset(df)
        if uncertain is not None and self.labels:
            self.labels = list(apply_uncertain(np.stack(self.labels), uncertain))
        self.details = df["patient_details"].astype(str).tolist()
        self.image_root = image_root
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self.rng = np.random.default_rng(seed)
        self.drop_last = drop_last
        self.device = device
        self.augment = augment
        if clahe is not None:
            from .clahe import Clahe
            if not isinstance(clahe, Clahe):
                raise TypeError(f"clahe must be an mmdx.Clahe or None, got "
                                f"{type(clahe).__name__}")
        self.clahe = clahe
        if window is not None:
            from .window import Window
            if not isinstance(window, Window):
                raise TypeError(f"window must be an mmdx.Window or None, got "
                                f"{type(window).__name__}")
        self.window = window

    def __len__(self):
        n = len(self.keys)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def order(self):
        n = len(self.keys)
        return self.rng.permutation(n) if self.shuffle else np.arange(n)

    def __iter__(self):
        from .preprocess import preprocess_batch
        dev = self.device
        if dev is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        order = self.order()
        for s in range(0, len(order), self.batch_size):
            idx = order[s:s + self.batch_size]
            if self.drop_last and len(idx) < self.batch_size:
                break
            imgs = [open_image(self.image_root, self.keys[i]) for i in idx]
            if self.window is not None:
                x = preprocess_batch(imgs, dev, clahe=self.clahe, window=self.window)
            else:
                x = preprocess_batch(imgs, dev, clahe=self.clahe)
            if self.augment is not None:
                x = self.augment(x)
            y = torch.from_numpy(np.stack([self.labels[i] for i in idx])).to(dev)
            yield x, [self.details[i] for i in idx], y
