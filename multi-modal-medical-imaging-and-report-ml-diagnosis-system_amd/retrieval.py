"""Similar-case retrieval: which earlier cases look like this one.

A `CaseIndex` holds the fused embedding (`FusionTransformerModel.forward(...)["z_fuse"]`, the
post-LayerNorm joint embedding of radiograph and patient details) of every indexed case, its
labels and a key; `search` is an EXACT top-k inner-product search over it, on the GPU one
purpose-built pass over the index (functional.topk_similar, csrc/retrieval.hip), on a CPU
device `reference_search`, the numpy float64 definition the kernel is tested against.

Definition.  score[i, j] = sum_t q[i, t] x[j, t] on the values as stored (rounded to the index
dtype); a NaN score counts as -inf; row exclude[i] is removed for query i; the result is the
first k remaining rows under the total order (score descending, id ascending), where +0.0 and
-0.0 tie (a zero score is reported as +0.0); slots past the number of remaining rows hold id -1
and score -inf.  With metric "cosine" rows and queries are divided by their fp32 L2 norm before
the one rounding to the index dtype, so the score is the cosine up to that rounding.

Embeddings of another model, or of differently equalised pixels, are not comparable: an index
stores the sha256 of the three state dicts it was built with (`model_fingerprint`) and the
loader's CLAHE config, and inference_similar() refuses a bundle that does not match.
"""
from __future__ import annotations

import hashlib
import math
import os

import numpy as np
import torch

__all__ = ["CaseIndex", "reference_search", "model_fingerprint", "METRICS"]

METRICS = ("cosine", "ip")
_DTYPES = (torch.float16, torch.bfloat16, torch.float32)
_CHUNK = 64   # queries per functional.topk_similar call


def _f64(x):
    """The stored values of a tensor or array as float64 (bf16 has no numpy type: via fp32)."""
    if torch.is_tensor(x):
        return x.detach().float().cpu().numpy().astype(np.float64)
    return np.asarray(x).astype(np.float64)


def reference_search(queries, index, k, exclude=None):
    """The definition (module docstring) in numpy float64 on the values as given: returns
    (scores float64 [nq, k], ids int64 [nq, k]).  The order is a stable sort on the negated
    score, so equal scores keep ascending ids; -0.0 is folded into +0.0 and NaN into -inf
    first."""
    q, x = _f64(queries), _f64(index)
    if q.ndim != 2 or x.ndim != 2 or q.shape[1] != x.shape[1]:
        raise ValueError(f"reference_search: queries {q.shape} and index {x.shape} are not "
                         f"[nq, d] and [N, d]")
    k = int(k)
    if k < 1:
        raise ValueError(f"reference_search: k = {k}")
    nq, N = q.shape[0], x.shape[0]
    ex = None
    if exclude is not None:
        ex = (exclude.detach().cpu().numpy() if torch.is_tensor(exclude)
              else np.asarray(exclude)).astype(np.int64).reshape(-1)
        if ex.shape != (nq,) or np.any(ex < -1) or np.any(ex >= N):
            raise ValueError(f"reference_search: exclude must be [{nq}] with entries in "
                             f"[-1, {N})")
    with np.errstate(invalid="ignore", over="ignore"):
        s = q @ x.T
    s = np.where(np.isnan(s), -np.inf, s) + 0.0
    scores = np.full((nq, k), -np.inf, dtype=np.float64)
    ids = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        order = np.argsort(-s[i], kind="stable")
        if ex is not None and ex[i] >= 0:
            order = order[order != ex[i]]
        m = min(k, order.size)
        ids[i, :m] = order[:m]
        scores[i, :m] = s[i, order[:m]]
    return scores, ids


def model_fingerprint(image_encoder, text_encoder, fusion_model):
    """sha256 (hex) over the three state dicts: per module, per key in sorted order, the key, the
    dtype, the shape and the tensor's CPU bytes.  One changed weight changes it."""
    h = hashlib.sha256()
    for name, m in (("image", image_encoder), ("text", text_encoder), ("fusion", fusion_model)):
        sd = m.state_dict()
        for key in sorted(sd):
            t = sd[key].detach().contiguous().cpu()
            h.update(f"{name}.{key}|{t.dtype}|{tuple(t.shape)}|".encode())
            h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _normalise(v32, metric):
    """fp32 rows divided by their fp32 L2 norm for "cosine" (an all-zero row stays zero)."""
    if metric == "ip":
        return v32
    n = torch.linalg.vector_norm(v32, dim=1, keepdim=True)
    return v32 / torch.where(n > 0, n, torch.ones_like(n))


def _check_rows(vectors, labels, keys, d=None, C=None):
    if not torch.is_tensor(vectors) or vectors.dim() != 2 or not vectors.is_floating_point():
        raise ValueError("CaseIndex: vectors must be a floating-point tensor [N, d]")
    N = vectors.shape[0]
    if d is not None and vectors.shape[1] != d:
        raise ValueError(f"CaseIndex: vectors are {vectors.shape[1]} wide, the index {d}")
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.shape[0] != N:
        raise ValueError(f"CaseIndex: labels must be a tensor [{N}, C]")
    if C is not None and labels.shape[1] != C:
        raise ValueError(f"CaseIndex: labels have {labels.shape[1]} classes, the index {C}")
    keys = [str(s) for s in keys]
    if len(keys) != N:
        raise ValueError(f"CaseIndex: {len(keys)} keys for {N} rows")
    # one device reduction: the only host sync of a build
    if not bool(torch.isfinite(vectors).all()):
        raise ValueError("CaseIndex: a vector has a non-finite entry")
    return keys


class CaseIndex:
    """vectors [N, d] (index dtype, on the device), labels [N, C] fp32 (NaN = no label), keys
    (list of str) and meta {metric, dtype, d, n_disease, class_names, fingerprint, clahe} plus
    "window" when the index was built from windowed 16-bit images (an index without the key
    was not: meta.get("window") is None)."""

    def __init__(self, vectors, labels, keys, meta):
        self._vec, self._lab, self._n = vectors, labels, vectors.shape[0]
        self.keys = list(keys)
        self.meta = dict(meta)

    # ------------------------------------------------------------------ construction
    @property
    def vectors(self):
        return self._vec[:self._n]

    @property
    def labels(self):
        return self._lab[:self._n]

    def __len__(self):
        return self._n

    @classmethod
    def from_vectors(cls, vectors, labels, keys, metric="cosine", dtype=torch.float16,
                     class_names=None, fingerprint=None, clahe=None, window=None):
        """Index the rows of `vectors` [N, d] (any float dtype; they are taken to fp32 first).
        "cosine" divides each row by its fp32 L2 norm, then rounds ONCE to `dtype` (an all-zero
        row stays zero); "ip" only rounds.  A non-finite input is a ValueError."""
        if metric not in METRICS:
            raise ValueError(f"CaseIndex: metric must be one of {METRICS}, got {metric!r}")
        if dtype not in _DTYPES:
            raise TypeError(f"CaseIndex: dtype must be one of {_DTYPES}, got {dtype}")
        keys = _check_rows(vectors, labels, keys)
        N, d = vectors.shape
        if N < 1 or d % 32 or not 32 <= d <= 4096:
            raise ValueError(f"CaseIndex: N = {N}, d = {d}: N >= 1, d a multiple of 32 in "
                             f"[32, 4096]")
        C = labels.shape[1]
        names = list(class_names) if class_names is not None else [str(c) for c in range(C)]
        if len(names) != C:
            raise ValueError(f"CaseIndex: {len(names)} class_names for {C} classes")
        vec = _normalise(vectors.detach().float(), metric).to(dtype).contiguous()
        lab = labels.detach().to(device=vec.device, dtype=torch.float32).contiguous()
        meta = {"metric": metric, "dtype": str(dtype).replace("torch.", ""), "d": int(d),
                "n_disease": int(C), "class_names": names, "fingerprint": fingerprint,
                "clahe": clahe}
        if window is not None:
            meta["window"] = window
        return cls(vec, lab, keys, meta)

    @classmethod
    def build(cls, image_encoder, text_encoder, fusion_model, batches, keys=None, tokenize=None,
              compute_dtype=None, metric="cosine", dtype=torch.float16, class_names=None):
        """Run the three modules over `batches` (as metrics.evaluate does: eval mode, no_grad,
        every `training` flag put back also on an exception, buffers grown on the device, no
        host sync per batch) and index z_fuse with the labels.  `keys` defaults to batches.keys
        when the loader has them and does not shuffle; a shuffling loader without explicit keys
        is a ValueError (its order is not the order of its keys).  Stores the models'
        fingerprint and the loader's CLAHE and window configs."""
        from .metrics import _append_rows
        from .training_pipeline import tokenize_patient_details
        if keys is None:
            if getattr(batches, "shuffle", False):
                raise ValueError("CaseIndex.build: a shuffling loader needs explicit keys")
            keys = getattr(batches, "keys", None)
            if keys is None:
                raise ValueError("CaseIndex.build: the loader has no keys; pass keys=")
        if tokenize is None:
            def tokenize(texts):
                return tokenize_patient_details(texts, max_len=96)
        modules = (image_encoder, text_encoder, fusion_model)
        flags = [(m, m.training) for top in modules for m in top.modules()]
        zbuf = ybuf = None
        n = 0
        try:
            for top in modules:
                top.eval()
            with torch.no_grad():
                for images, details, labels in batches:
                    tok = tokenize(list(details))
                    tok = {k: v.to(images.device) for k, v in tok.items()}
                    z_img = image_encoder(images)["embeddings"]
                    z_txt = text_encoder(**tok)["embeddings"]
                    if compute_dtype is not None:
                        z_img, z_txt = z_img.to(compute_dtype), z_txt.to(compute_dtype)
                    z = fusion_model(z_img=z_img, z_txt=z_txt, report_labels=None)["z_fuse"]
                    if zbuf is None:
                        try:
                            cap = len(batches) * labels.shape[0]
                        except TypeError:
                            cap = 4 * labels.shape[0]
                        cap = max(cap, labels.shape[0])
                        zbuf = torch.empty((cap, z.shape[1]), dtype=torch.float32,
                                           device=z.device)
                        ybuf = torch.empty((cap, labels.shape[1]), dtype=torch.float32,
                                           device=z.device)
                    zbuf, _ = _append_rows(zbuf, n, z.float())
                    ybuf, n = _append_rows(ybuf, n, labels.float())
        finally:
            for m, was in flags:
                m.training = was
        if n == 0:
            raise ValueError("CaseIndex.build: no rows")
        cl = getattr(batches, "clahe", None)
        wn = getattr(batches, "window", None)
        keys = list(keys)
        if getattr(batches, "drop_last", False):
            keys = keys[:n]
        return cls.from_vectors(zbuf[:n], ybuf[:n], keys,
                                metric=metric, dtype=dtype, class_names=class_names,
                                fingerprint=model_fingerprint(*modules),
                                clahe=cl.config() if cl is not None else None,
                                window=wn.config() if wn is not None else None)

    def add(self, vectors, labels, keys):
        """Append rows (normalised and rounded as from_vectors does), doubling the capacity
        when it is full, like metrics._append_rows."""
        from .metrics import _append_rows
        keys = _check_rows(vectors, labels, keys, self.meta["d"], self.meta["n_disease"])
        vec = _normalise(vectors.detach().float().to(self._vec.device),
                         self.meta["metric"]).to(self._vec.dtype)
        lab = labels.detach().to(device=self._lab.device, dtype=torch.float32)
        self._vec, _ = _append_rows(self._vec, self._n, vec)
        self._lab, self._n = _append_rows(self._lab, self._n, lab)
        self.keys.extend(keys)
        return self

    # ------------------------------------------------------------------ persistence
    def save(self, path):
        """One torch.save dict of tensors, lists and plain dicts (loads with
        weights_only=True), written to a tmp file and moved into place with os.replace."""
        blob = {"format": 1, "vectors": self.vectors.detach().cpu().contiguous(),
                "labels": self.labels.detach().cpu().contiguous(), "keys": list(self.keys),
                "meta": dict(self.meta)}
        path = str(path)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = path + ".tmp"
        torch.save(blob, tmp)
        os.replace(tmp, path)
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        blob = torch.load(str(path), map_location="cpu", weights_only=True)
        missing = [k for k in ("vectors", "labels", "keys", "meta") if k not in blob]
        if missing:
            raise ValueError(f"CaseIndex.load: missing keys {missing}")
        meta = blob["meta"]
        vec, lab = blob["vectors"], blob["labels"]
        if (vec.dim() != 2 or str(vec.dtype).replace("torch.", "") != meta.get("dtype")
                or vec.shape[1] != meta.get("d") or tuple(lab.shape) !=
                (vec.shape[0], meta.get("n_disease")) or len(blob["keys"]) != vec.shape[0]):
            raise ValueError("CaseIndex.load: the file's tensors do not match its meta")
        return cls(vec.to(device).contiguous(), lab.to(device).contiguous(), blob["keys"], meta)

    # ------------------------------------------------------------------ search
    def _prepare(self, queries):
        if not torch.is_tensor(queries) or queries.dim() != 2 or queries.shape[1] != \
                self.meta["d"]:
            raise ValueError(f"CaseIndex.search: queries must be [nq, {self.meta['d']}]")
        q = queries.detach().to(self._vec.device).float()
        return _normalise(q, self.meta["metric"]).to(self._vec.dtype).contiguous()

    def _search_prepared(self, q, k, exclude):
        vec = self.vectors
        if vec.device.type != "cuda":   # the CPU path is the definition itself
            s, i = reference_search(q, vec, k, exclude)
            return {"scores": torch.from_numpy(s.astype(np.float32)),
                    "ids": torch.from_numpy(i.astype(np.int32))}
        from . import functional as F
        nq = q.shape[0]
        scores = torch.empty((nq, k), dtype=torch.float32, device=vec.device)
        ids = torch.empty((nq, k), dtype=torch.int32, device=vec.device)
        for s in range(0, nq, _CHUNK):
            e = min(s + _CHUNK, nq)
            F.topk_similar(q[s:e], vec, k, None if exclude is None else exclude[s:e],
                           out=(scores[s:e], ids[s:e]))
        return {"scores": scores, "ids": ids}

    def search(self, queries, k, exclude=None):
        """queries fp32 [nq, d] -> {"scores" fp32 [nq, k], "ids" int32 [nq, k]} on the index's
        device: the queries are normalised in fp32 for "cosine", rounded to the index dtype and
        searched 64 at a time.  exclude: int32 [nq] row ids, -1 = none."""
        k = int(k)
        if not 1 <= k <= 64:
            raise ValueError(f"CaseIndex.search: k = {k} outside [1, 64]")
        q = self._prepare(queries)
        if q.shape[0] < 1:
            raise ValueError("CaseIndex.search: no queries")
        if exclude is not None:
            exclude = torch.as_tensor(exclude, dtype=torch.int32).to(self._vec.device)
            if tuple(exclude.shape) != (q.shape[0],):
                raise ValueError(f"CaseIndex.search: exclude must be [{q.shape[0]}]")
            exclude = exclude.contiguous()
        return self._search_prepared(q, k, exclude)

    def neighbours(self, queries, k, exclude=None):
        """search(), one host copy, and per query a list of {"rank", "key", "score", "labels":
        {class name: value, None where the case has no label}}; empty slots are left out."""
        r = self.search(queries, k, exclude)
        ids = r["ids"].to(torch.int64)
        lab = self._lab[ids.clamp_min(0)]                           # [nq, k, C]
        host = torch.cat([r["scores"].double().reshape(-1), ids.double().reshape(-1),
                          lab.double().reshape(-1)]).cpu().numpy()  # the one copy
        nq, C = ids.shape[0], self._lab.shape[1]
        sc = host[:nq * k].reshape(nq, k)
        idh = host[nq * k:2 * nq * k].reshape(nq, k).astype(np.int64)
        lh = host[2 * nq * k:].reshape(nq, k, C)
        names = self.meta["class_names"]
        out = []
        for i in range(nq):
            row = []
            for j in range(k):
                if idh[i, j] < 0:
                    continue
                row.append({"rank": j + 1, "key": self.keys[idh[i, j]], "score": float(sc[i, j]),
                            "labels": {names[c]: (None if math.isnan(lh[i, j, c])
                                                  else float(lh[i, j, c])) for c in range(C)}})
            out.append(row)
        return out

    def self_agreement(self, k):
        """Every indexed row queries the index with itself excluded (64 at a time; the stored
        rows are the queries as they are).  From the integer ids, on the host in float64:
        "label_jaccard_mean": the mean over (query, neighbour) pairs of |both positive| /
        |either positive| over the classes labelled in both rows (pairs with an empty union
        left out; NaN if none is left); "precision_at_k": per class c, the share of neighbours
        positive for c among the neighbours of the queries positive for c (NaN for a class
        without positive queries).  Also "k", "n" and "n_pairs"."""
        k = int(k)
        n = self._n
        if not 1 <= k <= 64:
            raise ValueError(f"self_agreement: k = {k} outside [1, 64]")
        ex = torch.arange(n, dtype=torch.int32, device=self._vec.device)
        ids = self._search_prepared(self.vectors, k, ex)["ids"].cpu().numpy().astype(np.int64)
        lab = self.labels.detach().cpu().numpy().astype(np.float64)
        C = lab.shape[1]
        known = ~np.isnan(lab)
        pos = known & (lab > 0.5)
        jac_sum, jac_n = 0.0, 0
        hit = np.zeros(C, dtype=np.int64)
        tot = np.zeros(C, dtype=np.int64)
        for i in range(n):
            for j in ids[i]:
                if j < 0:
                    continue
                both = known[i] & known[j]
                union = int(((pos[i] | pos[j]) & both).sum())
                if union:
                    jac_sum += int((pos[i] & pos[j] & both).sum()) / union
                    jac_n += 1
                tot += pos[i]
                hit += pos[i] & pos[j]
        names = self.meta["class_names"]
        return {"k": k, "n": n, "n_pairs": jac_n,
                "label_jaccard_mean": jac_sum / jac_n if jac_n else math.nan,
                "precision_at_k": {names[c]: (hit[c] / tot[c] if tot[c] else math.nan)
                                   for c in range(C)}}
