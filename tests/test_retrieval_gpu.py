"""GPU: mmdx_topk_similar (functional.topk_similar) against the float64 definition
(mmdx.retrieval.reference_search): exact integer cases at every tile and block edge, unit
gaussian rows within the derived fp32 accumulation bound, independence of batch, grid and
slicing, the rejections; then CaseIndex.build, inference_similar and the driver end to end."""
import io
import json
import math
import os

import numpy as np
import pytest
import torch

import mmdx
import mmdx.functional as F
from mmdx.retrieval import CaseIndex, model_fingerprint, reference_search

import retrieval_cases as RC

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BUCKET = "medical-ml-proj-bucket"
R = RC.R
FLOAT_SEEDS = RC.FLOAT_SEEDS


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _run(q, x, k, ex, dtype, dev, out=None):
    s, i = F.topk_similar(q.to(dtype).to(dev), x.to(dtype).to(dev), k,
                          None if ex is None else ex.to(dev), out=out)
    return s.cpu(), i.cpu()


def test_rows_per_block_is_the_one_the_cases_assume():
    assert F.topk_rows_per_block() == R


# ----------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("dtype", list(RC.DTYPES))
@pytest.mark.parametrize("case", range(len(RC.EXACT)), ids=[
    "N{}-d{}-nq{}-k{}{}".format(n, d, nq, k, "-ex" if e else "") for n, d, nq, k, e in RC.EXACT])
def test_exact_integer_cases_equal_the_reference_bit_for_bit(dev, case, dtype):
    q, x, ex, k, ref_s, ref_i = RC.exact_case(case)
    s, i = _run(q, x, k, ex, RC.DTYPES[dtype], dev)
    assert np.array_equal(i.numpy().astype(np.int64), ref_i)
    # integer dots below 2^24: the fp32 score is the float64 one exactly, +0.0 for zero
    assert np.array_equal(_bits(s), ref_s.astype(np.float32).view(np.int32))


def test_nan_and_infinite_scores_order_as_the_reference_says(dev):
    q, x, _ = RC.int_inputs(200, 32, 3)
    x[5, 0], x[77, 3], x[130, 1] = math.nan, math.inf, -math.inf
    x[131] = 0
    q[:, :4] = torch.tensor([[1.0, 1, 1, 1], [-1, 1, 1, -1], [0, 1, 1, 0]])
    for dtype in RC.DTYPES.values():
        ref_s, ref_i = reference_search(q.to(dtype), x.to(dtype), 64)
        s, i = _run(q, x, 64, None, dtype, dev)
        assert np.array_equal(i.numpy().astype(np.int64), ref_i)
        assert np.array_equal(_bits(s), ref_s.astype(np.float32).view(np.int32))
        ref_s, ref_i = reference_search(q.to(dtype), x.to(dtype)[:136], 64)
        s, i = _run(q, x[:136], 64, None, dtype, dev)       # two chunks, the second ragged
        assert np.array_equal(i.numpy().astype(np.int64), ref_i)


# ----------------------------------------------------------------------------- float cases
@pytest.mark.parametrize("dtype", list(RC.DTYPES))
def test_gaussian_rows_within_the_accumulation_bound(dev, dtype):
    """Measured (MI355X), worst |score - reference| / bound over the three seeds and both k:
    see profiles/retrieval_parity.txt."""
    worst = 0.0
    for seed in FLOAT_SEEDS[dtype]:
        q, x = RC.gaussian_inputs(5000, 1024, 17, RC.DTYPES[dtype], seed)
        S, B = RC.score_matrix(q, x), RC.accumulation_bound(q, x)
        for k in (5, 64):
            s, i = _run(q, x, k, None, RC.DTYPES[dtype], dev)
            s, i = s.numpy().astype(np.float64), i.numpy().astype(np.int64)
            rows = np.arange(17)[:, None]
            assert (i >= 0).all() and all(len(set(r)) == k for r in i.tolist())
            err, bound = np.abs(s - S[rows, i]), B[rows, i]
            worst = max(worst, float((err / bound).max()))
            print(f"{dtype} seed {seed} k {k}: worst error / bound {(err / bound).max():.4f}, "
                  f"largest bound {B.max():.3e}")
            assert (err <= bound).all()
            # no unreturned row beats the k-th returned one by more than the two bounds
            kth, kb = S[np.arange(17), i[:, -1]], B[np.arange(17), i[:, -1]]
            over = S - kth[:, None] - (B + kb[:, None])
            over[rows, i] = -np.inf
            assert (over <= 0).all()
            if k == 5:
                ok = RC.separated_queries(S, B, 5)
                print(f"  separated queries: {sum(ok)} of 17")
                assert sum(ok) >= 14, "vacuous: too few separated queries"
                ref_i = reference_search(q, x, 5)[1]
                for j in range(17):
                    if ok[j]:
                        assert i[j].tolist() == ref_i[j].tolist(), (seed, j)


# ----------------------------------------------------------------------------- independence
@pytest.fixture(scope="module")
def gauss17(dev):
    q, x = RC.gaussian_inputs(5000, 1024, 17, torch.float16, 0)
    qd, xd = q.to(dev), x.to(dev)
    ex = torch.arange(17, dtype=torch.int32, device=dev) * 7 - 1     # -1, 6, 13, ...
    s, i = F.topk_similar(qd, xd, 64, ex)
    return qd, xd, ex, s.clone(), i.clone()


def test_two_runs_give_equal_bytes(gauss17):
    qd, xd, ex, s0, i0 = gauss17
    s, i = F.topk_similar(qd, xd, 64, ex)
    assert torch.equal(_as_i32(s), _as_i32(s0)) and torch.equal(i, i0)


def _as_i32(t):
    return t.contiguous().view(torch.int32)


def test_a_query_alone_equals_its_row_of_the_batch(gauss17):
    qd, xd, ex, s0, i0 = gauss17
    for j in (0, 5, 15, 16):
        s, i = F.topk_similar(qd[j:j + 1], xd, 64, ex[j:j + 1])
        assert torch.equal(_as_i32(s)[0], _as_i32(s0)[j]) and torch.equal(i[0], i0[j]), j
    s, i = F.topk_similar(qd[3:12], xd, 5, ex[3:12])            # another nq and another k
    assert torch.equal(_as_i32(s), _as_i32(s0)[3:12, :5]) and torch.equal(i, i0[3:12, :5])


def test_slices_merged_on_the_host_equal_the_whole_index(gauss17):
    qd, xd, _, _, _ = gauss17
    whole_s, whole_i = F.topk_similar(qd, xd, 64)
    a, b = R + 3, 3 * R - 1
    parts = []
    for lo, hi in ((0, a), (a, b), (b, xd.shape[0])):
        s, i = F.topk_similar(qd, xd[lo:hi], 64)
        i = i.cpu().numpy().astype(np.int64)
        parts.append((s.cpu().numpy(), np.where(i >= 0, i + lo, -1)))
    ms, mi = RC.merge_host(parts, 64)
    assert np.array_equal(mi, whole_i.cpu().numpy().astype(np.int64))
    assert np.array_equal(ms.view(np.int32), _bits(whole_s))


def test_a_run_after_another_grid_on_the_same_stream_is_still_right(gauss17):
    qd, xd, ex, s0, i0 = gauss17
    ws = []
    for n in (1, R + 1, 700, 5000):                # 1, 2, 6 and 40 select blocks, back to back
        ws.append(F.topk_similar(qd, xd[:n], 64, torch.clamp(ex, max=n - 1)))
    assert torch.equal(_as_i32(ws[-1][0]), _as_i32(s0)) and torch.equal(ws[-1][1], i0)
    ref_s, ref_i = reference_search(qd, xd[:R + 1], 64, torch.clamp(ex, max=R))
    assert np.array_equal(ws[1][1].cpu().numpy().astype(np.int64), ref_i)


def test_out_tensors_are_filled_in_place(gauss17):
    qd, xd, ex, s0, i0 = gauss17
    s = torch.zeros(17, 64, device=qd.device)
    i = torch.zeros(17, 64, dtype=torch.int32, device=qd.device)
    rs, ri = F.topk_similar(qd, xd, 64, ex, out=(s, i))
    assert rs is s and ri is i
    assert torch.equal(_as_i32(s), _as_i32(s0)) and torch.equal(i, i0)


# ----------------------------------------------------------------------------- rejections
def test_every_limit_and_wrong_operand_raises_before_any_launch(dev):
    q = torch.ones(4, 64, dtype=torch.float16, device=dev)
    x = torch.ones(10, 64, dtype=torch.float16, device=dev)
    s = torch.full((4, 3), 7.0, device=dev)
    i = torch.full((4, 3), 7, dtype=torch.int32, device=dev)
    ex = torch.full((4,), -1, dtype=torch.int32, device=dev)
    out = (s, i)

    def bad(exc, *a, **kw):
        with pytest.raises(exc):
            F.topk_similar(*a, **{"out": out, **kw})

    bad(TypeError, q.double(), x.double(), 3)                        # dtype
    bad(TypeError, q.float(), x, 3)                                  # unequal dtypes
    bad(TypeError, q, x, 3, exclude=ex.long())
    bad(TypeError, q, x, 3.0)
    bad(TypeError, q, x, 3, out=(s, i.long()))
    bad(TypeError, q, x, 3, out=(s.half(), i))
    bad(ValueError, q.cpu(), x, 3)                                   # device
    bad(ValueError, q, x.cpu(), 3)
    bad(ValueError, q, x, 3, exclude=ex.cpu())
    bad(ValueError, q, x, 3, out=(s.cpu(), i))
    bad(ValueError, q.t().contiguous().t(), x, 3)                    # contiguity
    bad(ValueError, q, torch.ones(10, 128, dtype=torch.float16, device=dev)[:, :64], 3)
    bad(ValueError, q, x, 3, exclude=torch.stack([ex, ex], 1)[:, 0])
    bad(ValueError, q, x, 3, out=(torch.full((4, 6), 7.0, device=dev)[:, :3], i))
    bad(ValueError, q[0], x, 3)                                      # shapes
    bad(ValueError, q, x[:, :32], 3)
    bad(ValueError, q, x, 3, exclude=ex[:3])
    bad(ValueError, q, x, 2)                                         # out is [4, 3]
    bad(ValueError, q, x, 3, out=(s, s.view(torch.int32)))           # out aliases itself
    bad(ValueError, q, x, 0)                                         # limits
    bad(ValueError, q, x, 65, out=None)
    bad(ValueError, torch.ones(65, 64, dtype=torch.float16, device=dev), x, 3, out=None)
    bad(ValueError, q[:, :48].contiguous(), x[:, :48].contiguous(), 3)   # d % 32
    bad(ValueError, q[:, :16].contiguous(), x[:, :16].contiguous(), 3)   # d < 32
    wide = torch.ones(2, 4128, dtype=torch.float16, device=dev)
    bad(ValueError, wide, wide, 3, out=None)                             # d > 4096
    bad(ValueError, q, x[:0], 3)                                         # N < 1
    for v in (10, -2):                                                   # exclude in [-1, N)
        e = ex.clone()
        e[2] = v
        bad(ValueError, q, x, 3, exclude=e)
    # the C entry point itself: limits it can see on the host, and a short workspace
    ws = torch.empty(4 * 3 * 8, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def c_call(N=10, d=64, nq=4, k=3, nbytes=ws.numel(), dt=2):
        return mmdx._lib.lib().mmdx_topk_similar(st, dt, q.data_ptr(), x.data_ptr(), N, d, nq, k,
                                                 None, s.data_ptr(), i.data_ptr(),
                                                 ws.data_ptr(), nbytes)
    for kw in (dict(N=0), dict(N=(1 << 24) + 1), dict(d=48), dict(d=16), dict(d=4128),
               dict(nq=0), dict(nq=65), dict(k=0), dict(k=65), dict(nbytes=95), dict(dt=3)):
        assert c_call(**kw) != 0, kw
        assert mmdx._lib.lib().mmdx_last_error().startswith(b"topk_similar"), kw
    torch.cuda.synchronize()
    assert (s == 7.0).all() and (i == 7).all()                           # nothing ran
    assert c_call() == 0
    torch.cuda.synchronize()
    assert (i == torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)).all()
    assert (s == 64.0).all()


# ----------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def tiny(dev):
    torch.manual_seed(0)
    img = mmdx.ImageEncoderCNN("resnet18", 1024, 13).to(dev).eval()
    txt = mmdx.TextEncoderTransformer("bert-base-uncased@2", 512, 13).to(dev).eval()
    fus = mmdx.FusionTransformerModel(1024, 512, 1024, 13, with_report_head=False).to(dev).eval()
    return img, txt, fus


def _frame(tmp, n=5):
    """A feature frame over the two golden radiographs and n - 2 synthetic images."""
    import pandas as pd
    from PIL import Image
    root = tmp / "images"
    (root / "chest-x-ray-images").mkdir(parents=True)
    rng = np.random.default_rng(23)
    rows = []
    for j in range(n):
        key = f"chest-x-ray-images/img{j:02d}.jpg"
        if j < 2:
            data = open(os.path.join(GOLD, f"e{j + 1}.jpg"), "rb").read()
        else:
            arr = rng.integers(0, 256, (250 + 7 * j, 260, 3), dtype=np.uint8)
            buf = io.BytesIO()
            Image.fromarray(arr, "RGB").save(buf, format="JPEG", quality=90)
            data = buf.getvalue()
        (root / key).write_bytes(data)
        vec = (rng.random(13) < 0.4).astype(float).tolist()
        rows.append({"image_url": f"s3://{BUCKET}/{key}",
                     "patient_details": f"{40 + j} year old {'male' if j % 2 else 'female'} "
                                        f"PA view, cough, case {j}",
                     "disease_classification_vector": vec,
                     "report": f"Findings: case {j}."})
    return pd.DataFrame(rows), str(root)


def test_build_equals_from_vectors_of_z_fuse_collected_by_hand(dev, tiny, tmp_path):
    from mmdx.data import LocalCXRBatches
    img, txt, fus = tiny
    df, root = _frame(tmp_path)
    clahe = mmdx.Clahe(clip_limit=2.0, tiles=(4, 4))
    loader = LocalCXRBatches(df, root, batch_size=2, shuffle=False, device=dev, clahe=clahe)
    try:
        img.train()
        fus.train()
        fus.fusion_mlp[2].eval()
        flags = [[m.training for m in top.modules()] for top in tiny]
        idx = CaseIndex.build(img, txt, fus, loader, class_names=list(mmdx.DISEASES))
        assert [[m.training for m in top.modules()] for top in tiny] == flags

        def broken():
            yield next(iter(loader))
            raise RuntimeError("loader broke")
        with pytest.raises(RuntimeError, match="loader broke"):
            CaseIndex.build(img, txt, fus, broken(), keys=loader.keys)
        assert [[m.training for m in top.modules()] for top in tiny] == flags
    finally:
        for top in tiny:
            top.eval()
    zs, ys = [], []
    with torch.no_grad():
        for xb, db, yb in loader:
            tok = {k: v.to(dev) for k, v in
                   mmdx.tokenize_patient_details(list(db), max_len=96).items()}
            zs.append(fus(z_img=img(xb)["embeddings"], z_txt=txt(**tok)["embeddings"],
                          report_labels=None)["z_fuse"].float())
            ys.append(yb)
    want = CaseIndex.from_vectors(torch.cat(zs), torch.cat(ys), loader.keys)
    assert len(idx) == 5 and idx.keys == list(loader.keys)
    assert torch.equal(idx.vectors, want.vectors) and torch.equal(idx.labels, want.labels)
    assert idx.vectors.dtype == torch.float16 and idx.vectors.is_cuda
    assert idx.meta["fingerprint"] == model_fingerprint(img, txt, fus)
    assert idx.meta["clahe"] == clahe.config() and idx.meta["d"] == 1024
    assert idx.meta["class_names"] == list(mmdx.DISEASES)
    with pytest.raises(ValueError, match="shuffling"):
        CaseIndex.build(img, txt, fus, LocalCXRBatches(df, root, batch_size=2, shuffle=True,
                                                       device=dev))
    # the GPU search of the index is the definition's
    r = idx.search(torch.cat(zs)[:3], 4, exclude=[0, -1, 2])
    q = torch.nn.functional.normalize(torch.cat(zs)[:3], dim=1).half()
    ref_i = reference_search(q, idx.vectors, 4, np.array([0, -1, 2]))[1]
    assert r["ids"].cpu().numpy().astype(np.int64).tolist() == ref_i.tolist()
    sa = idx.self_agreement(2)
    cpu = CaseIndex(idx.vectors.cpu(), idx.labels.cpu(), idx.keys, idx.meta).self_agreement(2)
    assert sa["n"] == 5 and sa["precision_at_k"].keys() == set(mmdx.DISEASES)
    assert sa["n_pairs"] == cpu["n_pairs"]


def test_inference_similar_adds_the_neighbours_and_nothing_else(dev, tiny, tmp_path):
    from PIL import Image
    from mmdx.data import LocalCXRBatches
    from mmdx.inference_pipeline import (inference, inference_explained, inference_similar,
                                         load_model_bundle, save_model_bundle)
    img, txt, fus = tiny
    arts = {"class_names": list(mmdx.DISEASES), "thresholds": [0.5] * 13}
    path = save_model_bundle(fus, img, txt, str(tmp_path / "model"), timestamped_copy=False,
                             artifacts=arts)
    bundle = load_model_bundle(path, with_report_head=False)
    df, root = _frame(tmp_path)
    text = df["patient_details"][0]
    pil = Image.open(os.path.join(GOLD, "e1.jpg")).convert("RGB")
    plain = inference(bundle, pil, text)
    plain_x = inference_explained(bundle, pil, text, explain_text=1)
    assert set(plain) == {"report_text", "disease_probs", "disease_vector", "model_version",
                          "report_generated", "report_ids"}
    mods = (bundle["image_encoder"], bundle["text_encoder"], bundle["fusion_model"])
    idx = CaseIndex.build(*mods, LocalCXRBatches(df, root, batch_size=3, shuffle=False,
                                                 device=dev),
                          class_names=list(mmdx.DISEASES))
    assert "fingerprint" not in bundle
    out = inference_similar(bundle, pil, text, idx, k=3)
    assert bundle["fingerprint"] == idx.meta["fingerprint"]          # cached in the bundle
    assert set(out) == set(plain) | {"similar"}
    for key in plain:
        assert out[key] == plain[key], key                           # bit-identical floats
    sim = out["similar"]
    assert [e["rank"] for e in sim] == [1, 2, 3] and sim[0]["key"] == idx.keys[0]
    # the query case is in the index: cosine 1 up to the fp16 rounding of both unit vectors
    # (each element off by at most 2^-11 relative: |1 - q.x| <= 2 * 2^-11 + 2^-22) and the
    # fp32 accumulation (1024 * 2^-24)
    assert abs(sim[0]["score"] - 1.0) <= 2 * 2.0 ** -11 + 2.0 ** -22 + 1024 * 2.0 ** -24
    assert sim[0]["score"] >= sim[1]["score"] >= sim[2]["score"]
    y0 = [float(v) for v in df["disease_classification_vector"][0]]
    assert sim[0]["labels"] == dict(zip(mmdx.DISEASES, y0))
    # inference() and inference_explained() are what they were, also after the call
    assert inference(bundle, pil, text) == plain
    again = inference_explained(bundle, pil, text, explain_text=1)
    assert again.keys() == plain_x.keys() and again["token_relevance"] == \
        plain_x["token_relevance"]
    both = inference_similar(bundle, pil, text, idx, k=2, explain_text=1)
    assert set(both) == set(plain_x) | {"similar"} and both["similar"] == sim[:2]

    # another clahe config, another width, another model: refused before anything runs
    with pytest.raises(ValueError, match="clahe"):
        inference_similar(dict(bundle, clahe={"clip_limit": 2.0, "tiles": [8, 8]}), pil, text,
                          idx)
    other = CaseIndex(idx.vectors, idx.labels, idx.keys, dict(idx.meta, d=512))
    with pytest.raises(ValueError, match="wide"):
        inference_similar(bundle, pil, text, other)
    with pytest.raises(TypeError):
        inference_similar(bundle, pil, text, {"vectors": idx.vectors})
    w = bundle["fusion_model"].disease_head.weight
    changed = dict(bundle)
    changed.pop("fingerprint")
    try:
        with torch.no_grad():
            w[0, 0] += 1.0
        with pytest.raises(ValueError, match="fingerprint"):
            inference_similar(changed, pil, text, idx)
    finally:
        with torch.no_grad():
            w[0, 0] -= 1.0


@pytest.fixture(scope="module")
def feature_group(tmp_path_factory):
    import pandas as pd
    from PIL import Image
    root = tmp_path_factory.mktemp("retrieval_driver")
    mirror = root / "s3"
    (mirror / BUCKET / "chest-x-ray-images").mkdir(parents=True)
    rng = np.random.default_rng(29)
    rows = []
    for j in range(6):
        key = f"chest-x-ray-images/img{j:02d}.jpg"
        if j == 0:
            data = open(os.path.join(GOLD, "e1.jpg"), "rb").read()
        else:
            arr = rng.integers(0, 256, (250 + 5 * j, 270, 3), dtype=np.uint8)
            buf = io.BytesIO()
            Image.fromarray(arr, "RGB").save(buf, format="JPEG", quality=90)
            data = buf.getvalue()
        (mirror / BUCKET / key).write_bytes(data)
        vec = (rng.random(13) < 0.4).astype(float).tolist()
        rows.append({"image_url": f"s3://{BUCKET}/{key}",
                     "patient_details": f"{50 + j} year old male PA view, cough, case {j}",
                     "disease_classification_vector": json.dumps(vec),
                     "report": f"Findings: case {j}. The lungs are clear."})
    pq = root / "features.parquet"
    pd.DataFrame(rows).to_parquet(pq)
    return root, mirror, pq


def test_driver_writes_a_loadable_case_index_only_when_asked(dev, feature_group):
    from mmdx.inference_pipeline import load_model_bundle
    root, mirror, pq = feature_group
    outs = {}
    old = dict(os.environ)
    try:
        for name, kw in (("plain", {}), ("index", {"case_index": True})):
            os.environ.update(MMDX_FEATURES_PARQUET=str(pq), MMDX_S3_MIRROR=str(mirror),
                              AWS_S3_BUCKET_NAME=BUCKET,
                              MMDX_MODEL_REGISTRY=str(root / name / "registry"),
                              MMDX_MODEL_DIR=str(root / name / "model"))
            torch.manual_seed(0)
            outs[name] = mmdx.training_pipeline.training_tests(
                num_steps=1, b_fusion=3, batch_size=4, image_backbone="resnet18",
                text_model="bert-base-uncased@2",
                gen_kwargs=dict(max_new_tokens=4, min_new_tokens=1, num_beams=2), verbose=False,
                **kw)
            torch.cuda.synchronize()
    finally:
        os.environ.clear()
        os.environ.update(old)
    plain, out = outs["plain"], outs["index"]
    assert "case_index" not in plain and set(out) == set(plain) | {"case_index"}
    assert sorted(p.name for p in (root / "plain" / "model").iterdir() if
                  "case_index" in p.name) == []
    info = out["case_index"]
    assert info["path"] == str(root / "index" / "model" / "case_index.pt") and info["n"] == 3
    assert info["self_agreement"]["k"] == 2 and info["self_agreement"]["n"] == 3
    idx = CaseIndex.load(info["path"], device=dev)
    assert len(idx) == 3 and idx.meta["d"] == 1024 and idx.meta["clahe"] is None
    assert idx.meta["class_names"] == list(mmdx.DISEASES)
    assert all(k.startswith(f"s3://{BUCKET}/") for k in idx.keys)
    bundle = load_model_bundle(str(root / "index" / "model" / "model_bundle.pt"))
    assert idx.meta["fingerprint"] == model_fingerprint(
        bundle["image_encoder"], bundle["text_encoder"], bundle["fusion_model"])
