"""CPU: the float64 definition of the similar-case search (mmdx.retrieval.reference_search) on
hand-made cases, and CaseIndex without a GPU: from_vectors, add, save / load, self_agreement
on a planted index, the model fingerprint, and the C entry points' host-only shape checks."""
import inspect
import math

import numpy as np
import pytest
import torch

import mmdx
from mmdx import retrieval as RT
from mmdx.retrieval import CaseIndex, reference_search

import retrieval_cases as RC


# ----------------------------------------------------------------------------- the definition
def test_reference_ties_resolve_to_the_lower_id():
    x = np.zeros((6, 32))
    x[:, 0] = [1, 2, 2, 1, 2, 0]
    q = np.zeros((1, 32))
    q[0, 0] = 1
    s, ids = reference_search(q, x, 4)
    assert ids.tolist() == [[1, 2, 4, 0]] and s.tolist() == [[2.0, 2.0, 2.0, 1.0]]


def test_reference_signed_zeros_tie_and_are_reported_as_plus_zero():
    x = np.zeros((4, 32))
    x[:, 0] = [-1, 1, -1, 1]          # q = 0: products -0, +0, -0, +0
    q = np.zeros((1, 32))
    s, ids = reference_search(q, x, 4)
    assert ids.tolist() == [[0, 1, 2, 3]]
    assert not np.signbit(s).any() and (s == 0).all()
    q[0, 1] = -0.0
    assert reference_search(q, x, 4)[1].tolist() == [[0, 1, 2, 3]]


def test_reference_nan_scores_come_last_in_id_order_as_minus_inf():
    x = np.zeros((5, 32))
    x[:, 0] = [np.nan, -5, np.nan, 7, -np.inf]
    q = np.zeros((1, 32))
    q[0, 0] = 1
    s, ids = reference_search(q, x, 5)
    # -inf * 1 = -inf is a real score and ties with the NaN rows: id order among the three
    assert ids.tolist() == [[3, 1, 0, 2, 4]]
    assert s.tolist() == [[7.0, -5.0, -math.inf, -math.inf, -math.inf]]


def test_reference_exclude_removes_the_row_and_k_beyond_n_pads():
    x = np.zeros((3, 32))
    x[:, 0] = [3, 2, 1]
    q = np.zeros((2, 32))
    q[:, 0] = [1, -1]
    s, ids = reference_search(q, x, 5, exclude=np.array([0, -1]))
    assert ids.tolist() == [[1, 2, -1, -1, -1], [2, 1, 0, -1, -1]]
    assert s[0].tolist() == [2.0, 1.0, -math.inf, -math.inf, -math.inf]
    assert s[1].tolist() == [-1.0, -2.0, -3.0, -math.inf, -math.inf]
    with pytest.raises(ValueError):
        reference_search(q, x, 2, exclude=np.array([3, 0]))
    with pytest.raises(ValueError):
        reference_search(q, x, 2, exclude=np.array([-2, 0]))
    with pytest.raises(ValueError):
        reference_search(q, x[:, :16], 2)


def test_reference_reads_the_stored_16_bit_values():
    q, x = RC.gaussian_inputs(40, 64, 3, torch.bfloat16, 0)
    s, ids = reference_search(q, x, 7)
    S = RC.score_matrix(q, x)
    for i in range(3):
        assert ids[i].tolist() == np.argsort(-S[i], kind="stable")[:7].tolist()
        assert np.array_equal(s[i], S[i, ids[i]])


def test_host_merge_of_slices_equals_the_whole_reference():
    q, x, _ = RC.int_inputs(300, 32, 4)
    s, ids = reference_search(q, x, 9)
    parts = []
    for a, b in ((0, 131), (131, 200), (200, 300)):
        ps, pi = reference_search(q, x[a:b], 9)
        parts.append((ps.astype(np.float32), np.where(pi >= 0, pi + a, -1)))
    ms, mi = RC.merge_host(parts, 9)
    assert np.array_equal(mi, ids) and np.array_equal(ms, s.astype(np.float32))


# ----------------------------------------------------------------------------- CaseIndex
def _planted():
    """Two clusters of three rows each: rows 0-2 near e0 with label (1, 0), rows 3-5 near e1
    with label (0, 1), except row 5, which carries (1, 1), and row 2, whose class-1 label is
    missing.  Every row's two nearest neighbours are the other two of its cluster."""
    v = torch.zeros(6, 32)
    for i in range(6):
        v[i, i // 3] = 1.0
        v[i, 2 + i] = 0.1 * (1 + i % 3)
    y = torch.tensor([[1, 0], [1, 0], [1, math.nan], [0, 1], [0, 1], [1, 1]], dtype=torch.float32)
    return v, y, [f"case{i}" for i in range(6)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_from_vectors_normalises_and_rounds_once(dtype):
    g = torch.Generator().manual_seed(3)
    v = torch.randn(50, 64, generator=g) * 7
    v[11] = 0
    idx = CaseIndex.from_vectors(v, torch.zeros(50, 2), [str(i) for i in range(50)], dtype=dtype)
    assert idx.vectors.dtype == dtype and idx.meta["dtype"] == str(dtype).replace("torch.", "")
    want = (v / torch.linalg.vector_norm(v, dim=1, keepdim=True).clamp_min(1e-30)).to(dtype)
    assert torch.equal(idx.vectors, want)
    norms = idx.vectors.double().norm(dim=1)
    assert norms[11] == 0 and not idx.vectors[11].any()
    # each element is off by at most half an ulp (relative eps / 2): so is the norm, plus fp32
    eps = torch.finfo(dtype).eps
    rest = torch.cat([norms[:11], norms[12:]])
    assert ((rest - 1).abs() <= eps / 2 + 4 * torch.finfo(torch.float32).eps).all()
    ip = CaseIndex.from_vectors(v, torch.zeros(50, 2), [str(i) for i in range(50)], metric="ip",
                                dtype=dtype)
    assert torch.equal(ip.vectors, v.to(dtype))


def test_from_vectors_rejects_bad_input():
    v, y, keys = _planted()
    for bad in (math.nan, math.inf):
        w = v.clone()
        w[4, 7] = bad
        with pytest.raises(ValueError, match="non-finite"):
            CaseIndex.from_vectors(w, y, keys)
    with pytest.raises(ValueError):
        CaseIndex.from_vectors(v, y, keys[:-1])
    with pytest.raises(ValueError):
        CaseIndex.from_vectors(v, y[:-1], keys)
    with pytest.raises(ValueError):
        CaseIndex.from_vectors(v[:, :24], y, keys)          # d % 32
    with pytest.raises(ValueError):
        CaseIndex.from_vectors(v, y, keys, metric="l2")
    with pytest.raises(TypeError):
        CaseIndex.from_vectors(v, y, keys, dtype=torch.float64)


def test_search_on_a_cpu_index_is_the_reference_and_neighbours_name_the_cases():
    v, y, keys = _planted()
    idx = CaseIndex.from_vectors(v, y, keys, class_names=["a", "b"])
    assert idx.meta == {"metric": "cosine", "dtype": "float16", "d": 32, "n_disease": 2,
                        "class_names": ["a", "b"], "fingerprint": None, "clahe": None}
    r = idx.search(v[[0, 4]] * 3.0, 3, exclude=[0, -1])    # the scale is normalised away
    assert r["scores"].dtype == torch.float32 and r["ids"].dtype == torch.int32
    qn = (v[[0, 4]] / v[[0, 4]].norm(dim=1, keepdim=True)).half()
    s, ids = reference_search(qn, idx.vectors, 3, np.array([0, -1]))
    assert r["ids"].tolist() == ids.tolist() == [[1, 2, 3], [4, 3, 5]]
    assert np.array_equal(r["scores"].numpy(), s.astype(np.float32))
    nb = idx.neighbours(v[[0, 4]], 7, exclude=[0, -1])
    assert [len(n) for n in nb] == [5, 6]                  # empty slots are left out
    assert [e["rank"] for e in nb[0]] == [1, 2, 3, 4, 5]
    assert nb[0][1] == {"rank": 2, "key": "case2", "score": float(r["scores"][0, 1]),
                        "labels": {"a": 1.0, "b": None}}
    assert nb[1][0]["key"] == "case4" and abs(nb[1][0]["score"] - 1.0) <= 2 ** -10
    with pytest.raises(ValueError):
        idx.search(v[:, :16], 2)
    with pytest.raises(ValueError):
        idx.search(v, 65)


def test_self_agreement_on_a_planted_index():
    v, y, keys = _planted()
    res = CaseIndex.from_vectors(v, y, keys, class_names=["a", "b"]).self_agreement(2)
    # neighbours: 0 -> {1, 2}, 1 -> {0, 2}, 2 -> {0, 1}, 3 -> {4, 5}, 4 -> {3, 5}, 5 -> {3, 4}
    # Jaccard over the classes labelled in both rows: the six pairs inside cluster 0 give 1
    # (row 2's missing class drops out); 3-4 and 4-3 give 1; 3-5, 4-5, 5-3, 5-4 give 1 / 2
    assert res["n"] == 6 and res["k"] == 2 and res["n_pairs"] == 12
    assert res["label_jaccard_mean"] == (8 * 1.0 + 4 * 0.5) / 12
    # class a: positive queries 0, 1, 2, 5 -> 8 neighbours, positive: 6 (cluster 0) + 0 (3, 4)
    # class b: positive queries 3, 4, 5 -> 6 neighbours, all positive
    assert res["precision_at_k"] == {"a": 6 / 8, "b": 1.0}
    none = CaseIndex.from_vectors(v, torch.zeros(6, 2), keys).self_agreement(1)
    assert math.isnan(none["label_jaccard_mean"])
    assert all(math.isnan(p) for p in none["precision_at_k"].values())


def test_add_grows_past_the_initial_capacity():
    g = torch.Generator().manual_seed(5)
    v = torch.randn(23, 32, generator=g)
    y = (torch.rand(23, 3, generator=g) < 0.5).float()
    keys = [f"k{i}" for i in range(23)]
    whole = CaseIndex.from_vectors(v, y, keys)
    idx = CaseIndex.from_vectors(v[:3], y[:3], keys[:3])
    for a, b in ((3, 4), (4, 11), (11, 23)):
        idx.add(v[a:b], y[a:b], keys[a:b])
    assert len(idx) == 23 and idx.keys == keys
    assert idx._vec.shape[0] >= 23 and idx.vectors.is_contiguous()
    assert torch.equal(idx.vectors, whole.vectors) and torch.equal(idx.labels, whole.labels)
    assert idx.search(v[:5], 4)["ids"].tolist() == whole.search(v[:5], 4)["ids"].tolist()
    with pytest.raises(ValueError):
        idx.add(v[:2, :16], y[:2], keys[:2])
    with pytest.raises(ValueError):
        idx.add(v[:2], y[:2, :2], keys[:2])
    w = v[:2].clone()
    w[0, 0] = math.nan
    with pytest.raises(ValueError, match="non-finite"):
        idx.add(w, y[:2], keys[:2])
    assert len(idx) == 23


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_save_load_round_trip(tmp_path, dtype):
    v, y, keys = _planted()
    idx = CaseIndex.from_vectors(v, y, keys, dtype=dtype, class_names=["a", "b"],
                                 fingerprint="ab" * 32,
                                 clahe={"clip_limit": 2.0, "tiles": [8, 8]})
    idx.add(v[:1] * 2, y[:1], ["again"])            # a capacity beyond the rows is not saved
    path = idx.save(tmp_path / "sub" / "case_index.pt")
    assert sorted(p.name for p in (tmp_path / "sub").iterdir()) == ["case_index.pt"]
    blob = torch.load(path, map_location="cpu", weights_only=True)
    assert blob["vectors"].shape == (7, 32)
    back = CaseIndex.load(path, device="cpu")
    assert back.meta == idx.meta and back.keys == idx.keys
    assert torch.equal(back.vectors, idx.vectors)
    assert torch.equal(torch.isnan(back.labels), torch.isnan(idx.labels))
    assert torch.equal(back.labels.nan_to_num(7.0), idx.labels.nan_to_num(7.0))
    blob["meta"]["d"] = 64
    torch.save(blob, path)
    with pytest.raises(ValueError, match="meta"):
        CaseIndex.load(path, device="cpu")


def test_model_fingerprint_changes_with_one_weight():
    torch.manual_seed(0)
    mods = [torch.nn.Linear(4, 3), torch.nn.Sequential(torch.nn.Linear(3, 2)),
            torch.nn.BatchNorm1d(2)]
    a = RT.model_fingerprint(*mods)
    assert a == RT.model_fingerprint(*mods) and len(a) == 64
    with torch.no_grad():
        mods[1][0].weight[1, 2] += 2.0 ** -20
    b = RT.model_fingerprint(*mods)
    assert b != a
    mods[2].num_batches_tracked += 1                 # buffers count: they are state
    assert RT.model_fingerprint(*mods) != b
    assert RT.model_fingerprint(mods[1], mods[0], mods[2]) != RT.model_fingerprint(*mods)


# ----------------------------------------------------------------------------- surface
def test_public_surface():
    from mmdx.inference_pipeline import inference, inference_explained, inference_similar
    from mmdx.training_driver import training_tests
    import mmdx.functional as F
    assert mmdx.CaseIndex is CaseIndex and mmdx.retrieval is RT
    p = inspect.signature(inference_similar).parameters
    assert list(p) == ["model_bundle", "image_pil", "patient_details", "case_index", "k", "device",
                       "gen_kwargs", "explain", "explain_text"]
    assert p["k"].default == 5
    assert "case_index" not in inspect.signature(inference).parameters
    assert "case_index" not in inspect.signature(inference_explained).parameters
    assert inspect.signature(training_tests).parameters["case_index"].default is None
    assert list(inspect.signature(F.topk_similar).parameters) == ["queries", "index", "k",
                                                                  "exclude", "out"]


def test_workspace_query_is_host_only_and_rejects_unsupported_shapes():
    lib = mmdx._lib.lib()
    assert lib.mmdx_topk_rows_per_block() == RC.R
    ws = lib.mmdx_topk_similar_workspace_size
    assert ws(1, 32, 1, 1) == 8
    assert ws(5000, 1024, 17, 5) == 40 * 17 * 5 * 8          # 40 chunks, one block each
    assert ws(1 << 24, 4096, 64, 64) == 128 * 64 * 64 * 8    # capped: 512 blocks in 4 groups
    assert ws(1 << 18, 1024, 16, 64) == 512 * 16 * 64 * 8
    for bad in ((0, 32, 1, 1), ((1 << 24) + 1, 32, 1, 1), (5, 16, 1, 1), (5, 48, 1, 1),
                (5, 4128, 1, 1), (5, 32, 0, 1), (5, 32, 65, 1), (5, 32, 1, 0), (5, 32, 1, 65)):
        assert ws(*bad) == 0, bad


def test_topk_similar_checks_everything_it_can_on_the_host():
    import mmdx.functional as F
    q, x = torch.zeros(2, 32), torch.zeros(5, 32)
    with pytest.raises(TypeError):
        F.topk_similar(q.double(), x.double(), 1)
    with pytest.raises(TypeError):
        F.topk_similar(q.half(), x, 1)
    with pytest.raises(TypeError):
        F.topk_similar(q, x, 1.0)
    with pytest.raises(TypeError):
        F.topk_similar(q, x, 1, exclude=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        F.topk_similar(q, x[:, :16], 1)
    with pytest.raises(ValueError):
        F.topk_similar(q, x, 0)
    with pytest.raises(ValueError):
        F.topk_similar(q, x, 65)
    with pytest.raises(ValueError, match="GPU"):
        F.topk_similar(q, x, 1)                              # CPU tensors: no fallback here
