"""CPU: the host half of the validation metrics (mmdx.metrics: AUROC from pair counts, F1
threshold picking, token-id ROUGE-L) on hand-built counts and sequences, and the argument
checks of the two metric entry points, which precede any HIP call and so run without a GPU."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-modal-medical-imaging-and-report-ml-diagnosis-system_amd")


def _counts(rows):
    """[(u2, n_pos, n_neg, n_nan)] per class + the micro row of the same items pooled as if
    every class used one score scale (enough for the host arithmetic under test)."""
    micro = [sum(r[0] for r in rows), sum(r[1] for r in rows), sum(r[2] for r in rows),
             sum(r[3] for r in rows)]
    return np.array(list(rows) + [micro], dtype=np.int64)


# ----------------------------------------------------------------------------- AUROC
def test_auroc_perfect_inverted_tied():
    from mmdx.metrics import auroc_from_counts
    # 3 positives x 4 negatives = 12 pairs: all won (u2 = 24), all lost (0), all tied (12)
    k = np.array([[24, 3, 4, 0], [0, 3, 4, 0], [12, 3, 4, 0], [36, 9, 12, 0]], dtype=np.int64)
    per_class, macro, micro = auroc_from_counts(k)
    assert per_class == [1.0, 0.0, 0.5]
    assert macro == 0.5
    assert micro == 36 / (2 * 9 * 12)


def test_auroc_tied_is_exactly_half_at_odd_sizes():
    from mmdx.metrics import auroc_from_counts
    per_class, _, micro = auroc_from_counts(_counts([(7 * 11, 7, 11, 0)]))
    assert per_class == [0.5] and micro == 0.5


def test_auroc_class_without_positives_is_nan_and_left_out_of_macro():
    from mmdx.metrics import auroc_from_counts
    k = np.array([[24, 3, 4, 0], [0, 0, 7, 0], [0, 7, 0, 0], [6, 3, 4, 0],
                  [100, 13, 15, 0]], dtype=np.int64)
    per_class, macro, micro = auroc_from_counts(k)
    assert per_class[0] == 1.0 and per_class[3] == 0.25
    assert math.isnan(per_class[1]) and math.isnan(per_class[2])
    assert macro == (1.0 + 0.25) / 2
    assert micro == 100 / (2 * 13 * 15)
    per_class, macro, micro = auroc_from_counts(np.array([[0, 0, 5, 0], [0, 0, 5, 0]]))
    assert math.isnan(per_class[0]) and math.isnan(macro) and math.isnan(micro)


def test_auroc_accepts_a_torch_tensor():
    import torch
    from mmdx.metrics import auroc_from_counts
    k = torch.tensor([[24, 3, 4, 0], [24, 3, 4, 0]])
    assert auroc_from_counts(k) == ([1.0], 1.0, 1.0)


def test_auroc_nan_scores_raise_and_name_the_classes():
    from mmdx.metrics import auroc_from_counts
    k = np.array([[24, 3, 4, 0], [10, 3, 3, 1], [10, 3, 2, 2], [50, 9, 9, 3]], dtype=np.int64)
    with pytest.raises(ValueError, match=r"\[1, 2\]"):
        auroc_from_counts(k)


# ----------------------------------------------------------------------------- thresholds
def test_grid_logits_default_grid():
    from mmdx.metrics import default_grid, grid_logits
    g = default_grid()
    assert len(g) == 99 and g.count(0.5) == 1 and g[0] == 0.01 and g[-1] == 0.99
    z = grid_logits(g)
    assert z.dtype == np.float32 and z[g.index(0.5)] == 0.0
    assert np.all(np.diff(z) > 0)
    want = np.log(np.float64(0.25) / np.float64(0.75)).astype(np.float32)
    assert grid_logits([0.25, 0.5])[0] == want
    with pytest.raises(ValueError):
        grid_logits([0.5, 0.25])


def test_pick_thresholds_maximises_f1():
    from mmdx.metrics import pick_thresholds
    grid = [0.2, 0.4, 0.5, 0.6, 0.8]
    # class 0: 4 positives; F1 per point = 8/14, 8/11, 6/8, 6/7, 2/5 -> 0.6
    # class 1: 2 positives; F1 = 4/12, 4/8, 4/6, 2/4, 0 -> 0.5
    tp = [[4, 4, 3, 3, 1], [2, 2, 2, 1, 0]]
    fp = [[6, 3, 1, 0, 0], [8, 4, 2, 1, 0]]
    r = pick_thresholds(tp, fp, [4, 2], grid)
    assert r["thresholds"] == [0.6, 0.5]
    c0, c1 = r["per_class"]
    assert (c0["precision"], c0["recall"], c0["f1"], c0["n_pos"]) == (1.0, 0.75, 6 / 7, 4)
    assert (c0["precision_at_0p5"], c0["recall_at_0p5"], c0["f1_at_0p5"]) == (0.75, 0.75, 0.75)
    assert (c1["precision"], c1["recall"], c1["f1"]) == (0.5, 1.0, 4 / 6)
    # micro at the chosen points: tp 3 + 2, fp 0 + 2, fn 1 + 0
    assert r["micro"] == {"precision": 5 / 7, "recall": 5 / 6, "f1": 10 / 13}
    # micro at 0.5: tp 3 + 2, fp 1 + 2, fn 1 + 0
    assert r["micro_at_0p5"] == {"precision": 5 / 8, "recall": 5 / 6, "f1": 10 / 14}


def test_pick_thresholds_tie_rule_nearest_half_then_lower():
    from mmdx.metrics import pick_thresholds
    grid = [0.3, 0.4, 0.5, 0.6, 0.7]
    n_pos = [2, 2, 2]
    # class 0: the best F1 (1.0) at 0.3, 0.4 and 0.7 -> 0.4 is nearest 0.5
    # class 1: the best F1 at 0.4 and 0.6, equally near -> the lower one
    # class 2: every point equal -> 0.5 itself
    tp = [[2, 2, 1, 1, 2], [1, 2, 1, 2, 1], [1, 1, 1, 1, 1]]
    fp = [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]]
    assert pick_thresholds(tp, fp, n_pos, grid)["thresholds"] == [0.4, 0.4, 0.5]
    # the same on the default grid, where 0.49 and 0.51 are not equally far from 0.5 in binary
    from mmdx.metrics import default_grid
    g = default_grid()
    tp1 = [[1 if p in (0.49, 0.51, 0.9) else 0 for p in g]]
    assert pick_thresholds(tp1, [[0] * 99], [1], g)["thresholds"] == [0.49]


def test_pick_thresholds_class_without_positives_keeps_half():
    from mmdx.metrics import pick_thresholds
    grid = [0.25, 0.5, 0.75]
    r = pick_thresholds([[0, 0, 0], [3, 2, 1]], [[5, 2, 0], [3, 0, 0]], [0, 3], grid)
    assert r["thresholds"] == [0.5, 0.5]
    assert r["per_class"][0] == {"precision": 0.0, "recall": 0.0, "f1": 0.0, "n_pos": 0,
                                 "precision_at_0p5": 0.0, "recall_at_0p5": 0.0,
                                 "f1_at_0p5": 0.0}
    # min_pos: a class below it keeps 0.5 although another point scores higher
    r = pick_thresholds([[2, 1, 1]], [[0, 1, 1]], [2], grid, min_pos=3)
    assert r["thresholds"] == [0.5]
    assert pick_thresholds([[2, 1, 1]], [[0, 1, 1]], [2], grid)["thresholds"] == [0.25]
    with pytest.raises(ValueError, match="0.5"):
        pick_thresholds([[1, 1]], [[0, 0]], [1], [0.25, 0.75])


# ----------------------------------------------------------------------------- ROUGE-L
def test_rouge_l_identical_disjoint_empty():
    from mmdx.metrics import rouge_l
    assert rouge_l([[5, 6, 7, 8]], [[5, 6, 7, 8]]) == 1.0
    assert rouge_l([[5, 6, 7]], [[8, 9, 10, 11]]) == 0.0
    assert rouge_l([[]], [[5, 6]]) == 0.0
    assert rouge_l([[5, 6]], [[]]) == 0.0
    assert rouge_l([[0, 1, 0]], [[5, 6, 1, -100, -100]]) == 0.0   # only ignored ids
    assert rouge_l([], []) == 0.0


def test_rouge_l_hand_computed_lcs_and_batch_mean():
    import torch
    from mmdx.metrics import rouge_l
    # pred 3 9 4 5 7 (5 tokens), ref 3 4 8 5 6 7 (6 tokens): LCS = 3 4 5 7 = 4
    p, r = 4 / 5, 4 / 6
    f = 2 * p * r / (p + r)
    pred = [0, 3, 9, 4, 5, 7, 1, 0, 0]          # decoder start, eos and pad are ignored
    ref = [3, 4, 8, 5, 6, 7, 1, -100, -100]
    assert rouge_l([pred], [ref]) == f
    # a second row scoring 1 and tensors as inputs: the mean over the batch
    got = rouge_l(torch.tensor([pred, [0, 4, 4, 2, 1, 0, 0, 0, 0]]),
                  torch.tensor([ref, [4, 4, 2, 1, -100, -100, -100, -100, -100]]))
    assert got == (f + 1.0) / 2
    # order matters: the reversed sequence shares only single tokens
    assert rouge_l([[1, 5, 6, 7]], [[7, 6, 5]]) == 2 * (1 / 3) * (1 / 3) / (2 / 3)
    with pytest.raises(ValueError):
        rouge_l([[1]], [[1], [2]])


# ----------------------------------------------------------------------------- C ABI checks
@pytest.fixture(scope="module")
def lib():
    import mmdx
    if not os.path.exists(mmdx._lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], check=True)
    return mmdx._lib.lib()


def _rejected(lib, rc, needle):
    assert rc != 0
    msg = lib.mmdx_last_error().decode()
    assert needle in msg, msg


def test_auroc_pairs_rejects_bad_arguments(lib):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    f = lib.mmdx_auroc_pairs
    _rejected(lib, f(None, p, 4, 2, p, None), "null")
    _rejected(lib, f(p, None, 4, 2, p, None), "null")
    _rejected(lib, f(p, p, 4, 2, None, None), "null")
    _rejected(lib, f(p, p, 0, 2, p, None), "empty")
    _rejected(lib, f(p, p, 4, 0, p, None), "empty")
    _rejected(lib, f(p, p, -3, 2, p, None), "empty")
    _rejected(lib, f(p, p, 4, 65, p, None), "C = 65")
    _rejected(lib, f(p, p, 2 ** 24 + 1, 1, p, None), "2^24")
    _rejected(lib, f(p, p, 2 ** 20 + 1, 16, p, None), "2^24")


def test_confusion_grid_rejects_bad_arguments(lib):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    f = lib.mmdx_confusion_grid
    for k in (0, 1, 4, 6, 7):
        args = [p, p, 4, 2, p, 3, p, p, None]
        args[k] = None
        _rejected(lib, f(*args), "null")
    _rejected(lib, f(p, p, 0, 2, p, 3, p, p, None), "empty")
    _rejected(lib, f(p, p, 4, 65, p, 3, p, p, None), "C = 65")
    _rejected(lib, f(p, p, 2 ** 24 + 1, 1, p, 3, p, p, None), "2^24")
    _rejected(lib, f(p, p, 4, 2, p, 0, p, p, None), "T = 0")
    _rejected(lib, f(p, p, 4, 2, p, 257, p, p, None), "T = 257")


def test_functional_wrappers_refuse_cpu_tensors():
    import torch
    import mmdx.functional as F
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        F.auroc_counts(z, z)
    with pytest.raises(RuntimeError, match="GPU"):
        F.confusion_grid(z, z, torch.zeros(2))
