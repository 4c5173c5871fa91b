"""CPU: the host half of the bootstrap (mmdx.bootstrap): the numpy yardsticks against brute
force, the interval and paired-difference arithmetic on hand-made integers, and every argument
check that precedes a launch (evaluate, the training driver, the two C entry points), which
run without a GPU."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-modal-medical-imaging-and-report-ml-diagnosis-system_amd")


# ----------------------------------------------------------------------------- weights
def test_reference_weights_rows_sum_to_n_and_batches_concatenate():
    from mmdx.bootstrap import reference_weights
    for N in (1, 2, 63, 1000):
        w = reference_weights(8, N, seed=3)
        assert w.dtype == np.int32 and w.shape == (8, N)
        assert (w >= 0).all() and np.array_equal(w.sum(1), [N] * 8)
        parts = np.concatenate([reference_weights(3, N, seed=3, r0=0),
                                reference_weights(5, N, seed=3, r0=3)])
        assert np.array_equal(w, parts)
    assert np.array_equal(reference_weights(4, 1, seed=9), np.ones((4, 1), np.int32))
    a, b = reference_weights(4, 257, seed=1), reference_weights(4, 257, seed=2)
    assert not any(np.array_equal(x, y) for x in a for y in b)
    assert len({r.tobytes() for r in a}) == 4           # replicates differ from each other
    with pytest.raises(ValueError):
        reference_weights(0, 4, seed=0)


def test_reference_weights_draw_is_the_documented_stream():
    """Draw by draw in Python integers: key_r = mix64(seed ^ ((r + 1) G)),
    idx = (mix64(key_r + (k + 1) G) * N) >> 64."""
    from mmdx.bootstrap import GOLDEN, reference_weights
    M = (1 << 64) - 1

    def mix64(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    for seed, r, N in ((7, 0, 5), (0xDEADBEEFCAFEF00D, 11, 300), (2 ** 64 - 1, 4, 4097)):
        key = mix64(seed ^ (((r + 1) * GOLDEN) & M))
        want = np.zeros(N, np.int32)
        for k in range(N):
            want[(mix64((key + (k + 1) * GOLDEN) & M) * N) >> 64] += 1
        assert np.array_equal(reference_weights(1, N, seed, r0=r)[0], want)


def test_reference_weights_variance_is_that_of_resampling():
    """[64, 1024] at seed 7: a weight is Binomial(N, 1 / N), variance 1 - 1 / N; its fourth
    central moment is about 4 (near Poisson(1): 3 + 1), so the sample variance of 65536 weights
    has standard error sqrt(3 / 65536) and the bound is six of them."""
    from mmdx.bootstrap import reference_weights
    w = reference_weights(64, 1024, seed=7).astype(np.float64)
    var = w.var()
    print("weight variance", var, "zero fraction", (w == 0).mean())
    assert abs(var - (1 - 1 / 1024)) <= 6 * math.sqrt(3 / 65536)


# ----------------------------------------------------------------------------- counts
def _brute(s, y, w, pred):
    """The definition as a double loop over (positive, negative) pairs."""
    R = w.shape[0]
    N, C = s.shape
    cols = [(s[:, c], y[:, c] > 0.5, pred[:, c], np.arange(N)) for c in range(C)]
    cols.append((s.reshape(-1), y.reshape(-1) > 0.5, pred.reshape(-1), np.arange(N * C) // C))
    out = np.zeros((R, C + 1, 5), dtype=np.int64)
    for r in range(R):
        for c, (sc, pos, pr, row) in enumerate(cols):
            u2 = wp = wn = tp = fp = 0
            for i in range(len(sc)):
                if sc[i] != sc[i]:
                    continue
                wi = int(w[r, row[i]])
                if not pos[i]:
                    wn += wi
                    fp += wi if pr[i] else 0
                    continue
                wp += wi
                tp += wi if pr[i] else 0
                for j in range(len(sc)):
                    if sc[j] != sc[j] or pos[j]:
                        continue
                    u2 += wi * int(w[r, row[j]]) * (int(sc[i] > sc[j]) + int(sc[i] >= sc[j]))
            out[r, c] = (u2, wp, wn, tp, fp)
    return out


def _tiny(seed, N, C):
    """Scores on four values with both zeros among them, 10 % NaN, a class without positives."""
    g = np.random.default_rng(seed)
    s = g.choice(np.array([-1.0, -0.0, 0.0, 2.5], np.float32), size=(N, C))
    s[g.random((N, C)) < 0.1] = np.nan
    y = (g.random((N, C)) < 0.4).astype(np.float32)
    y[:, 0] = 0.0
    pred = g.random((N, C)) < 0.5
    return s, y, pred


@pytest.mark.parametrize("seed,N,C", [(0, 1, 1), (1, 7, 3), (2, 24, 2), (3, 40, 1)])
def test_reference_counts_equal_brute_force(seed, N, C):
    from mmdx.bootstrap import reference_counts, reference_weights
    s, y, pred = _tiny(seed, N, C)
    w = reference_weights(3, N, seed=seed)
    got = reference_counts(s, y, w, pred)
    assert got.dtype == np.int64 and got.shape == (3, C + 1, 5)
    assert np.array_equal(got, _brute(s, y, w, pred))
    assert not got[:, 0, [0, 1, 3]].any()                # the class without positives
    none = reference_counts(s, y, w)
    assert np.array_equal(none[..., :3], got[..., :3]) and not none[..., 3:].any()
    # continuous scores too (no ties)
    s2 = np.random.default_rng(seed + 50).standard_normal((N, C)).astype(np.float32)
    assert np.array_equal(reference_counts(s2, y, w, pred), _brute(s2, y, w, pred))


def _midrank_row(s, pos):
    """(u2, n_pos, n_neg) of one class from unweighted midranks: the formula of
    tests/test_metrics_gpu.py."""
    nan = np.isnan(s)
    s, pos = s[~nan], pos[~nan]
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    u2 = 0
    if n_pos:
        _, inv, cnt = np.unique(s, return_inverse=True, return_counts=True)
        cum = np.cumsum(cnt).astype(np.int64)
        rank2 = 2 * cum - cnt + 1
        u2 = int(rank2[inv.reshape(-1)][pos].sum()) - n_pos * (n_pos + 1)
    return [u2, n_pos, n_neg]


def test_reference_counts_with_unit_weights_are_the_unweighted_midranks():
    from mmdx.bootstrap import reference_counts
    g = np.random.default_rng(5)
    s = (np.round(g.standard_normal((300, 5)) * 4) / 4).astype(np.float32)
    s[g.random(s.shape) < 0.05] = np.nan
    s[:4, 1] = [0.0, -0.0, np.inf, -np.inf]
    y = (g.random(s.shape) < 0.2).astype(np.float32)
    pos = y > 0.5
    want = [_midrank_row(s[:, c], pos[:, c]) for c in range(5)]
    want.append(_midrank_row(s.reshape(-1), pos.reshape(-1)))
    got = reference_counts(s, y, np.ones((1, 300), np.int32))
    assert np.array_equal(got[0, :, :3], np.array(want, dtype=np.int64))


# ----------------------------------------------------------------------------- intervals
def _boot(rows):
    """[R, C + 1, 5] from per-replicate lists of (u2, w_pos, w_neg, tp, fp) rows."""
    return np.array(rows, dtype=np.int64)


def test_intervals_quantiles_se_and_n_valid():
    from mmdx.bootstrap import intervals
    # one class + micro (the same numbers); 5 replicates with w_pos = 4, w_neg = 5:
    # AUROC = u2 / 40 = 0.1, 0.2, 0.5, 0.7, 1.0
    u2 = [4, 8, 20, 28, 40]
    tp = [0, 1, 2, 3, 4]
    fp = [5, 4, 2, 1, 0]
    b = _boot([[(u, 4, 5, t, f)] * 2 for u, t, f in zip(u2, tp, fp)])
    iv = intervals(b, level=0.5)
    assert iv["level"] == 0.5 and iv["n_replicates"] == 5
    a = iv["auroc_per_class"][0]
    v = np.array([0.1, 0.2, 0.5, 0.7, 1.0])
    # linear quantiles of 5 points at 0.25 / 0.75: exactly the 2nd and 4th order statistics
    assert a == {"lo": 0.2, "hi": 0.7, "se": float(np.std(v, ddof=1)), "n_valid": 5}
    assert iv["auroc_micro"] == a and iv["auroc_macro"] == a
    # level 0.9: positions 0.2 and 3.8 between the order statistics
    a9 = intervals(b, level=0.9)["auroc_per_class"][0]
    assert a9["lo"] == pytest.approx(0.1 + 0.2 * 0.1, abs=1e-15)
    assert a9["hi"] == pytest.approx(0.7 + 0.8 * 0.3, abs=1e-15)
    sens = iv["sensitivity_per_class"][0]
    assert (sens["lo"], sens["hi"], sens["n_valid"]) == (0.25, 0.75, 5)
    spec = iv["specificity_per_class"][0]
    assert (spec["lo"], spec["hi"]) == (1 - 4 / 5, 1 - 1 / 5)
    f1 = [2 * t / (t + f + 4) for t, f in zip(tp, fp)]
    got = iv["f1_micro"]
    assert got["lo"] == sorted(f1)[1] and got["hi"] == sorted(f1)[3]
    assert got["se"] == float(np.std(f1, ddof=1))
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            intervals(b, level=bad)
    with pytest.raises(ValueError):
        intervals(b[..., :4])
    with pytest.raises(ValueError):
        intervals(b.astype(np.float64))


def test_intervals_macro_rule_and_invalid_replicates():
    from mmdx.bootstrap import intervals, replicate_stats
    # two classes; class 1 has no positives in replicate 1 and no negatives in replicate 2
    b = _boot([
        [(8, 2, 2, 1, 1), (4, 2, 2, 2, 0), (0, 4, 4, 3, 1)],     # 1.0 and 0.5 -> macro 0.75
        [(4, 2, 2, 1, 1), (0, 0, 4, 0, 2), (0, 2, 6, 1, 3)],     # 0.5 and nan -> macro 0.5
        [(0, 2, 2, 1, 1), (0, 4, 0, 3, 0), (0, 6, 2, 4, 1)],     # 0.0 and nan -> macro 0.0
    ])
    st = replicate_stats(b)
    assert st["auroc"][:, 0].tolist() == [1.0, 0.5, 0.0]
    assert st["auroc"][0, 1] == 0.5 and np.isnan(st["auroc"][1:, 1]).all()
    assert st["auroc_macro"].tolist() == [0.75, 0.5, 0.0]
    # sensitivity and F1 need positives, specificity needs negatives
    assert np.isnan(st["sensitivity"][1, 1]) and np.isnan(st["f1"][1, 1])
    assert st["specificity"][1, 1] == 0.5
    assert st["sensitivity"][2, 1] == 0.75 and np.isnan(st["specificity"][2, 1])
    assert st["f1"][2, 1] == 6 / 7
    iv = intervals(b)
    c1 = iv["auroc_per_class"][1]
    assert c1["n_valid"] == 1 and all(math.isnan(c1[k]) for k in ("lo", "hi", "se"))
    assert iv["auroc_per_class"][0]["n_valid"] == 3 and iv["auroc_macro"]["n_valid"] == 3
    assert iv["sensitivity_per_class"][1]["n_valid"] == 2
    assert iv["specificity_per_class"][1]["n_valid"] == 2
    # no class defined anywhere: macro has no valid replicate at all
    z = _boot([[(0, 0, 3, 0, 0), (0, 0, 3, 0, 0)]] * 4)
    m = intervals(z)["auroc_macro"]
    assert m["n_valid"] == 0 and math.isnan(m["lo"]) and math.isnan(m["se"])


def test_paired_delta_interval_p_value_and_mismatch():
    from mmdx.bootstrap import paired_delta
    # w_pos = 2, w_neg = 5: AUROC = u2 / 20
    ua = [20, 16, 12, 10, 14, 18]
    ub = [10, 12, 12, 14, 10, 8]
    a = _boot([[(u, 2, 5, 0, 0)] * 2 for u in ua])
    b = _boot([[(u, 2, 5, 0, 0)] * 2 for u in ub])
    d = np.array([(x - y) / 20 for x, y in zip(ua, ub)])     # .5 .2 0 -.2 .2 .5
    r = paired_delta(a, b, level=0.5)
    for leaf in (r["per_class"][0], r["macro"], r["micro"]):
        assert leaf["n_valid"] == 6
        lo, hi = np.quantile(d, [0.25, 0.75])
        assert leaf["lo"] == pytest.approx(lo, abs=1e-15)
        assert leaf["hi"] == pytest.approx(hi, abs=1e-15)
        assert leaf["se"] == pytest.approx(np.std(d, ddof=1), abs=1e-15)
        # #(d <= 0) = 2, #(d >= 0) = 5 -> 2 * 3 / 7
        assert leaf["p_two_sided"] == 2 * 3 / 7
    assert r["level"] == 0.5 and r["n_replicates"] == 6
    same = paired_delta(a, a)["micro"]
    assert same["p_two_sided"] == 1.0 and same["lo"] == same["hi"] == 0.0
    # every difference positive: 2 * (0 + 1) / (6 + 1)
    up = _boot([[(u + 2, 2, 5, 0, 0)] * 2 for u in ua])
    assert paired_delta(up, a)["micro"]["p_two_sided"] == 2 / 7
    other = b.copy()
    other[3, 0, 1] += 1                                     # another resample: w_pos differs
    with pytest.raises(ValueError, match="w_pos"):
        paired_delta(a, other)
    with pytest.raises(ValueError):
        paired_delta(a, b[:5])
    # a class undefined in every replicate: no valid difference, p = 1
    ud = _boot([[(0, 0, 7, 0, 0), (u, 2, 5, 0, 0)] for u in ua])
    leaf = paired_delta(ud, ud)["per_class"][0]
    assert leaf["n_valid"] == 0 and leaf["p_two_sided"] == 1.0 and math.isnan(leaf["lo"])


def test_batch_size_keeps_the_workspace_at_64_mib():
    from mmdx.bootstrap import batch_size
    assert batch_size(1000, 300) == 1000
    assert batch_size(1000, 65536) == 256
    assert batch_size(5, 2 ** 24) == 1 and batch_size(5, 2 ** 24 + 1) == 1
    assert all(batch_size(R, N) * N * 4 <= 64 << 20 for R, N in ((10 ** 6, 4096), (200, 65536)))


# ----------------------------------------------------------------------------- argument checks
def test_evaluate_checks_bootstrap_arguments_before_any_device_work():
    from mmdx.metrics import evaluate

    class Boom:
        def modules(self):
            raise AssertionError("evaluate touched a module before checking its arguments")

    def batches():
        raise AssertionError("evaluate read a batch before checking its arguments")
        yield

    m = Boom()
    for bad in (-1, 1.5, "8", None, True):
        with pytest.raises(ValueError, match="bootstrap"):
            evaluate(m, m, m, batches(), bootstrap=bad)
    for bad in (0.0, 1.0, -0.2, 2, "0.9", None):
        with pytest.raises(ValueError, match="ci_level"):
            evaluate(m, m, m, batches(), bootstrap=8, ci_level=bad)
    with pytest.raises(ValueError, match="bootstrap_seed"):
        evaluate(m, m, m, batches(), bootstrap=8, bootstrap_seed=0.5)


def test_training_tests_bootstrap_needs_validation_rows():
    from mmdx.training_driver import training_tests
    with pytest.raises(ValueError, match="val_rows"):
        training_tests(bootstrap=16, val_rows=0)
    with pytest.raises(ValueError, match="bootstrap"):
        training_tests(bootstrap=-3, val_rows=8)
    with pytest.raises(ValueError, match="bootstrap"):
        training_tests(bootstrap=2.5, val_rows=8)


def test_functional_wrappers_refuse_cpu_tensors_and_bad_arguments():
    import torch
    import mmdx.functional as F
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="GPU"):
        F.bootstrap_plan(z, z)
    with pytest.raises(TypeError):
        F.bootstrap_plan(z.double(), z)
    with pytest.raises(ValueError, match="GPU"):
        F.bootstrap_weights(2, 4, 0, device="cpu")
    with pytest.raises(TypeError):
        F.bootstrap_weights(2.0, 4, 0)
    for R, N, r0 in ((0, 4, 0), (2, 0, 0), (2, 4, -1), (2 ** 13, 2 ** 13 + 1, 0)):
        with pytest.raises(ValueError):
            F.bootstrap_weights(R, N, 0, r0=r0)
    with pytest.raises(TypeError, match="plan"):
        F.bootstrap_counts(None, torch.zeros(2, 4, dtype=torch.int32))


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


def test_bootstrap_weights_rejects_bad_arguments(lib):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    f = lib.mmdx_bootstrap_weights
    _rejected(lib, f(2, 0, 4, 7, None, None), "null")
    _rejected(lib, f(0, 0, 4, 7, p, None), "empty")
    _rejected(lib, f(2, 0, 0, 7, p, None), "empty")
    _rejected(lib, f(-1, 0, 4, 7, p, None), "empty")
    _rejected(lib, f(2, -1, 4, 7, p, None), "r0")
    _rejected(lib, f(2 ** 13, 0, 2 ** 13 + 1, 7, p, None), "2^26")
    _rejected(lib, f(1, 0, 2 ** 26 + 1, 7, p, None), "2^26")


def test_bootstrap_counts_rejects_bad_arguments(lib):
    buf = ctypes.create_string_buffer(1024)
    p = (ctypes.addressof(buf) + 15) & ~15
    f = lib.mmdx_bootstrap_counts
    size = lib.mmdx_bootstrap_counts_workspace_size
    # the transposed weights [N][R rounded up to 8] + the segment partials.  [4, 3]: one segment
    # per column, 3 + 1 columns, two orders; 3 words per replicate
    need = size(2, 4, 3)
    assert need == 4 * 8 * 4 + 2 * 4 * 2 * 3 * 8
    # [4097, 2]: 3 segments of 2048 items per class column, 5 for the 8194 micro items
    assert size(5, 4097, 2) == 4097 * 8 * 4 + 2 * (2 * 3 + 5) * 5 * 3 * 8
    assert size(9, 4, 3) == 4 * 16 * 4 + 2 * 4 * 9 * 3 * 8
    for R, N, C in ((0, 4, 3), (2, 0, 3), (2, 4, 0), (2, 4, 65), (1, 2 ** 24 + 1, 1),
                    (2 ** 13, 2 ** 13 + 1, 1)):
        assert size(R, N, C) == 0
    for k in (0, 1, 2, 6, 7):
        args = [p, p, p, 2, 4, 3, p, p, need, None]
        args[k] = None
        _rejected(lib, f(*args), "null")
    _rejected(lib, f(p, p, p, 0, 4, 3, p, p, need, None), "empty")
    _rejected(lib, f(p, p, p, 2, 0, 3, p, p, need, None), "empty")
    _rejected(lib, f(p, p, p, 2, 4, 0, p, p, need, None), "empty")
    _rejected(lib, f(p, p, p, 2, 4, 65, p, p, need, None), "C = 65")
    _rejected(lib, f(p, p, p, 1, 2 ** 24 + 1, 1, p, p, need, None), "2^24")
    _rejected(lib, f(p, p, p, 1, 2 ** 20 + 1, 16, p, p, need, None), "2^24")
    _rejected(lib, f(p, p, p, 2 ** 13, 2 ** 13 + 1, 1, p, p, need, None), "2^26")
    _rejected(lib, f(p + 4, p, p, 2, 4, 3, p, p, need, None), "16-byte aligned")
    _rejected(lib, f(p, p + 8, p, 2, 4, 3, p, p, need, None), "16-byte aligned")
    _rejected(lib, f(p, p, p, 2, 4, 3, p, p + 8, need, None), "workspace must be 16-byte")
    _rejected(lib, f(p, p, p, 2, 4, 3, p, p, need - 1, None), f"{need} needed")
