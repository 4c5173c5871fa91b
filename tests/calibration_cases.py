"""Shared inputs of tests/test_calibration_{cpu,gpu}.py: the fit cases and a numpy statement of
the reliability bins."""
import numpy as np

# name: (shape, scale, shift, prevalence, sep)
FIT_CASES = {
    "easy": ((300, 13), 1.0, 0.0, 0.2, 1.0),
    "far": ((300, 13), 10.0, 5.0, 0.2, 1.0),
    "rare": ((2000, 13), 3.0, -4.0, 0.01, 1.0),
    "big": ((4096, 13), 2.0, 1.0, 0.15, 1.0),
    "c1": ((300, 1), 1.0, 0.0, 0.2, 1.0),
    "c64": ((300, 64), 1.0, 0.0, 0.2, 1.0),
}


def make_case(shape, scale, shift, prevalence, sep, seed=0):
    """logits = scale * (randn + sep * (2 y - 1)) + shift, labels Bernoulli(prevalence), 10 % of
    the labels NaN ("no label").  float32 [N, C] each."""
    rng = np.random.default_rng(seed)
    y = (rng.random(shape) < prevalence).astype(np.float32)
    z = (scale * (rng.standard_normal(shape) + sep * (2.0 * y - 1.0)) + shift).astype(np.float32)
    y[rng.random(shape) < 0.1] = np.nan
    return z, y


def sigmoid64(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def ref_bins(z, y, edges, scale=None, bias=None):
    """(count, positives, n_nan, sum p, sum (p - y)^2) of every class and, in row C, of all
    classes pooled: z' in float32 as multiply then add, bin = #{edges <= z'}, p in float64."""
    z = np.asarray(z, dtype=np.float32)
    N, C = z.shape
    if scale is not None:
        z = z * np.asarray(scale, np.float32)[None, :]
        z = z + np.asarray(bias, np.float32)[None, :]
    nb = len(edges) + 1
    cnt = np.zeros((C + 1, nb), np.int64)
    pos = np.zeros((C + 1, nb), np.int64)
    sp = np.zeros((C + 1, nb), np.float64)
    sb = np.zeros((C + 1, nb), np.float64)
    n_nan = np.zeros(C + 1, np.int64)
    for c in range(C):
        zc, yc = z[:, c], y[:, c] > 0.5
        ok = ~np.isnan(zc)
        n_nan[c] = int((~ok).sum())
        k = np.searchsorted(edges, zc[ok], side="right")
        p = sigmoid64(zc[ok])
        q = sigmoid64(-zc[ok].astype(np.float64))
        d = np.where(yc[ok], q, p)
        np.add.at(cnt[c], k, 1)
        np.add.at(pos[c], k, yc[ok].astype(np.int64))
        np.add.at(sp[c], k, p)
        np.add.at(sb[c], k, d * d)
    for a in (cnt, pos, sp, sb):
        a[C] = a[:C].sum(0)
    n_nan[C] = n_nan[:C].sum()
    return cnt, pos, n_nan, sp, sb
