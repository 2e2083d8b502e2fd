"""Helper module (like util.py; not a conftest): a float64 numpy restatement of include/him.h "Feature-space set
metrics" -- the plane-mean pooling, the streaming moments, the KID kernel sums -- and of the two measures built on them
(KID, the Frechet distance), written from the definitions; the derived error bounds of the GPU tests; switches that
plant the defects the bounds must catch; seeded inputs.  u = 2^-53 throughout."""
import json
import os

import numpy as np

U = 2.0 ** -53
EPS32 = 2.0 ** -24
FEAT_MAX_DIM = 4096          # HIM_FEAT_MAX_DIM of include/him.h
KID_BAD_INDEX = 1


# ---------------------------------------------------------------------------------------------------------- kernels
def pool(x):
    """(B, C) float64 plane means of x (B, C, h, w)."""
    x = np.asarray(x, np.float64)
    return x.reshape(x.shape[0], x.shape[1], -1).sum(-1) / (x.shape[2] * x.shape[3])


def pool_bound(x):
    """2^-24 |ref| (the one rounding to fp32) + u sum|x| (the double summation, whatever its order: every partial sum of
    the plane is below sum|x|, a tree over h w terms rounds fewer than h w times, and the division by h w follows)."""
    x = np.asarray(x, np.float64)
    return EPS32 * np.abs(pool(x)) + U * np.abs(x).reshape(x.shape[0], x.shape[1], -1).sum(-1)


def moments(feat, rowmap='f64'):
    """(sum (D,), second (D, D)) in float64.  ``rowmap='f32'`` plants the defect of an epilogue that stores the 16 x 16
    accumulator tiles of the fp64 matrix instruction with the f32 instruction's row formula: the value of tile row
    (lane >> 4) + 4 q lands in row 4 (lane >> 4) + q."""
    X = np.asarray(feat, np.float64)
    second = X.T @ X
    if rowmap == 'f32':
        D = X.shape[1]
        out = second.copy()
        for t in range(0, D, 16):
            for g in range(4):
                for q in range(4):
                    src, dst = t + g + 4 * q, t + 4 * g + q
                    if src < D and dst < D:
                        out[dst] = second[src]
        second = out
    return X.sum(0), second


def moments_bound(feat):
    """(bound of sum, bound of second): (n + 4) u sum_i |x_ia x_ib| -- exact products, n - 1 additions in any order,
    one more into the accumulator, and slack for the reference's own rounding."""
    A = np.abs(np.asarray(feat, np.float64))
    return (len(A) + 4) * U * A.sum(0), (len(A) + 4) * U * (A.T @ A)


def kid_sums(x, y, ix, iy, gamma=0.0, coef0=1.0, keep_diagonal=False):
    """(n_subsets, 3) float64: sum_{i != j} k(x_i, x_j), the same for y, sum_{i, j} k(x_i, y_j) over the rows the tables
    index, k = (gamma a.b + coef0)^3, gamma == 0 meaning 1 / D; NaN for a subset with an index outside its matrix."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    g = 1.0 / x.shape[1] if gamma == 0 else float(gamma)
    out = np.empty((len(ix), 3))
    for s in range(len(ix)):
        if (ix[s] < 0).any() or (ix[s] >= len(x)).any() or (iy[s] < 0).any() or (iy[s] >= len(y)).any():
            out[s] = np.nan
            continue
        X, Y = x[ix[s]], y[iy[s]]
        kxx, kyy, kxy = (g * X @ X.T + coef0) ** 3, (g * Y @ Y.T + coef0) ** 3, (g * X @ Y.T + coef0) ** 3
        if not keep_diagonal:
            kxx, kyy = kxx - np.diag(np.diag(kxx)), kyy - np.diag(np.diag(kyy))
        out[s] = kxx.sum(), kyy.sum(), kxy.sum()
    return out


def kid_sums_bound(x, y, ix, iy, gamma=0.0, coef0=1.0):
    """(n_subsets, 3): (3 D + P + 16) u sum T^3 with T_ij = gamma sum_k |x_ik y_jk| + |coef0| over the P summed pairs: the
    dot product's summation error carried through the cube to first order (3 D), the cube's own roundings (16) and the
    summation of P terms in any order."""
    x, y = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(y, np.float64))
    D = x.shape[1]
    g = 1.0 / D if gamma == 0 else float(gamma)
    out = np.empty((len(ix), 3))
    for s in range(len(ix)):
        X, Y = x[ix[s]], y[iy[s]]
        m = len(X)
        txx, tyy, txy = (g * X @ X.T + abs(coef0)) ** 3, (g * Y @ Y.T + abs(coef0)) ** 3, (g * X @ Y.T + abs(coef0)) ** 3
        out[s] = ((3 * D + m * (m - 1) + 16) * U * (txx.sum() - np.trace(txx)),
                  (3 * D + m * (m - 1) + 16) * U * (tyy.sum() - np.trace(tyy)), (3 * D + m * m + 16) * U * txy.sum())
    return out


# --------------------------------------------------------------------------------------------------------- measures
def subsets(seed, which, n, n_subsets, subset_size):
    """util.metrics.kid_subsets restated."""
    out = np.empty((n_subsets, subset_size), np.int32)
    for s in range(n_subsets):
        out[s] = np.random.RandomState([int(seed) & 0x7fffffff, int(which), s]).permutation(n)[:subset_size]
    return out


def kid_estimates(sums, m):
    """The unbiased MMD^2 estimate per subset from the three sums."""
    s = np.asarray(sums, np.float64)
    return (s[:, 0] + s[:, 1]) / (m * (m - 1.0)) - 2.0 * s[:, 2] / (m * float(m))


def kid_estimates_bound(bounds, m):
    b = np.asarray(bounds, np.float64)
    return b[:, 0] / (m * (m - 1.0)) + b[:, 1] / (m * (m - 1.0)) + 2.0 * b[:, 2] / (m * float(m))


def kid(x, y, n_subsets, subset_size, seed=0, gamma=0.0, coef0=1.0, keep_diagonal=False):
    """(mean, population std, estimates, m) of KID between the row sets x and y."""
    m = min(subset_size, len(x), len(y))
    ix, iy = subsets(seed, 0, len(x), n_subsets, m), subsets(seed, 1, len(y), n_subsets, m)
    est = kid_estimates(kid_sums(x, y, ix, iy, gamma, coef0, keep_diagonal), m)
    return float(est.mean()), float(est.std()), est, m


def gaussian_fit(x, ddof=1):
    x = np.asarray(x, np.float64)
    mu = x.mean(0)
    c = x - mu
    return mu, c.T @ c / (len(x) - ddof)


def frechet_gaussians(mu1, S1, mu2, S2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2), the last term from the (real, non-negative up to rounding)
    eigenvalues of the product itself -- not the route util.metrics.frechet_from_moments takes."""
    lam = np.maximum(np.linalg.eigvals(S1 @ S2).real, 0.0)
    lam[lam < len(lam) * 2.0 ** -52 * lam.max()] = 0.0         # rounding of a null space (fewer rows than dimensions)
    d = mu1 - mu2
    return float(d @ d + np.trace(S1) + np.trace(S2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def frechet(x, y, ddof=1):
    return frechet_gaussians(*(gaussian_fit(x, ddof) + gaussian_fit(y, ddof)))


def frechet_scale(x, y):
    (m1, S1), (m2, S2) = gaussian_fit(x), gaussian_fit(y)
    return float(np.trace(S1) + np.trace(S2) + (m1 - m2) @ (m1 - m2))


# ------------------------------------------------------------------------------------------------ comparison helpers
class RowFile(object):
    """Rows that go straight to a .jsonl file: a line is on disk before its assertion runs."""

    def __init__(self, path):
        self.path = path

    def append(self, row):
        os.makedirs(os.path.dirname(self.path), exist_ok=True)
        with open(self.path, 'a') as f:
            f.write(json.dumps(row) + '\n')


def check_bound(case, tensor, got, ref, bound, rows=None, kernel=None):
    """|got - ref| <= bound element by element; records the worst error, its bound and the worst error / bound."""
    g, r, b = (np.asarray(v, np.float64) for v in (got, ref, bound))
    assert g.shape == r.shape, '%s %s: shape %s against %s' % (case, tensor, g.shape, r.shape)
    err = np.abs(g - r)
    finite = bool(np.isfinite(err).all())
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / b)
    worst = int(np.argmax(ratio)) if finite and err.size else 0
    row = dict(kernel=kernel or tensor, case=case, tensor=tensor, err=float(err.reshape(-1)[worst]) if finite else None,
               bound=float(np.broadcast_to(b, err.shape).reshape(-1)[worst]),
               ratio=float(ratio.reshape(-1)[worst]) if finite else None)
    if rows is not None:
        rows.append(row)
    print('%s %s: err %r bound %r ratio %r' % (case, tensor, row['err'], row['bound'], row['ratio']))
    assert finite, '%s %s: a value is not finite' % (case, tensor)
    assert bool((err <= b).all()), '%s %s: error %.3e > bound %.3e (ratio %.3f)' % (case, tensor, row['err'], row['bound'],
                                                                                    row['ratio'])
    return row


def check_equal(case, tensor, got, want, rows=None, kernel=None):
    """Exact equality of values (the integer cases)."""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same = g.shape == w.shape and bool((g == w).all())
    if rows is not None:
        rows.append(dict(kernel=kernel or tensor, case=case, tensor=tensor, err=0.0 if same else float(np.abs(g - w).max()),
                         bound=0.0, ratio=None))
    assert same, '%s %s: not equal to the integer result at %s' % (case, tensor, np.argwhere(g != w)[:4].tolist())


# ---------------------------------------------------------------------------------------------------- seeded inputs
def maps(seed, B, C, h, w):
    """fp32 feature maps like a ReLU's: non-negative, a different level per channel."""
    g = np.random.default_rng(seed)
    return (np.maximum(g.standard_normal((B, C, h, w)) + 0.5, 0.0) * g.uniform(0.2, 3.0, (1, C, 1, 1))).astype(np.float32)


def features(seed, n, D, shift=0.0, scale=1.0):
    """fp32 descriptor rows (n, D): positive on average, like pooled ReLU features, plus ``shift``."""
    g = np.random.default_rng(seed)
    return (np.abs(g.standard_normal((n, D))) * scale + 0.3 * g.standard_normal((n, D)) + shift).astype(np.float32)


def int_rows(seed, n, D, hi):
    """fp32 rows of integers in [-hi, hi] whose squared norms are all different."""
    g = np.random.default_rng(seed)
    rows, seen = [], set()
    while len(rows) < n:
        r = g.integers(-hi, hi + 1, D)
        q = int((r * r).sum())
        if q not in seen:
            seen.add(q)
            rows.append(r)
    return np.array(rows).astype(np.float32)


def images(seed, B, H, W):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.sin(yy[None, None] * g.uniform(0.05, 0.4, (B, 3, 1, 1)) + xx[None, None] * g.uniform(0.05, 0.4, (B, 3, 1, 1)))
    return (0.6 * base + 0.3 * g.standard_normal((B, 3, H, W))).astype(np.float32)


