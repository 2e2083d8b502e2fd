"""Helper module (like util.py; not a conftest): a float64 numpy restatement of include/him.h's k-nearest-neighbour
entries (him_knn_radii, him_knn_membership) and of the four measures built on them -- improved precision and recall
(Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020) -- written from the definitions; the derived error
bounds of the GPU tests; CPU stand-ins of the kernels with switches that plant the defects the checks must catch; seeded
inputs and the list of cases the CPU and the GPU tests share.

Definitions.  X (nx, D) real, Y (ny, D) generated, fp32 rows; d2(a, b) the squared Euclidean distance.
  radius      r2_k(X)_i = the k-th smallest d2(x_i, x_j) over j != i, self excluded by POSITION (a duplicate row is a
              neighbour at distance 0);
  indicator   I(Q -> R)[j, i] = [ d2(q_j, r_i) <= r2_k(R)_i ]: the radius is the reference row's, the comparison is <=;
  counts      row_count[j] = sum_i I[j, i], col_count[i] = sum_j I[j, i];
  Y -> X      precision = mean_j [row_count_j > 0], density = sum_j row_count_j / (k ny), coverage = mean_i [col_count_i > 0];
  X -> Y      recall = mean_j [row_count_j > 0] (j over the real rows, against the generated rows' radii).
A row with a non-finite feature takes part in no true comparison: every distance to or from it is NaN, it is nobody's
neighbour, and its own radius is NaN; a row with fewer than k finite neighbours has the radius +inf.

Reference.  ``dist2`` is the DIRECT form sum_k (a_k - b_k)^2 from the fp32 inputs -- deliberately not the kernel's Gram
form -- evaluated in numpy's extended precision (64-bit significand, unit roundoff v = 2^-64): a difference, a square
and D - 1 additions round at most D + 1 times, so the reference is within (D + 2) v d2 <= (D + 2) 2^-11 u S of the true
value (S below), under 3 u S for every D <= 4096 = HIM_FEAT_MAX_DIM.

Bounds, derived and not tuned, u = 2^-53, S_ab = |a|^2 + |b|^2 + 2 sum_k |a_k b_k|.
  The kernel computes fl(fl(na + nb) - 2 dot), na = |a|^2, nb = |b|^2 and dot = a.b each a sum of D EXACT products (fp32
  operands widened to fp64) added in some order -- lanes striding the columns and a butterfly for the norms, the matrix
  instruction's own order for the dot product.  Any order of D - 1 additions gives |sum_got - sum| <= gamma_(D-1) sum|terms|,
  gamma_m = m u / (1 - m u); the factor 2 is exact; the two final operations round once each, at most u (na + nb) and
  u |d2| <= u S.  The clamp at 0 moves a value towards the non-negative truth.  To first order that is (D - 1 + 2) u S;
  the second-order part of gamma (D^2 u^2 S, below 2^-29 u S) and the reference's own 3 u S fit into
      pair       |d2_got - d2_ref| <= e_ab = (D + 8) u S_ab.
  The k-th order statistic of a row of values is 1-Lipschitz in the max norm (self is excluded by position on both sides),
      radius     |r2_got,i - r2_ref,i| <= max_{j != i} e_ij.
  Integer-valued features whose sums stay below 2^53 round nowhere: radii and counts EQUAL the integer result.

Decisions.  [d2 <= r2] is certain when the reference margin |d2_ref - r2_i| exceeds e_ij (plus the radius bound when
the radii come from the kernel too); ``membership_bounds`` returns the counts of the certainly-inside and of the
not-certainly-outside pairs, and the kernel's count must lie between them.  For every real-valued case of the GPU tests
(``REAL_CASES``) the reference alone has ZERO uncertain decisions -- tests/test_prdc_cpu.py asserts it -- so the two
bounds coincide and counts are compared for equality.  Ties (duplicate rows, lattice points) use integer features."""
import json
import os
from collections import OrderedDict

import numpy as np

U = 2.0 ** -53
FEAT_MAX_DIM = 4096          # HIM_FEAT_MAX_DIM of include/him.h
KNN_MAX_K = 16               # HIM_KNN_MAX_K
KNN_NONFINITE = 1            # HIM_KNN_NONFINITE
# constants of csrc/him_prdc.hip the shapes of the GPU tests are chosen by
TILE, CHUNK_TILES, MAX_CHUNKS, MEMBER_SPLIT = 64, 8, 16, 64

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    raise RuntimeError('prdc_fixture: the reference needs numpy.longdouble with a 64-bit significand')


# ------------------------------------------------------------------------------------------------------- reference
def finite_rows(x):
    return np.isfinite(np.asarray(x, np.float64)).all(1)


def dist2(a, b):
    """(na, nb) float64: sum_k (a_k - b_k)^2 in extended precision, rounded to float64 once; NaN where either row has a
    non-finite feature."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    fa, fb = finite_rows(a), finite_rows(b)
    al, bl = np.where(fa[:, None], a, 0).astype(LD), np.where(fb[:, None], b, 0).astype(LD)
    out = np.empty((len(a), len(b)), np.float64)
    for i0 in range(0, len(a), 64):
        diff = al[i0:i0 + 64, None, :] - bl[None, :, :]
        out[i0:i0 + 64] = (diff * diff).sum(-1).astype(np.float64)
    out[~fa, :] = np.nan
    out[:, ~fb] = np.nan
    return out


def dist2_bound(a, b):
    """e_ab = (D + 8) u (|a|^2 + |b|^2 + 2 sum_k |a_k b_k|), (na, nb); rows with a non-finite feature give NaN."""
    a, b = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    with np.errstate(invalid='ignore', over='ignore'):
        return (a.shape[1] + 8) * U * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] + 2.0 * (a @ b.T))


def kth_smallest(d2, k, exclude_self=True):
    """Per row of the square matrix d2 the k-th smallest entry off the diagonal; NaN entries never count (a row with
    fewer than k others has +inf); a row whose own entries are all NaN (a non-finite row) gives NaN."""
    d = np.array(d2, np.float64)
    bad = np.isnan(d).all(1)
    if exclude_self:
        d[np.arange(len(d)), np.arange(len(d))] = np.inf
    d[np.isnan(d)] = np.inf
    r = np.sort(d, 1)[:, k - 1]
    r[bad] = np.nan
    return r


def radii(x, k):
    return kth_smallest(dist2(x, x), k)


def radii_bound(x):
    """max_{j != i} e_ij per row (the finite rows only)."""
    e = dist2_bound(x, x)
    e[np.arange(len(e)), np.arange(len(e))] = 0.0
    e[~np.isfinite(e)] = 0.0
    return e.max(1)


def membership(q, r, radii2, strict=False):
    """(row_count (nq,), col_count (nr,)) int64 of I[j, i] = d2(q_j, r_i) <= radii2[i].  ``strict`` plants `<`."""
    d = dist2(q, r)
    with np.errstate(invalid='ignore'):
        ind = (d < np.asarray(radii2)[None, :]) if strict else (d <= np.asarray(radii2)[None, :])
    return ind.sum(1), ind.sum(0)


def membership_bounds(q, r, radii2, radius_bound=0.0):
    """(row_lo, row_hi, col_lo, col_hi, n_uncertain): a pair is certainly inside when d2_ref + e <= r2 - rb, certainly
    outside when d2_ref - e > r2 + rb, and uncertain otherwise; lo counts the first kind, hi all but the second."""
    d, e = dist2(q, r), dist2_bound(q, r)
    r2, rb = np.asarray(radii2, np.float64)[None, :], np.broadcast_to(np.asarray(radius_bound, np.float64), (len(r),))[None, :]
    with np.errstate(invalid='ignore'):
        sure_in = d + e <= r2 - rb
        sure_out = (d - e > r2 + rb) | np.isnan(d) | np.isnan(r2)
    maybe = ~sure_out
    return sure_in.sum(1), maybe.sum(1), sure_in.sum(0), maybe.sum(0), int((maybe & ~sure_in).sum())


def counts(real, fake, k):
    """(row_fake_in_real, col_real_covered, row_real_in_fake) of the reference."""
    row_fr, col_r = membership(fake, real, radii(real, k))
    row_rf, _ = membership(real, fake, radii(fake, k))
    return row_fr, col_r, row_rf


def prdc_from_counts(k, row_fake_in_real, col_real_covered, row_real_in_fake):
    """util.metrics.prdc_from_counts restated by explicit loops."""
    ny, nx = len(row_fake_in_real), len(col_real_covered)
    inside = covered = back = total = 0
    for j in range(ny):
        inside += 1 if row_fake_in_real[j] > 0 else 0
        total += int(row_fake_in_real[j])
    for i in range(nx):
        covered += 1 if col_real_covered[i] > 0 else 0
    for j in range(len(row_real_in_fake)):
        back += 1 if row_real_in_fake[j] > 0 else 0
    return OrderedDict([('precision', inside / ny), ('recall', back / len(row_real_in_fake)),
                        ('density', total / (k * ny)), ('coverage', covered / nx)])


def prdc(real, fake, k):
    return prdc_from_counts(k, *counts(real, fake, k))


# ----------------------------------------------------------------------------------- CPU stand-ins of the kernels
def _seq_sum(terms):
    """Sum along the last axis, strictly left to right in float64 (numpy's cumulative sum adds sequentially)."""
    return np.cumsum(terms, -1)[..., -1]


def standin_dist2(a, b, clamp=True):
    """The kernel's Gram form in float64: exact products, the norms summed left to right and the dot product right to
    left (two different orders, as on the device), |a|^2 + |b|^2 - 2 a.b, clamped at 0 unless ``clamp`` is off."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = _seq_sum(a * a), _seq_sum(b * b)
    dot = np.stack([_seq_sum((a[i][None, :] * b)[:, ::-1]) for i in range(len(a))])
    d = (na[:, None] + nb[None, :]) - 2.0 * dot
    return np.where(d < 0.0, 0.0, d) if clamp else d


def f32_rowmap(tile_rows):
    """The defect of an epilogue that reads the fp64 accumulator tile with the f32 instruction's row formula: the value
    of tile row (lane >> 4) + 4 q is taken for row 4 (lane >> 4) + q, in every 16-row tile."""
    out = np.array(tile_rows)
    n = len(out)
    for t in range(0, n, 16):
        for g in range(4):
            for q in range(4):
                src, dst = t + g + 4 * q, t + 4 * g + q
                if src < n and dst < n:
                    out[dst] = tile_rows[src]
    return out


def standin_radii(x, k, keep_self=False, kth=0, rowmap='f64', ragged=False, clamp=True):
    """him_knn_radii on the CPU.  Defects: ``keep_self`` (the diagonal takes part), ``kth`` = -1 / +1 (the neighbouring
    order statistic), ``rowmap='f32'``, ``ragged`` (the zero rows that pad the last 64-column tile take part),
    ``clamp=False``."""
    x = np.asarray(x, np.float32)
    n = len(x)
    cols = x
    if ragged and n % TILE:
        cols = np.concatenate([x, np.zeros((TILE - n % TILE, x.shape[1]), np.float32)])
    d = standin_dist2(x, cols, clamp)
    if rowmap == 'f32':
        d = f32_rowmap(d)
    if not keep_self:
        d[np.arange(n), np.arange(n)] = np.inf
    return np.sort(d, 1)[:, k - 1 + kth]


def standin_membership(q, r, radii2, strict=False, query_radius=False, swap=False, rowmap='f64', ragged=False):
    """him_knn_membership on the CPU: (row_count, col_count).  Defects: ``strict`` (`<`), ``query_radius`` (the radius
    of the query's position instead of the reference's), ``swap`` (the two outputs exchanged), ``rowmap='f32'``,
    ``ragged`` (the zero rows that pad the last 64-row query tile are counted into col_count)."""
    q, r, radii2 = np.asarray(q, np.float32), np.asarray(r, np.float32), np.asarray(radii2, np.float64)
    rows = q
    if ragged and len(q) % TILE:
        rows = np.concatenate([q, np.zeros((TILE - len(q) % TILE, q.shape[1]), np.float32)])
    d = standin_dist2(rows, r)
    if rowmap == 'f32':
        d = f32_rowmap(d)
    rad = np.resize(radii2, len(rows))[:, None] if query_radius else radii2[None, :]
    ind = (d < rad) if strict else (d <= rad)
    row_count, col_count = ind[:len(q)].sum(1), ind.sum(0)
    return (col_count, row_count) if swap else (row_count, col_count)


# ------------------------------------------------------------------------------------------------ comparison helpers
class RowFile(object):
    """Rows that go straight to a .jsonl file: a line is on disk before its assertion runs."""

    def __init__(self, path):
        self.path = path

    def append(self, row):
        os.makedirs(os.path.dirname(self.path), exist_ok=True)
        with open(self.path, 'a') as f:
            f.write(json.dumps(row) + '\n')


def _record(rows, case, tensor, err, bound, ratio):
    row = dict(case=case, tensor=tensor, error=err, bound=bound, ratio=ratio)
    if rows is not None:
        rows.append(row)
    print('%s %s: error %r bound %r ratio %r' % (case, tensor, err, bound, ratio))
    return row


def check_bound(case, tensor, got, ref, bound, rows=None):
    """NaN exactly where the reference has NaN, +inf where it has +inf, and |got - ref| <= bound elsewhere; records the
    worst error, its bound and the worst error / bound."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    b = np.broadcast_to(np.asarray(bound, np.float64), r.shape)
    assert g.shape == r.shape, '%s %s: shape %s against %s' % (case, tensor, g.shape, r.shape)
    same_kind = bool((np.isnan(g) == np.isnan(r)).all() and (np.isposinf(g) == np.isposinf(r)).all())
    fin = np.isfinite(r) & np.isfinite(g)
    err = np.where(fin, np.abs(np.where(fin, g, 0.0) - np.where(fin, r, 0.0)), 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / b)
    worst = int(np.argmax(ratio)) if err.size else 0
    row = _record(rows, case, tensor, float(err.reshape(-1)[worst]) if err.size else 0.0,
                  float(b.reshape(-1)[worst]) if err.size else 0.0, float(ratio.reshape(-1)[worst]) if err.size else 0.0)
    assert same_kind and bool(np.isfinite(g[np.isfinite(r)]).all()), '%s %s: NaN or inf in other places than the reference' % (case, tensor)
    assert bool((err <= b).all()), '%s %s: error %.3e > bound %.3e (ratio %.3f)' % (case, tensor, row['error'], row['bound'],
                                                                                    row['ratio'])
    return row


def check_equal(case, tensor, got, want, rows=None):
    """Exact equality of values (integer features; counts), NaN matching NaN."""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same = g.shape == w.shape and bool(((g == w) | (np.isnan(g) & np.isnan(w))).all())
    err = None if g.shape != w.shape else float(np.nanmax(np.abs(np.where(g == w, 0.0, g - w)), initial=0.0))
    _record(rows, case, tensor, err, 0.0, None)
    assert same, '%s %s: not equal to the exact result (shape %s against %s)%s' % (
        case, tensor, g.shape, w.shape, '' if g.shape != w.shape else ' at %s' % np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:4].tolist())


def check_counts(case, tensor, got, lo, hi, rows=None):
    """lo <= got <= hi element by element (lo == hi wherever no decision is uncertain)."""
    g, lo, hi = np.asarray(got, np.int64), np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    ok = g.shape == lo.shape and bool(((g >= lo) & (g <= hi)).all())
    off = None if g.shape != lo.shape else float(np.maximum(np.maximum(lo - g, g - hi), 0).max(initial=0))
    _record(rows, case, tensor, off, float((hi - lo).max(initial=0)), None)
    assert ok, '%s %s: a count outside [lower, upper] (shape %s against %s)' % (case, tensor, g.shape, lo.shape)


def check_nonnegative(case, tensor, got, rows=None):
    """The clamp: no squared distance, hence no radius, is below 0."""
    g = np.asarray(got, np.float64)
    low = float(np.nanmin(g, initial=0.0))
    _record(rows, case, tensor, -low, 0.0, None)
    assert not low < 0.0, '%s %s: a negative squared distance %.3e' % (case, tensor, low)


# ---------------------------------------------------------------------------------------------------- seeded inputs
def features(seed, n, D, shift=0.0, scale=1.0):
    """fp32 descriptor rows (n, D): positive on average, like pooled ReLU features, plus ``shift``."""
    g = np.random.default_rng(seed)
    return (np.abs(g.standard_normal((n, D))) * scale + 0.3 * g.standard_normal((n, D)) + shift).astype(np.float32)


def lattice(seed, n, D, hi):
    """fp32 rows of integers in [-hi, hi]: lattice points, with ties between distances and (for small hi) equal rows."""
    return np.random.default_rng(seed).integers(-hi, hi + 1, (n, D)).astype(np.float32)


def distinct_norm_rows(seed, n, D, hi):
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


def with_duplicates(x, times):
    """Every row ``times`` times, the copies dealt over the matrix (row i of x at positions i, i + n, ...)."""
    return np.concatenate([np.asarray(x, np.float32)] * times)


def int_dist2(a, b):
    """The integer result: sum_k (a_k - b_k)^2 in int64."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T))


def int_radii(x, k, block=1024):
    """The exact radii of integer rows, in blocks of rows (the 8193-row case)."""
    x = np.asarray(x).astype(np.int64)
    out = np.empty(len(x), np.int64)
    for i0 in range(0, len(x), block):
        d = int_dist2(x[i0:i0 + block], x)
        d[np.arange(len(d)), i0 + np.arange(len(d))] = np.iinfo(np.int64).max
        out[i0:i0 + block] = np.partition(d, k - 1, 1)[:, k - 1]
    return out


def int_membership(q, r, radii2):
    ind = int_dist2(q, r) <= np.asarray(radii2, np.int64)[None, :]
    return ind.sum(1), ind.sum(0)


# The real-valued cases of the GPU tests, (nq, nr, D, k): the fake set q (seed 2 s + 1, shifted) against the real set r
# (seed 2 s), s the position in this list.  tests/test_prdc_cpu.py asserts that none has an uncertain decision.
REAL_CASES = ((33, 70, 5, 3), (70, 33, 67, 5), (17, 17, 1, 1), (65, 64, 4, 5), (64, 130, 16, 16), (130, 63, 3, 3),
              (40, 40, 24, 5), (130, 130, 67, 5))


def real_case(index):
    nq, nr, D, k = REAL_CASES[index]
    return features(2 * index + 1, nq, D, shift=0.15, scale=1.1), features(2 * index, nr, D), k
