"""Brute-force restatement of include/him.h "Distance transform and boundary metrics" in numpy (helper module, not a
conftest; it never imports the package's kernels and needs no scipy).  Distances are int64 over ALL pixel-seed pairs, so
keep planes at or below ~2500 pixels; the tie rule is an argmin over the key (d2, seed index).  Statistics and scores
are float64.  The keyword arguments ``metric`` / ``tie`` / ``neighbours`` / ``strict`` exist for the planted defects of
tests/test_edt_cpu.py: their defaults are the contract."""
import math

import numpy as np

NONZERO, EQUALS, BOUNDARY_OF, ANY_BOUNDARY = 0, 1, 2, 3
NONE = 2 ** 31 - 1
BAD_JOB = 1
NP_OF = {0: np.uint8, 1: np.int32, 2: np.int64, 3: np.float32}


# ------------------------------------------------------------------------------------------------------------ seeds
def _differs(plane, neighbours=4):
    """True where a neighbour INSIDE the plane holds another value."""
    H, W = plane.shape
    out = np.zeros((H, W), bool)
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if neighbours == 8 else [])
    for dy, dx in steps:
        a = plane[0:H - dy, max(0, -dx):W - max(0, dx)]
        b = plane[dy:H, max(0, dx):W - max(0, -dx)]
        d = a != b
        out[0:H - dy, max(0, -dx):W - max(0, dx)] |= d
        out[dy:H, max(0, dx):W - max(0, -dx)] |= d
    return out


def seeds(plane, value, rule, neighbours=4):
    if rule == NONZERO:
        return plane != 0
    if rule == EQUALS:
        return plane == value
    if rule == BOUNDARY_OF:
        return (plane == value) & _differs(plane, neighbours)
    if rule == ANY_BOUNDARY:
        return _differs(plane, neighbours)
    raise ValueError(rule)


# -------------------------------------------------------------------------------------------------------- transform
def edt(seed, metric='euclid', tie='left'):
    """(dist2 int32 (H,W), nearest int32 (H,W)) of a boolean seed plane."""
    H, W = seed.shape
    ys, xs = np.nonzero(seed)
    if len(ys) == 0:
        return np.full((H, W), NONE, np.int32), np.full((H, W), -1, np.int32)
    py, px = np.divmod(np.arange(H * W, dtype=np.int64), W)
    dy = py[:, None] - ys[None, :].astype(np.int64)
    dx = px[:, None] - xs[None, :].astype(np.int64)
    d2 = dy * dy + dx * dx if metric == 'euclid' else (np.abs(dy) + np.abs(dx)) ** 2
    index = ys.astype(np.int64) * W + xs
    order = index if tie == 'left' else ys.astype(np.int64) * W + (W - 1 - xs)
    pick = np.argmin(d2 * (H * W) + order[None, :], axis=1)
    rows = np.arange(H * W)
    return d2[rows, pick].reshape(H, W).astype(np.int32), index[pick].reshape(H, W).astype(np.int32)


def edt_jobs(src, jobs, **kw):
    """him_edt: src (B,H,W), jobs (K,3) -> dist2 (K,H,W) int32, nearest (K,H,W) int32, status (K,2) int32."""
    B, H, W = src.shape
    seed_kw = {k: v for k, v in kw.items() if k == 'neighbours'}
    edt_kw = {k: v for k, v in kw.items() if k in ('metric', 'tie')}
    K = len(jobs)
    dist2 = np.full((K, H, W), NONE, np.int32)
    nearest = np.full((K, H, W), -1, np.int32)
    status = np.zeros((K, 2), np.int32)
    for k, (b, v, rule) in enumerate(np.asarray(jobs).tolist()):
        if not 0 <= b < B or not 0 <= rule <= 3:
            status[k, 1] = BAD_JOB
            continue
        s = seeds(src[b], v, rule, **seed_kw)
        status[k, 0] = int(s.sum())
        dist2[k], nearest[k] = edt(s, **edt_kw)
    return dist2, nearest, status


def boundary_stats(src, jobs, dist2, tol2, strict=False, **seed_kw):
    """him_boundary_stats: counts (K,4) int64 [n_seed, n_matched, max_d2, n_unreachable] and sumd (K,) float64."""
    B = src.shape[0]
    K = len(jobs)
    counts = np.zeros((K, 4), np.int64)
    counts[:, 2] = -1
    sumd = np.zeros(K, np.float64)
    for k, (b, v, rule) in enumerate(np.asarray(jobs).tolist()):
        if not 0 <= b < B or not 0 <= rule <= 3:
            continue
        d = dist2[k][seeds(src[b], v, rule, **seed_kw)].astype(np.int64)
        reach = d[d != NONE]
        counts[k] = [len(d), int((d < tol2).sum() if strict else (d <= tol2).sum()), reach.max() if len(reach) else -1,
                     len(d) - len(reach)]
        sumd[k] = math.fsum(np.sqrt(reach.astype(np.float64)))
    return counts, sumd


# ----------------------------------------------------------------------------------------------------------- scores
def label_ids(pred, kind=None):
    """ids (B,H,W) of what confusion_matrix accepts: ids, (B,C>1,H,W) scores (lowest channel of the maximum) or, with
    kind='prob', probabilities thresholded at 0.5."""
    pred = np.asarray(pred)
    if kind == 'prob':
        return (pred.reshape(pred.shape[0], pred.shape[-2], pred.shape[-1]) > np.float32(0.5)).astype(np.int32)
    if pred.ndim == 4 and pred.shape[1] > 1:
        return np.argmax(pred, axis=1).astype(np.int32)          # numpy: the first maximum
    return pred.reshape(-1, pred.shape[-2], pred.shape[-1])


def class_jobs(B, classes, rule=BOUNDARY_OF):
    return np.array([[b, c, rule] for b in range(B) for c in classes], np.int32).reshape(-1, 3)


def tol2_of(tolerance):
    return int(math.floor(float(tolerance) ** 2))


def scores_from_counts(cp, sp, cg, sg):
    """precision, recall, f1, assd, hausdorff (float64, same shape as the leading dims) from the two directions' counts
    (..., 4) and distance sums (...)."""
    cp, cg = np.asarray(cp, np.int64), np.asarray(cg, np.int64)
    n_p, n_g = cp[..., 0].astype(np.float64), cg[..., 0].astype(np.float64)
    both, none = (n_p > 0) & (n_g > 0), (n_p == 0) & (n_g == 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        prec = np.where(both, cp[..., 1] / n_p, 0.0)
        rec = np.where(both, cg[..., 1] / n_g, 0.0)
        f1 = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
        assd = np.where(both, (np.asarray(sp) + np.asarray(sg)) / (n_p + n_g), np.nan)
        hd = np.where(both, np.sqrt(np.maximum(cp[..., 2], cg[..., 2]).astype(np.float64)), np.nan)
    out = {}
    for name, v in (('precision', prec), ('recall', rec), ('f1', f1)):
        out[name] = np.where(none, np.nan, v)
    out['assd'], out['hausdorff'] = assd, hd
    return out


def boundary_scores(pred_ids, gt_ids, n_class, tolerance=2.0, classes=None, **kw):
    """util.metrics.boundary_scores on id planes (B,H,W): dict of (B,n) float64 arrays plus 'counts' (B,n,2,4) int64
    ([..., 0, :] the prediction's boundary against the ground truth's, [..., 1, :] the mirror) and 'sumd' (B,n,2)."""
    classes = list(range(n_class)) if classes is None else list(classes)
    B, n = pred_ids.shape[0], len(classes)
    jobs = class_jobs(B, classes)
    t2 = tol2_of(tolerance)
    stat_kw = {k: v for k, v in kw.items() if k in ('strict', 'neighbours')}
    d_gt = edt_jobs(gt_ids, jobs, **{k: v for k, v in kw.items() if k != 'strict'})[0]
    d_pr = edt_jobs(pred_ids, jobs, **{k: v for k, v in kw.items() if k != 'strict'})[0]
    cp, sp = boundary_stats(pred_ids, jobs, d_gt, t2, **stat_kw)
    cg, sg = boundary_stats(gt_ids, jobs, d_pr, t2, **stat_kw)
    out = scores_from_counts(cp, sp, cg, sg)
    out = {k: v.reshape(B, n) for k, v in out.items()}
    out['counts'] = np.stack([cp, cg], 1).reshape(B, n, 2, 4)
    out['sumd'] = np.stack([sp, sg], 1).reshape(B, n, 2)
    return out


def mask_boundary_scores(prob, gt_mask, tolerance=2.0):
    """(B,) arrays: the boundary of ``prob > 0.5`` against the boundary of the 0/1 mask."""
    p = label_ids(prob, 'prob')
    g = (np.asarray(gt_mask).reshape(p.shape) != 0).astype(np.int32)
    out = boundary_scores(p, g, 2, tolerance, classes=[1])
    return {k: v[:, 0] for k, v in out.items()}


def diag_tolerance(H, W, frac=0.0075):
    return frac * math.sqrt(H * H + W * W)


def boundary_band(gt_ids, radius):
    """(B,1,H,W) float32 mask of the pixels within ``radius`` of a class boundary."""
    B = gt_ids.shape[0]
    d2 = edt_jobs(gt_ids, class_jobs(B, [0], ANY_BOUNDARY))[0]
    return (d2 <= tol2_of(radius)).astype(np.float32)[:, None]


def confusion(pred_ids, gt_ids, n, mask=None):
    c = np.zeros((n, n), np.int64)
    keep = np.ones(gt_ids.shape, bool) if mask is None else (np.asarray(mask).reshape(gt_ids.shape) != 0)
    np.add.at(c, (gt_ids[keep].astype(np.int64), pred_ids[keep].astype(np.int64)), 1)
    return c


def pooled_boundary_summary(batches, n_class, tolerance):
    """What Evaluator.summary() reports for layouts: per class, counts and sums pooled over every sample first.
    ``batches``: (pred_ids, gt_ids) pairs.  Returns boundary_f1, per_class_boundary_f1 (nan: no boundary), boundary_assd."""
    cnt, sm = np.zeros((n_class, 2, 4), np.int64), np.zeros((n_class, 2), np.float64)
    for p, g in batches:
        r = boundary_scores(p, g, n_class, tolerance)
        cnt += r['counts'].sum(0)
        sm += r['sumd'].sum(0)
    n_p, n_g = cnt[:, 0, 0].astype(np.float64), cnt[:, 1, 0].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        prec = np.where(n_p > 0, cnt[:, 0, 1] / n_p, 0.0)
        rec = np.where(n_g > 0, cnt[:, 1, 1] / n_g, 0.0)
        f1 = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
        reach = (cnt[:, :, 0] - cnt[:, :, 3]).sum(1).astype(np.float64)
        assd = np.where(reach > 0, sm.sum(1) / reach, np.nan)
    seen = (n_p + n_g) > 0
    f1 = np.where(seen, f1, np.nan)
    return dict(boundary_f1=float(f1[seen].mean()) if seen.any() else float('nan'), per_class_boundary_f1=f1,
                boundary_assd=float(np.nanmean(assd)) if np.isfinite(assd).any() else float('nan'))


# ------------------------------------------------------------------------------------------------------ comparisons
def assert_edt_equal(got, want, what=''):
    """(dist2, nearest or None, status): equality, nothing excluded."""
    for name, g, w in zip(('dist2', 'nearest', 'status'), got, want):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, '%s %s: shape %s, expected %s' % (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            i = tuple(int(v[0]) for v in np.nonzero(g != w))
            raise AssertionError('%s %s: %d cells differ, first at %s: got %d, expected %d'
                                 % (what, name, int((g != w).sum()), i, g[i], w[i]))


def assert_stats_equal(got_counts, got_sumd, want_counts, want_sumd, what=''):
    """counts: equality; sumd: within n_seed * 2^-52 relative (only the order of the additions differs)."""
    got_counts, want_counts = np.asarray(got_counts), np.asarray(want_counts)
    assert got_counts.shape == want_counts.shape and np.array_equal(got_counts, want_counts), \
        '%s counts:\n%s\nexpected\n%s' % (what, got_counts, want_counts)
    got_sumd, want_sumd = np.asarray(got_sumd, np.float64), np.asarray(want_sumd, np.float64)
    bound = want_counts[..., 0].reshape(want_sumd.shape) * 2.0 ** -52 * np.abs(want_sumd)
    err = np.abs(got_sumd - want_sumd)
    assert (err <= bound).all(), '%s sumd: error %s above %s' % (what, err.max(), bound[err.argmax()])


def assert_scores_equal(got, want, what='', rel=1e-12):
    """Integer parts equal, float64 parts within ``rel`` relative, the nan pattern identical."""
    assert np.array_equal(np.asarray(got['counts']), want['counts']), '%s counts differ' % what
    for k in ('precision', 'recall', 'f1', 'assd', 'hausdorff'):
        g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), '%s %s: nan pattern\n%s\nexpected\n%s' % (what, k, g, w)
        ok = ~np.isnan(w)
        assert (np.abs(g[ok] - w[ok]) <= rel * np.abs(w[ok])).all(), '%s %s:\n%s\nexpected\n%s' % (what, k, g, w)


# ------------------------------------------------------------------------------------------------------------ planes
def blocky(seed, B, H, W, classes, cell=7, salt=0.02):
    """Random label planes of blocks of ``cell`` pixels with a little salt noise, ids drawn from ``classes``."""
    g = np.random.default_rng(seed)
    classes = np.asarray(classes)
    coarse = classes[g.integers(0, len(classes), size=(B, (H + cell - 1) // cell, (W + cell - 1) // cell))]
    full = np.repeat(np.repeat(coarse, cell, 1), cell, 2)[:, :H, :W].copy()
    noise = g.random((B, H, W)) < salt
    full[noise] = classes[g.integers(0, len(classes), size=int(noise.sum()))]
    return full.astype(np.int64)


def layout_pair(seed=5, B=3, H=40, W=56):
    """(pred, gt) int64 id planes with 5 classes: class 4 absent from both, class 3 in the prediction only; the
    prediction is the ground truth shifted by (2, 3) with fresh blocks in one corner."""
    gt = blocky(seed, B, H, W, (0, 1, 2))
    pred = np.roll(gt, (2, 3), (1, 2)).copy()
    pred[:, :9, :11] = blocky(seed + 1, B, 9, 11, (0, 1, 2, 3), cell=4)
    return pred, gt


def scores_of(ids, n, seed):
    """fp32 scores (B,n,H,W) whose arg-max (lowest channel on a tie) is ``ids``; quarter steps, ties abound."""
    g = np.random.default_rng(seed)
    B, H, W = ids.shape
    s = g.integers(0, 4, size=(B, n, H, W)).astype(np.float32) * np.float32(0.25)
    top = s.max(1)
    chan = np.arange(n)[None, :, None, None]
    s = np.where(chan == ids[:, None], top[:, None], s)                    # a tie with every other maximum ...
    s = np.where(chan < ids[:, None], np.minimum(s, top[:, None] - np.float32(0.25)), s)   # ... none of them lower
    return s.astype(np.float32)
