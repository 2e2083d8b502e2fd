"""Integer numpy restatement of include/him.h "Panoptic matching" and the deterministic planes the panoptic tests run on
(helper module like ccl_fixture.py; imports nothing from the package).

``match_reference`` works plane by plane with ``np.unique`` on the ids (the rank order) and on the pair keys
``row * n_pred + column`` (the overlaps), takes the integer counts as they are, and divides only where the contract
does: ``float(inter) / float(union)`` per matched pair, added in plane and rank order."""
import numpy as np

import ccl_fixture as cf

OVERFLOW, ID_RANGE, CLS_RANGE, MIXED, CCL = 1, 2, 4, 8, 16
REFUSED = OVERFLOW | ID_RANGE | CLS_RANGE
# the kernel's walk (csrc/him_panoptic.hip): a lane reads PX pixels per step, a workgroup STEP = 256 * PX pixels per step,
# and a workgroup's share of a plane is a multiple of STEP, at least SHARE_MIN pixels
PX, STEP, SHARE_MIN = 4, 1024, 2048
IDS = 65536
SEG_NP = {0: np.uint8, 1: np.int32, 2: np.int64}
CLS_NP = {0: np.uint8, 1: np.int32, 2: np.int64, 3: np.float32}


def _integral(a):
    a = np.asarray(a)
    if a.dtype.kind == 'f':
        with np.errstate(invalid='ignore'):
            ok = np.isfinite(a) & (a == np.floor(a)) & (np.abs(a) < 2.0 ** 31)
        return ok, np.where(ok, a, -1).astype(np.int64)
    return np.ones(a.shape, bool), a.astype(np.int64)


def plane_reference(pred_seg, pred_cls, gt_seg, gt_cls, n_class, mask=None, ignore=-1, max_segments=1024):
    """ONE plane -> dict(status [n_gt, n_pred, flags, 0], rows (n_gt, 6) int64 or None, pairs, fp_classes)."""
    ps = np.asarray(pred_seg).reshape(-1).astype(np.int64)
    gs = np.asarray(gt_seg).reshape(-1).astype(np.int64)
    pc_int, pc = _integral(np.asarray(pred_cls).reshape(-1))
    gc_int, gc = _integral(np.asarray(gt_cls).reshape(-1))
    void = np.zeros(ps.shape, bool)
    if mask is not None:
        void |= np.asarray(mask).reshape(-1) == 0
    if ignore >= 0:
        void |= gc_int & (gc == ignore)
    live = ~void
    ps_ok, gs_ok = (ps >= 0) & (ps < IDS), (gs >= 0) & (gs < IDS)
    pc_ok, gc_ok = pc_int & (pc >= 0) & (pc < n_class), gc_int & (gc >= 0) & (gc < n_class)
    flags = 0
    if (~ps_ok).any() or (live & ~gs_ok).any():
        flags |= ID_RANGE
    if (~pc_ok).any() or (live & ~gc_ok).any():
        flags |= CLS_RANGE
    pids = np.unique(ps[ps_ok])
    gids = np.unique(gs[live & gs_ok])
    if len(pids) > max_segments or len(gids) > max_segments:
        flags |= OVERFLOW
    out = dict(status=[len(gids), len(pids), flags, 0], rows=None, tp=[], fp=[], fn=[])
    if flags & REFUSED:
        return out
    n_p = len(pids)
    prank = np.searchsorted(pids, ps)
    grow = np.where(live, np.searchsorted(gids, np.where(live, gs, gids[0] if len(gids) else 0)) + 1, 0)
    keys, cnt = np.unique(grow * n_p + prank, return_counts=True)
    table = np.zeros((len(gids) + 1, n_p), np.int64)
    table.reshape(-1)[keys] = cnt
    p_area, g_area, void_p = table.sum(0), table[1:].sum(1), table[0]
    p_min = np.array([pc[ps == i].min() for i in pids], np.int64)
    p_max = np.array([pc[ps == i].max() for i in pids], np.int64)
    g_min = np.array([gc[live & (gs == i)].min() for i in gids], np.int64)
    g_max = np.array([gc[live & (gs == i)].max() for i in gids], np.int64)
    if (p_min != p_max).any() or (g_min != g_max).any():
        out['status'][2] |= MIXED
    rows, taken = [], np.zeros(n_p, bool)
    for g in range(len(gids)):
        inter = table[g + 1]
        union = g_area[g] + p_area - inter - void_p
        hit = np.nonzero((p_min == g_min[g]) & (2 * inter > union))[0]
        assert len(hit) <= 1, 'a ground-truth segment matched twice'
        if len(hit):
            p = int(hit[0])
            assert not taken[p], 'a predicted segment matched twice'
            taken[p] = True
            rows.append([gids[g], g_min[g], g_area[g], pids[p], inter[p], union[p]])
            out['tp'].append((int(g_min[g]), int(inter[p]), int(union[p])))
        else:
            rows.append([gids[g], g_min[g], g_area[g], -1, 0, 0])
            out['fn'].append(int(g_min[g]))
    for p in range(n_p):
        if not taken[p] and not 2 * void_p[p] > p_area[p]:
            out['fp'].append(int(p_min[p]))
    out['rows'] = np.array(rows, np.int64).reshape(-1, 6)
    return out


def match_reference(pred_seg, pred_cls, gt_seg, gt_cls, n_class, mask=None, ignore=-1, max_segments=1024):
    """A (B,H,W) batch -> (counts (n_class,3) int64, iou_sum (n_class,) float64, status (B,4) int32, rows per plane)."""
    B = len(pred_seg)
    counts, iou = np.zeros((n_class, 3), np.int64), np.zeros(n_class, np.float64)
    status, rows = np.zeros((B, 4), np.int32), []
    for b in range(B):
        r = plane_reference(pred_seg[b], pred_cls[b], gt_seg[b], gt_cls[b], n_class,
                            None if mask is None else mask[b], ignore, max_segments)
        status[b] = r['status']
        rows.append(r['rows'])
        for c, inter, union in r['tp']:
            counts[c, 0] += 1
            iou[c] += float(inter) / float(union)
        for c in r['fp']:
            counts[c, 1] += 1
        for c in r['fn']:
            counts[c, 2] += 1
    return counts, iou, status, rows


def scores_reference(counts, iou_sum):
    """(pq, sq, rq) means over the classes with tp + fp + fn > 0, and the per-class pq (nan: absent)."""
    counts, iou_sum = np.asarray(counts, np.float64).reshape(-1, 3), np.asarray(iou_sum, np.float64)
    pq, sq, rq = [], [], []
    for (tp, fp, fn), s in zip(counts, iou_sum):
        den = tp + 0.5 * fp + 0.5 * fn
        pq.append(s / den if den > 0 else np.nan)
        sq.append(s / tp if tp > 0 else np.nan)
        rq.append(tp / den if den > 0 else np.nan)
    seen = counts.sum(1) > 0
    mean = lambda v: float(np.mean([x for x, k in zip(v, seen) if k])) if seen.any() else float('nan')
    return mean(pq), mean(sq), mean(rq), np.array(pq)


# ---- planes -----------------------------------------------------------------------------------------------------------
# the hand-drawn pair of test_panoptic_cpu.py: areas g1 6, g2 6, g3 8, g7 4; p5 7, p6 5, p3 10, p9 2
HAND_GT_SEG = np.array([[1, 1, 1, 2, 2, 2],
                        [1, 1, 1, 2, 2, 2],
                        [3, 3, 3, 3, 7, 7],
                        [3, 3, 3, 3, 7, 7]])
HAND_PRED_SEG = np.array([[5, 5, 5, 5, 6, 6],
                          [5, 5, 5, 6, 6, 6],
                          [3, 3, 3, 3, 3, 9],
                          [3, 3, 3, 3, 3, 9]])
HAND_GT_CLS_OF, HAND_PRED_CLS_OF = {1: 1, 2: 2, 3: 0, 7: 2}, {5: 1, 6: 2, 3: 0, 9: 2}


def classes_of(seg, table):
    return np.vectorize(table.get)(seg)


def hand_planes():
    """(pred_seg, pred_cls, gt_seg, gt_cls) of the hand-drawn 4 x 6 pair, n_class 3."""
    return (HAND_PRED_SEG.copy(), classes_of(HAND_PRED_SEG, HAND_PRED_CLS_OF), HAND_GT_SEG.copy(),
            classes_of(HAND_GT_SEG, HAND_GT_CLS_OF))


def own_ids(H, W, cls=3):
    """Every pixel is its own segment: ids 0..H*W-1 in raster order, one class."""
    return np.arange(H * W, dtype=np.int64).reshape(H, W), np.full((H, W), cls, np.int64)


def shifted(a, dy=0, dx=0):
    """``a`` moved down / right by (dy, dx) with the edge replicated."""
    H, W = a.shape
    yy = np.clip(np.arange(H) - dy, 0, H - 1)
    xx = np.clip(np.arange(W) - dx, 0, W - 1)
    return np.ascontiguousarray(a[yy][:, xx])


def stripes_and_bands(H=40, W=256):
    """gt: vertical stripes 37 wide (every row run ends inside a lane's 4 pixels somewhere), pred: horizontal bands 3 high
    (they straddle every border between two shares of SHARE_MIN pixels and between two steps of STEP pixels); classes by
    id.  H * W = 5 shares."""
    yy, xx = np.mgrid[0:H, 0:W]
    gt_seg, pred_seg = xx // 37, yy // 3
    return pred_seg, pred_seg % 5, gt_seg, gt_seg % 5


def perturbed_layouts(B=3, H=97, W=193, things=cf.CITY_THINGS, salt=0.02):
    """(pred_seg, pred_cls, gt_seg, gt_cls), each (B,H,W) int64: the ground truth is ``ccl_fixture.coarse_layout`` labelled
    by ``label_reference`` (8-connected); the prediction is the same layout moved by 2 pixels with salt noise of its
    own, labelled the same way."""
    out = [[], [], [], []]
    for b in range(B):
        gt_cls = cf.coarse_layout(H, W, seed=b, salt=salt).astype(np.int64)
        clean = cf.coarse_layout(H, W, seed=b, salt=0.0).astype(np.int64)
        rng = np.random.RandomState(1000 + b)
        noise = rng.rand(H, W) < salt
        pred_cls = np.where(noise, rng.randint(0, 35, size=(H, W)), shifted(clean, 2, 2))
        gt_seg = cf.label_reference(gt_cls, things, 8)[0]
        pred_seg = cf.label_reference(pred_cls, things, 8)[0]
        for lst, a in zip(out, (pred_seg, pred_cls, gt_seg, gt_cls)):
            lst.append(a.astype(np.int64))
    return tuple(np.stack(v) for v in out)


def stuff_layouts(B=1, H=48, W=96, classes=6, seed=5):
    """(pred, gt) class planes (B,H,W) of a few large stuff regions; the prediction is the ground truth moved by 3 pixels,
    with a block of class ``classes`` (absent from the ground truth) painted over the upper middle, so that class IoUs on
    both sides of 0.5 occur."""
    gt = np.stack([cf.coarse_layout(H, W, classes=classes, cell=24, seed=seed + b, salt=0.0) for b in range(B)])
    pred = np.stack([shifted(g, 3, 3) for g in gt]).astype(np.int64)
    pred[:, :H // 2, 3 * W // 8:5 * W // 8] = classes
    return pred, gt.astype(np.int64)
