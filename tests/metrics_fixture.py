"""Float64 numpy restatement of the evaluation metrics of include/him.h "Evaluation metrics" (helper module like
util.py; not a conftest).  Written from the definitions alone: a loop over the 11 x 11 window taps for the moments,
``np.add.at`` for the confusion matrix.  It shares no code with the package's util/metrics.py and is the yardstick of
tests/test_metrics_*.py; ``dtype=np.float32`` evaluates the same definition naively in fp32 (the ``e32`` of
tests/README.md)."""
import numpy as np

WIN = 11


def gauss():
    """g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in double, then rounded to fp32."""
    g = np.exp(-((np.arange(WIN, dtype=np.float64) - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(np.float32)


def map_values(x, scale, offset, quantize):
    """x' of the header, fp32: x * scale + offset with both operations rounded on their own; the (127.5, 127.5, quantize)
    preset is tensor2im's (x + 1) / 2 * 255; quantize: trunc(clip(., 0, 255))."""
    x = np.asarray(x, dtype=np.float32)
    if quantize and scale == 127.5 and offset == 127.5:
        v = (x + np.float32(1)) / np.float32(2) * np.float32(255)
    else:
        v = x * np.float32(scale) + np.float32(offset)
    assert v.dtype == np.float32
    if quantize:
        v = np.trunc(np.clip(v, np.float32(0), np.float32(255)))
    return v.astype(np.float32)


def ssim_map(a, b, data_range, dtype=np.float64):
    """(H-10, W-10) SSIM of two 2-D planes of mapped values, every step in ``dtype`` with the naive moment formula."""
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    H, W = a.shape
    if H < WIN or W < WIN:
        return np.zeros((max(H - WIN + 1, 0), max(W - WIN + 1, 0)), dtype)
    g = gauss().astype(dtype)
    oh, ow = H - WIN + 1, W - WIN + 1
    mom = [np.zeros((oh, ow), dtype) for _ in range(5)]
    for i in range(WIN):
        for j in range(WIN):
            wgt = dtype(g[i] * g[j])
            pa, pb = a[i:i + oh, j:j + ow], b[i:i + oh, j:j + ow]
            for m, v in zip(mom, (pa, pb, pa * pa, pb * pb, pa * pb)):
                m += wgt * v
    mu_a, mu_b, eaa, ebb, eab = mom
    va, vb, cab = eaa - mu_a * mu_a, ebb - mu_b * mu_b, eab - mu_a * mu_b
    c1, c2 = dtype((0.01 * data_range) ** 2), dtype((0.03 * data_range) ** 2)
    out = (2 * mu_a * mu_b + c1) * (2 * cab + c2) / ((mu_a * mu_a + mu_b * mu_b + c1) * (va + vb + c2))
    assert out.dtype == dtype
    return out


def clip_box(box, H, W):
    """(x0, y0, w, h) of an inclusive (xmin, ymin, xmax, ymax) box clipped to the image; w or h 0: empty."""
    if box is None:
        return 0, 0, W, H
    x0, y0 = max(int(box[0]), 0), max(int(box[1]), 0)
    x1, y1 = min(int(box[2]), W - 1), min(int(box[3]), H - 1)
    return x0, y0, max(x1 - x0 + 1, 0), max(y1 - y0 + 1, 0)


def image_sums(a, b, scale, offset, quantize, data_range, box=None, dtype=np.float64):
    """((B, C, 5) sums in ``dtype``, list of per-plane maps) of two (B, C, H, W) arrays; box: None or (B, 4)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    B, C, H, W = a.shape
    sums, maps = np.zeros((B, C, 5), dtype), []
    for n in range(B):
        x0, y0, w, h = clip_box(None if box is None else box[n], H, W)
        for c in range(C):
            if w == 0 or h == 0:
                maps.append(np.zeros((0, 0), dtype))
                continue
            ca = map_values(a[n, c, y0:y0 + h, x0:x0 + w], scale, offset, quantize).astype(dtype)
            cb = map_values(b[n, c, y0:y0 + h, x0:x0 + w], scale, offset, quantize).astype(dtype)
            m = ssim_map(ca, cb, data_range, dtype)
            d = ca - cb
            sums[n, c] = [m.sum(dtype=dtype), m.size, (d * d).sum(dtype=dtype), np.abs(d).sum(dtype=dtype), d.size]
            maps.append(m)
    return sums, maps


def labels_of(t, kind, n):
    """Integer labels of a prediction / ground-truth array of one of the header's kinds; -1 where the pixel must be
    skipped (negative, >= n, non-integral).  kind 4: (B, C, H, W) scores; kind 5: probabilities."""
    t = np.asarray(t)
    if kind == 4:
        lab = np.argmax(t, axis=1).astype(np.int64)            # first = lowest channel of the maximum
    elif kind == 5:
        lab = (t.reshape(t.shape[0], *t.shape[-2:]) > np.float32(0.5)).astype(np.int64)
    else:
        f = t.reshape(t.shape[0], *t.shape[-2:]).astype(np.float64)
        ok = (f == np.floor(f)) & (f >= 0) & (f < n)
        lab = np.where(ok, f, -1).astype(np.int64)
    return np.where((lab >= 0) & (lab < n), lab, -1)


def confusion(pred, pred_kind, gt, gt_kind, n, mask=None, ignore=-1, per_sample=False):
    """(counts (B or 1, n, n) int64, skipped): row = ground truth, column = prediction."""
    p, g = labels_of(pred, pred_kind, n), labels_of(gt, gt_kind, n)
    B = p.shape[0]
    raw = np.asarray(gt).reshape(B, *p.shape[-2:])
    use = np.ones(p.shape, bool)
    if mask is not None:
        use &= np.asarray(mask).reshape(p.shape) != 0
    if ignore >= 0:
        use &= raw.astype(np.float64) != float(ignore)
    bad = use & ((p < 0) | (g < 0))
    use &= ~bad
    counts = np.zeros((B if per_sample else 1, n, n), np.int64)
    bi = np.broadcast_to(np.arange(B).reshape(B, 1, 1), p.shape) if per_sample else np.zeros(p.shape, np.int64)
    np.add.at(counts, (bi[use], g[use], p[use]), 1)
    return counts, int(bad.sum())


def scores(conf):
    """pixel_acc, mean_acc, mean_iou, fw_iou, per_class_iou, per_class_acc, absent of an (n, n) matrix, float64; classes
    with neither ground truth nor prediction are left out of the means (nan per class)."""
    c = np.asarray(conf, np.float64)
    total, tp, gt, pr = c.sum(), np.diag(c), c.sum(1), c.sum(0)
    present = (gt + pr) > 0
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = np.where(present, tp / (gt + pr - tp), np.nan)
        acc = np.where(gt > 0, tp / gt, np.nan)
    return dict(pixel_acc=tp.sum() / total if total else float('nan'),
                mean_acc=float(np.nanmean(acc)) if (gt > 0).any() else float('nan'),
                mean_iou=float(np.nanmean(iou)) if present.any() else float('nan'),
                fw_iou=float(np.nansum(np.where(gt > 0, gt * iou, 0.0)) / total) if total else float('nan'),
                per_class_iou=iou, per_class_acc=acc, absent=int((~present).sum()))


def rel_err(got, ref):
    """tests/README.md's metric: maximum error over maximum |ref|."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    err = np.abs(got - ref)
    if not np.isfinite(err).all():
        return float('inf')
    return float(err.max()) / max(float(np.abs(ref).max()), 1e-30)
