"""Evaluation metrics on the device: SSIM / PSNR / L1 of a generated image against the real one (inside the edited box),
pixel accuracy and IoU of a predicted layout, IoU of a generated object mask, and the contour measures of both (boundary
F-score, average symmetric surface distance, Hausdorff distance, the "trimap" band) on an exact distance transform, and
the panoptic quality of a layout (instances matched at IoU > 0.5).  The
reference ships no metric code; the definitions are those of include/him.h "Evaluation metrics", "Distance transform
and boundary metrics" and "Panoptic matching".  Every function queues device work on the current stream
and returns device tensors; nothing synchronises with the host before ``Evaluator.summary()`` as long as every argument
is a device tensor: a ``box`` given as a list or array (and any host tensor) is copied to the device first, which waits
on the host.  The device calls of one operator share one cached workspace per device (``ops.image_metrics`` /
``ops.confusion``); a call on another stream than the last one waits for that one's event first."""
import json
import math
from collections import OrderedDict

import numpy as np
import torch

from .. import ops


def _mapping(data_range, as_bytes):
    """``as_bytes``: the inputs are generator-range tensors in [-1, 1] and are compared as the bytes ``tensor2im`` saves
    (the preset of him_image_metrics); otherwise they are compared as they stand."""
    if as_bytes:
        return dict(scale=127.5, offset=127.5, quantize=True, data_range=float(data_range))
    return dict(scale=1.0, offset=0.0, quantize=False, data_range=float(data_range))


def _box(box, B, device):
    """None, or a (B, 4) int32 device tensor of inclusive (xmin, ymin, xmax, ymax) from a tensor / array / sequence.  Only
    a device tensor passes without a host-to-device copy (a pageable copy synchronises with the host)."""
    if box is None:
        return None
    if not torch.is_tensor(box):
        box = torch.from_numpy(np.asarray(box, dtype=np.int32).reshape(-1, 4))
    box = box.reshape(-1, 4).to(device=device, dtype=torch.int32, non_blocking=True)
    if box.shape[0] == 1 and B > 1:
        box = box.expand(B, 4)
    return box.contiguous()


def _image_pair(a, b):
    a = a if a.dim() == 4 else a.unsqueeze(0)
    b = b if b.dim() == 4 else b.unsqueeze(0)
    if not a.is_cuda:
        a = a.cuda()
    return a.float(), b.to(a.device).float()


def image_sums(a, b, data_range=255., as_bytes=True, box=None, want_map=False):
    """The raw (B, C, 5) float64 device sums of ``ops.image_metrics`` (and the SSIM map or None)."""
    a, b = _image_pair(a, b)
    return ops.image_metrics(a, b, box=_box(box, a.shape[0], a.device), want_map=want_map, **_mapping(data_range, as_bytes))


def _ratio(sums, num, den):
    return sums[:, :, num].sum(1) / sums[:, :, den].sum(1)          # 0 / 0 = nan: no window / no pixel


def ssim(a, b, data_range=255., as_bytes=True, box=None, return_map=False):
    """Per-image SSIM (B,) float64 on the device, the mean over channels and windows; nan where no 11 x 11 window fits.
    With ``return_map`` also the (B, C, H-10, W-10) map (whole images only)."""
    sums, smap = image_sums(a, b, data_range, as_bytes, box, return_map)
    out = _ratio(sums, 0, 1)
    return (out, smap) if return_map else out


def psnr(a, b, data_range=255., as_bytes=True, box=None):
    """Per-image 10 log10(L^2 / MSE) (B,) float64 on the device; inf for identical images, nan for an empty box."""
    sums, _ = image_sums(a, b, data_range, as_bytes, box)
    return 10.0 * torch.log10(float(data_range) ** 2 / _ratio(sums, 2, 4))


def l1(a, b, data_range=255., as_bytes=True, box=None):
    """Per-image mean absolute error (B,) float64 on the device, in the units of the mapped values."""
    sums, _ = image_sums(a, b, data_range, as_bytes, box)
    return _ratio(sums, 3, 4)


def _labels(t, keys):
    """What the models hand out: a tensor, a dict of generate() / reconstruct(), or the 3-tuple of gen_layout()."""
    if isinstance(t, dict):
        for k in keys:
            if k in t:
                return t[k]
        raise KeyError('none of %s in %s' % (keys, sorted(t)))
    if isinstance(t, (tuple, list)):
        return t[-1]
    return t


def _plane(t):
    if not t.is_cuda:
        t = t.cuda()
    if t.dtype not in (torch.uint8, torch.int32, torch.int64, torch.float32):
        t = t.float()
    return t


def confusion_matrix(pred, gt, n_class, mask=None, ignore_label=None, per_sample=False, out=None, pred_kind=None):
    """``(counts, status)`` on the device: int64 (B or 1, n_class, n_class), row = ground truth, column = prediction, and
    the status record of ``ops.confusion``.  ``pred``: ids, or (B, C > 1, H, W) scores; ``out`` accumulates."""
    pred = _plane(_labels(pred, ('comb_pred_label', 'comb_recon_label')))
    gt = _plane(gt).to(pred.device)
    if mask is not None:
        mask = mask.to(pred.device).float()
    return ops.confusion(pred, gt, n_class, mask=mask, ignore=-1 if ignore_label is None else int(ignore_label),
                         per_sample=per_sample, out=out, pred_kind=pred_kind)


def segmentation_scores(conf):
    """pixel_acc, mean_acc, mean_iou, fw_iou, per_class_iou, per_class_acc and n_absent of an (n, n) (or (1, n, n))
    confusion matrix, in float64 on the host.  Classes absent from both prediction and ground truth are left out of the
    means (their per-class entries are nan) and counted in ``n_absent``."""
    c = conf.detach().cpu().numpy() if torch.is_tensor(conf) else np.asarray(conf)
    c = c.reshape(c.shape[-2], c.shape[-1]).astype(np.float64)
    tp, n_gt, n_pred, total = np.diagonal(c), c.sum(axis=1), c.sum(axis=0), float(c.sum())
    union = n_gt + n_pred - tp
    seen, has_gt = (n_gt + n_pred) > 0, n_gt > 0
    iou = np.full(len(tp), np.nan)
    acc = np.full(len(tp), np.nan)
    iou[seen] = tp[seen] / union[seen]
    acc[has_gt] = tp[has_gt] / n_gt[has_gt]
    nan = float('nan')
    return OrderedDict([
        ('pixel_acc', float(tp.sum()) / total if total > 0 else nan),
        ('mean_acc', float(acc[has_gt].mean()) if has_gt.any() else nan),
        ('mean_iou', float(iou[seen].mean()) if seen.any() else nan),
        ('fw_iou', float((n_gt[has_gt] * iou[has_gt]).sum()) / total if total > 0 else nan),
        ('per_class_iou', iou), ('per_class_acc', acc), ('n_absent', int((~seen).sum()))])


def mask_iou(prob, gt_mask):
    """Per-sample intersection over union (B,) float64 on the device of ``prob > 0.5`` against ``gt_mask`` (0 / 1), from
    the n = 2 per-sample confusion matrix; nan where both are empty."""
    prob = _plane(_labels(prob, ('obj_pred_label', 'obj_recon_label'))).float()
    counts, _ = ops.confusion(prob, _plane(gt_mask).to(prob.device), 2, per_sample=True, pred_kind='prob')
    c = counts.double()
    return c[:, 1, 1] / (c[:, 1, 1] + c[:, 0, 1] + c[:, 1, 0])


def box_of_mask(mask):
    """(B, 4) int32 device tensor: the inclusive extent (xmin, ymin, xmax, ymax) of the non-zero pixels of a (B, 1, H, W)
    mask; an all-zero mask gives an empty box.  Device reductions only, no host synchronisation."""
    m = (mask.reshape(mask.shape[0], mask.shape[-2], mask.shape[-1]) != 0)
    rows, cols = m.any(2).int(), m.any(1).int()
    H, W = rows.shape[1], cols.shape[1]
    none = rows.sum(1) == 0
    ymin, xmin = rows.argmax(1), cols.argmax(1)
    ymax, xmax = H - 1 - rows.flip(1).argmax(1), W - 1 - cols.flip(1).argmax(1)
    box = torch.stack([xmin, ymin, xmax, ymax], 1)
    return torch.where(none[:, None], -1, box).to(torch.int32).contiguous()        # (-1, -1, -1, -1) clips to nothing


_EDT_CHUNK_PIXELS = 1 << 26     # job pixels per him_edt call of boundary_scores: 256 MiB of int32 distances


def _id_planes(t, keys, pred_kind=None):
    """(B, H, W) device id planes of what ``confusion_matrix`` accepts; scores and probabilities go through
    ``ops.label_ids`` (the arg-max and threshold rules of him_confusion)."""
    t = _plane(_labels(t, keys))
    if pred_kind == 'prob':
        return ops.label_ids(t.float().reshape(-1, 1, t.shape[-2], t.shape[-1]), 'prob')
    if t.dim() == 4 and t.shape[1] > 1:
        return ops.label_ids(t.float(), 'scores')
    return t.reshape(-1, t.shape[-2], t.shape[-1]).contiguous()


def _boundary_raw(pred, gt, classes, tol2):
    """counts (B, n, 2, 4) int64 and sumd (B, n, 2) float64 of two (B, H, W) id planes: [..., 0, :] the boundary of the
    prediction measured against the ground truth's, [..., 1, :] the mirror image."""
    B, H, W = pred.shape
    per = max(1, _EDT_CHUNK_PIXELS // (B * H * W))
    cnt, sm = [], []
    for i in range(0, len(classes), per):
        part = classes[i:i + per]
        jobs = ops.edt_jobs(B, part, 'boundary_of', pred.device)
        d_gt = ops.distance_transform(gt, jobs)[0]
        cp, sp = ops.boundary_stats(pred, jobs, d_gt, tol2)
        d_pred = ops.distance_transform(pred, jobs)[0]
        cg, sg = ops.boundary_stats(gt, jobs, d_pred, tol2)
        cnt.append(torch.stack([cp, cg], 1).reshape(B, len(part), 2, 4))
        sm.append(torch.stack([sp, sg], 1).reshape(B, len(part), 2))
    return torch.cat(cnt, 1), torch.cat(sm, 1)


def _boundary_measures(counts, sumd):
    """precision, recall, f1, assd, hausdorff (float64) of counts (..., 2, 4) and sumd (..., 2)."""
    c = counts.double()
    n_p, n_g = c[..., 0, 0], c[..., 1, 0]
    both, none = (n_p > 0) & (n_g > 0), (n_p == 0) & (n_g == 0)
    zero, nan = torch.zeros_like(n_p), torch.full_like(n_p, float('nan'))
    prec = torch.where(both, c[..., 0, 1] / n_p, zero)
    rec = torch.where(both, c[..., 1, 1] / n_g, zero)
    f1 = torch.where(prec + rec > 0, 2 * prec * rec / (prec + rec), zero)
    assd = torch.where(both, (sumd[..., 0] + sumd[..., 1]) / (n_p + n_g), nan)
    hd = torch.where(both, torch.sqrt(torch.maximum(c[..., 0, 2], c[..., 1, 2]).clamp(min=0)), nan)
    return OrderedDict([('precision', torch.where(none, nan, prec)), ('recall', torch.where(none, nan, rec)),
                        ('f1', torch.where(none, nan, f1)), ('assd', assd), ('hausdorff', hd)])


def diag_tolerance(H, W, frac=0.0075):
    """The usual boundary tolerance in pixels: a fraction of the image diagonal."""
    return float(frac) * math.sqrt(float(H) * H + float(W) * W)


def boundary_scores(pred, gt, n_class, tolerance=2.0, classes=None):
    """Contour measures of a predicted layout per sample and class, as device tensors of shape (B, n): ``precision``,
    ``recall``, ``f1`` (the boundary F-score within ``tolerance`` pixels), ``assd`` (average symmetric surface distance),
    ``hausdorff``, all float64, plus the integer ``counts`` (B, n, 2, 4) and the distance sums ``sumd`` (B, n, 2) of
    ``ops.boundary_stats`` ([..., 0, :] prediction against ground truth, [..., 1, :] the mirror image).  The boundary of
    class c is its inner 4-neighbour boundary; definitions in include/him.h "Distance transform and boundary metrics":
    nan where a class has no boundary in either map, zeros (and nan distances) where it has one in exactly one.
    ``pred``, ``gt``: what ``confusion_matrix`` accepts.  ``classes``: the ids to score, default ``range(n_class)``,
    processed in chunks that bound the distance maps to 256 MiB.  No host synchronisation (a class list that is not a run
    of consecutive ids is copied to the device)."""
    p = _id_planes(pred, ('comb_pred_label', 'comb_recon_label'))
    g = _id_planes(gt, ()).to(p.device)
    if p.shape != g.shape:
        raise ValueError('boundary_scores: pred %s and gt %s differ' % (tuple(p.shape), tuple(g.shape)))
    classes = list(range(int(n_class))) if classes is None else [int(c) for c in classes]
    tol2 = int(math.floor(float(tolerance) ** 2))
    counts, sumd = _boundary_raw(p, g, classes, tol2)
    out = _boundary_measures(counts, sumd)
    out['counts'], out['sumd'] = counts, sumd
    return out


def mask_boundary_scores(prob, gt_mask, tolerance=2.0):
    """``boundary_scores`` of ``prob > 0.5`` against a 0 / 1 mask, shape (B,): the outline quality of a generated object
    mask (the box2mask measure)."""
    p = _id_planes(prob, ('obj_pred_label', 'obj_recon_label'), 'prob')
    g = _plane(gt_mask).to(p.device)
    g = ops.label_ids(g.float().reshape(-1, 1, g.shape[-2], g.shape[-1]), 'prob') if g.dtype == torch.float32 \
        else g.reshape(-1, g.shape[-2], g.shape[-1]).contiguous()
    if p.shape != g.shape:
        raise ValueError('mask_boundary_scores: prob %s and gt_mask %s differ' % (tuple(p.shape), tuple(g.shape)))
    counts, sumd = _boundary_raw(p, g, [1], int(math.floor(float(tolerance) ** 2)))
    out = OrderedDict((k, v[:, 0]) for k, v in _boundary_measures(counts, sumd).items())
    out['counts'], out['sumd'] = counts[:, 0], sumd[:, 0]
    return out


def boundary_band(gt, radius):
    """fp32 (B, 1, H, W) device mask of the pixels within ``radius`` of any class boundary of ``gt`` (squared distance
    <= floor(radius^2) to a pixel with a differing 4-neighbour), ready for ``confusion_matrix(mask=...)``: the confusion
    matrix restricted to it gives the "trimap" IoU."""
    g = _id_planes(gt, ())
    dist2 = ops.distance_transform(g, rule='any_boundary')[0]
    return (dist2 <= int(math.floor(float(radius) ** 2))).float().unsqueeze(1)


def panoptic_scores(counts, iou_sum, things=None):
    """Panoptic quality from the (n, 3) tp / fp / fn counts and the (n,) IoU sums of ``ops.panoptic_match``, in float64
    on the host.  Per class ``pq = iou / (tp + fp/2 + fn/2)``, ``sq = iou / tp``, ``rq = tp / (tp + fp/2 + fn/2)``, each
    nan where its denominator is 0.  ``pq`` and ``rq`` are the means over the classes with tp + fp + fn > 0, ``sq`` the
    mean over those of them where it is defined (tp > 0); classes seen in neither map are counted in ``n_absent``.  With
    ``things`` (the class ids that have instances) also ``pq_things`` and ``pq_stuff``, the same mean over the two groups."""
    c = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    s = iou_sum.detach().cpu().numpy() if torch.is_tensor(iou_sum) else np.asarray(iou_sum)
    c, s = c.reshape(-1, 3).astype(np.float64), s.reshape(-1).astype(np.float64)
    tp, den = c[:, 0], c[:, 0] + 0.5 * c[:, 1] + 0.5 * c[:, 2]
    seen = c.sum(1) > 0
    with np.errstate(divide='ignore', invalid='ignore'):
        pq = np.where(den > 0, s / den, np.nan)
        sq = np.where(tp > 0, s / tp, np.nan)
        rq = np.where(den > 0, tp / den, np.nan)
    out = OrderedDict([('pq', _nanmean(pq[seen])), ('sq', _nanmean(sq[seen])), ('rq', _nanmean(rq[seen]))])
    if things is not None:
        is_thing = np.zeros(len(pq), bool)
        is_thing[[int(t) for t in things if 0 <= int(t) < len(pq)]] = True
        out['pq_things'], out['pq_stuff'] = _nanmean(pq[seen & is_thing]), _nanmean(pq[seen & ~is_thing])
    out['per_class_pq'], out['n_absent'] = pq, int((~seen).sum())
    return out


def _seg_planes(t):
    t = _plane(t)
    if t.dtype not in (torch.uint8, torch.int32, torch.int64):
        t = t.to(torch.int32)
    return t.reshape(-1, t.shape[-2], t.shape[-1]).contiguous()


def panoptic_quality(pred, gt, n_class, things, gt_inst=None, connectivity=8, min_area=1, ignore_label=None, mask=None,
                     out=None, max_segments=1024):
    """``(counts, iou_sum, status)`` of ``ops.panoptic_match`` on the device for a predicted layout against the ground
    truth.  ``pred``, ``gt``: what ``confusion_matrix`` accepts (scores and probabilities go through ``ops.label_ids``).
    Predicted segments are the connected components of the classes in ``things`` (``ops.label_instances_launch``; every
    other class is one segment per plane); ground-truth segments come from ``gt_inst`` (the dataset's instance map, ids
    0..65535) when given, else from the same labelling of ``gt``.  A labelling that reports a flag of its own (more than
    ``max_segments`` objects, a class outside 0..255) sets ``ops.PQ_CCL`` in that plane's status on the device.  ``out``
    accumulates.  No host synchronisation."""
    p = _id_planes(pred, ('comb_pred_label', 'comb_recon_label'))
    g = _id_planes(gt, ()).to(p.device)
    if p.shape != g.shape:
        raise ValueError('panoptic_quality: pred %s and gt %s differ' % (tuple(p.shape), tuple(g.shape)))
    label = dict(connectivity=connectivity, min_area=min_area, max_objects=int(max_segments))
    p_seg, _, st = ops.label_instances_launch(p, things, **label)
    ccl = st['out'][:, 1].clone()            # the next labelling of this shape overwrites the record
    if gt_inst is None:
        g_seg, _, st = ops.label_instances_launch(g, things, **label)
        ccl = ccl | st['out'][:, 1]
    else:
        g_seg = _seg_planes(gt_inst).to(p.device)
    if mask is not None:
        mask = mask.to(p.device).float()
    res = ops.panoptic_match(p_seg, p, g_seg, g, n_class, mask=mask, ignore=-1 if ignore_label is None else int(ignore_label),
                             max_segments=max_segments, out=out)
    res[2][:, 2].bitwise_or_((ccl != 0).to(torch.int32) * ops.PQ_CCL)
    return res[:3]


PANOPTIC_KEYS = ('pq', 'sq', 'rq', 'pq_things', 'pq_stuff', 'per_class_pq', 'n_segments_gt', 'n_segments_pred',
                 'panoptic_flags')


def swd_tables(seed, C, n_dirs=512, device='cuda'):
    """The direction table of the sliced Wasserstein distance: (49 C, n_dirs) fp32 on ``device``, every column a seeded
    normal draw (``numpy.random.RandomState(seed)``, float64) scaled to unit length.  Drawn on the host, uploaded once."""
    d = np.random.RandomState(int(seed) & 0x7fffffff).randn(int(n_dirs), 49 * int(C))
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    return torch.from_numpy(np.ascontiguousarray(d.T).astype(np.float32)).to(device)


def swd_positions(seed, index, B, n_patches, h, w, level=0, which=0, device=None):
    """The patch corners (B, n_patches, 2) int32 (y, x) of the images ``index .. index + B - 1`` of set ``which`` on a
    level of h x w: uniform over [0, h - 7] x [0, w - 7], one seeded host generator per (seed, set, level, image), so
    the table of an image does not depend on how the set is cut into batches.  A host array, or a device tensor."""
    out = np.empty((int(B), int(n_patches), 2), np.int32)
    for b in range(int(B)):
        rs = np.random.RandomState([int(seed) & 0x7fffffff, int(which), int(level), int(index) + b])
        out[b, :, 0] = rs.randint(0, h - 6, int(n_patches))
        out[b, :, 1] = rs.randint(0, w - 6, int(n_patches))
    return out if device is None else torch.from_numpy(out).to(device)


class SlicedWasserstein(object):
    """Streams two image sets (``add(fake, real)``, batch by batch) into per-level descriptor matrices on the device and
    gives the sliced Wasserstein distance of every Laplacian level (include/him.h "Set-level metrics").  The buffers
    grow geometrically on the device; nothing goes to the host."""

    def __init__(self, n_patches=128, n_dirs=512, levels=None, seed=0, same_positions=False):
        self.n_patches, self.n_dirs, self.seed = int(n_patches), int(n_dirs), int(seed)
        self.want_levels, self.same_positions = levels, bool(same_positions)
        self.n_images, self.shape, self.levels, self.dirs = 0, None, 0, None
        self._desc, self._stats, self._rows, self.clamped = None, None, 0, None

    def add(self, fake, real):
        fake, real = _image_pair(fake, real)
        if fake.shape != real.shape:
            raise ValueError('sliced_wasserstein: fake %s and real %s differ' % (tuple(fake.shape), tuple(real.shape)))
        B, C, H, W = fake.shape
        dev, n = fake.device, self.n_patches
        if self.shape is None:
            self.shape, self.levels = (C, H, W), ops.lap_levels(H, W, self.want_levels)
            self.dirs = swd_tables(self.seed, C, self.n_dirs, dev)
            self._desc = [[None, None] for _ in range(self.levels)]
            self._stats = [[ops.swd_stats(C, dev), ops.swd_stats(C, dev)] for _ in range(self.levels)]
            with torch.cuda.device(dev):
                self.clamped = torch.zeros(1, dtype=torch.int32, device=dev)
        elif self.shape != (C, H, W):
            raise ValueError('sliced_wasserstein: images of %s after images of %s' % ((C, H, W), self.shape))
        need = self._rows + B * n
        for which, x in enumerate((fake, real)):
            for l, lv in enumerate(ops.lap_pyramid(x, self.levels)):
                pos = swd_positions(self.seed, self.n_images, B, n, H >> l, W >> l, l,
                                    0 if self.same_positions else which, dev)
                desc = self._desc[l][which]
                if desc is None or desc.shape[0] < need:
                    with torch.cuda.device(dev):
                        grown = torch.empty((max(need, 2 * (0 if desc is None else desc.shape[0])), 49 * C),
                                            dtype=torch.float32, device=dev)
                    if desc is not None:
                        grown[:self._rows].copy_(desc[:self._rows])
                    desc = self._desc[l][which] = grown
                ops.swd_gather(lv, pos, desc, self._rows, self._stats[l][which], self.clamped)
        self._rows, self.n_images = need, self.n_images + B
        return self

    @property
    def n_descriptors(self):
        return self._rows

    def distances(self):
        """(levels,) float64 on the device, finest level first; NaN for a level with a channel that does not vary."""
        if not self._rows:
            raise ValueError('sliced_wasserstein: no images were added')
        return torch.stack([ops.sliced_wasserstein(d[0][:self._rows], d[1][:self._rows], s[0], s[1], self.dirs)[0]
                            for d, s in zip(self._desc, self._stats)])


def sliced_wasserstein(fake, real, n_patches=128, n_dirs=512, levels=None, seed=0, same_positions=False):
    """The sliced Wasserstein distance between two whole image sets (N, C, H, W), C = 1 or 3, per Laplacian level:
    (levels,) float64 on the device, finest first (Karras et al. 2018 report these times 1e3).  ``n_patches`` 7 x 7
    patches per image and level, normalised per set, level and channel, projected onto ``n_dirs`` seeded unit directions,
    sorted, and compared rank by rank.  ``same_positions`` uses one corner table for both sets."""
    return SlicedWasserstein(n_patches, n_dirs, levels, seed, same_positions).add(fake, real).distances()


def kid_subsets(seed, which, n, n_subsets, subset_size):
    """The subset table of KID: (n_subsets, subset_size) int32 on the host, row s a draw without replacement from
    ``range(n)`` by ``numpy.random.RandomState([seed, which, s])`` (``which``: 0 the generated set, 1 the real one).
    Seeded on the host and uploaded once, like ``swd_positions``; it depends on the size of the set only, not on how
    the set was batched."""
    n, n_subsets, subset_size = int(n), int(n_subsets), int(subset_size)
    if not 1 <= subset_size <= n or n_subsets < 1:
        raise ValueError('kid_subsets: %d subsets of %d rows out of %d' % (n_subsets, subset_size, n))
    out = np.empty((n_subsets, subset_size), np.int32)
    for s in range(n_subsets):
        out[s] = np.random.RandomState([int(seed) & 0x7fffffff, int(which), s]).permutation(n)[:subset_size]
    return out


def _psd_eigenvalues(lam):
    """Eigenvalues of a positive semi-definite matrix as computed: those below D eps max(lambda) are rounding of the
    null space (fewer rows than dimensions) and count as zero, so that their square roots -- sqrt(eps) each, and of
    either sign before the clipping -- do not reach the result."""
    lam = np.maximum(lam, 0.0)
    if lam.size:
        lam[lam < len(lam) * np.finfo(np.float64).eps * lam.max()] = 0.0
    return lam


def frechet_from_moments(n1, sum1, second1, n2, sum2, second2):
    """The Frechet distance |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2) between the Gaussians fitted to two sets,
    from their row counts, column sums (D,) and X^T X (D, D): float64 numpy on the host, O(D^3) whatever the set size.
    Means and covariances with ddof = 1.  tr (S1 S2)^(1/2) is the sum of sqrt(max(lambda, 0)) over the eigenvalues of the
    symmetric S1^(1/2) S2 S1^(1/2), which has the spectrum of S1 S2: two ``numpy.linalg.eigh`` calls, no complex
    arithmetic, and rank-deficient covariances (fewer rows than dimensions) give a finite value.  NaN below 2 rows."""
    n1, n2 = int(n1), int(n2)
    if n1 < 2 or n2 < 2:
        return float('nan')
    mu, cov = [], []
    for n, s, q in ((n1, sum1, second1), (n2, sum2, second2)):
        s, q = np.asarray(s, np.float64).reshape(-1), np.asarray(q, np.float64)
        m = s / n
        mu.append(m)
        cov.append((q.reshape(len(s), len(s)) - n * np.outer(m, m)) / (n - 1))
    lam, Q = np.linalg.eigh((cov[0] + cov[0].T) * 0.5)
    root = (Q * np.sqrt(_psd_eigenvalues(lam))) @ Q.T                    # the symmetric square root of S1
    M = root @ cov[1] @ root
    lam = _psd_eigenvalues(np.linalg.eigvalsh((M + M.T) * 0.5))
    d = mu[0] - mu[1]
    return float(d @ d + np.trace(cov[0]) + np.trace(cov[1]) - 2.0 * np.sqrt(lam).sum())


VGG_SLICE_CHANNELS = (64, 128, 256, 512, 512)


class FeatureDistance(object):
    """Streams two sets into feature-space descriptors on the device and gives KID and the Frechet distance between them
    (include/him.h "Feature-space set metrics").  ``add(fake, real)`` runs a frozen ``Vgg19`` (the one given, e.g.
    ``model.criterionVGG.vgg``; otherwise one with the build's seeded synthetic weights is made on first use) without
    autograd, one image per pass so that a row does not depend on the batching, and writes the plane means of the slices
    ``layers`` (0 = relu1_1 .. 4 = relu5_1, concatenated) into rows of geometrically grown device buffers; ``add_features`` takes ready-made (n, D) fp32 device rows of any extractor
    instead, and there the two sets may differ in size.  Every new row is folded into float64 moment accumulators as it
    arrives.  The Frechet distance is called ``frechet``, not FID: the features are not Inception's."""

    def __init__(self, layers=(4,), n_subsets=100, subset_size=1000, seed=0, vgg=None, nearest_k=None):
        self.layers = tuple(int(l) for l in layers)
        # opt-in: the k of ``prdc()`` (precision, recall, density, coverage by k-nearest neighbours)
        self.nearest_k = None if nearest_k is None else int(nearest_k)
        if self.nearest_k is not None and not 1 <= self.nearest_k <= ops.KNN_MAX_K:
            raise ValueError('feature_distances: nearest_k %d outside 1..%d' % (self.nearest_k, ops.KNN_MAX_K))
        if not self.layers or any(l < 0 or l > 4 for l in self.layers):
            raise ValueError('feature_distances: layers %r, each one of 0..4' % (layers,))
        self.n_subsets, self.subset_size, self.seed, self.vgg = int(n_subsets), int(subset_size), int(seed), vgg
        if self.n_subsets < 1 or self.subset_size < 2:
            raise ValueError('feature_distances: n_subsets %d (>= 1), subset_size %d (>= 2)' % (self.n_subsets, self.subset_size))
        self.D = None
        self._rows, self._n, self._sum, self._second = [None, None], [0, 0], [None, None], [None, None]

    def _reserve(self, which, n, D, dev):
        if self.D is None:
            self.D = int(D)
            for w in (0, 1):
                self._sum[w], self._second[w] = ops.feat_moment_buffers(self.D, dev)
        elif self.D != int(D):
            raise ValueError('feature_distances: rows of %d features after rows of %d' % (D, self.D))
        buf, need = self._rows[which], self._n[which] + n
        if buf is None or buf.shape[0] < need:
            with torch.cuda.device(dev):
                grown = torch.empty((max(need, 2 * (0 if buf is None else buf.shape[0])), self.D), dtype=torch.float32,
                                    device=dev)
            if buf is not None:
                grown[:self._n[which]].copy_(buf[:self._n[which]])
            buf = self._rows[which] = grown
        return buf

    def _fold(self, which, n):
        ops.feat_moments(self._rows[which], self._n[which], n, self._sum[which], self._second[which])
        self._n[which] += n

    def add(self, fake, real):
        fake, real = _image_pair(fake, real)
        if fake.shape != real.shape or fake.shape[1] != 3 or min(fake.shape[-2:]) < 16:
            raise ValueError('feature_distances: fake %s and real %s must be equal (B, 3, H, W) batches with '
                             'min(H, W) >= 16' % (tuple(fake.shape), tuple(real.shape)))
        if self.vgg is None:
            from ..models.layer_util import Vgg19
            from .. import synth
            self.vgg = Vgg19()
            self.vgg.load_state_dict(synth.init_state_dict(self.vgg.state_dict(), 3, 'vgg'))
            self.vgg.to(fake.device)
        B, D = fake.shape[0], sum(VGG_SLICE_CHANNELS[l] for l in self.layers)
        for which, x in enumerate((fake, real)):
            buf = self._reserve(which, B, D, x.device)
            for b in range(B):
                # one image per pass: the convolution kernels are chosen by shape, batch size included, so only this
                # makes an image's row independent of the batch it arrived in
                with torch.no_grad():
                    maps = self.vgg(x[b:b + 1].contiguous())
                c0 = 0
                for l in self.layers:
                    c0 = ops.feat_pool(maps[l], buf, self._n[which] + b, c0)
            self._fold(which, B)
        return self

    def add_features(self, fake=None, real=None):
        for which, rows in enumerate((fake, real)):
            if rows is None:
                continue
            if not torch.is_tensor(rows) or not rows.is_cuda or rows.dtype != torch.float32 or rows.dim() != 2:
                raise ValueError('feature_distances: features must be (n, D) fp32 device tensors')
            if rows.shape[0] == 0:
                continue
            buf = self._reserve(which, rows.shape[0], rows.shape[1], rows.device)
            buf[self._n[which]:self._n[which] + rows.shape[0]].copy_(rows.detach())
            self._fold(which, rows.shape[0])
        return self

    @property
    def n_features(self):
        return (self._n[0], self._n[1])

    def features(self, which):
        """The (n, D) fp32 device rows of set ``which`` (0 generated, 1 real): a view of the buffer."""
        return self._rows[which][:self._n[which]]

    def kid_sums(self):
        """``(sums (n_subsets, 3) float64, status, m)`` of ``ops.kid_sums`` on the seeded subsets."""
        m = min(self.subset_size, self._n[0], self._n[1])
        if m < 2:
            raise ValueError('feature_distances: KID needs 2 rows per set, got %d and %d' % self.n_features)
        dev = self._rows[0].device
        ix = torch.from_numpy(kid_subsets(self.seed, 0, self._n[0], self.n_subsets, m)).to(dev)
        iy = torch.from_numpy(kid_subsets(self.seed, 1, self._n[1], self.n_subsets, m)).to(dev)
        out, status = ops.kid_sums(self.features(0), self.features(1), ix, iy, 0.0, 1.0)
        return out, status, m

    def kid(self):
        """``(mean, std)`` float64 device scalars over the subsets of the unbiased MMD^2 estimate with the kernel
        (x.y / D + 1)^3; ``subset_size`` is clipped to the smaller set.  ``std`` is the population deviation."""
        s, _, m = self.kid_sums()
        est = (s[:, 0] + s[:, 1]) / float(m * (m - 1)) - 2.0 * s[:, 2] / float(m * m)
        return est.mean(), est.std(unbiased=False)

    def frechet(self):
        """The Frechet distance as a host float (one host synchronisation); NaN below 2 rows in either set."""
        if min(self._n) < 2:
            return float('nan')
        return frechet_from_moments(self._n[0], self._sum[0].cpu().numpy(), self._second[0].cpu().numpy(),
                                    self._n[1], self._sum[1].cpu().numpy(), self._second[1].cpu().numpy())

    def prdc_counts(self, nearest_k=None):
        """``(k, row_fake_in_real, col_real_covered, row_real_in_fake, status)``: the int32 device counts of
        ``ops.knn_membership`` of the generated rows against the real rows' k-th-neighbour radii (rows and columns) and of
        the real rows against the generated rows' radii (rows); two radii calls and two membership calls."""
        k = _nearest_k(self.nearest_k if nearest_k is None else nearest_k)
        if min(self._n) <= k:
            raise ValueError('feature_distances: precision / recall with k = %d need more than k rows per set, got %d and %d'
                             % ((k,) + self.n_features))
        fake, real = self.features(0), self.features(1)
        r_real, status = ops.knn_radii(real, k)
        r_fake, _ = ops.knn_radii(fake, k, status)
        row_fr, col_r, _ = ops.knn_membership(fake, real, r_real, True, status)
        row_rf, _, _ = ops.knn_membership(real, fake, r_fake, False, status)
        return k, row_fr, col_r, row_rf, status

    def prdc(self, nearest_k=None):
        """``OrderedDict(precision, recall, density, coverage)`` of float64 device scalars on the rows held so far, with
        ``nearest_k`` neighbours (default: the constructor's, else 5).  The generated set is tested against the real
        rows' radii for precision, density and coverage, the real set against the generated rows' radii for recall.  All
        four are NaN when either set has at most k rows."""
        k = _nearest_k(self.nearest_k if nearest_k is None else nearest_k)
        if min(self._n) <= k:
            dev = self._rows[0].device if self._rows[0] is not None else None
            return OrderedDict((key, torch.tensor(float('nan'), dtype=torch.float64, device=dev)) for key in PRDC_KEYS[:4])
        return prdc_from_counts(*self.prdc_counts(k)[:4])


def _nearest_k(k):
    k = 5 if k is None else int(k)
    if not 1 <= k <= ops.KNN_MAX_K:
        raise ValueError('feature_distances: nearest_k %d outside 1..%d' % (k, ops.KNN_MAX_K))
    return k


def prdc_from_counts(k, row_fake_in_real, col_real_covered, row_real_in_fake):
    """Precision, recall, density and coverage from the membership counts of ``ops.knn_membership``, as an
    ``OrderedDict`` of float64 scalars on the device of the counts (no host synchronisation):
    precision = the share of generated rows inside some real row's k-th-neighbour ball (``row_fake_in_real > 0``);
    density = the number of such balls around a generated row, summed, over k times the generated rows;
    coverage = the share of real rows whose ball holds a generated row (``col_real_covered > 0``);
    recall = the share of real rows inside some generated row's ball (``row_real_in_fake > 0``)."""
    k = int(k)
    for t in (row_fake_in_real, col_real_covered, row_real_in_fake):
        if not torch.is_tensor(t) or t.dim() != 1 or t.numel() < 1 or t.dtype.is_floating_point:
            raise ValueError('prdc_from_counts: the counts must be non-empty one-dimensional integer tensors')
    if k < 1:
        raise ValueError('prdc_from_counts: k %d < 1' % k)
    f64 = torch.float64
    return OrderedDict([('precision', (row_fake_in_real > 0).to(f64).mean()),
                        ('recall', (row_real_in_fake > 0).to(f64).mean()),
                        ('density', row_fake_in_real.sum().to(f64) / float(k * row_fake_in_real.numel())),
                        ('coverage', (col_real_covered > 0).to(f64).mean())])


def feature_prdc(fake, real, nearest_k=5, **kw):
    """Precision, recall, density and coverage between two whole image sets (N, 3, H, W) in VGG19 feature space:
    ``OrderedDict(precision, recall, density, coverage)`` of float64 device scalars; ``kw``: the arguments of
    ``FeatureDistance``."""
    return FeatureDistance(nearest_k=nearest_k, **kw).add(fake, real).prdc()


def feature_distances(fake, real, **kw):
    """KID and the Frechet distance between two whole image sets (N, 3, H, W) in VGG19 feature space:
    ``dict(kid, kid_std, frechet, n_features)`` with the first two float64 device scalars; ``kw``: the arguments of
    ``FeatureDistance``."""
    fd = FeatureDistance(**kw).add(fake, real)
    mean, std = fd.kid()
    return OrderedDict([('kid', mean), ('kid_std', std), ('frechet', fd.frechet()), ('n_features', fd.n_features)])


FEATURE_KEYS = ('kid', 'kid_std', 'frechet', 'n_features')
PRDC_KEYS = ('precision', 'recall', 'density', 'coverage', 'nearest_k')
SWD_KEYS = ('swd', 'swd_levels', 'swd_descriptors')
BOUNDARY_KEYS = ('boundary_f1', 'per_class_boundary_f1', 'boundary_assd', 'mask_boundary_f1', 'mask_hausdorff')
BAND_KEYS = ('band_mean_iou',)
SUMMARY_KEYS = ('n_images', 'ssim', 'psnr', 'l1', 'n_layouts', 'pixel_acc', 'mean_acc', 'mean_iou', 'fw_iou',
                'per_class_iou', 'per_class_acc', 'n_absent', 'skipped_pixels', 'n_object_masks', 'mask_iou')


class Evaluator(object):
    """Accumulates the three groups of measures on the device: ``add_image`` (SSIM / PSNR / L1 per image, as the bytes
    ``tensor2im`` saves), ``add_layout`` (one pooled ``label_nc`` x ``label_nc`` confusion matrix), ``add_object_mask``
    (IoU per sample).  It takes what ``Pix2PixHDModel_condImg.inference``, ``TwoStreamAE_mask.evaluate`` / ``generate`` /
    ``reconstruct`` and ``JointInference.gen_layout`` / ``gen_image`` return (a tensor, their dict, or their tuple, whose
    last entry is the generated tensor).  Nothing crosses to the host before ``summary()``."""

    def __init__(self, label_nc, data_range=255., as_bytes=True, boundary_tolerance=None, band_radius=None, swd=None,
                 features=None, panoptic=None):
        self.label_nc, self.data_range, self.as_bytes = int(label_nc), float(data_range), bool(as_bytes)
        self._image, self._conf, self._mask, self._layouts = [], None, [], 0
        # opt-in contour measures: the tolerance of the boundary F-score in pixels, the radius of the trimap band
        self.boundary_tolerance = None if boundary_tolerance is None else float(boundary_tolerance)
        self.band_radius = None if band_radius is None else float(band_radius)
        self._bcounts, self._bsumd, self._mask_boundary, self._band = None, None, [], None
        # opt-in set-level measure: True, or a dict of n_patches, n_dirs, levels, seed, same_positions
        self._swd = None if swd is None or swd is False else SlicedWasserstein(**({} if swd is True else dict(swd)))
        # opt-in feature-space measures: True, or a dict of layers, n_subsets, subset_size, seed, vgg, nearest_k (the last
        # adds PRDC_KEYS to the summary)
        self._features = None if features is None or features is False else \
            FeatureDistance(**({} if features is True else dict(features)))
        # opt-in panoptic quality: True, or a dict of things, connectivity, min_area, ignore_label, max_segments
        self._pq_opt, self._pq, self._pq_tot = None, None, None
        if panoptic is not None and panoptic is not False:
            opt = dict(things=ops.CITYSCAPES_THINGS, connectivity=8, min_area=1, ignore_label=None, max_segments=1024)
            given = {} if panoptic is True else dict(panoptic)
            unknown = sorted(set(given) - set(opt))
            if unknown:
                raise ValueError('Evaluator: panoptic options %s (known: %s)' % (unknown, sorted(opt)))
            opt.update(given)
            opt['things'] = tuple(int(c) for c in opt['things'])
            self._pq_opt = opt

    def add_image(self, fake, real, box=None):
        fake = _labels(fake, ('fake_image',))
        sums, _ = image_sums(fake, real, self.data_range, self.as_bytes, box)
        self._image.append(sums.sum(1))                               # (B, 5): channels pooled
        if self._swd is not None:
            self._swd.add(fake, real)                                 # whole images, as the tensors stand
        if self._features is not None:
            self._features.add(fake, real)
        return self

    def add_layout(self, pred, gt, mask=None, gt_inst=None):
        if self._conf is None:
            pred_t = _plane(_labels(pred, ('comb_pred_label', 'comb_recon_label')))
            with torch.cuda.device(pred_t.device):
                self._conf = (torch.zeros((1, self.label_nc, self.label_nc), dtype=torch.int64, device=pred_t.device),
                              torch.zeros(2, dtype=torch.int32, device=pred_t.device))
        confusion_matrix(pred, gt, self.label_nc, mask=mask, out=self._conf)
        self._layouts += 1
        if self.boundary_tolerance is not None:
            bs = boundary_scores(pred, gt, self.label_nc, self.boundary_tolerance)
            counts, sumd = bs['counts'].sum(0), bs['sumd'].sum(0)        # (n, 2, 4), (n, 2): samples pooled
            self._bcounts = counts if self._bcounts is None else self._bcounts + counts
            self._bsumd = sumd if self._bsumd is None else self._bsumd + sumd
        if self.band_radius is not None:
            band = boundary_band(gt, self.band_radius)
            if mask is not None:
                band = band * (mask.to(band.device).float().reshape(band.shape) != 0).float()
            if self._band is None:
                with torch.cuda.device(band.device):
                    self._band = (torch.zeros((1, self.label_nc, self.label_nc), dtype=torch.int64, device=band.device),
                                  torch.zeros(2, dtype=torch.int32, device=band.device))
            confusion_matrix(pred, gt, self.label_nc, mask=band, out=self._band)
        if self._pq_opt is not None:
            self._add_panoptic(pred, gt, mask, gt_inst)
        return self

    def _add_panoptic(self, pred, gt, mask, gt_inst):
        p = _id_planes(pred, ('comb_pred_label', 'comb_recon_label'))
        dev, n = p.device, self.label_nc
        with torch.cuda.device(dev):
            if self._pq is None:
                self._pq = (torch.zeros((n, 3), dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev))
                self._pq_tot = torch.zeros(3, dtype=torch.int64, device=dev)        # segments gt, pred, flag bits
            status = torch.zeros((p.shape[0], 4), dtype=torch.int32, device=dev)   # per call: batches may differ in size
        panoptic_quality(p, gt, n, gt_inst=gt_inst, mask=mask, out=self._pq + (status,), **self._pq_opt)
        self._pq_tot[:2] += status[:, :2].sum(0)
        bits = torch.arange(5, device=dev)
        self._pq_tot[2] |= ((((status[:, 2:3].long() >> bits) & 1).amax(0)) << bits).sum()

    def add_object_mask(self, prob, gt):
        self._mask.append(mask_iou(prob, gt))
        if self.boundary_tolerance is not None:
            bs = mask_boundary_scores(prob, gt, self.boundary_tolerance)
            self._mask_boundary.append(torch.stack([bs['f1'], bs['hausdorff']], 1))
        return self

    def summary(self):
        """The measures so far as plain python values (the one host synchronisation)."""
        nan = float('nan')
        out = OrderedDict((k, nan) for k in SUMMARY_KEYS)
        out.update(n_images=0, n_layouts=0, n_object_masks=0, n_absent=0, skipped_pixels=0, per_class_iou=[],
                   per_class_acc=[])
        if self._image:
            s = torch.cat(self._image, 0).cpu().numpy()
            with np.errstate(divide='ignore', invalid='ignore'):
                per_ssim, mse, mae = s[:, 0] / s[:, 1], s[:, 2] / s[:, 4], s[:, 3] / s[:, 4]
                per_psnr = 10.0 * np.log10(self.data_range ** 2 / mse)
            out.update(n_images=int(len(s)), ssim=_nanmean(per_ssim), psnr=_nanmean(per_psnr), l1=_nanmean(mae))
        if self._conf is not None:
            sc = segmentation_scores(self._conf[0])
            status = self._conf[1].cpu().numpy()
            sc['per_class_iou'] = [None if math.isnan(v) else float(v) for v in sc['per_class_iou']]
            sc['per_class_acc'] = [None if math.isnan(v) else float(v) for v in sc['per_class_acc']]
            out.update(sc)
            out.update(n_layouts=int(self._layouts), skipped_pixels=int(status[0]))
        if self._mask:
            m = torch.cat(self._mask, 0).cpu().numpy()
            out.update(n_object_masks=int(len(m)), mask_iou=_nanmean(m))
        if self.boundary_tolerance is not None:
            out.update((k, nan) for k in BOUNDARY_KEYS)
            out['per_class_boundary_f1'] = []
            if self._bcounts is not None:
                out.update(_pooled_boundary(self._bcounts.cpu().numpy(), self._bsumd.cpu().numpy()))
            if self._mask_boundary:
                m = torch.cat(self._mask_boundary, 0).cpu().numpy()
                out.update(mask_boundary_f1=_nanmean(m[:, 0]), mask_hausdorff=_nanmean(m[:, 1]))
        if self.band_radius is not None:
            out['band_mean_iou'] = segmentation_scores(self._band[0])['mean_iou'] if self._band is not None else nan
        if self._swd is not None:
            out.update(swd=nan, swd_levels=[], swd_descriptors=int(self._swd.n_descriptors))
            if self._swd.n_descriptors:
                lv = self._swd.distances().cpu().numpy() * 1e3           # as the paper reports them
                out.update(swd=float(lv.mean()), swd_levels=[float(v) for v in lv])
        if self._features is not None:
            n = self._features.n_features
            out.update(kid=nan, kid_std=nan, frechet=nan, n_features=int(n[0]))         # rows per set
            if min(n) >= 2:
                mean, std = self._features.kid()
                out.update(kid=float(mean.item()), kid_std=float(std.item()), frechet=self._features.frechet())
            if self._features.nearest_k is not None:
                out.update((key, float(v.item())) for key, v in self._features.prdc().items())
                out['nearest_k'] = int(self._features.nearest_k)
        if self._pq_opt is not None:
            out.update((k, nan) for k in PANOPTIC_KEYS)
            out.update(per_class_pq=[], n_segments_gt=0, n_segments_pred=0, panoptic_flags=0)
            if self._pq is not None:
                sc = panoptic_scores(self._pq[0], self._pq[1], self._pq_opt['things'])
                tot = self._pq_tot.cpu().numpy()
                out.update((k, sc[k]) for k in ('pq', 'sq', 'rq', 'pq_things', 'pq_stuff'))
                out.update(per_class_pq=[None if math.isnan(v) else float(v) for v in sc['per_class_pq']],
                           n_segments_gt=int(tot[0]), n_segments_pred=int(tot[1]), panoptic_flags=int(tot[2]))
        return out

    def write_json(self, path):
        with open(path, 'w') as f:
            json.dump({k: (None if isinstance(v, float) and not math.isfinite(v) else v)
                       for k, v in self.summary().items()}, f, indent=1)
        return path


def _pooled_boundary(counts, sumd):
    """boundary_f1 (the mean over the classes with a boundary in either map), per_class_boundary_f1 (None: no boundary)
    and boundary_assd (the mean over the classes of sum of distances / reachable boundary pixels) from counts (n, 2, 4)
    and sums (n, 2) pooled over every sample."""
    n_p, n_g = counts[:, 0, 0].astype(np.float64), counts[:, 1, 0].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        prec = np.where(n_p > 0, counts[:, 0, 1] / n_p, 0.0)
        rec = np.where(n_g > 0, counts[:, 1, 1] / n_g, 0.0)
        f1 = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
        reach = (counts[:, :, 0] - counts[:, :, 3]).sum(1).astype(np.float64)
        assd = np.where(reach > 0, sumd.sum(1) / reach, np.nan)
    seen = (n_p + n_g) > 0
    return dict(boundary_f1=float(f1[seen].mean()) if seen.any() else float('nan'),
                per_class_boundary_f1=[float(v) if k else None for v, k in zip(f1, seen)],
                boundary_assd=_nanmean(assd))


def _nanmean(v):
    v = np.asarray(v, np.float64)
    keep = ~np.isnan(v)
    return float(v[keep].mean()) if keep.any() else float('nan')


def evaluate_mask2image(model, dataset, how_many, evaluator=None):
    """The loop of the reference's vis_mask2image.py (``model.inference`` per sample of ``dataset``, batch 1, the first
    ``how_many`` samples) feeding an ``Evaluator`` (passed through as it is: one built with ``swd=...`` also collects the
    set-level sliced Wasserstein distance): generated against real image inside the edited box.  The box is the
    loader's ``input_bbox`` when the sample carries one, else the extent of ``mask_in``.  Returns the evaluator."""
    ev = evaluator if evaluator is not None else Evaluator(getattr(model.opt, 'label_nc', 35))
    for i, data in enumerate(dataset):
        if i >= how_many:
            break
        fake = model.inference(label=data['label'], inst=data['inst'], image=data['image'], mask_in=data['mask_in'],
                               mask_out=data['mask_out'])
        if 'input_bbox' in data:      # the loader's (wmin, hmin, wmax, hmax), the far edges exclusive
            box = torch.as_tensor(data['input_bbox']).reshape(-1, 4).to(fake.device, torch.int32).clone()
            box[:, 2:] -= 1
        else:
            box = box_of_mask(data['mask_in'].to(fake.device))
        ev.add_image(fake, data['image'], box=box)
    return ev
