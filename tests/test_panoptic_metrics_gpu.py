"""-m gpu: the Python surface of panoptic matching -- ``metrics.panoptic_quality`` (device labelling + matching) against
the fixture run on ``ccl_fixture.label_reference``'s planes, the stuff-only cross-check against the confusion matrix, and
``Evaluator(panoptic=...)``."""
import numpy as np
import pytest
import torch

import ccl_fixture as cf
import panoptic_fixture as fx

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
PARENT_SUMMARY_KEYS = {'n_images', 'ssim', 'psnr', 'l1', 'n_layouts', 'pixel_acc', 'mean_acc', 'mean_iou', 'fw_iou',
                       'per_class_iou', 'per_class_acc', 'n_absent', 'skipped_pixels', 'n_object_masks', 'mask_iou'}
CACHE = {}


def layouts():
    """The perturbed layouts and the fixture's answer on them, computed once."""
    if not CACHE:
        planes = fx.perturbed_layouts()
        CACHE['planes'] = planes
        CACHE['ref'] = fx.match_reference(*planes, 35)
    return CACHE['planes'], CACHE['ref']


def dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda', dtype)


def assert_counts(counts, iou, ref):
    counts, iou = counts.cpu().numpy(), iou.cpu().numpy()
    assert np.array_equal(counts, ref[0]), (counts.tolist(), ref[0].tolist())
    for c in range(len(iou)):
        print('class %d tp %d iou_sum %.17g reference %.17g' % (c, ref[0][c, 0], iou[c], ref[1][c]))
        assert abs(iou[c] - ref[1][c]) <= max(int(ref[0][c, 0]), 1) * EPS * abs(ref[1][c])


def test_panoptic_quality_with_given_and_derived_instances():
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    (pred_seg, pred_cls, gt_seg, gt_cls), ref = layouts()
    for gt_inst in (dev(gt_seg, torch.int32), None):
        counts, iou, status = metrics.panoptic_quality(dev(pred_cls, torch.uint8), dev(gt_cls), 35, cf.CITY_THINGS,
                                                       gt_inst=gt_inst)
        assert_counts(counts, iou, ref)
        assert np.array_equal(status.cpu().numpy(), ref[2])
    # scores (B, C, H, W) go through the arg-max; a mask and an ignored class reach the kernel
    scores = torch.nn.functional.one_hot(dev(pred_cls), 35).permute(0, 3, 1, 2).float().contiguous()
    mask = (np.random.RandomState(2).rand(3, 97, 193) > 0.1).astype(np.float32)
    counts, iou, status = metrics.panoptic_quality(scores, dev(gt_cls, torch.float32), 35, cf.CITY_THINGS,
                                                   gt_inst=dev(gt_seg), ignore_label=7, mask=dev(mask, torch.float32)[:, None])
    ref = fx.match_reference(pred_seg, pred_cls, gt_seg, gt_cls, 35, mask=mask, ignore=7)
    assert_counts(counts, iou, ref)
    assert np.array_equal(status.cpu().numpy(), ref[2])


def test_stuff_only_pq_is_the_class_iou_above_one_half():
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    pred, gt = fx.stuff_layouts()
    n = 8
    counts, iou, status = metrics.panoptic_quality(dev(pred), dev(gt), n, ())
    assert status.cpu().numpy()[0, 2] == 0
    pq = metrics.panoptic_scores(counts, iou)['per_class_pq']
    class_iou = metrics.segmentation_scores(metrics.confusion_matrix(dev(pred), dev(gt), n)[0])['per_class_iou']
    assert (class_iou[~np.isnan(class_iou)] > 0.5).any() and (class_iou[~np.isnan(class_iou)] <= 0.5).any()
    for c in range(n):
        if np.isnan(class_iou[c]):
            assert np.isnan(pq[c])
        else:
            assert pq[c] == (class_iou[c] if class_iou[c] > 0.5 else 0.0), (c, pq[c], class_iou[c])


def test_evaluator_pools_two_batches():
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    (pred_seg, pred_cls, gt_seg, gt_cls), ref = layouts()
    ev = metrics.Evaluator(35, panoptic=dict(things=cf.CITY_THINGS))
    ev.add_layout(dev(pred_cls[:2]), dev(gt_cls[:2]))
    ev.add_layout(dev(pred_cls[2:]), dev(gt_cls[2:]), gt_inst=dev(gt_seg[2:], torch.int32))
    s = ev.summary()
    pq, sq, rq, per_class = fx.scores_reference(ref[0], ref[1])
    assert s['pq'] == pytest.approx(pq, rel=1e-12) and s['rq'] == pytest.approx(rq, rel=1e-12)
    assert 0.0 < s['pq'] < s['sq'] <= 1.0 and 0.0 < s['pq_things'] < 1.0 and 0.0 < s['pq_stuff'] <= 1.0
    assert s['n_segments_gt'] == int(ref[2][:, 0].sum()) and s['n_segments_pred'] == int(ref[2][:, 1].sum())
    assert s['panoptic_flags'] == 0 and s['n_layouts'] == 2
    for got, want in zip(s['per_class_pq'], per_class):
        assert (got is None and np.isnan(want)) or got == pytest.approx(want, rel=1e-12)


def test_panoptic_flags_report_an_overflowed_labelling():
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    board = dev(cf.checkerboard()[None])                                   # 2145 four-connected objects, more than 1024
    ev = metrics.Evaluator(35, panoptic=dict(things=(24, 25), connectivity=4))
    s = ev.add_layout(board, board).summary()
    assert s['panoptic_flags'] & ops.PQ_CCL
    ok = metrics.Evaluator(35, panoptic=dict(things=(24, 25), connectivity=8)).add_layout(board, board).summary()
    assert ok['panoptic_flags'] == 0 and ok['pq'] == 1.0 and ok['n_segments_gt'] == 2


def test_evaluator_without_the_option_keeps_its_keys():
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    _, pred_cls, _, gt_cls = layouts()[0]
    s = metrics.Evaluator(35).add_layout(dev(pred_cls), dev(gt_cls)).summary()
    assert set(s) == PARENT_SUMMARY_KEYS
    with_option = metrics.Evaluator(35, panoptic=True).add_layout(dev(pred_cls), dev(gt_cls)).summary()
    assert set(with_option) == PARENT_SUMMARY_KEYS | set(metrics.PANOPTIC_KEYS)
    assert all(with_option[k] == s[k] or (s[k] != s[k]) for k in PARENT_SUMMARY_KEYS)
