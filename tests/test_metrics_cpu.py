"""not gpu: the host side of the evaluation metrics -- the C ABI's declarations, the argument checks the library makes
before it launches anything, the float64 fixture the GPU tests measure against (tests/metrics_fixture.py) checked against
closed forms, ``segmentation_scores`` on a hand-written matrix and the keys of the ``Evaluator``'s JSON."""
import json
import math
import os
import re

import numpy as np
import pytest

import metrics_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('him_image_metrics', 'him_image_metrics_workspace', 'him_confusion', 'him_confusion_workspace')


def test_header_declares_and_cabi_lists_the_entry_points():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        header = f.read()
    assert re.search(r'^int him_image_metrics\(', header, flags=re.M)
    assert re.search(r'^size_t him_image_metrics_workspace\(int B, int C, int H, int W\);', header, flags=re.M)
    assert re.search(r'^int him_confusion\(', header, flags=re.M)
    assert re.search(r'^size_t him_confusion_workspace\(int n\);', header, flags=re.M)
    for name in NAMES:
        assert name in _cabi.EXPORTS
        assert getattr(_cabi.lib._load(), name) is not None
    m = re.search(r'tile of (\d+) x (\d+) window origins', header)
    assert m and (int(m.group(1)), int(m.group(2))) == (16, 64)          # the GPU tests' shapes are worded in the tile


def test_image_metrics_argument_checks_return_an_error_before_any_launch():
    """Nothing below reaches a launch: the pointers are never dereferenced on the host, and every call is refused."""
    from neurips18_hierchical_image_manipulation_amd import _cabi
    dll = _cabi.lib._load()
    ws_fn, fn = dll.him_image_metrics_workspace, dll.him_image_metrics
    need = int(ws_fn(2, 3, 1024, 2048))
    assert need >= 2 * 3 * (1024 // 16) * (2048 // 64) * 3 * 8
    assert int(ws_fn(0, 3, 8, 8)) == 0 and int(ws_fn(1, 2, 8, 8)) == 0 and int(ws_fn(1, 3, 0, 8)) == 0
    p = 1 << 20                                             # an aligned non-null address, never read
    good = dict(a=p, b=p, B=2, C=3, H=1024, W=2048, scale=127.5, offset=127.5, quantize=1, data_range=255.0, box=0,
                sums=p, map_out=0, ws=p, ws_bytes=need, stream=0)
    order = list(good)
    assert fn(*[dict(good, B=0)[k] for k in order]) != 0
    bad = [('H', 0), ('W', -3), ('B', 0), ('C', 2), ('C', 0), ('C', 4), ('a', 0), ('b', 0), ('sums', 0), ('ws', 0),
           ('ws_bytes', need - 1), ('ws_bytes', 0), ('data_range', 0.0), ('ws', p + 4)]
    for name, value in bad:
        rc = fn(*[dict(good, **{name: value})[k] for k in order])
        assert rc != 0, (name, value, rc)
        assert b'image_metrics' in dll.him_last_error(), (name, dll.him_last_error())
    assert fn(*[dict(good, B=1, C=1, H=65535 * 16 + 1, W=1, ws_bytes=1 << 30)[k] for k in order]) != 0      # grid rows
    assert fn(*[dict(good, B=21846, C=3, H=1, W=1, ws_bytes=1 << 30)[k] for k in order]) != 0             # planes
    rc = fn(*[dict(good, box=p, map_out=p)[k] for k in order])               # the map is for whole-image calls
    assert rc != 0 and b'map_out' in dll.him_last_error()
    with pytest.raises(_cabi.HimError, match='image_metrics'):
        _cabi.lib.him_image_metrics(*[dict(good, ws_bytes=need - 1)[k] for k in order])


def test_confusion_argument_checks_return_an_error_before_any_launch():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    dll = _cabi.lib._load()
    ws_fn, fn = dll.him_confusion_workspace, dll.him_confusion
    need = int(ws_fn(35))
    assert need >= 8 and int(ws_fn(0)) == 0 and int(ws_fn(257)) == 0 and int(ws_fn(256)) > 0
    p = 1 << 20
    good = dict(pred=p, pred_kind=2, gt=p, gt_kind=3, mask=0, B=2, C=1, H=64, W=257, n=35, ignore=-1, per_sample=0,
                accumulate=0, counts=p, status=p, ws=p, ws_bytes=need, stream=0)
    order = list(good)
    bad = [('H', 0), ('W', 0), ('B', 0), ('n', 0), ('n', 257), ('n', -1), ('pred', 0), ('gt', 0), ('counts', 0),
           ('status', 0), ('ws', 0), ('pred_kind', 6), ('pred_kind', -1), ('gt_kind', 4), ('gt_kind', -1), ('C', 3),
           ('ignore', -2), ('ws_bytes', need - 1), ('ws_bytes', 0), ('counts', p + 4)]
    for name, value in bad:
        rc = fn(*[dict(good, **{name: value})[k] for k in order])
        assert rc != 0, (name, value, rc)
        assert b'confusion' in dll.him_last_error(), (name, dll.him_last_error())
    assert fn(*[dict(good, pred_kind=4, C=0)[k] for k in order]) != 0
    with pytest.raises(_cabi.HimError, match='confusion'):
        _cabi.lib.him_confusion(*[dict(good, ws_bytes=need - 1)[k] for k in order])


def test_bindings_refuse_host_tensors():
    import torch
    from neurips18_hierchical_image_manipulation_amd import ops
    with pytest.raises(ValueError, match='device tensor'):
        ops.image_metrics(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16), scale=1.0, offset=0.0, quantize=False,
                          data_range=1.0)
    with pytest.raises(ValueError, match='device tensor'):
        ops.confusion(torch.zeros(1, 1, 4, 4, dtype=torch.int64), torch.zeros(1, 1, 4, 4, dtype=torch.int64), 3)


# ------------------------------------------------------------------------------------------------- the fixture itself
def _noise(seed, *shape):
    return np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(255)


def test_fixture_window_is_the_stated_gaussian():
    g = fx.gauss()
    assert g.dtype == np.float32 and g.shape == (11,) and abs(float(g.astype(np.float64).sum()) - 1) < 1e-7
    assert np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(float(g[4]) / float(g[5]) - math.exp(-1 / 4.5)) < 1e-6


def test_fixture_ssim_of_an_image_with_itself_is_one_and_ssim_is_symmetric():
    a, b = _noise(1, 23, 31), _noise(2, 23, 31)
    m = fx.ssim_map(a, a, 255.0)
    assert m.shape == (13, 21) and np.abs(m - 1).max() < 1e-12
    assert np.array_equal(fx.ssim_map(a, b, 255.0), fx.ssim_map(b, a, 255.0))
    assert fx.ssim_map(a, b, 255.0).max() < 0.5


def test_fixture_single_window_equals_the_closed_formula():
    a, b = _noise(3, 11, 11).astype(np.float64), _noise(4, 11, 11).astype(np.float64)
    g = fx.gauss().astype(np.float64)
    w = np.outer(g, g)
    mu_a, mu_b = (w * a).sum(), (w * b).sum()
    va, vb = (w * a * a).sum() - mu_a ** 2, (w * b * b).sum() - mu_b ** 2
    cab = (w * a * b).sum() - mu_a * mu_b
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    want = (2 * mu_a * mu_b + c1) * (2 * cab + c2) / ((mu_a ** 2 + mu_b ** 2 + c1) * (va + vb + c2))
    got = fx.ssim_map(a, b, 255.0)
    assert got.shape == (1, 1) and abs(got[0, 0] - want) < 1e-13
    sums, maps = fx.image_sums(a[None, None], b[None, None], 1.0, 0.0, False, 255.0)
    d = a.astype(np.float32).astype(np.float64) - b.astype(np.float32).astype(np.float64)
    assert np.allclose(sums[0, 0], [want, 1, (d * d).sum(), np.abs(d).sum(), 121], rtol=1e-12, atol=0)


def test_fixture_scaling_both_images_and_the_range_leaves_ssim_unchanged():
    a, b = _noise(5, 14, 19).astype(np.float64), _noise(6, 14, 19).astype(np.float64)
    m = fx.ssim_map(a, b, 255.0)
    assert np.abs(fx.ssim_map(a / 255.0, b / 255.0, 1.0) - m).max() < 1e-12
    assert np.abs(fx.ssim_map(a * 4.0, b * 4.0, 1020.0) - m).max() < 1e-12


def test_fixture_boxes_mapping_and_confusion():
    a, b = _noise(7, 1, 1, 20, 30) / 127.5 - 1, _noise(8, 1, 1, 20, 30) / 127.5 - 1
    q = fx.map_values(a, 127.5, 127.5, True)
    assert q.min() >= 0 and q.max() <= 255 and np.array_equal(q, np.trunc(q))
    box = np.array([[3, 2, 40, 15]])
    s, m = fx.image_sums(a, b, 127.5, 127.5, True, 255.0, box)
    s2, m2 = fx.image_sums(a[:, :, 2:16, 3:30], b[:, :, 2:16, 3:30], 127.5, 127.5, True, 255.0)
    assert np.array_equal(s, s2) and s[0, 0, 4] == 14 * 27 and s[0, 0, 1] == 4 * 17
    thin, _ = fx.image_sums(a, b, 127.5, 127.5, True, 255.0, np.array([[0, 0, 9, 19]]))
    assert thin[0, 0, 1] == 0 and thin[0, 0, 0] == 0 and thin[0, 0, 4] == 200 and thin[0, 0, 2] > 0
    none, _ = fx.image_sums(a, b, 127.5, 127.5, True, 255.0, np.array([[5, 5, 4, 9]]))
    assert not none.any()
    pred = np.array([[[0, 1, 2, 7], [1, 1, -1, 2]]], np.int64)
    gt = np.array([[[0, 1, 1, 2], [2, 1, 0, 1.5]]], np.float32)
    c, skipped = fx.confusion(pred, 2, gt, 3, 3)
    assert skipped == 3 and c.sum() == 5 and c[0, 0, 0] == 1 and c[0, 1, 1] == 2 and c[0, 1, 2] == 1 and c[0, 2, 1] == 1


# --------------------------------------------------------------------------------------------- the public host pieces
def test_segmentation_scores_on_a_hand_written_matrix_with_one_absent_class():
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    conf = np.array([[6, 0, 2], [0, 0, 0], [1, 0, 3]], np.int64)          # class 1: neither ground truth nor prediction
    s = metrics.segmentation_scores(conf)
    assert s['n_absent'] == 1
    assert s['pixel_acc'] == pytest.approx(9 / 12, abs=1e-15)
    assert s['per_class_acc'][0] == pytest.approx(6 / 8) and s['per_class_acc'][2] == pytest.approx(3 / 4)
    assert s['per_class_iou'][0] == pytest.approx(6 / 9) and s['per_class_iou'][2] == pytest.approx(3 / 6)
    assert math.isnan(s['per_class_iou'][1]) and math.isnan(s['per_class_acc'][1])
    assert s['mean_acc'] == pytest.approx((6 / 8 + 3 / 4) / 2, abs=1e-15)
    assert s['mean_iou'] == pytest.approx((6 / 9 + 3 / 6) / 2, abs=1e-15)
    assert s['fw_iou'] == pytest.approx((8 * 6 / 9 + 4 * 3 / 6) / 12, abs=1e-15)
    ref = fx.scores(conf)
    for k in ('pixel_acc', 'mean_acc', 'mean_iou', 'fw_iou'):
        assert s[k] == pytest.approx(ref[k], abs=1e-15)
    assert s['n_absent'] == ref['absent']
    # a class that is predicted but never true counts in the IoU mean (IoU 0) and not in the accuracy mean
    s = metrics.segmentation_scores(np.array([[[2, 1], [0, 0]]]))
    assert s['n_absent'] == 0 and s['mean_iou'] == pytest.approx((2 / 3 + 0) / 2) and s['mean_acc'] == pytest.approx(2 / 3)
    empty = metrics.segmentation_scores(np.zeros((2, 2), np.int64))
    assert math.isnan(empty['pixel_acc']) and empty['n_absent'] == 2


def test_evaluator_json_keys(tmp_path):
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    ev = metrics.Evaluator(35)
    s = ev.summary()
    assert tuple(s) == metrics.SUMMARY_KEYS
    assert s['n_images'] == 0 and s['n_layouts'] == 0 and s['n_object_masks'] == 0 and math.isnan(s['ssim'])
    path = ev.write_json(str(tmp_path / 'm.json'))
    with open(path) as f:
        got = json.load(f)
    assert sorted(got) == sorted(['n_images', 'ssim', 'psnr', 'l1', 'n_layouts', 'pixel_acc', 'mean_acc', 'mean_iou',
                                  'fw_iou', 'per_class_iou', 'per_class_acc', 'n_absent', 'skipped_pixels',
                                  'n_object_masks', 'mask_iou'])
    assert got['ssim'] is None and got['n_images'] == 0
