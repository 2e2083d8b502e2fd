"""not gpu: the host side of the distance transform and the boundary metrics -- the C ABI's declarations and exports, the
argument checks the library makes before it launches anything, the brute-force fixture of tests/edt_fixture.py against
scipy (where installed) and on planes whose answer is written out here, and planted defects showing that the comparison
helpers of the GPU tests can fail."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import edt_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_WORKSPACE = -1, -2


def test_header_declares_and_library_exports_the_entry_points():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        header = f.read()
    for decl in (r'^int him_edt\(', r'^size_t him_edt_workspace\(', r'^int him_boundary_stats\(',
                 r'^size_t him_boundary_stats_workspace\(', r'^int him_label_ids\(', r'^#define HIM_EDT_NONZERO 0$',
                 r'^#define HIM_EDT_EQUALS 1$', r'^#define HIM_EDT_BOUNDARY_OF 2$', r'^#define HIM_EDT_ANY_BOUNDARY 3$',
                 r'^#define HIM_EDT_NONE 2147483647$', r'^#define HIM_EDT_BAD_JOB 1$'):
        assert re.search(decl, header, flags=re.M), decl
    assert os.path.isfile(_cabi.LIB_PATH), 'libhim_hip.so not built'
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in ('him_edt', 'him_edt_workspace', 'him_boundary_stats', 'him_boundary_stats_workspace', 'him_label_ids'):
        assert name in _cabi.EXPORTS and hasattr(dll, name), name
    from neurips18_hierchical_image_manipulation_amd import ops
    assert ops.EDT_RULES == {'nonzero': fx.NONZERO, 'equals': fx.EQUALS, 'boundary_of': fx.BOUNDARY_OF,
                             'any_boundary': fx.ANY_BOUNDARY}
    assert ops.EDT_NONE == fx.NONE and ops.EDT_BAD_JOB == fx.BAD_JOB


def test_argument_checks_return_before_any_launch():
    """Nothing below reaches a launch: the pointers are never dereferenced on the host, and every call is refused."""
    from neurips18_hierchical_image_manipulation_amd import _cabi
    dll = _cabi.lib._load()
    ws_fn, fn = dll.him_edt_workspace, dll.him_edt
    need = int(ws_fn(280, 256, 512))
    assert need >= 280 * 256 * 512 * 2 and need % 16 == 0
    assert int(ws_fn(1, 1, 1)) >= 2 and int(ws_fn(4096, 16384, 16384)) == 4096 * 16384 * 16384 * 2
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 16385, 8), (1, 8, 16385), (4097, 16384, 16384)):
        assert int(ws_fn(*shape)) == 0 and int(dll.him_boundary_stats_workspace(*shape)) == 0, shape
    p = 1 << 20                                             # an aligned non-null address, never read
    order = ['src', 'kind', 'B', 'H', 'W', 'jobs', 'K', 'dist2', 'nearest', 'status', 'ws', 'ws_bytes', 'stream']
    good = dict(src=p, kind=0, B=8, H=256, W=512, jobs=p, K=280, dist2=p, nearest=p, status=p, ws=p, ws_bytes=need,
                stream=0)
    bad = [('src', 0), ('jobs', 0), ('dist2', 0), ('status', 0), ('ws', 0), ('kind', 4), ('kind', -1), ('B', 0), ('H', 0),
           ('W', 0), ('H', -2), ('H', 16385), ('W', 16385), ('K', 0), ('K', -1), ('dist2', p + 2), ('nearest', p + 1),
           ('ws', p + 1)]
    for name, value in bad:
        args = dict(good, **{name: value})
        rc = fn(*[args[k] for k in order])
        assert rc == E_INVALID, (name, value, rc)
        assert b'edt' in dll.him_last_error(), (name, dll.him_last_error())
    assert fn(*[dict(good, K=4097, H=16384, W=16384, ws_bytes=1 << 62)[k] for k in order]) == E_INVALID     # K H W > 2^40
    assert fn(*[dict(good, kind=1, src=p + 2)[k] for k in order]) == E_INVALID
    for short in (need - 1, 0):
        assert fn(*[dict(good, ws_bytes=short)[k] for k in order]) == E_WORKSPACE
        assert b'edt' in dll.him_last_error()
    with pytest.raises(_cabi.HimError, match='edt'):
        _cabi.lib.him_edt(*[dict(good, kind=7)[k] for k in order])

    sfn = dll.him_boundary_stats
    sneed = int(dll.him_boundary_stats_workspace(280, 256, 512))
    assert sneed >= 280 * 40 and sneed % 8 == 0
    order = ['src', 'kind', 'B', 'H', 'W', 'jobs', 'K', 'dist2', 'tol2', 'counts', 'sumd', 'ws', 'ws_bytes', 'stream']
    good = dict(src=p, kind=2, B=8, H=256, W=512, jobs=p, K=280, dist2=p, tol2=4, counts=p, sumd=p, ws=p, ws_bytes=sneed,
                stream=0)
    bad = [('src', 0), ('jobs', 0), ('dist2', 0), ('counts', 0), ('sumd', 0), ('ws', 0), ('kind', 4), ('B', 0), ('H', 0),
           ('W', 16385), ('K', 0), ('tol2', -1), ('counts', p + 4), ('sumd', p + 4), ('ws', p + 4), ('src', p + 4)]
    for name, value in bad:
        rc = sfn(*[dict(good, **{name: value})[k] for k in order])
        assert rc == E_INVALID, (name, value, rc)
        assert b'boundary_stats' in dll.him_last_error()
    assert sfn(*[dict(good, ws_bytes=sneed - 1)[k] for k in order]) == E_WORKSPACE

    lfn = dll.him_label_ids
    order = ['src', 'pred_kind', 'B', 'C', 'H', 'W', 'ids', 'stream']
    good = dict(src=p, pred_kind=4, B=2, C=5, H=8, W=8, ids=p, stream=0)
    for name, value in (('src', 0), ('ids', 0), ('pred_kind', 3), ('pred_kind', 6), ('B', 0), ('H', 0), ('W', 0), ('C', 0),
                        ('src', p + 2)):
        assert lfn(*[dict(good, **{name: value})[k] for k in order]) == E_INVALID, (name, value)
    assert lfn(*[dict(good, pred_kind=5, C=2)[k] for k in order]) == E_INVALID


def test_binding_refuses_host_tensors_and_bad_arguments():
    import torch
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    with pytest.raises(ValueError, match='device tensor'):
        ops.distance_transform(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match='device tensor'):
        ops.boundary_stats(torch.zeros(4, 4, dtype=torch.uint8), None, None, 1)
    assert metrics.diag_tolerance(256, 512) == fx.diag_tolerance(256, 512) == 0.0075 * math.sqrt(256 ** 2 + 512 ** 2)
    assert metrics.diag_tolerance(3, 4, frac=0.5) == 2.5
    ev = metrics.Evaluator(35)
    assert list(ev.summary()) == list(metrics.SUMMARY_KEYS)
    ev = metrics.Evaluator(35, boundary_tolerance=2.0, band_radius=3)
    assert list(ev.summary()) == list(metrics.SUMMARY_KEYS + metrics.BOUNDARY_KEYS + metrics.BAND_KEYS)
    assert list(metrics.Evaluator(35, band_radius=3).summary()) == list(metrics.SUMMARY_KEYS + metrics.BAND_KEYS)


def test_fixture_transform_on_hand_drawn_planes():
    seed = np.zeros((3, 5), bool)
    seed[1, 1] = seed[1, 3] = True
    d2, near = fx.edt(seed)
    assert d2.tolist() == [[2, 1, 2, 1, 2], [1, 0, 1, 0, 1], [2, 1, 2, 1, 2]]
    assert near.tolist() == [[6, 6, 6, 8, 8], [6, 6, 6, 8, 8], [6, 6, 6, 8, 8]]           # the left seed wins column 2
    seed = np.zeros((5, 3), bool)
    seed[1, 1] = seed[3, 1] = True
    d2, near = fx.edt(seed)
    assert near[2].tolist() == [4, 4, 4] and d2[2].tolist() == [2, 1, 2]                  # the upper seed wins row 2
    d2, near = fx.edt(np.zeros((2, 3), bool))
    assert (d2 == fx.NONE).all() and (near == -1).all()
    corner = np.zeros((7, 9), bool)
    corner[0, 0] = True
    assert fx.edt(corner)[0][6, 8] == 36 + 64


def test_fixture_seed_rules_on_a_hand_drawn_plane():
    plane = np.array([[1, 1, 1, 0],
                      [1, 1, 1, 0],
                      [1, 1, 2, 2],
                      [1, 1, 2, 2]])
    assert fx.seeds(plane, 0, fx.NONZERO).sum() == 14
    assert fx.seeds(plane, 2, fx.EQUALS).sum() == 4
    # class 1 touches the border on three sides: the border is no boundary, only the pixels facing 0 or 2 are
    assert fx.seeds(plane, 1, fx.BOUNDARY_OF).astype(int).tolist() == [[0, 0, 1, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 1, 0, 0]]
    assert fx.seeds(plane, 2, fx.BOUNDARY_OF).astype(int).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 1], [0, 0, 1, 0]]
    assert fx.seeds(plane, 7, fx.ANY_BOUNDARY).astype(int).tolist() == [[0, 0, 1, 1], [0, 0, 1, 1], [0, 1, 1, 1], [0, 1, 1, 0]]
    # the 8-neighbour stand-in also sees (1, 1) -> (2, 2)
    assert fx.seeds(plane, 1, fx.BOUNDARY_OF, neighbours=8)[1, 1] and not fx.seeds(plane, 1, fx.BOUNDARY_OF)[1, 1]
    assert not fx.seeds(np.ones((3, 3), int), 1, fx.BOUNDARY_OF).any() and not fx.seeds(np.ones((3, 3), int), 1, fx.ANY_BOUNDARY).any()


def _small_cases():
    pred, gt = fx.layout_pair()
    yield 'sparse', fx.blocky(1, 1, 33, 65, (0, 0, 0, 0, 0, 0, 0, 3), cell=2)[0] != 0
    for c in (0, 1, 2):
        yield 'boundary_of_%d' % c, fx.seeds(gt[0], c, fx.BOUNDARY_OF)
    yield 'any_boundary', fx.seeds(pred[1], 0, fx.ANY_BOUNDARY)
    yield 'equals', fx.seeds(pred[2], 1, fx.EQUALS)
    one = np.zeros((31, 63), bool)
    one[30, 0] = True
    yield 'corner', one
    yield 'all', np.ones((5, 9), bool)


def test_fixture_equals_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    n = 0
    for name, seed in _small_cases():
        d2, near = fx.edt(seed)
        want = np.rint(ndimage.distance_transform_edt(~seed) ** 2).astype(np.int64)
        assert np.array_equal(d2, want), name
        ys, xs = np.divmod(near.astype(np.int64), seed.shape[1])
        py, px = np.mgrid[0:seed.shape[0], 0:seed.shape[1]]
        assert seed[ys, xs].all() and np.array_equal((py - ys) ** 2 + (px - xs) ** 2, d2), name
        n += 1
    assert n == 8


def test_planted_defects_are_caught_by_the_comparison_helpers():
    pred, gt = fx.layout_pair()
    jobs = np.array([[0, 1, fx.BOUNDARY_OF], [1, 0, fx.ANY_BOUNDARY], [2, 2, fx.EQUALS], [0, 0, fx.NONZERO]], np.int32)
    want = fx.edt_jobs(gt, jobs)
    fx.assert_edt_equal(fx.edt_jobs(gt, jobs), want)
    # a city-block distance instead of the Euclidean one
    with pytest.raises(AssertionError, match='dist2'):
        fx.assert_edt_equal(fx.edt_jobs(gt, jobs, metric='city'), want)
    # a right-wins tie: the distances are right, only the feature transform tells
    right = fx.edt_jobs(gt, jobs, tie='right')
    assert np.array_equal(right[0], want[0])
    with pytest.raises(AssertionError, match='nearest'):
        fx.assert_edt_equal(right, want)
    # an 8-neighbour boundary rule
    eight = fx.edt_jobs(gt, jobs, neighbours=8)
    assert (eight[2][:, 0] >= want[2][:, 0]).all() and (eight[2][:2, 0] > want[2][:2, 0]).all()
    with pytest.raises(AssertionError):
        fx.assert_edt_equal(eight, want)
    # a < instead of <= tolerance
    cjobs = fx.class_jobs(3, [0, 1, 2])
    d_gt = fx.edt_jobs(gt, cjobs)[0]
    counts, sumd = fx.boundary_stats(pred, cjobs, d_gt, 4)
    fx.assert_stats_equal(counts, sumd, counts, sumd)
    strict, ssum = fx.boundary_stats(pred, cjobs, d_gt, 4, strict=True)
    assert (strict[:, 1] < counts[:, 1]).any()
    with pytest.raises(AssertionError, match='counts'):
        fx.assert_stats_equal(strict, ssum, counts, sumd)
    # a sum that is off by more than the order of the additions explains
    with pytest.raises(AssertionError, match='sumd'):
        fx.assert_stats_equal(counts, sumd * (1 + 1e-9), counts, sumd)
    # the score comparison: the nan pattern and the values
    a = fx.boundary_scores(pred, gt, 5, 2.0)
    fx.assert_scores_equal(a, a)
    b = dict(a, f1=np.where(np.isnan(a['f1']), 0.0, a['f1']))
    with pytest.raises(AssertionError, match='nan pattern'):
        fx.assert_scores_equal(b, a)
    with pytest.raises(AssertionError):
        fx.assert_scores_equal(fx.boundary_scores(pred, gt, 5, 2.0, strict=True), a)


def test_scores_of_two_concentric_squares():
    """Ground truth: a 12 x 12 square; prediction: the concentric 16 x 16 square, two pixels further out on every side.
    Prediction boundary: 60 pixels, the 48 beside the truth's sides at distance 2, per corner three at sqrt(8), sqrt(5),
    sqrt(5); truth boundary: 44 pixels, each 2 from the prediction's."""
    gt = np.zeros((1, 24, 24), np.int64)
    gt[0, 6:18, 6:18] = 1
    pred = np.zeros((1, 24, 24), np.int64)
    pred[0, 4:20, 4:20] = 1
    r = fx.boundary_scores(pred, gt, 2, tolerance=2.0)
    assert r['counts'][0, 1].tolist() == [[60, 48, 8, 0], [44, 44, 4, 0]]
    assert r['precision'][0, 1] == 0.8 and r['recall'][0, 1] == 1.0
    assert r['f1'][0, 1] == pytest.approx(2 * 0.8 / 1.8, rel=1e-15)
    assert r['hausdorff'][0, 1] == math.sqrt(8)
    assert r['assd'][0, 1] == pytest.approx((48 * 2 + 4 * math.sqrt(8) + 8 * math.sqrt(5) + 44 * 2) / 104, rel=1e-15)
    # below the corner distances nothing changes; at sqrt(5) the eight pixels beside the corners match, at sqrt(8) all
    assert fx.boundary_scores(pred, gt, 2, tolerance=2.2)['precision'][0, 1] == 0.8
    assert fx.boundary_scores(pred, gt, 2, tolerance=math.sqrt(5) + 1e-9)['precision'][0, 1] == 56 / 60
    assert fx.boundary_scores(pred, gt, 2, tolerance=3.0)['precision'][0, 1] == 1.0
    assert fx.boundary_scores(pred, gt, 2, tolerance=1.9)['f1'][0, 1] == 0.0
    # a class in one map only: zeros and nan distances; in neither: all nan
    r = fx.boundary_scores(pred, np.zeros_like(gt), 3, 2.0)
    assert [r[k][0, 1] for k in ('precision', 'recall', 'f1')] == [0, 0, 0] and np.isnan(r['assd'][0, 1])
    assert np.isnan(r['hausdorff'][0, 1]) and r['counts'][0, 1].tolist() == [[60, 0, -1, 60], [0, 0, -1, 0]]
    assert all(np.isnan(r[k][0, 2]) for k in ('precision', 'recall', 'f1', 'assd', 'hausdorff'))
    # the mask form and the band
    m = fx.mask_boundary_scores(np.where(pred == 1, 0.9, 0.5).astype(np.float32)[:, None], gt[:, None].astype(np.float32))
    assert m['precision'][0] == 0.8 and m['recall'][0] == 1.0 and m['hausdorff'][0] == math.sqrt(8)
    band = fx.boundary_band(gt, 1)
    assert band.shape == (1, 1, 24, 24) and band.dtype == np.float32
    # rows 5 (outside) and 6 (inside) face each other across the boundary; radius 1 adds one row on either side
    assert band[0, 0, 3:9, 10].tolist() == [0, 1, 1, 1, 1, 0]
    assert band[0, 0, 5, 5] == 1 and band[0, 0, 4, 4] == 0 and band[0, 0, 12, 12] == 0


def test_generated_planes_have_the_structure_the_gpu_cases_rely_on():
    pred, gt = fx.layout_pair()
    assert pred.shape == gt.shape == (3, 40, 56)
    assert not (gt == 4).any() and not (pred == 4).any() and (pred == 3).any() and not (gt == 3).any()
    ids = fx.blocky(9, 2, 17, 23, (0, 1, 2, 3, 4))
    s = fx.scores_of(ids, 6, 3)
    assert s.dtype == np.float32 and np.array_equal(fx.label_ids(s), ids)
    assert ((s == s.max(1, keepdims=True)).sum(1) > 1).any()                      # ties occur
    r = fx.boundary_scores(pred, gt, 5, 2.0)
    assert np.isnan(r['f1'][:, 4]).all() and (r['f1'][:, 3] == 0).all() and np.isnan(r['assd'][:, 3]).all()
    assert (r['f1'][:, :3] > 0).all() and (r['f1'][:, :3] < 1).all()
