"""not gpu: the host side of the k-nearest-neighbour measures (precision, recall, density, coverage) -- declarations,
exports and bindings of the C ABI, the argument checks the library makes before it launches anything, self-checks of the
float64 fixture of tests/prdc_fixture.py (among them the condition the GPU tests rest on: no real-valued case has an
uncertain decision), util.metrics.prdc_from_counts against a brute-force loop, and CPU stand-ins of the kernels with one
planted defect each, which the checks used on the GPU must catch."""
import ctypes
import os
import re

import numpy as np
import pytest

import prdc_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_WORKSPACE = -1, -2
ENTRIES = ('him_knn_radii_ws', 'him_knn_radii', 'him_knn_membership_ws', 'him_knn_membership')


def test_header_declares_library_exports_and_cabi_binds_every_entry():
    from neurips18_hierchical_image_manipulation_amd import _cabi, ops
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        header = f.read()
    for name in ENTRIES:
        assert re.search(r'^(int|size_t) %s\(' % name, header, flags=re.M), name
    for decl in (r'^#define HIM_KNN_MAX_K %d$' % fx.KNN_MAX_K, r'^#define HIM_KNN_NONFINITE %d$' % fx.KNN_NONFINITE):
        assert re.search(decl, header, flags=re.M), decl
    assert os.path.isfile(_cabi.LIB_PATH), 'libhim_hip.so not built'
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in ENTRIES:
        assert name in _cabi.EXPORTS and hasattr(dll, name), name
    assert (ops.KNN_MAX_K, ops.KNN_NONFINITE, ops.FEAT_MAX_DIM) == (fx.KNN_MAX_K, fx.KNN_NONFINITE, fx.FEAT_MAX_DIM)
    for f in ('knn_radii', 'knn_membership'):
        assert callable(getattr(ops, f))
    with open(os.path.join(ROOT, 'neurips18_hierchical_image_manipulation_amd', 'csrc', 'him_prdc.hip')) as f:
        src = f.read()
    for name, value in (('KNN_TILE', fx.TILE), ('KNN_CHUNK_TILES', fx.CHUNK_TILES), ('KNN_MAX_CHUNKS', fx.MAX_CHUNKS),
                        ('KNN_MEMBER_SPLIT', fx.MEMBER_SPLIT)):                     # what the GPU shapes are chosen by
        assert re.search(r'^#define %s %d\b' % (name, value), src, flags=re.M), name


def test_argument_checks_return_before_any_launch():
    """Nothing below reaches a launch: the pointers are never dereferenced on the host, and every call is refused with a
    text that names the entry and the argument."""
    from neurips18_hierchical_image_manipulation_amd import _cabi
    dll = _cabi.lib._load()
    p = 1 << 20

    # the norms and one partial list of k per row and chunk; 130 rows are one chunk, 513 two, 8193 fifteen of nine tiles
    assert int(dll.him_knn_radii_ws(130, 67, 5)) == (130 + 130 * 5) * 8
    assert int(dll.him_knn_radii_ws(512, 4, 3)) == (512 + 512 * 3) * 8
    assert int(dll.him_knn_radii_ws(513, 4, 3)) == (513 + 513 * 2 * 3) * 8
    assert int(dll.him_knn_radii_ws(8192, 4, 16)) == (8192 + 8192 * 16 * 16) * 8
    assert int(dll.him_knn_radii_ws(8193, 4, 16)) == (8193 + 8193 * 15 * 16) * 8
    assert int(dll.him_knn_radii_ws(2, 1, 1)) > 0 and int(dll.him_knn_radii_ws(17, fx.FEAT_MAX_DIM, fx.KNN_MAX_K)) > 0
    for n, dim, k in ((5, 4, 5), (5, 4, 0), (5, 4, -1), (40, 4, fx.KNN_MAX_K + 1), (40, 0, 3), (40, fx.FEAT_MAX_DIM + 1, 3),
                      (0, 4, 1), (-3, 4, 1), (1 << 31, 4, 1)):
        assert int(dll.him_knn_radii_ws(n, dim, k)) == 0, (n, dim, k)
    order = ['x', 'n', 'D', 'k', 'radii2', 'status', 'ws', 'ws_bytes', 'stream']
    need = int(dll.him_knn_radii_ws(130, 67, 5))
    good = dict(x=p, n=130, D=67, k=5, radii2=p, status=p, ws=p, ws_bytes=need, stream=0)
    for name, value, word in (('k', 0, b'k'), ('k', -2, b'k'), ('k', fx.KNN_MAX_K + 1, b'k'), ('n', 5, b'n'), ('n', 4, b'n'),
                              ('n', 0, b'n'), ('n', -1, b'n'), ('n', 1 << 31, b'n'), ('D', 0, b'D'), ('D', -1, b'D'),
                              ('D', fx.FEAT_MAX_DIM + 1, b'D'), ('x', 0, b'x'), ('radii2', 0, b'radii2'),
                              ('status', 0, b'status'), ('ws', 0, b'ws'), ('x', p + 2, b'x'), ('radii2', p + 4, b'radii2'),
                              ('status', p + 1, b'status'), ('ws', p + 4, b'ws')):
        call = dict(good, **{name: value})
        if name in ('n', 'k'):
            call['ws_bytes'] = 1 << 40
        assert dll.him_knn_radii(*[call[k] for k in order]) == E_INVALID, (name, value)
        text = dll.him_last_error()
        assert b'knn_radii' in text and word in text.split(b':', 1)[1], (name, value, text)
    for short in (need - 1, 0):
        assert dll.him_knn_radii(*[dict(good, ws_bytes=short)[k] for k in order]) == E_WORKSPACE
        assert b'knn_radii' in dll.him_last_error() and b'ws_bytes' in dll.him_last_error()

    assert int(dll.him_knn_membership_ws(33, 70, 5)) == (33 + 70) * 8
    for nq, nr, dim in ((0, 4, 4), (4, 0, 4), (-1, 4, 4), (4, 1 << 31, 4), (4, 4, 0), (4, 4, fx.FEAT_MAX_DIM + 1)):
        assert int(dll.him_knn_membership_ws(nq, nr, dim)) == 0, (nq, nr, dim)
    order = ['q', 'nq', 'r', 'nr', 'D', 'radii2', 'row_count', 'col_count', 'status', 'ws', 'ws_bytes', 'stream']
    need = int(dll.him_knn_membership_ws(33, 70, 5))
    good = dict(q=p, nq=33, r=p, nr=70, D=5, radii2=p, row_count=p, col_count=p, status=p, ws=p, ws_bytes=need, stream=0)
    for name, value, word in (('nq', 0, b'nq'), ('nr', 0, b'nr'), ('nq', -1, b'nq'), ('nr', 1 << 31, b'nr'), ('D', 0, b'D'),
                              ('D', fx.FEAT_MAX_DIM + 1, b'D'), ('q', 0, b'q'), ('r', 0, b'r'), ('radii2', 0, b'radii2'),
                              ('status', 0, b'status'), ('ws', 0, b'ws'), ('q', p + 2, b'q'), ('r', p + 1, b'r'),
                              ('radii2', p + 4, b'radii2'), ('row_count', p + 2, b'row_count'),
                              ('col_count', p + 1, b'col_count'), ('ws', p + 4, b'ws')):
        call = dict(good, **{name: value})
        if name in ('nq', 'nr'):
            call['ws_bytes'] = 1 << 40
        assert dll.him_knn_membership(*[call[k] for k in order]) == E_INVALID, (name, value)
        text = dll.him_last_error()
        assert b'knn_membership' in text and word in text.split(b':', 1)[1], (name, value, text)
    assert dll.him_knn_membership(*[dict(good, row_count=0, col_count=0)[k] for k in order]) == E_INVALID
    assert b'both null' in dll.him_last_error()
    for short in (need - 1, 0):
        assert dll.him_knn_membership(*[dict(good, ws_bytes=short)[k] for k in order]) == E_WORKSPACE
        assert b'knn_membership' in dll.him_last_error() and b'ws_bytes' in dll.him_last_error()
    with pytest.raises(_cabi.HimError, match='knn_radii'):
        _cabi.lib.him_knn_radii(*[dict(good, x=p, n=3, k=5, radii2=p)[k] for k in
                                  ['x', 'n', 'D', 'k', 'radii2', 'status', 'ws', 'ws_bytes', 'stream']])


def test_bindings_refuse_host_tensors_and_bad_arguments():
    import torch
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    with pytest.raises(ValueError, match='knn_radii.*device tensor'):
        ops.knn_radii(torch.zeros(8, 4), 3)
    with pytest.raises(ValueError, match='knn_membership.*device tensor'):
        ops.knn_membership(torch.zeros(8, 4), torch.zeros(8, 4), torch.zeros(8, dtype=torch.float64))
    for k in (0, fx.KNN_MAX_K + 1):
        with pytest.raises(ValueError, match='nearest_k'):
            metrics.FeatureDistance(nearest_k=k)
        with pytest.raises(ValueError, match='nearest_k'):
            metrics.FeatureDistance().prdc(k)
    with pytest.raises(ValueError, match='more than k rows'):
        metrics.FeatureDistance().prdc_counts(3)
    with pytest.raises(ValueError, match='prdc_from_counts'):
        metrics.prdc_from_counts(3, torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match='prdc_from_counts'):
        metrics.prdc_from_counts(0, *([torch.zeros(4, dtype=torch.int32)] * 3))
    with pytest.raises(ValueError, match='prdc_from_counts'):
        metrics.prdc_from_counts(3, torch.zeros(0, dtype=torch.int32), *([torch.zeros(4, dtype=torch.int32)] * 2))


def test_evaluator_keys_with_and_without_nearest_k_and_nan_below_k_plus_one_rows():
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    assert metrics.PRDC_KEYS == ('precision', 'recall', 'density', 'coverage', 'nearest_k')
    assert metrics.FEATURE_KEYS == ('kid', 'kid_std', 'frechet', 'n_features')
    assert list(metrics.Evaluator(35).summary()) == list(metrics.SUMMARY_KEYS)
    assert list(metrics.Evaluator(35, features=True).summary()) == list(metrics.SUMMARY_KEYS + metrics.FEATURE_KEYS)
    assert list(metrics.Evaluator(35, features=dict(n_subsets=4)).summary()) == list(metrics.SUMMARY_KEYS + metrics.FEATURE_KEYS)
    out = metrics.Evaluator(35, swd=dict(n_patches=4, n_dirs=8), features=dict(n_subsets=4, nearest_k=5)).summary()
    assert list(out) == list(metrics.SUMMARY_KEYS + metrics.SWD_KEYS + metrics.FEATURE_KEYS + metrics.PRDC_KEYS)
    assert out['nearest_k'] == 5 and all(out[k] != out[k] for k in metrics.PRDC_KEYS[:4])
    fd = metrics.FeatureDistance()
    assert fd.nearest_k is None and metrics.FeatureDistance(nearest_k=7).nearest_k == 7
    got = fd.prdc()
    assert list(got) == list(metrics.PRDC_KEYS[:4])
    assert all(v.dtype.is_floating_point and v.element_size() == 8 and v.dim() == 0 and bool(v != v) for v in got.values())


def test_prdc_from_counts_agrees_with_a_brute_force_loop():
    import torch
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    g = np.random.default_rng(0)
    for k, ny, nx in ((5, 40, 56), (1, 7, 3), (16, 33, 70)):
        row_fr = g.integers(0, 4, ny) * g.integers(0, 2, ny)
        col_r, row_rf = g.integers(0, 3, nx) * g.integers(0, 2, nx), g.integers(0, 2, nx)
        want = fx.prdc_from_counts(k, row_fr, col_r, row_rf)
        got = metrics.prdc_from_counts(k, *(torch.from_numpy(v.astype(np.int32)) for v in (row_fr, col_r, row_rf)))
        assert list(got) == list(want) == list(metrics.PRDC_KEYS[:4])
        for key in want:
            assert got[key].dtype == torch.float64 and got[key].dim() == 0
            assert abs(float(got[key]) - want[key]) <= 4 * fx.U * max(want[key], 1.0), key


# -------------------------------------------------------------------------------------------------- fixture self-checks
@pytest.mark.parametrize('index', range(len(fx.REAL_CASES)))
def test_no_real_valued_gpu_case_has_an_uncertain_decision(index):
    """The condition the GPU tests rest on; both directions, with the reference radii and with radii carrying the radius
    bound (the chained calls of the Python surface).  If a seed violates it, the seed changes, never the rule."""
    fake, real, k = fx.real_case(index)
    for q, r in ((fake, real), (real, fake)):
        r2 = fx.radii(r, k)
        assert np.isfinite(r2).all() and (r2 > 0).all()
        for rb in (0.0, fx.radii_bound(r)):
            row_lo, row_hi, col_lo, col_hi, uncertain = fx.membership_bounds(q, r, r2, rb)
            assert uncertain == 0 and (row_lo == row_hi).all() and (col_lo == col_hi).all()
            ref_rows, ref_cols = fx.membership(q, r, r2)
            assert (ref_rows == row_lo).all() and (ref_cols == col_lo).all()
    # the radius is well separated from its neighbours in the order statistics, so k - 1 and k + 1 are different values
    d = np.sort(fx.dist2(real, real) + np.diag(np.full(len(real), np.inf)), 1)
    if len(real) > k + 1:
        assert ((d[:, k] - d[:, k - 1]) > 2 * fx.radii_bound(real)).all()


def test_fixture_closed_forms():
    k = 3
    a = fx.features(1, 30, 8)
    far = (fx.features(2, 25, 8) + np.float32(1000.0)).astype(np.float32)
    assert list(fx.prdc(a, far, k).values()) == [0.0, 0.0, 0.0, 0.0]                 # two far-apart clusters
    same = fx.prdc(a, a, k)                                                          # Y = X, distinct rows
    assert same['precision'] == same['recall'] == same['coverage'] == 1.0
    # every point lies in its own ball and in those of the points it is a k-nearest neighbour of: k + 1 balls on average
    assert same['density'] == pytest.approx((k + 1.0) / k)
    # a hand-made line: 0, 1, 3, 7 with k = 1 has the radii 1, 1, 4, 16
    line = np.array([[0.0], [1.0], [3.0], [7.0]], np.float32)
    assert fx.radii(line, 1).tolist() == [1.0, 1.0, 4.0, 16.0]
    assert fx.radii(line, 2).tolist() == [9.0, 4.0, 9.0, 36.0]
    rows, cols = fx.membership(np.array([[2.0], [-1.0], [20.0]], np.float32), line, fx.radii(line, 1))
    assert rows.tolist() == [2, 1, 0] and cols.tolist() == [1, 1, 1, 0]              # 2 is within 1 of 1 and within 2 of 3
    # self by position: a duplicate row is a neighbour at distance 0, and `<=` counts it
    dup = fx.with_duplicates(fx.lattice(3, 6, 4, 3), 3)
    assert (fx.radii(dup, 2) == 0).all() and (fx.radii(dup, 3) > 0).any()
    rows, cols = fx.membership(dup, dup, fx.radii(dup, 2))
    assert (rows >= 3).all() and (cols >= 3).all()
    # integers: the extended-precision direct form and the int64 Gram form agree exactly
    x, y = fx.lattice(4, 70, 5, 6), fx.lattice(5, 33, 5, 6)
    assert (fx.dist2(x, y) == fx.int_dist2(x, y)).all() and (fx.radii(x, 5) == fx.int_radii(x, 5, block=16)).all()
    r2 = fx.int_radii(y, 3)
    assert all((a == b).all() for a, b in zip(fx.membership(x, y, r2), fx.int_membership(x, y, r2)))
    # a non-finite row: NaN radius, nobody's neighbour, the others as if it were not there
    bad = x.copy()
    bad[7, 2], bad[20, 0] = np.nan, np.inf
    keep = np.ones(len(x), bool)
    keep[[7, 20]] = False
    r2 = fx.radii(bad, 4)
    assert np.isnan(r2[[7, 20]]).all() and (r2[keep] == fx.radii(x[keep], 4)).all()
    rows, cols = fx.membership(bad, bad, r2)
    assert (rows[[7, 20]] == 0).all() and (cols[[7, 20]] == 0).all()


# ------------------------------------------------------------------------------------------------------ planted defects
def _radii_checks(case, x, k, got):
    """What tests/test_prdc_abi_gpu.py asserts of a real-valued radii call."""
    fx.check_nonnegative(case, 'radii2 sign', got)
    fx.check_bound(case, 'radii2', got, fx.radii(x, k), fx.radii_bound(x))


def _member_checks(case, q, r, r2, got):
    """... and of a real-valued membership call on the reference radii."""
    row_lo, row_hi, col_lo, col_hi, _ = fx.membership_bounds(q, r, r2)
    fx.check_counts(case, 'row_count', got[0], row_lo, row_hi)
    fx.check_counts(case, 'col_count', got[1], col_lo, col_hi)


def test_clean_stand_ins_pass_the_gpu_checks():
    for index in range(len(fx.REAL_CASES)):
        fake, real, k = fx.real_case(index)
        _radii_checks('clean %d' % index, real, k, fx.standin_radii(real, k))
        r2 = fx.radii(real, k)
        _member_checks('clean %d' % index, fake, real, r2, fx.standin_membership(fake, real, r2))
    x = fx.lattice(6, 70, 5, 4)
    fx.check_equal('clean int', 'radii2', fx.standin_radii(x, 5), fx.int_radii(x, 5))


@pytest.mark.parametrize('defect', [dict(keep_self=True), dict(kth=-1), dict(kth=1), dict(rowmap='f32'), dict(ragged=True)],
                         ids=lambda d: '%s=%s' % list(d.items())[0])
def test_planted_radii_defects_turn_the_gpu_checks_red(defect):
    fake, real, k = fx.real_case(0)                                                  # 70 rows: a ragged tile of 6
    real = (real - np.float32(0.9)).astype(np.float32)                               # rows near the origin, where the padding sits
    _radii_checks('clean', real, k, fx.standin_radii(real, k))
    with pytest.raises(AssertionError, match='radii2'):
        _radii_checks('defect', real, k, fx.standin_radii(real, k, **defect))
    x = fx.distinct_norm_rows(7, 70, 5, 9)                                            # the integer case catches it too
    fx.check_equal('clean int', 'radii2', fx.standin_radii(x, k), fx.int_radii(x, k))
    with pytest.raises(AssertionError, match='radii2'):
        fx.check_equal('defect int', 'radii2', fx.standin_radii(x, k, **defect), fx.int_radii(x, k))


def test_a_missing_clamp_turns_the_sign_check_red():
    # real-valued duplicate rows: the norms and the dot product are summed in different orders, so |a|^2 + |a|^2 - 2 a.a
    # is a rounding error of either sign; the bound alone would let a small negative value pass
    x = fx.with_duplicates(fx.features(8, 40, 67), 2)
    raw = fx.standin_dist2(x[:40], x[40:], clamp=False)
    assert (np.diag(raw) < 0).any()
    _radii_checks('clean', x, 1, fx.standin_radii(x, 1))
    assert (fx.radii(x, 1) == 0).all()
    with pytest.raises(AssertionError, match='negative'):
        _radii_checks('defect', x, 1, fx.standin_radii(x, 1, clamp=False))


@pytest.mark.parametrize('defect', [dict(query_radius=True), dict(swap=True), dict(rowmap='f32'), dict(ragged=True)],
                         ids=lambda d: '%s=%s' % list(d.items())[0])
def test_planted_membership_defects_turn_the_gpu_checks_red(defect):
    fake, real, k = fx.real_case(0)                                                  # 33 x 70: nq != nr, both ragged
    r2 = fx.radii(real, k)
    _member_checks('clean', fake, real, r2, fx.standin_membership(fake, real, r2))
    if 'ragged' in defect:                                                           # the padding counts where a ball holds the origin
        real = (real - np.float32(0.9)).astype(np.float32)
        fake = (fake - np.float32(0.9)).astype(np.float32)
        r2 = fx.radii(real, k)
        assert fx.membership_bounds(fake, real, r2)[4] == 0
        _member_checks('clean', fake, real, r2, fx.standin_membership(fake, real, r2))
    with pytest.raises(AssertionError, match='count'):
        _member_checks('defect', fake, real, r2, fx.standin_membership(fake, real, r2, **defect))


def test_strict_comparison_turns_the_duplicate_row_check_red():
    # duplicate integer rows with k <= the number of copies besides the row itself: the radius is exactly 0 and only
    # `<=` counts the copies
    x = fx.with_duplicates(fx.distinct_norm_rows(9, 20, 5, 4), 3)
    r2 = fx.int_radii(x, 2)
    assert (r2 == 0).all()
    want = fx.int_membership(x, x, r2)
    assert (want[0] == 3).all() and (want[1] == 3).all()
    got = fx.standin_membership(x, x, r2)
    fx.check_equal('clean', 'row_count', got[0], want[0])
    fx.check_equal('clean', 'col_count', got[1], want[1])
    with pytest.raises(AssertionError, match='row_count'):
        fx.check_equal('defect', 'row_count', fx.standin_membership(x, x, r2, strict=True)[0], want[0])
