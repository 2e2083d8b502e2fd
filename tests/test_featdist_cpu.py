"""not gpu: the host side of the feature-space set metrics -- declarations, exports and bindings of the C ABI, the
argument checks the library makes before it launches anything, the host helpers of util.metrics (kid_subsets,
frechet_from_moments) against closed forms, SciPy and the numpy fixture of tests/featdist_fixture.py, properties of the
KID estimator, and planted defects showing that the checks used on the GPU can fail."""
import ctypes
import os
import re

import numpy as np
import pytest

import featdist_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_WORKSPACE = -1, -2
ENTRIES = ('him_feat_pool', 'him_feat_moments_ws', 'him_feat_moments', 'him_kid_sums_ws', 'him_kid_sums')
D = ctypes.c_double


def test_header_declares_library_exports_and_cabi_binds_every_entry():
    from neurips18_hierchical_image_manipulation_amd import _cabi, ops
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        header = f.read()
    assert 'Feature-space set metrics' in header
    for name in ENTRIES:
        assert re.search(r'^(int|size_t) %s\(' % name, header, flags=re.M), name
    for decl in (r'^#define HIM_FEAT_MAX_DIM %d$' % fx.FEAT_MAX_DIM, r'^#define HIM_KID_BAD_INDEX %d$' % fx.KID_BAD_INDEX):
        assert re.search(decl, header, flags=re.M), decl
    assert os.path.isfile(_cabi.LIB_PATH), 'libhim_hip.so not built'
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in ENTRIES:
        assert name in _cabi.EXPORTS and hasattr(dll, name), name
    assert (ops.FEAT_MAX_DIM, ops.KID_BAD_INDEX) == (fx.FEAT_MAX_DIM, fx.KID_BAD_INDEX)
    for f in ('feat_pool', 'feat_moments', 'kid_sums'):
        assert callable(getattr(ops, f))


def test_argument_checks_return_before_any_launch():
    """Nothing below reaches a launch: the pointers are never dereferenced on the host, and every call is refused."""
    from neurips18_hierchical_image_manipulation_amd import _cabi
    dll = _cabi.lib._load()
    p = 1 << 20

    order = ['x', 'B', 'C', 'h', 'w', 'feat', 'capacity', 'row0', 'D', 'c0', 'stream']
    good = dict(x=p, B=4, C=64, h=3, w=5, feat=p, capacity=10, row0=6, D=96, c0=32, stream=0)
    for name, value in (('row0', 7), ('row0', -1), ('capacity', 9), ('c0', 33), ('c0', -1), ('D', 95), ('B', 0), ('C', 0),
                        ('h', 0), ('w', 0), ('h', -3), ('D', 0), ('capacity', 0), ('x', 0), ('feat', 0), ('x', p + 2),
                        ('feat', p + 1)):
        assert dll.him_feat_pool(*[dict(good, **{name: value})[k] for k in order]) == E_INVALID, (name, value)
        assert b'feat_pool' in dll.him_last_error(), (name, value)
    assert dll.him_feat_pool(*[dict(good, h=1 << 16, w=1 << 16)[k] for k in order]) == E_INVALID       # h w > 2^31 - 1

    order = ['feat', 'row0', 'n', 'D', 'sum', 'second', 'ws', 'ws_bytes', 'stream']
    need = int(dll.him_feat_moments_ws(130, 512))
    assert need >= 16 and int(dll.him_feat_moments_ws(1, fx.FEAT_MAX_DIM)) > 0
    for n, dim in ((0, 4), (-1, 4), (4, 0), (4, fx.FEAT_MAX_DIM + 1), (4, -1)):
        assert int(dll.him_feat_moments_ws(n, dim)) == 0, (n, dim)
    good = dict(feat=p, row0=0, n=130, D=512, sum=p, second=p, ws=p, ws_bytes=need, stream=0)
    for name, value in (('D', 0), ('D', fx.FEAT_MAX_DIM + 1), ('D', -5), ('n', 0), ('n', -1), ('row0', -1), ('feat', 0),
                        ('sum', 0), ('second', 0), ('ws', 0), ('feat', p + 2), ('sum', p + 4), ('second', p + 4)):
        assert dll.him_feat_moments(*[dict(good, **{name: value})[k] for k in order]) == E_INVALID, (name, value)
        assert b'feat_moments' in dll.him_last_error(), (name, value)
    for short in (need - 1, 0):
        assert dll.him_feat_moments(*[dict(good, ws_bytes=short)[k] for k in order]) == E_WORKSPACE
        assert b'feat_moments' in dll.him_last_error()

    order = ['x', 'nx', 'y', 'ny', 'D', 'ix', 'iy', 'n_subsets', 'm', 'gamma', 'coef0', 'out', 'status', 'ws', 'ws_bytes',
             'stream']
    need = int(dll.him_kid_sums_ws(3, 130))
    assert need == 3 * 3 * 3 * 3 * 8                                   # 3 subsets x 3 blocks x (3 x 3 tiles of 64) doubles
    assert int(dll.him_kid_sums_ws(1, 2)) == 3 * 8
    for ns, m in ((0, 16), (-1, 16), (2, 1), (2, 0), (2, -4)):
        assert int(dll.him_kid_sums_ws(ns, m)) == 0, (ns, m)
    good = dict(x=p, nx=40, y=p, ny=56, D=70, ix=p, iy=p, n_subsets=3, m=130, gamma=D(0.0), coef0=D(1.0), out=p, status=p,
                ws=p, ws_bytes=need, stream=0)
    for name, value in (('m', 1), ('m', 0), ('n_subsets', 0), ('n_subsets', -1), ('D', 0), ('nx', 0), ('ny', 0), ('nx', -1),
                        ('nx', 1 << 31), ('gamma', D(-1.0)), ('gamma', D(float('nan'))), ('gamma', D(float('inf'))),
                        ('coef0', D(float('nan'))), ('coef0', D(float('inf'))), ('x', 0), ('y', 0), ('ix', 0), ('iy', 0),
                        ('out', 0), ('status', 0), ('ws', 0), ('x', p + 2), ('out', p + 4), ('ix', p + 1)):
        call = dict(good, **{name: value})
        if name in ('m', 'n_subsets'):
            call['ws_bytes'] = 1 << 40
        assert dll.him_kid_sums(*[call[k] for k in order]) == E_INVALID, (name, value)
        assert b'kid_sums' in dll.him_last_error(), (name, value)
    for short in (need - 1, 0):
        assert dll.him_kid_sums(*[dict(good, ws_bytes=short)[k] for k in order]) == E_WORKSPACE
        assert b'kid_sums' in dll.him_last_error()
    with pytest.raises(_cabi.HimError, match='kid_sums'):
        _cabi.lib.him_kid_sums(*[dict(good, m=1)[k] for k in order])


def test_bindings_refuse_host_tensors_and_evaluator_keys():
    import torch
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    with pytest.raises(ValueError, match='feat_pool.*device tensor'):
        ops.feat_pool(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3), 0)
    with pytest.raises(ValueError, match='feat_moments.*device tensor'):
        ops.feat_moments(torch.zeros(4, 4), 0, 4, torch.zeros(4, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match='kid_sums.*device tensor'):
        ops.kid_sums(torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(1, 2, dtype=torch.int32),
                     torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match='device'):
        metrics.FeatureDistance().add_features(torch.zeros(4, 4))
    assert metrics.FEATURE_KEYS == ('kid', 'kid_std', 'frechet', 'n_features')
    assert list(metrics.Evaluator(35).summary()) == list(metrics.SUMMARY_KEYS)
    assert list(metrics.Evaluator(35, swd=dict(n_patches=4, n_dirs=8)).summary()) == list(metrics.SUMMARY_KEYS + metrics.SWD_KEYS)
    out = metrics.Evaluator(35, swd=dict(n_patches=4, n_dirs=8), features=dict(n_subsets=4)).summary()
    assert list(out) == list(metrics.SUMMARY_KEYS + metrics.SWD_KEYS + metrics.FEATURE_KEYS)
    assert out['n_features'] == 0 and all(out[k] != out[k] for k in ('kid', 'kid_std', 'frechet'))
    out = metrics.Evaluator(35, features=True).summary()
    assert list(out) == list(metrics.SUMMARY_KEYS + metrics.FEATURE_KEYS)
    fd = metrics.FeatureDistance()
    assert fd.n_features == (0, 0) and fd.frechet() != fd.frechet()
    with pytest.raises(ValueError, match='2 rows'):
        fd.kid()
    with pytest.raises(ValueError, match='layers'):
        metrics.FeatureDistance(layers=(5,))


def test_kid_subsets():
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    t = metrics.kid_subsets(3, 0, 50, 7, 20)
    assert t.shape == (7, 20) and t.dtype == np.int32 and t.min() >= 0 and t.max() < 50
    assert all(len(set(row.tolist())) == 20 for row in t)                          # no index twice in a row
    full = metrics.kid_subsets(3, 0, 50, 7, 50)
    assert all(sorted(row.tolist()) == list(range(50)) for row in full)            # subset_size == n: a permutation
    assert len({tuple(row.tolist()) for row in full}) == 7                         # and the subsets differ
    assert not np.array_equal(t, metrics.kid_subsets(3, 1, 50, 7, 20))             # the other set: another table
    assert not np.array_equal(t, metrics.kid_subsets(4, 0, 50, 7, 20))
    assert np.array_equal(t, metrics.kid_subsets(3, 0, 50, 7, 20))
    assert np.array_equal(t, fx.subsets(3, 0, 50, 7, 20))
    with pytest.raises(ValueError, match='kid_subsets'):
        metrics.kid_subsets(3, 0, 5, 2, 6)


def _moments_of(mu, S, n):
    """(n, sum, second) whose ddof = 1 fit is exactly the Gaussian N(mu, S)."""
    mu, S = np.asarray(mu, np.float64), np.asarray(S, np.float64)
    return n, n * mu, (n - 1) * S + n * np.outer(mu, mu)


def _raw(x):
    x = np.asarray(x, np.float64)
    return len(x), x.sum(0), x.T @ x


def test_frechet_from_moments_closed_forms():
    from neurips18_hierchical_image_manipulation_amd.util.metrics import frechet_from_moments as fm
    x = fx.features(1, 200, 24)
    (_, S), raw = fx.gaussian_fit(x), _raw(x)
    assert abs(fm(*(raw + raw))) <= 1e-9 * 2 * np.trace(S)                          # a set against itself
    dim, s = 16, 1.7
    mu = np.random.default_rng(2).standard_normal(dim)
    got = fm(*(_moments_of(np.zeros(dim), np.eye(dim), 500) + _moments_of(mu, s * s * np.eye(dim), 300)))
    want = mu @ mu + dim * (1 - s) ** 2                                             # N(0, I) against N(mu, s^2 I)
    assert abs(got - want) <= 1e-9 * want, (got, want)
    g = np.random.default_rng(3)
    a, b = g.uniform(0.1, 4.0, dim), g.uniform(0.1, 4.0, dim)
    got = fm(*(_moments_of(np.zeros(dim), np.diag(a), 50) + _moments_of(np.zeros(dim), np.diag(b), 60)))
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()                                   # commuting diagonal covariances
    assert abs(got - want) <= 1e-9 * (a.sum() + b.sum()), (got, want)
    assert fm(1, np.zeros(3), np.zeros((3, 3)), 5, np.zeros(3), np.eye(3)) != fm(1, np.zeros(3), np.zeros((3, 3)), 5, np.zeros(3), np.eye(3))
    assert np.isnan(fm(5, np.zeros(3), np.eye(3), 1, np.zeros(3), np.zeros((3, 3))))


def test_frechet_from_moments_against_scipy_sqrtm_and_the_fixture():
    from neurips18_hierchical_image_manipulation_amd.util.metrics import frechet_from_moments as fm
    x, y = fx.features(4, 300, 20), fx.features(5, 260, 20, shift=0.4, scale=1.3)
    got, scale = fm(*(_raw(x) + _raw(y))), fx.frechet_scale(x, y)
    assert abs(got - fx.frechet(x, y)) <= 1e-9 * scale
    la = pytest.importorskip('scipy.linalg')
    (m1, S1), (m2, S2) = fx.gaussian_fit(x), fx.gaussian_fit(y)
    root = la.sqrtm(S1 @ S2)
    root = root[0] if isinstance(root, tuple) else root
    want = (m1 - m2) @ (m1 - m2) + np.trace(S1) + np.trace(S2) - 2.0 * np.trace(root).real
    assert abs(got - want) <= 1e-9 * scale, (got, want)


def test_frechet_of_rank_deficient_covariances_is_finite():
    from neurips18_hierchical_image_manipulation_amd.util.metrics import frechet_from_moments as fm
    x, y = fx.features(6, 8, 32), fx.features(7, 8, 32, shift=0.2)                  # 8 rows, 32 dimensions
    got, scale = fm(*(_raw(x) + _raw(y))), fx.frechet_scale(x, y)
    assert np.isfinite(got) and got >= -1e-9 * scale
    assert abs(fm(*(_raw(x) + _raw(x)))) <= 1e-9 * scale                            # the null space does not leak in
    assert abs(got - fx.frechet(x, y)) <= 1e-9 * scale


def test_fixture_kid_is_centred_for_one_distribution_and_positive_for_a_shift():
    # 40 subsets of 50 rows out of 2000 per set: the subsets hardly overlap, so their spread measures the mean's error
    g = np.random.default_rng(8)
    pool = (np.abs(g.standard_normal((4000, 8))) + 0.2).astype(np.float32)
    mean, std, est, m = fx.kid(pool[:2000], pool[2000:], 40, 50, seed=1)
    assert m == 50 and abs(mean) < 3.0 * std / np.sqrt(len(est)), (mean, std)      # within 3 standard errors of zero
    shifted, sstd, _, _ = fx.kid(pool[:2000], pool[2000:] + np.float32(0.5), 40, 50, seed=1)
    assert shifted > 0 and shifted > 3.0 * sstd / np.sqrt(40) and shifted > 10 * abs(mean), (shifted, mean)


def test_planted_defects_turn_the_gpu_checks_red():
    x, y = fx.features(9, 40, 70), fx.features(10, 56, 70, shift=0.3)
    ix, iy = fx.subsets(0, 0, 40, 3, 37), fx.subsets(0, 1, 56, 3, 37)
    ref, bound = fx.kid_sums(x, y, ix, iy), fx.kid_sums_bound(x, y, ix, iy)
    # a float64 restatement that sums in another order passes its own check
    fx.check_bound('clean', 'kid', fx.kid_sums(x[:, ::-1], y[:, ::-1], ix, iy), ref, bound)
    with pytest.raises(AssertionError, match='kid'):                                # the diagonal kept
        fx.check_bound('diagonal', 'kid', fx.kid_sums(x, y, ix, iy, keep_diagonal=True), ref, bound)
    with pytest.raises(AssertionError, match='kid'):                                # gamma = 1 in place of 1 / D
        fx.check_bound('gamma', 'kid', fx.kid_sums(x, y, ix, iy, gamma=1.0), ref, bound)
    xi, yi = fx.int_rows(1, 40, 6, 9), fx.int_rows(2, 56, 6, 9)
    want = fx.kid_sums(xi, yi, ix, iy, 1.0, 0.0)
    assert np.abs(want).max() < 2.0 ** 53
    with pytest.raises(AssertionError, match='kid'):
        fx.check_equal('diagonal', 'kid', fx.kid_sums(xi, yi, ix, iy, 1.0, 0.0, keep_diagonal=True), want)
    feat = fx.features(11, 17, 16)                                                  # one 16 x 16 tile
    (s, q), (bs, bq) = fx.moments(feat), fx.moments_bound(feat)
    fx.check_bound('clean', 'second', fx.moments(feat[::-1])[1], q, bq)
    with pytest.raises(AssertionError, match='second'):                             # the f32 row map on the f64 tile
        fx.check_bound('rowmap', 'second', fx.moments(feat, rowmap='f32')[1], q, bq)
    wrong = fx.moments(feat, rowmap='f32')[1]
    assert (wrong[[0, 5, 10, 15]] == q[[0, 5, 10, 15]]).all() and (wrong != q).any(1).sum() == 12   # 3 rows of every 4
    ref_f, scale = fx.frechet(x, y), fx.frechet_scale(x, y)
    assert abs(fx.frechet(x[::-1], y) - ref_f) <= 1e-9 * scale
    assert abs(fx.frechet(x, y, ddof=0) - ref_f) > 1e-9 * scale                     # a population covariance
    maps = fx.maps(12, 2, 5, 3, 5)
    fx.check_bound('clean', 'pool', fx.pool(maps).astype(np.float32), fx.pool(maps), fx.pool_bound(maps))
    with pytest.raises(AssertionError, match='pool'):                               # a 3 x 5 plane divided by 16, not 15
        fx.check_bound('count', 'pool', fx.pool(maps) * (15.0 / 16.0), fx.pool(maps), fx.pool_bound(maps))
