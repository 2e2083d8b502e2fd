"""-m gpu: him_feat_pool, him_feat_moments and him_kid_sums at the C ABI inside tests/abi_harness.py's guarded arena,
against the float64 numpy restatement of tests/featdist_fixture.py.

Arena (tests/README.md): every buffer of a call is a view in ONE allocation between 64 KiB bands; NaN bands beside
inputs, 0xA5 bands beside outputs and workspace, compared bit for bit afterwards; fresh outputs and workspace are
pre-filled with NaN bytes (the moment accumulators, which the entry adds to, with the values the case starts from); the
workspace is exactly the queried size; inputs are compared bit for bit after the call.

Bounds, derived and not tuned, u = 2^-53:
  pool     |got - ref64| <= 2^-24 |ref64| + u sum|x| per plane; cells outside the written block keep their fill;
  moments  |second_ab - ref| <= (n + 4) u sum_i |x_ia x_ib|, likewise for sum; second equals its transpose bit for bit;
           small-integer features give sum and second EQUAL to the integer result;
  KID      |S - ref| <= (3 D + P + 16) u sum T^3, T_ij = gamma sum_k |x_ik y_jk| + |coef0|, P the number of summed pairs;
           integer features with gamma = 1, coef0 = 0 give all three sums EQUAL to the integer result (rows of distinct
           norms: a wrong diagonal or edge mask cannot cancel).
One JSON line per checked tensor goes to featdist_abi_rows.jsonl in the GPU tests' report directory before its assertion
runs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi_harness as ah
import featdist_fixture as fx
from test_model_gpu import OUT as REPORT_DIR

pytestmark = pytest.mark.gpu

ROWS = fx.RowFile(os.path.join(REPORT_DIR, 'featdist_abi_rows.jsonl'))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _as_floats(arr):
    raw = np.ascontiguousarray(arr).tobytes()
    assert len(raw) % 4 == 0
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy().view(np.float32))


def _bytes_of(view, n):
    return bytes(view.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)[:n])


def _finish(lib, ar, rc, inputs):
    torch.cuda.synchronize()
    assert rc == 0, lib.him_last_error()
    bad = ar.guard_failures()
    assert not bad, '; '.join(bad)
    for name, arr in inputs.items():
        raw = np.ascontiguousarray(arr).tobytes()
        assert _bytes_of(ar.t[name], len(raw)) == raw, 'input %s was written' % name


def _np(ar, name, dtype, shape):
    return ar.t[name].contiguous().view(torch.uint8).cpu().numpy().reshape(-1).view(dtype)[:int(np.prod(shape))].reshape(shape).copy()


def call_pool(slices, capacity, row0, D):
    """``slices``: [(x (B, C, h, w), c0), ...], one call each into the same NaN-filled feat (capacity, D)."""
    lib = ah.raw_lib()
    specs = {'x%d' % i: ('in', torch.from_numpy(x)) for i, (x, _) in enumerate(slices)}
    specs['feat'] = ('ws', capacity * D * 4)
    ar = ah.Arena('cuda', specs)
    for i, (x, c0) in enumerate(slices):
        B, C, h, w = x.shape
        rc = lib.him_feat_pool(ar.ptr('x%d' % i), B, C, h, w, ar.ptr('feat'), capacity, row0, D, c0, _stream())
        assert rc == 0, lib.him_last_error()
    _finish(lib, ar, 0, {'x%d' % i: x for i, (x, _) in enumerate(slices)})
    return _np(ar, 'feat', np.float32, (capacity, D))


def call_moments(feat, calls, sum0=None, second0=None):
    """him_feat_moments once per (row0, n) of ``calls`` into the same accumulators; (sum, second)."""
    lib = ah.raw_lib()
    D = feat.shape[1]
    s0 = np.zeros(D) if sum0 is None else sum0
    q0 = np.zeros((D, D)) if second0 is None else second0
    need = max(int(lib.him_feat_moments_ws(n, D)) for _, n in calls)
    assert need > 0
    ar = ah.Arena('cuda', {'feat': ('in', torch.from_numpy(feat)), 'sum': ('out', (D * 2,), _as_floats(s0)),
                           'second': ('out', (D * D * 2,), _as_floats(q0)), 'ws': ('ws', need)})
    for row0, n in calls:
        assert int(lib.him_feat_moments_ws(n, D)) <= need
        rc = lib.him_feat_moments(ar.ptr('feat'), row0, n, D, ar.ptr('sum'), ar.ptr('second'), ar.ptr('ws'), need, _stream())
        assert rc == 0, lib.him_last_error()
    _finish(lib, ar, 0, {'feat': feat})
    return _np(ar, 'sum', np.float64, (D,)), _np(ar, 'second', np.float64, (D, D))


def call_kid(x, y, ix, iy, gamma=0.0, coef0=1.0):
    lib = ah.raw_lib()
    n_subsets, m = ix.shape
    need = int(lib.him_kid_sums_ws(n_subsets, m))
    assert need > 0
    ar = ah.Arena('cuda', {'x': ('in', torch.from_numpy(x)), 'y': ('in', torch.from_numpy(y)), 'ix': ('in', _as_floats(ix)),
                           'iy': ('in', _as_floats(iy)), 'out': ('ws', n_subsets * 3 * 8),
                           'status': ('out', (1,), _as_floats(np.zeros(1, np.int32))), 'ws': ('ws', need)})
    rc = lib.him_kid_sums(ar.ptr('x'), x.shape[0], ar.ptr('y'), y.shape[0], x.shape[1], ar.ptr('ix'), ar.ptr('iy'), n_subsets, m,
                          ctypes.c_double(gamma), ctypes.c_double(coef0), ar.ptr('out'), ar.ptr('status'), ar.ptr('ws'), need,
                          _stream())
    _finish(lib, ar, rc, {'x': x, 'y': y, 'ix': ix, 'iy': iy})
    return _np(ar, 'out', np.float64, (n_subsets, 3)), int(_np(ar, 'status', np.int32, (1,))[0])


# 1 x 1: the smallest plane (relu5_1 of a 16 x 16 image); 3 x 5: less than a wave; 16 x 16: exactly the 256 threads of the
# workgroup; 33 x 65: odd, 2145 elements, more than eight strides of the workgroup
@pytest.mark.parametrize('C', [1, 5, 64])
@pytest.mark.parametrize('plane', [(1, 1), (3, 5), (16, 16), (33, 65)], ids=lambda p: '%dx%d' % p)
def test_pool(plane, C):
    h, w = plane
    case = 'pool %dx%d C%d' % (h, w, C)
    B, C2, c0, row0 = 3, 2, 3, 2
    D, capacity = c0 + C + C2 + 1, row0 + B + 1
    a, b = fx.maps(h * w + C, B, C, h, w), fx.maps(h * w + C + 1, B, C2, 2 * h + 1, w)
    feat = call_pool([(a, c0), (b, c0 + C)], capacity, row0, D)
    fx.check_bound(case, 'slice0', feat[row0:row0 + B, c0:c0 + C], fx.pool(a), fx.pool_bound(a), ROWS, 'pool')
    fx.check_bound(case, 'slice1', feat[row0:row0 + B, c0 + C:c0 + C + C2], fx.pool(b), fx.pool_bound(b), ROWS, 'pool')
    rest = feat.view(np.uint32).copy()
    rest[row0:row0 + B, c0:c0 + C + C2] = 0xFFFFFFFF
    assert (rest == 0xFFFFFFFF).all()                                       # rows and columns outside the block keep their fill
    again = call_pool([(a, c0), (b, c0 + C)], capacity, row0, D)
    assert again.tobytes() == feat.tobytes()


def test_pool_refused_call_writes_nothing():
    lib = ah.raw_lib()
    x = fx.maps(1, 2, 4, 3, 5)
    ar = ah.Arena('cuda', {'x': ('in', torch.from_numpy(x)), 'feat': ('ws', 3 * 8 * 4)})
    for cap, row0, D, c0 in ((3, 2, 8, 0), (3, 0, 8, 5), (3, -1, 8, 0)):
        assert lib.him_feat_pool(ar.ptr('x'), 2, 4, 3, 5, ar.ptr('feat'), cap, row0, D, c0, _stream()) == ah.E_INVALID
    torch.cuda.synchronize()
    assert not ar.guard_failures() and bool((ar.t['feat'] == ah.NAN_BYTE).all())


# (1, 1): one row, one column; (5, 3): less than a tile both ways; (17, 70): n = 4 * 4 + 1, D = 4 * 16 + 6; (64, 64): whole
# tiles only; (130, 512): 32 x 32 tiles, the descriptor length of relu5_1; (37, 129): one column into a ninth tile
@pytest.mark.parametrize('n,D', [(1, 1), (5, 3), (17, 70), (64, 64), (130, 512), (37, 129)])
def test_moments(n, D):
    case = 'moments %dx%d' % (n, D)
    feat = fx.features(n + D, n + 3, D)                                     # three more rows behind the last one
    s, q = call_moments(feat, [(0, n)])
    (rs, rq), (bs, bq) = fx.moments(feat[:n]), fx.moments_bound(feat[:n])
    fx.check_bound(case, 'sum', s, rs, bs, ROWS, 'moments')
    fx.check_bound(case, 'second', q, rq, bq, ROWS, 'moments')
    assert q.tobytes() == np.ascontiguousarray(q.T).tobytes()                # the two triangles, bit for bit
    s2, q2 = call_moments(feat, [(0, n)])
    assert s2.tobytes() == s.tobytes() and q2.tobytes() == q.tobytes()
    if n > 1:                                                               # rows 1 .. n: row0 > 0 reads the right rows
        s1, q1 = call_moments(feat, [(1, n)])
        fx.check_bound(case, 'second row0=1', q1, fx.moments(feat[1:n + 1])[1], fx.moments_bound(feat[1:n + 1])[1], ROWS,
                       'moments')


def test_moments_streamed_in_two_calls():
    feat = fx.features(3, 37, 129)
    s, q = call_moments(feat, [(0, 17), (17, 20)])
    (rs, rq), (bs, bq) = fx.moments(feat), fx.moments_bound(feat)
    fx.check_bound('moments 17+20', 'sum', s, rs, bs, ROWS, 'moments')
    fx.check_bound('moments 17+20', 'second', q, rq, bq, ROWS, 'moments')
    assert q.tobytes() == np.ascontiguousarray(q.T).tobytes()


def test_moments_of_small_integers_are_exact():
    g = np.random.default_rng(5)
    feat = g.integers(-8, 9, (37, 70)).astype(np.float32)
    s, q = call_moments(feat, [(0, 20), (20, 17)])
    i = feat.astype(np.int64)
    fx.check_equal('moments int', 'sum', s, i.sum(0), ROWS, 'moments')
    fx.check_equal('moments int', 'second', q, i.T @ i, ROWS, 'moments')


def _tables(seed, nx, ny, n_subsets, m):
    return fx.subsets(seed, 0, nx, n_subsets, m), fx.subsets(seed, 1, ny, n_subsets, m)


# (2, 1, 1): the smallest call; (16, 4, 2): one accumulator, one k step of four; (37, 70, 3): a ragged tile, D = 4 * 16 + 6
# with D % 4 != 0 (the scalar loads); (64, 512, 2): one whole tile; (130, 96, 2): 3 x 3 tiles, off-diagonal ones doubled
@pytest.mark.parametrize('m,D,n_subsets', [(2, 1, 1), (16, 4, 2), (37, 70, 3), (64, 512, 2), (130, 96, 2)])
def test_kid_sums(m, D, n_subsets):
    case = 'kid m%d D%d' % (m, D)
    nx, ny = m + 3, m + 9
    x, y = fx.features(m + D, nx, D), fx.features(m + D + 1, ny, D, shift=0.3, scale=1.2)
    ix, iy = _tables(m, nx, ny, n_subsets, m)
    assert (m == 2 or not np.array_equal(ix[0], np.arange(m))) and (np.sort(ix, 1)[:, 1:] != np.sort(ix, 1)[:, :-1]).all()
    for gamma, coef0 in ((0.0, 1.0), (0.37, -0.5)):
        out, status = call_kid(x, y, ix, iy, gamma, coef0)
        assert status == 0
        ref, bound = fx.kid_sums(x, y, ix, iy, gamma, coef0), fx.kid_sums_bound(x, y, ix, iy, gamma, coef0)
        for k, name in enumerate(('xx', 'yy', 'xy')):
            fx.check_bound('%s g%g' % (case, gamma), name, out[:, k], ref[:, k], bound[:, k], ROWS, 'kid')
        again, _ = call_kid(x, y, ix, iy, gamma, coef0)
        assert again.tobytes() == out.tobytes()


@pytest.mark.parametrize('m,D,hi', [(2, 3, 5), (37, 6, 9), (130, 8, 12)])
def test_kid_sums_of_integers_are_exact(m, D, hi):
    nx, ny = m + 3, m + 9
    x, y = fx.int_rows(m, nx, D, hi), fx.int_rows(m + 1, ny, D, hi)
    ix, iy = _tables(m + 7, nx, ny, 2, m)
    out, status = call_kid(x, y, ix, iy, 1.0, 0.0)
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    want = np.empty((2, 3), np.int64)
    for s in range(2):
        X, Y = xi[ix[s]], yi[iy[s]]
        kxx, kyy, kxy = (X @ X.T) ** 3, (Y @ Y.T) ** 3, (X @ Y.T) ** 3
        want[s] = kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum()
        assert max(np.abs(kxx).sum(), np.abs(kyy).sum(), np.abs(kxy).sum()) < 2 ** 53
    assert status == 0
    fx.check_equal('kid int m%d' % m, 'sums', out, want, ROWS, 'kid')


def test_kid_bad_indices_flag_their_subsets_only():
    m, D, nx, ny = 37, 70, 40, 56
    x, y = fx.features(1, nx, D), fx.features(2, ny, D, shift=0.3)
    ix, iy = _tables(3, nx, ny, 4, m)
    clean, status = call_kid(x, y, ix, iy)
    assert status == 0
    bx, by = ix.copy(), iy.copy()
    bx[0, 5], by[2, 7] = nx, -1
    out, status = call_kid(x, y, bx, by)                                    # the arena's bands surround x and y
    assert status == fx.KID_BAD_INDEX
    assert np.isnan(out[0]).all() and np.isnan(out[2]).all()
    assert out[[1, 3]].tobytes() == clean[[1, 3]].tobytes()
    assert np.isnan(fx.kid_sums(x, y, bx, by)[[0, 2]]).all()
