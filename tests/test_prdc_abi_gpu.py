"""-m gpu: him_knn_radii and him_knn_membership at the C ABI inside tests/abi_harness.py's guarded arena, against the
float64 restatement of tests/prdc_fixture.py (definitions, reference and the derivation of every bound: its docstring).

Arena (tests/README.md): every buffer of a call is a view in ONE allocation between 64 KiB bands; NaN bands beside
inputs, 0xA5 bands beside outputs and workspace, compared bit for bit afterwards; outputs and workspace are pre-filled
with NaN bytes (the status word, which the entry ORs into, with 0); the workspace is exactly the queried size; inputs
are compared bit for bit after the call.

Checks, u = 2^-53: |r2_got - r2_ref| <= max_j e_ij with e_ab = (D + 8) u (|a|^2 + |b|^2 + 2 sum_k |a_k b_k|), and no radius
below 0; integer features give radii and counts EQUAL to the integer result; the real-valued cases (fixture.REAL_CASES)
have no uncertain decision, so their counts are compared for equality too (through the lower and upper counts).
Shapes: n in {k + 1, 15, 16, 17, 63, 64, 65, 130} and one n above each boundary of csrc/him_prdc.hip --
  KNN_TILE * KNN_CHUNK_TILES = 512 columns: 513 rows are the first to take two column chunks and the merge of two lists;
  KNN_TILE * KNN_CHUNK_TILES * KNN_MAX_CHUNKS = 8192: 8193 rows are the first whose chunks grow (nine tiles, fifteen chunks);
  KNN_TILE * KNN_MEMBER_SPLIT = 4096 reference rows: 4161 are 66 tiles, so that workgroups take a second tile;
  k = 4 | 5 and 8 | 9 change the length of the register list (4, 8, 16).
One JSON line per checked tensor goes to prdc_abi_rows.jsonl in the GPU tests' report directory before its assertion
runs."""
import os

import numpy as np
import pytest
import torch

import abi_harness as ah
import prdc_fixture as fx
from test_model_gpu import OUT as REPORT_DIR

pytestmark = pytest.mark.gpu

ROWS = fx.RowFile(os.path.join(REPORT_DIR, 'prdc_abi_rows.jsonl'))


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


def _np(ar, name, dtype, n):
    return ar.t[name].contiguous().view(torch.uint8).cpu().numpy().reshape(-1).view(dtype)[:n].copy()


def call_radii(x, k):
    """(radii2 (n,) float64, status)."""
    lib = ah.raw_lib()
    n, D = x.shape
    need = int(lib.him_knn_radii_ws(n, D, k))
    assert need > 0
    ar = ah.Arena('cuda', {'x': ('in', torch.from_numpy(x)), 'radii2': ('ws', n * 8),
                           'status': ('out', (1,), _as_floats(np.zeros(1, np.int32))), 'ws': ('ws', need)})
    rc = lib.him_knn_radii(ar.ptr('x'), n, D, k, ar.ptr('radii2'), ar.ptr('status'), ar.ptr('ws'), need, _stream())
    _finish(lib, ar, rc, {'x': x})
    return _np(ar, 'radii2', np.float64, n), int(_np(ar, 'status', np.int32, 1)[0])


def call_membership(q, r, radii2, want_rows=True, want_cols=True):
    """(row_count or None, col_count or None, status)."""
    lib = ah.raw_lib()
    (nq, D), nr = q.shape, r.shape[0]
    radii2 = np.ascontiguousarray(radii2, np.float64)
    need = int(lib.him_knn_membership_ws(nq, nr, D))
    assert need > 0
    specs = {'q': ('in', torch.from_numpy(q)), 'r': ('in', torch.from_numpy(r)), 'radii2': ('in', _as_floats(radii2))}
    if want_rows:
        specs['row_count'] = ('ws', nq * 4)
    if want_cols:
        specs['col_count'] = ('ws', nr * 4)
    specs.update(status=('out', (1,), _as_floats(np.zeros(1, np.int32))), ws=('ws', need))
    ar = ah.Arena('cuda', specs)
    rc = lib.him_knn_membership(ar.ptr('q'), nq, ar.ptr('r'), nr, D, ar.ptr('radii2'), ar.ptr('row_count'), ar.ptr('col_count'),
                                ar.ptr('status'), ar.ptr('ws'), need, _stream())
    _finish(lib, ar, rc, {'q': q, 'r': r, 'radii2': radii2})
    return (_np(ar, 'row_count', np.int32, nq) if want_rows else None, _np(ar, 'col_count', np.int32, nr) if want_cols else None,
            int(_np(ar, 'status', np.int32, 1)[0]))


def _check_real_radii(case, x, k):
    got, status = call_radii(x, k)
    assert status == 0
    fx.check_nonnegative(case, 'radii2 sign', got, ROWS)
    fx.check_bound(case, 'radii2', got, fx.radii(x, k), fx.radii_bound(x), ROWS)
    return got


def _check_int_radii(case, x, k):
    got, status = call_radii(x, k)
    assert status == 0
    fx.check_equal(case, 'radii2', got, fx.int_radii(x, k), ROWS)
    return got


# every D of {1, 3, 4, 5, 16, 67} and every k of {1, 3, 5, 16} at every n; k is clipped to n - 1
DK = ((1, 1), (3, 3), (4, 5), (5, 16), (16, 3), (67, 5))


@pytest.mark.parametrize('n', [0, 15, 16, 17, 63, 64, 65, 130], ids=lambda n: 'n%s' % (n or 'k+1'))
def test_radii_shapes(n):
    for D, k in DK:
        rows = n or k + 1
        kk = min(k, rows - 1)
        case = 'radii n%d D%d k%d' % (rows, D, kk)
        x = fx.features(rows * 131 + D, rows + 3, D)[:rows]
        got = _check_real_radii(case + ' real', np.ascontiguousarray(x), kk)
        again, _ = call_radii(np.ascontiguousarray(x), kk)
        assert again.tobytes() == got.tobytes()                                      # two identical calls, identical bytes
        _check_int_radii(case + ' lattice', fx.lattice(rows + D, rows, D, 3), kk)   # ties between distances, equal rows


@pytest.mark.parametrize('D', [1, 3, 4, 5, 16, 67])
@pytest.mark.parametrize('k', [1, 3, 4, 5, 8, 9, 16])
def test_radii_every_k_and_D_at_17_rows_and_distinct_norms(k, D):
    _check_real_radii('radii n17 D%d k%d real' % (D, k), fx.features(k * 100 + D, 17, D), k)
    if D >= 3:
        _check_int_radii('radii n17 D%d k%d norms' % (D, k), fx.distinct_norm_rows(k + D, 17, D, 9), k)


def test_radii_across_two_column_chunks():
    n = fx.TILE * fx.CHUNK_TILES + 1                                                 # 513
    _check_real_radii('radii n%d D5 k5 real' % n, fx.features(11, n, 5), 5)
    _check_int_radii('radii n%d D3 k16 lattice' % n, fx.lattice(12, n, 3, 6), 16)


def test_radii_where_the_chunks_grow():
    n = fx.TILE * fx.CHUNK_TILES * fx.MAX_CHUNKS + 1                                 # 8193
    _check_int_radii('radii n%d D3 k5 lattice' % n, fx.lattice(13, n, 3, 40), 5)


def test_radii_of_duplicate_rows_are_zero():
    x = fx.with_duplicates(fx.distinct_norm_rows(9, 20, 5, 4), 3)                    # integer rows, three copies each
    got = _check_int_radii('radii duplicates k2', x, 2)
    assert (got == 0).all()
    got = _check_int_radii('radii duplicates k3', x, 3)
    assert (got > 0).all()
    real = fx.with_duplicates(fx.features(8, 40, 67), 2)                             # real rows: a rounding error, never below 0
    got = _check_real_radii('radii real duplicates k1', real, 1)
    assert (fx.radii(real, 1) == 0).all() and (got >= 0).all()


@pytest.mark.parametrize('index', range(len(fx.REAL_CASES)))
def test_membership_real_cases(index):
    fake, real, k = fx.real_case(index)
    case = 'member %dx%d D%d k%d' % (len(fake), len(real), fake.shape[1], k)
    for tag, q, r in (('', fake, real), (' back', real, fake)):
        r2 = fx.radii(r, k)
        row_lo, row_hi, col_lo, col_hi, uncertain = fx.membership_bounds(q, r, r2)
        assert uncertain == 0
        rows, cols, status = call_membership(q, r, r2)
        assert status == 0
        fx.check_counts(case + tag, 'row_count', rows, row_lo, row_hi, ROWS)
        fx.check_counts(case + tag, 'col_count', cols, col_lo, col_hi, ROWS)
        again = call_membership(q, r, r2)
        assert again[0].tobytes() == rows.tobytes() and again[1].tobytes() == cols.tobytes()
        only_rows = call_membership(q, r, r2, want_cols=False)                       # either count pointer may be NULL
        only_cols = call_membership(q, r, r2, want_rows=False)
        assert only_rows[1] is None and only_rows[0].tobytes() == rows.tobytes()
        assert only_cols[0] is None and only_cols[1].tobytes() == cols.tobytes()


@pytest.mark.parametrize('nq,nr,D,k,hi', [(33, 70, 5, 3, 3), (70, 33, 3, 5, 2), (17, 16, 1, 1, 9), (65, 130, 4, 16, 2),
                                          (64, 64, 16, 5, 1), (6, 6, 67, 5, 1)])
def test_membership_of_integers_is_exact(nq, nr, D, k, hi):
    q, r = fx.lattice(nq + D, nq, D, hi), fx.lattice(nr + D + 1, nr, D, hi)
    r2 = fx.int_radii(r, k)
    rows, cols, status = call_membership(q, r, r2.astype(np.float64))
    want = fx.int_membership(q, r, r2)
    assert status == 0
    fx.check_equal('member int %dx%d D%d' % (nq, nr, D), 'row_count', rows, want[0], ROWS)
    fx.check_equal('member int %dx%d D%d' % (nq, nr, D), 'col_count', cols, want[1], ROWS)


def test_membership_where_workgroups_take_a_second_reference_tile():
    nq, nr = 33, fx.TILE * (fx.MEMBER_SPLIT + 2) - 63                               # 4161 rows: 66 tiles
    q, r = fx.lattice(21, nq, 3, 12), fx.lattice(22, nr, 3, 12)
    r2 = fx.int_radii(r, 5)
    rows, cols, status = call_membership(q, r, r2.astype(np.float64))
    want = fx.int_membership(q, r, r2)
    assert status == 0
    fx.check_equal('member int 33x%d' % nr, 'row_count', rows, want[0], ROWS)
    fx.check_equal('member int 33x%d' % nr, 'col_count', cols, want[1], ROWS)


def test_membership_of_duplicate_rows_counts_the_copies():
    x = fx.with_duplicates(fx.distinct_norm_rows(9, 20, 5, 4), 3)
    r2 = fx.int_radii(x, 2)
    assert (r2 == 0).all()                                                           # the radius is exactly 0: `<=` decides
    rows, cols, status = call_membership(x, x, r2.astype(np.float64))
    assert status == 0
    fx.check_equal('member duplicates', 'row_count', rows, np.full(60, 3), ROWS)
    fx.check_equal('member duplicates', 'col_count', cols, np.full(60, 3), ROWS)


def test_non_finite_rows_set_the_status_bit_and_leave_the_others_alone():
    x = fx.lattice(31, 70, 5, 6)
    bad = x.copy()
    bad[7, 2], bad[64, 0] = np.nan, np.inf                                           # one in each tile
    keep = np.ones(70, bool)
    keep[[7, 64]] = False
    clean, status = call_radii(x, 4)
    assert status == 0
    got, status = call_radii(bad, 4)
    assert status == fx.KNN_NONFINITE
    assert np.isnan(got[[7, 64]]).all()
    fx.check_equal('radii nonfinite', 'radii2', got, fx.radii(bad, 4), ROWS)
    fx.check_equal('radii nonfinite', 'radii2 of the others', got[keep], fx.int_radii(x[keep], 4), ROWS)
    real = fx.features(32, 70, 67)
    rbad = real.copy()
    rbad[3, 66], rbad[69, 1] = -np.inf, np.nan
    got, status = call_radii(rbad, 5)
    assert status == fx.KNN_NONFINITE
    fx.check_bound('radii nonfinite real', 'radii2', got, fx.radii(rbad, 5), fx.radii_bound(rbad), ROWS)
    # membership: a NaN row among the queries, an inf row among the references
    q, qbad = fx.lattice(33, 33, 5, 6), None
    qbad = q.copy()
    qbad[5, 4] = np.nan
    r2 = fx.radii(bad, 4)
    rows, cols, status = call_membership(qbad, bad, r2)
    assert status == fx.KNN_NONFINITE
    want = fx.membership(qbad, bad, r2)
    fx.check_equal('member nonfinite', 'row_count', rows, want[0], ROWS)
    fx.check_equal('member nonfinite', 'col_count', cols, want[1], ROWS)
    assert rows[5] == 0 and (cols[[7, 64]] == 0).all()
    ok_q = np.arange(33) != 5
    clean_rows, clean_cols = fx.int_membership(q[ok_q], x[keep], fx.int_radii(x[keep], 4))
    assert (rows[ok_q] == clean_rows).all() and (cols[keep] == clean_cols).all()


def test_refused_calls_write_nothing():
    lib = ah.raw_lib()
    x, q = fx.features(1, 40, 8), fx.features(2, 33, 8)
    n, D, k = 40, 8, 5
    need_r, need_m = int(lib.him_knn_radii_ws(n, D, k)), int(lib.him_knn_membership_ws(33, n, D))
    ar = ah.Arena('cuda', {'x': ('in', torch.from_numpy(x)), 'q': ('in', torch.from_numpy(q)),
                           'r2in': ('in', _as_floats(np.ones(n, np.float64))), 'radii2': ('ws', n * 8), 'row_count': ('ws', 33 * 4),
                           'col_count': ('ws', n * 4), 'status': ('ws', 4), 'ws': ('ws', max(need_r, need_m))})
    P = ar.ptr
    st = _stream()
    I, W = ah.E_INVALID, ah.E_WORKSPACE
    radii_calls = [((P('x'), n, D, 0), I), ((P('x'), n, D, fx.KNN_MAX_K + 1), I), ((P('x'), 5, D, 5), I), ((P('x'), 0, D, 1), I),
                   ((P('x'), 1 << 31, D, 1), I), ((P('x'), n, 0, k), I), ((P('x'), n, fx.FEAT_MAX_DIM + 1, k), I), ((0, n, D, k), I),
                   ((P('x') + 2, n, D, k), I)]
    for args, want in radii_calls:
        assert lib.him_knn_radii(*args, P('radii2'), P('status'), P('ws'), 1 << 40, st) == want, args
        assert b'knn_radii' in lib.him_last_error()
    for radii2, status, ws, nbytes, want in ((0, P('status'), P('ws'), need_r, I), (P('radii2'), 0, P('ws'), need_r, I),
                                             (P('radii2'), P('status'), 0, need_r, I), (P('radii2') + 4, P('status'), P('ws'), need_r, I),
                                             (P('radii2'), P('status'), P('ws'), need_r - 1, W), (P('radii2'), P('status'), P('ws'), 0, W)):
        assert lib.him_knn_radii(P('x'), n, D, k, radii2, status, ws, nbytes, st) == want
    good = [P('q'), 33, P('x'), n, D, P('r2in'), P('row_count'), P('col_count'), P('status'), P('ws'), need_m, st]
    for pos, value, want in ((1, 0, I), (3, 0, I), (1, 1 << 31, I), (4, 0, I), (4, fx.FEAT_MAX_DIM + 1, I), (0, 0, I), (2, 0, I),
                             (5, 0, I), (8, 0, I), (9, 0, I), (0, P('q') + 1, I), (5, P('r2in') + 4, I), (6, P('row_count') + 2, I),
                             (10, need_m - 1, W), (10, 0, W)):
        call = list(good)
        call[pos] = value
        assert lib.him_knn_membership(*call) == want, (pos, value)
        assert b'knn_membership' in lib.him_last_error()
    call = list(good)
    call[6] = call[7] = 0
    assert lib.him_knn_membership(*call) == I
    torch.cuda.synchronize()
    assert not ar.guard_failures()
    for name in ('radii2', 'row_count', 'col_count', 'status', 'ws'):
        assert bool((ar.t[name] == ah.NAN_BYTE).all()), name
