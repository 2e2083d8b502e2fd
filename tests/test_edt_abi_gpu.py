"""-m gpu: him_edt, him_boundary_stats and him_label_ids at the C ABI inside tests/abi_harness.py's guarded arena, against
the brute-force fixture of tests/edt_fixture.py.

Arena: every buffer of a call is a view in ONE allocation between 64 KiB bands; NaN bands beside src, jobs and the
incoming dist2, 0xA5 bands beside dist2, nearest, status, counts, sumd and the workspace, compared bit for bit
afterwards; outputs and workspace are pre-filled with NaN bytes; the workspace is exactly the queried size; the inputs
are compared with what went in.

Comparison: EQUALITY for dist2, nearest, status and counts, nothing excluded (fx.assert_edt_equal, fx.assert_stats_equal);
sumd within n_seed * 2^-52 relative of the float64 fixture (only the order of the additions differs).

Shapes are worded in the kernels' constants (csrc/him_edt.hip): the column pass works on tiles of TW = 64 columns x
TH = 32 rows and stages CH = 64 rows per step; the row pass scans STEP = 256 columns at a time with a carry; the
statistics pass gives SROWS = 16 rows to a workgroup."""
import numpy as np
import pytest
import torch

import abi_harness as ah
import edt_fixture as fx

pytestmark = pytest.mark.gpu

TW, TH, CH, STEP, SROWS = 64, 32, 64, 256, 16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _as_floats(raw):
    """Any bytes as the float32 tensor holding them (the arena's 'in' kind), padded with 0xFF to whole words."""
    raw = raw + b'\xff' * (-len(raw) % 4)
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy().view(np.float32))


def _plane_spec(src, shift):
    """src with ``shift`` elements of 0xFF in front: the 'in' spec and the byte offset of the plane."""
    raw = b'\xff' * (shift * src.itemsize) + np.ascontiguousarray(src).tobytes()
    return ('in', _as_floats(raw)), shift * src.itemsize, raw


def _same_bytes(view, raw):
    return bytes(view.contiguous().view(torch.uint8).cpu().numpy()[:len(raw)]) == raw


def call_edt(src, kind, jobs, want_nearest=True, shift=0):
    """One guarded him_edt call on src (B,H,W) of fx.NP_OF[kind]; returns (dist2, nearest or None, status)."""
    lib = ah.raw_lib()
    src = np.ascontiguousarray(src.astype(fx.NP_OF[kind]))
    jobs = np.ascontiguousarray(np.asarray(jobs, np.int32).reshape(-1, 3))
    B, H, W = src.shape
    K = len(jobs)
    need = int(lib.him_edt_workspace(K, H, W))
    assert need >= K * H * W * 2
    spec, off, raw = _plane_spec(src, shift)
    specs = {'src': spec, 'jobs': ('in', _as_floats(jobs.tobytes())), 'dist2': ('ws', K * H * W * 4)}
    if want_nearest:
        specs['nearest'] = ('ws', K * H * W * 4)
    specs.update(status=('ws', K * 8), ws=('ws', need))
    ar = ah.Arena('cuda', specs)
    rc = lib.him_edt(ar.ptr('src') + off, kind, B, H, W, ar.ptr('jobs'), K, ar.ptr('dist2'), ar.ptr('nearest'),
                     ar.ptr('status'), ar.ptr('ws'), need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.him_last_error()
    bad = ar.guard_failures()
    assert not bad, '; '.join(bad)
    assert _same_bytes(ar.t['src'], raw) and _same_bytes(ar.t['jobs'], jobs.tobytes())       # inputs are never written
    dist2 = ar.t['dist2'].cpu().numpy().view(np.int32).reshape(K, H, W).copy()
    nearest = ar.t['nearest'].cpu().numpy().view(np.int32).reshape(K, H, W).copy() if want_nearest else None
    status = ar.t['status'].cpu().numpy().view(np.int32).reshape(K, 2).copy()
    return dist2, nearest, status


def call_stats(src, kind, jobs, dist2, tol2, shift=0):
    """One guarded him_boundary_stats call; returns (counts (K,4) int64, sumd (K,) float64)."""
    lib = ah.raw_lib()
    src = np.ascontiguousarray(src.astype(fx.NP_OF[kind]))
    jobs = np.ascontiguousarray(np.asarray(jobs, np.int32).reshape(-1, 3))
    dist2 = np.ascontiguousarray(dist2.astype(np.int32))
    B, H, W = src.shape
    K = len(jobs)
    need = int(lib.him_boundary_stats_workspace(K, H, W))
    assert need > 0
    spec, off, raw = _plane_spec(src, shift)
    specs = {'src': spec, 'jobs': ('in', _as_floats(jobs.tobytes())), 'dist2': ('in', _as_floats(dist2.tobytes())),
             'counts': ('ws', K * 32), 'sumd': ('ws', K * 8), 'ws': ('ws', need)}
    ar = ah.Arena('cuda', specs)
    rc = lib.him_boundary_stats(ar.ptr('src') + off, kind, B, H, W, ar.ptr('jobs'), K, ar.ptr('dist2'), tol2,
                                ar.ptr('counts'), ar.ptr('sumd'), ar.ptr('ws'), need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.him_last_error()
    bad = ar.guard_failures()
    assert not bad, '; '.join(bad)
    assert _same_bytes(ar.t['src'], raw) and _same_bytes(ar.t['dist2'], dist2.tobytes())
    counts = ar.t['counts'].cpu().numpy().view(np.int64).reshape(K, 4).copy()
    sumd = ar.t['sumd'].cpu().numpy().view(np.float64).copy()
    return counts, sumd


def check_edt(src, kind, jobs, what, **kw):
    got = call_edt(src, kind, jobs, **kw)
    fx.assert_edt_equal(got, fx.edt_jobs(np.asarray(src), jobs), what)
    return got


def sparse(seed, H, W, p=0.02):
    g = np.random.default_rng(seed)
    return (g.random((1, H, W)) < p).astype(np.int64) * g.integers(1, 200, size=(1, H, W))


NZ = [[0, 0, fx.NONZERO]]
# 1x1, one row, one column; one below / at / one above a tile edge in both directions; a plane taller than one staged
# chunk (CH + TH + 5 rows: the sweep walks up and down over chunk borders) and one of three chunks; rows wider than one
# scan step (the carry between steps); widths that are no multiple of 4
SHAPES = [(1, 1), (1, 70), (70, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (TH - 1, TW + 1), (TH + 1, TW - 1),
          (CH + TH + 5, 21), (2 * CH + 2, 19), (5, STEP + 3), (3, 2 * STEP + 1), (2, STEP)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_sparse_seeds_no_seed_all_seeds_and_a_corner_seed(shape):
    H, W = shape
    src = sparse(H * 1000 + W, H, W, 0.03)
    check_edt(src, 1, NZ, 'sparse')
    check_edt(src, 0, NZ, 'sparse, shifted base', shift=1)
    got = check_edt(np.zeros((1, H, W), np.int64), 1, NZ, 'no seed')
    assert (got[0] == fx.NONE).all() and (got[1] == -1).all() and got[2].tolist() == [[0, 0]]
    got = check_edt(np.ones((1, H, W), np.int64), 1, NZ, 'all seeds')
    assert not got[0].any() and np.array_equal(got[1].reshape(-1), np.arange(H * W)) and got[2][0, 0] == H * W
    for cy, cx in ((0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0)):
        one = np.zeros((1, H, W), np.int64)
        one[0, cy, cx] = 9
        got = check_edt(one, 2, NZ, 'corner seed')
        far = got[0][0, H - 1 - cy, W - 1 - cx]
        assert far == (H - 1) ** 2 + (W - 1) ** 2 == got[0].max()                 # a full diagonal away


def test_seeds_only_in_another_tile_than_the_outputs():
    H, W = 2 * CH + TH + 3, 2 * TW + 5                      # 3 x 3 column-pass tiles and more, three staged chunks
    for ys, xs in ((slice(0, 3), slice(0, 3)), (slice(H - 2, H), slice(W - 4, W)), (slice(CH, CH + 2), slice(TW, TW + 2)),
                   (slice(0, 1), slice(W - 1, W))):
        src = np.zeros((1, H, W), np.int64)
        src[0, ys, xs] = 1
        got = call_edt(src, 1, NZ)
        # too large for the pair matrix: the few seeds are listed, every pixel is compared
        sy, sx = np.nonzero(src[0])
        py, px = np.mgrid[0:H, 0:W]
        d2 = (py[..., None] - sy) ** 2 + (px[..., None] - sx) ** 2
        idx = sy * W + sx
        pick = np.argmin(d2 * (H * W) + idx, axis=-1)
        fx.assert_edt_equal(got, (np.take_along_axis(d2, pick[..., None], -1)[None, ..., 0].astype(np.int32),
                                  idx[pick][None].astype(np.int32), np.array([[len(sy), 0]], np.int32)), 'far tile')


def test_tie_rule_left_then_up():
    # two seeds at equal distance left / right and up / down of whole rows and columns; four corners around a centre
    for H, W, pts in ((3, 5, [(1, 1), (1, 3)]), (5, 3, [(1, 1), (3, 1)]), (5, 5, [(0, 0), (0, 4), (4, 0), (4, 4)]),
                      (TH + 7, TW + 9, [(TH - 3, TW - 4), (TH - 3, TW + 4), (TH + 5, TW - 4), (TH + 5, TW + 4)]),
                      (2 * CH + 1, 3, [(CH - 1 - 40, 1), (CH - 1 + 40, 1)]),        # the tie crosses a chunk border
                      (2, 2 * STEP + 1, [(0, STEP - 200), (0, STEP + 200)])):       # ... and a scan-step border
        src = np.zeros((1, H, W), np.int64)
        for y, x in pts:
            src[0, y, x] = 1
        got = check_edt(src, 1, NZ, 'tie %dx%d' % (H, W))
        cy, cx = (pts[0][0] + pts[-1][0]) // 2, (pts[0][1] + pts[-1][1]) // 2
        assert got[1][0, cy, cx] == pts[0][0] * W + pts[0][1]                      # the smallest y', then the smallest x'


@pytest.mark.parametrize('kind', [0, 1, 2, 3])
def test_all_rules_and_kinds_several_jobs_per_plane_and_bad_jobs_between_good_ones(kind):
    H, W = TH + 1, TW + 1
    src = fx.blocky(40 + kind, 2, H, W, (0, 1, 2, 5), cell=6, salt=0.03)
    if kind != 0:
        src[1][src[1] == 5] = 300                            # an id above a byte
    jobs = [[0, 0, fx.NONZERO], [0, 1, fx.EQUALS], [0, 1, fx.BOUNDARY_OF], [0, 0, fx.ANY_BOUNDARY],
            [2, 1, fx.BOUNDARY_OF],                          # plane outside 0..B-1
            [1, 2, fx.BOUNDARY_OF], [1, 300, fx.EQUALS], [1, 0, 4],                 # ... an unknown rule
            [-1, 0, fx.NONZERO], [1, 5, fx.BOUNDARY_OF], [1, 77, fx.BOUNDARY_OF],   # a class that is absent
            [0, 2, fx.BOUNDARY_OF], [1, 0, -1], [1, 0, fx.ANY_BOUNDARY]]
    got = check_edt(src, kind, jobs, 'kind %d' % kind, shift=1 if kind == 0 else 0)
    assert got[2][:, 1].tolist() == [0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0]
    for k in (4, 7, 8, 10, 12):
        assert (got[0][k] == fx.NONE).all() and (got[1][k] == -1).all() and got[2][k, 0] == 0
    again = call_edt(src, kind, jobs, shift=1 if kind == 0 else 0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))            # two runs: identical bits
    plain = call_edt(src, kind, jobs, want_nearest=False)
    assert plain[1] is None and plain[0].tobytes() == got[0].tobytes()             # nearest = NULL changes nothing else


def test_boundary_of_a_class_touching_the_image_border():
    H, W = TH + 3, TW + 2
    src = np.zeros((1, H, W), np.int64)
    src[0, :, :20] = 1                                       # class 1 fills the left part: three sides on the border
    got = check_edt(src, 1, [[0, 1, fx.BOUNDARY_OF], [0, 0, fx.BOUNDARY_OF], [0, 0, fx.ANY_BOUNDARY]], 'border')
    assert got[2][:, 0].tolist() == [H, H, 2 * H]            # one column each, not the frame
    assert np.array_equal(got[0][0], np.broadcast_to((np.arange(W) - 19) ** 2, (H, W)))
    full = np.full((1, H, W), 3, np.int64)                   # a class covering the plane has no boundary at all
    got = check_edt(full, 1, [[0, 3, fx.BOUNDARY_OF], [0, 0, fx.ANY_BOUNDARY]], 'full')
    assert (got[0] == fx.NONE).all() and got[2].tolist() == [[0, 0], [0, 0]]


@pytest.mark.parametrize('kind', [0, 1, 2, 3])
def test_boundary_stats_equal_the_fixture(kind):
    H, W = 2 * SROWS + 5, TW + 6                             # three statistics slots per job, the last one ragged
    pred, gt = fx.layout_pair(seed=20 + kind, B=2, H=H, W=W)
    jobs = np.concatenate([fx.class_jobs(2, [0, 1, 2, 3, 4]), [[5, 1, fx.BOUNDARY_OF], [1, 0, fx.ANY_BOUNDARY],
                                                               [0, 0, fx.NONZERO], [0, 2, fx.EQUALS], [0, 1, 9]]])
    d_gt = fx.edt_jobs(gt, jobs)[0]
    got_d = call_edt(gt, kind, jobs, want_nearest=False)[0]
    assert np.array_equal(got_d, d_gt)
    for tol2 in (0, 4, 5, 10 ** 6):
        want = fx.boundary_stats(pred, jobs, d_gt, tol2)
        got = call_stats(pred, kind, jobs, got_d, tol2, shift=1 if kind == 0 else 0)
        fx.assert_stats_equal(got[0], got[1], want[0], want[1], 'kind %d tol2 %d' % (kind, tol2))
    assert (want[0][:, 3] > 0).any() and (want[0][:, 0] == 0).any()                # unreachable seeds; jobs without seeds
    hit4, hit5 = fx.boundary_stats(pred, jobs, d_gt, 4)[0][:, 1], fx.boundary_stats(pred, jobs, d_gt, 5)[0][:, 1]
    assert (hit5 > hit4).any()                                # seeds exactly at d2 = 5: <= is exercised
    again = call_stats(pred, kind, jobs, got_d, 4)
    first = call_stats(pred, kind, jobs, got_d, 4)
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()


def test_boundary_stats_shapes():
    for H, W in ((1, 1), (1, 70), (70, 1), (SROWS, STEP), (SROWS + 1, STEP + 1), (SROWS - 1, STEP - 1)):
        src = fx.blocky(H + W, 1, H, W, (0, 1), cell=3)
        other = np.roll(src, 1, 2)
        jobs = [[0, 1, fx.BOUNDARY_OF], [0, 0, fx.ANY_BOUNDARY], [0, 1, fx.EQUALS]]
        d = fx.edt_jobs(other, jobs)[0]
        want = fx.boundary_stats(src, jobs, d, 1)
        got = call_stats(src, 2, jobs, d, 1)
        fx.assert_stats_equal(got[0], got[1], want[0], want[1], '%dx%d' % (H, W))


def test_label_ids_take_the_rules_of_the_confusion_matrix():
    lib = ah.raw_lib()
    ids = fx.blocky(3, 2, 19, 27, (0, 1, 2, 3, 4), cell=3)
    scores = fx.scores_of(ids, 6, 8)
    half = np.nextafter(np.float32(0.5), np.float32(1))
    prob = np.array([0.2, 0.5, 0.8, half], np.float32)[np.random.default_rng(2).integers(0, 4, size=(2, 1, 19, 27))]
    for src, pk, C in ((scores, 4, 6), (prob, 5, 1), (scores[:, :1], 4, 1)):
        ar = ah.Arena('cuda', {'src': ('in', torch.from_numpy(src.copy())), 'ids': ('ws', 2 * 19 * 27 * 4)})
        rc = lib.him_label_ids(ar.ptr('src'), pk, 2, C, 19, 27, ar.ptr('ids'), _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.him_last_error()
        assert not ar.guard_failures() and torch.equal(ar.t['src'].cpu(), torch.from_numpy(src))
        got = ar.t['ids'].cpu().numpy().view(np.int32).reshape(2, 19, 27)
        want = fx.label_ids(src, 'prob') if pk == 5 else (fx.label_ids(src) if C > 1 else np.zeros((2, 19, 27), np.int32))
        assert np.array_equal(got, want), pk
