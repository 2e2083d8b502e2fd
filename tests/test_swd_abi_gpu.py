"""-m gpu: him_lap_pyramid, him_swd_gather, him_swd_project, him_sort_segments and him_swd_distance at the C ABI inside
tests/abi_harness.py's guarded arena, against the numpy restatement of tests/swd_fixture.py.

Arena (tests/README.md): every buffer of a call is a view in ONE allocation between 64 KiB bands; NaN bands beside
inputs, 0xA5 bands beside outputs and workspace, compared bit for bit afterwards; fresh outputs and workspace are
pre-filled with NaN bytes; the workspace is exactly the queried size; inputs are compared bit for bit after the call.

Bounds, no fixed tolerance: pyramid levels and projections max|err| / max|ref64| <= max(8 e32, 16 2^-24) with e32 the
fixture's own fp32 twin; gathered rows EQUAL an index of the kernel's own pyramid output; channel sums against
math.fsum within count 2^-53 sum|x|; sorted keys bit for bit the fixture's key-sort of the kernel's input; NaN and clamp
counts equal; per-direction distance sums against float64 of the kernel's own sorted arrays within N 2^-53 sum.
Nothing is excluded.  One JSON line per checked tensor goes to swd_abi_rows.jsonl in the GPU tests' report directory
before its assertion runs."""
import os

import numpy as np
import pytest
import torch

import abi_harness as ah
import swd_fixture as fx
from test_model_gpu import OUT as REPORT_DIR

pytestmark = pytest.mark.gpu

ROWS = fx.RowFile(os.path.join(REPORT_DIR, 'swd_abi_rows.jsonl'))
LDS = fx.LDS_MAX


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _as_floats(arr):
    raw = np.ascontiguousarray(arr).tobytes()
    raw = raw + b'\xff' * (-len(raw) % 4)
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


def call_pyramid(x, levels, expect=0):
    lib = ah.raw_lib()
    B, C, H, W = x.shape
    off = [int(lib.him_lap_level_offset(B, C, H, W, l)) for l in range(levels + 1)]
    need = int(lib.him_lap_pyramid_ws(B, C, H, W, levels))
    ar = ah.Arena('cuda', {'x': ('in', torch.from_numpy(x)), 'lap': ('ws', max(off[-1], 1) * 4),
                           'gauss': ('ws', max(off[-1] - off[1], 4) * 4), 'ws': ('ws', max(need, 16))})
    rc = lib.him_lap_pyramid(ar.ptr('x'), B, C, H, W, levels, ar.ptr('lap'), ar.ptr('gauss'), ar.ptr('ws'), need, _stream())
    if expect:
        torch.cuda.synchronize()
        assert rc == expect and need == 0, (rc, need)
        assert not ar.guard_failures()
        for name in ('lap', 'gauss', 'ws'):                                   # a refused call writes nothing
            assert bool((ar.t[name] == ah.NAN_BYTE).all()), name
        return None
    _finish(lib, ar, rc, {'x': x})
    lap = _np(ar, 'lap', np.float32, (off[-1],))
    gauss = _np(ar, 'gauss', np.float32, (max(off[-1] - off[1], 0),))
    laps = [lap[off[l]:off[l + 1]].reshape(B, C, H >> l, W >> l) for l in range(levels)]
    gs = [gauss[off[l] - off[1]:off[l + 1] - off[1]].reshape(B, C, H >> l, W >> l) for l in range(1, levels)]
    return laps, gs


def call_gather(level, pos, capacity, row0, stats, clamped=0):
    lib = ah.raw_lib()
    B, C, h, w = level.shape
    n, K = pos.shape[1], 49 * C
    need = int(lib.him_swd_gather_ws(B, C))
    st_in, status_in = np.ascontiguousarray(stats, np.float64), np.array([clamped], np.int32)
    ar = ah.Arena('cuda', {'level': ('in', torch.from_numpy(level)), 'pos': ('in', _as_floats(pos)),
                           'desc': ('ws', capacity * K * 4), 'stats': ('out', (C * 8,), _as_floats(st_in)),
                           'status': ('out', (1,), _as_floats(status_in)), 'ws': ('ws', need)})
    rc = lib.him_swd_gather(ar.ptr('level'), B, C, h, w, ar.ptr('pos'), n, ar.ptr('desc'), capacity, row0, ar.ptr('stats'),
                            ar.ptr('status'), ar.ptr('ws'), need, _stream())
    _finish(lib, ar, rc, {'level': level, 'pos': pos})
    return (_np(ar, 'desc', np.float32, (capacity, K)), _np(ar, 'stats', np.float64, (C, 4)),
            int(_np(ar, 'status', np.int32, (1,))[0]))


def call_project(desc, C, stats, dirs):
    lib = ah.raw_lib()
    N, n_dirs = desc.shape[0], dirs.shape[1]
    zero = np.zeros(1, np.int32)
    ar = ah.Arena('cuda', {'desc': ('in', torch.from_numpy(desc)), 'stats': ('in', _as_floats(stats)),
                           'dirs': ('in', torch.from_numpy(dirs)), 'out': ('ws', n_dirs * N * 4),
                           'status': ('out', (1,), _as_floats(zero))})
    rc = lib.him_swd_project(ar.ptr('desc'), N, C, ar.ptr('stats'), ar.ptr('dirs'), n_dirs, ar.ptr('out'), ar.ptr('status'),
                             _stream())
    _finish(lib, ar, rc, {'desc': desc, 'stats': stats, 'dirs': dirs})
    return _np(ar, 'out', np.float32, (n_dirs, N)), int(_np(ar, 'status', np.int32, (1,))[0])


def call_sort(x):
    lib = ah.raw_lib()
    S, N = x.shape
    need = int(lib.him_sort_segments_ws(S, N))
    assert need >= (16 if N <= LDS else S * N * 4)
    ar = ah.Arena('cuda', {'keys': ('out', (S, N), torch.from_numpy(x)), 'status': ('ws', 4), 'ws': ('ws', need)})
    assert _bytes_of(ar.t['keys'], x.nbytes) == x.tobytes()                    # the upload kept every NaN payload
    rc = lib.him_sort_segments(ar.ptr('keys'), S, N, ar.ptr('status'), ar.ptr('ws'), need, _stream())
    _finish(lib, ar, rc, {})
    return _np(ar, 'keys', np.float32, (S, N)), int(_np(ar, 'status', np.int32, (1,))[0])


def call_distance(a, b):
    lib = ah.raw_lib()
    n_dirs, N = a.shape
    ar = ah.Arena('cuda', {'a': ('in', torch.from_numpy(a)), 'b': ('in', torch.from_numpy(b)), 'sums': ('ws', n_dirs * 8),
                           'mean': ('ws', 8)})
    rc = lib.him_swd_distance(ar.ptr('a'), N, ar.ptr('b'), N, n_dirs, ar.ptr('sums'), ar.ptr('mean'), _stream())
    _finish(lib, ar, rc, {'a': a, 'b': b})
    return _np(ar, 'sums', np.float64, (n_dirs,)), float(_np(ar, 'mean', np.float64, (1,))[0])


def border_positions(seed, B, n, h, w):
    """Random corners with, per image, the four extreme corners and four corners outside the plane (to be clamped)."""
    pos = fx.positions(seed, 0, B, n, h, w)
    fixed = [(0, 0), (0, w - 7), (h - 7, 0), (h - 7, w - 7), (-3, 2), (2, w - 6), (h, w + 5), (-2 ** 31, 2 ** 31 - 1)]
    pos[:, :len(fixed)] = np.array(fixed[:n], np.int64).astype(np.int32)
    return pos


# 1 x 1 x 16 x 16: one level, 16 x 16 leaves patches reaching all four borders; 2 x 3 x 32 x 64: two levels, one tile wide;
# 3 x 3 x 48 x 80: two levels, 80 and 40 columns are no multiple of the 64-column tile, 48 and 24 rows give ragged halves
SHAPES = [(1, 1, 16, 16), (2, 3, 32, 64), (3, 3, 48, 80)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pyramid_gather_and_channel_sums(shape):
    B, C, H, W = shape
    case = 'x'.join(map(str, shape))
    x = fx.images(sum(shape), *shape)
    L = fx.n_levels(H, W)
    assert L == int(ah.raw_lib().him_lap_levels(H, W, 0)) == (1 if H == 16 else 2)
    laps, gs = call_pyramid(x, L)
    (l64, g64), (l32, g32) = fx.pyramid(x), fx.pyramid(x, dtype=np.float32)
    for l in range(L):
        fx.check_direct(case, 'lap%d' % l, laps[l], l64[l], l32[l], ROWS)
    for l in range(1, L):
        fx.check_direct(case, 'gauss%d' % l, gs[l - 1], g64[l], g32[l], ROWS)
    again = call_pyramid(x, L)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(laps + gs, again[0] + again[1]))
    n = 12
    for l, lv in enumerate(laps):
        h, w = lv.shape[-2:]
        pos = border_positions(l + 5, B, n, h, w)
        want, moved = fx.gather(lv, pos)                                         # an index of the kernel's own output
        assert moved == 4 * B
        cap, row0 = B * n + 5, 3
        stats0 = np.array([[0.0, 0.0, np.inf, -np.inf]] * C)
        desc, stats, clamped = call_gather(lv, pos, cap, row0, stats0, clamped=7)
        assert torch.equal(torch.from_numpy(desc[row0:row0 + B * n]), torch.from_numpy(want))
        rest = np.concatenate([desc[:row0], desc[row0 + B * n:]]).view(np.uint32)
        assert (rest == 0xFFFFFFFF).all()                                         # rows outside the batch stay as they were
        assert clamped == 7 + moved
        d = want.astype(np.float64).reshape(-1, C, 49)
        for c in range(C):
            fx.check_sum(case, 'L%d sum c%d' % (l, c), stats[c, 0], d[:, c], ROWS)
            fx.check_sum(case, 'L%d sum2 c%d' % (l, c), stats[c, 1], d[:, c] ** 2, ROWS)
            assert stats[c, 2] == d[:, c].min() and stats[c, 3] == d[:, c].max()
        d2, s2, c2 = call_gather(lv, pos, cap, row0, stats0, clamped=7)
        assert d2.tobytes() == desc.tobytes() and s2.tobytes() == stats.tobytes() and c2 == clamped
        if B > 1:                                                                 # streamed in two calls: the same bits
            da, sa, ca = call_gather(lv[:1], pos[:1], cap, row0, stats0, clamped=7)
            db, sb, cb = call_gather(lv[1:], pos[1:], cap, row0 + n, sa, clamped=ca)
            assert sb.tobytes() == stats.tobytes() and cb == clamped
            assert np.array_equal(da[row0:row0 + n], want[:n]) and np.array_equal(db[row0 + n:row0 + B * n], want[n:])


def test_pyramid_refuses_sizes_its_levels_do_not_divide():
    call_pyramid(fx.images(1, 3, 3, 40, 72), 4, expect=ah.E_INVALID)


@pytest.mark.parametrize('C,N,n_dirs', [(1, 12, 5), (3, 150, 70), (3, 64, 64), (1, 129, 130)])
def test_projection(C, N, n_dirs):
    case = 'proj C%d N%d D%d' % (C, N, n_dirs)
    g = np.random.default_rng(N)
    desc = (g.standard_normal((N, 49 * C)) * 0.3 + np.repeat([0.7, -0.2, 0.1][:C], 49)).astype(np.float32)
    dirs = fx.directions(N, C, n_dirs)
    d = desc.astype(np.float64).reshape(N, C, 49)
    stats = np.stack([d.sum((0, 2)), (d * d).sum((0, 2)), d.min((0, 2)), d.max((0, 2))], 1)
    out, status = call_project(desc, C, stats, dirs)
    assert status == 0
    fx.check_direct(case, 'out', out, fx.project(desc, C, dirs), fx.project(desc, C, dirs, np.float32), ROWS)
    again, _ = call_project(desc, C, stats, dirs)
    assert again.tobytes() == out.tobytes()
    flat = desc.copy()
    flat[:, (C - 1) * 49:] = np.float32(0.3)                                      # the last channel does not vary
    d = flat.astype(np.float64).reshape(N, C, 49)
    stats = np.stack([d.sum((0, 2)), (d * d).sum((0, 2)), d.min((0, 2)), d.max((0, 2))], 1)
    out, status = call_project(flat, C, stats, dirs)
    assert status == fx.ZERO_DEVIATION and np.isnan(out).all() and np.isnan(fx.project(flat, C, dirs)).all()


# below, at and above a wave, the 256 threads of a workgroup and a power of two; both sides of the switch from the LDS sort
# to the merge path (one pass, buffers swapped an odd number of times); three chunks (two passes, a run without a partner)
SORT_N = [1, 2, 63, 64, 65, 255, 256, 257, 4097, LDS, LDS + 1]
SORT_CASES = [(S, N) for N in SORT_N for S in (1, 3, 128)] + [(3, 3 * LDS + 5), (3, 70001)]


@pytest.mark.parametrize('S,N', SORT_CASES, ids=lambda v: str(v))
def test_sort_segments(S, N):
    first = None
    for i, kind in enumerate(fx.SORT_KINDS):
        x = fx.sort_input(kind, 100 * i + S + N, S, N)
        got, nans = call_sort(x)
        fx.check_sorted_bits('sort %s %dx%d' % (kind, S, N), got, x, nans, ROWS)
        if kind == 'nans':
            first = (x, got, nans)
    again, nans = call_sort(first[0])
    assert again.tobytes() == first[1].tobytes() and nans == first[2]


def test_distance_sums():
    for n_dirs, N in ((5, 1), (7, 300), (3, 1000)):
        g = np.random.default_rng(N)
        a = call_sort(g.standard_normal((n_dirs, N)).astype(np.float32))[0]
        b = call_sort((g.standard_normal((n_dirs, N)) * 1.5 + 0.2).astype(np.float32))[0]
        sums, mean = call_distance(a, b)
        terms = np.abs(a.astype(np.float64) - b.astype(np.float64))
        for d in range(n_dirs):
            fx.check_sum('dist %dx%d' % (n_dirs, N), 'dir%d' % d, sums[d], terms[d], ROWS)
        fx.check_sum('dist %dx%d' % (n_dirs, N), 'mean', mean * (n_dirs * N), terms, ROWS)
        again = call_distance(a, b)
        assert again[0].tobytes() == sums.tobytes() and again[1] == mean
    lib = ah.raw_lib()
    assert lib.him_swd_distance(1 << 20, 10, 1 << 20, 11, 4, 1 << 20, 1 << 20, 0) == ah.E_INVALID     # unequal N: no launch
