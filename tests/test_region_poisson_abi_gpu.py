"""-m gpu: him_region_poisson_solve and him_region_poisson_apply at the C ABI inside tests/abi_harness.py's guarded arena,
against tests/region_poisson_fixture.py, both modes, rtol 1e-10.

Arena: every buffer of a call is a view in ONE allocation between 64 KiB bands; NaN bands beside the inputs, 0xA5 bands
beside outputs and workspace, compared bit for bit afterwards; u, status, resid and the workspace are pre-filled with NaN
bytes; the inputs are compared with what went in; a refused call writes nothing.

Bounds: region_poisson_fixture.compare (all derived): the error of u under ||r_true|| / lam_min, ||r_true|| under
rtol ||b|| plus the recursive residual's drift, the canvas one fp32 rounding more, bit for bit outside Omega.  One JSON
line per bounded quantity goes to region_poisson_abi_rows.jsonl in the GPU tests' report directory before anything is
asserted.

Shapes are worded in the kernel's tile (csrc/him_region_poisson.hip): 64 columns x 4 rows per workgroup."""
import json
import os

import numpy as np
import pytest
import torch

import abi_harness as ah
import region_poisson_fixture as fx
from test_model_gpu import OUT as REPORT_DIR

pytestmark = pytest.mark.gpu

OUT = os.path.join(REPORT_DIR, 'region_poisson_abi_rows.jsonl')
E_INVALID, E_WORKSPACE = ah.E_INVALID, ah.E_WORKSPACE
RTOL = 1e-10


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report(rows):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'a') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')
            print(json.dumps(r))


def _as_floats(a):
    """Any array's bytes, padded to whole words, as the float32 tensor holding them (the arena's 'in' kind)."""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.pad(b, (0, -b.size % 4)).copy().view(np.float32))


def _check(lib, ar, specs, rc, expect):
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.him_last_error())
    bad = ar.guard_failures()
    assert not bad, '; '.join(bad)
    for k, s in specs.items():
        if s[0] == 'in':
            assert torch.equal(ah.bits(ar.t[k]), ah.bits(s[1])), 'input %s was written' % k
    if expect != 0:
        ah.untouched(ar, specs)


def call_solve(O, P, x0, y0, R, mixed, rtol=RTOL, max_iter=None, expect=0, null=None, misalign=None, short_ws=0, **over):
    """One guarded him_region_poisson_solve -> (u (3,H,W) float64, status (8,) int32, resid (3,) float64)."""
    lib = ah.raw_lib()
    Hc, Wc = O.shape[1:]
    H, W = P.shape[1:]
    nws = int(lib.him_region_poisson_ws(H, W))
    specs = {'canvas': ('in', torch.from_numpy(O.copy())), 'P': ('in', torch.from_numpy(P.copy())),
             'region': ('in', _as_floats(np.ascontiguousarray(R, np.uint8))), 'u': ('ws', 8 * 3 * H * W),
             'status': ('ws', 32), 'resid': ('ws', 24), 'ws': ('ws', nws + 8)}
    ar = ah.Arena('cuda', specs)
    ptr = lambda k: 0 if k == null else ar.ptr(k) + (4 if k == misalign else 0)      # noqa: E731
    a = dict(dict(Hc=Hc, Wc=Wc, x0=x0, y0=y0, H=H, W=W, mixed=int(mixed), rtol=rtol,
                  max_iter=fx.default_cap(H, W) if max_iter is None else max_iter), **over)
    rc = lib.him_region_poisson_solve(ptr('canvas'), a['Hc'], a['Wc'], a['x0'], a['y0'], a['H'], a['W'], ptr('P'),
                                      ptr('region'), a['mixed'], a['rtol'], a['max_iter'], ptr('u'), ptr('status'),
                                      ptr('resid'), ptr('ws'), nws - short_ws, _stream())
    _check(lib, ar, specs, rc, expect)
    if expect != 0:
        return None, None, None
    host = lambda k, dt, n: ar.t[k].cpu().numpy()[:n * np.dtype(dt).itemsize].view(dt).copy()     # noqa: E731
    return host('u', np.float64, 3 * H * W).reshape(3, H, W), host('status', np.int32, 8), host('resid', np.float64, 3)


def call_apply(P, u, R, O, x0, y0, expect=0, null=None, misalign=None, **over):
    """One guarded him_region_poisson_apply -> the canvas (3,Hc,Wc) float32."""
    lib = ah.raw_lib()
    Hc, Wc = O.shape[1:]
    H, W = P.shape[1:]
    specs = {'P': ('in', torch.from_numpy(P.copy())), 'u': ('in', _as_floats(np.pad(np.ascontiguousarray(u, np.float64).reshape(-1), (0, 1)))),
             'region': ('in', _as_floats(np.ascontiguousarray(R, np.uint8))),
             'canvas': ('out', tuple(O.shape), torch.from_numpy(O.copy()))}
    ar = ah.Arena('cuda', specs)
    ptr = lambda k: 0 if k == null else ar.ptr(k) + (4 if k == misalign else 0)      # noqa: E731
    a = dict(dict(Hc=Hc, Wc=Wc, x0=x0, y0=y0, H=H, W=W), **over)
    rc = lib.him_region_poisson_apply(ptr('P'), ptr('u'), ptr('region'), ptr('canvas'), a['Hc'], a['Wc'], a['x0'], a['y0'],
                                      a['H'], a['W'], _stream())
    _check(lib, ar, specs, rc, expect)
    return None if expect != 0 else ar.t['canvas'].cpu().numpy().copy()


def check_case(name, O, P, x0, y0, R, mixed, twice=False):
    """Solve and apply through the arena and judge both with the fixture -> (u, status, resid, canvas, system)."""
    s = fx.system(O, P, x0, y0, R, mixed)
    u, status, resid = call_solve(O, P, x0, y0, R, mixed)
    canvas = call_apply(P, u, R, O, x0, y0)
    rows = []
    bad = fx.compare(u, canvas, status, O, P, x0, y0, R, mixed, RTOL, s=s, rows=rows, case='%s mixed%d' % (name, mixed))
    _report(rows)
    assert not bad, '; '.join(bad)
    assert status[3] <= fx.default_cap(*P.shape[1:]) // 2 or s['n'] == 0
    assert np.isfinite(resid).all() and (resid <= RTOL * (1 + 1e-12)).all()
    if twice:
        again = call_solve(O, P, x0, y0, R, mixed)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (u, status, resid)))       # two runs, the same bits
    return u, status, resid, canvas, s


# ------------------------------------------------------------------------------------------------------- thin windows
@pytest.mark.parametrize('shape', [(1, 9), (9, 1)], ids=['1x9', '9x1'])
@pytest.mark.parametrize('mixed', [0, 1])
def test_a_thin_window_inside_the_canvas_is_all_ring(shape, mixed):
    H, W = shape
    O, P = fx.scene(1, H + 6, W + 6, H, W)
    R = np.ones((H, W), np.uint8)
    u, status, resid = call_solve(O, P, 3, 3, R, mixed)
    assert status.tolist() == [15, 0, H * W, 0, fx.EMPTY, 0, 0, 0] and not u.any() and not resid.any()
    canvas = call_apply(P, u, R, O, 3, 3)
    assert torch.equal(ah.bits(torch.from_numpy(canvas)), ah.bits(torch.from_numpy(O)))


@pytest.mark.parametrize('shape', [(1, 9), (9, 1)], ids=['1x9', '9x1'])
@pytest.mark.parametrize('mixed', [0, 1])
def test_a_thin_window_across_the_canvas_is_a_neumann_strip(shape, mixed):
    H, W = shape
    Hc, Wc, x0, y0 = (1, W + 6, 3, 0) if H == 1 else (H + 6, 1, 0, 3)        # the thin axis spans the canvas
    O, P = fx.scene(2, Hc, Wc, H, W)
    _, status, _, _, s = check_case('strip %dx%d' % shape, O, P, x0, y0, np.ones((H, W), np.uint8), mixed)
    assert s['n'] == 7 and status[2] == 2 and int(np.diag(s['A']).max()) == 2      # deg 2 all along the strip


@pytest.mark.parametrize('case', fx.hand_cases(), ids=[c[0] for c in fx.hand_cases()])
def test_hand_written_answers(case):
    name, O, P, x0, y0, R, mixed, want = case
    u, status, resid = call_solve(O, P, x0, y0, R, mixed)
    assert status[1] == len(want) and status[4] == 0 and status[3] <= len(want)
    for (y, x), v in want.items():
        assert np.abs(u[:, y, x] - v).max() <= 2 * RTOL + fx.HAND_SLACK, (name, y, x)
    canvas = call_apply(P, u, R, O, x0, y0)
    assert fx.compare(u, canvas, status, O, P, x0, y0, R, mixed, RTOL, case=name) == []


# -------------------------------------------------------------------------------------------------- the larger regions
POSITIONS = {'corner': (0, 0), 'right_bottom': (80 - 53, 60 - 37), 'interior': (9, 7)}


@pytest.mark.parametrize('where', list(POSITIONS))
@pytest.mark.parametrize('mixed', [0, 1])
def test_blob_with_hole_island_and_spur(where, mixed):
    x0, y0 = POSITIONS[where]
    R = fx.blob_region()
    O, P = fx.scene(5, 60, 80, 37, 53)
    _, status, _, _, s = check_case('blob ' + where, O, P, x0, y0, R, mixed, twice=(where == 'corner'))
    flags = s['flags']
    assert status[2] > 0 and (where == 'interior' or 0 in flags)             # pixels dropped on a counted side ...
    if where != 'interior':
        om = s['omega']
        assert om[0].any() or om[-1].any() or om[:, 0].any() or om[:, -1].any()   # ... and kept on an uncounted one


@pytest.mark.parametrize('mixed', [0, 1])
def test_full_window(mixed):
    O, P = fx.scene(6, 60, 80, 37, 53)
    _, status, _, _, s = check_case('full 37x53', O, P, 9, 7, np.ones((37, 53), np.uint8), mixed)
    assert s['n'] == 35 * 51 and status[2] == 37 * 53 - 35 * 51


@pytest.mark.parametrize('mixed', [0, 1])
def test_diagonal_band_across_tiles(mixed):
    """67 x 261: more than four 64-column tiles, 17 four-row chunks, column 256; at most 2000 unknowns."""
    R = fx.band_region()
    O, P = fx.scene(7, 100, 300, 67, 261)
    _, _, _, _, s = check_case('band 67x261', O, P, 17, 13, R, mixed, twice=(mixed == 1))
    assert 1500 < s['n'] <= 2000 and s['omega'][:, 256:].any()


def test_whole_canvas_window_is_singular():
    O, P = fx.scene(8, 6, 70, 6, 70)
    for mixed in (0, 1):
        u, status, resid = call_solve(O, P, 0, 0, np.ones((6, 70), np.uint8), mixed)
        assert status.tolist() == [0, 420, 0, 0, fx.SINGULAR, 0, 0, 0] and not u.any() and not resid.any()
        canvas = call_apply(P, u, np.ones((6, 70), np.uint8), O, 0, 0)
        assert np.array_equal(canvas, P)                                       # u = 0: the patch is written


# ------------------------------------------------------------------------------------------------ channels and flags
def test_a_channel_with_nothing_to_solve_next_to_two_live_ones():
    R = fx.blob_region()
    O, P = fx.scene(9, 60, 80, 37, 53)
    P[1] = O[1, 7:7 + 37, 9:9 + 53]                                              # channel 1: P == O, b == 0
    for mixed in (0, 1):
        u, status, resid, _, s = check_case('dead channel', O, P, 9, 7, R, mixed)
        assert not s['b'][1].any() and not u[1].any() and resid[1] == 0 and (resid[[0, 2]] > 0).all() and status[3] > 10


def test_max_iter_3_is_reported_and_leaves_u_finite():
    R = fx.blob_region()
    O, P = fx.scene(5, 60, 80, 37, 53)
    for mixed in (0, 1):
        u, status, resid = call_solve(O, P, 9, 7, R, mixed, max_iter=3)
        s = fx.system(O, P, 9, 7, R, mixed)
        assert status.tolist() == [15, s['n'], s['dropped'], 3, fx.MAX_ITER_HIT, 0, 0, 0]
        assert np.isfinite(u).all() and u.any() and not u[:, ~s['omega']].any() and (resid > RTOL).all() and (resid < 1).all()
        want = fx.cg(s, RTOL, 3)[0]                                              # three steps of the restatement
        assert np.abs(u - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_a_nan_in_the_patch_on_omega_is_reported():
    R = fx.blob_region()
    O, P = fx.scene(5, 60, 80, 37, 53)
    s = fx.system(O, P, 9, 7, R)
    y, x = np.argwhere(s['omega'])[100]
    P[2, y, x] = np.nan
    for mixed in (0, 1):
        u, status, resid = call_solve(O, P, 9, 7, R, mixed)
        assert status.tolist() == [15, s['n'], s['dropped'], 0, fx.NONFINITE, 0, 0, 0] and not u.any() and not resid.any()
    P[2, y, x] = 0.5
    yo, xo = np.argwhere(~s['omega'] & (R == 0))[0]
    far = np.abs(np.argwhere(s['omega']) - [yo, xo]).sum(1).min() > 1
    P[2, yo, xo] = np.nan                                                         # outside Omega and not beside it: unread
    if far:
        _, status, _ = call_solve(O, P, 9, 7, R, 0)
        assert status[4] == 0


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing():
    R = fx.blob_region()
    O, P = fx.scene(5, 60, 80, 37, 53)
    ok = dict(O=O, P=P, x0=9, y0=7, R=R, mixed=0)
    for kw in (dict(null='canvas'), dict(null='P'), dict(null='region'), dict(null='u'), dict(null='status'),
               dict(null='resid'), dict(x0=-1), dict(y0=-1), dict(Wc=9 + 52), dict(Hc=7 + 36), dict(H=0), dict(W=0),
               dict(rtol=0.0), dict(rtol=1.0), dict(rtol=float('nan')), dict(max_iter=0), dict(mixed=2), dict(mixed=-1),
               dict(misalign='u'), dict(misalign='ws')):
        call_solve(**dict(ok, expect=E_INVALID, **kw))
    call_solve(**dict(ok, expect=E_WORKSPACE, null='ws'))
    call_solve(**dict(ok, expect=E_WORKSPACE, short_ws=1))
    u = np.zeros((3, 37, 53))
    for kw in (dict(null='P'), dict(null='u'), dict(null='region'), dict(null='canvas'), dict(x0=-1), dict(y0=60 - 36),
               dict(H=0), dict(W=0), dict(misalign='u')):
        call_apply(**dict(dict(P=P, u=u, R=R, O=O, x0=9, y0=7, expect=E_INVALID), **kw))
