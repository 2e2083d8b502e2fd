"""-m gpu: the boundary-weighted and surface loss kernels (csrc/him_boundary_loss.hip) at the C ABI inside
tests/abi_harness.py's guarded arena, against the float64 restatement of tests/boundary_loss_fixture.py.

Arena: every buffer of a case is a view in ONE allocation between 64 KiB bands, compared bit for bit afterwards; fresh
outputs and the workspace are pre-filled with NaN; the workspace is exactly him_bw_loss_ws() bytes; inputs are compared
bit for bit after the calls.  The int32 distance planes travel as their bit patterns.

Bound (abi_harness.Bound.limit, nothing new): error <= max(8 * e32, 16 * 2^-24) in the metric maximum error over
maximum |ref64|, e32 = the same metric of the fixture's float32 form; for the loss scalar, sum_w and every gradient.
The backward calls are fed the float64 sum_w rounded to fp32 and g = 0.75.  Every case runs twice on fresh arenas and
the two sets of outputs are compared bit for bit."""
import math
import os

import numpy as np
import pytest
import torch

import abi_harness as ah
import boundary_loss_fixture as fx
from boundary_loss_fixture import F32, F64
from test_model_gpu import OUT as REPORT_DIR

pytestmark = pytest.mark.gpu
LOG = ah.RowLog(os.path.join(REPORT_DIR, 'boundary_loss_abi_rows.jsonl'))
G = 0.75
SHAPE_IDS = ['%dx%d' % s for s in fx.SHAPES]
NLL_PLANES = ['uniform', 'checker', 'object', 'ignore']
PAIR_PLANES = ['uniform', 'checker', 'object', 'full']
SURFACE_PLANES = ['empty', 'full', 'object', 'checker']


def _lib():
    return ah.raw_lib()


def _st():
    return ah._stream('cuda')


def _ibits(d2):
    """An int32 plane as the fp32 tensor of the same bits (the arena's views are fp32)."""
    return torch.from_numpy(np.ascontiguousarray(d2, dtype=np.int32)).view(torch.float32)


def _scalar(v):
    return torch.tensor([float(v)], dtype=torch.float32)


def _run(specs, calls):
    """The calls of one case on one arena: return codes, bands and inputs checked; the outputs as CPU tensors."""
    lib = _lib()
    ar = ah.Arena('cuda', specs)
    for fn, args in calls:
        rc = getattr(lib, fn)(*args(ar.ptr))
        assert rc == 0, '%s returned %d (%s)' % (fn, rc, lib.him_last_error())
    torch.cuda.synchronize()
    bad = ar.guard_failures()
    assert not bad, '; '.join(bad)
    for name, s in specs.items():
        if s[0] == 'in':
            assert torch.equal(ah.bits(ar.t[name]), ah.bits(s[1])), 'input %s was written' % name
    return {k: ar.t[k].cpu() for k, s in specs.items() if s[0] == 'out'}


def _twice(specs, calls):
    a, b = _run(specs, calls), _run(specs, calls)
    for k in a:
        assert torch.equal(ah.bits(a[k]), ah.bits(b[k])), '%s differs between two calls on the same inputs' % k
    return a


def _ws():
    return int(_lib().him_bw_loss_ws())


# ------------------------------------------------------------------------------------------------------------- cases
def run_nll(B, C, H, W, plane, amp, sigma):
    ck = ah.Checks('bw_nll|%dx%dx%dx%d|%s|A%g|s%g' % (B, C, H, W, plane, amp, sigma), LOG)
    logp, label = fx.logp_planes(B, C, H, W), fx.label_plane(plane, B, C, H, W)
    mask, d2 = fx.mask_plane(plane, B, H, W), fx.cached_d2('label', plane, B, C, H, W)
    r64, r32 = (fx.bw_nll(logp, label, mask, d2, amp, sigma, dt, g=G) for dt in (F64, F32))
    assert bool(torch.isfinite(r64['loss'])), 'the case has no valid position'
    nws = _ws()
    specs = {'logp': ('in', logp), 'label': ('in', label), 'mask': ('in', mask), 'd2': ('in', _ibits(d2)),
             'g': ('in', _scalar(G)), 'sum_w': ('in', _scalar(r64['sum_w'])), 'out2': ('out', (2,), None),
             'dlogp': ('out', (B, C, H, W), None), 'ws': ('ws', nws)}
    got = _twice(specs, [
        ('him_bw_nll_fwd', lambda P: (P('logp'), P('label'), P('mask'), P('d2'), B, C, H * W, amp, sigma, P('out2'), P('ws'),
                                      nws, _st())),
        ('him_bw_nll_bwd', lambda P: (P('label'), P('mask'), P('d2'), P('g'), P('sum_w'), amp, sigma, P('dlogp'), B, C,
                                      H * W, _st()))])
    ck.row('loss', got['out2'][0], r64['loss'], r32['loss'])
    ck.row('sum_w', got['out2'][1], r64['sum_w'], r32['sum_w'])
    ck.row('dlogp', got['dlogp'], r64['dlogp'], r32['dlogp'])
    ck.done()


def run_pair(B, H, W, plane, kind, amp, sigma, clamp):
    ck = ah.Checks('bw_pair|%dx%dx%d|%s|%s|A%g|s%g%s' % (B, H, W, plane, kind, amp, sigma, '|clamp' if clamp else ''), LOG)
    t, p = fx.object_plane(plane, B, H, W), fx.prob_plane(B, H, W, clamp=clamp)
    d2 = fx.cached_d2('object', plane, B, 2, H, W)
    r64, r32 = (fx.bw_pair(p, t, d2, amp, sigma, kind, dt, g=G) for dt in (F64, F32))
    n, k, nws = B * H * W, {'bce': 0, 'l1': 1}[kind], _ws()
    specs = {'p': ('in', p), 't': ('in', t), 'd2': ('in', _ibits(d2)), 'g': ('in', _scalar(G)),
             'sum_w': ('in', _scalar(r64['sum_w'])), 'out2': ('out', (2,), None), 'dp': ('out', (B, 1, H, W), None),
             'ws': ('ws', nws)}
    got = _twice(specs, [
        ('him_bw_pair_fwd', lambda P: (P('p'), P('t'), P('d2'), n, k, amp, sigma, P('out2'), P('ws'), nws, _st())),
        ('him_bw_pair_bwd', lambda P: (P('p'), P('t'), P('d2'), n, k, P('g'), P('sum_w'), amp, sigma, P('dp'), _st()))])
    ck.row('loss', got['out2'][0], r64['loss'], r32['loss'])
    ck.row('sum_w', got['out2'][1], r64['sum_w'], r32['sum_w'])
    ck.row('dp', got['dp'], r64['dp'], r32['dp'])
    ck.done()


def run_surface(B, H, W, plane):
    ck = ah.Checks('surface|%dx%dx%d|%s' % (B, H, W, plane), LOG)
    t, p = fx.object_plane(plane, B, H, W), fx.prob_plane(B, H, W, seed=3)
    fg, bg = fx.cached_d2('surface', plane, B, 2, H, W)
    r64, r32 = (fx.surface(p, t, fg, bg, dt, g=G) for dt in (F64, F32))
    nws = _ws()
    specs = {'p': ('in', p), 't': ('in', t), 'fg': ('in', _ibits(fg)), 'bg': ('in', _ibits(bg)), 'g': ('in', _scalar(G)),
             'out': ('out', (1,), None), 'dp': ('out', (B, 1, H, W), None), 'ws': ('ws', nws)}
    got = _twice(specs, [
        ('him_surface_fwd', lambda P: (P('p'), P('t'), P('fg'), P('bg'), B, H, W, P('out'), P('ws'), nws, _st())),
        ('him_surface_bwd', lambda P: (P('t'), P('fg'), P('bg'), B, H, W, P('g'), P('dp'), _st()))])
    if plane in ('empty', 'full'):                     # the needed distance is NONE everywhere: exact zeros
        ck.exact('loss', got['out'], torch.zeros(1))
        ck.exact('dp', got['dp'], torch.zeros(B, 1, H, W))
    else:
        ck.row('loss', got['out'][0], r64['loss'], r32['loss'])
        ck.row('dp', got['dp'], r64['dp'], r32['dp'])
    ck.done()


# ------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize('shape', fx.SHAPES, ids=SHAPE_IDS)
def test_bw_nll(shape):
    """Every (B, C) with every plane; the four (A, sigma) rotate so that each meets every plane and every (B, C)."""
    H, W = shape
    i = 0
    for B in (1, 3):
        for C in (1, 2, 35):
            for j, plane in enumerate(NLL_PLANES):
                amp, sigma = fx.AMP_SIGMA[(i + j) % 4]
                run_nll(B, C, H, W, plane, amp, sigma)
            i += 1


@pytest.mark.parametrize('amp,sigma', fx.AMP_SIGMA)
def test_bw_nll_every_amplitude_on_every_plane(amp, sigma):
    for plane in NLL_PLANES:
        run_nll(3, 35, 17, 33, plane, amp, sigma)


@pytest.mark.parametrize('kind', ['bce', 'l1'])
@pytest.mark.parametrize('shape', fx.SHAPES, ids=SHAPE_IDS)
def test_bw_pair(shape, kind):
    H, W = shape
    for i, B in enumerate((1, 3)):
        for j, plane in enumerate(PAIR_PLANES):
            amp, sigma = fx.AMP_SIGMA[(i + j) % 4]
            run_pair(B, H, W, plane, kind, amp, sigma, clamp=(j + i) % 2 == 0)


@pytest.mark.parametrize('kind', ['bce', 'l1'])
@pytest.mark.parametrize('amp,sigma', fx.AMP_SIGMA)
def test_bw_pair_every_amplitude_on_every_plane(amp, sigma, kind):
    for plane in PAIR_PLANES:
        for clamp in (False, True):
            run_pair(3, 17, 33, plane, kind, amp, sigma, clamp)


@pytest.mark.parametrize('shape', fx.SHAPES, ids=SHAPE_IDS)
def test_surface(shape):
    H, W = shape
    for B in (1, 3):
        for plane in SURFACE_PLANES:
            run_surface(B, H, W, plane)


def test_no_valid_position_gives_nan_as_torch():
    B, C, H, W = 2, 3, 7, 5
    logp, label = fx.logp_planes(B, C, H, W), fx.label_plane('checker', B, C, H, W)
    mask = torch.zeros(B, 1, H, W)
    d2 = fx.boundary_d2(label.numpy())
    assert math.isnan(float(torch.nn.functional.nll_loss(logp, torch.full((B, H, W), 255), ignore_index=255)))
    assert math.isnan(float(fx.bw_nll(logp, label, mask, d2, 4.0, 1.0)['loss']))
    nws = _ws()
    specs = {'logp': ('in', logp), 'label': ('in', label), 'mask': ('in', mask), 'd2': ('in', _ibits(d2)),
             'out2': ('out', (2,), None), 'ws': ('ws', nws)}
    got = _run(specs, [('him_bw_nll_fwd', lambda P: (P('logp'), P('label'), P('mask'), P('d2'), B, C, H * W, 4.0, 1.0,
                                                     P('out2'), P('ws'), nws, _st()))])
    assert math.isnan(float(got['out2'][0])) and float(got['out2'][1]) == 0.0


def test_refusals_return_their_code_and_write_nothing():
    lib = _lib()
    B, C, H, W = 2, 3, 7, 5
    n, hw, nws = B * H * W, H * W, _ws()
    label, t = fx.label_plane('object', B, C, H, W), fx.object_plane('object', B, H, W)
    d2 = _ibits(fx.boundary_d2(label.numpy()))
    specs = {'logp': ('in', fx.logp_planes(B, C, H, W)), 'label': ('in', label), 'mask': ('in', fx.mask_plane('object', B, H, W)),
             'p': ('in', fx.prob_plane(B, H, W)), 't': ('in', t), 'd2': ('in', d2), 'g': ('in', _scalar(G)),
             'sum_w': ('in', _scalar(50.0)), 'out2': ('out', (2,), None), 'dlogp': ('out', (B, C, H, W), None),
             'dp': ('out', (B, 1, H, W), None), 'ws': ('ws', nws)}
    st = _st()
    nan, inf = float('nan'), float('inf')
    bad_as = [(-1.0, 1.0), (1.0, 0.0), (1.0, -1.0), (nan, 1.0), (1.0, nan), (inf, 1.0), (1.0, inf)]

    def nll_fwd(P, **o):
        a = dict(logp=P('logp'), label=P('label'), mask=P('mask'), d2=P('d2'), B=B, C=C, hw=hw, amp=4.0, sigma=1.0,
                 out2=P('out2'), ws=P('ws'), nws=nws)
        a.update(o)
        return ('him_bw_nll_fwd', (a['logp'], a['label'], a['mask'], a['d2'], a['B'], a['C'], a['hw'], a['amp'], a['sigma'],
                                   a['out2'], a['ws'], a['nws'], st))

    def nll_bwd(P, **o):
        a = dict(label=P('label'), mask=P('mask'), d2=P('d2'), g=P('g'), sum_w=P('sum_w'), amp=4.0, sigma=1.0,
                 dlogp=P('dlogp'), B=B, C=C, hw=hw)
        a.update(o)
        return ('him_bw_nll_bwd', (a['label'], a['mask'], a['d2'], a['g'], a['sum_w'], a['amp'], a['sigma'], a['dlogp'],
                                   a['B'], a['C'], a['hw'], st))

    def pair_fwd(P, **o):
        a = dict(p=P('p'), t=P('t'), d2=P('d2'), n=n, kind=0, amp=4.0, sigma=1.0, out2=P('out2'), ws=P('ws'), nws=nws)
        a.update(o)
        return ('him_bw_pair_fwd', (a['p'], a['t'], a['d2'], a['n'], a['kind'], a['amp'], a['sigma'], a['out2'], a['ws'],
                                    a['nws'], st))

    def pair_bwd(P, **o):
        a = dict(p=P('p'), t=P('t'), d2=P('d2'), n=n, kind=1, g=P('g'), sum_w=P('sum_w'), amp=4.0, sigma=1.0, dp=P('dp'))
        a.update(o)
        return ('him_bw_pair_bwd', (a['p'], a['t'], a['d2'], a['n'], a['kind'], a['g'], a['sum_w'], a['amp'], a['sigma'],
                                    a['dp'], st))

    def surf_fwd(P, **o):
        a = dict(p=P('p'), t=P('t'), fg=P('d2'), bg=P('d2'), B=B, H=H, W=W, out=P('out2'), ws=P('ws'), nws=nws)
        a.update(o)
        return ('him_surface_fwd', (a['p'], a['t'], a['fg'], a['bg'], a['B'], a['H'], a['W'], a['out'], a['ws'], a['nws'], st))

    def surf_bwd(P, **o):
        a = dict(t=P('t'), fg=P('d2'), bg=P('d2'), B=B, H=H, W=W, g=P('g'), dp=P('dp'))
        a.update(o)
        return ('him_surface_bwd', (a['t'], a['fg'], a['bg'], a['B'], a['H'], a['W'], a['g'], a['dp'], st))

    cases = []
    weighted = [(nll_fwd, ['logp', 'label', 'mask', 'd2', 'out2'], ['B', 'C', 'hw']),
                (nll_bwd, ['label', 'mask', 'd2', 'g', 'sum_w', 'dlogp'], ['B', 'C', 'hw']),
                (pair_fwd, ['p', 't', 'd2', 'out2'], ['n']), (pair_bwd, ['p', 't', 'd2', 'g', 'sum_w', 'dp'], ['n'])]
    for build, ptrs, dims in weighted:
        cases += [(build, {k: 0}, ah.E_INVALID) for k in ptrs + dims]
        cases += [(build, {'amp': a, 'sigma': s}, ah.E_INVALID) for a, s in bad_as]
    cases += [(pair_fwd, {'kind': 2}, ah.E_INVALID), (pair_fwd, {'kind': -1}, ah.E_INVALID), (pair_bwd, {'kind': 2}, ah.E_INVALID)]
    cases += [(surf_fwd, {k: 0}, ah.E_INVALID) for k in ('p', 't', 'fg', 'bg', 'out', 'B', 'H', 'W')]
    cases += [(surf_bwd, {k: 0}, ah.E_INVALID) for k in ('t', 'fg', 'bg', 'g', 'dp', 'B', 'H', 'W')]
    for build in (nll_fwd, pair_fwd, surf_fwd):
        cases += [(build, {'nws': nws - 1}, ah.E_WORKSPACE), (build, {'ws': 0}, ah.E_WORKSPACE)]
    ar = ah.Arena('cuda', specs)
    for build, over, code in cases:
        fn, args = build(ar.ptr, **over)
        rc = getattr(lib, fn)(*args)
        assert rc == code, '%s with %s returned %d, expected %d' % (fn, over, rc, code)
    torch.cuda.synchronize()
    assert not ar.guard_failures()
    ah.untouched(ar, specs)
