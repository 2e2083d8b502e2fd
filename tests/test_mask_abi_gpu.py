"""-m gpu: the box2mask building blocks of csrc/him_mask.hip (and him_act_bwd) at the C ABI inside tests/abi_harness.py's
guarded arena, against the float64 restatements of tests/mask_fixture.py.

Arena: every buffer of a call is a view in ONE allocation between 64 KiB bands; NaN bands beside inputs, 0xA5 bands beside
outputs and workspace, compared bit for bit afterwards; fresh outputs and the workspace are pre-filled with NaN; the
workspace is exactly him_batchnorm_ws(C) / him_mask_loss_ws() bytes; inputs are compared bit for bit after the call.

Bound (tests/README.md, direct form, per tensor): error <= max(8 * e32, 16 * 2^-24) in the metric maximum error over
maximum |ref64|, e32 = the same metric of the fixture's float32 form.  save_rstd also per element.  Results the header
promises exactly are compared with torch.equal.  No element is excluded except in him_resize_compose (fixture MARGIN).
One JSON line per checked tensor goes to mask_abi_rows.jsonl in the GPU tests' report directory before anything is
asserted.

The runners take the library and the device as parameters: tests/test_mask_fixture_cpu.py passes CPU stand-ins with one
planted defect each."""
import os

import pytest
import torch

import abi_harness as ah
import mask_fixture as fx
from mask_fixture import F32, F64
from test_model_gpu import OUT as REPORT_DIR

pytestmark = pytest.mark.gpu
OUT = os.path.join(REPORT_DIR, 'mask_abi_rows.jsonl')
LOG = ah.RowLog(OUT)
ROWS = LOG.rows
call, untouched, _bits = ah.call, ah.untouched, ah.bits      # the guarded call and its helpers live in abi_harness.py


@pytest.fixture(autouse=True)
def _dump():
    yield
    flush()


def flush():
    LOG.flush()


def _lib():
    return ah.raw_lib()


class Checks(ah.Checks):
    """abi_harness.Checks on this module's rows, with mask_fixture's metric and limit."""

    def __init__(self, case):
        ah.Checks.__init__(self, case, LOG, flush=lambda: flush(), metric=fx.rel_err, limit=fx.limit)


def _st(dev):
    return ah._stream(dev)


# ------------------------------------------------------------------------------------------------------- BatchNorm2d
def run_bn(lib, dev, c, dx=True, accumulate=0, chained=False, tag=''):
    """Forward, then the backward fed with the float64 statistics rounded to fp32 (``chained``: with the forward's own)."""
    ck = Checks(c.tag() + tag + ('|acc' if accumulate else '') + ('' if dx else '|nodx') + ('|chained' if chained else ''))
    r64, r32 = c.ref(F64), c.ref(F32)
    B, C, hw = c.B, c.C, c.hw
    nws = int(lib.him_batchnorm_ws(C))
    specs = {'x': ('in', c.x)}
    for k in ('residual', 'gamma', 'beta'):
        if getattr(c, k) is not None:
            specs[k] = ('in', getattr(c, k))
    if c.running:
        specs['run_mean'] = ('out', (C,), c.rm0) if c.training else ('in', c.rm0)
        specs['run_var'] = ('out', (C,), c.rv0) if c.training else ('in', c.rv0)
    specs.update(y=('out', (B, C, hw), None), save_mean=('out', (C,), None), save_rstd=('out', (C,), None), ws=('ws', nws))
    ar = call(lib, dev, 'him_batchnorm_fwd', specs, lambda P: (
        P('x'), P('residual'), P('gamma'), P('beta'), P('run_mean'), P('run_var'), P('y'), P('save_mean'), P('save_rstd'),
        B, C, hw, fx.BN_EPS, fx.BN_MOMENTUM, int(c.training), fx.ACTS[c.act], fx.SLOPE, P('ws'), nws, _st(dev)))
    names = ['y', 'save_mean', 'save_rstd'] + (['run_mean', 'run_var'] if c.running and c.training else [])
    got = {k: ar.t[k].cpu() for k in names}
    for k in names:
        lim = ck.row(k, got[k], r64[k], r32[k])
        if k == 'save_rstd':
            ck.row('save_rstd/element', got[k], r64[k], r32[k], metric=fx.elem_err, lim=lim)
    mean, rstd = (got['save_mean'], got['save_rstd']) if chained else (r64['save_mean'].float(), r64['save_rstd'].float())
    if not (torch.isfinite(mean).all() and torch.isfinite(rstd).all()):
        ck.done()
    specs = {'x': ('in', c.x), 'dy': ('in', c.dy), 'save_mean': ('in', mean), 'save_rstd': ('in', rstd)}
    if c.affine:
        specs.update(gamma=('in', c.gamma), beta=('in', c.beta),
                     dgamma=('out', (C,), c.dgamma0 if accumulate else None),
                     dbeta=('out', (C,), c.dbeta0 if accumulate else None))
    if dx:
        specs['dx'] = ('out', (B, C, hw), None)
    specs['ws'] = ('ws', nws)
    ar = call(lib, dev, 'him_batchnorm_bwd', specs, lambda P: (
        P('x'), P('gamma'), P('beta'), P('save_mean'), P('save_rstd'), P('dy'), P('dx'), P('dgamma'), P('dbeta'), B, C, hw,
        int(c.training), fx.ACTS[c.act], fx.SLOPE, accumulate, P('ws'), nws, _st(dev)))
    if dx:
        ck.row('dx', ar.t['dx'], r64['dx'], r32['dx'])
    if c.affine:
        for k, base in (('dgamma', c.dgamma0), ('dbeta', c.dbeta0)):
            add64, add32 = (base.double(), base) if accumulate else (0, 0)
            ck.row(k, ar.t[k], r64[k] + add64, r32[k] + add32)
    ck.done()


BN_SHAPES = [(2, 3, 1), (5, 3, 12), (64, 2, 4), (3, 2, 7), (2, 2, 1028), (2, 2, 2052), (1, 2, 1025), (2, 2, 2500), (8, 4, 1024)]
BN_CROSS = [(5, 3, 12), (3, 2, 7)]                      # one vector, one scalar shape: the full option cross
ACT_NAMES = ['none', 'relu', 'lrelu', 'tanh', 'sigmoid']


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('shape', BN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_batchnorm_shapes(shape, training):
    act = ACT_NAMES[BN_SHAPES.index(shape) % 5]
    run_bn(_lib(), 'cuda', fx.BNCase(*shape, training, act, residual=BN_SHAPES.index(shape) % 2 == 1))
    run_bn(_lib(), 'cuda', fx.BNCase(*shape, training, act), chained=True)


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('act', ACT_NAMES)
@pytest.mark.parametrize('shape', BN_CROSS, ids=lambda s: 'x'.join(map(str, s)))
def test_batchnorm_option_cross(shape, act, training):
    for residual in (False, True):
        for affine in (True, False):
            for running in ((True, False) if training else (True,)):
                c = fx.BNCase(*shape, training, act, residual=residual, affine=affine, running=running)
                for dx in (True, False):
                    for accumulate in ((0, 1) if affine else (0,)):
                        run_bn(_lib(), 'cuda', c, dx=dx, accumulate=accumulate)


@pytest.mark.parametrize('gen', fx.BN_ILL)
@pytest.mark.parametrize('shape', [(8, 4, 1024), (4, 16, 117)], ids=lambda s: 'x'.join(map(str, s)))
def test_batchnorm_ill_conditioned(shape, gen):
    """With the statistics as they were first written (pivot x[0][c][0], q/n - ms*ms) the save_rstd rows of first30,
    first100 and offset100_first-100 measured 5.2e-5 to 7.9e-4 against the limit 9.5e-7, and y, dx, dgamma and the running
    variance followed; const_plus_noise and the constant channel passed then as now."""
    c = fx.BNCase(*shape, True, 'none', gen=gen)
    if gen == 'const_channel':
        assert float(c.ref(F64)['save_rstd'][1]) == fx.BN_EPS ** -0.5
    run_bn(_lib(), 'cuda', c, chained=True)


# ------------------------------------------------------------------------------------------- stand-alone activation
SPECIALS = torch.tensor([0.0, -0.0, 88.0, -88.0, 1e-30, -1e-30, 20.0, -20.0])


def act_input(n):
    x = fx.rand(n, seed=n % 1000, scale=2.0)
    x[:min(n, 8)] = SPECIALS[:min(n, 8)]
    if n > 16:
        x[-8:] = SPECIALS.flip(0)
    return x


def run_act(lib, dev, n, act):
    ck = Checks('act|%s|n%d' % (act, n))
    x = act_input(n)
    ar = call(lib, dev, 'him_act_fwd', {'x': ('in', x), 'y': ('out', (n,), None)},
              lambda P: (P('x'), P('y'), n, fx.ACTS[act], fx.SLOPE, _st(dev)))
    ck.row('y', ar.t['y'], fx.act_fn(x.double(), act), fx.act_fn(x, act))
    y, dy = fx.act_fn(x, act), fx.rand(n, seed=3)
    ar = call(lib, dev, 'him_act_bwd', {'y': ('in', y), 'dy': ('in', dy), 'dz': ('out', (n,), None)},
              lambda P: (P('y'), P('dy'), P('dz'), n, fx.ACTS[act], fx.SLOPE, _st(dev)))
    ck.row('dz', ar.t['dz'], fx.act_bwd(y, dy, act, F64), fx.act_bwd(y, dy, act, F32))
    ck.done()


@pytest.mark.parametrize('act', ACT_NAMES[1:])
@pytest.mark.parametrize('n', [1, 255, fx.GRID_CAP + 257])
def test_activation(n, act):
    run_act(_lib(), 'cuda', n, act)


# ------------------------------------------------------------------------------------------------------ bilinear x2
def run_upsample(lib, dev, planes, H, W, align, fwd=True):
    ck = Checks('upsample2|%dx%dx%d|align%d' % (planes, H, W, align))
    x, dy = fx.rand(planes, H, W, seed=1), fx.rand(planes, 2 * H, 2 * W, seed=2)
    if fwd:
        ar = call(lib, dev, 'him_upsample2_fwd', {'x': ('in', x), 'y': ('out', (planes, 2 * H, 2 * W), None)},
                  lambda P: (P('x'), P('y'), planes, H, W, align, _st(dev)))
        ck.row('y', ar.t['y'], fx.upsample2(x, align, F64), fx.upsample2(x, align, F32))
    ar = call(lib, dev, 'him_upsample2_bwd', {'dy': ('in', dy), 'dx': ('out', (planes, H, W), None)},
              lambda P: (P('dy'), P('dx'), planes, H, W, align, _st(dev)))
    ck.row('dx', ar.t['dx'], fx.upsample2(x, align, F64, dy), fx.upsample2(x, align, F32, dy))
    ck.done()


@pytest.mark.parametrize('align', [0, 1])
@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 1, 7), (1, 9, 1), (3, 2, 2), (2, 5, 3), (1, 63, 65), (3, 420, 420),
                                   (3, 840, 840)], ids=lambda s: 'x'.join(map(str, s)))
def test_bilinear_upsample2(shape, align):
    run_upsample(_lib(), 'cuda', *shape, align, fwd=shape != (3, 840, 840))


# ------------------------------------------------------------------------------------------------------ log-softmax
def run_logsoftmax(lib, dev, B, C, hw, big=False):
    ck = Checks('logsoftmax|%dx%dx%d%s' % (B, C, hw, '|pm80' if big else ''))
    x = fx.rand(B, C, hw, seed=1, scale=3.0)
    if big:
        x = (x / x.abs().max() * 80.0)
        x[:, C // 2] = 80.0                              # one dominant channel
        x[:, 0] = -80.0
    dy = fx.rand(B, C, hw, seed=2)
    ar = call(lib, dev, 'him_logsoftmax_fwd', {'x': ('in', x), 'y': ('out', (B, C, hw), None)},
              lambda P: (P('x'), P('y'), B, C, hw, _st(dev)))
    ck.row('y', ar.t['y'], fx.log_softmax(x, F64), fx.log_softmax(x, F32))
    y = fx.log_softmax(x, F32)
    ar = call(lib, dev, 'him_logsoftmax_bwd', {'y': ('in', y), 'dy': ('in', dy), 'dx': ('out', (B, C, hw), None)},
              lambda P: (P('y'), P('dy'), P('dx'), B, C, hw, _st(dev)))
    ck.row('dx', ar.t['dx'], fx.log_softmax_bwd(y, dy, F64), fx.log_softmax_bwd(y, dy, F32))
    ck.done()


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 2, 16), (2, 35, 99), (3, 70, 256), (1, 2, fx.GRID_CAP + 300)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_log_softmax(shape):
    run_logsoftmax(_lib(), 'cuda', *shape)


def test_log_softmax_logits_of_magnitude_80():
    run_logsoftmax(_lib(), 'cuda', 2, 35, 99, big=True)


# ------------------------------------------------------------------------------------------------- gate combination
def run_gate(lib, dev, B, C, hw, fwd=True, bwd=True):
    ck = Checks('gate_comb|%dx%dx%d' % (B, C, hw))
    ctx, obj, dout = fx.rand(B, C, hw, seed=1, scale=2.0), fx.rand(B, 1, hw, seed=2, scale=2.0), fx.rand(B, C, hw, seed=3)
    p = torch.sigmoid(obj)
    ins = {'ctx': ('in', ctx), 'p': ('in', p), 'obj': ('in', obj)}
    if fwd:
        ar = call(lib, dev, 'him_gate_comb_fwd', dict(ins, out=('out', (B, C, hw), None)),
                  lambda P: (P('ctx'), P('p'), P('obj'), P('out'), B, C, hw, _st(dev)))
        ck.row('out', ar.t['out'], fx.gate_comb(ctx, p, obj, F64), fx.gate_comb(ctx, p, obj, F32))
        ck.exact('out==f32', ar.t['out'], fx.gate_comb(ctx, p, obj, F32))
    if bwd:
        ar = call(lib, dev, 'him_gate_comb_bwd',
                  dict(ins, dout=('in', dout), dctx=('out', (B, C, hw), None), dp=('out', (B, 1, hw), None),
                       dobj=('out', (B, 1, hw), None)),
                  lambda P: (P('ctx'), P('p'), P('obj'), P('dout'), P('dctx'), P('dp'), P('dobj'), B, C, hw, _st(dev)))
        r64, r32 = fx.gate_comb_bwd(ctx, p, obj, dout, F64), fx.gate_comb_bwd(ctx, p, obj, dout, F32)
        for k in ('dctx', 'dp', 'dobj'):
            ck.row(k, ar.t[k], r64[k], r32[k])
    ck.done()


@pytest.mark.parametrize('shape,fwd,bwd', [((1, 1, 1), 1, 1), ((2, 35, 99), 1, 1), ((3, 49, 1024), 1, 1),
                                           ((1, 3, 700000), 1, 0), ((1, 2, fx.GRID_CAP + 300), 0, 1)],
                         ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gate_combination(shape, fwd, bwd):
    run_gate(_lib(), 'cuda', *shape, fwd=bool(fwd), bwd=bool(bwd))


# ------------------------------------------------------------------------------------------------------- masked NLL
def run_nll(lib, dev, B, C, hw, kind='random'):
    ck = Checks('masked_nll|%dx%dx%d|%s' % (B, C, hw, kind))
    logp, label, mask = fx.nll_case(B, C, hw, kind)
    nws = int(lib.him_mask_loss_ws())
    ar = call(lib, dev, 'him_masked_nll_fwd',
              {'logp': ('in', logp), 'label': ('in', label), 'mask': ('in', mask), 'out2': ('out', (2,), None), 'ws': ('ws', nws)},
              lambda P: (P('logp'), P('label'), P('mask'), P('out2'), B, C, hw, P('ws'), nws, _st(dev)))
    out2 = ar.t['out2'].cpu()
    g = torch.tensor([0.7])
    loss64, count, d64 = fx.masked_nll(logp, label, mask, F64, g)
    loss32, _, d32 = fx.masked_nll(logp, label, mask, F32, g)
    ROWS.append(dict(case=ck.case, tensor='count', error=abs(float(out2[1]) - count), e32=0.0, ratio=None, limit=0.0))
    if float(out2[1]) != count:
        ck.failed.append('%s: count %r, expected %d' % (ck.case, float(out2[1]), count))
    if count == 0:
        assert bool(torch.isnan(out2[0])) and bool(torch.isnan(loss64)), ck.case
    else:
        ck.row('loss', out2[:1], loss64.reshape(1), loss32.reshape(1))
    cnt = torch.tensor([float(count)])
    ar = call(lib, dev, 'him_masked_nll_bwd',
              {'label': ('in', label), 'mask': ('in', mask), 'g': ('in', g), 'count': ('in', cnt),
               'dlogp': ('out', (B, C, hw), None)},
              lambda P: (P('label'), P('mask'), P('g'), P('count'), P('dlogp'), B, C, hw, _st(dev)))
    d = ar.t['dlogp'].cpu()
    if count == 0:
        assert bool((d == 0).all()), ck.case
    else:
        ck.row('dlogp', d, d64, d32)
        assert bool((d[d64 == 0] == 0).all()), '%s: an ignored or other-class element is not exactly 0' % ck.case
    ck.done()


@pytest.mark.parametrize('case', [(3, 35, 168, 'random'), (1, 2, 1, 'one'), (3, 2, 90001, 'random'), (3, 35, 168, 'none'),
                                  (3, 35, 168, 'one')], ids=lambda c: 'x'.join(map(str, c)))
def test_masked_nll(case):
    assert 3 * 90001 > fx.LOSS_CAP
    run_nll(_lib(), 'cuda', *case)


# --------------------------------------------------------------------------------------------------------------- BCE
def run_bce(lib, dev, n, kind='interior'):
    ck = Checks('bce|n%d|%s' % (n, kind))
    if kind == 'interior':
        p, t = torch.sigmoid(fx.rand(n, seed=1, scale=3.0)), (fx.uniform(n, seed=2) > 0.5).float()
    else:
        p, t = fx.bce_saturated()
    nws = int(lib.him_mask_loss_ws())
    ar = call(lib, dev, 'him_bce_mean_fwd', {'p': ('in', p), 't': ('in', t), 'out': ('out', (1,), None), 'ws': ('ws', nws)},
              lambda P: (P('p'), P('t'), n, P('out'), P('ws'), nws, _st(dev)))
    ck.row('loss', ar.t['out'], fx.bce_mean(p, t, F64).reshape(1), fx.bce_mean(p, t, F32).reshape(1))
    g = torch.tensor([0.7])
    ar = call(lib, dev, 'him_bce_mean_bwd', {'p': ('in', p), 't': ('in', t), 'g': ('in', g), 'dp': ('out', (n,), None)},
              lambda P: (P('p'), P('t'), n, P('g'), P('dp'), _st(dev)))
    r64, r32 = fx.bce_mean_bwd(p, t, float(g), F64), fx.bce_mean_bwd(p, t, float(g), F32)
    ck.row('dp', ar.t['dp'], r64, r32)
    if kind == 'saturated':
        ck.row('dp/element', ar.t['dp'], r64, r32, metric=fx.elem_err)
    ck.done()


@pytest.mark.parametrize('n,kind', [(1, 'interior'), (396, 'interior'), (270003, 'interior'), (64, 'saturated')])
def test_bce(n, kind):
    run_bce(_lib(), 'cuda', n, kind)


# --------------------------------------------------------------------------------------------------- space-to-batch
@pytest.mark.parametrize('d', [1, 2, 4])
@pytest.mark.parametrize('shape', [(1, 1, 4, 4), (2, 3, 8, 12), (1, 2, 1024, 1028)], ids=lambda s: 'x'.join(map(str, s)))
def test_space_to_batch_both_directions(shape, d):
    lib, dev = _lib(), 'cuda'
    B, C, H, W = shape
    ck = Checks('space_to_batch|%s|d%d' % ('x'.join(map(str, shape)), d))
    x = fx.rand(*shape, seed=1)
    want = fx.space_to_batch(x, d)
    ar = call(lib, dev, 'him_space_to_batch', {'x': ('in', x), 'y': ('out', tuple(want.shape), None)},
              lambda P: (P('x'), P('y'), B, C, H, W, d, 0, _st(dev)))
    y = ar.t['y'].cpu()
    ck.exact('phases', y, want)
    ar = call(lib, dev, 'him_space_to_batch', {'x': ('in', y), 'y': ('out', shape, None)},
              lambda P: (P('x'), P('y'), B, C, H, W, d, 1, _st(dev)))
    ck.exact('round trip', ar.t['y'], x)
    ck.exact('inverse', ar.t['y'], fx.batch_to_space(want, d, B))
    ck.done()


def test_space_to_batch_refuses_an_indivisible_height():
    specs = {'x': ('in', fx.rand(1, 1, 6, 8, seed=1)), 'y': ('out', (16, 1, 1, 2), None)}
    for H, W in ((6, 8), (8, 6)):
        ar = call(_lib(), 'cuda', 'him_space_to_batch', specs,
                  lambda P: (P('x'), P('y'), 1, 1, H, W, 4, 0, _st('cuda')), expect=ah.E_UNSUPPORTED)
        untouched(ar, specs)


# ------------------------------------------------------------------------------------------------------- class mask
def run_class_mask(lib, dev, B, NC, Ctot, c0, hw, cls):
    ck = Checks('class_mask|%dx%dx%dx%dx%d' % (B, NC, Ctot, c0, hw))
    mask, before = fx.uniform(B, hw, seed=1), fx.rand(B, Ctot, hw, seed=2)
    cls = torch.tensor(cls, dtype=F32)
    ar = call(lib, dev, 'him_class_mask', {'mask': ('in', mask), 'cls': ('in', cls), 'dst': ('out', (B, Ctot, hw), before)},
              lambda P: (P('mask'), P('cls'), P('dst'), B, NC, Ctot, c0, hw, _st(dev)))
    want = fx.class_mask(mask, cls, before, NC, c0)
    assert torch.equal(_bits(ar.t['dst']), _bits(want)), ck.case            # bit for bit: prefill and written channels
    ck.exact('dst', ar.t['dst'], want)
    ck.done()


@pytest.mark.parametrize('case', [(1, 1, 1, 0, 1, [0.0]), (3, 35, 40, 2, 99, [34.0, 35.0, 0.0]), (3, 35, 40, 2, 99, [-1.0, 7.0, 99.0]),
                                  (2, 35, 35, 0, 30001, [3.0, 34.0])], ids=lambda c: 'x'.join(map(str, c[:5])))
def test_class_mask(case):
    run_class_mask(_lib(), 'cuda', *case)


# ------------------------------------------------------------------------------------------------- him_resize_compose
def run_resize(lib, dev, case, lo, hi, background, align, tag, exclude=True):
    src, label, mask, cls = case
    (h, w), (H, W) = lo, hi
    C = src.shape[0]
    specs = {'src': ('in', src), 'label': ('in', label)}
    if background:
        specs['mask'] = ('in', mask)
    specs['dst'] = ('ws', H * W * 8) if background else ('out', (H, W), None)
    ar = call(lib, dev, 'him_resize_compose', specs, lambda P: (
        P('src') if background else 0, 0 if background else P('src'), C, h, w, P('label'), P('mask'), cls,
        int(background), P('dst'), H, W, align, _st(dev)))
    got = ar.t['dst'].cpu()
    got = got.view(torch.int64).view(H, W) if background else got
    want, margin = fx.resize_compose(src, label, mask, cls, background, align)
    keep = (margin >= fx.MARGIN) if exclude else torch.ones(H, W, dtype=torch.bool)
    left_out = 1.0 - float(keep.double().mean())
    wrong = int((got[keep] != want[keep].to(got.dtype)).sum())
    ROWS.append(dict(case=tag, tensor='decision', error=wrong / float(H * W), e32=0.0, ratio=None, limit=0.0,
                     left_out=left_out))
    flush()
    assert left_out <= fx.MAX_LEFT_OUT, '%s: %.4f of the pixels left out' % (tag, left_out)
    assert wrong == 0, '%s: %d decisions differ from the float64 restatement' % (tag, wrong)
    return got


@pytest.mark.parametrize('align', [0, 1])
@pytest.mark.parametrize('background', [0, 1], ids=['object', 'background'])
@pytest.mark.parametrize('lo,hi', fx.RESIZE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_resize_compose(lo, hi, background, align):
    tag = 'resize_compose|%dx%d->%dx%d|bg%d|align%d' % (lo + hi + (background, align))
    run_resize(_lib(), 'cuda', fx.resize_case(lo, hi, background), lo, hi, background, align, tag)


@pytest.mark.parametrize('align', [0, 1])
def test_resize_compose_first_index_wins_a_tie(align):
    got = run_resize(_lib(), 'cuda', fx.resize_tie_case(), (8, 8), (16, 16), 1, align, 'resize_compose|tie|align%d' % align,
                     exclude=False)
    assert bool((got == 3).all())


# ----------------------------------------------------------------------------------------------------- return codes
def test_refused_calls_write_nothing():
    lib, dev = _lib(), 'cuda'
    st = _st(dev)
    c = fx.BNCase(5, 3, 12, True)
    nws = int(lib.him_batchnorm_ws(3))
    specs = {'x': ('in', c.x), 'dy': ('in', c.dy), 'run_mean': ('out', (3,), c.rm0), 'run_var': ('out', (3,), c.rv0),
             'y': ('out', (5, 3, 12), None), 'save_mean': ('out', (3,), None), 'save_rstd': ('out', (3,), None),
             'dgamma': ('out', (3,), None), 'ws': ('ws', nws)}

    def fwd(B=5, C=3, hw=12, training=1, run=True, ws_bytes=nws):
        return lambda P: (P('x'), 0, 0, 0, P('run_mean') if run else 0, P('run_var') if run else 0, P('y'), P('save_mean'),
                          P('save_rstd'), B, C, hw, fx.BN_EPS, fx.BN_MOMENTUM, training, 0, fx.SLOPE, P('ws'), ws_bytes, st)

    def bwd(B=5, C=3, hw=12, ws_bytes=nws):
        return lambda P: (P('x'), 0, 0, P('run_mean'), P('run_var'), P('dy'), P('y'), P('dgamma'), P('save_mean'), B, C, hw, 1,
                          0, fx.SLOPE, 0, P('ws'), ws_bytes, st)

    for fn, args, code in [
            ('him_batchnorm_fwd', fwd(ws_bytes=nws - 1), ah.E_WORKSPACE), ('him_batchnorm_bwd', bwd(ws_bytes=nws - 1), ah.E_WORKSPACE),
            ('him_batchnorm_fwd', fwd(B=256, C=256, hw=1), ah.E_UNSUPPORTED), ('him_batchnorm_bwd', bwd(B=256, C=256, hw=1), ah.E_UNSUPPORTED),
            ('him_batchnorm_fwd', fwd(training=0, run=False), ah.E_INVALID),
            ('him_batchnorm_fwd', fwd(B=0), ah.E_INVALID), ('him_batchnorm_fwd', fwd(C=-1), ah.E_INVALID),
            ('him_batchnorm_fwd', fwd(hw=0), ah.E_INVALID), ('him_batchnorm_bwd', bwd(hw=-3), ah.E_INVALID),
            ('him_upsample2_fwd', lambda P: (P('x'), P('y'), 0, 3, 4, 0, st), ah.E_INVALID),
            ('him_upsample2_bwd', lambda P: (P('x'), P('y'), 3, -1, 4, 0, st), ah.E_INVALID),
            ('him_logsoftmax_fwd', lambda P: (P('x'), P('y'), 5, 0, 12, st), ah.E_INVALID),
            ('him_logsoftmax_bwd', lambda P: (P('x'), P('dy'), P('y'), 5, 3, 0, st), ah.E_INVALID),
            ('him_gate_comb_fwd', lambda P: (P('x'), P('dy'), P('dy'), P('y'), 0, 3, 12, st), ah.E_INVALID),
            ('him_gate_comb_bwd', lambda P: (P('x'), P('dy'), P('dy'), P('dy'), P('y'), P('y'), P('y'), 5, 3, -12, st), ah.E_INVALID),
            ('him_space_to_batch', lambda P: (P('x'), P('y'), 5, 3, 0, 4, 1, 0, st), ah.E_INVALID),
            ('him_space_to_batch', lambda P: (P('x'), P('y'), 5, 3, 3, 4, 0, 0, st), ah.E_INVALID),
            ('him_class_mask', lambda P: (P('x'), P('dy'), P('y'), 5, 3, 2, 0, 12, st), ah.E_INVALID),
            ('him_class_mask', lambda P: (P('x'), P('dy'), P('y'), 5, 0, 3, 0, 12, st), ah.E_INVALID),
            ('him_resize_compose', lambda P: (P('x'), P('x'), 3, 0, 4, P('dy'), P('dy'), 1, 0, P('y'), 6, 8, 0, st), ah.E_INVALID),
            ('him_resize_compose', lambda P: (0, 0, 3, 3, 4, P('dy'), P('dy'), 1, 0, P('y'), 6, 8, 0, st), ah.E_INVALID),
            ('him_bce_mean_fwd', lambda P: (P('x'), P('dy'), 0, P('y'), P('ws'), nws, st), ah.E_INVALID)]:
        untouched(call(lib, dev, fn, specs, args, expect=code), specs)
    nl = int(lib.him_mask_loss_ws())
    lspecs = {'p': ('in', fx.uniform(3, 2, 12, seed=1)), 't': ('in', fx.uniform(3, 12, seed=2)), 'out': ('out', (2,), None),
              'ws': ('ws', nl)}
    for fn, args in [('him_masked_nll_fwd', lambda P: (P('p'), P('t'), P('t'), P('out'), 3, 2, 12, P('ws'), nl - 1, st)),
                     ('him_bce_mean_fwd', lambda P: (P('p'), P('p'), 72, P('out'), P('ws'), nl - 1, st))]:
        untouched(call(lib, dev, fn, lspecs, args, expect=ah.E_WORKSPACE), lspecs)

