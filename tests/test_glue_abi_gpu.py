"""-m gpu: the pooling, encoding, loss and spectral-norm entry points (csrc/him_elem.hip, csrc/him_loss.hip, him_sn_* and
him_div_scalar_* of csrc/him_optim.hip) at the C ABI inside tests/abi_harness.py's guarded arena, against the float64
restatements of tests/glue_fixture.py.

Arena: every buffer of a call is a view in ONE allocation between 64 KiB bands; NaN bands beside inputs, 0xA5 bands beside
outputs and workspace, compared bit for bit afterwards; fresh outputs and the workspace are pre-filled with NaN; every
workspace has exactly the bytes its size function names; inputs are compared bit for bit after the call.

Bound (tests/README.md, direct form, per tensor): error <= max(8 * e32, 16 * 2^-24) in the metric maximum error over
maximum |ref64|.  e32 is the same metric of the fixture's float32 form; for a reduced quantity the maximum over three
float32 summation orders (glue_fixture.ORDERS).  Results the header promises exactly are compared with torch.equal against
the float32 restatement; a channel-slice writer's WHOLE destination is compared bit for bit with the prefill outside the
slice.  Nothing is excluded anywhere.  One JSON line per checked tensor goes to glue_abi_rows.jsonl in the GPU tests'
report directory before anything is asserted.

The runners take the library and the device as parameters: tests/test_glue_fixture_cpu.py passes CPU stand-ins with one
planted defect each."""
import ctypes
import os

import pytest
import torch

import abi_harness as ah
import glue_fixture as fx
from abi_harness import call, untouched
from glue_fixture import BIG, F32, F64
from test_model_gpu import OUT as REPORT_DIR

pytestmark = pytest.mark.gpu
OUT = os.path.join(REPORT_DIR, 'glue_abi_rows.jsonl')
LOG = ah.RowLog(OUT)
ROWS = LOG.rows


@pytest.fixture(autouse=True)
def _dump():
    yield
    flush()


def flush():
    LOG.flush()


def _lib():
    return ah.raw_lib()


def _st(dev):
    return ah._stream(dev)


class Checks(ah.Checks):
    def __init__(self, case):
        ah.Checks.__init__(self, case, LOG, flush=lambda: flush(), limit=fx.limit)

    def whole(self, name, got, want):
        """A prefilled destination, bit for bit: the written slice AND every channel beside it."""
        self.exact(name, ah.bits(got), ah.bits(want))


def _table(ctype, values):
    t = (ctype * len(values))(*values)
    return t, ctypes.addressof(t)


def _dims(*shape):
    return 'x'.join(map(str, shape))


# ------------------------------------------------------------------------ fill, add, scale, uint8 -> float (all exact)
def run_elementwise(lib, dev, n):
    ck = Checks('elementwise|n%d' % n)
    a, b = fx.rand(n, seed=1), fx.rand(n, seed=2)
    ar = call(lib, dev, 'him_add', {'a': ('in', a), 'b': ('in', b), 'out': ('out', (n,), None)},
              lambda P: (P('a'), P('b'), P('out'), n, _st(dev)))
    ck.exact('add', ar.t['out'], a + b)
    ar = call(lib, dev, 'him_fill', {'p': ('out', (n,), None)}, lambda P: (P('p'), n, -2.5, _st(dev)))
    ck.exact('fill', ar.t['p'], torch.full((n,), -2.5))
    ar = call(lib, dev, 'him_scale', {'p': ('out', (n,), a)}, lambda P: (P('p'), n, 0.3, _st(dev)))
    ck.exact('scale', ar.t['p'], a * torch.tensor(0.3))
    u8 = torch.arange((n + 3) // 4 * 4, dtype=torch.int64).mul(37).remainder(256).to(torch.uint8)
    ar = call(lib, dev, 'him_u8_to_f32', {'src': ('in', u8.view(F32)), 'dst': ('out', (n,), None)},
              lambda P: (P('src'), P('dst'), n, _st(dev)))
    ck.exact('u8_to_f32', ar.t['dst'], u8[:n].float())
    ck.done()


@pytest.mark.parametrize('n', [1, 100, 1025, BIG])
def test_fill_add_scale_widen(n):
    run_elementwise(_lib(), 'cuda', n)


# --------------------------------------------------------------------------------------------------- L1 / MSE means
LOSS_N = [1, 3, 255, 1025, (1 << 20) + 4, BIG]


def run_loss_fwd(lib, dev, n, offset):
    """Both means; ``offset``: operand b (L1) / x (MSE) starts one float behind a 16-byte boundary (the scalar path)."""
    ck = Checks('loss_fwd|n%d|off%d' % (n, offset))
    a, b = fx.l1_pair(n, seed=n % 1000)
    nws = int(lib.him_reduce_ws(n))
    pad = torch.cat([fx.rand(offset, seed=9), b])
    ar = call(lib, dev, 'him_l1_mean_fwd', {'a': ('in', a), 'b': ('in', pad), 'out': ('out', (1,), None), 'ws': ('ws', nws)},
              lambda P: (P('a'), P('b') + 4 * offset, n, P('out'), P('ws'), nws, _st(dev)))
    ck.row('l1', ar.t['out'], fx.l1_mean(a, b, F64), fx.orders32(lambda dt, o: fx.l1_mean(a, b, dt, o)))
    pad = torch.cat([fx.rand(offset, seed=9), a])
    for target in (0.0, 1.0):
        ar = call(lib, dev, 'him_mse_const_fwd', {'x': ('in', pad), 'out': ('out', (1,), None), 'ws': ('ws', nws)},
                  lambda P: (P('x') + 4 * offset, n, target, P('out'), P('ws'), nws, _st(dev)))
        ck.row('mse|target%d' % target, ar.t['out'], fx.mse_const(a, target, F64),
               fx.orders32(lambda dt, o: fx.mse_const(a, target, dt, o)))
    ck.done()


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('n', LOSS_N)
def test_l1_and_mse_means(n, offset):
    run_loss_fwd(_lib(), 'cuda', n, offset)


def run_loss_bwd(lib, dev, n, accumulate):
    ck = Checks('loss_bwd|n%d|acc%d' % (n, accumulate))
    a, b = fx.l1_pair(n, seed=n % 1000, relu=bool(accumulate & 2))
    g, d0 = torch.tensor([0.7]), fx.rand(n, seed=5)
    ar = call(lib, dev, 'him_l1_mean_bwd',
              {'a': ('in', a), 'b': ('in', b), 'g': ('in', g), 'da': ('out', (n,), d0 if accumulate & 1 else None)},
              lambda P: (P('a'), P('b'), n, P('g'), P('da'), accumulate, _st(dev)))
    r64, r32 = (fx.l1_bwd(a, b, 0.7, accumulate, d0, dt) for dt in (F64, F32))
    ck.row('l1 da', ar.t['da'], r64, r32)
    if not accumulate & 1:
        zero = (r64 == 0)
        ck.exact('l1 da zeros', ar.t['da'].cpu()[zero], torch.zeros(int(zero.sum())))
    if accumulate < 2:
        for target in (0.0, 1.0):
            ar = call(lib, dev, 'him_mse_const_bwd', {'x': ('in', a), 'g': ('in', g), 'dx': ('out', (n,), d0 if accumulate else None)},
                      lambda P: (P('x'), n, target, P('g'), P('dx'), accumulate, _st(dev)))
            ck.row('mse dx|target%d' % target, ar.t['dx'], fx.mse_bwd(a, target, 0.7, accumulate, d0, F64),
                   fx.mse_bwd(a, target, 0.7, accumulate, d0, F32))
    ck.done()


@pytest.mark.parametrize('accumulate', [0, 1, 2, 3])
@pytest.mark.parametrize('n', [100, 1025, BIG])
def test_l1_and_mse_backward(n, accumulate):
    run_loss_bwd(_lib(), 'cuda', n, accumulate)


MULTI_N = [1, 3, 255, BIG, 4096, 777, (1 << 16) + 4, 1025, 5, 1000, 2048, 33, 100001, 7, 256, 1023, 4097, 513]
MULTI_NULL = (7, 17)                                     # one null da in each of the two launch tables


def run_l1_multi(lib, dev, accumulate, fwd=True):
    """18 pairs = two launch tables; against float64 and, bit for bit, against the single-pair entry points."""
    ck = Checks('l1_multi|acc%d' % accumulate)
    np_ = len(MULTI_N)
    pairs = [fx.l1_pair(n, seed=10 + i, relu=True) for i, n in enumerate(MULTI_N)]
    g = fx.rand(np_, seed=3) + 2.0
    d0 = [fx.rand(n, seed=40 + i) for i, n in enumerate(MULTI_N)]
    nws = int(lib.him_l1_multi_ws(np_))
    specs = {}
    for i, (a, b) in enumerate(pairs):
        specs['a%d' % i], specs['b%d' % i] = ('in', a), ('in', b)
    keep = []

    def tables(P):
        ta, tb = (_table(ctypes.c_void_p, [P('%s%d' % (k, i)) for i in range(np_)]) for k in 'ab')
        tn = _table(ctypes.c_size_t, MULTI_N)
        keep.extend([ta, tb, tn])
        return ta[1], tb[1], tn[1]

    if fwd:
        fs = dict(specs, out=('out', (np_,), None), ws=('ws', nws))
        ar = call(lib, dev, 'him_l1_multi_fwd', fs, lambda P: tables(P) + (np_, P('out'), P('ws'), nws, _st(dev)))
        out = ar.t['out'].cpu()
        for i, (a, b) in enumerate(pairs):
            ck.row('out[%d]' % i, out[i:i + 1], fx.l1_mean(a, b, F64), fx.orders32(lambda dt, o: fx.l1_mean(a, b, dt, o)))
            n, nw1 = MULTI_N[i], int(lib.him_reduce_ws(MULTI_N[i]))
            one = call(lib, dev, 'him_l1_mean_fwd', {'a': ('in', a), 'b': ('in', b), 'out': ('out', (1,), None), 'ws': ('ws', nw1)},
                       lambda P: (P('a'), P('b'), n, P('out'), P('ws'), nw1, _st(dev)))
            ck.exact('out[%d]==single' % i, out[i:i + 1], one.t['out'].cpu())
    bs = dict(specs, g=('in', g))
    for i, n in enumerate(MULTI_N):
        if i not in MULTI_NULL:
            bs['da%d' % i] = ('out', (n,), d0[i] if accumulate & 1 else None)

    def bargs(P):
        td = _table(ctypes.c_void_p, [P('da%d' % i) if i not in MULTI_NULL else 0 for i in range(np_)])
        keep.append(td)
        return tables(P) + (np_, P('g'), td[1], accumulate, _st(dev))

    ar = call(lib, dev, 'him_l1_multi_bwd', bs, bargs)
    for i, (a, b) in enumerate(pairs):
        if i in MULTI_NULL:
            continue
        got, n = ar.t['da%d' % i].cpu(), MULTI_N[i]
        ck.row('da[%d]' % i, got, fx.l1_bwd(a, b, float(g[i]), accumulate, d0[i], F64), fx.l1_bwd(a, b, float(g[i]), accumulate, d0[i], F32))
        one = call(lib, dev, 'him_l1_mean_bwd',
                   {'a': ('in', a), 'b': ('in', b), 'g': ('in', g[i:i + 1]), 'da': ('out', (n,), d0[i] if accumulate & 1 else None)},
                   lambda P: (P('a'), P('b'), n, P('g'), P('da'), accumulate, _st(dev)))
        ck.exact('da[%d]==single' % i, got, one.t['da'].cpu())
    ck.done()


@pytest.mark.parametrize('accumulate', [0, 1, 2, 3])
def test_l1_multi_two_tables(accumulate):
    run_l1_multi(_lib(), 'cuda', accumulate, fwd=accumulate == 0)


def run_lincomb(lib, dev, n):
    ck = Checks('lincomb|n%d' % n)
    terms, w = fx.rand(n, seed=n) * 3.0, [float(v) for v in fx.rand(n, seed=50 + n)]
    scale, g = 0.37, torch.tensor([1.7])
    keep = []

    def fargs(P):
        keep.extend([_table(ctypes.c_void_p, [P('terms') + 4 * i for i in range(n)]), _table(ctypes.c_float, w)])
        return keep[0][1], keep[1][1], n, scale, P('out'), _st(dev)

    ar = call(lib, dev, 'him_lincomb_fwd', {'terms': ('in', terms), 'out': ('out', (1,), None)}, fargs)
    ck.exact('out', ar.t['out'], fx.lincomb(terms.tolist(), w, scale))
    ck.row('out/f64', ar.t['out'], (terms.double() * torch.tensor(w, dtype=F32).double()).sum().reshape(1) * float(torch.tensor(scale)),
           fx.lincomb(terms.tolist(), w, scale))
    skip = n // 2                                         # one null dterms entry (none at n == 1)
    before = fx.rand(n, seed=7)

    def bargs(P):
        keep.extend([_table(ctypes.c_void_p, [0 if (i == skip and n > 1) else P('d') + 4 * i for i in range(n)]),
                     _table(ctypes.c_float, w)])
        return P('g'), keep[-1][1], n, scale, keep[-2][1], _st(dev)

    ar = call(lib, dev, 'him_lincomb_bwd', {'g': ('in', g), 'd': ('out', (n,), before)}, bargs)
    want = fx.lincomb_bwd(float(g), w, scale)
    if n > 1:
        want[skip] = before[skip]
    ck.whole('dterms', ar.t['d'], want)
    ck.done()


@pytest.mark.parametrize('n', range(1, 9))
def test_lincomb(n):
    run_lincomb(_lib(), 'cuda', n)


# ------------------------------------------------------------------------------------------------------------ pools
AVG_SHAPES = [(3, 1, 1), (3, 1, 2), (2, 2, 3), (2, 5, 4), (3, 17, 33), (2, 16, 32), (3, 700, 999)]


def run_avgpool(lib, dev, planes, H, W):
    assert planes * H * W > fx.GRID_CAP or H < 700
    ck = Checks('avgpool|' + _dims(planes, H, W))
    OH, OW = fx.pool_out(H), fx.pool_out(W)
    x, dy = fx.rand(planes, H, W, seed=1), fx.rand(planes, OH, OW, seed=2)
    ar = call(lib, dev, 'him_avgpool3s2_fwd', {'x': ('in', x), 'y': ('out', (planes, OH, OW), None)},
              lambda P: (P('x'), P('y'), planes, H, W, OH, OW, _st(dev)))
    ck.row('y', ar.t['y'], fx.avgpool(x, F64), fx.avgpool(x, F32))
    ar = call(lib, dev, 'him_avgpool3s2_bwd', {'dy': ('in', dy), 'dx': ('out', (planes, H, W), None)},
              lambda P: (P('dy'), P('dx'), planes, H, W, OH, OW, _st(dev)))
    ck.row('dx', ar.t['dx'], fx.avgpool(x, F64, dy), fx.avgpool(x, F32, dy))
    ck.done()


@pytest.mark.parametrize('shape', AVG_SHAPES, ids=lambda s: _dims(*s))
def test_average_pool(shape):
    run_avgpool(_lib(), 'cuda', *shape)


# multiples of k; a tail in H only, in W only, in both; one tail case whose planes x H x W is above the cap
MAX_SHAPES = [(2, 3, 8, 16), (2, 2, 9, 16), (2, 2, 8, 17), (2, 3, 9, 17), (2, 2, 33, 65), (8, 2, 16, 24), (8, 2, 70, 67),
              (16, 2, 32, 48), (16, 1, 37, 50), (2, 3, 701, 999)]


def run_maxpool(lib, dev, k, planes, H, W):
    ck = Checks('maxpool|k%d|%s' % (k, _dims(planes, H, W)))
    OH, OW = H // k, W // k
    x, dy = fx.maxpool_input(planes, H, W, k), fx.rand(planes, OH, OW, seed=3)
    ar = call(lib, dev, 'him_maxpool_fwd', {'x': ('in', x), 'y': ('out', (planes, OH, OW), None)},
              lambda P: (P('x'), P('y'), planes, H, W, k, _st(dev)))
    ck.exact('y', ar.t['y'], fx.maxpool(x, k, F32))
    for fn, gate in (('him_maxpool_bwd', False), ('him_maxpool_relu_bwd', True)):
        ar = call(lib, dev, fn, {'x': ('in', x), 'dy': ('in', dy), 'dx': ('out', (planes, H, W), None)},
                  lambda P: (P('x'), P('dy'), P('dx'), planes, H, W, k, _st(dev)))
        dx = ar.t['dx'].cpu()
        ck.exact(fn[4:] + ' dx', dx, fx.maxpool(x, k, F32, dy, gate))
        ck.row(fn[4:] + ' dx/f64', dx, fx.maxpool(x, k, F64, dy, gate), fx.maxpool(x, k, F32, dy, gate))
        tail = torch.cat([dx[:, OH * k:, :].reshape(-1), dx[:, :, OW * k:].reshape(-1)])
        ck.exact(fn[4:] + ' dx tail', ah.bits(tail), torch.zeros(tail.numel(), dtype=torch.int32))
    ck.done()


@pytest.mark.parametrize('shape', MAX_SHAPES, ids=lambda s: _dims(*s))
def test_max_pool(shape):
    run_maxpool(_lib(), 'cuda', *shape)


# --------------------------------------------------------------------------------------------- channel-slice writers
PLANES = [(1, 7), (7, 1), (3, 3), (9, 13)]
SLICES = ['first', 'middle', 'last']


def _c0(where, Ctot, n):
    return {'first': 0, 'middle': 2, 'last': Ctot - n}[where]


def run_onehot(lib, dev, B, nc, where, H, W, pool=True):
    Ctot = nc + 5
    c0 = _c0(where, Ctot, nc)
    ck = Checks('onehot|%s|c0=%d of %d' % (_dims(B, nc, H, W), c0, Ctot))
    hw = H * W
    label, before = fx.label_map(B, hw, nc, seed=1), fx.rand(B, Ctot, hw, seed=2)
    ar = call(lib, dev, 'him_onehot', {'label': ('in', label), 'dst': ('out', (B, Ctot, hw), before)},
              lambda P: (P('label'), P('dst'), B, nc, Ctot, c0, hw, _st(dev)))
    ck.whole('dst', ar.t['dst'], fx.slice_write(before, c0, fx.onehot(label, nc)))
    if pool:
        OH, OW = fx.pool_out(H), fx.pool_out(W)
        pbefore = fx.rand(B, Ctot, OH, OW, seed=3)
        ar = call(lib, dev, 'him_onehot_pool3s2', {'label': ('in', label), 'dst': ('out', (B, Ctot, OH, OW), pbefore)},
                  lambda P: (P('label'), P('dst'), B, nc, Ctot, c0, H, W, OH, OW, _st(dev)))
        got = ar.t['dst'].cpu()
        full = call(lib, dev, 'him_onehot', {'label': ('in', label), 'dst': ('out', (B, nc, hw), None)},
                    lambda P: (P('label'), P('dst'), B, nc, nc, 0, hw, _st(dev))).t['dst'].cpu()
        two = call(lib, dev, 'him_avgpool3s2_fwd', {'x': ('in', full), 'y': ('out', (B, nc, OH, OW), None)},
                   lambda P: (P('x'), P('y'), B * nc, H, W, OH, OW, _st(dev))).t['y'].cpu()
        ck.whole('pool3s2==avgpool(onehot)', got, fx.slice_write(pbefore, c0, two))
        oh = fx.onehot(label, nc).view(B * nc, H, W)
        ck.row('pool3s2', got[:, c0:c0 + nc], fx.avgpool(oh, F64).view(B, nc, OH, OW), fx.avgpool(oh, F32).view(B, nc, OH, OW))
    ck.done()


@pytest.mark.parametrize('where', SLICES)
@pytest.mark.parametrize('plane', PLANES, ids=lambda s: _dims(*s))
def test_onehot_slices(plane, where):
    run_onehot(_lib(), 'cuda', 2, 4, where, *plane)


@pytest.mark.parametrize('case', [(1, 3, 'middle', 1, 85), (3, 35, 'last', 31, 33), (1, 3, 'middle', 701, 999)], ids=lambda c: _dims(*c))
def test_onehot_sizes(case):
    assert case[3] < 700 or case[0] * case[1] * case[3] * case[4] > fx.GRID_CAP
    run_onehot(_lib(), 'cuda', *case)


def run_edges(lib, dev, B, H, W, where, Ctot=4):
    c0 = _c0(where, Ctot, 1)
    ck = Checks('edges|%s|c0=%d of %d' % (_dims(B, H, W), c0, Ctot))
    inst, before = fx.inst_map(B, H, W, seed=4), fx.rand(B, Ctot, H, W, seed=5)
    ar = call(lib, dev, 'him_edges', {'inst': ('in', inst), 'dst': ('out', (B, Ctot, H, W), before)},
              lambda P: (P('inst'), P('dst'), B, H, W, Ctot, c0, _st(dev)))
    ck.whole('dst', ar.t['dst'], fx.slice_write(before, c0, fx.edges(inst).unsqueeze(1)))
    ck.done()


@pytest.mark.parametrize('where', SLICES)
@pytest.mark.parametrize('plane', PLANES + [(1, 1), (2, 2), (40, 41)], ids=lambda s: _dims(*s))
def test_edges_slices(plane, where):
    run_edges(_lib(), 'cuda', 2, *plane, where)


def test_edges_above_the_grid_cap():
    assert 701 * 2993 > fx.GRID_CAP
    run_edges(_lib(), 'cuda', 1, 701, 2993, 'first', Ctot=1)


def run_tile_embed(lib, dev, B, hw, where, Ctot=7):
    c0 = _c0(where, Ctot, 3)
    ck = Checks('tile_embed|%s|c0=%d of %d' % (_dims(B, hw), c0, Ctot))
    emb, mask, before = fx.rand(B, 3, seed=1), fx.uniform(B, hw, seed=2), fx.rand(B, Ctot, hw, seed=3)
    ar = call(lib, dev, 'him_tile_embed', {'emb': ('in', emb), 'mask': ('in', mask), 'dst': ('out', (B, Ctot, hw), before)},
              lambda P: (P('emb'), P('mask'), P('dst'), B, Ctot, c0, hw, _st(dev)))
    ck.whole('dst', ar.t['dst'], fx.slice_write(before, c0, fx.tile_embed(emb, mask)))
    ck.done()


@pytest.mark.parametrize('where', SLICES)
@pytest.mark.parametrize('hw', [7, 9, 117])
def test_tile_embed_slices(hw, where):
    run_tile_embed(_lib(), 'cuda', 2, hw, where)


def test_tile_embed_above_the_grid_cap():
    assert 3 * 699053 > fx.GRID_CAP
    run_tile_embed(_lib(), 'cuda', 1, 699053, 'first', Ctot=3)


def run_copy_channels(lib, dev, B, hw, where, mode, fractional=False, accumulate=0, n=3, Csrc=5, Cdst=7):
    cs0, cd0 = _c0(where, Csrc, n), _c0(where, Cdst, n)
    ck = Checks('copy_channels|%s|src %d of %d|dst %d of %d|mode%d%s%s' % (
        _dims(B, n, hw), cs0, Csrc, cd0, Cdst, mode, '|fractional' if fractional else '', '|acc' if accumulate else ''))
    src, before = fx.rand(B, Csrc, hw, seed=1), fx.rand(B, Cdst, hw, seed=2)
    mask = fx.uniform(B, hw, seed=3) if fractional else fx.box_mask(B, hw, seed=3)
    ar = call(lib, dev, 'him_copy_channels', {'src': ('in', src), 'mask': ('in', mask), 'dst': ('out', (B, Cdst, hw), before)},
              lambda P: (P('src'), Csrc, cs0, P('dst'), Cdst, cd0, n, B, hw, P('mask'), mode, accumulate, _st(dev)))
    got = ar.t['dst'].cpu()
    want64, want32 = (fx.copy_channels(src, cs0, n, mask, mode, dt) for dt in (F64, F32))
    if accumulate:
        want64, want32 = before[:, cd0:cd0 + n].double() + want64, before[:, cd0:cd0 + n] + want32
    if accumulate or (fractional and mode):
        ck.row('slice', got[:, cd0:cd0 + n], want64, want32)
        ck.whole('beside the slice', fx.slice_write(got, cd0, torch.zeros(B, n, hw)), fx.slice_write(before, cd0, torch.zeros(B, n, hw)))
    else:
        ck.whole('dst', got, fx.slice_write(before, cd0, want32))
    ck.done()


@pytest.mark.parametrize('where', SLICES)
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_copy_channels_slices_and_modes(mode, where):
    for hw in (7, 9, 117):
        run_copy_channels(_lib(), 'cuda', 2, hw, where, mode)
    run_copy_channels(_lib(), 'cuda', 2, 117, where, mode, fractional=True)
    run_copy_channels(_lib(), 'cuda', 2, 117, where, mode, accumulate=1)
    run_copy_channels(_lib(), 'cuda', 2, 117, where, mode, fractional=True, accumulate=1)


@pytest.mark.parametrize('mode', [0, 2])
def test_copy_channels_above_the_grid_cap(mode):
    assert 2 * 349527 * 3 > fx.GRID_CAP
    run_copy_channels(_lib(), 'cuda', 1, 349527, 'last', mode, fractional=mode == 0, n=2 * 3, Csrc=6, Cdst=6)


def run_blend(lib, dev, B, C, hw, where, fractional):
    Ca, Cb = C + 2, C + 3
    ca0, cb0 = _c0(where, Ca, C), _c0(where, Cb, C)
    ck = Checks('blend|%s|a %d of %d|b %d of %d%s' % (_dims(B, C, hw), ca0, Ca, cb0, Cb, '|fractional' if fractional else ''))
    a, b = fx.rand(B, Ca, hw, seed=1), fx.rand(B, Cb, hw, seed=2)
    m = fx.uniform(B, hw, seed=3) if fractional else fx.box_mask(B, hw, seed=3)
    ar = call(lib, dev, 'him_blend', {'a': ('in', a), 'b': ('in', b), 'm': ('in', m), 'out': ('out', (B, C, hw), None)},
              lambda P: (P('a'), Ca, ca0, P('b'), Cb, cb0, P('m'), P('out'), B, C, hw, _st(dev)))
    if fractional:
        ck.row('out', ar.t['out'], fx.blend(a, ca0, b, cb0, C, m, F64), fx.blend(a, ca0, b, cb0, C, m, F32))
    else:
        ck.exact('out', ar.t['out'], fx.blend(a, ca0, b, cb0, C, m, F32))
    ck.done()


@pytest.mark.parametrize('fractional', [False, True], ids=['binary', 'fractional'])
@pytest.mark.parametrize('where', SLICES)
def test_blend(where, fractional):
    for hw in (7, 100, 1025):
        run_blend(_lib(), 'cuda', 2, 3, hw, where, fractional)


@pytest.mark.parametrize('fractional', [False, True], ids=['binary', 'fractional'])
def test_blend_above_the_grid_cap(fractional):
    assert 699053 * 3 > fx.GRID_CAP
    run_blend(_lib(), 'cuda', 1, 3, 699053, 'first', fractional)


# ----------------------------------------------------------------------------------------------------- masked image
def run_masked_image(lib, dev, B, C, H, W, null=None):
    ck = Checks('masked_image|%s|null=%s' % (_dims(B, C, H, W), null))
    image = fx.rand(B, C, H, W, seed=1)
    boxes = [(2, 3, 5, 3), (3, 2, 4, 3), (0, 0, W, H), (4, 1, W + 5, H + 4)]        # empty, one pixel, the image, past it
    bbox = torch.tensor([boxes[b % 4] for b in range(B)], dtype=F32)
    specs = {'image': ('in', image), 'bbox': ('in', bbox)}
    shapes = {'mask': (B, 1, H, W), 'obj': (B, C, H, W), 'ctx': (B, C, H, W)}
    for k, s in shapes.items():
        if k != null:
            specs[k] = ('out', s, None)
    ar = call(lib, dev, 'him_masked_image', specs,
              lambda P: (P('image'), P('bbox'), P('mask'), P('obj'), P('ctx'), B, C, H, W, -0.25, _st(dev)))
    want = dict(zip(('mask', 'obj', 'ctx'), fx.masked_image(image, bbox, -0.25)))
    for k in shapes:
        if k != null:
            ck.exact(k, ar.t[k], want[k])
    ck.done()


@pytest.mark.parametrize('null', [None, 'mask', 'obj', 'ctx'])
def test_masked_image_boxes_and_null_outputs(null):
    run_masked_image(_lib(), 'cuda', 4, 1, 5, 7, null)
    run_masked_image(_lib(), 'cuda', 4, 3, 9, 13, null)


def test_masked_image_above_the_grid_cap():
    assert 3 * 700 * 999 > fx.GRID_CAP
    run_masked_image(_lib(), 'cuda', 1, 3, 700, 999)


# ------------------------------------------------------------------------------------------------------ masked mean
def run_masked_mean(lib, dev, hw, kind, with_noise, B=2):
    ck = Checks('masked_mean|hw%d|%s|noise%d' % (hw, kind, with_noise))
    image = fx.rand(B, 3, hw, seed=hw) * 0.3 + torch.tensor([0.6, -0.6, 0.1]).view(1, 3, 1)
    mask = fx.mean_mask(kind, B, hw, seed=hw + 1)
    noise = torch.tensor([[3.0, 3.0, 1.01], [0.97, -3.0, -3.0]]) if with_noise else None
    specs = {'image': ('in', image), 'mask': ('in', mask), 'emb': ('out', (B, 3), None)}
    if with_noise:
        specs['noise'] = ('in', noise)
    ar = call(lib, dev, 'him_masked_mean', specs, lambda P: (P('image'), P('mask'), P('noise'), P('emb'), B, hw, _st(dev)))
    ck.row('emb', ar.t['emb'], fx.masked_mean(image, mask, noise, F64), fx.orders32(lambda dt, o: fx.masked_mean(image, mask, noise, dt, o)))
    if kind == 'empty':
        ck.exact('emb zeros', ar.t['emb'], torch.zeros(B, 3))
    ck.done()


@pytest.mark.parametrize('with_noise', [0, 1])
@pytest.mark.parametrize('kind', fx.MASK_KINDS)
@pytest.mark.parametrize('hw', [1, 100, 256, 5000])
def test_masked_mean(hw, kind, with_noise):
    run_masked_mean(_lib(), 'cuda', hw, kind, with_noise)


# ---------------------------------------------------------------------------------------------------- spectral norm
_SN_REF = {}


def _sn_ref(rows, cols, scale):
    key = (rows, cols, scale)
    if key not in _SN_REF:
        W, u = fx.sn_case(rows, cols, scale)
        _SN_REF[key] = (W, u, fx.sn_chain(W, u, F64, g_sigma=0.7), [fx.sn_chain(W, u, F32, o, g_sigma=0.7) for o in fx.ORDERS])
    return _SN_REF[key]


def run_sn(lib, dev, rows, cols, accumulate=0, chained=False, scale=1.0):
    ck = Checks('sn|%dx%d|scale%g%s%s' % (rows, cols, scale, '|acc' if accumulate else '', '|chained' if chained else ''))
    W, u, r64, r32 = _sn_ref(rows, cols, scale)
    nws = int(lib.him_sn_ws(rows, cols))
    ar = call(lib, dev, 'him_sn_power_iter_fwd',
              {'W': ('in', W), 'u': ('in', u), 'v': ('out', (cols,), None), 'u_out': ('out', (rows,), None),
               'sigma': ('out', (1,), None), 'ws': ('ws', nws)},
              lambda P: (P('W'), P('u'), rows, cols, P('v'), P('u_out'), P('sigma'), P('ws'), nws, _st(dev)))
    got = {k: ar.t[k].cpu() for k in ('v', 'u_out', 'sigma')}
    for k in got:
        ck.row(k, got[k], r64[k], [r[k] for r in r32])
    fed = got if chained else {k: r64[k].float() for k in got}
    if not all(bool(torch.isfinite(t).all()) for t in fed.values()):
        ck.done()
    g, d0 = torch.tensor([0.7]), fx.rand(rows, cols, seed=9, scale=float(r64['dW'].abs().max()))
    ar = call(lib, dev, 'him_sn_power_iter_bwd',
              {'W': ('in', W), 'u': ('in', u), 'v': ('in', fed['v']), 'u_out': ('in', fed['u_out']), 'sigma': ('in', fed['sigma']),
               'g': ('in', g), 'dW': ('out', (rows, cols), d0 if accumulate else None), 'ws': ('ws', nws)},
              lambda P: (P('W'), P('u'), P('v'), P('u_out'), P('sigma'), P('g'), rows, cols, P('dW'), accumulate, P('ws'), nws,
                         _st(dev)))
    ck.row('dW', ar.t['dW'], r64['dW'] + (d0.double() if accumulate else 0), [r['dW'] + (d0 if accumulate else 0) for r in r32])
    ck.done()


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('shape', fx.SN_SHAPES, ids=lambda s: _dims(*s))
def test_spectral_norm(shape, accumulate):
    assert 513 * 4100 > fx.GRID_CAP
    run_sn(_lib(), 'cuda', *shape, accumulate=accumulate)
    if not accumulate:
        run_sn(_lib(), 'cuda', *shape, chained=True)


@pytest.mark.parametrize('shape', [(1, 8192), (16, 72)], ids=lambda s: _dims(*s))
def test_spectral_norm_where_the_eps_counts(shape):
    """|s| and |t| of the order 1e-8: the 1e-12 of both normalisations is 1e-4 of the result."""
    run_sn(_lib(), 'cuda', *shape, scale=1e-10)


def run_sn_zero(lib, dev, rows, cols, accumulate):
    ck = Checks('sn|%dx%d|W=0%s' % (rows, cols, '|acc' if accumulate else ''))
    W, u = torch.zeros(rows, cols), fx.rand(rows, seed=2)
    nws = int(lib.him_sn_ws(rows, cols))
    ar = call(lib, dev, 'him_sn_power_iter_fwd',
              {'W': ('in', W), 'u': ('in', u), 'v': ('out', (cols,), None), 'u_out': ('out', (rows,), None),
               'sigma': ('out', (1,), None), 'ws': ('ws', nws)},
              lambda P: (P('W'), P('u'), rows, cols, P('v'), P('u_out'), P('sigma'), P('ws'), nws, _st(dev)))
    zeros = {'v': torch.zeros(cols), 'u_out': torch.zeros(rows), 'sigma': torch.zeros(1)}
    for k, z in zeros.items():
        ck.exact(k, ar.t[k], z)
    g, d0 = torch.tensor([0.7]), fx.rand(rows, cols, seed=9)
    ar = call(lib, dev, 'him_sn_power_iter_bwd',
              dict({k: ('in', z) for k, z in zeros.items()}, W=('in', W), u=('in', u), g=('in', g),
                   dW=('out', (rows, cols), d0 if accumulate else None), ws=('ws', nws)),
              lambda P: (P('W'), P('u'), P('v'), P('u_out'), P('sigma'), P('g'), rows, cols, P('dW'), accumulate, P('ws'), nws,
                         _st(dev)))
    ck.exact('dW', ar.t['dW'], d0 if accumulate else torch.zeros(rows, cols))
    ck.done()


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('shape', [(1, 300), (16, 72), (300, 48)], ids=lambda s: _dims(*s))
def test_spectral_norm_of_a_zero_weight(shape, accumulate):
    run_sn_zero(_lib(), 'cuda', *shape, accumulate)


def div_scalar_ws(n):
    """include/him.h: min(ceil(n / 1024), 1024) floats."""
    return min((n + 1023) // 1024, 1024) * 4


def run_div_scalar(lib, dev, n, accumulate):
    ck = Checks('div_scalar|n%d%s' % (n, '|acc' if accumulate else ''))
    W, sigma, dout, d0 = fx.rand(n, seed=1), torch.tensor([1.7]), fx.rand(n, seed=2), fx.rand(n, seed=3)
    ar = call(lib, dev, 'him_div_scalar_fwd', {'W': ('in', W), 'sigma': ('in', sigma), 'out': ('out', (n,), None)},
              lambda P: (P('W'), P('sigma'), P('out'), n, _st(dev)))
    ck.row('out', ar.t['out'], fx.div_scalar(W, sigma, F64), fx.div_scalar(W, sigma, F32))
    nws = div_scalar_ws(n)
    ar = call(lib, dev, 'him_div_scalar_bwd',
              {'W': ('in', W), 'sigma': ('in', sigma), 'dout': ('in', dout), 'dW': ('out', (n,), d0 if accumulate else None),
               'dsigma': ('out', (1,), None), 'ws': ('ws', nws)},
              lambda P: (P('W'), P('sigma'), P('dout'), P('dW'), P('dsigma'), n, accumulate, P('ws'), nws, _st(dev)))
    r64 = fx.div_scalar_bwd(W, sigma, dout, accumulate, d0, F64)
    r32 = fx.orders32(lambda dt, o: fx.div_scalar_bwd(W, sigma, dout, accumulate, d0, dt, o))
    ck.row('dW', ar.t['dW'], r64[0], r32[0][0])
    ck.row('dsigma', ar.t['dsigma'], r64[1], [r[1] for r in r32])
    ck.done()


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('n', [1, 1025, BIG])
def test_div_scalar(n, accumulate):
    run_div_scalar(_lib(), 'cuda', n, accumulate)


# ----------------------------------------------------------------------------------------------------- return codes
def refusals(lib, dev):
    """(fn, argument builder, code): every one returns before any launch (read off the C source)."""
    st = _st(dev)
    nr, ns = int(lib.him_reduce_ws(12)), int(lib.him_sn_ws(3, 4))
    I, W = ah.E_INVALID, ah.E_WORKSPACE
    x, y, z, ws = 'x', 'y', 'z', 'ws'
    return [
        # a slice out of range
        ('him_onehot', lambda P: (P(x), P(y), 1, 3, 4, 2, 4, st), I), ('him_onehot', lambda P: (P(x), P(y), 1, 3, 4, -1, 4, st), I),
        ('him_onehot_pool3s2', lambda P: (P(x), P(y), 1, 3, 4, 2, 2, 2, 1, 1, st), I),
        ('him_edges', lambda P: (P(x), P(y), 1, 2, 2, 3, 3, st), I), ('him_edges', lambda P: (P(x), P(y), 1, 2, 2, 3, -1, st), I),
        ('him_tile_embed', lambda P: (P(x), P(z), P(y), 1, 4, 2, 4, st), I),
        ('him_copy_channels', lambda P: (P(x), 3, 2, P(y), 4, 0, 2, 1, 4, 0, 0, 0, st), I),
        ('him_copy_channels', lambda P: (P(x), 3, 0, P(y), 4, 3, 2, 1, 4, 0, 0, 0, st), I),
        ('him_copy_channels', lambda P: (P(x), 3, 0, P(y), 4, 0, 2, 1, 4, 0, 1, 0, st), I),       # mask_mode without a mask
        ('him_blend', lambda P: (P(x), 3, 2, P(z), 3, 0, P(z), P(y), 1, 2, 4, st), I),
        ('him_blend', lambda P: (P(x), 3, 0, P(z), 3, -1, P(z), P(y), 1, 2, 4, st), I),
        # bad OH / OW
        ('him_avgpool3s2_fwd', lambda P: (P(x), P(y), 1, 3, 4, 1, 2, st), I), ('him_avgpool3s2_fwd', lambda P: (P(x), P(y), 1, 3, 4, 2, 3, st), I),
        ('him_avgpool3s2_bwd', lambda P: (P(x), P(y), 1, 3, 4, 3, 2, st), I),
        ('him_onehot_pool3s2', lambda P: (P(x), P(y), 1, 3, 3, 0, 3, 4, 2, 3, st), I),
        # k <= 0, or larger than the plane
        ('him_maxpool_fwd', lambda P: (P(x), P(y), 1, 3, 4, 0, st), I), ('him_maxpool_fwd', lambda P: (P(x), P(y), 1, 3, 4, 4, st), I),
        ('him_maxpool_bwd', lambda P: (P(x), P(z), P(y), 1, 3, 4, -2, st), I),
        ('him_maxpool_relu_bwd', lambda P: (P(x), P(z), P(y), 1, 3, 4, 0, st), I),
        # a workspace too small, n == 0
        ('him_l1_mean_fwd', lambda P: (P(x), P(z), 12, P(y), P(ws), nr - 1, st), W), ('him_l1_mean_fwd', lambda P: (P(x), P(z), 12, P(y), 0, nr, st), W),
        ('him_mse_const_fwd', lambda P: (P(x), 12, 1.0, P(y), P(ws), nr - 1, st), W),
        ('him_l1_mean_fwd', lambda P: (P(x), P(z), 0, P(y), P(ws), nr, st), I), ('him_mse_const_fwd', lambda P: (P(x), 0, 1.0, P(y), P(ws), nr, st), I),
        ('him_sn_power_iter_fwd', lambda P: (P(x), P(z), 3, 4, P(y), P(y), P(y), P(ws), ns - 1, st), W),
        ('him_sn_power_iter_bwd', lambda P: (P(x), P(z), P(z), P(z), P(z), P(z), 3, 4, P(y), 0, P(ws), ns - 1, st), W),
        ('him_sn_power_iter_fwd', lambda P: (P(x), P(z), 0, 4, P(y), P(y), P(y), P(ws), ns, st), I),
        ('him_sn_power_iter_bwd', lambda P: (P(x), P(z), P(z), P(z), P(z), P(z), 3, -4, P(y), 0, P(ws), ns, st), I),
        ('him_div_scalar_bwd', lambda P: (P(x), P(z), P(z), P(y), P(y), 2000, 0, P(ws), 2 * 4 - 1, st), W),
        # lincomb with n outside 1..8 (refused before the tables are read)
        ('him_lincomb_fwd', lambda P: (P(x), P(z), 0, 1.0, P(y), st), I), ('him_lincomb_fwd', lambda P: (P(x), P(z), 9, 1.0, P(y), st), I),
        ('him_lincomb_bwd', lambda P: (P(x), P(z), 9, 1.0, P(y), st), I), ('him_lincomb_bwd', lambda P: (P(x), P(z), -1, 1.0, P(y), st), I),
        # non-positive B / planes / hw / H / W
        ('him_masked_mean', lambda P: (P(x), P(z), 0, P(y), 0, 4, st), I), ('him_masked_mean', lambda P: (P(x), P(z), 0, P(y), -1, 4, st), I),
        ('him_masked_mean', lambda P: (P(x), P(z), 0, P(y), 1, 0, st), I),
        ('him_masked_image', lambda P: (P(x), P(z), P(y), 0, 0, 1, 1, 0, 4, 0.0, st), I),
        ('him_onehot', lambda P: (P(x), P(y), 0, 3, 4, 0, 4, st), I), ('him_onehot', lambda P: (P(x), P(y), 1, 0, 4, 0, 4, st), I),
        ('him_onehot', lambda P: (P(x), P(y), 1, 3, 4, 0, 0, st), I),
        ('him_onehot_pool3s2', lambda P: (P(x), P(y), 0, 3, 4, 0, 2, 2, 1, 1, st), I),
        ('him_onehot_pool3s2', lambda P: (P(x), P(y), 1, 3, 4, 0, 0, 2, 0, 1, st), I),
        ('him_edges', lambda P: (P(x), P(y), 1, 0, 2, 3, 0, st), I), ('him_edges', lambda P: (P(x), P(y), -1, 2, 2, 3, 0, st), I),
        ('him_tile_embed', lambda P: (P(x), P(z), P(y), 0, 4, 0, 4, st), I), ('him_tile_embed', lambda P: (P(x), P(z), P(y), 1, 4, 0, 0, st), I),
        ('him_copy_channels', lambda P: (P(x), 3, 0, P(y), 4, 0, 2, 0, 4, 0, 0, 0, st), I),
        ('him_copy_channels', lambda P: (P(x), 3, 0, P(y), 4, 0, 2, 1, -4, 0, 0, 0, st), I),
        ('him_copy_channels', lambda P: (P(x), 3, 0, P(y), 4, 0, -1, 1, 4, 0, 0, 0, st), I),
        ('him_blend', lambda P: (P(x), 3, 0, P(z), 3, 0, P(z), P(y), 0, 2, 4, st), I),
        ('him_blend', lambda P: (P(x), 3, 0, P(z), 3, 0, P(z), P(y), 1, 2, 0, st), I),
        ('him_avgpool3s2_fwd', lambda P: (P(x), P(y), 0, 3, 4, 2, 2, st), I), ('him_avgpool3s2_bwd', lambda P: (P(x), P(y), 1, 0, 4, 0, 2, st), I),
        ('him_maxpool_fwd', lambda P: (P(x), P(y), 0, 3, 4, 2, st), I), ('him_maxpool_bwd', lambda P: (P(x), P(z), P(y), -1, 3, 4, 2, st), I),
        # a null pointer with work to do
        ('him_add', lambda P: (P(x), 0, P(y), 4, st), I), ('him_fill', lambda P: (0, 4, 1.0, st), I), ('him_scale', lambda P: (0, 4, 1.0, st), I),
        ('him_u8_to_f32', lambda P: (0, P(y), 4, st), I),
        ('him_masked_mean', lambda P: (P(x), 0, 0, P(y), 1, 4, st), I), ('him_masked_mean', lambda P: (P(x), P(z), 0, 0, 1, 4, st), I),
        ('him_masked_image', lambda P: (P(x), 0, P(y), 0, 0, 1, 1, 2, 2, 0.0, st), I),
        ('him_onehot', lambda P: (0, P(y), 1, 3, 4, 0, 4, st), I), ('him_onehot_pool3s2', lambda P: (P(x), 0, 1, 3, 4, 0, 2, 2, 1, 1, st), I),
        ('him_edges', lambda P: (P(x), 0, 1, 2, 2, 3, 0, st), I), ('him_tile_embed', lambda P: (P(x), 0, P(y), 1, 4, 0, 4, st), I),
        ('him_copy_channels', lambda P: (0, 3, 0, P(y), 4, 0, 2, 1, 4, 0, 0, 0, st), I),
        ('him_blend', lambda P: (P(x), 3, 0, P(z), 3, 0, 0, P(y), 1, 2, 4, st), I),
        ('him_avgpool3s2_fwd', lambda P: (P(x), 0, 1, 3, 4, 2, 2, st), I), ('him_avgpool3s2_bwd', lambda P: (0, P(y), 1, 3, 4, 2, 2, st), I),
        ('him_maxpool_fwd', lambda P: (0, P(y), 1, 3, 4, 2, st), I), ('him_maxpool_relu_bwd', lambda P: (P(x), 0, P(y), 1, 3, 4, 2, st), I),
        ('him_sn_power_iter_fwd', lambda P: (P(x), 0, 3, 4, P(y), P(y), P(y), P(ws), ns, st), I),
        ('him_sn_power_iter_bwd', lambda P: (P(x), P(z), 0, P(z), P(z), P(z), 3, 4, P(y), 0, P(ws), ns, st), I),
        ('him_div_scalar_fwd', lambda P: (P(x), 0, P(y), 4, st), I),
        ('him_div_scalar_bwd', lambda P: (P(x), P(z), P(z), P(y), 0, 4, 0, P(ws), 4, st), I),
    ]


def run_refusals(lib, dev):
    specs = {'x': ('in', fx.rand(64, seed=1)), 'z': ('in', fx.rand(64, seed=2)), 'y': ('out', (64,), fx.rand(64, seed=3)),
             'ws': ('ws', 4096)}
    for fn, args, code in refusals(lib, dev):
        untouched(call(lib, dev, fn, specs, args, expect=code), specs)
    # npairs <= 0: nothing to do, nothing read, nothing written
    for fn, args in (('him_l1_multi_fwd', lambda P: (0, 0, 0, 0, P('y'), P('ws'), 4096, _st(dev))),
                     ('him_l1_multi_bwd', lambda P: (0, 0, 0, -1, P('x'), 0, 0, _st(dev)))):
        untouched(call(lib, dev, fn, specs, args, expect=0), specs)
    t = _table(ctypes.c_void_p, [0])
    untouched(call(lib, dev, 'him_l1_multi_fwd', specs, lambda P: (t[1], t[1], t[1], 1, P('y'), P('ws'), 4096 - 1, _st(dev)),
                   expect=ah.E_WORKSPACE), specs)


def test_refused_calls_write_nothing():
    run_refusals(_lib(), 'cuda')
