"""him_grad_stats / him_adam_guarded_step at the C ABI, in guarded arenas (abi_harness.Arena).

Every buffer of a call lives between two guard bands; after each call the return code and the bands are checked.

Bounds.  Sums of squares: every square of an fp32 value is exact in double, so the device's sum differs from the exact sum
(math.fsum of the exact squares) by at most (count - 1) roundings of a partial sum that never exceeds the total: relative
error <= count * 2^-53, the linear-summation bound, whatever the order.  st[2] / st[3]: the double formulas applied to the
device's OWN st[0], sqrt to 1 ulp of double, the coefficient to the bit of its fp32 value.  The guarded Adam step: bit for
bit against him_adam_step / him_adam_ema_step (the same kernel body)."""
import math

import pytest
import torch

import abi_harness as H

pytestmark = pytest.mark.gpu

CH = 16384                      # optim.GUARD_CHUNK
BIG = 4096 * 256 + 77
SIZES = [1, 63, 64, 65, 255, 256, 257, CH - 1, CH, CH + 1, BIG]
U = 2.0 ** -53
HP = dict(lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8)


def test_chunk_size_is_the_librarys():
    from neurips18_hierchical_image_manipulation_amd.optim import GUARD_CHUNK
    assert GUARD_CHUNK == CH


def _g(n, seed=0, scale=0.1):
    return torch.randn(n, generator=torch.Generator().manual_seed(2000 + seed)) * scale


def _as_f32(t):
    return t.contiguous().view(torch.float32)


class Stats(object):
    """One guarded arena for him_grad_stats: g behind ``off`` floats of NaN slack, the int64 table, seg_out, st, ws."""

    def __init__(self, lib, g, off=0, seg=(), st0=None, ws_bytes=None):
        self.lib, self.n, self.off, self.seg = lib, g.numel(), off, [tuple(s) for s in seg]
        self.nseg = len(self.seg)
        need = int(lib.him_grad_stats_ws(self.n, self.nseg))
        self.ws_bytes = need if ws_bytes is None else ws_bytes
        specs = {'g': ('in', torch.cat([torch.full((off,), float('nan')), g]))}
        if self.nseg:
            specs['seg'] = ('in', _as_f32(torch.tensor(self.seg, dtype=torch.int64)))
            specs['seg_out'] = ('out', (4 * self.nseg,), None)
        specs['st'] = ('out', (16,), _as_f32(torch.zeros(8, dtype=torch.float64) if st0 is None else st0))
        specs['ws'] = ('ws', max(self.ws_bytes, 8))
        self.ar = H.Arena('cuda', specs)

    def gptr(self):
        return self.ar.ptr('g') + 4 * self.off

    def set_g(self, g):
        self.ar.t['g'][self.off:].copy_(g)

    def call(self, max_norm=0.0, row='stats'):
        ar = self.ar
        rc = self.lib.him_grad_stats(self.gptr(), self.n, ar.ptr('seg'), self.nseg, ar.ptr('seg_out'), ar.ptr('st'),
                                     max_norm, ar.ptr('ws'), self.ws_bytes, H._stream('cuda'))
        H._finish(self.lib, '%s n=%d off=%d nseg=%d' % (row, self.n, self.off, self.nseg), rc, ar, 'cuda')
        assert bool(torch.isnan(ar.t['g'][:self.off]).all()), 'the element in front of g was written'
        return self

    def st(self):
        return self.ar.t['st'].view(torch.float64).cpu().tolist()

    def st_bits(self):
        return self.ar.t['st'].view(torch.int64).cpu().tolist()

    def seg_out(self):
        return self.ar.t['seg_out'].view(torch.float64).view(-1, 2).cpu().tolist() if self.nseg else []

    def seg_bits(self):
        return self.ar.t['seg_out'].view(torch.int64).cpu().tolist() if self.nseg else []


def _exact(g):
    """(exact sum of squares of the finite elements, rounded once; finite count; non-finite count) in float64."""
    d = g.double()
    fin = torch.isfinite(d)
    sq = (d[fin] * d[fin]).tolist()              # exact products
    return math.fsum(sq), len(sq), int((~fin).sum())


def _check_sum(what, got, g):
    ref, cnt, bad = _exact(g)
    bound = max(cnt, 1) * U * ref
    err = abs(got[0] - ref)
    print('%s: sum %.17g ref %.17g err/bound %.3f (count %d)' % (what, got[0], ref, err / bound if bound else 0.0, cnt))
    assert math.isfinite(got[0]) and err <= bound, (what, got[0], ref, err, bound)
    assert got[1] == float(bad), (what, got[1], bad)


def _coef(st0, max_norm):
    """The clip rule in double from the device's own sum, rounded to fp32 once and widened."""
    if max_norm <= 0.0 or math.isinf(max_norm):
        return 1.0
    c = min(1.0, max_norm / (math.sqrt(st0) + 1e-6))
    return float(torch.tensor(c, dtype=torch.float64).float())


def _check_st(what, st, g, max_norm):
    _check_sum(what + ' st', st, g)
    ref2 = math.sqrt(st[0])
    assert abs(st[2] - ref2) <= math.ulp(ref2), (what, st[2], ref2)
    assert st[3] == _coef(st[0], max_norm), (what, st[3], _coef(st[0], max_norm))
    assert st[6] == 0.0 and st[7] == 0.0


def _table(lens):
    """Slot-aligned (64-float) segments of these lengths, zero padding between them -> (seg, n)."""
    seg, off = [], 0
    for n in lens:
        seg.append((off, n))
        off += (n + 63) // 64 * 64
    return seg, off


def _fill(seg, n, seed=0, pad=0.0):
    g = torch.full((n,), pad)
    vals = _g(n, seed)
    for b, ln in seg:
        g[b:b + ln] = vals[b:b + ln]
    return g


SMALL_TABLE = [1, 63, 64, 65, 0, 255, 257, CH - 1, CH, CH + 1, 3 * CH + 5, 256]     # zero-length and multi-chunk included
BIG_TABLE = [65, BIG, 0, 1]


# ------------------------------------------------------------------------------------------------------------- stats
@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('n', SIZES)
def test_stats_of_a_plain_buffer(n, off):
    lib = H.raw_lib()
    g = _g(n, seed=n % 97)
    true_norm = math.sqrt(_exact(g)[0])
    s = Stats(lib, g, off)
    for k, max_norm in enumerate((0.0, float('inf'), 2.0 * true_norm, 0.5 * true_norm)):
        st = s.call(max_norm).st()
        _check_st('n=%d off=%d max_norm=%g' % (n, off, max_norm), st, g, max_norm)
        assert st[4] == k + 1 and st[5] == 0.0
    assert 0.0 < st[3] <= 0.5                              # the last call clips
    first = s.st_bits()[:4]
    assert s.call(0.5 * true_norm).st_bits()[:4] == first, 'two identical calls differ'
    # the same values behind the other alignment: the same bits (the order of the additions does not follow the pointer)
    other = Stats(lib, g, 1 - off).call(0.5 * true_norm)
    assert other.st_bits()[:4] == first


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('lens', [SMALL_TABLE, BIG_TABLE], ids=['small', 'big'])
def test_stats_with_a_segment_table(lens, off):
    lib = H.raw_lib()
    seg, n = _table(lens)
    g = _fill(seg, n, seed=5)
    s = Stats(lib, g, off, seg).call(1.0)
    _check_st('table off=%d' % off, s.st(), g, 1.0)
    out = s.seg_out()
    for i, (b, ln) in enumerate(seg):
        _check_sum('segment %d [%d, +%d)' % (i, b, ln), out[i], g[b:b + ln])
    assert out[lens.index(0)] == [0.0, 0.0]
    bits = (s.st_bits()[:4], s.seg_bits())
    assert (s.call(1.0).st_bits()[:4], s.seg_bits()) == bits, 'two identical calls differ'
    # padding that is NOT zero belongs to no segment but to the whole
    g2 = _fill(seg, n, seed=5, pad=3.0)
    s2 = Stats(lib, g2, off, seg).call(1.0)
    _check_st('table with padding off=%d' % off, s2.st(), g2, 1.0)
    assert s2.seg_bits() == bits[1]
    assert s2.st()[0] > s.st()[0]


def test_values_up_to_1e30_need_the_double_accumulator():
    lib = H.raw_lib()
    n = 3 * CH + 5
    g = _g(n, seed=3, scale=1.0)
    g = g / g.abs().max() * 1e30
    assert not math.isfinite(float((g * g).sum()))            # an fp32 accumulator overflows
    seg = [(0, CH + 1), (CH + 64, 2 * CH - 59)]
    s = Stats(lib, g, 1, seg).call(1.0)
    _check_st('1e30', s.st(), g, 1.0)
    for i, (b, ln) in enumerate(seg):
        _check_sum('1e30 segment %d' % i, s.seg_out()[i], g[b:b + ln])
    assert 0.0 < s.st()[3] < 1e-29


@pytest.mark.parametrize('off', [0, 1])
def test_non_finite_elements_are_counted_and_left_out(off):
    lib = H.raw_lib()
    seg, n = _table(SMALL_TABLE)
    assert seg[-1][0] + seg[-1][1] == n
    clean = _fill(seg, n, seed=8)
    g = clean.clone()
    big = SMALL_TABLE.index(3 * CH + 5)
    mid = seg[big][0] + seg[big][1] // 2
    g[0], g[n - 1], g[mid] = float('nan'), float('inf'), float('-inf')
    s = Stats(lib, g, off, seg).call(1.0)
    st, out = s.st(), s.seg_out()
    _check_st('non-finite off=%d' % off, st, g, 1.0)
    assert st[1] == 3.0 and (st[4], st[5]) == (1.0, 1.0)
    for i, (b, ln) in enumerate(seg):
        _check_sum('non-finite segment %d' % i, out[i], g[b:b + ln])
    assert [o[1] for o in out] == [1.0 if i in (0, big, len(seg) - 1) else 0.0 for i in range(len(seg))]
    # the counters run across calls: clean, dirty, clean on one st
    s.set_g(clean)
    assert s.call(1.0).st()[4:6] == [2.0, 1.0] and s.st()[1] == 0.0
    s.set_g(g)
    assert s.call(1.0).st()[4:6] == [3.0, 2.0]
    s.set_g(clean)
    assert s.call(1.0).st()[4:6] == [4.0, 2.0]


# ------------------------------------------------------------------------------------------------------ guarded step
NAMES = ('p', 'g', 'm', 'v', 'ema')


def _inputs(n, seed=0):
    gen = torch.Generator().manual_seed(1000 + seed)
    r = lambda s=1.0: torch.randn(n, generator=gen) * s      # noqa: E731
    return dict(p=r(), g=r(0.1), m=r(0.05), v=r(0.01).abs(), ema=r())


class Bufs(object):
    """The five Adam buffers in one guarded arena, ``off`` floats of NaN slack in front of each."""

    def __init__(self, vals, off):
        self.n, self.off = vals['p'].numel(), off
        specs = {k: ('out', (self.n + off,), torch.cat([torch.full((off,), float('nan')), vals[k]])) for k in NAMES}
        self.ar = H.Arena('cuda', specs)

    def ptr(self, k):
        return self.ar.ptr(k) + 4 * self.off

    def get(self, k):
        return self.ar.t[k][self.off:].cpu()

    def check(self, lib, row, rc):
        H._finish(lib, row, rc, self.ar, 'cuda')
        for k, t in self.ar.t.items():
            assert bool(torch.isnan(t[:self.off]).all()), '%s: the element in front of %s was written' % (row, k)


def _plain(lib, vals, off, hp, step, ema):
    b = Bufs(vals, off)
    args = (b.n, hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], step)
    if ema:
        rc = lib.him_adam_ema_step(b.ptr('p'), b.ptr('g'), b.ptr('m'), b.ptr('v'), b.ptr('ema'), *args, 0.999,
                                   H._stream('cuda'))
    else:
        rc = lib.him_adam_step(b.ptr('p'), b.ptr('g'), b.ptr('m'), b.ptr('v'), *args, H._stream('cuda'))
    b.check(lib, 'unguarded n=%d' % b.n, rc)
    return b


def _guarded(lib, vals, off, hp, step, ema, st_ptr):
    b = Bufs(vals, off)
    rc = lib.him_adam_guarded_step(b.ptr('p'), b.ptr('g'), b.ptr('m'), b.ptr('v'), b.ptr('ema') if ema else 0, b.n, hp['lr'],
                                   hp['beta1'], hp['beta2'], hp['eps'], step, 0.999, st_ptr, H._stream('cuda'))
    b.check(lib, 'guarded n=%d' % b.n, rc)
    return b


def _same(what, a, b, vals, ema):
    for k in ('p', 'm', 'v') + (('ema',) if ema else ()):
        assert torch.equal(a.get(k), b.get(k)), '%s: %s differs' % (what, k)
    if not ema:
        assert torch.equal(b.get('ema'), vals['ema']), '%s: ema was written without an ema pointer' % what
    assert torch.equal(b.get('g'), a.get('g')), '%s: the gradient buffer was modified' % what


@pytest.mark.parametrize('n', [1, 63, 257, BIG])
def test_guarded_step(n):
    lib = H.raw_lib()
    off = 0 if n == 257 else 1
    vals = _inputs(n, seed=n % 89)
    g = vals['g']
    norm = math.sqrt(_exact(g)[0])
    dirty = dict(vals, g=g.clone())
    dirty['g'][n // 2] = float('inf')
    # the four decisions, each left in device memory by a statistics pass of its own
    s_off = Stats(lib, g, off).call(0.0)
    s_below = Stats(lib, g, off).call(2.0 * norm)
    s_above = Stats(lib, g, off).call(0.5 * norm)
    s_skip = Stats(lib, dirty['g'], off).call(0.5 * norm)
    assert s_off.st()[3] == 1.0 and s_below.st()[3] == 1.0 and s_skip.st()[1] == 1.0
    c = s_above.st()[3]
    assert 0.0 < c <= 0.5 and c == float(torch.tensor(c).float())
    # fl32(g * c) on the host: the product of two fp32 values is exact in double, one rounding to fp32
    scaled = dict(vals, g=(g.double() * c).float())
    for ema in (False, True):
        for step, beta1 in [(s, b1) for s in (1, 1000) for b1 in (0.5, 0.0)]:
            hp = dict(HP, beta1=beta1)
            what = 'n=%d ema=%d step=%d beta1=%g' % (n, ema, step, beta1)
            ref = _plain(lib, vals, off, hp, step, ema)
            assert not torch.equal(ref.get('p'), vals['p'])
            _same(what + ' clipping off', ref, _guarded(lib, vals, off, hp, step, ema, s_off.ar.ptr('st')), vals, ema)
            _same(what + ' below max_norm', ref, _guarded(lib, vals, off, hp, step, ema, s_below.ar.ptr('st')), vals, ema)
            got = _guarded(lib, vals, off, hp, step, ema, s_above.ar.ptr('st'))
            want = _plain(lib, scaled, off, hp, step, ema)
            for k in ('p', 'm', 'v') + (('ema',) if ema else ()):
                assert torch.equal(got.get(k), want.get(k)), '%s clipped: %s differs from the pre-scaled step' % (what, k)
            assert torch.equal(got.get('g'), g), what + ': clipping rewrote the gradient'
            if n > 1:
                assert not torch.equal(got.get('m'), ref.get('m'))
            skipped = _guarded(lib, dirty, off, hp, step, ema, s_skip.ar.ptr('st'))
            for k in NAMES:
                a, b = skipped.get(k), dirty[k]
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), '%s skipped: %s changed' % (what, k)


# ------------------------------------------------------------------------------------------------------ return codes
def test_return_codes_and_refused_calls_write_nothing():
    lib = H.raw_lib()
    n = CH + 1
    seg = [(0, 65), (128, CH - 127)]
    g = _g(n)
    mark = torch.arange(1.0, 9.0, dtype=torch.float64)
    s = Stats(lib, g, 0, seg, st0=mark)
    ar, stream = s.ar, H._stream('cuda')
    G, SEG, OUT, STP, WS, nb = s.gptr(), ar.ptr('seg'), ar.ptr('seg_out'), ar.ptr('st'), ar.ptr('ws'), s.ws_bytes
    invalid = {
        'nseg < 0': lib.him_grad_stats(G, n, SEG, -1, OUT, STP, 1.0, WS, nb, stream),
        'max_norm nan': lib.him_grad_stats(G, n, SEG, 2, OUT, STP, float('nan'), WS, nb, stream),
        'max_norm < 0': lib.him_grad_stats(G, n, SEG, 2, OUT, STP, -1.0, WS, nb, stream),
        'null g': lib.him_grad_stats(0, n, SEG, 2, OUT, STP, 1.0, WS, nb, stream),
        'null st': lib.him_grad_stats(G, n, SEG, 2, OUT, 0, 1.0, WS, nb, stream),
        'null ws': lib.him_grad_stats(G, n, SEG, 2, OUT, STP, 1.0, 0, nb, stream),
        'null seg': lib.him_grad_stats(G, n, 0, 2, OUT, STP, 1.0, WS, nb, stream),
        'null seg_out': lib.him_grad_stats(G, n, SEG, 2, 0, STP, 1.0, WS, nb, stream),
    }
    short = lib.him_grad_stats(G, n, SEG, 2, OUT, STP, 1.0, WS, nb - 1, stream)
    torch.cuda.synchronize()
    assert {k: v for k, v in invalid.items() if v != H.E_INVALID} == {}
    assert short == H.E_WORKSPACE
    assert int(lib.him_grad_stats_ws(n, 2)) == nb and int(lib.him_grad_stats_ws(n, 0)) < nb
    assert ar.guard_failures() == []
    assert torch.equal(ar.t['st'].view(torch.float64).cpu(), mark), 'a refused call wrote st'
    assert bool((ar.t['seg_out'].view(torch.int32) == -1).all()), 'a refused call wrote seg_out'
    assert bool((ar.t['ws'] == H.NAN_BYTE).all()), 'a refused call wrote the workspace'
    # n == 0: nothing is read (null g, null ws), zeros are written and the call counts
    rc = lib.him_grad_stats(0, 0, SEG, 2, OUT, STP, 1.0, 0, 0, stream)
    H._finish(lib, 'n == 0', rc, ar, 'cuda')
    assert s.st() == [0.0, 0.0, 0.0, 1.0, 6.0, 6.0, 0.0, 0.0] and s.seg_out() == [[0.0, 0.0], [0.0, 0.0]]
    assert bool((ar.t['ws'] == H.NAN_BYTE).all())
    # the accepted call on the same arena
    s.call(1.0)
    _check_st('accepted', s.st(), g, 1.0)

    # the guarded Adam entry
    vals = _inputs(63)
    b = Bufs(vals, 0)
    P = b.ptr
    args = (HP['lr'], HP['beta1'], HP['beta2'], HP['eps'])
    bad = {
        'null st': lib.him_adam_guarded_step(P('p'), P('g'), P('m'), P('v'), P('ema'), 63, *args, 1, 0.999, 0, stream),
        'null st, no ema': lib.him_adam_guarded_step(P('p'), P('g'), P('m'), P('v'), 0, 63, *args, 1, 0.999, 0, stream),
        'step 0': lib.him_adam_guarded_step(P('p'), P('g'), P('m'), P('v'), P('ema'), 63, *args, 0, 0.999, STP, stream),
        'decay 1': lib.him_adam_guarded_step(P('p'), P('g'), P('m'), P('v'), P('ema'), 63, *args, 1, 1.0, STP, stream),
        'null p': lib.him_adam_guarded_step(0, P('g'), P('m'), P('v'), P('ema'), 63, *args, 1, 0.999, STP, stream),
    }
    ok = {
        'n == 0': lib.him_adam_guarded_step(0, 0, 0, 0, 0, 0, *args, 1, 0.999, 0, stream),
        # without an ema pointer the decay is ignored, whatever it is
        'decay ignored': lib.him_adam_guarded_step(P('p'), P('g'), P('m'), P('v'), 0, 0, *args, 1, 7.0, STP, stream),
    }
    torch.cuda.synchronize()
    assert {k: v for k, v in bad.items() if v != H.E_INVALID} == {}
    assert {k: v for k, v in ok.items() if v != 0} == {}
    assert b.ar.guard_failures() == []
    for k in NAMES:
        assert torch.equal(b.get(k), vals[k]), 'a refused call wrote %s' % k
