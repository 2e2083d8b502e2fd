"""him_adam_ema_step / him_ema_update / him_swap at the C ABI, in guarded arenas (abi_harness.Arena).

Every buffer of a call lives between two guard bands; after each call the return code and the bands are checked.  Sizes
cover one thread, a partial wavefront, the block size and its neighbours, and 4096 * 256 + 77: one element more than the
launch cap of 4096 blocks of 256 covers, so the grid-stride loop takes its second trip.  Each size runs with every pointer
256-byte aligned and with every pointer advanced by one float (4-byte alignment only).

Bounds.  p, m, v: bit-identical to him_adam_step (the same kernel body).  ema': the kernel rounds the difference p' - ema
once and the FMA once, so against a float64 evaluation of ema + w * (p' - ema) from the same fp32 inputs the error is at
most 2^-24 * |p' - ema| * w + 2^-24 * |ema'| <= 3 * 2^-24 * max(|p'|, |ema|, |ema'|).  K steps: the recursion contracts
the carried error by d per step, so it stays below min(K, 1 / (1 - d)) times the one-step bound."""
import pytest
import torch

import abi_harness as H

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SIZES = [1, 63, 255, 256, 257, 4096 * 256 + 77]
HP = dict(lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8)
NAMES = ('p', 'g', 'm', 'v', 'ema')


def _inputs(n, seed=0):
    gen = torch.Generator().manual_seed(1000 + seed)
    r = lambda s=1.0: torch.randn(n, generator=gen) * s      # noqa: E731
    return dict(p=r(), g=r(0.1), m=r(0.05), v=r(0.01).abs(), ema=r())


class Bufs(object):
    """The five buffers in one guarded arena; ``off`` floats of slack in front of each (1: pointers 4-byte aligned only).
    The slack element keeps its NaN fill: a kernel that rounded a pointer down would change it."""

    def __init__(self, vals, off):
        self.n, self.off = next(iter(vals.values())).numel(), off
        specs = {k: ('out', (self.n + off,), torch.cat([torch.full((off,), float('nan')), vals[k]])) for k in vals}
        self.ar = H.Arena('cuda', specs)

    def ptr(self, k):
        return self.ar.ptr(k) + 4 * self.off

    def get(self, k):
        return self.ar.t[k][self.off:].cpu()

    def check(self, lib, row, rc):
        H._finish(lib, row, rc, self.ar, 'cuda')
        for k, t in self.ar.t.items():
            assert bool(torch.isnan(t[:self.off]).all()), '%s: the element in front of %s was written' % (row, k)


def _adam(lib, b, step, hp=HP):
    rc = lib.him_adam_step(b.ptr('p'), b.ptr('g'), b.ptr('m'), b.ptr('v'), b.n, hp['lr'], hp['beta1'], hp['beta2'],
                           hp['eps'], step, H._stream('cuda'))
    b.check(lib, 'adam n=%d' % b.n, rc)


def _fused(lib, b, step, decay, hp=HP):
    rc = lib.him_adam_ema_step(b.ptr('p'), b.ptr('g'), b.ptr('m'), b.ptr('v'), b.ptr('ema'), b.n, hp['lr'], hp['beta1'],
                               hp['beta2'], hp['eps'], step, decay, H._stream('cuda'))
    b.check(lib, 'adam_ema n=%d off=%d step=%d' % (b.n, b.off, step), rc)


def _ema_ref64(p_new, ema, decay):
    w = torch.tensor(1.0 - decay, dtype=torch.float64).float().double()      # the kernel's fp32 w, widened
    return ema.double() + w * (p_new.double() - ema.double())


def _assert_ema(got, p_new, ema, decay, k=1.0, what=''):
    ref = _ema_ref64(p_new, ema, decay)
    bound = k * 3 * EPS * torch.maximum(torch.maximum(p_new.abs(), ema.abs()), got.abs()).double()
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print('%s ema: worst error / bound = %.3f' % (what, worst))
    assert bool((err <= bound).all()), '%s: ema error %.3f x the bound at %d' % (what, worst, int((err / bound).argmax()))


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('n', SIZES)
def test_fused_step_equals_adam_and_averages(n, off):
    lib = H.raw_lib()
    vals = _inputs(n)
    # beta1 0.5 / 0.0: both branches of the first-moment lerp (1 - beta1 < 0.5)
    for step, beta1 in [(s, b1) for s in (1, 2, 1000) for b1 in (0.5, 0.0)]:
        hp = dict(HP, beta1=beta1)
        a, f, z, e = Bufs(vals, off), Bufs(vals, off), Bufs(vals, off), Bufs(vals, off)
        _adam(lib, a, step, hp)
        _fused(lib, f, step, 0.999, hp)
        what = 'n=%d off=%d step=%d beta1=%g' % (n, off, step, beta1)
        for k in ('p', 'm', 'v'):
            assert torch.equal(a.get(k), f.get(k)), '%s: %s differs from him_adam_step' % (what, k)
        assert torch.equal(f.get('g'), vals['g'])
        assert not torch.equal(f.get('p'), vals['p'])
        _assert_ema(f.get('ema'), f.get('p'), vals['ema'], 0.999, what=what)
        # ema_decay 0: a copy of p', not a lerp
        _fused(lib, z, step, 0.0, hp)
        assert torch.equal(z.get('ema'), z.get('p')) and torch.equal(z.get('p'), a.get('p')), what
        # him_ema_update on the Adam entry's p': the same bits as the fused entry's ema'
        _adam(lib, e, step, hp)
        rc = lib.him_ema_update(e.ptr('ema'), e.ptr('p'), n, 0.999, H._stream('cuda'))
        e.check(lib, 'ema_update ' + what, rc)
        assert torch.equal(e.get('ema'), f.get('ema')), '%s: him_ema_update differs from the fused entry' % what
        assert torch.equal(e.get('p'), a.get('p'))


def test_200_fused_steps_against_the_float64_recursion():
    lib = H.raw_lib()
    n, d, K = 257, 0.99, 200
    vals = _inputs(n, seed=7)
    b = Bufs(vals, 1)
    ref = vals['ema'].double()
    w = torch.tensor(1.0 - d, dtype=torch.float64).float().double()
    scale = float(vals['ema'].abs().max())
    gen = torch.Generator().manual_seed(99)
    for step in range(1, K + 1):
        b.ar.t['g'][1:].copy_(torch.randn(n, generator=gen) * 0.1)
        _fused(lib, b, step, d)
        p = b.get('p')                       # every p' on the host: the recursion runs over the kernel's own parameters
        ref = ref + w * (p.double() - ref)
        scale = max(scale, float(p.abs().max()))
    got = b.get('ema')
    scale = max(scale, float(got.abs().max()))
    bound = min(K, 1.0 / (1.0 - d)) * 3 * EPS * scale
    err = float((got.double() - ref).abs().max())
    print('200 steps: max error %.3e, bound %.3e' % (err, bound))
    assert err <= bound, (err, bound)


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('n', SIZES)
def test_swap_exchanges_exactly(n, off):
    lib = H.raw_lib()
    vals = _inputs(n, seed=3)
    b = Bufs(dict(a=vals['p'], b=vals['ema']), off)
    for trip, (wa, wb) in enumerate((('ema', 'p'), ('p', 'ema'))):      # a second swap restores both
        rc = lib.him_swap(b.ptr('a'), b.ptr('b'), n, H._stream('cuda'))
        b.check(lib, 'swap n=%d off=%d trip %d' % (n, off, trip), rc)
        assert torch.equal(b.get('a'), vals[wa]) and torch.equal(b.get('b'), vals[wb]), (n, off, trip)
    assert not torch.equal(vals['p'], vals['ema'])


def test_return_codes_and_refused_calls_write_nothing():
    lib = H.raw_lib()
    n = 63
    vals = _inputs(n)
    b = Bufs(vals, 0)
    st = H._stream('cuda')
    P = b.ptr
    args = (HP['lr'], HP['beta1'], HP['beta2'], HP['eps'])
    bad = {
        'step 0': lib.him_adam_ema_step(P('p'), P('g'), P('m'), P('v'), P('ema'), n, *args, 0, 0.999, st),
        'decay 1': lib.him_adam_ema_step(P('p'), P('g'), P('m'), P('v'), P('ema'), n, *args, 1, 1.0, st),
        'decay < 0': lib.him_adam_ema_step(P('p'), P('g'), P('m'), P('v'), P('ema'), n, *args, 1, -0.5, st),
        'decay nan': lib.him_adam_ema_step(P('p'), P('g'), P('m'), P('v'), P('ema'), n, *args, 1, float('nan'), st),
        'null ema': lib.him_adam_ema_step(P('p'), P('g'), P('m'), P('v'), 0, n, *args, 1, 0.999, st),
        'null p': lib.him_adam_ema_step(0, P('g'), P('m'), P('v'), P('ema'), n, *args, 1, 0.999, st),
        'update decay 1': lib.him_ema_update(P('ema'), P('p'), n, 1.0, st),
        'update decay < 0': lib.him_ema_update(P('ema'), P('p'), n, -1e-3, st),
        'update null': lib.him_ema_update(0, P('p'), n, 0.5, st),
        'swap null': lib.him_swap(P('p'), 0, n, st),
    }
    torch.cuda.synchronize()
    assert {k: v for k, v in bad.items() if v != H.E_INVALID} == {}
    ok = {
        'fused n=0': lib.him_adam_ema_step(0, 0, 0, 0, 0, 0, *args, 1, 0.999, st),
        'update n=0': lib.him_ema_update(0, 0, 0, 0.999, st),
        'swap n=0': lib.him_swap(0, 0, 0, st),
    }
    torch.cuda.synchronize()
    assert {k: v for k, v in ok.items() if v != 0} == {}
    assert b.ar.guard_failures() == []
    for k in NAMES:
        assert torch.equal(b.get(k), vals[k]), 'a refused call wrote %s' % k
