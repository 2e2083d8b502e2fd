"""him_diffaug_fwd / him_diffaug_bwd / him_diffaug_draw at the C ABI, in guarded arenas (abi_harness.Arena): the return
code and the bands are checked after every call.

Bounds.  Geometric-only rows copy and zero: bit for bit against index arithmetic on the host.  Colour rows: the op rule of
tests/README.md "How op tests bound errors" -- error over max|ref64| <= max(8 * e32, 16 * 2^-24), e32 being the error of
the same formulas in fp32 by torch on the CPU.  The per-sample sums (workspace) against math.fsum of the exact addends:
every addend is an fp32 value, exact in double, so any summation order stays within count * 2^-53 of sum|x| relative
(the linear-summation bound of test_grad_guard_abi_gpu.py, stated on the absolute values because these sums cancel).
The adjoint identity <fwd_lin(v), w> = <v, bwd(w)> is evaluated in float64 from the device's outputs; each inner product
inherits the op rule through its terms: |<a, w> - <a64, w>| <= sum|w| * max|a - a64|, so the two sides may differ by
lim(fwd) * max|fwd64| * sum|w| + lim(bwd) * max|bwd64| * sum|v|."""
import ctypes
import math

import pytest
import torch

import abi_harness as H
import diffaug_fixture as F
from neurips18_hierchical_image_manipulation_amd import augment

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SHAPES = [(3, 3, 0, 5, 7), (2, 7, 4, 16, 16), (2, 5, 1, 33, 65), (1, 42, 39, 64, 128)]
IDS = ['x'.join(map(str, s)) for s in SHAPES]
BIG = 2 ** 31 - 1


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(4000 + seed))


def _i32_as_f32(rows):
    return F.table_tensor(rows).contiguous().view(torch.float32)


class Call(object):
    """One guarded arena: input (behind ``off`` floats of NaN slack), table, output (``off`` floats of slack too), workspace."""

    def __init__(self, shape, rows, ch, cw, policy=7, off=0, g=None, ws_bytes=None, out_prefill=None):
        self.lib = H.raw_lib()
        self.B, self.C, self.c0, self.Hh, self.W = shape
        self.rows, self.ch, self.cw, self.policy, self.off = rows, ch, cw, policy, off
        self.g = g if g is not None else (0, self.C)
        self.need = int(self.lib.him_diffaug_ws(self.B, self.Hh, self.W))
        self.ws_bytes = self.need if ws_bytes is None else ws_bytes
        self.n_in = self.B * self.C * self.Hh * self.W
        self.out_shape = (self.B, self.g[1], self.Hh, self.W)
        self.n_out = self.B * self.g[1] * self.Hh * self.W
        pre = None
        if out_prefill is not None:
            pre = torch.full((off + self.n_out,), out_prefill)
        self.ar = H.Arena('cuda', {'src': ('in', torch.full((off + self.n_in,), float('nan'))),
                                   'table': ('in', _i32_as_f32(rows)),
                                   'dst': ('out', (off + self.n_out,), pre),
                                   'ws': ('ws', max(self.ws_bytes, 8))})

    def run(self, what, src, row='diffaug', expect=0):
        ar, lib = self.ar, self.lib
        ar.t['src'][self.off:].copy_(src.reshape(-1))
        a = (ar.ptr('src') + 4 * self.off, ar.ptr('table'), ar.ptr('dst') + 4 * self.off, self.B, self.C, self.c0, self.Hh,
             self.W, self.ch, self.cw, self.policy)
        tail = (ar.ptr('ws'), self.ws_bytes, H._stream('cuda'))
        if what == 'fwd':
            rc = lib.him_diffaug_fwd(*(a + tail))
        else:
            rc = lib.him_diffaug_bwd(*(a + self.g + tail))
        tag = '%s %s %s off=%d g=%s' % (row, what, (self.B, self.C, self.c0, self.Hh, self.W), self.off, self.g)
        if expect != 0:
            torch.cuda.synchronize()
            assert rc == expect, (tag, rc)
            assert not ar.guard_failures(), tag
            return None
        H._finish(lib, tag, rc, ar, 'cuda')
        if self.off:
            assert bool(torch.isnan(ar.t['src'][:self.off]).all())
            assert bool(torch.isnan(ar.t['dst'][:self.off]).all()), 'the elements in front of the output were written'
        return ar.t['dst'][self.off:].view(self.out_shape).cpu()

    def sums(self):
        return self.ar.t['ws'][:8 * self.B].view(torch.float64).cpu()


def _tables(B, Hh, W, ch, cw):
    """Named hand-written tables; every row index is taken modulo the list, so each batch size sees mixed rows."""
    geo = [F.row(ty=0, tx=0, bits=2), F.row(ty=1, tx=1, bits=2), F.row(ty=-2, tx=-3, bits=2), F.row(ty=2, tx=4, bits=2),
           F.row(ty=Hh, tx=0, bits=2), F.row(ty=0, tx=-W, bits=2), F.row(ty=-Hh - 5, tx=W + 9, bits=2),
           F.row(ty=BIG, tx=-BIG - 1, bits=2), F.row(ty=Hh - 1, tx=-(W - 1), bits=2),
           F.row(ty=3, tx=-3, bits=0), F.row(ty=-1, tx=1, cy=1, cx=1, bits=4)]
    cut = [F.row(cy=0, cx=0, bits=4), F.row(cy=-ch + 1, cx=2, bits=4), F.row(cy=1, cx=-cw + 1, bits=4),
           F.row(cy=Hh - 1, cx=1, bits=4), F.row(cy=2, cx=W - 1, bits=4), F.row(cy=-ch, cx=0, bits=4),
           F.row(cy=Hh, cx=W, bits=4), F.row(cy=BIG, cx=BIG, bits=4), F.row(cy=-BIG - 1, cx=-BIG - 1, bits=4),
           F.row(ty=1, tx=-3, cy=1, cx=2, bits=6), F.row(ty=-2, tx=4, cy=-1, cx=W - 2, bits=6)]
    col = [F.row(0.3, 0.4, 1.3, bits=1), F.row(-0.5, 0.0, 0.5, bits=1), F.row(0.25, 2.0, 1.5, bits=1),
           F.row(0.1, 1.0, 0.5, 1, 1, 1, 1, 7), F.row(-0.2, 1.7, 0.6, -2, -3, -1, W - 2, 7), F.row(0.4, 0.5, 0.5, 2, 4, Hh - 1, 0, 7),
           F.row(0.3, 2.0, 1.2, Hh, 1, 0, 0, 3), F.row(0.3, 0.0, 0.8, 0, 0, -ch, -cw, 5), F.row(0.45, 1.3, 0.5, 0, 1, 0, 0, 6),
           F.row(0.2, 0.8, 1.1, -2, -1, 0, 0, 0), F.row(-0.3, 0.6, 1.4, 0, -W, 0, 0, 3)]

    def take(rows, start):
        return [rows[(start + i) % len(rows)] for i in range(B)]
    out = {}
    for name, rows in (('geo', geo), ('cut', cut), ('col', col)):
        for start in range(0, len(rows), B):
            out['%s%d' % (name, start)] = take(rows, start)
    out['mixed'] = take(col, 3)                 # starts at a full row; from B = 2 on, rows with different bits in one batch
    return out


def _sizes(Hh, W):
    """Cutout sizes of the call: a rectangle, one row, one column, empty, covering the plane."""
    return [((Hh + 1) // 2, (W + 1) // 2), (1, W), (Hh, 1), (0, 3), (Hh, W)]


def _geometric(rows, policy=7):
    return all(not (r[7] & policy & 1) for r in rows)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_sums(what, got, parts):
    """parts[b]: the exact addends (float64 tensor of fp32 values) of sample b, or None for a row without colour."""
    for b, p in enumerate(parts):
        if p is None:
            assert float(got[b]) == 0.0, (what, b)
            continue
        vals = p.reshape(-1).tolist()
        ref, mag = math.fsum(vals), math.fsum(abs(v) for v in vals)
        bound = len(vals) * U * mag
        err = abs(float(got[b]) - ref)
        print('%s sample %d: sum %.17g ref %.17g err/bound %.3f (count %d)' % (what, b, float(got[b]), ref,
                                                                                err / bound if bound else 0.0, len(vals)))
        assert math.isfinite(float(got[b])) and err <= bound, (what, b, float(got[b]), ref, err, bound)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_forward_and_backward_against_the_oracle(shape):
    B, C, c0, Hh, W = shape
    x, dout = _rand(*shape[:2], Hh, W, seed=1) + 0.25, _rand(*shape[:2], Hh, W, seed=2)
    x64, d64 = x.double(), dout.double()
    for si, (ch, cw) in enumerate(_sizes(Hh, W)):
        for name, rows in _tables(B, Hh, W, ch, cw).items():
            if si > 0 and not name.startswith('cut') and name != 'mixed':
                continue                       # the other size classes matter to rows that cut
            row = '%s ch=%d cw=%d' % (name, ch, cw)
            c = Call(shape, rows, ch, cw)
            y = c.run('fwd', x, row)
            fsum = c.sums().clone()
            dx = c.run('bwd', dout, row)
            bsum = c.sums().clone()
            if _geometric(rows):
                assert torch.equal(_bits(y), _bits(F.forward(x, rows, ch, cw, c0))), row
                assert torch.equal(_bits(dx), _bits(F.backward(dout, rows, ch, cw, c0)[0])), row
                continue
            H.check_tensor(row, 'y', 'plane', y, F.forward(x64, rows, ch, cw, c0), F.forward(x, rows, ch, cw, c0), H.DIRECT)
            ref_dx, _ = F.backward(d64, rows, ch, cw, c0)
            H.check_tensor(row, 'dx', 'plane', dx, ref_dx, F.backward(dout, rows, ch, cw, c0)[0], H.DIRECT)
            colour = [bool(r[7] & 1) for r in rows]
            _check_sums(row + ' fwd', fsum, [x64[b, c0:c0 + 3] if colour[b] else None for b in range(B)])
            g = F.routed(d64, rows, ch, cw)
            _check_sums(row + ' bwd', bsum, [g[b, c0:c0 + 3] if colour[b] else None for b in range(B)])
            # rows without the colour bit inside a colour call are copies to the bit
            for b in range(B):
                if not colour[b]:
                    assert torch.equal(_bits(y[b]), _bits(F.forward(x[b:b + 1], rows[b:b + 1], ch, cw, c0)[0])), (row, b)
                    assert torch.equal(_bits(dx[b]), _bits(F.backward(dout[b:b + 1], rows[b:b + 1], ch, cw, c0)[0][0])), (row, b)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_call_policy_masks_the_rows(shape):
    """policy = translation | cutout: the colour bit of the rows is ignored, no workspace is needed, the image may have any
    position (c0 + 3 > C is legal) -- and the result is copies and zeros."""
    B, C, c0, Hh, W = shape
    x, dout = _rand(*shape[:2], Hh, W, seed=3), _rand(*shape[:2], Hh, W, seed=4)
    ch, cw = _sizes(Hh, W)[0]
    rows = _tables(B, Hh, W, ch, cw)['mixed']
    c = Call((B, C, C - 1, Hh, W), rows, ch, cw, policy=6, ws_bytes=0)
    assert torch.equal(_bits(c.run('fwd', x)), _bits(F.forward(x, rows, ch, cw, c0, 6)))
    assert torch.equal(_bits(c.run('bwd', dout)), _bits(F.backward(dout, rows, ch, cw, c0, 6)[0]))
    assert bool((c.ar.t['ws'] == H.NAN_BYTE).all()), 'a call without colour wrote the workspace'


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_adjoint_identity(shape):
    B, C, c0, Hh, W = shape
    v, w = _rand(*shape[:2], Hh, W, seed=5), _rand(*shape[:2], Hh, W, seed=6)
    ch, cw = _sizes(Hh, W)[0]
    lim = H.DIRECT.limit
    for name, rows in _tables(B, Hh, W, ch, cw).items():
        lin = [[F.f32_bits(0.0)] + r[1:] for r in rows]             # b = 0: the forward is linear
        c = Call(shape, lin, ch, cw)
        fv = c.run('fwd', v, name).double()
        bw = c.run('bwd', w, name).double()
        lhs, rhs = float((fv * w.double()).sum()), float((v.double() * bw).sum())
        f64, f32 = F.forward(v.double(), lin, ch, cw, c0), F.forward(v, lin, ch, cw, c0)
        b64, b32 = F.backward(w.double(), lin, ch, cw, c0)[0], F.backward(w, lin, ch, cw, c0)[0]
        ef = H.rel_err(f32, f64)[0]
        eb = H.rel_err(b32, b64)[0]
        bound = (lim(ef) * float(f64.abs().max()) * float(w.double().abs().sum())
                 + lim(eb) * float(b64.abs().max()) * float(v.double().abs().sum()))
        exact = float((f64 * w.double()).sum())
        print('%s %s: <fwd v, w> %.12g  <v, bwd w> %.12g  float64 %.12g  |diff| %.3e bound %.3e'
              % (name, shape, lhs, rhs, exact, abs(lhs - rhs), bound))
        assert abs(exact - float((v.double() * b64).sum())) <= 1e-9 * max(1.0, abs(exact))
        assert abs(lhs - rhs) <= bound, (name, lhs, rhs, bound)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_backward_of_a_channel_range(shape):
    B, C, c0, Hh, W = shape
    dout = _rand(*shape[:2], Hh, W, seed=7)
    ch, cw = _sizes(Hh, W)[0]
    ranges = {(c0, 3), (0, C), (0, 1), (C - 1, 1), (c0 + 1, 2), (c0, 1), (max(c0 - 1, 0), min(3, C)), (0, 0)}
    for name in ('col0', 'mixed', 'geo0'):
        rows = _tables(B, Hh, W, ch, cw)[name]
        full = Call(shape, rows, ch, cw).run('bwd', dout, name)
        for g0, gn in sorted(ranges):
            part = Call(shape, rows, ch, cw, g=(g0, gn)).run('bwd', dout, name)      # bands around a gn-channel buffer
            assert part.shape == (B, gn, Hh, W)
            assert torch.equal(_bits(part), _bits(full[:, g0:g0 + gn])), (name, g0, gn)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_determinism_and_a_pointer_offset_by_four_bytes(shape):
    B, C, c0, Hh, W = shape
    x = _rand(*shape[:2], Hh, W, seed=8)
    ch, cw = _sizes(Hh, W)[0]
    for name in ('mixed', 'geo0'):
        rows = _tables(B, Hh, W, ch, cw)[name]
        for what in ('fwd', 'bwd'):
            c = Call(shape, rows, ch, cw)
            a = c.run(what, x, name)
            sa = _bits(c.sums().clone().view(torch.float32)) if name == 'mixed' else None
            b = c.run(what, x, name)
            assert torch.equal(_bits(a), _bits(b)), 'two identical calls differ'
            if sa is not None:
                assert torch.equal(sa, _bits(c.sums().view(torch.float32)))
            for off in (1, 3):
                c2 = Call(shape, rows, ch, cw, off=off)
                assert torch.equal(_bits(c2.run(what, x, name)), _bits(a)), (what, off)
                if sa is not None:
                    assert torch.equal(sa, _bits(c2.sums().view(torch.float32))), (what, off)


def test_invalid_arguments_are_refused_and_write_nothing():
    shape = (2, 5, 1, 6, 10)
    B, C, c0, Hh, W = shape
    x = _rand(B, C, Hh, W, seed=9)
    rows = [F.row(0.1, 0.5, 1.2, 1, -1, 1, 1, 7)] * B
    E = H.E_INVALID

    def untouched(c):
        assert bool(torch.isnan(c.ar.t['dst']).all()) and bool((c.ar.t['ws'] == H.NAN_BYTE).all())
    for what in ('fwd', 'bwd'):
        for bad in (dict(shape=(B, C, 3, Hh, W)), dict(shape=(B, C, -1, Hh, W)), dict(ch=-1), dict(cw=-2), dict(policy=8)):
            kw = dict(shape=shape, rows=rows, ch=3, cw=3)
            kw.update(bad)
            c = Call(**kw)
            c.run(what, x, expect=E)
            untouched(c)
        c = Call(shape, rows, 3, 3)
        c.ws_bytes = c.need - 1                  # a workspace below the query
        c.run(what, x, expect=E)
        untouched(c)
        # null pointers, negative sizes: straight at the entry
        c = Call(shape, rows, 3, 3)
        ar, lib, st = c.ar, c.lib, H._stream('cuda')
        P = ar.ptr
        good = [P('src'), P('table'), P('dst'), B, C, c0, Hh, W, 3, 3, 7]
        extra = [] if what == 'fwd' else [0, C]
        fn = lib.him_diffaug_fwd if what == 'fwd' else lib.him_diffaug_bwd
        for i in (0, 1, 2):
            a = list(good)
            a[i] = 0
            assert fn(*(a + extra + [P('ws'), c.need, st])) == E
        for i in (3, 4, 6, 7):
            a = list(good)
            a[i] = -1
            assert fn(*(a + extra + [P('ws'), c.need, st])) == E
        assert fn(*(good + extra + [0, c.need, st])) == E                       # colour without a workspace
        if what == 'bwd':
            for g in ((-1, 2), (0, C + 1), (C, 1), (2, -1)):
                assert fn(*(good + list(g) + [P('ws'), c.need, st])) == E
        torch.cuda.synchronize()
        assert not ar.guard_failures()
        untouched(c)
    assert int(H.raw_lib().him_diffaug_ws(-1, 4, 4)) == 0


DRAWS = [(0, 0, 0, 1, 5, 7, 7), (1, 2, 3, 4, 16, 16, 7), (-5, 10 ** 12, 2 ** 40, 3, 33, 65, 7), (2 ** 62, 7, 0, 2, 256, 512, 7),
         (3, 1, 0, 64, 256, 512, 7), (3, 1, 0, 5, 64, 128, 1), (3, 1, 0, 5, 64, 128, 2), (3, 1, 0, 5, 64, 128, 4),
         (3, 1, 0, 5, 64, 128, 5), (9, 9, 9, 4, 7, 9, 0)]


@pytest.mark.parametrize('seed,step,sample0,B,Hh,W,policy', DRAWS)
def test_device_draw_equals_the_python_mirror(seed, step, sample0, B, Hh, W, policy):
    lib = H.raw_lib()
    for rt, rc in ((0.125, 0.5), (0.0, 0.0), (0.3, 0.77), (1.0, 1.5)):
        ar = H.Arena('cuda', {'table': ('out', (B * 8,), None)})
        ch, cw = ctypes.c_int(-1), ctypes.c_int(-1)
        rc_ = lib.him_diffaug_draw(ar.ptr('table'), B, Hh, W, seed, step, sample0, policy, rt, rc, ctypes.byref(ch),
                                   ctypes.byref(cw), H._stream('cuda'))
        H._finish(lib, 'draw %s' % ((seed, step, sample0, B, Hh, W, policy, rt, rc),), rc_, ar, 'cuda')
        rows, h, w = augment.draw(B, Hh, W, seed, step, sample0, policy, rt, rc)
        assert (ch.value, cw.value) == (h, w)
        got = ar.t['table'].view(torch.int32).view(B, 8).cpu()
        assert torch.equal(got, F.table_tensor(rows)), (got.tolist(), rows)


def test_draw_refuses_bad_arguments():
    lib = H.raw_lib()
    ar = H.Arena('cuda', {'table': ('out', (16,), None)})
    ch, cw = ctypes.c_int(0), ctypes.c_int(0)
    st = H._stream('cuda')
    good = [ar.ptr('table'), 2, 8, 8, 0, 0, 0, 7, 0.125, 0.5, ctypes.byref(ch), ctypes.byref(cw), st]
    for i, v in ((0, 0), (1, -1), (2, 0), (3, 0), (7, 8), (8, -0.1), (9, float('nan')), (8, 1e9), (10, None), (11, None)):
        a = list(good)
        a[i] = v
        assert lib.him_diffaug_draw(*a) == H.E_INVALID, i
    torch.cuda.synchronize()
    assert not ar.guard_failures() and bool(torch.isnan(ar.t['table']).all())
