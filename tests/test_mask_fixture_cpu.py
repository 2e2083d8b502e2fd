"""The checks of tests/test_mask_abi_gpu.py must be able to FAIL, and tests/mask_fixture.py must keep its own conditions.
Runs without a GPU: Python stand-ins of the entry points write into a CPU arena through raw addresses (abi_harness.mem),
bands included; each planted defect must be caught by the check that is meant to catch it, and the stand-ins without a
defect are green."""
import pytest
import torch
import torch.nn.functional as F

import abi_harness as ah
import mask_fixture as fx
import test_mask_abi_gpu as M
from mask_fixture import F32, F64


@pytest.fixture(autouse=True)
def _no_report():
    yield
    del M.ROWS[:]


@pytest.fixture(autouse=True)
def _rows_stay_in_memory(monkeypatch):
    monkeypatch.setattr(M, 'flush', lambda: None)


def _act_code(code):
    return [k for k, v in fx.ACTS.items() if v == code][0]


class StandIn(object):
    """The entry points the defects live in, in fp32 torch on the CPU; ``defect`` plants one fault."""

    def __init__(self, defect=None):
        self.defect = defect

    def him_last_error(self):
        return b'stand-in'

    def him_batchnorm_ws(self, C):
        return C * 32 * 2 * 4 + C * 2 * 4 + 256

    def him_mask_loss_ws(self):
        return 1024 * 2 * 4 + 256

    def him_batchnorm_fwd(self, x, residual, gamma, beta, run_mean, run_var, y, save_mean, save_rstd, B, C, hw, eps, momentum,
                          training, act, slope, ws, ws_bytes, stream):
        X = ah.mem(x, B * C * hw).view(B, C, hw)
        n = B * hw
        if training:
            if self.defect == 'shift_first':         # the statistics before they were centred: pivot x[0][c][0], q/n - ms^2
                shift = X[0, :, 0].view(1, C, 1)
                d = X - shift
                ms = d.sum((0, 2)) / n
                mu = shift.view(C) + ms
                var = ((d * d).sum((0, 2)) / n - ms * ms).clamp_min(0)
            else:
                mu = X.mean((0, 2))
                var = ((X - mu.view(1, C, 1)) ** 2).mean((0, 2))
            if run_mean:
                rm, rv = ah.mem(run_mean, C), ah.mem(run_var, C)
                rm.copy_((1 - momentum) * rm + momentum * mu)
                rv.copy_((1 - momentum) * rv + momentum * var * (n / max(n - 1.0, 1.0)))
        else:
            mu, var = ah.mem(run_mean, C).clone(), ah.mem(run_var, C).clone()
        rs = (var + eps).rsqrt()
        g = ah.mem(gamma, C) if gamma else torch.ones(C)
        b = ah.mem(beta, C) if beta else torch.zeros(C)
        out = fx.act_fn((X - mu.view(1, C, 1)) * (rs * g).view(1, C, 1) + b.view(1, C, 1), _act_code(act))
        if residual:
            out = out + ah.mem(residual, B * C * hw).view(B, C, hw)
        ah.mem(y, B * C * hw).copy_(out.reshape(-1))
        ah.mem(save_mean, C).copy_(mu)
        ah.mem(save_rstd, C).copy_(rs)
        return 0

    def him_batchnorm_bwd(self, x, gamma, beta, save_mean, save_rstd, dy, dx, dgamma, dbeta, B, C, hw, training, act, slope,
                          accumulate, ws, ws_bytes, stream):
        X, DY = ah.mem(x, B * C * hw).view(B, C, hw), ah.mem(dy, B * C * hw).view(B, C, hw)
        mu, rs = ah.mem(save_mean, C).view(1, C, 1), ah.mem(save_rstd, C).view(1, C, 1)
        g = (ah.mem(gamma, C) if gamma else torch.ones(C)).view(1, C, 1)
        b = (ah.mem(beta, C) if beta else torch.zeros(C)).view(1, C, 1)
        xh = (X - mu) * rs
        z = (xh * g + b).requires_grad_(True)
        (dz,) = torch.autograd.grad(fx.act_fn(z, _act_code(act)), z, DY)
        a, q = dz.sum((0, 2)), (dz * xh).sum((0, 2))
        n = B * hw
        if dx:
            m1, m2 = (a / n, q / n) if training else (torch.zeros(C), torch.zeros(C))
            ah.mem(dx, B * C * hw).copy_((g * rs * (dz - m1.view(1, C, 1) - xh * m2.view(1, C, 1))).reshape(-1))
        for ptr, v in ((dgamma, q), (dbeta, a)):
            if ptr:
                t = ah.mem(ptr, C)
                t.copy_(t + v if accumulate else v)
        return 0

    def him_act_fwd(self, x, y, n, act, slope, stream):
        m = min(n, fx.GRID_CAP) if self.defect == 'stops_at_cap' else n
        ah.mem(y, n)[:m] = fx.act_fn(ah.mem(x, n), _act_code(act))[:m]
        return 0

    def him_act_bwd(self, y, dy, dz, n, act, slope, stream):
        ah.mem(dz, n).copy_(fx.act_bwd(ah.mem(y, n), ah.mem(dy, n), _act_code(act), F32))
        return 0

    def him_masked_nll_fwd(self, logp, label, mask, out2, B, C, hw, ws, ws_bytes, stream):
        LP, L, Mk = ah.mem(logp, B * C * hw).view(B, C, hw), ah.mem(label, B * hw).view(B, hw), ah.mem(mask, B * hw).view(B, hw)
        valid = ((Mk > 0.5) if self.defect == 'mask_gt' else (Mk >= 0.5)) & (L >= 0) & (L < C)
        if self.defect == 'drops_second_trip':
            valid = valid & (torch.arange(B * hw).view(B, hw) < fx.LOSS_CAP)
        picked = LP.gather(1, L.clamp(0, C - 1).long().view(B, 1, hw)).view(B, hw)
        cnt = valid.sum().float()
        out = ah.mem(out2, 2)
        out[0] = -(picked * valid).sum() / cnt
        out[1] = cnt
        return 0

    def him_masked_nll_bwd(self, label, mask, g, count, dlogp, B, C, hw, stream):
        L, Mk = ah.mem(label, B * hw).view(B, 1, hw), ah.mem(mask, B * hw).view(B, 1, hw)
        scale = -ah.mem(g, 1)[0] / ah.mem(count, 1)[0]
        hit = (Mk >= 0.5) & (L == torch.arange(C, dtype=F32).view(1, C, 1))
        ah.mem(dlogp, B * C * hw).copy_(torch.where(hit, scale, torch.zeros(())).reshape(-1))
        return 0

    def him_upsample2_fwd(self, x, y, planes, H, W, align, stream):
        out = fx.upsample2(ah.mem(x, planes * H * W).view(planes, H, W), align, F32)
        extra = 1 if self.defect == 'past_plane' else 0                 # the last plane runs one float too far
        ah.mem(y, out.numel() + extra)[:out.numel()] = out.reshape(-1)
        if extra:
            ah.mem(y, out.numel() + 1)[-1] = out.reshape(-1)[-1]
        return 0

    def him_upsample2_bwd(self, dy, dx, planes, H, W, align, stream):
        g = fx.upsample2(torch.zeros(planes, H, W), align, F32, ah.mem(dy, planes * 4 * H * W).view(planes, 2 * H, 2 * W))
        ah.mem(dx, planes * H * W).copy_(g.reshape(-1))
        return 0

    def him_resize_compose(self, comb, obj, C, h, w, label, mask, cls, background, dst, H, W, align, stream):
        lab = ah.mem(label, H * W).view(H, W)
        if not background:
            out, _ = fx.resize_compose(ah.mem(obj, h * w).view(1, h, w), lab, None, cls, 0, align, F32)
            ah.mem(dst, H * W).copy_(out.reshape(-1))
            return 0
        v = fx.resize(ah.mem(comb, C * h * w).view(C, h, w), H, W, align, F32)
        m = ah.mem(mask, H * W).view(1, H, W)
        val = v * m + (1 - m) * (lab.view(1, H, W) == torch.arange(C, dtype=F32).view(C, 1, 1)).float()
        best = (C - 1 - val.flip(0).argmax(0)) if self.defect == 'argmax_last' else torch.from_numpy(val.numpy().argmax(0))
        ah.mem(dst, 2 * H * W).view(torch.int64).copy_(best.reshape(-1))
        return 0


def _runs(lib):
    """defect -> the run that must catch it."""
    return {
        'shift_first': lambda: M.run_bn(lib, 'cpu', fx.BNCase(8, 4, 1024, True, 'none', gen='first100'), chained=True),
        'stops_at_cap': lambda: M.run_act(lib, 'cpu', fx.GRID_CAP + 257, 'tanh'),
        'drops_second_trip': lambda: M.run_nll(lib, 'cpu', 3, 2, 90001),
        'past_plane': lambda: M.run_upsample(lib, 'cpu', 2, 5, 3, 0),
        'mask_gt': lambda: M.run_nll(lib, 'cpu', 3, 35, 168),
        'argmax_last': lambda: M.run_resize(lib, 'cpu', fx.resize_tie_case(), (8, 8), (16, 16), 1, 0, 'tie', exclude=False),
    }


DEFECTS = [('shift_first', r'save_rstd: error .* > limit'), ('stops_at_cap', r'act\|tanh\|n2097409 y: error inf'),
           ('drops_second_trip', r'count \d+\.0, expected'), ('past_plane', r'guard behind y changed: first byte at \+0'),
           ('mask_gt', r'count \d+\.0, expected'), ('argmax_last', r'decisions differ from the float64 restatement')]


@pytest.mark.parametrize('defect', [d[0] for d in DEFECTS])
def test_stand_in_without_defect_is_green(defect):
    _runs(StandIn())[defect]()
    assert all(r['error'] <= r['limit'] for r in M.ROWS)


@pytest.mark.parametrize('defect,message', DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defect_is_caught_by_its_check(defect, message):
    import re
    with pytest.raises(AssertionError) as e:
        _runs(StandIn(defect))[defect]()
    assert re.search(message, str(e.value)), str(e.value)


def test_stand_in_option_cross_is_green():
    """The BatchNorm runner's own plumbing (NULL pointers, accumulate, eval mode, every epilogue) against a correct stand-in."""
    for training in (True, False):
        for act in M.ACT_NAMES:
            c = fx.BNCase(3, 2, 7, training, act, residual=True, affine=act != 'tanh', running=not (training and act == 'relu'))
            M.run_bn(StandIn(), 'cpu', c, dx=act != 'sigmoid', accumulate=1 if c.affine else 0)


# ------------------------------------------------------------------------------------------- the fixture's own conditions
def _bn_cases():
    for shape in M.BN_SHAPES:
        for training in (True, False):
            yield fx.BNCase(*shape, training, M.ACT_NAMES[M.BN_SHAPES.index(shape) % 5])
    for shape in M.BN_CROSS:
        for training in (True, False):
            for act in M.ACT_NAMES:
                for affine in (True, False):
                    yield fx.BNCase(*shape, training, act, affine=affine)
    for shape in ((8, 4, 1024), (4, 16, 117)):
        for gen in fx.BN_ILL:
            yield fx.BNCase(*shape, True, 'none', gen=gen)


def _inside(what, r32, r64):
    e32 = fx.rel_err(r32, r64)
    assert e32 < float('inf') and e32 <= fx.limit(e32), '%s: the float32 restatement is %.3e from float64' % (what, e32)


def test_batchnorm_cases_keep_the_sign_margin_and_float32_stays_near_float64():
    seen = 0
    for c in _bn_cases():
        if c.act in ('relu', 'lrelu'):
            mean, rstd = c.stats(F64)
            g = c.gamma.double() if c.affine else torch.ones(c.C, dtype=F64)
            b = c.beta.double() if c.affine else torch.zeros(c.C, dtype=F64)
            z = (c.x.double() - mean.view(1, -1, 1)) * (rstd * g).view(1, -1, 1) + b.view(1, -1, 1)
            assert float(z.abs().min()) > fx.Z_MARGIN, (c.tag(), float(z.abs().min()))
            seen += 1
        for k, v in c.ref(F64).items():
            _inside(c.tag() + ' ' + k, c.ref(F32)[k], v)
    assert seen >= 16
    c = fx.BNCase(8, 4, 1024, True, 'none', gen='const_channel')
    assert float(c.ref(F64)['save_rstd'][1]) == fx.BN_EPS ** -0.5


def test_resize_compose_cases_leave_out_at_most_half_a_percent():
    for lo, hi in fx.RESIZE_SHAPES:
        for background in (0, 1):
            for align in (0, 1):
                src, label, mask, cls = fx.resize_case(lo, hi, background)
                want, margin = fx.resize_compose(src, label, mask, cls, background, align)
                share = float((margin < fx.MARGIN).double().mean())
                assert share <= fx.MAX_LEFT_OUT, (lo, hi, background, align, share)
                w32, _ = fx.resize_compose(src, label, mask, cls, background, align, F32)
                keep = margin >= fx.MARGIN
                assert torch.equal(w32[keep].double(), want[keep].double()), (lo, hi, background, align)
    src, label, mask, cls = fx.resize_tie_case()
    assert bool((fx.resize_compose(src, label, mask, cls, 1, 0)[0] == 3).all())


def test_float32_restatements_stay_near_float64_and_follow_torch():
    for n in (1, 255, fx.GRID_CAP + 257):
        for act in M.ACT_NAMES[1:]:
            x = M.act_input(n)
            _inside('act ' + act, fx.act_fn(x, act), fx.act_fn(x.double(), act))
            y, dy = fx.act_fn(x, act), fx.rand(n, seed=3)
            _inside('act_bwd ' + act, fx.act_bwd(y, dy, act, F32), fx.act_bwd(y, dy, act, F64))
    for planes, H, W in ((2, 5, 3), (1, 63, 65), (3, 420, 420)):
        for align in (0, 1):
            x, dy = fx.rand(planes, H, W, seed=1), fx.rand(planes, 2 * H, 2 * W, seed=2)
            _inside('upsample', fx.upsample2(x, align, F32), fx.upsample2(x, align, F64))
            _inside('upsample bwd', fx.upsample2(x, align, F32, dy), fx.upsample2(x, align, F64, dy))
            # the hand-written resize of him_resize_compose is the same map as F.interpolate
            _inside('resize', fx.resize(x, 2 * H, 2 * W, align, F64), fx.upsample2(x, align, F64))
    x, dy = fx.rand(2, 35, 99, seed=1, scale=3.0), fx.rand(2, 35, 99, seed=2)
    y = fx.log_softmax(x, F32)
    _inside('log_softmax', y, fx.log_softmax(x, F64))
    _inside('log_softmax bwd', fx.log_softmax_bwd(y, dy, F32), fx.log_softmax_bwd(y, dy, F64))
    xg = x.double().requires_grad_(True)
    (gx,) = torch.autograd.grad(F.log_softmax(xg, 1), xg, dy.double())
    assert fx.rel_err(fx.log_softmax_bwd(y, dy, F64), gx) < fx.FLOOR             # from the fp32 y: autograd's value
    ctx, obj, dout = fx.rand(2, 35, 99, seed=1), fx.rand(2, 1, 99, seed=2), fx.rand(2, 35, 99, seed=3)
    p = torch.sigmoid(obj)
    _inside('gate', fx.gate_comb(ctx, p, obj, F32), fx.gate_comb(ctx, p, obj, F64))
    c64, p64, o64 = (t.double().requires_grad_(True) for t in (ctx, p, obj))
    grads = torch.autograd.grad((1 - p64) * c64 + p64 * o64, (c64, p64, o64), dout.double())
    for k, gr in zip(('dctx', 'dp', 'dobj'), grads):
        assert fx.rel_err(fx.gate_comb_bwd(ctx, p, obj, dout, F64)[k], gr) < 1e-14, k
        _inside('gate ' + k, fx.gate_comb_bwd(ctx, p, obj, dout, F32)[k], fx.gate_comb_bwd(ctx, p, obj, dout, F64)[k])
    for case in ((3, 35, 168, 'random'), (3, 2, 90001, 'random'), (3, 35, 168, 'one')):
        logp, label, mask = fx.nll_case(*case)
        l64, n64, d64 = fx.masked_nll(logp, label, mask, F64, 0.7)
        l32, n32, d32 = fx.masked_nll(logp, label, mask, F32, 0.7)
        assert n64 == n32 > 0
        _inside('nll', l32, l64)
        _inside('nll bwd', d32, d64)
    logp, label, mask = fx.nll_case(3, 35, 168)
    assert all(float(v) in mask.view(-1)[:3].tolist() for v in torch.tensor([0.5, 0.49999997, 0.50000006]))
    assert {255.0, -1.0, 35.0} <= set(label.view(-1).tolist())
    assert fx.masked_nll(*fx.nll_case(3, 35, 168, 'none'), F64)[1] == 0 and fx.masked_nll(*fx.nll_case(1, 2, 1, 'one'), F64)[1] == 1
    for p, t in ((torch.sigmoid(fx.rand(396, seed=1, scale=3.0)), (fx.uniform(396, seed=2) > 0.5).float()), fx.bce_saturated()):
        _inside('bce', fx.bce_mean(p, t, F32), fx.bce_mean(p, t, F64))
        assert fx.elem_err(fx.bce_mean_bwd(p, t, 0.7, F32), fx.bce_mean_bwd(p, t, 0.7, F64)) < float('inf')
        pg = p.double().requires_grad_(True)
        ref = F.binary_cross_entropy(pg, t.double())
        assert abs(float(ref.detach()) - float(fx.bce_mean(p, t, F64))) <= 1e-14 * abs(float(ref.detach()))       # torch's clamps, restated
        (gp,) = torch.autograd.grad(ref, pg, torch.tensor(0.7, dtype=F64))
        assert fx.elem_err(fx.bce_mean_bwd(p, t, 0.7, F64), gp) < 1e-12
    x = fx.rand(2, 3, 8, 12, seed=1)
    for d in (1, 2, 4):
        y = fx.space_to_batch(x, d)
        assert torch.equal(fx.batch_to_space(y, d, 2), x)
        assert torch.equal(y[(1 * d + d - 1) * d + 0, 2, 1, 2], x[1, 2, 1 * d + d - 1, 2 * d])
