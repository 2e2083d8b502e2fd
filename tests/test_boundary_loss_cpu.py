"""The restatement of the boundary-weighted and surface losses (tests/boundary_loss_fixture.py) against torch's own
weighted losses and autograd, on hand-drawn planes, and against planted defects; the library's exports, the training
parser's three settings and the host-side refusals.  No GPU: nothing here launches a kernel."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import boundary_loss_fixture as fx
import edt_fixture as ef
from boundary_loss_fixture import F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['him_bw_loss_ws', 'him_bw_nll_fwd', 'him_bw_nll_bwd', 'him_bw_pair_fwd', 'him_bw_pair_bwd', 'him_surface_fwd',
           'him_surface_bwd']


def _case(B=2, C=4, H=9, W=11, plane='ignore'):
    label = fx.label_plane(plane, B, C, H, W)
    return (fx.logp_planes(B, C, H, W), label, fx.mask_plane(plane, B, H, W), fx.boundary_d2(label.numpy()))


# ------------------------------------------------------------------------------------------------------- distances
@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (7, 5), (17, 33), (40, 56)], ids=lambda s: '%dx%d' % s)
def test_separable_transform_equals_the_brute_force_one(shape):
    H, W = shape
    g = np.random.default_rng(H * 100 + W)
    for density in (0.0, 0.02, 0.3, 1.0):
        seed = g.random((H, W)) < density
        assert np.array_equal(fx.edt_separable(seed), ef.edt(seed)[0]), (shape, density)


def test_large_planes_take_the_separable_transform_and_small_ones_the_brute_force():
    assert 64 * 64 > fx.BRUTE_MAX >= 17 * 33
    lab = fx.label_plane('checker', 1, 2, 96, 160)
    assert int(fx.boundary_d2(lab.numpy()).max()) == 0               # every pixel of a checkerboard is a boundary


# ------------------------------------------------------------------------------------- against torch's own losses
@pytest.mark.parametrize('amp,sigma', fx.AMP_SIGMA)
def test_nll_equals_torch_nll_with_a_weight_per_pixel_and_its_autograd(amp, sigma):
    logp, label, mask, d2 = _case()
    B, C, H, W = logp.shape
    lp = logp.double().requires_grad_(True)
    w = fx.weight(d2, amp, sigma, F64)
    tgt = label[:, 0].long()
    tgt = torch.where((mask[:, 0] >= 0.5) & (tgt < C), tgt, torch.full_like(tgt, 255))
    per = F.nll_loss(lp, tgt, ignore_index=255, reduction='none')
    valid = tgt != 255
    want = (per * w)[valid].sum() / w[valid].sum()
    (dwant,) = torch.autograd.grad(want, lp, torch.tensor(0.75, dtype=F64))
    want = want.detach()
    got = fx.bw_nll(logp, label, mask, d2, amp, sigma, F64, g=0.75)
    assert abs(float(got['loss'] - want)) <= 1e-13 * abs(float(want))
    assert float((got['dlogp'] - dwant).abs().max()) <= 1e-13 * float(dwant.abs().max())
    assert abs(float(got['sum_w'] - w[valid].sum())) <= 1e-12 * float(got['sum_w'])


@pytest.mark.parametrize('kind', ['bce', 'l1'])
@pytest.mark.parametrize('amp,sigma', fx.AMP_SIGMA)
def test_pair_equals_torch_weighted_loss_and_its_autograd(kind, amp, sigma):
    B, H, W = 2, 9, 11
    t = fx.object_plane('object', B, H, W)
    d2 = fx.boundary_d2(t.numpy())
    p = fx.prob_plane(B, H, W).double().requires_grad_(True)
    w = fx.weight(d2, amp, sigma, F64)[:, None]
    if kind == 'bce':
        want = F.binary_cross_entropy(p, t.double(), weight=w, reduction='sum') / w.sum()
    else:
        want = (w * (p - t.double()).abs()).sum() / w.sum()
    (dwant,) = torch.autograd.grad(want, p, torch.tensor(1.5, dtype=F64))
    want = want.detach()
    got = fx.bw_pair(p.detach(), t, d2, amp, sigma, kind, F64, g=1.5)
    assert abs(float(got['loss'] - want)) <= 1e-13 * abs(float(want))
    assert float((got['dp'] - dwant).abs().max()) <= 1e-12 * float(dwant.abs().max())


def test_surface_equals_its_autograd_and_is_negative_inside_the_mask():
    B, H, W = 2, 9, 11
    t = fx.object_plane('object', B, H, W)
    fg, bg = fx.surface_d2(t.numpy())
    p = fx.prob_plane(B, H, W).double().requires_grad_(True)
    f = fx.phi(t, fg, bg, F64)[:, None]
    want = (f * p).sum() / (B * H * W * math.sqrt(H * H + W * W))
    (dwant,) = torch.autograd.grad(want, p, torch.tensor(2.0, dtype=F64))
    want, f = want.detach(), f.detach()
    got = fx.surface(p.detach(), t, fg, bg, F64, g=2.0)
    assert float(got['loss']) == float(want) and torch.equal(got['dp'], dwant)
    assert bool((f[t > 0.5] < 0).all()) and bool((f[t < 0.5] > 0).all())
    assert float(fx.surface(t, t, fg, bg)['loss']) < 0 < float(fx.surface(1 - t, t, fg, bg)['loss'])
    for kind in ('empty', 'full'):                                   # the needed distance is NONE: phi = 0, not 2^15.5
        t = fx.object_plane(kind, B, H, W)
        fg, bg = fx.surface_d2(t.numpy())
        out = fx.surface(p.detach(), t, fg, bg)
        assert float(out['loss']) == 0.0 and not bool(out['dp'].any())


# --------------------------------------------------------------------------------------------- amplitude 0, by hand
def test_amplitude_zero_reproduces_the_unweighted_losses():
    logp, label, mask, d2 = _case()
    C = logp.shape[1]
    tgt = label[:, 0].long()
    tgt = torch.where((mask[:, 0] >= 0.5) & (tgt < C), tgt, torch.full_like(tgt, 255))
    got = fx.bw_nll(logp, label, mask, d2, 0.0, 5.0, F64)
    want = F.nll_loss(logp.double(), tgt, ignore_index=255)
    assert abs(float(got['loss'] - want)) <= 1e-14 * float(want) and float(got['sum_w']) == float((tgt != 255).sum())
    t, p = fx.object_plane('object', 2, 9, 11), fx.prob_plane(2, 9, 11)
    d2 = fx.boundary_d2(t.numpy())
    assert abs(float(fx.bw_pair(p, t, d2, 0.0, 5.0, 'bce')['loss'] - F.binary_cross_entropy(p.double(), t.double()))) < 1e-14
    assert abs(float(fx.bw_pair(p, t, d2, 0.0, 5.0, 'l1')['loss'] - F.l1_loss(p.double(), t.double()))) < 1e-14


def test_half_planes_weigh_the_two_boundary_columns_one_plus_amp():
    H, W, A, s = 4, 8, 3.0, 1.5
    label = torch.zeros(1, 1, H, W)
    label[..., W // 2:] = 1
    d2 = fx.boundary_d2(label.numpy())
    assert np.array_equal(d2[0, 0], [9, 4, 1, 0, 0, 1, 4, 9])
    w = fx.weight(d2, A, s, F64)
    assert bool((w[0, :, 3:5] == 1 + A).all())
    assert abs(float(w[0, 0, 0]) - (1 + A * math.exp(-9 / (2 * s * s)))) < 1e-15
    logp = torch.log(torch.tensor([0.25, 0.75])).view(1, 2, 1, 1).expand(1, 2, H, W).contiguous()
    out = fx.bw_nll(logp, label, torch.ones(1, 1, H, W), d2, A, s, F64)
    cols = w[0, 0]
    l0, l1 = float(logp[0, 0, 0, 0]), float(logp[0, 1, 0, 0])        # log 0.25, log 0.75 as fp32 holds them
    want = float((cols[:4].sum() * -l0 + cols[4:].sum() * -l1) / cols.sum())
    assert abs(float(out['loss']) - want) < 1e-14
    uniform = fx.weight(fx.boundary_d2(torch.zeros(1, 1, H, W).numpy()), A, s, F64)
    assert bool((uniform == 1).all())                                # no boundary: NONE everywhere, weight exactly 1


# ------------------------------------------------------------------------------------------------- planted defects
def _differs(a, b):
    return abs(float(a) - float(b)) > 1e-6 * max(abs(float(b)), 1e-30)


def test_planted_defects_change_the_result():
    logp, label, mask, d2 = _case()
    A, s = 4.0, 1.0
    good = fx.bw_nll(logp, label, mask, d2, A, s)
    assert _differs(fx.bw_nll(logp, label, mask, d2, A, s, denominator='count')['loss'], good['loss'])
    assert _differs(fx.bw_nll(logp, label, mask, d2, A, s, exponent='d')['loss'], good['loss'])
    bad = fx.bw_nll(logp, label, mask, d2, A, s, exponent='d')['dlogp']
    assert float((bad - good['dlogp']).abs().max()) > 1e-2 * float(good['dlogp'].abs().max())
    t, p = fx.object_plane('object', 2, 9, 11), fx.prob_plane(2, 9, 11)
    od2 = fx.boundary_d2(t.numpy())
    for kind in ('bce', 'l1'):
        ok = fx.bw_pair(p, t, od2, A, s, kind)
        assert _differs(fx.bw_pair(p, t, od2, A, s, kind, denominator='count')['loss'], ok['loss'])
        assert _differs(fx.bw_pair(p, t, od2, A, s, kind, exponent='d')['loss'], ok['loss'])
    # NONE through exp: invisible at sigma 1 (underflow), plain at sigma 1000 where exp(-(2^31 - 1) / 2e6) is not 0
    none = np.full((2, 9, 11), fx.NONE, np.int32)
    assert bool((fx.weight(none, 1.0, 1000.0, F64) == 1).all())
    assert bool((fx.weight(none, 1.0, 1e5, F64, none='exp') > 1.5).all())
    e = fx.object_plane('empty', 2, 9, 11)
    assert _differs(fx.bw_pair(p, e, none, 1.0, 1e5, 'bce', none='exp')['sum_w'], fx.bw_pair(p, e, none, 1.0, 1e5, 'bce')['sum_w'])
    fg, bg = fx.surface_d2(t.numpy())
    ok = fx.surface(p, t, fg, bg)
    flipped = fx.surface(p, t, fg, bg, phi_sign=-1)
    assert float(flipped['loss']) == -float(ok['loss']) != 0.0 and torch.equal(flipped['dp'], -ok['dp'])
    gate = fx.mask_plane('object', 2, 9, 11)
    lab2 = fx.label_plane('object', 2, 4, 9, 11)
    lp2 = fx.logp_planes(2, 4, 9, 11)
    a = fx.trainer_terms(lp2, p, lab2, gate, t, A, s)
    b = fx.trainer_terms(lp2, p, lab2, gate, t, A, s, use_gate=False)
    assert _differs(b['obj'], a['obj']) and _differs(b['surface'], a['surface']) and float(a['comb']) == float(b['comb'])


def test_fp32_form_is_close_and_not_identical():
    logp, label, mask, d2 = _case(3, 35, 17, 33)
    r64, r32 = fx.bw_nll(logp, label, mask, d2, 4.0, 1.0, F64), fx.bw_nll(logp, label, mask, d2, 4.0, 1.0, F32)
    assert r32['loss'].dtype == F32 and r32['dlogp'].dtype == F32
    assert abs(float(r32['loss']) - float(r64['loss'])) <= 1e-5 * float(r64['loss'])


# --------------------------------------------------------------------------------------- library, parser, refusals
def test_the_library_exports_the_symbols_and_the_header_declares_them():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        header = f.read()
    dll = _cabi.lib._load()
    for name in SYMBOLS:
        assert name in _cabi._SIGS and hasattr(dll, name), name
        assert re.search(r'\b(int|size_t) %s\(' % name, header), name
    ws = int(_cabi.lib.him_bw_loss_ws())
    assert ws >= 64 * 16 and ws % 8 == 0


def test_the_training_parser_carries_the_three_settings_and_nothing_else_moves():
    from neurips18_hierchical_image_manipulation_amd import options
    assert options.BOUNDARY_ATTRS == (('boundary_weight', float, 0.0), ('boundary_sigma', float, 5.0),
                                      ('surface_weight', float, 0.0))
    plain = options.BoxToMaskTrainOptions().parse(save=False, default_args=[])
    assert (plain.boundary_weight, plain.boundary_sigma, plain.surface_weight) == (0.0, 5.0, 0.0)
    opt = options.BoxToMaskTrainOptions().parse(save=False, default_args=['--boundary_weight', '2'])
    assert opt.boundary_weight == 2.0 and type(opt.boundary_weight) is float
    opt = options.BoxToMaskTrainOptions().parse(
        save=False, default_args=['--surface_weight', '0.5', '--boundary_sigma', '3', '--use_gan', '--ema_decay', '0.9'])
    assert (opt.surface_weight, opt.boundary_sigma, opt.use_gan, opt.ema_decay) == (0.5, 3.0, True, 0.9)
    # the argparse tables are the reference's (tests/golden/option_defaults.json); the settings travel as attributes only
    names = {n for n, _, _ in options.BOUNDARY_ATTRS}
    for table in options.BoxToMaskTrainOptions.tables:
        assert not names & {n for n, _, _ in table}
    rest = {k: v for k, v in vars(plain).items() if k not in names}
    test_side = vars(options.BoxToMaskTestOptions().parse(save=False, default_args=[]))
    assert not names & set(test_side)                                # a training setting: the test parser has none of it
    assert set(rest) == (set(test_side) | {n for n, _, _ in options.BOX2MASK_TRAIN_FLAGS}) - \
        ({n for n, _, _ in options.BOX2MASK_TEST_FLAGS} - {n for n, _, _ in options.BOX2MASK_TRAIN_FLAGS})
    with pytest.raises(SystemExit):
        options.BoxToMaskTestOptions().parse(save=False, default_args=['--boundary_weight', '2'])


def test_host_side_refusals():
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd.models.mask_losses import MaskReconLoss
    p, t = torch.rand(1, 1, 4, 4), torch.zeros(1, 1, 4, 4)
    logp = torch.zeros(1, 3, 4, 4)
    for call in (lambda: ops.boundary_weighted_bce(p, t, 1.0, 1.0), lambda: ops.boundary_weighted_l1(p, t, 1.0, 1.0),
                 lambda: ops.surface_loss(p, t), lambda: ops.boundary_weighted_nll(logp, t, t, 1.0, 1.0)):
        with pytest.raises(ValueError, match='device tensor'):
            call()
    for amp, sigma in ((-1.0, 1.0), (1.0, 0.0), (1.0, -2.0), (float('nan'), 1.0), (1.0, float('inf')), (float('inf'), 1.0)):
        with pytest.raises(ValueError, match='amp'):
            ops.boundary_weighted_bce(p, t, amp, sigma)
        with pytest.raises(ValueError, match='amp'):
            ops.boundary_weighted_nll(logp, t, t, amp, sigma)
    with pytest.raises(ValueError):
        MaskReconLoss(boundary_weight=-1.0)
    with pytest.raises(ValueError):
        MaskReconLoss(boundary_weight=1.0, boundary_sigma=0.0)
    m = MaskReconLoss()
    assert (m.boundary_weight, m.boundary_sigma) == (0.0, 5.0)
