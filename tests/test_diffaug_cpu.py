"""Differentiable augmentation without a GPU: the Python mirror of the parameter draw, the flags, the exported symbols,
and the float64 restatement (diffaug_fixture) against torch.autograd, which makes it the oracle of the GPU tests."""
import ctypes
import os

import pytest
import torch

import diffaug_fixture as F
from neurips18_hierchical_image_manipulation_amd import augment

SHAPES = [(5, 7), (16, 16), (256, 512)]


def _triples(n):
    """n (seed, step, sample0) triples spread over small, large and negative values (a 64-bit LCG: deterministic)."""
    out, s = [], 12345
    for i in range(n):
        s = (s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out.append(((s >> 40) - (1 << 23) if i % 3 else i, (s >> 20) % 100003 if i % 2 else i, (s >> 8) % 4099))
    return out


def test_draw_is_deterministic():
    a = augment.draw(4, 16, 24, 7, 3, 0, 7)
    assert a == augment.draw(4, 16, 24, 7, 3, 0, 7)
    # a batch is the same rows as its samples drawn one by one: a row depends on (seed, step, sample0 + b) alone
    singles = [augment.draw(1, 16, 24, 7, 3, b, 7)[0][0] for b in range(4)]
    assert a[0] == singles


@pytest.mark.parametrize('H,W', SHAPES)
def test_every_field_lies_in_its_range(H, W):
    sy, sx, ch, cw = augment.sizes(H, W, 7)
    assert (sy, sx) == (int(H * 0.125 + 0.5), int(W * 0.125 + 0.5)) and (ch, cw) == (int(H * 0.5 + 0.5), int(W * 0.5 + 0.5))
    seen = {k: set() for k in ('ty', 'tx', 'cy', 'cx')}
    for seed, step, sample in _triples(3000):
        rows, h, w = augment.draw(1, H, W, seed, step, sample, 7)
        assert (h, w) == (ch, cw)
        r = rows[0]
        assert all(-2 ** 31 <= v < 2 ** 31 for v in r)
        b, a, k = (F.bits_f32(v) for v in r[:3])
        assert -0.5 <= b < 0.5 and 0.0 <= a < 2.0 and 0.5 <= k <= 1.5
        assert -sy <= r[3] <= sy and -sx <= r[4] <= sx
        assert -(ch // 2) <= r[5] <= H - (ch % 2) - ch // 2
        assert -(cw // 2) <= r[6] <= W - (cw % 2) - cw // 2
        assert r[7] == 7
        for key, v in zip(('ty', 'tx', 'cy', 'cx'), r[3:7]):
            seen[key].add(v)
    # 3000 draws reach both ends of every integer range of the small planes
    if (H, W) != (256, 512):
        assert seen['ty'] == set(range(-sy, sy + 1)) and seen['tx'] == set(range(-sx, sx + 1))
        assert seen['cy'] == set(range(-(ch // 2), H - (ch % 2) - ch // 2 + 1))
        assert seen['cx'] == set(range(-(cw // 2), W - (cw % 2) - cw // 2 + 1))


def test_rows_differ_across_seed_step_and_sample():
    base = augment.draw(1, 256, 512, 1, 2, 3, 7)[0][0]
    assert augment.draw(1, 256, 512, 2, 2, 3, 7)[0][0] != base
    assert augment.draw(1, 256, 512, 1, 3, 3, 7)[0][0] != base
    assert augment.draw(1, 256, 512, 1, 2, 4, 7)[0][0] != base
    # the three arguments are not interchangeable
    assert augment.draw(1, 256, 512, 2, 1, 3, 7)[0][0] != augment.draw(1, 256, 512, 1, 2, 3, 7)[0][0]
    rows = augment.draw(64, 256, 512, 0, 0, 0, 7)[0]
    assert len({tuple(r) for r in rows}) == 64
    for col in range(7):
        assert len({r[col] for r in rows}) > 32, col


@pytest.mark.parametrize('policy', range(8))
def test_a_policy_without_a_member_clears_its_bit_and_leaves_neutral_values(policy):
    full = augment.draw(3, 16, 16, 5, 6, 0, 7)
    rows, ch, cw = augment.draw(3, 16, 16, 5, 6, 0, policy)
    assert (ch, cw) == ((8, 8) if policy & 4 else (0, 0))
    for r, f in zip(rows, full[0]):
        assert r[7] == policy
        assert r[:3] == (f[:3] if policy & 1 else [F.f32_bits(0.0), F.f32_bits(1.0), F.f32_bits(1.0)])
        assert r[3:5] == (f[3:5] if policy & 2 else [0, 0])
        assert r[5:7] == (f[5:7] if policy & 4 else [0, 0])


def test_zero_ratios_draw_the_identity():
    rows, ch, cw = augment.draw(8, 32, 64, 1, 1, 0, 6, 0.0, 0.0)
    # no shift and an EMPTY rectangle (its corner is still drawn, from [0, H] x [0, W])
    assert (ch, cw) == (0, 0) and all(r[3:5] == [0, 0] and 0 <= r[5] <= 32 and 0 <= r[6] <= 64 for r in rows)
    x = torch.randn(8, 4, 32, 64, generator=torch.Generator().manual_seed(1))
    assert torch.equal(F.forward(x, rows, ch, cw, 1), x)


def test_policy_strings():
    assert augment.parse_policy('') == 0 and augment.parse_policy(None) == 0
    assert augment.parse_policy('color') == 1 and augment.parse_policy('translation') == 2
    assert augment.parse_policy('cutout') == 4 and augment.parse_policy('color,translation,cutout') == 7
    assert augment.parse_policy('cutout, color') == 5
    for bad in ('colour', 'color;cutout', 'color,', 'all', 'flip', 7):
        with pytest.raises(ValueError):
            augment.parse_policy(bad)


def test_parser_defaults_and_types():
    from neurips18_hierchical_image_manipulation_amd import options
    opt = options.MaskToImageTrainOptions().parse(save=False, default_args=[])
    assert (opt.diffaug, opt.diffaug_seed, opt.diffaug_translation, opt.diffaug_cutout) == ('', 0, 0.125, 0.5)
    assert type(opt.diffaug) is str and type(opt.diffaug_seed) is int
    assert type(opt.diffaug_translation) is float and type(opt.diffaug_cutout) is float
    opt = options.MaskToImageTrainOptions().parse(save=False, default_args=[
        '--diffaug', 'color,cutout', '--diffaug_seed', '9', '--diffaug_translation', '0.25', '--diffaug_cutout', '0.3'])
    assert (opt.diffaug, opt.diffaug_seed, opt.diffaug_translation, opt.diffaug_cutout) == ('color,cutout', 9, 0.25, 0.3)
    done = options.complete(dict(model='pix2pixHD_condImg'))
    assert (done.diffaug, done.diffaug_seed, done.diffaug_translation, done.diffaug_cutout) == ('', 0, 0.125, 0.5)
    # the test-time parser and the box2mask parsers do not know the flags
    for cls in (options.MaskToImageTestOptions, options.BoxToMaskTrainOptions, options.BoxToMaskTestOptions):
        with pytest.raises(SystemExit):
            cls().parse(save=False, default_args=['--diffaug', 'color'])


def test_symbols_are_exported_by_the_built_library():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    names = ('him_diffaug_ws', 'him_diffaug_fwd', 'him_diffaug_bwd', 'him_diffaug_draw')
    assert set(names) <= set(_cabi.EXPORTS)
    assert os.path.isfile(_cabi.LIB_PATH), 'libhim_hip.so is not built'
    with open(_cabi.LIB_PATH, 'rb') as f:
        blob = f.read()
    for n in names:
        assert n.encode() + b'\0' in blob, n
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'him.h')).read()
    for n in names:
        assert n + '(' in header, n
    assert ctypes.sizeof(ctypes.c_longlong) == 8


# ------------------------------------------------------------------------------------------------ the oracle itself
def _rows_for(B, H, W, ch, cw):
    """Every kind of row once: colour only, geometry only, everything, shifts past the plane, cutouts over the edges."""
    rows = [F.row(0.3, 0.4, 1.3, 1, -2, 1, 2, 7), F.row(-0.2, 1.7, 0.6, -1, 3, -1, W - 2, 7), F.row(0.1, 0.0, 0.5, 0, 0, 0, 0, 1),
            F.row(0.4, 2.0, 1.5, 2, 1, H - 1, -1, 6), F.row(0.25, 0.5, 0.75, H, 0, 0, 0, 3), F.row(0.0, 1.0, 1.0, 0, -W - 3, 0, 0, 2),
            F.row(-0.5, 1.2, 0.9, 0, 1, -ch, -cw, 5), F.row(0.2, 0.8, 1.1, -2, -1, 0, 0, 0)]
    return [rows[i % len(rows)] for i in range(B)]


@pytest.mark.parametrize('B,C,c0,H,W,ch,cw', [(8, 3, 0, 5, 7, 2, 3), (8, 7, 4, 6, 6, 3, 3), (8, 5, 1, 4, 9, 9, 9), (8, 4, 0, 3, 3, 0, 2)])
def test_restated_backward_is_autograd_of_the_restated_forward(B, C, c0, H, W, ch, cw):
    g = torch.Generator().manual_seed(B * 1000 + C * 100 + H)
    rows = _rows_for(B, H, W, ch, cw)
    for policy in (7, 6, 1, 5):
        x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        dout = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
        y = F.forward(x, rows, ch, cw, c0, policy)
        (auto,) = torch.autograd.grad(y, x, dout)
        mine, S = F.backward(dout, rows, ch, cw, c0, policy)
        assert float((auto - mine).abs().max()) <= 1e-14 * max(1.0, float(auto.abs().max())), policy
        # S_b is the sum of what the geometric adjoint routes back to the image channels
        g_all = F.routed(dout, rows, ch, cw, policy)
        for b in range(B):
            want = g_all[b, c0:c0 + 3].sum() if rows[b][7] & policy & 1 else 0.0
            assert abs(float(S[b]) - float(want)) <= 1e-12


def test_restated_forward_properties():
    """The statements of the issue, checked on the restatement: geometric rows only copy and zero; brightness and saturation
    leave the sample mean at mean(x) + b; the forward with b = 0 is linear."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 5, 6, 8, generator=g, dtype=torch.float64)
    rows = [F.row(0.3, 0.4, 1.3, 2, -3, 1, 2, 6), F.row(0.3, 0.4, 1.0, 0, 0, 0, 0, 1)]
    y = F.forward(x, rows, 3, 4, 1)
    # out[y, x] = in[y + 2, x - 3]: row 0 lies above the cutout (rows 1..3, columns 2..5), columns 6..7 beside it
    assert torch.equal(y[0, :, 0, 3:8], x[0, :, 2, 0:5]) and torch.equal(y[0, :, 1:4, 6:8], x[0, :, 3:6, 3:5])
    assert bool((y[0, :, 1:4, 2:6] == 0).all()) and bool((y[0, :, 4:, :] == 0).all()) and bool((y[0, :, :, :3] == 0).all())
    assert torch.equal(y[1, 0], x[1, 0]) and torch.equal(y[1, 4], x[1, 4])
    assert abs(float(y[1, 1:4].mean()) - (float(x[1, 1:4].mean()) + F.bits_f32(rows[1][0]))) < 1e-12
    lin = [F.row(0.0, 0.4, 1.3, 1, -1, 1, 2, 7)] * 2
    u, v = torch.randn(2, 2, 5, 6, 8, generator=g, dtype=torch.float64)
    both = F.forward(2.0 * u - 3.0 * v, lin, 3, 4, 1)
    assert float((both - (2.0 * F.forward(u, lin, 3, 4, 1) - 3.0 * F.forward(v, lin, 3, 4, 1))).abs().max()) < 1e-12
