"""-m gpu: the Python layers of the sliced Wasserstein distance (ops.lap_pyramid / sort_segments / sliced_wasserstein,
util.metrics.sliced_wasserstein and Evaluator(swd=...)) against the numpy restatement of tests/swd_fixture.py.

The distance is a mean of differences of sorted projections and may cancel, so its error and the fp32 twin's e32 are both
taken in units of the largest |projection| of the level; the bound is the direct-form rule max(8 e32, 16 2^-24)."""
import numpy as np
import pytest
import torch

import swd_fixture as fx
from neurips18_hierchical_image_manipulation_amd import ops
from neurips18_hierchical_image_manipulation_amd.util import metrics

pytestmark = pytest.mark.gpu

KW = dict(n_patches=16, n_dirs=64, seed=4)
_SETS = {}


def sets():
    """16 seeded 3 x 32 x 64 images per set and the fixture's answer in float64 and fp32, computed once."""
    if not _SETS:
        fake, real = fx.images(21, 16, 3, 32, 64), fx.images(22, 16, 3, 32, 64) * 0.8 + 0.05
        _SETS.update(fake=fake, real=real.astype(np.float32))
        _SETS['ref64'] = fx.swd(_SETS['fake'], _SETS['real'], 16, 64, seed=4)
        _SETS['ref32'] = fx.swd(_SETS['fake'], _SETS['real'], 16, 64, seed=4, dtype=np.float32)
    return _SETS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_levels_match_the_fixture_within_the_direct_form_bound():
    s = sets()
    got = metrics.sliced_wasserstein(dev(s['fake']), dev(s['real']), **KW).cpu().numpy()
    assert got.shape == (2,) and got.dtype == np.float64
    for l, (r64, r32) in enumerate(zip(s['ref64'], s['ref32'])):
        scale = max(np.abs(r64['proj_a']).max(), np.abs(r64['proj_b']).max())
        err, e32 = abs(got[l] - r64['dist']) / scale, abs(r32['dist'] - r64['dist']) / scale
        print('level %d: got %.9e ref %.9e err %.3e e32 %.3e limit %.3e' % (l, got[l], r64['dist'], err, e32,
                                                                           fx.direct_limit(e32)))
        assert err <= fx.direct_limit(e32), (l, got[l], r64['dist'], err, e32)
    assert (got > 0).all()


def test_ops_layers_agree_with_the_fixture():
    s = sets()
    laps, gauss = ops.lap_pyramid(dev(s['fake']), want_gauss=True)
    l64, g64 = fx.pyramid(s['fake'])
    l32, g32 = fx.pyramid(s['fake'], dtype=np.float32)
    assert len(laps) == 2 and len(gauss) == 1
    for l in range(2):
        fx.check_direct('ops', 'lap%d' % l, laps[l].cpu().numpy(), l64[l], l32[l])
    fx.check_direct('ops', 'gauss1', gauss[0].cpu().numpy(), g64[1], g32[1])
    x = fx.sort_input('nans', 3, 5, 1000)
    keys, status = ops.sort_segments(dev(x))
    fx.check_sorted_bits('ops', keys.cpu().numpy(), x, int(status.item()))
    one, status = ops.sort_segments(dev(x[0]))
    fx.check_sorted_bits('ops 1-d', one.cpu().numpy()[None], x[:1], int(status.item()))
    with pytest.raises(ValueError, match='levels'):
        ops.lap_pyramid(dev(s['fake']), levels=3)
    with pytest.raises(ValueError, match='descriptors'):
        ops.sliced_wasserstein(torch.zeros(4, 49).cuda(), torch.zeros(5, 49).cuda(), None, None, None)


def test_identical_sets_with_the_same_positions_give_exactly_zero():
    s = sets()
    x = dev(s['fake'])
    got = metrics.sliced_wasserstein(x, x.clone(), same_positions=True, **KW).cpu().numpy()
    assert got.tolist() == [0.0, 0.0]
    other = metrics.sliced_wasserstein(x, x.clone(), **KW).cpu().numpy()
    assert (other > 0).all()                                    # other corners: another sample of the same set


def test_a_blurred_set_loses_more_on_the_finest_level():
    s = sets()
    real = s['real']
    blurred = fx.up(fx.down(real.astype(np.float64))).astype(np.float32)       # one down / up round trip
    got = metrics.sliced_wasserstein(dev(blurred), dev(real), same_positions=True, **KW).cpu().numpy()
    assert np.isfinite(got).all() and got[0] > got[-1], got


def test_evaluator_in_three_batches_equals_the_one_shot_function_bit_for_bit():
    s = sets()
    fake, real = dev(s['fake']), dev(s['real'])
    ev = metrics.Evaluator(35, swd=KW)
    for a, b in ((0, 5), (5, 6), (6, 16)):                      # 5 + 1 + 10 images: the buffers grow twice
        ev.add_image(fake[a:b], real[a:b])
    out = ev.summary()
    once = metrics.sliced_wasserstein(fake, real, **KW).cpu().numpy()
    assert out['swd_descriptors'] == 16 * 16 and out['n_images'] == 16
    assert out['swd_levels'] == [float(v) for v in once * 1e3]
    assert out['swd'] == float((once * 1e3).mean())
    assert list(out) == list(metrics.SUMMARY_KEYS + metrics.SWD_KEYS)
    assert int(ev._swd.clamped.item()) == 0


def test_a_constant_channel_gives_nan_on_its_level_only():
    """A checkerboard channel: [1, 4, 6, 4, 1] sums an alternating signal to exactly 0 (mirrored borders keep the
    alternation), so the channel is constant on the last level, where the distance must be NaN, and a full-contrast
    pattern on level 0, which stays finite."""
    s = sets()
    yy, xx = np.mgrid[0:32, 0:64]
    fake, real = s['fake'].copy(), s['real'].copy()
    fake[:, 1] = real[:, 1] = (0.5 * (-1.0) ** (yy + xx)).astype(np.float32)
    ref = fx.swd(fake, real, 16, 64, seed=4)
    assert np.isnan(ref[1]['dist']) and np.isfinite(ref[0]['dist'])
    got = metrics.sliced_wasserstein(dev(fake), dev(real), **KW).cpu().numpy()
    assert np.isfinite(got[0]) and np.isnan(got[1]), got
    ev = metrics.Evaluator(35, swd=KW).add_image(dev(fake), dev(real))
    out = ev.summary()
    assert np.isfinite(out['swd_levels'][0]) and np.isnan(out['swd_levels'][1]) and np.isnan(out['swd'])


def test_evaluator_without_swd_keeps_its_keys():
    s = sets()
    ev = metrics.Evaluator(35).add_image(dev(s['fake'][:2]), dev(s['real'][:2]))
    out = ev.summary()
    assert list(out) == list(metrics.SUMMARY_KEYS) and out['n_images'] == 2
    assert not any(k.startswith('swd') for k in out)
