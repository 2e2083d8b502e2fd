"""-m gpu: the Python layers of the k-nearest-neighbour measures (ops.knn_radii / knn_membership,
util.metrics.FeatureDistance.prdc, prdc_from_counts, feature_prdc and Evaluator(features=dict(nearest_k=...))) against
the float64 restatement of tests/prdc_fixture.py.  The radii are held to the fixture's radius bound; the counts come from
chained calls (the kernel's radii feed the kernel's membership test), so a decision is certain when its reference margin
exceeds e_ij plus the radius bound -- which holds for every decision of the cases used here (tests/test_prdc_cpu.py
asserts it), so the counts, and with them the four measures, are compared for equality."""
import numpy as np
import pytest
import torch

import featdist_fixture as ffx
import prdc_fixture as fx
from neurips18_hierchical_image_manipulation_amd import ops, synth
from neurips18_hierchical_image_manipulation_amd.models.layer_util import Vgg19
from neurips18_hierchical_image_manipulation_amd.util import metrics

pytestmark = pytest.mark.gpu

_SHARED = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def vgg():
    if 'vgg' not in _SHARED:
        net = Vgg19()
        net.load_state_dict(synth.init_state_dict(net.state_dict(), 3, 'vgg'))
        _SHARED['vgg'] = net.cuda()
    return _SHARED['vgg']


def case(index):
    """(fake, real, k, reference counts) of fixture.REAL_CASES[index], computed once."""
    if index not in _SHARED:
        fake, real, k = fx.real_case(index)
        _SHARED[index] = (fake, real, k, fx.counts(real, fake, k))
    return _SHARED[index]


@pytest.mark.parametrize('index', [6, 7], ids=lambda i: '%dx%d' % fx.REAL_CASES[i][1:3])          # 40 x 24 and 130 x 67
def test_ops_agree_with_the_fixture(index):
    fake, real, k, (row_fr, col_r, row_rf) = case(index)
    tag = 'ops %dx%d' % real.shape
    for q, r, want_rows, want_cols in ((fake, real, row_fr, col_r), (real, fake, row_rf, None)):
        r2, status = ops.knn_radii(dev(r), k)
        assert r2.dtype == torch.float64 and r2.is_cuda and tuple(r2.shape) == (len(r),)
        fx.check_bound(tag, 'radii2', r2.cpu().numpy(), fx.radii(r, k), fx.radii_bound(r))
        lo_r, hi_r, lo_c, hi_c, uncertain = fx.membership_bounds(q, r, fx.radii(r, k), fx.radii_bound(r))
        assert uncertain == 0 and (lo_r == want_rows).all()
        rows, cols, status2 = ops.knn_membership(dev(q), dev(r), r2, status=status)
        assert status2 is status and int(status.item()) == 0
        assert rows.dtype == torch.int32 and cols.dtype == torch.int32 and rows.is_cuda
        fx.check_counts(tag, 'row_count', rows.cpu().numpy(), lo_r, hi_r)
        fx.check_counts(tag, 'col_count', cols.cpu().numpy(), lo_c, hi_c)
        if want_cols is not None:
            assert (cols.cpu().numpy() == want_cols).all()
        rows2, none, _ = ops.knn_membership(dev(q), dev(r), r2, want_cols=False)
        assert none is None and torch.equal(rows2, rows)
        again, _ = ops.knn_radii(dev(r), k)
        assert torch.equal(again, r2)                                                    # identical bits from run to run


def test_feature_distance_prdc_equals_the_fixture_and_does_not_depend_on_the_batching():
    fake, real, k, ref = case(7)
    want = fx.prdc_from_counts(k, *ref)
    fd = metrics.FeatureDistance(nearest_k=k).add_features(dev(fake), dev(real))
    kk, row_fr, col_r, row_rf, status = fd.prdc_counts()
    assert kk == k and int(status.item()) == 0
    for got, w in zip((row_fr, col_r, row_rf), ref):
        assert (got.cpu().numpy() == w).all()
    got = fd.prdc()
    assert list(got) == list(want) == list(metrics.PRDC_KEYS[:4])
    for key in want:
        assert got[key].dtype == torch.float64 and got[key].is_cuda and got[key].dim() == 0
        assert abs(float(got[key]) - want[key]) <= 4 * fx.U * max(want[key], 1.0), key
    other = fd.prdc(3)                                                                   # another k on the same rows
    want3 = fx.prdc(real, fake, 3)
    assert all(abs(float(other[key]) - want3[key]) <= 4 * fx.U * max(want3[key], 1.0) for key in want3)
    # rows added as 2 + 3 give the bits of 5 at once
    once = metrics.FeatureDistance(nearest_k=2).add_features(dev(fake[:5]), dev(real[:5])).prdc()
    cut = metrics.FeatureDistance(nearest_k=2).add_features(dev(fake[:2]), dev(real[:2]))
    cut = cut.add_features(dev(fake[2:5]), dev(real[2:5])).prdc()
    assert all(torch.equal(once[key], cut[key]) for key in once)
    # at most k rows in either set: NaN for all four keys
    few = metrics.FeatureDistance(nearest_k=5).add_features(dev(fake[:5]), dev(real[:9])).prdc()
    assert all(v.is_cuda and bool(v != v) for v in few.values())
    with pytest.raises(ValueError, match='knn_radii'):
        ops.knn_radii(dev(fake[:5]), 5)
    with pytest.raises(ValueError, match='radii2'):
        ops.knn_membership(dev(fake), dev(real), torch.zeros(3, dtype=torch.float64).cuda())


def test_evaluator_adds_the_prdc_keys_only_when_asked():
    net = vgg()
    fake, real = dev(ffx.images(9, 6, 32, 32)), dev(ffx.images(10, 6, 32, 32))
    kw = dict(layers=(4,), n_subsets=3, subset_size=4, seed=1, vgg=net)
    ev = metrics.Evaluator(35, features=dict(kw, nearest_k=3))
    ev.add_image(fake[:2], real[:2]).add_image(fake[2:], real[2:])
    out = ev.summary()
    assert list(out) == list(metrics.SUMMARY_KEYS + metrics.FEATURE_KEYS + metrics.PRDC_KEYS)
    assert out['nearest_k'] == 3 and out['n_features'] == 6
    for key in ('precision', 'recall', 'coverage'):
        assert isinstance(out[key], float) and np.isfinite(out[key]) and 0.0 <= out[key] <= 1.0, (key, out[key])
    assert np.isfinite(out['density']) and out['density'] >= 0.0
    fd = metrics.FeatureDistance(**kw).add(fake, real)
    x, y = fd.features(0).cpu().numpy(), fd.features(1).cpu().numpy()
    print('evaluator prdc', {key: out[key] for key in metrics.PRDC_KEYS}, 'fixture', fx.prdc(y, x, 3))
    plain = metrics.Evaluator(35, features=kw)
    plain.add_image(fake[:2], real[:2]).add_image(fake[2:], real[2:])
    base = plain.summary()
    assert list(base) == list(metrics.SUMMARY_KEYS + metrics.FEATURE_KEYS)               # exactly today's keys
    assert all(base[key] == out[key] or (base[key] != base[key] and out[key] != out[key]) for key in base)
    one = metrics.feature_prdc(fake, real, nearest_k=3, layers=(4,), vgg=net)
    assert list(one) == list(metrics.PRDC_KEYS[:4]) and all(float(one[key]) == out[key] for key in one)
