"""The weight-gradient plan as a table: him_conv2d_bwd_weight_plan / him_deconv2d_bwd_weight_plan over the grid of
tools/wgrad_plan_table.py (the conv, its transposed twin, the dense slice of a one-hot stem) against
tests/golden/wgrad_plan_table.json, written by the library as it was before the selection became WGradPlan
(csrc/him_conv.hip plan_wgrad), with a dry-run switch in its run_wgrad.  No GPU: the queries are host functions.

The parent's table is NOT sound everywhere: where its `need` exceeds its `slab` the call was refused at the reported
workspace size (HIM_E_WORKSPACE).  On this grid that is
  * every transposed conv and one-hot dense slice whose adjoint / dense conv has the F(2x2) weight-gradient shape: run_wgrad
    chose Winograd although neither caller reserves its transforms.  Both now plan without it (allow_wino = false);
  * the tiny-M 5x5 conv off the "same" geometry (EXTRA): 512 generic splits against the 256 slabs its class reserves.
Such rows, and the transposed-conv rows on which the parent's Winograd choice happened to fit (only under a wgrad_splits
override, which inflates the fast family's bound), are the only ones allowed to differ -- never in `slab`."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
_spec = importlib.util.spec_from_file_location('wgrad_plan_table', os.path.join(ROOT, 'tools', 'wgrad_plan_table.py'))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)
T = W.T
NF = len(W.FIELDS)
FAM, NEED, SPLITS, SLAB = (W.FIELDS.index(f) for f in ('family', 'need', 'splits', 'slab'))
WINO, GENERIC = W.FAMILIES.index('wino'), W.FAMILIES.index('generic')


@pytest.fixture(scope='module')
def tables():
    with open(W.GOLDEN) as f:
        return T.unpack(json.load(f)), W.table(W.load())


def parts(v):
    return {c: v[i * NF:(i + 1) * NF] for i, c in enumerate(W.CALLERS)}


def test_the_grid_is_the_committed_one(tables):
    want, got = tables
    for k in ('columns', 'descriptors', 'algos'):
        assert got[k] == want[k], 'tools/wgrad_plan_table.py no longer enumerates the committed grid (%s)' % k
    assert got['descriptors'][:-len(W.EXTRA)] == [list(d) for d in T.descriptors()] and got['algos'] == T.algos()


def test_every_plan_is_the_parents_selection(tables):
    want, got = tables
    w, g = T.expand(want), T.expand(got)
    assert set(w) == set(g) and len(w) == len(want['descriptors']) * len(want['algos'])
    bad, fixed = [], {c: set() for c in W.CALLERS}
    for key in sorted(w):
        for caller, a in parts(w[key]).items():
            b = parts(g[key])[caller]
            refused = a[FAM] >= 0 and a[NEED] > a[SLAB]
            no_wino = caller != 'conv' and a[FAM] == WINO
            if a == b:
                continue
            if (refused or no_wino) and a[SLAB] == b[SLAB] and b[NEED] <= b[SLAB] and not (no_wino and b[FAM] == WINO):
                fixed[caller].add(key[0])
                if no_wino and not refused:
                    assert want['algos'][key[1]].get('wgrad_splits', 0) > 1
                continue
            bad.append('%s | %s | %s: (golden, built) %s %s' % (want['descriptors'][key[0]], want['algos'][key[1]], caller, a, b))
    assert not bad, '%d plans moved:\n%s' % (len(bad), '\n'.join(bad[:20]))
    tiny5 = want['descriptors'].index(list(W.EXTRA[2]))
    assert fixed['conv'] == {tiny5}
    assert {want['descriptors'].index(list(d)) for d in W.EXTRA[:2]} <= fixed['onehot_dense']


def test_every_plan_fits_the_slab_region_it_reports(tables):
    _, got = tables
    n = {c: 0 for c in W.CALLERS}
    for key, v in T.expand(got).items():
        for caller, b in parts(v).items():
            if b[FAM] >= 0:
                n[caller] += 1
                assert b[NEED] <= b[SLAB], (got['descriptors'][key[0]], got['algos'][key[1]], caller, b)
    assert all(n.values()), n


def test_the_grid_reaches_every_family(tables):
    want, got = tables
    for tab in (want, got):
        conv = [parts(v)['conv'] for v in T.expand(tab).values()]
        assert {b[FAM] for b in conv} - {-1} == set(range(len(W.FAMILIES)))
        assert {b[SPLITS] > 1 for b in conv if b[FAM] == GENERIC} == {False, True}
    for caller in ('deconv', 'onehot_dense'):
        assert WINO not in {parts(v)[caller][FAM] for v in T.expand(got).values()}, caller
