"""The convolution dispatch as a table: every pure size / panel / layout query of the C ABI over the fixed grid of
tools/conv_plan_table.py (descriptors x HimAlgo overrides, conv and the transposed conv whose adjoint it is) against
tests/golden/conv_plan_table.json, written by the library as it was before the selection became ConvPlan
(csrc/him_conv.hip plan_fprop / plan_dgrad).  No GPU: the queries are host functions of the descriptor."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
_spec = importlib.util.spec_from_file_location('conv_plan_table', os.path.join(ROOT, 'tools', 'conv_plan_table.py'))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)


@pytest.fixture(scope='module')
def tables():
    with open(T.GOLDEN) as f:
        return T.unpack(json.load(f)), T.table(T.load())


def test_the_grid_is_the_committed_one(tables):
    want, got = tables
    for k in ('columns', 'descriptors', 'algos'):
        assert got[k] == want[k], 'tools/conv_plan_table.py no longer enumerates the committed grid (%s)' % k


def test_every_query_answers_as_before_the_plan(tables):
    want, got = tables
    w, g = T.expand(want), T.expand(got)
    assert set(w) == set(g) and len(w) == len(want['descriptors']) * len(want['algos'])
    bad = []
    for key in sorted(w):
        if w[key] != g[key]:
            diff = {c: (a, b) for c, a, b in zip(want['columns'], w[key], g[key]) if a != b}
            bad.append('%s | %s: (golden, built) %s' % (want['descriptors'][key[0]], want['algos'][key[1]], diff))
    assert not bad, '%d of %d rows moved:\n%s' % (len(bad), len(w), '\n'.join(bad[:20]))


def test_the_grid_reaches_every_family_and_every_answer(tables):
    want, _ = tables
    col = {c: i for i, c in enumerate(want['columns'])}
    rows = T.expand(want)
    for kind in ('panel_layout_fwd', 'panel_layout_bwd'):
        assert {v[col[kind]] for v in rows.values()} == {0, 1, 2, 3, 4}, kind
    for flag in ('in_act_fused', 'shares_fwd_panel', 'resblock_supported'):
        assert {v[col[flag]] for v in rows.values()} == {0, 1}, flag
    for size in ('fwd_keep_bytes', 'onehot_fwd_ws', 'resblock_ws'):
        assert {v[col[size]] > 0 for v in rows.values()} == {False, True}, size
    # split-K moves the workspace: some descriptor's fwd_ws and bwd_data_ws differ under ALGO_NO_SPLITK alone
    base, nosplit = want['algos'].index({}), want['algos'].index({'disable': T.A.ALGO_NO_SPLITK})
    for size in ('fwd_ws', 'bwd_data_ws', 'deconv_fwd_ws'):
        assert any(rows[(i, base)][col[size]] != rows[(i, nosplit)][col[size]] for i in range(len(want['descriptors']))), size
