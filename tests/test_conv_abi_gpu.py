"""-m gpu: every kernel selection of the convolution family (the HimAlgo fields and disable bits of include/him.h) through
the guarded C-ABI harness of tests/abi_harness.py against float64 -- see tests/README.md "How op tests bound errors".

One table (ROWS): shape, HimAlgo overrides, passes, and the relation of the override to the base selection on the same
inputs -- 'identical' (the code documents bit-identity: torch.equal), 'differs' (another summation order: not equal, which
proves the knob reached the library) or 'any' (with the reason).  Citations name the functions of csrc/ that hold the choice."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import abi_harness as H
from neurips18_hierchical_image_manipulation_amd import _cabi as A
from test_model_gpu import OUT as REPORT_DIR
from test_ops_gpu import CONV_CASES, DECONV_CASES, WINO_CASES, WINO4_CASES, ONEHOT_CASES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HIM_H = os.path.join(HERE, '..', 'include', 'him.h')
OUT = os.path.join(REPORT_DIR, 'conv_abi_rows.jsonl')      # next to the model tests' trajectory reports
ALL3 = ('fwd', 'bwd_data', 'bwd_weight')
NOWINO = {'wino_min_c': -1}          # him_common.h algo_wino_min_c / him_conv.hip wino_fused_ok: every Winograd form off -> the direct form
WINO16 = {'wino_min_c': 16}          # separate-transform F(2x2) from 16 channels (the setting of WINO_CASES)


_CASES = {}


def case_of(c, act=None):
    key = (tuple(c), act)
    if key not in _CASES:
        if len(_CASES) >= 8:             # the float64 references of full-size cases are large: keep a few
            _CASES.pop(next(iter(_CASES)))
        _CASES[key] = H.DeconvCase(c, act or 'none') if len(c) == 5 else H.ConvCase(c)
    return _CASES[key]


def bound_for(lib, case, a, what):
    """The row class follows the kernel family the LIBRARY reports for (descriptor, HimAlgo) (him_conv2d_panel_layout:
    2 = F(2x2) separate transforms, 3 = fused F(2x2), 4 = F(4x4)); Winograd families keep the tolerances of
    test_winograd_conv3x3_fwd_bwd (2e-5, 5e-5 from 512 channels), test_persistent_fused_winograd_kernel (2e-5) and
    test_winograd_f4x4_frozen_conv_fwd_and_gated_dgrad (3e-5); everything else is a direct-form row."""
    if case.deconv:
        return H.DIRECT
    d = case.desc(a)
    wide = 5e-5 if case.Cin >= 512 else 2e-5
    if what == 'bwd_weight':
        # him_conv.hip wino_wgrad_ok: the F(2x2) layers with both channel counts % 128 == 0
        a2 = H.algo(**a.as_dict())       # the forward's F(4x4) marks do not move the weight gradient
        a2.disable &= ~(A.ALGO_FROZEN_WEIGHTS | A.ALGO_WINO4_TRAIN_FWD)
        wino = lib.him_conv2d_panel_layout(ctypes.byref(case.desc(a2)), 0) == 2
        return H.Bound(wide) if wino and case.Cin % 128 == 0 and case.Cout % 128 == 0 else H.DIRECT
    lay = lib.him_conv2d_panel_layout(ctypes.byref(d), 0 if what in ('fwd', 'in_act', 'fwd_keep_wgrad') else 1)
    return {2: H.Bound(wide), 3: H.Bound(2e-5), 4: H.Bound(3e-5)}.get(lay, H.DIRECT)


def run(case, over, what, **kw):
    lib = H.raw_lib()
    a = H.algo(**over)
    return H.run_pass(lib, case, a, what, bound=bound_for(lib, case, a, what), **kw)


@pytest.fixture(autouse=True)
def _dump():
    yield
    H.dump_report(OUT)


# ------------------------------------------------------------------------------------------------------ the matrix
ROWS = []


def row(name, case, passes, over, rel, base=None, why=None):
    assert rel in ('identical', 'differs') or (rel == 'any' and why), name
    ROWS.append({'name': name, 'case': case, 'passes': passes, 'over': over, 'base': base or {}, 'rel': rel, 'why': why})


def all_rows():
    return ROWS + [{'name': 'default', 'over': {k: 0 for k in ('tile_wb', 'tile_nb')}}] + EXTRA_ROWS


TAILS = (1, 160, 9, 13, 136, 3, 1, 1, 'reflect', 'none')        # CONV_CASES: M, N, K tails in every tile dimension
D160 = (2, 96, 9, 17, 160, 4, 1, 2, 'zero', 'none')             # Cout 160
ODD192 = (3, 256, 9, 13, 192, 3, 1, 1, 'zero', 'none')          # Cout 192, odd plane
SPLITK = (2, 256, 16, 32, 256, 3, 1, 1, 'reflect', 'none')      # CONV_CASES: "folded reflect dgrad under split-K"
S2BIG = (2, 136, 16, 32, 160, 3, 2, 1, 'zero', 'none')          # stride 2: the data gradient has four phases, M = Cin = 136
PATCH = (2, 64, 17, 33, 128, 4, 2, 2, 'zero', 'none')           # CONV_CASES: PatchGAN block (split-K slabs feed the norm)
DECONV = (2, 136, 4, 6, 72)                                     # DECONV_CASES: four phases, M = 72 fwd / 136 dgrad

# tile_nb: him_conv.hip launch_gconv -- read for M > 64 on the fast path only.  Every tile shape walks K in the same order, so
# the sums may or may not move: 'any' (the code promises neither); error bounds and guards are the check.
TILE_WHY = 'him_conv.hip launch_gconv: the tile shape changes the launch grid, the K loop order is not documented either way'
for code in range(1, 8):
    row('tile_nb=%d tails' % code, TAILS, ('fwd', 'bwd_data'), dict(NOWINO, tile_nb=code), 'any', NOWINO, TILE_WHY)
for code in (1, 2, 3, 5, 6, 7):
    row('tile_nb=%d cout160' % code, D160, ('fwd', 'bwd_data'), {'tile_nb': code}, 'any', None, TILE_WHY)
    row('tile_nb=%d split-K' % code, SPLITK, ('fwd', 'bwd_data'), dict(NOWINO, tile_nb=code), 'any', NOWINO, TILE_WHY)
for code in (1, 5, 6, 7):
    row('tile_nb=%d odd192' % code, ODD192, ('fwd', 'bwd_data'), dict(NOWINO, tile_nb=code), 'any', NOWINO, TILE_WHY)
for code in (1, 2, 4, 5, 6, 7):
    row('tile_nb=%d stride-2 phases' % code, S2BIG, ('fwd', 'bwd_data'), {'tile_nb': code}, 'any', None, TILE_WHY)
    row('tile_nb=%d deconv' % code, DECONV, ('fwd', 'bwd_data'), {'tile_nb': code}, 'any', None, TILE_WHY)

# tile_wb: him_conv.hip launch_gconv, p.wbatch -- the batched GEMM of the separate-transform Winograd layers when it runs on the conv
# kernel: always under NO_BGEMM (wino_batched_gemm), and without it where 16 * (M/128) * (N/128) < 512.
W128 = (1, 128, 6, 10, 128, 'reflect')       # WINO_CASES: 15 tiles -> 128 GEMM columns, 16 GEMM tiles: conv kernel either way
W256 = (2, 128, 8, 8, 256, 'zero')           # WINO_CASES: rectangular
W512 = (16, 512, 16, 16, 512, 'zero')        # WINO_CASES: 1024 columns, 16*4*8 = 512 tiles: the LDS-DMA GEMM unless NO_BGEMM


def wino(c):
    B, Cin, Hh, W, Cout, pm = c
    return (B, Cin, Hh, W, Cout, 3, 1, 1, pm, 'none')


for code in range(1, 8):
    row('tile_wb=%d' % code, wino(W128), ALL3, dict(WINO16, tile_wb=code), 'any', WINO16, TILE_WHY)
    row('tile_wb=%d NO_BGEMM' % code, wino(W256), ALL3, dict(WINO16, tile_wb=code, disable=A.ALGO_NO_BGEMM), 'any',
        dict(WINO16, disable=A.ALGO_NO_BGEMM), TILE_WHY)
for code in (1, 3, 6):
    row('tile_wb=%d NO_BGEMM 512ch' % code, wino(W512), ('fwd',), dict(tile_wb=code, disable=A.ALGO_NO_BGEMM), 'any',
        dict(disable=A.ALGO_NO_BGEMM), TILE_WHY)

# wgrad_tile x wgrad_splits: him_conv_wgrad.inc:423-435 (mirrored by wgrad_cfg below: the relation is computed from it)
WG_M = (4, 64, 24, 33, 136, 3, 1, 1, 'zero', 'none')            # M > 64, C % 128 != 0, K = 3168 positions
WG_C = (4, 128, 20, 24, 64, 3, 1, 1, 'reflect', 'none')         # M <= 64, C % 128 == 0, reflect gather
WG_99 = (8, 128, 9, 11, 256, 3, 1, 1, 'reflect', 'none')        # odd plane of 99 positions with a reflect gather, M > 64
WG_P = (3, 128, 8, 10, 256, 4, 1, 2, 'zero', 'none')            # CONV_CASES: PatchGAN plane 9x11 = 99, 4x4 window


def wgrad_cfg(case, tile, splits):
    B, C, Hh, W, M, k, s, p = case[:8]
    OH, OW = (Hh + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    BM = 128 if (M > 64 and tile == 0) else 64
    BN = 128 if (C % 128 == 0 and tile != 2) else 64
    tiles = -(-M // BM) * (C * k * k // BN)
    maxs = -(-B * OH * OW // 256)
    sp = max(1, min(maxs, 256, -(-768 // tiles)))
    if splits > 0:
        sp = max(1, min(maxs, splits))
    return BM, BN, sp


for c in (WG_M, WG_C, WG_99, WG_P):
    for tile in (0, 1, 2):
        for splits in (0, 1, 2, 3, 1000):
            if tile == 0 and splits == 0:
                continue
            got, base = wgrad_cfg(c, tile, splits), wgrad_cfg(c, 0, 0)
            rel = 'identical' if got == base else ('differs' if got[2] != base[2] else 'any')
            row('wgrad_tile=%d splits=%d %s' % (tile, splits, 'x'.join(map(str, c[:5]))), c, ('bwd_weight',),
                {'wgrad_tile': tile, 'wgrad_splits': splits}, rel, None,
                'him_conv_wgrad.inc:425-426: another tile, the same number of K slabs (%s vs %s)' % (got, base))

# split-K: him_conv.hip fast_ksplit; the default cap is 4
for over, rel in (({'disable': A.ALGO_NO_SPLITK}, 'differs'), ({'ksplit_max': 1}, 'differs'), ({'ksplit_max': 2}, 'any'),
                  ({'ksplit_max': 3}, 'any'), ({'ksplit_max': 8}, 'any')):
    why = 'him_conv.hip fast_ksplit: the cost model may pick the same factor under another cap'
    tag = ','.join('%s=%d' % kv for kv in over.items())
    row('%s conv' % tag, SPLITK, ('fwd', 'bwd_data'), dict(NOWINO, **over), rel, NOWINO, why)
    row('%s in_act' % tag, PATCH, ('fwd', 'in_act'), over, rel, None, why)

# wino_tblock: him_conv.hip wino_tblock "results are bit-identical"
for tb in (64, 128, 256):
    for c in ((1, 48, 9, 13, 32, 'reflect'), W128):
        row('wino_tblock=%d %s' % (tb, 'x'.join(map(str, c[:5]))), wino(c), ALL3, dict(WINO16, wino_tblock=tb), 'identical', WINO16)

# fused Winograd chunk: him_common.h algo_wino_fused_chunk (anything but 4 is 8); him_conv.hip wino_fused2_ok: chunk 4 also leaves the persistent kernel
FUSED = (2, 128, 16, 32, 128, 3, 1, 1, 'zero', 'relu')          # CONV_CASES: fused Winograd kernel, fwd + zero-pad dgrad
row('wino_fused_chunk=8', FUSED, ('fwd', 'bwd_data'), {'wino_fused_chunk': 8}, 'identical')
row('wino_fused_chunk=4', FUSED, ('fwd', 'bwd_data'), {'wino_fused_chunk': 4}, 'differs')
# thresholds moved across the channel count (him_conv.hip wino_shape_ok, wino_fused_ok; him_conv_wino4.inc wino4_shape_ok)
C32 = wino((2, 32, 16, 32, 32, 'reflect'))
C256 = (1, 256, 8, 16, 256, 3, 1, 1, 'zero', 'relu')            # CONV_CASES "VGG mid": separate transforms by default (>= 256)
row('wino_min_c=32 at 32 channels', C32, ALL3, {'wino_min_c': 32}, 'differs')
row('wino_min_c=33 at 32 channels', C32, ALL3, {'wino_min_c': 33}, 'identical')
row('wino_min_c<0 at 128 channels', FUSED, ('fwd', 'bwd_data'), NOWINO, 'differs')
row('wino_min_c=257 at 256 channels', C256, ('fwd', 'bwd_data'), {'wino_min_c': 257}, 'differs')
row('wino_fused_min_c<0', FUSED, ('fwd', 'bwd_data'), {'wino_fused_min_c': -1}, 'differs')
row('wino_fused_min_c=129 at 128 channels', FUSED, ('fwd', 'bwd_data'), {'wino_fused_min_c': 129}, 'differs')
row('wino_fused_min_c=128 at 128 channels', FUSED, ('fwd', 'bwd_data'), {'wino_fused_min_c': 128}, 'identical')
row('wino_fused_max_c=127 at 128 channels', FUSED, ('fwd', 'bwd_data'), {'wino_fused_max_c': 127}, 'differs')
row('wino_fused_max_c=256 at 256 channels', C256, ('fwd', 'bwd_data'), {'wino_fused_max_c': 256, 'wino_min_c': 257}, 'differs',
    {'wino_min_c': 257})
FROZEN = {'disable': A.ALGO_FROZEN_WEIGHTS}
W4 = (2, 256, 16, 32, 256, 3, 1, 1, 'zero', 'none')             # WINO4_CASES: 64 tiles of 4x4
row('wino4_min_c<0', W4, ('fwd', 'bwd_data'), dict(FROZEN, wino4_min_c=-1), 'differs', FROZEN)
row('wino4_min_c=257 at 256 channels', W4, ('fwd', 'bwd_data'), dict(FROZEN, wino4_min_c=257), 'differs', FROZEN)
row('wino4_min_c=256 at 256 channels', W4, ('fwd', 'bwd_data'), dict(FROZEN, wino4_min_c=256), 'identical', FROZEN)
row('FROZEN_WEIGHTS', W4, ('fwd', 'bwd_data'), FROZEN, 'differs')
row('WINO4_TRAIN_FWD', (8, 256, 16, 32, 256, 3, 1, 1, 'reflect', 'none'), ('fwd',), {'disable': A.ALGO_WINO4_TRAIN_FWD}, 'differs')
row('NO_BGEMM_PERSISTENT', W4, ('fwd',), {'disable': A.ALGO_FROZEN_WEIGHTS | A.ALGO_NO_BGEMM_PERSISTENT}, 'identical', FROZEN)
row('NO_WINO_FUSED2', FUSED, ('fwd', 'bwd_data'), {'disable': A.ALGO_NO_WINO_FUSED2}, 'differs')

# the disable bits the op tests never flipped, each at a shape (from CONV_CASES' comments) where it changes the kernel
KERNEL_WHY = 'another kernel for the same sums; whether its order differs is not documented at %s'
row('NO_DFOLD', (2, 16, 16, 32, 16, 3, 1, 1, 'reflect', 'none'), ('bwd_data',), {'disable': A.ALGO_NO_DFOLD}, 'any', None,
    KERNEL_WHY % 'him_conv.hip plan_dgrad (dfold)')
row('NO_DFOLD split-K', SPLITK, ('bwd_data',), dict(NOWINO, disable=A.ALGO_NO_DFOLD), 'any', NOWINO, KERNEL_WHY % 'him_conv.hip plan_dgrad (dfold)')
row('WINO_PADDED_DGRAD', C32, ('bwd_data',), dict(WINO16, disable=A.ALGO_WINO_PADDED_DGRAD), 'any', WINO16,
    KERNEL_WHY % 'him_conv.hip plan_dgrad (wino_fold)')
row('WINO_PADDED_DGRAD 4x4', wino((2, 32, 4, 4, 32, 'reflect')), ('bwd_data',), dict(WINO16, disable=A.ALGO_WINO_PADDED_DGRAD),
    'any', WINO16, KERNEL_WHY % 'him_conv.hip plan_dgrad (wino_fold)')
for c in ((2, 20, 9, 70, 2, 3, 1, 1, 'zero', 'none'), (1, 12, 70, 9, 4, 5, 1, 2, 'reflect', 'none'),
          (2, 8, 12, 66, 4, 7, 1, 3, 'reflect', 'none')):
    row('NO_SMALL_WIN %d' % c[5], c, ('bwd_weight',), {'disable': A.ALGO_NO_SMALL_WIN}, 'any', None, KERNEL_WHY % 'him_conv.hip small_win_ok')
for c in ((40, 16, 40, 70, 3, 7, 1, 3, 'reflect', 'none'), (34, 12, 33, 65, 4, 3, 1, 1, 'zero', 'none')):
    row('NO_FEWOUT_TILED %d' % c[5], c, ('fwd',), {'disable': A.ALGO_NO_FEWOUT_TILED}, 'any', None,
        KERNEL_WHY % 'him_conv_direct.inc:438')
row('NO_FEWOUT_TILED dgrad', (8, 2, 130, 250, 8, 3, 1, 1, 'zero', 'none'), ('bwd_data',), {'disable': A.ALGO_NO_FEWOUT_TILED}, 'any',
    None, KERNEL_WHY % 'him_conv_direct.inc:438')
row('NO_FEWIN_TILED fwd', (8, 4, 120, 250, 16, 7, 1, 3, 'zero', 'none'), ('fwd',), {'disable': A.ALGO_NO_FEWIN_TILED}, 'any', None,
    KERNEL_WHY % 'him_conv_direct.inc:593')
row('NO_FEWIN_TILED dgrad', (8, 16, 130, 250, 2, 3, 1, 1, 'zero', 'none'), ('bwd_data',), {'disable': A.ALGO_NO_FEWIN_TILED}, 'any',
    None, KERNEL_WHY % 'him_conv_direct.inc:593')
row('NO_FEWIN_FOLD', (8, 32, 128, 250, 3, 7, 1, 3, 'reflect', 'none'), ('bwd_data',), {'disable': A.ALGO_NO_FEWIN_FOLD}, 'any', None,
    KERNEL_WHY % 'him_conv.hip run_dgrad (fewin fold)')
row('NO_FEWIN_REFLECT', (2, 3, 37, 150, 64, 7, 1, 3, 'reflect', 'none'), ('fwd',), {'disable': A.ALGO_NO_FEWIN_REFLECT}, 'any', None,
    KERNEL_WHY % 'him_conv_direct.inc:601')
for c in ((2, 96, 37, 150, 3, 7, 1, 3, 'zero', 'none'), (2, 4, 20, 140, 32, 5, 1, 2, 'zero', 'none')):
    row('NO_FEWCH_MFMA %d' % c[5], c, ('bwd_weight',), {'disable': A.ALGO_NO_FEWCH_MFMA}, 'any', None,
        KERNEL_WHY % 'him_wgrad_fewch.inc:201')
for c in (TAILS, PATCH, (3, 128, 8, 10, 256, 4, 1, 2, 'zero', 'none')):
    row('GENERIC_CONV %s' % 'x'.join(map(str, c[:5])), c, ALL3, dict(NOWINO, disable=A.ALGO_GENERIC_CONV), 'any', NOWINO,
        KERNEL_WHY % 'him_conv.hip use_fast, him_conv_wgrad.inc:422')
row('GENERIC_CONV deconv', DECONV, ALL3, {'disable': A.ALGO_GENERIC_CONV}, 'any', None, KERNEL_WHY % 'him_conv.hip use_fast')
row('NO_BGEMM', wino(W512), ALL3, {'disable': A.ALGO_NO_BGEMM}, 'any', None, KERNEL_WHY % 'him_conv.hip wino_batched_gemm')
# him_resblock.inc resblock_ok is the only reader of the bit: the layerwise path (the plain conv entry points) must not move
row('NO_RESBLOCK_FUSED layerwise', wino(W128), ALL3, dict(WINO16, disable=A.ALGO_NO_RESBLOCK_FUSED), 'identical', WINO16)

EXTRA_ROWS = [{'name': 'NO_ONEHOT_RLE (test_onehot_weight_gradient_per_pixel_and_per_run)', 'over': {'disable': A.ALGO_NO_ONEHOT_RLE}}]


@pytest.mark.parametrize('r', ROWS, ids=[r['name'] for r in ROWS])
def test_selection_matrix(r):
    case = case_of(r['case'])
    equal = []
    for what in r['passes']:
        for acc in ((0, 1) if what == 'bwd_weight' else (0,)):
            base = run(case, r['base'], what, accumulate=acc)
            got = run(case, r['over'], what, accumulate=acc)
            same = all(torch.equal(base[k], got[k]) for k in base)
            equal.append(same)
            if r['rel'] == 'identical':
                assert same, '%s %s: documented as bit-identical to the base selection' % (r['name'], what)
    H.REPORT.append({'row': r['name'], 'relation': r['rel'], 'bit_equal_per_pass': equal})
    if r['rel'] == 'differs':
        assert not all(equal), '%s: bit-equal to the base selection in every pass -- the override did not reach a launch' % r['name']


# -------------------------------------------------------------------------------- the default selection, every pass
@pytest.mark.parametrize('c', CONV_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_default_selection_conv(c):
    case = case_of(c)
    run(case, {}, 'fwd')
    run(case, {}, 'fwd', bias=False)
    run(case, {}, 'bwd_data')
    for acc in (0, 1):
        run(case, {}, 'bwd_weight', accumulate=acc)
        run(case, {}, 'bwd_weight', accumulate=acc, dbias=False)
    for what in ('fwd', 'bwd_data'):
        run(case, {}, what, panel=True)
    if c[9] == 'none':
        run(case, {}, 'in_act')
        run(case, {}, 'in_act', panel=True)


@pytest.mark.parametrize('c', DECONV_CASES, ids=lambda c: 'x'.join(map(str, c)))
@pytest.mark.parametrize('act', ['none', 'relu'])
def test_default_selection_deconv(c, act):
    case = case_of(c, act)
    for panel in (False, True):
        run(case, {}, 'fwd', panel=panel)
        run(case, {}, 'bwd_data', panel=panel)
    run(case, {}, 'fwd', bias=False)
    for acc in (0, 1):
        run(case, {}, 'bwd_weight', accumulate=acc)
    run(case, {}, 'bwd_weight', accumulate=1, dbias=False)


@pytest.mark.parametrize('c', WINO_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_default_selection_winograd(c):
    """WINO_CASES under their own setting (threshold 16 channels), plain, panel and kept-input forms."""
    case = case_of(wino(c))
    big = c[1] >= 512
    for panel in (False, True):
        run(case, WINO16, 'fwd', panel=panel)
        run(case, WINO16, 'bwd_data', panel=panel)
    for acc in ((1,) if big else (0, 1)):
        run(case, WINO16, 'bwd_weight', accumulate=acc)
        run(case, WINO16, 'fwd_keep_wgrad', accumulate=acc)


@pytest.mark.parametrize('c', WINO4_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_default_selection_f4x4_frozen(c):
    case = case_of(c + (3, 1, 1, 'zero', 'none'))
    for panel in (False, True):
        run(case, FROZEN, 'fwd', panel=panel)
        run(case, FROZEN, 'bwd_data_gated', panel=panel)


@pytest.mark.parametrize('c', [CONV_CASES[2], CONV_CASES[4], FUSED, W4], ids=lambda c: 'x'.join(map(str, c)))
def test_refused_calls_write_nothing(c):
    H.negative_paths(H.raw_lib(), case_of(c), H.algo())


# --------------------------------------------------------------------------------------- him_winograd_gemm on its own
GEMM = [
    # M, K, N, tile_wb, NO_BGEMM -- him_conv.hip launch_gconv with maxN = 16 * N, tiles128 = 16 * N/128 * ceil(M/128)
    (128, 32, 128, 0, 0), (136, 48, 256, 0, 0),                  # default tile, M tail
    (128, 16, 8192, A.TILE_128x256, 1),                          # 128x256 eligible: N % 256 == 0, tiles256 = 512
    (128, 32, 256, A.TILE_128x256, 1), (128, 32, 384, A.TILE_128x256, 1),   # not eligible: tiles256 = 16; N % 256 != 0
    (128, 32, 128, A.TILE_MIXED, 1),                             # tiles128 = 16: 128x64
    (128, 32, 1664, A.TILE_MIXED, 1),                            # 208: inside 200..256 -> 128x128
    (128, 32, 2560, A.TILE_MIXED, 1),                            # 320: between the thresholds -> 128x64
    (256, 32, 2048, A.TILE_MIXED, 1),                            # 512: 128x128
    (1024, 1024, 1024, 0, 0), (1024, 1024, 1024, A.TILE_128x128, 1),   # the LDS-DMA GEMM / the conv kernel at benchmark size
]


@pytest.mark.parametrize('g', GEMM, ids=str)
def test_winograd_gemm_against_float64(g):
    M, K, N, tile, nobg = g
    H.run_wino_gemm(H.raw_lib(), M, K, N, H.algo(tile_wb=tile, disable=A.ALGO_NO_BGEMM if nobg else 0))


@pytest.mark.parametrize('g', [(128, 24, 128), (128, 32, 192), (128, 8, 128), (4, 32, 128)], ids=str)
def test_winograd_gemm_refuses_shapes_outside_its_contract(g):
    H.run_wino_gemm(H.raw_lib(), g[0], g[1], g[2], H.algo(), expect_error=True)


# ---------------------------------------------------------------------------------------------------- other readers
def test_resblock_fused_switch():
    lib = H.raw_lib()
    d = A.HimResBlock(2, 640, 8, 12, 1e-5, H.algo())
    assert lib.him_resblock_supported(ctypes.byref(d)) == 1
    d.algo.disable = A.ALGO_NO_RESBLOCK_FUSED
    assert lib.him_resblock_supported(ctypes.byref(d)) == 0 and lib.him_resblock_ws(ctypes.byref(d)) == 0


def onehot_both_forms(c, over):
    """The one-hot weight gradient (and forward) of case `c` under HimAlgo `over`, per run and per pixel (NO_ONEHOT_RLE), both
    accumulate modes, in guarded arenas of exactly the reported size against float64; returns dw per (bit, accumulate)."""
    lib = H.raw_lib()
    B, NC, Cd, Hh, W, Cout, k, pm = c
    g = torch.Generator().manual_seed(11)
    coarse = torch.randint(0, NC, (B, 1, (Hh + 3) // 4, (W + 3) // 4), generator=g)
    label = coarse.repeat_interleave(4, 2).repeat_interleave(4, 3)[:, :, :Hh, :W].clone()
    label[:, :, 1::5, 2::7] = torch.randint(0, NC, label[:, :, 1::5, 2::7].shape, generator=g)
    onehot = torch.zeros(B, NC, Hh, W).scatter_(1, label, 1.0)
    case = H.ConvCase((B, NC + Cd, Hh, W, Cout, k, 1, k // 2, pm, 'none'))
    case.x = torch.cat([onehot, case.x[:, NC:]], 1)
    case.w = H.rand(Cout, NC + Cd, k, k, seed=2, scale=0.05)
    got = {}
    for bit in (0, A.ALGO_NO_ONEHOT_RLE):
        a = H.algo(**dict(over, disable=bit))
        d = case.desc(a)
        row_ = '%s|%s|onehot' % (case.tag(), H.algo_tag(a))
        nws = int(lib.him_conv2d_onehot_bwd_weight_ws(ctypes.byref(d), NC))
        assert nws > 0
        for acc in (0, 1):
            specs = {'label': ('in', label.float()), 'x': ('in', case.x), 'dy': ('in', case.dy),
                     'dw': ('out', tuple(case.w.shape), H.rand(*case.w.shape, seed=7) if acc else None),
                     'dbias': ('out', (Cout,), H.rand(Cout, seed=8) if acc else None), 'ws': ('ws', nws)}
            ar = H.Arena('cuda', specs)
            rc = lib.him_conv2d_onehot_bwd_weight(ctypes.byref(d), ar.ptr('label'), NC, ar.ptr('x'), ar.ptr('dy'), ar.ptr('dw'),
                                                  ar.ptr('dbias'), acc, ar.ptr('ws'), nws, torch.cuda.current_stream().cuda_stream)
            H._finish(lib, row_, rc, ar, 'cuda')
            add = specs['dw'][2] if acc else 0
            dw = ar.t['dw'].cpu()
            H.check_tensor(row_ + ('+acc' if acc else ''), 'dw', 'weight', dw, case.ref(torch.float64, 'dw') + (add.double() if acc else 0),
                           case.ref(torch.float32, 'dw') + add, H.DIRECT)
            got[(bit, acc)] = dw
        nws = int(lib.him_conv2d_onehot_fwd_ws(ctypes.byref(d), NC))
        specs = {'label': ('in', label.float()), 'x': ('in', case.x), 'w': ('in', case.w), 'bias': ('in', case.b),
                 'y': ('out', (B, Cout, case.OH, case.OW), None), 'ws': ('ws', nws)}
        ar = H.Arena('cuda', specs)
        rc = lib.him_conv2d_onehot_fwd(ctypes.byref(d), ar.ptr('label'), NC, ar.ptr('x'), ar.ptr('w'), ar.ptr('bias'), ar.ptr('y'),
                                       ar.ptr('ws'), nws, torch.cuda.current_stream().cuda_stream)
        H._finish(lib, row_ + ' fwd', rc, ar, 'cuda')
        H.check_tensor(row_ + ' fwd', 'y', 'plane', ar.t['y'].cpu(), case.ref(torch.float64, 'y'), case.ref(torch.float32, 'y'), H.DIRECT)
    return got


@pytest.mark.parametrize('c', ONEHOT_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_onehot_weight_gradient_per_pixel_and_per_run(c):
    """him_conv_onehot.inc:263: NO_ONEHOT_RLE selects the per-pixel weight gradient; both forms, both accumulate modes, in
    guarded arenas against the float64 dense convolution on the materialised one-hot tensor."""
    got = onehot_both_forms(c, {})
    assert not torch.equal(got[(0, 0)], got[(A.ALGO_NO_ONEHOT_RLE, 0)]), 'NO_ONEHOT_RLE did not reach the launch'


@pytest.mark.parametrize('pm', ['reflect', 'zero'])
def test_onehot_dense_slice_with_the_winograd_shape(pm):
    """him_conv.hip plan_wgrad(allow_wino = false): a 3x3 "same" stem whose dense slice (128 -> 128 channels, threshold 16) has
    the F(2x2) weight-gradient shape.  The one-hot workspace reserves no Winograd transforms; before the plan run_wgrad chose
    Winograd all the same and the call ended in HIM_E_WORKSPACE with the label-id slice of dw already written."""
    onehot_both_forms((1, 3, 128, 8, 8, 128, 3, pm), WINO16)


def test_tiny_5x5_weight_gradient_fits_its_reported_workspace():
    """him_conv.hip plan_wgrad: Cout <= 4 with a 5x5 kernel off the "same" geometry runs the generic kernel, whose splits
    (268 here: 67 600 positions / 256) are capped at the 256 slabs its class reserves; uncapped, the call was refused."""
    case = case_of((1, 1, 520, 520, 1, 5, 2, 2, 'zero', 'none'))
    for acc in (0, 1):
        run(case, {}, 'bwd_weight', accumulate=acc)
