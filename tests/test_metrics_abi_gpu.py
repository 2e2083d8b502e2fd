"""-m gpu: him_image_metrics and him_confusion at the C ABI inside tests/abi_harness.py's guarded arena, against the
float64 restatement of tests/metrics_fixture.py.

Arena: every buffer of a call is a view in ONE allocation between 64 KiB bands; NaN bands beside the images and the box,
0xA5 bands beside sums, map, counts, status and workspace, compared bit for bit afterwards; outputs and workspace are
pre-filled with NaN bytes; the workspace is exactly the queried size.

Bound of the image metrics (tests/README.md, direct form): per map element and per ``sums`` entry, error <=
max(8 * e32, 16 * 2^-24) in the metric maximum error over maximum |ref|, e32 = the same metric of the fixture evaluated
naively in fp32 against float64 on the same case; no element is excluded.  One JSON line per checked tensor goes to
metrics_abi_rows.jsonl in the GPU tests' report directory.  The confusion matrix is integer: equality.

Shapes are worded in the kernel's tile of 16 x 64 window origins (include/him.h)."""
import json
import os

import numpy as np
import pytest
import torch

import abi_harness as ah
import metrics_fixture as fx
from test_model_gpu import OUT as REPORT_DIR

pytestmark = pytest.mark.gpu

OUT = os.path.join(REPORT_DIR, 'metrics_abi_rows.jsonl')       # next to the model tests' trajectory reports
TH, TW = 16, 64
FACTOR, FLOOR = 8.0, 16 * 2.0 ** -24
ROWS = []


@pytest.fixture(autouse=True)
def _dump():
    yield
    if ROWS:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        with open(OUT, 'a') as f:
            for r in ROWS:
                f.write(json.dumps(r) + '\n')
        del ROWS[:]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    """Any 4-byte-element array as the float32 tensor holding the same bits (the arena's 'in' kind)."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.float32).copy())


# ---------------------------------------------------------------------------------------------------- image metrics
def call_image(a, b, scale, offset, quantize, L, box=None, want_map=False, shift=0):
    """One guarded him_image_metrics call; returns (sums (B,C,5) float64 numpy, map or None).  ``shift``: both image
    bases are moved that many floats off their 256-byte aligned start (a NaN sits in front)."""
    lib = ah.raw_lib()
    B, C, H, W = a.shape
    need = int(lib.him_image_metrics_workspace(B, C, H, W))
    assert need > 0
    pad = np.full(shift, np.nan, np.float32)
    specs = {'a': ('in', torch.from_numpy(np.concatenate([pad, a.reshape(-1)]))),
             'b': ('in', torch.from_numpy(np.concatenate([pad, b.reshape(-1)])))}
    if box is not None:
        specs['box'] = ('in', _bits(np.asarray(box, np.int32)))
    specs['sums'] = ('ws', B * C * 5 * 8)
    if want_map:
        specs['map'] = ('out', (B, C, H - 10, W - 10), None)
    specs['ws'] = ('ws', need)
    ar = ah.Arena('cuda', specs)
    rc = lib.him_image_metrics(ar.ptr('a') + 4 * shift, ar.ptr('b') + 4 * shift, B, C, H, W, scale, offset,
                               1 if quantize else 0, L, ar.ptr('box'), ar.ptr('sums'), ar.ptr('map'), ar.ptr('ws'), need,
                               _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.him_last_error()
    bad = ar.guard_failures()
    assert not bad, '; '.join(bad)
    assert torch.equal(ar.t['a'][shift:].cpu(), torch.from_numpy(a.reshape(-1)))           # inputs are never written
    sums = ar.t['sums'].cpu().numpy().view(np.float64).reshape(B, C, 5).copy()
    assert np.isfinite(sums).all(), sums
    smap = ar.t['map'].cpu().numpy().copy() if want_map else None
    return sums, smap


def make_pair(kind, seed, B, C, H, W):
    """(a, b, scale, offset, L): values as the call takes them.  'noise': uniform [0, 255); 'flat': a bright flat field
    plus noise of amplitude 1/255 (the cancellation case of E[x^2] - mu^2), L = 1; 'step': a vertical step edge, the
    second image shifted by one pixel; 'gen': generator-range values in [-1, 1] for the byte preset."""
    g = np.random.default_rng(seed)
    u = lambda: g.random((B, C, H, W), dtype=np.float32)              # noqa: E731
    if kind == 'noise':
        a = u() * np.float32(255)
        return a, (a + (u() - np.float32(0.5)) * np.float32(60)).astype(np.float32), 1.0, 0.0, 255.0
    if kind == 'flat':
        return (np.float32(0.97) + u() / np.float32(255)).astype(np.float32), \
            (np.float32(0.97) + u() / np.float32(255)).astype(np.float32), 1.0, 0.0, 1.0
    if kind == 'step':
        x = np.arange(W)[None, None, None, :]
        a = np.where(x < W // 2, 0.1, 0.9).astype(np.float32) * np.ones((B, C, H, 1), np.float32)
        b = np.where(x < W // 2 + 1, 0.1, 0.9).astype(np.float32) * np.ones((B, C, H, 1), np.float32)
        return (a * 255 + u()).astype(np.float32), (b * 255 + u()).astype(np.float32), 1.0, 0.0, 255.0
    a = u() * np.float32(2.2) - np.float32(1.1)                       # a few values clip
    return a, (a + (u() - np.float32(0.5)) * np.float32(0.4)).astype(np.float32), 127.5, 127.5, 255.0


def check(case, got_sums, got_map, a, b, scale, offset, quantize, L, box=None):
    """Every map element and every ``sums`` entry against float64 under max(8 * e32, 16 * 2^-24); rows are reported
    before anything is asserted."""
    s64, m64 = fx.image_sums(a, b, scale, offset, quantize, L, box)
    s32, m32 = fx.image_sums(a, b, scale, offset, quantize, L, box, dtype=np.float32)
    checks = []
    if got_map is not None:
        ref = np.stack(m64).reshape(got_map.shape)
        checks.append(('map', got_map, ref, np.stack(m32).reshape(got_map.shape)))
    for k, name in enumerate(('ssim_sum', 'ssim_windows', 'sq_err_sum', 'abs_err_sum', 'pixels')):
        checks.append((name, got_sums[:, :, k], s64[:, :, k], s32[:, :, k]))
    failed = []
    for name, got, ref, ref32 in checks:
        err, e32 = fx.rel_err(got, ref), fx.rel_err(ref32, ref)
        limit = max(FACTOR * e32, FLOOR)
        ROWS.append(dict(case=case, tensor=name, error=err, e32=e32, ratio=(err / e32 if e32 > 0 else None), limit=limit))
        print('%s %s: error %.3e e32 %.3e limit %.3e' % (case, name, err, e32, limit))
        if not err <= limit:
            failed.append('%s %s: error %.3e > limit %.3e (e32 %.3e)' % (case, name, err, limit, e32))
    assert np.array_equal(got_sums[:, :, 1], s64[:, :, 1]) and np.array_equal(got_sums[:, :, 4], s64[:, :, 4]), case
    assert not failed, '; '.join(failed)


SHAPES = [(1, 1, 11, 11), (1, 1, 11, 40), (1, 1, 40, 11), (1, 1, 12, 27),
          (1, 1, TH + 10 + 1, TW + 10 + 1),                 # one tile plus one window origin in each direction
          (2, 3, 2 * TH + 10 + 5, 2 * TW + 10 + 7),         # two tiles plus a ragged edge in both directions
          (1, 1, TH + 10, TW + 10)]                         # exactly one tile


@pytest.mark.parametrize('kind', ['noise', 'flat', 'step', 'gen'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_whole_image_map_and_sums_against_float64(shape, kind):
    B, C, H, W = shape
    a, b, scale, offset, L = make_pair(kind, 11 + H + W, B, C, H, W)
    for quantize in ((True,) if kind == 'gen' else (False, True) if kind in ('noise', 'step') else (False,)):
        case = '%s|%s|q%d' % ('x'.join(map(str, shape)), kind, quantize)
        sums, smap = call_image(a, b, scale, offset, quantize, L, want_map=True)
        check(case, sums, smap, a, b, scale, offset, quantize, L)
        if kind == 'flat':
            # the per-tile pivot: on the cancellation case the map is at least ten times closer to float64 than the naive
            # fp32 formula (a figure of the numbers' formats, not of this kernel: differences to the pivot are below
            # 1/255, so their squares carry 2^-24 * 1.5e-5 where the naive E[x^2] carries 2^-24 * 0.95)
            row = [r for r in ROWS if r['case'] == case and r['tensor'] == 'map'][-1]
            assert row['error'] <= row['e32'] / 10, row
        plain, none = call_image(a, b, scale, offset, quantize, L, want_map=False)
        assert none is None and plain.tobytes() == sums.tobytes(), case          # the map does not change the sums
        again, _ = call_image(a, b, scale, offset, quantize, L, want_map=True)
        assert torch.equal(torch.from_numpy(again), torch.from_numpy(sums)), case       # two calls: identical bits


@pytest.mark.parametrize('shape', [(1, 1, 12, 27), (2, 3, 2 * TH + 15, 2 * TW + 17)], ids=lambda s: 'x'.join(map(str, s)))
def test_base_shifted_by_four_bytes(shape):
    a, b, scale, offset, L = make_pair('noise', 5, *shape)
    sums, smap = call_image(a, b, scale, offset, False, L, want_map=True, shift=1)
    check('%s|noise|shift4' % 'x'.join(map(str, shape)), sums, smap, a, b, scale, offset, False, L)
    aligned, amap = call_image(a, b, scale, offset, False, L, want_map=True)
    assert aligned.tobytes() == sums.tobytes() and amap.tobytes() == smap.tobytes()


BOXES = {'interior': (20, 9, 100, 40), 'left_top': (0, 0, 30, 20), 'right_bottom': (60, 20, 144, 46),
         'top_right': (100, 0, 144, 15), 'bottom_left': (0, 30, 40, 46), 'eleven_wide': (33, 5, 43, 40),
         'eleven_high': (10, 7, 90, 17), 'ten_wide': (50, 3, 59, 44), 'ten_high': (3, 20, 120, 29),
         'partly_outside': (-7, -3, 50, 30), 'past_the_far_edges': (90, 25, 400, 300), 'empty': (30, 30, 29, 40),
         'outside': (200, 5, 260, 40), 'one_pixel': (70, 21, 70, 21), 'whole': (0, 0, 144, 46)}


@pytest.mark.parametrize('name', list(BOXES))
@pytest.mark.parametrize('quantize', [False, True])
def test_box_equals_the_fixture_on_the_cropped_image(name, quantize):
    B, C, H, W = 2, 3, 47, 145
    a, b, scale, offset, L = make_pair('gen' if quantize else 'noise', 21, B, C, H, W)
    other = BOXES['interior'] if name != 'interior' else BOXES['left_top']
    box = np.array([BOXES[name], other], np.int32)                    # a different box per batch item
    sums, _ = call_image(a, b, scale, offset, quantize, L, box=box)
    check('box_%s|q%d' % (name, quantize), sums, None, a, b, scale, offset, quantize, L, box)
    # the same numbers as the whole-image call on the numpy-cropped images
    x0, y0, w, h = fx.clip_box(BOXES[name], H, W)
    if w > 0 and h > 0:
        ca, cb = np.ascontiguousarray(a[:1, :, y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(b[:1, :, y0:y0 + h, x0:x0 + w])
        crop, _ = fx.image_sums(ca, cb, scale, offset, quantize, L)
        assert np.array_equal(sums[0, :, 1], crop[0, :, 1]) and np.array_equal(sums[0, :, 4], crop[0, :, 4])
        if min(w, h) >= 11:
            whole, _ = call_image(ca, cb, scale, offset, quantize, L)
            assert np.array_equal(whole[0, :, 1:], sums[0, :, 1:]), name          # integer counts and error sums
            assert np.allclose(whole[0, :, 0], sums[0, :, 0], rtol=max(FACTOR * 1e-6, FLOOR), atol=0)
    else:
        assert not sums[0].any()
    if name in ('ten_wide', 'ten_high', 'one_pixel'):
        assert (sums[0, :, 1] == 0).all() and (sums[0, :, 0] == 0).all() and (sums[0, :, 2] > 0).all()
        assert (sums[0, :, 4] == w * h).all()
    if name in ('eleven_wide', 'eleven_high'):
        assert (sums[0, :, 1] == max(w - 10, 0) * max(h - 10, 0)).all() and (sums[0, :, 1] > 0).all()


@pytest.mark.parametrize('shape', [(1, 1, 11, 11), (2, 3, 2 * TH + 15, 2 * TW + 17)], ids=lambda s: 'x'.join(map(str, s)))
def test_identical_inputs_give_one_within_four_ulp(shape):
    for kind, quantize in (('noise', False), ('flat', False), ('gen', True)):
        a, _, scale, offset, L = make_pair(kind, 31, *shape)
        sums, smap = call_image(a, a.copy(), scale, offset, quantize, L, want_map=True)
        assert np.abs(smap.astype(np.float64) - 1.0).max() <= 4 * 2.0 ** -23, (kind, np.abs(smap - 1).max())
        assert (sums[:, :, 2] == 0).all() and (sums[:, :, 3] == 0).all()
        assert np.abs(sums[:, :, 0] / sums[:, :, 1] - 1).max() <= 4 * 2.0 ** -23


def test_byte_preset_equals_the_fixture_on_tensor2im_bytes():
    """scale = offset = 127.5 with quantize: the values compared are the bytes him_tensor2im_bytes(normalize=1) writes."""
    lib = ah.raw_lib()
    C, H, W = 3, 37, 91
    a, b, scale, offset, L = make_pair('gen', 41, 1, C, H, W)
    planes = []
    for img in (a, b):
        src = torch.from_numpy(img[0]).cuda()
        dst = torch.empty((H, W, 3), dtype=torch.uint8, device='cuda')
        assert lib.him_tensor2im_bytes(src.data_ptr(), C, H, W, 1, dst.data_ptr(), _stream()) == 0
        planes.append(dst.cpu().numpy().transpose(2, 0, 1)[None].astype(np.float32))
    assert np.array_equal(planes[0], fx.map_values(a, 127.5, 127.5, True))            # the fixture's preset = the bytes
    sums, smap = call_image(a, b, scale, offset, True, L, want_map=True)
    check('byte_preset', sums, smap, planes[0], planes[1], 1.0, 0.0, False, L)
    # a scale next to the preset's takes the plain order x * scale + offset, as the fixture's plain mapping does
    near = float(np.nextafter(np.float32(127.5), np.float32(128)))
    plain, pmap = call_image(a, b, near, 127.5, True, L, want_map=True)
    check('beside_the_preset', plain, pmap, a, b, near, 127.5, True, L)


# ------------------------------------------------------------------------------------------------- confusion matrix
NP_OF = {0: np.uint8, 1: np.int32, 2: np.int64, 3: np.float32}


def make_labels(g, kind, B, H, W, n, dirty):
    """ids of kind 0..3: uniform in [0, n) and, with ``dirty``, a few negative / >= n / non-integral values."""
    ids = g.integers(0, n, size=(B, 1, H, W)).astype(np.int64)
    out = ids.astype(NP_OF[kind])
    if dirty and out.size >= 8:
        flat = out.reshape(-1)
        where = g.choice(flat.size, size=max(flat.size // 8, 3), replace=False)
        for j, i in enumerate(where):
            pick = j % 3
            if pick == 0 and n < 256:
                flat[i] = n if kind == 0 else n + 7
            elif pick == 1 and kind != 0:
                flat[i] = -1
            elif pick == 2 and kind == 3:
                flat[i] = flat[i] + np.float32(0.5)
            elif kind == 2:
                flat[i] = (1 << 40) + 3                      # an int64 whose low 32 bits are a valid id
    return out


def make_pred(g, kind, B, H, W, n, dirty):
    if kind <= 3:
        return make_labels(g, kind, B, H, W, n, dirty), 1
    if kind == 4:
        C = min(n + 1, 9)                                    # n = 2: channel 2 is a label outside [0, n)
        return (g.integers(0, 4, size=(B, C, H, W)).astype(np.float32) * np.float32(0.25)), C      # exact ties abound
    vals = np.array([0.2, 0.5, 0.8, np.nextafter(np.float32(0.5), np.float32(1))], np.float32)     # 0.5 itself is 0
    return vals[g.integers(0, 4, size=(B, 1, H, W))], 1


def call_conf(pred, pk, C, gt, gk, n, mask=None, ignore=-1, per_sample=False, accumulate=False, shift=0, before=None):
    """One guarded him_confusion call; returns (counts, status[0], status[1]).  ``shift``: every plane's base is moved
    that many ELEMENTS off its aligned start; ``before``: (counts, status) the outputs hold when the call starts."""
    lib = ah.raw_lib()
    B, _, H, W = gt.shape
    need = int(lib.him_confusion_workspace(n))
    planes = {'pred': pred, 'gt': gt}
    if mask is not None:
        planes['mask'] = mask
    rows = B if per_sample else 1
    specs = {k: ('ws', v.nbytes + shift * v.itemsize) for k, v in planes.items()}
    specs.update(counts=('ws', rows * n * n * 8), status=('ws', 8), ws=('ws', need))
    ar = ah.Arena('cuda', specs)
    off = {}
    for k, v in planes.items():
        off[k] = shift * v.itemsize
        ar.t[k][off[k]:off[k] + v.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8)))
    if before is not None:
        ar.t['counts'].copy_(torch.from_numpy(before[0].reshape(-1).view(np.uint8)))
        ar.t['status'].copy_(torch.from_numpy(np.asarray(before[1], np.int32).view(np.uint8)))
    rc = lib.him_confusion(ar.ptr('pred') + off['pred'], pk, ar.ptr('gt') + off['gt'], gk,
                           ar.ptr('mask') + off['mask'] if mask is not None else 0, B, C, H, W, n, ignore,
                           1 if per_sample else 0, 1 if accumulate else 0, ar.ptr('counts'), ar.ptr('status'), ar.ptr('ws'),
                           need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.him_last_error()
    bad = ar.guard_failures()
    assert not bad, '; '.join(bad)
    for k, v in planes.items():
        assert bytes(ar.t[k][off[k]:off[k] + v.nbytes].cpu().numpy()) == v.tobytes(), k
    counts = ar.t['counts'].cpu().numpy().view(np.int64).reshape(rows, n, n).copy()
    status = ar.t['status'].cpu().numpy().view(np.int32)
    return counts, int(status[0]), int(status[1])


# widths 1, 7, 13, 257: the element path; 8 and 256 with an aligned base: four pixels per lane (the path of every real
# label plane); 8 and 256 with the base shifted by one element: the width allows the vector path, the base does not
CONF_SHAPES = [(1, 1, 0), (3, 7, 0), (3, 13, 1), (64, 257, 0), (4, 8, 0), (4, 8, 1), (64, 256, 0), (64, 256, 1)]


@pytest.mark.parametrize('n', [2, 35, 151, 256])
@pytest.mark.parametrize('shape', CONF_SHAPES, ids=lambda s: '%dx%d%s' % (s[0], s[1], '+shift' if s[2] else ''))
def test_confusion_equals_the_fixture_for_every_kind(shape, n):
    H, W, shift = shape
    B = 2
    g = np.random.default_rng(100 * H + n)
    mask = (g.random((B, 1, H, W)) < 0.7).astype(np.float32)
    big = H * W > 1000
    seen = 0
    for pk in range(6):
        for gk in range(4):
            if big and W % 4 and (pk + gk) % 2:              # at 64 x 257 every kind still occurs on both sides
                continue
            pred, C = make_pred(g, pk, B, H, W, n, dirty=True)
            gt = make_labels(g, gk, B, H, W, n, dirty=True)
            for use_mask, ignore, per_sample in ((False, -1, False), (True, n // 2, True)):
                m = mask if use_mask else None
                want, skipped = fx.confusion(pred, pk, gt, gk, n, m, ignore, per_sample)
                got, s0, s1 = call_conf(pred, pk, C, gt, gk, n, m, ignore, per_sample, shift=shift)
                assert got.dtype == want.dtype and np.array_equal(got, want), (pk, gk, use_mask)
                assert s0 == skipped and s1 == (1 if skipped else 0), (pk, gk, s0, skipped, s1)
                seen += 1
    assert seen >= 24


def test_ties_thresholds_and_the_ignore_label_beyond_n():
    n = 4
    scores = np.zeros((1, 4, 2, 3), np.float32)
    scores[0, :, 0, 0] = [1, 1, 0, 0]          # tie 0 / 1 -> 0
    scores[0, :, 0, 1] = [0, 2, 2, 2]          # tie 1 / 2 / 3 -> 1
    scores[0, :, 0, 2] = [-1, -1, -1, -1]      # all equal -> 0
    scores[0, :, 1, 0] = [0, 0, 0, 5]
    scores[0, :, 1, 1] = [0, 3, 0, 3]          # -> 1
    scores[0, :, 1, 2] = [2, 0, 2, 0]          # -> 0
    gt = np.array([[[[0, 1, 2], [3, 3, 255]]]], np.uint8)
    got, s0, _ = call_conf(scores, 4, 4, gt, 0, n, ignore=255)
    want = np.zeros((1, 4, 4), np.int64)
    for r, c in ((0, 0), (1, 1), (2, 0), (3, 3), (3, 1)):
        want[0, r, c] += 1
    assert np.array_equal(got, want) and s0 == 0             # 255 is the ignore label: left out, not "skipped"
    got, s0, s1 = call_conf(scores, 4, 4, gt, 0, n)
    assert np.array_equal(got, want) and s0 == 1 and s1 == 1       # without it the pixel is out of range
    half = np.nextafter(np.float32(0.5), np.float32(1))
    prob = np.array([[[[0.5, half, 0.0, 1.0, 0.49999997, np.float32(0.5)]]]], np.float32)
    gt1 = np.ones((1, 1, 1, 6), np.int32)
    got, s0, _ = call_conf(prob, 5, 1, gt1, 1, 2, per_sample=True)
    assert np.array_equal(got, np.array([[[0, 0], [4, 2]]])) and s0 == 0
    assert np.array_equal(got, fx.confusion(prob, 5, gt1, 1, 2, per_sample=True)[0])


def test_per_sample_sums_to_the_pooled_form_and_accumulate_doubles():
    B, H, W, n = 3, 64, 257, 35
    g = np.random.default_rng(9)
    pred, gt = make_labels(g, 2, B, H, W, n, True), make_labels(g, 3, B, H, W, n, True)
    pooled, sp, _ = call_conf(pred, 2, 1, gt, 3, n)
    per, ss, _ = call_conf(pred, 2, 1, gt, 3, n, per_sample=True)
    assert per.shape == (B, n, n) and np.array_equal(per.sum(0, keepdims=True), pooled) and sp == ss > 0
    assert np.array_equal(pooled, fx.confusion(pred, 2, gt, 3, n)[0])
    for n2 in (35, 256):                                     # the LDS-private and the direct path
        first, s0, f0 = call_conf(pred, 2, 1, gt, 3, n2)
        twice, s1, f1 = call_conf(pred, 2, 1, gt, 3, n2, accumulate=True, before=(first, [s0, f0]))
        assert np.array_equal(twice, 2 * first) and s1 == 2 * s0 and f1 == f0
        zero = (np.zeros_like(first), [0, 0])
        once, s2, _ = call_conf(pred, 2, 1, gt, 3, n2, accumulate=True, before=zero)
        assert np.array_equal(once, first) and s2 == s0
    huge = (np.zeros((1, n, n), np.int64), [2 ** 31 - 2, 0])
    _, s3, f3 = call_conf(pred, 2, 1, gt, 3, n, accumulate=True, before=huge)
    assert s3 == 2 ** 31 - 1 and f3 == 3                      # the skipped count saturates and says so


@pytest.mark.parametrize('n', [35, 151, 256])
def test_all_pixels_in_one_cell_and_two_runs_are_identical(n):
    B, H, W = 2, 64, 257
    gt = np.full((B, 1, H, W), n - 1, np.uint8 if n <= 255 else np.int32)
    gk = 0 if n <= 255 else 1
    pred = np.full((B, 1, H, W), n - 2, np.float32)
    got, s0, _ = call_conf(pred, 3, 1, gt, gk, n)
    want = np.zeros((1, n, n), np.int64)
    want[0, n - 1, n - 2] = B * H * W
    assert np.array_equal(got, want) and s0 == 0
    g = np.random.default_rng(n)
    p2, C = make_pred(g, 4, B, H, W, n, True)
    g2 = make_labels(g, 2, B, H, W, n, True)
    runs = [call_conf(p2, 4, C, g2, 2, n, per_sample=True) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1:] == runs[1][1:]
    assert np.array_equal(runs[0][0], fx.confusion(p2, 4, g2, 2, n, per_sample=True)[0])
