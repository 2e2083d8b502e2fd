"""-m gpu: him_panoptic_match at the C ABI inside tests/abi_harness.py's guarded arena, against the numpy restatement of
tests/panoptic_fixture.py.

Arena: every buffer of a call is a view in ONE allocation between 64 KiB bands; NaN bands beside the five input planes,
0xA5 bands beside counts, iou_sum, matches, status and the workspace, compared bit for bit afterwards; fresh outputs and
the workspace are pre-filled with 0xFF bytes; the workspace is exactly the queried size; the inputs are compared byte for
byte with what went in.

Comparison: EQUALITY for counts, status and the matches rows; iou_sum within tp * 2^-52 relative of the fixture's sum
(the worst case of any order of adding tp float64 terms in (0.5, 1]).  Every overwriting call is made twice on the same
arena and the two sets of outputs must be bitwise equal.

Shapes are worded in the kernel's constants (csrc/him_panoptic.hip): a lane reads PX = 4 pixels per step, as one vector
load where every base is 16-byte aligned and W % PX == 0; a workgroup walks STEP = 1024 pixels per step and owns a share
of at least SHARE_MIN = 2048 pixels."""
import itertools

import numpy as np
import pytest
import torch

import abi_harness as ah
import ccl_fixture as cf
import panoptic_fixture as fx

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _as_floats(raw):
    raw = raw + b'\xff' * (-len(raw) % 4)
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy().view(np.float32))


def _plane_spec(src, shift):
    raw = b'\xff' * (shift * src.itemsize) + np.ascontiguousarray(src).tobytes()
    return ('in', _as_floats(raw)), shift * src.itemsize, raw


def _same_bytes(view, raw):
    return bytes(view.contiguous().view(torch.uint8).cpu().numpy()[:len(raw)]) == raw


def _put(view, array):
    view.copy_(torch.from_numpy(np.frombuffer(np.ascontiguousarray(array).tobytes(), np.uint8).copy()))


def call_match(planes, n_class, kinds=(1, 1, 1, 1), mask=None, ignore=-1, max_segments=1024, want_matches=True, shift=0,
               into=None):
    """One guarded him_panoptic_match call (two, compared bit for bit, when it overwrites) on (pred_seg, pred_cls, gt_seg,
    gt_cls), each (B,H,W); ``into`` = (counts, iou_sum, status) to accumulate into.  Returns (counts, iou_sum, status,
    matches or None) as numpy arrays."""
    lib = ah.raw_lib()
    np_of = (fx.SEG_NP[kinds[0]], fx.CLS_NP[kinds[1]], fx.SEG_NP[kinds[2]], fx.CLS_NP[kinds[3]])
    arrays = [np.ascontiguousarray(np.asarray(a).astype(t)) for a, t in zip(planes, np_of)]
    B, H, W = arrays[0].shape
    M = max_segments
    need = int(lib.him_panoptic_match_workspace(B, M))
    assert need > 0 and need % 16 == 0
    names = ('pred_seg', 'pred_cls', 'gt_seg', 'gt_cls')
    specs, offs, raws = {}, {}, {}
    for name, a in zip(names, arrays):
        specs[name], offs[name], raws[name] = _plane_spec(a, shift)
    if mask is not None:
        specs['mask'], offs['mask'], raws['mask'] = _plane_spec(np.ascontiguousarray(mask, np.float32), shift)
    specs.update(counts=('ws', n_class * 24), iou_sum=('ws', n_class * 8), status=('ws', B * 16))
    if want_matches:
        specs['matches'] = ('ws', B * M * 24)
    specs['ws'] = ('ws', need)
    ar = ah.Arena('cuda', specs)
    if into is not None:
        _put(ar.t['counts'], into[0].astype(np.int64))
        _put(ar.t['iou_sum'], into[1].astype(np.float64))
        _put(ar.t['status'], into[2].astype(np.int32))
    outs = []
    for _ in range(1 if into is not None else 2):
        rc = lib.him_panoptic_match(
            ar.ptr('pred_seg') + offs['pred_seg'], kinds[0], ar.ptr('pred_cls') + offs['pred_cls'], kinds[1],
            ar.ptr('gt_seg') + offs['gt_seg'], kinds[2], ar.ptr('gt_cls') + offs['gt_cls'], kinds[3],
            ar.ptr('mask') + offs['mask'] if mask is not None else 0, B, H, W, n_class, ignore, M,
            0 if into is None else 1, ar.ptr('counts'), ar.ptr('iou_sum'), ar.ptr('matches'), ar.ptr('status'),
            ar.ptr('ws'), need, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.him_last_error()
        bad = ar.guard_failures()
        assert not bad, '; '.join(bad)
        for name in raws:
            assert _same_bytes(ar.t[name], raws[name]), name + ' was written'
        outs.append({k: bytes(ar.t[k].cpu().numpy()) for k in ('counts', 'iou_sum', 'status', 'matches') if k in ar.t})
    if len(outs) == 2:
        assert outs[0] == outs[1], 'two consecutive calls differ'
    o = outs[-1]
    matches = np.frombuffer(o['matches'], np.int32).reshape(B, M, 6).copy() if want_matches else None
    return (np.frombuffer(o['counts'], np.int64).reshape(n_class, 3).copy(), np.frombuffer(o['iou_sum'], np.float64).copy(),
            np.frombuffer(o['status'], np.int32).reshape(B, 4).copy(), matches)


def assert_equal(got, ref, what):
    counts, iou, status, matches = got
    r_counts, r_iou, r_status, r_rows = ref
    assert np.array_equal(status, r_status), (what, status.tolist(), r_status.tolist())
    assert np.array_equal(counts, r_counts), (what, counts.tolist(), r_counts.tolist())
    for c in range(len(iou)):
        print('%s: class %d tp %d iou_sum %.17g reference %.17g' % (what, c, r_counts[c, 0], iou[c], r_iou[c]))
        assert abs(iou[c] - r_iou[c]) <= max(int(r_counts[c, 0]), 1) * EPS * abs(r_iou[c]), (what, c, iou[c], r_iou[c])
    if matches is not None:
        for b, rows in enumerate(r_rows):
            if rows is None:
                continue
            n = len(rows)
            assert np.array_equal(matches[b, :n], rows), (what, b)
            assert (matches[b, n:] == -1).all(), (what, b, 'rows behind the segment count were written')


def check(planes, n_class, what, **kw):
    ref_kw = {k: kw[k] for k in ('mask', 'ignore', 'max_segments') if k in kw}
    got = call_match(planes, n_class, **kw)
    assert_equal(got, fx.match_reference(*planes, n_class, **ref_kw), what)
    return got


def _batch(*planes):
    return tuple(np.asarray(a)[None] for a in planes)


PERTURBED = {}


def perturbed(H=97, W=193):
    if (H, W) not in PERTURBED:
        PERTURBED[(H, W)] = fx.perturbed_layouts(3, H, W)
    return PERTURBED[(H, W)]


def test_identity():
    _, _, gt_seg, gt_cls = perturbed()
    counts, iou, status, matches = check((gt_seg, gt_cls, gt_seg, gt_cls), 35, 'identity')
    n = int(status[:, 0].sum())
    assert n == status[:, 1].sum() == counts[:, 0].sum() > 300 and not counts[:, 1:].any()
    assert np.array_equal(iou, counts[:, 0].astype(np.float64))            # every IoU is exactly 1
    assert all((matches[b, :status[b, 0], 0] == matches[b, :status[b, 0], 3]).all() for b in range(3))


def test_the_threshold():
    cls_of = lambda seg, c2: np.where(seg == 0, 0, np.where(seg == 1, 1, c2))
    # |g| = |p| = 3, inter 2, union 4: IoU exactly 0.5 is no match; the background (5 and 5, inter 4, union 6) matches
    gt, pred = np.array([[1, 1, 1, 0, 0, 0, 0, 0]]), np.array([[0, 2, 2, 2, 0, 0, 0, 0]])
    counts = check(_batch(pred, cls_of(pred, 1), gt, cls_of(gt, 1)), 3, 'IoU 0.5')[0]
    assert counts.tolist() == [[1, 0, 0], [0, 1, 1], [0, 0, 0]]
    # |g| = |p| = 4, inter 3, union 5: a match; the background (4 and 4, inter 3, union 5) too
    gt, pred = np.array([[1, 1, 1, 1, 0, 0, 0, 0]]), np.array([[0, 2, 2, 2, 2, 0, 0, 0]])
    counts, iou, _, matches = check(_batch(pred, cls_of(pred, 1), gt, cls_of(gt, 1)), 3, 'IoU 0.6')
    assert counts.tolist() == [[1, 0, 0], [1, 0, 0], [0, 0, 0]] and iou.tolist() == [3 / 5, 3 / 5, 0.0]
    assert matches[0, :2].tolist() == [[0, 0, 4, 0, 3, 5], [1, 1, 4, 2, 3, 5]]
    # equal shapes of different class: one false positive and one false negative
    counts = check(_batch(gt, np.where(gt == 1, 2, 0), gt, cls_of(gt, 1)), 3, 'other class')[0]
    assert counts.tolist() == [[1, 0, 0], [0, 0, 1], [0, 1, 0]]


def test_void():
    hand = fx.hand_planes()
    mask = np.ones((1, 4, 6), np.float32)
    mask[0, 2, 5] = 0                                                      # 2 * void_p == |p9|: still a false positive
    assert check(_batch(*hand), 3, 'half void', mask=mask)[0].tolist() == [[1, 0, 0], [1, 0, 0], [1, 1, 1]]
    mask[0, 3, 5] = 0                                                      # one more: not counted
    assert check(_batch(*hand), 3, 'all void', mask=mask)[0].tolist() == [[1, 0, 0], [1, 0, 0], [1, 0, 1]]
    # g = 2 pixels inside p = 4 pixels: inter 2, union 4, no match -- until the other 2 pixels of p are void
    gt, pred = np.array([[1, 1, 0, 0, 0, 0, 0, 0]]), np.array([[2, 2, 2, 2, 0, 0, 0, 0]])
    planes = _batch(pred, (pred != 0) * 1, gt, (gt != 0) * 1)
    assert check(planes, 2, 'no void')[0].tolist() == [[1, 0, 0], [0, 1, 1]]
    mask = np.array([[[1, 1, 0, 0, 1, 1, 1, 1]]], np.float32)
    counts, iou, _, _ = check(planes, 2, 'void out of the union', mask=mask)
    assert counts.tolist() == [[1, 0, 0], [1, 0, 0]] and iou.tolist() == [1.0, 1.0]
    # ignore at and above n_class, alone and together with a mask
    gt_cls = hand[3].copy()
    gt_cls[2:, 4] = 3
    for ignore, cls_value in ((3, 3), (200, 200)):
        gt_cls[2:, 4] = cls_value
        got = check(_batch(hand[0], hand[1], hand[2], gt_cls), 3, 'ignore %d' % ignore, ignore=ignore, kinds=(1, 1, 1, 3))
        assert got[0].tolist() == [[1, 0, 0], [1, 0, 0], [2, 0, 0]]
    mask = np.ones((1, 4, 6), np.float32)
    mask[0, 0, :3] = 0
    check(_batch(hand[0], hand[1], hand[2], gt_cls), 3, 'mask and ignore', ignore=200, mask=mask)


def test_ids():
    yy, xx = np.mgrid[0:8, 0:8]
    ids = np.array([0, 255, 1000, 65535])
    gt = ids[(yy // 4) * 2 + xx // 4]
    pred = ids[::-1][(fx.shifted(yy, 1) // 4) * 2 + xx // 4]              # other ids on nearly the same quadrants
    cls = lambda seg: (seg > 200) * 1 + (seg > 60000) * 1                   # 0, 1, 1, 2 in id order
    pred_cls = (pred < 60000) * 1 + (pred < 200) * 1                        # the class of the quadrant's ground truth
    got = check(_batch(pred, pred_cls, gt, cls(gt)), 3, 'sparse ids', kinds=(2, 0, 1, 2))
    assert got[3][0, :4, 0].tolist() == [0, 255, 1000, 65535] and got[2].tolist() == [[4, 4, 0, 0]]
    one = np.full((1, 97, 193), 65535)
    counts, iou, status, _ = check((one, one * 0 + 7, one, one * 0 + 7), 8, 'one id')
    assert counts[7].tolist() == [1, 0, 0] and iou[7] == 1.0 and status.tolist() == [[1, 1, 0, 0]]
    one = np.full((1, 96, 192), 4)                                           # the vector path, five shares
    check((one, one, one, one), 8, 'one id, vector path', kinds=(0, 0, 0, 0))
    seg, c = fx.own_ids(16, 32)
    got = check(_batch(fx.shifted(seg, 0, 1), c, seg, c), 4, 'runs of length 1')
    assert got[2].tolist() == [[512, 16 * 31, 0, 0]]


def test_shapes():
    planes = tuple(a[None] for a in fx.stripes_and_bands())
    check(planes, 5, 'runs across every share border')
    check(planes, 5, 'bases shifted by one element', shift=1)
    check(planes, 5, 'bytes shifted by one element', shift=1, kinds=(0, 0, 0, 0))
    mask = (np.random.RandomState(3).rand(*planes[0].shape) > 0.3).astype(np.float32)
    check(planes, 5, 'with a mask', mask=mask, kinds=(0, 3, 2, 1))
    for W in (5, 7, 130):                                                  # no multiple of PX
        p = tuple(a[None, :, :W] for a in fx.stripes_and_bands(40, 256))
        check(p, 5, 'width %d' % W, kinds=(1, 0, 2, 3))
    pred_seg, pred_cls, gt_seg, gt_cls = perturbed(96, 192)                # the vector path on a real layout
    check((pred_seg[:2], pred_cls[:2], gt_seg[:2], gt_cls[:2]), 35, 'perturbed 96 x 192', kinds=(1, 0, 2, 3))


def test_every_kind_combination():
    wide = tuple(np.kron(a, np.ones((1, 2), np.int64))[None] for a in fx.hand_planes())      # 4 x 12: the vector path
    ref = fx.match_reference(*wide, 3)
    for kinds in itertools.product((0, 1, 2), (0, 1, 2, 3), (0, 1, 2), (0, 1, 2, 3)):
        assert_equal(call_match(wide, 3, kinds=kinds, max_segments=16), ref, 'kinds %s' % (kinds,))
    narrow = _batch(*fx.hand_planes())                                     # 4 x 6: element by element
    for k in range(3):
        check(narrow, 3, 'element path kinds %d' % k, kinds=(k, k, k, k + 1), max_segments=16)


def _three_planes(special=None):
    """B = 3 planes of 33 x 65: small layouts, or ``special`` (pred_seg, pred_cls, gt_seg, gt_cls) between two of them."""
    out = [[], [], [], []]
    for b in range(3):
        if b == 1 and special is not None:
            planes = special
        else:
            cls = cf.coarse_layout(33, 65, seed=40 + b).astype(np.int64)
            seg = cf.label_reference(cls, cf.CITY_THINGS, 8)[0].astype(np.int64)
            planes = (fx.shifted(seg, 1, 0), fx.shifted(cls, 1, 0), seg, cls)
        for lst, a in zip(out, planes):
            lst.append(np.asarray(a, np.int64))
    return tuple(np.stack(v) for v in out)


def test_flags():
    seg, cls = fx.own_ids(33, 65)
    planes = _three_planes((seg, cls, seg, cls))
    counts, _, status, _ = check(planes, 35, 'overflow')
    assert status[1].tolist() == [2145, 2145, fx.OVERFLOW, 0] and status[0, 2] == status[2, 2] == 0
    others = fx.match_reference(*(a[[0, 2]] for a in planes), 35)[0]       # the other two planes are counted, alone
    assert np.array_equal(counts, others) and counts[:, 0].sum() > 0
    base = _three_planes()
    for bad, kind in ((65536, 1), (-1, 1), (1 << 40, 2), (-1, 2)):
        for side in (0, 2):
            planes = [a.copy() for a in base]
            planes[side][1, 5, 7] = bad
            kinds = [1, 1, 1, 1]
            kinds[side] = kind
            status = check(tuple(planes), 35, 'id %d' % bad, kinds=tuple(kinds))[2]
            assert status[:, 2].tolist() == [0, fx.ID_RANGE, 0]
    for bad, kind in ((35, 1), (255, 0), (-1, 2), (3.5, 3), (float('nan'), 3)):
        for side in (1, 3):
            planes = [a.astype(np.float64) for a in base]
            planes[side][1, 5, 7] = bad
            kinds = [1, 1, 1, 1]
            kinds[side] = kind
            status = check(tuple(planes), 35, 'class %r' % bad, kinds=tuple(kinds))[2]
            assert status[:, 2].tolist() == [0, fx.CLS_RANGE, 0]
    planes = [a.copy() for a in base]
    planes[1][1, 5, 7] = (planes[1][1, 5, 7] + 1) % 35                      # another class under a predicted segment
    status = check(tuple(planes), 35, 'mixed')[2]
    assert status[:, 2].tolist() == [0, fx.MIXED, 0]


def test_accumulate_equals_the_concatenated_batch():
    planes = perturbed()
    first, second = tuple(a[:2] for a in planes), tuple(a[1:] for a in planes)
    zero = (np.zeros((35, 3), np.int64), np.zeros(35), np.zeros((2, 4), np.int32))
    a = call_match(first, 35, into=zero, want_matches=False)
    b = call_match(second, 35, into=a[:3], want_matches=False)
    whole = tuple(np.concatenate([x, y]) for x, y in zip(first, second))
    ref = fx.match_reference(*whole, 35)
    one = call_match(whole, 35, want_matches=False)
    assert_equal(one, ref, 'concatenated')
    pooled = ref[2][:2] + ref[2][2:]
    pooled[:, 2] = ref[2][:2, 2] | ref[2][2:, 2]
    assert_equal(b, (ref[0], ref[1], pooled, ref[3]), 'accumulated')
    assert np.array_equal(b[0], one[0]) and np.array_equal(b[2][:, :2], one[2][:2, :2] + one[2][2:, :2])
    # an accumulating call keeps flags that were there and the caller's spare bit
    kept = (a[0], a[1], a[2] | np.array([[0, 0, fx.CCL, 0], [0, 0, fx.MIXED, 0]], np.int32))
    c = call_match(second, 35, into=kept, want_matches=False)
    assert c[2][:, 2].tolist() == [fx.CCL, fx.MIXED] and np.array_equal(c[0], b[0])


def test_matches_may_be_null():
    planes = perturbed()
    with_rows = call_match(planes, 35)
    without = call_match(planes, 35, want_matches=False)
    assert without[3] is None
    for x, y in zip(with_rows[:3], without[:3]):
        assert x.tobytes() == y.tobytes()


def test_perturbed_layout():
    planes = perturbed()
    counts, iou, status, matches = check(planes, 35, 'perturbed layout')
    assert counts[:, 0].sum() > 50 and counts[:, 1].sum() > 50 and counts[:, 2].sum() > 50
    mask = (np.random.RandomState(9).rand(3, 97, 193) > 0.1).astype(np.float32)
    check(planes, 35, 'perturbed layout, mask and ignore', mask=mask, ignore=7, kinds=(1, 0, 1, 0))
    check(planes, 35, 'perturbed layout, few segments allowed', max_segments=150)
