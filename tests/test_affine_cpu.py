"""not gpu: the host side of the affine layout edits -- ``ops.affine_map`` (exact quarter turns and flips, the inverse,
the destination box by brute force, every refusal), the oracle of tests/affine_fixture.py on masks written out by hand,
the C ABI's declarations, exports and signatures, the refusals the library makes before it launches anything, and the
argument checks of the ``ops`` wrappers and of ``JointInference``."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import affine_fixture as fx
from neurips18_hierchical_image_manipulation_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
ONE = 1 << 24
BOXES = [(3, 5, 10, 9), (2, 2, 7, 7), (4, 1, 5, 10), (0, 0, 9, 1)]          # 7 x 4, 5 x 5, 1 x 9, 9 x 1
PERMUTATIONS = [dict(angle=a, flip=f) for a in (0, 90, 180, 270, -90, 450) for f in ('', 'x', 'y', 'xy')]
GENERAL = [dict(angle=30), dict(angle=-17.5), dict(shear=0.3), dict(scale=(0.5, 1.7)), dict(angle=200, scale=1.3, shear=-0.4),
           dict(angle=45, flip='x', scale=(2.0, 0.7), shift=(3.5, -2.25))]


def _plane(rows):
    return np.array([[int(c) for c in r] for r in rows], np.int64)


# ---------------------------------------------------------------------------------------------------------- affine_map
def test_identity_and_record():
    m = ops.affine_map((3, 5, 10, 9))
    assert m.inv == (ONE, 0, 0, 0, ONE, 0) and all(type(v) is int for v in m.inv)
    assert m.dst_box == (3, 5, 10, 9) and m.src_box == (3, 5, 10, 9)
    assert m.fwd.dtype == np.float64 and m.fwd.shape == (2, 3) and np.array_equal(m.fwd, [[1, 0, 0], [0, 1, 0]])
    with pytest.raises(ValueError):
        m.fwd[0, 0] = 2.0                                                    # read-only
    with pytest.raises(AttributeError):
        m.inv = ()
    s = ops.affine_map((3, 5, 10, 9), shift=(4, -7))
    assert s.inv == (ONE, 0, -4 * ONE, 0, ONE, 7 * ONE) and s.dst_box == (7, -2, 14, 2)
    c = ops.affine_map((3, 5, 10, 9), dst_center=(20, 30.5))
    assert c.dst_box == (17, 29, 24, 33)


@pytest.mark.parametrize('box', BOXES)
@pytest.mark.parametrize('kw', PERMUTATIONS, ids=lambda k: '%s%s' % (k['angle'], k['flip']))
def test_quarter_turns_and_flips_permute_pixels(box, kw):
    m = ops.affine_map(box, shift=(2, -1), **kw)
    x0, y0, x1, y1 = m.dst_box
    y, x = np.mgrid[y0 - 2:y1 + 2, x0 - 2:x1 + 2]
    U, V = fx.uv(m.inv, x, y)
    assert not (U & (ONE - 1)).any() and not (V & (ONE - 1)).any()           # all-zero fractions: no tie, weights (0,1,0,0)
    w, h = box[2] - box[0], box[3] - box[1]
    swap = (kw['angle'] // 90) % 2 == 1
    assert (x1 - x0, y1 - y0) == ((h, w) if swap else (w, h))
    xs, ys = fx.nearest(m.inv, x, y)
    inside = (xs >= box[0]) & (xs < box[2]) & (ys >= box[1]) & (ys < box[3])
    # a bijection between the destination box and the source box
    assert np.array_equal(inside, (x >= x0) & (x < x1) & (y >= y0) & (y < y1))
    assert len(set(zip(xs[inside].tolist(), ys[inside].tolist()))) == w * h
    # the centre moved by the shift, snapped by at most half a pixel towards +x / +y
    cs = np.array([(box[0] + box[2] - 1) / 2.0, (box[1] + box[3] - 1) / 2.0])
    cd = np.array([(x0 + x1 - 1) / 2.0, (y0 + y1 - 1) / 2.0])
    snap = cd - (cs + np.array([2, -1]))
    assert ((snap == 0) | (snap == 0.5)).all(), snap


@pytest.mark.parametrize('box', BOXES)
@pytest.mark.parametrize('kw', PERMUTATIONS[:8] + GENERAL, ids=str)
def test_forward_map_composed_with_the_inverse_returns_every_source_pixel(box, kw):
    m = ops.affine_map(box, **kw)
    y, x = np.mgrid[box[1]:box[3], box[0]:box[2]]
    d = m.fwd[:, :2] @ np.stack([x.ravel(), y.ravel()]).astype(np.float64) + m.fwd[:, 2:]
    a = np.array(m.inv, np.float64).reshape(2, 3) / ONE
    back = a[:, :2] @ d + a[:, 2:]
    # the coefficients are rounded to 2^-24: 2 * 2^-25 * |d| + 2^-25 per coordinate, |d| < 64 here
    assert np.abs(back - np.stack([x.ravel(), y.ravel()])).max() <= 2.0 ** -17


@pytest.mark.parametrize('box', BOXES)
@pytest.mark.parametrize('kw', PERMUTATIONS[:8] + GENERAL, ids=str)
def test_dst_box_holds_every_pixel_that_reads_the_source_box(box, kw):
    m = ops.affine_map(box, **kw)
    x0, y0, x1, y1 = m.dst_box
    margin = 12
    y, x = np.mgrid[y0 - margin:y1 + margin, x0 - margin:x1 + margin]
    xs, ys = fx.nearest(m.inv, x, y)
    inside = (xs >= box[0]) & (xs < box[2]) & (ys >= box[1]) & (ys < box[3])
    assert inside.any()
    in_box = (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
    assert not (inside & ~in_box).any()
    # rounded outwards, not padded: every side of the box is within a pixel of a pixel that reads the source
    yy, xx = np.nonzero(inside)
    assert xx.min() + x0 - margin <= x0 + 1 and xx.max() + x0 - margin >= x1 - 2
    assert yy.min() + y0 - margin <= y0 + 1 and yy.max() + y0 - margin >= y1 - 2


def test_affine_map_refusals():
    box = (3, 5, 10, 9)
    nan, inf = float('nan'), float('inf')
    bad = [dict(angle=nan), dict(angle=inf), dict(angle='a'), dict(angle=True), dict(shear=nan), dict(shear=2.01), dict(shear=-3),
           dict(scale=nan), dict(scale=(1, inf)), dict(scale=(1, 2, 3)), dict(scale='a'), dict(scale=0), dict(scale=0.2),
           dict(scale=4.1), dict(scale=(1, -0.1)), dict(scale=3, shear=2),       # a singular value of 7.2
           dict(flip='z'), dict(flip='xx'), dict(flip=None), dict(flip=1), dict(shift=(nan, 0)), dict(shift=3), dict(shift=(1, 2, 3)),
           dict(dst_center=(0, inf)), dict(dst_center=5), dict(shift=(1 << 21, 0)), dict(dst_center=(0, -(1 << 21)))]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.affine_map(box, **kw)
    for b in ((3, 5, 3, 9), (3, 5, 10), (0.5, 0, 4, 4), None):
        with pytest.raises(ValueError):
            ops.affine_map(b)
    for kw in (dict(scale=4), dict(scale=0.25), dict(shear=2, scale=1.5), dict(scale=(0.25, 4)), dict(flip='yx')):
        ops.affine_map(box, **kw)                                            # the limits themselves pass
    assert list(inspect.signature(ops.affine_map).parameters) == ['src_box', 'angle', 'scale', 'shear', 'flip', 'shift',
                                                                  'dst_center']
    assert 'alias' in ops.affine_map.__doc__ and 'Pillow' in ops.affine_map.__doc__


# -------------------------------------------------------------------------------------------------- the oracle, by hand
HAND = _plane(['1100000',
               '1010000',
               '0001000',
               '0000110',
               '0000011'])


def _rotated(mask, **kw):
    h, w = mask.shape
    src = np.zeros((h + 4, w + 6), np.int64)
    src[2:2 + h, 3:3 + w] = mask * 7
    m = ops.affine_map((3, 2, 3 + w, 2 + h), **kw)
    return fx.mask(src, 7, m.src_box, m.dst_box, m.inv), m


def test_oracle_quarter_turns_and_flips_of_a_mask_written_out_by_hand():
    got, m = _rotated(HAND, angle=90)
    assert got.shape == (7, 5) and np.array_equal(got, np.rot90(HAND).astype(bool))   # rot90 is counter-clockwise
    assert np.array_equal(got, _plane(['00001', '00011', '00010', '00100', '01000', '10000', '11000']).astype(bool))
    assert np.array_equal(_rotated(HAND, angle=180)[0], np.rot90(HAND, 2).astype(bool))
    assert np.array_equal(_rotated(HAND, angle=270)[0], np.rot90(HAND, 3).astype(bool))
    assert np.array_equal(_rotated(HAND, flip='x')[0], HAND[:, ::-1].astype(bool))
    assert np.array_equal(_rotated(HAND, flip='y')[0], HAND[::-1].astype(bool))
    assert np.array_equal(_rotated(HAND, angle=90, flip='x')[0], np.rot90(HAND[:, ::-1]).astype(bool))   # flip first


def test_oracle_rotated_square_has_the_area_and_the_symmetry_of_the_map():
    """A filled 9 x 9 square turned by 30 degrees about its centre, which stays a pixel centre.  A destination pixel at
    the offset (dx, dy) from the centre is set iff its source point (c dx - s dy, s dx + c dy), c = cos 30, s = sin 30
    (the transpose of the forward rotation [[c, s], [-s, c]]), lies in [-4.5, 4.5)^2.  Counted here directly in float64
    with a margin of 1e-6 either way: no lattice point comes that close to a side, so the count is unambiguous -- 81
    pixels, in rows of 3, 5, 7, 10, 10, 11, 10, 10, 7, 5, 3 -- and the map's 2^-24 rounding (below 2^-20 pixel here)
    cannot move one across.  The map commutes with the point reflection about the centre, so the mask equals itself
    turned by 180 degrees except where the half-open sides decide: compared on the pixels whose source point is at least
    2^-10 away from a side."""
    src = np.zeros((15, 16), np.int64)
    src[3:12, 2:11] = 5
    m = ops.affine_map((2, 3, 11, 12), angle=30)
    got = fx.mask(src, 5, m.src_box, m.dst_box, m.inv)
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    want = np.zeros((13, 13), int)
    for dy in range(-6, 7):
        for dx in range(-6, 7):
            r = max(abs(c * dx - s * dy), abs(s * dx + c * dy))
            assert abs(r - 4.5) > 1e-6
            want[dy + 6, dx + 6] = r < 4.5
    assert want.sum(1).tolist() == [0, 3, 5, 7, 10, 10, 11, 10, 10, 7, 5, 3, 0] and want.sum() == 81
    assert np.array_equal(got, want.astype(bool))
    x0, y0, x1, y1 = m.dst_box
    assert (x0 + x1 - 1) / 2.0 == 6.0 and (y0 + y1 - 1) / 2.0 == 7.0 and got.shape[0] == got.shape[1]
    y, x = np.mgrid[y0:y1, x0:x1]
    U, V = fx.uv(m.inv, x, y)
    clear = np.ones_like(got)
    for c, lo, hi in ((U, 2, 11), (V, 3, 12)):
        for side in (lo, hi):
            clear &= np.abs(c - (side * ONE - fx.HALF)) > (1 << 14)
    turned = got[::-1, ::-1]
    assert np.array_equal(got[clear & clear[::-1, ::-1]], turned[clear & clear[::-1, ::-1]])
    assert got[got.shape[0] // 2, got.shape[1] // 2] and not got[0, 0] and not got[-1, -1]
    # the four corners of the turned square reach the box's sides: 9 * (cos 30 + sin 30) = 12.29 -> 13 pixels
    assert got.shape == (13, 13)


def test_oracle_place_counts_blocks_and_clips():
    src = np.zeros((6, 8), np.int64)
    src[1:4, 2:6] = [[9, 9, 9, 9], [9, 8, 0, 9], [9, 0, 0, 0]]             # 8: another instance inside the box
    label = np.full((6, 8), 2, np.int64)
    label[:, 1] = 6
    inst = label.copy()
    m = ops.affine_map((2, 1, 6, 4), angle=90, shift=(-2.5, -0.5))        # centre (3.5, 2) -> (1, 1.5)
    assert m.dst_box == (0, 0, 3, 4)
    want = np.rot90(src[1:4, 2:6] == 9)
    lo, io, ch, st, mask = fx.place(label, inst, src, 9, m.src_box, m.dst_box, m.inv, 7, 90, protect=(6,))
    assert np.array_equal(mask, want)
    full = np.zeros((6, 8), bool)
    full[0:4, 0:3] = want
    blocked, wrote = full & (label == 6), full & (label != 6)
    assert st == [int(wrote.sum()), int(blocked.sum()), 0, 0, 2, 3] and blocked.sum() == 2   # column 1 of [110, 100, 100, 111]
    assert np.array_equal(ch, wrote.astype(np.uint8)) and (lo[wrote] == 7).all() and (io[wrote] == 90).all()
    assert np.array_equal(lo[~wrote], label[~wrote])
    off = ops.affine_map((2, 1, 6, 4), angle=90, shift=(-4.5, -0.5))            # hangs over the left edge
    _, _, ch2, st2, mask2 = fx.place(label, inst, src, 9, off.src_box, off.dst_box, off.inv, 7, 90)
    assert np.array_equal(mask2, want) and st2[0] == int(want[:, 2:].sum()) and st2[2] == 0
    _, _, ch3, st3, _ = fx.place(label, inst, src, 5, m.src_box, m.dst_box, m.inv, 7, 90)
    assert not ch3.any() and st3 == [0, 0] + fx.EMPTY_BOX


def test_oracle_bicubic_weights_and_bound_terms():
    w = fx.keys(np.array([0.0, 0.5, 0.25]))
    assert np.array_equal(w[:, 0], [0.0, 1.0, 0.0, 0.0])
    assert np.allclose(w[:, 1], [-0.0625, 0.5625, 0.5625, -0.0625], rtol=0, atol=1e-15)
    assert np.allclose(w.sum(0), 1.0, rtol=0, atol=1e-15)
    src = fx.picture(1, 6, 7)
    ident = (ONE, 0, 0, 0, ONE, 0)
    ref, S, A = fx.warp(src, ident, (0, 0, 6, 7))
    assert np.array_equal(ref, src.astype(np.float64)) and np.array_equal(S, np.abs(ref)) and (A >= S).all()
    half = (ONE, 0, ONE // 2, 0, ONE, 0)                                      # half a pixel to the right, row 0
    ref, _, _ = fx.warp(src, half, (2, 0, 1, 1))
    row = src[:, 0, 1:5].astype(np.float64)
    assert np.allclose(ref[:, 0, 0], row @ [-0.0625, 0.5625, 0.5625, -0.0625], rtol=0, atol=1e-15)
    far = fx.warp(src, ident, (-5, -5, 2, 2))[0]                             # every tap clamped to the corner pixel
    assert np.allclose(far, src[:, :1, :1], rtol=0, atol=1e-15)
    assert fx.reads(ident, (0, 0, 6, 7), 6, 7, 3, 3).sum() == 16 and fx.reads(ident, (0, 0, 6, 7), 6, 7, 0, 0).sum() == 4


# ------------------------------------------------------------------------------------------------------------ the C ABI
NAMES = ('him_layout_place_affine', 'him_canvas_warp_affine')


def test_header_declares_and_library_exports_the_entry_points_with_the_ctypes_signatures():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        header = f.read()
    assert 'Affine layout edits' in header
    for decl in (r'^int him_layout_place_affine\(', r'^int him_canvas_warp_affine\('):
        assert re.search(decl, header, flags=re.M), decl
    assert os.path.isfile(_cabi.LIB_PATH), 'libhim_hip.so not built'
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    plain = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in NAMES:
        assert name in _cabi.EXPORTS and hasattr(dll, name), name
        ret, params = re.search(r'^(\w+) %s\(([^)]*)\);' % name, plain, flags=re.M | re.S).groups()
        res, args = _cabi._SIGS[name]
        assert ret == 'int' and res is ctypes.c_int
        want = [ctypes.c_void_p if '*' in prm else ctypes.c_int for prm in params.split(',')]
        assert list(args) == want, name
    # the affine place takes him_layout_place's arguments with xs / ys replaced by inv
    place = re.search(r'^int him_layout_place\(([^)]*)\);', plain, flags=re.M | re.S).group(1)
    affine = re.search(r'^int him_layout_place_affine\(([^)]*)\);', plain, flags=re.M | re.S).group(1)
    norm = lambda s: [' '.join(p.split()) for p in s.split(',')]         # noqa: E731
    want = norm(place)
    i = want.index('const int* xs')
    assert want[i + 1] == 'const int* ys' and norm(affine) == want[:i] + ['const long long* inv'] + want[i + 2:]
    assert (ops.AFFINE_FRAC_BITS, ops.AFFINE_MAX_LINEAR, ops.AFFINE_MAX_OFFSET) == (fx.FRAC, fx.MAX_LINEAR, fx.MAX_OFFSET)


def _inv(*v):
    return (ctypes.c_longlong * 6)(*v)


def test_library_refuses_bad_arguments_before_any_launch():
    """Nothing below reaches a launch: the device addresses are never dereferenced on the host, and every call is
    refused.  ``inv`` is host memory and real."""
    from neurips18_hierchical_image_manipulation_amd import _cabi
    dll = _cabi.lib._load()
    H, W = 64, 96
    p, step = 1 << 24, 1 << 20                          # aligned, non-null, far apart; never read
    ident = _inv(ONE, 0, 0, 0, ONE, 0)
    ia = ctypes.addressof(ident)
    order = ['inst_src', 'inst_kind', 'Hs', 'Ws', 'id', 'sx0', 'sy0', 'sx1', 'sy1', 'inv', 'label_dst', 'label_kind',
             'inst_dst', 'Hd', 'Wd', 'dx0', 'dy0', 'dx1', 'dy1', 'cls', 'new_id', 'protect', 'n_class', 'changed', 'status',
             'stream']
    good = dict(inst_src=p, inst_kind=1, Hs=H, Ws=W, id=5, sx0=3, sy0=4, sx1=20, sy1=30, inv=ia, label_dst=p + 3 * step,
                label_kind=0, inst_dst=p + 4 * step, Hd=H, Wd=W, dx0=-5, dy0=-6, dx1=40, dy1=50, cls=7, new_id=1005,
                protect=0, n_class=0, changed=p + 5 * step, status=p + 6 * step, stream=0)
    bad = [('inst_src', 0), ('inv', 0), ('label_dst', 0), ('inst_dst', 0), ('status', 0), ('inst_kind', 4),
           ('label_kind', -1), ('Hs', 0), ('Wd', 16385), ('sx0', -1), ('sx1', W + 1), ('sy1', 4), ('sy1', H + 1), ('dx1', -5),
           ('dy1', -7), ('dx0', -(1 << 20) - 1), ('dy1', (1 << 20) + 1), ('cls', 256), ('cls', -1), ('protect', p + 7 * step),
           ('inst_src', p + 1), ('inv', ia + 4), ('status', p + 6 * step + 2),
           # the aliasing refusals of him_layout_place
           ('inst_src', p + 4 * step), ('inst_src', p + 3 * step), ('inst_src', p + 4 * step - 4), ('inst_src', p + 5 * step),
           ('inst_dst', p + 3 * step), ('changed', p + 4 * step + 8)]
    for name, value in bad:
        rc = dll.him_layout_place_affine(*[dict(good, **{name: value})[k] for k in order])
        assert rc == E_INVALID, (name, value, rc)
        assert b'layout_place_affine' in dll.him_last_error(), (name, dll.him_last_error())
    assert b'overlaps' in (dll.him_layout_place_affine(*[dict(good, inst_src=p + 4 * step)[k] for k in order]),
                           dll.him_last_error())[1]
    # coefficient limits: the limit itself is not refused for its value (the call is refused for a NULL status instead,
    # with another message), one past it is
    lin, off = 1 << 30, 1 << 52
    for k in range(6):
        lim = off if k in (2, 5) else lin
        for sign in (1, -1):
            v = [ONE, 0, 0, 0, ONE, 0]
            v[k] = sign * (lim + 1)
            over = _inv(*v)
            assert dll.him_layout_place_affine(*[dict(good, inv=ctypes.addressof(over))[a] for a in order]) == E_INVALID
            assert b'coefficient' in dll.him_last_error()
            v[k] = sign * lim
            at = _inv(*v)
            assert dll.him_layout_place_affine(*[dict(good, inv=ctypes.addressof(at), status=0)[a] for a in order]) == E_INVALID
            assert b'null' in dll.him_last_error()

    order = ['src', 'Hs', 'Ws', 'inv', 'x0', 'y0', 'H', 'W', 'P', 'stream']
    good = dict(src=p, Hs=H, Ws=W, inv=ia, x0=-3, y0=5, H=40, W=50, P=p + step, stream=0)
    bad = [('src', 0), ('inv', 0), ('P', 0), ('src', p + 2), ('P', p + step + 1), ('inv', ia + 4), ('Hs', 0), ('Ws', 16385),
           ('H', 0), ('W', 0), ('H', 2049), ('W', 2049), ('x0', (1 << 20) + 1), ('y0', -(1 << 20) - 1),
           ('P', p), ('P', p + 3 * H * W * 4 - 4), ('src', p + step + 4)]
    for name, value in bad:
        rc = dll.him_canvas_warp_affine(*[dict(good, **{name: value})[k] for k in order])
        assert rc == E_INVALID, (name, value, rc)
        assert b'canvas_warp_affine' in dll.him_last_error(), (name, dll.him_last_error())
    for k in range(6):
        v = [ONE, 0, 0, 0, ONE, 0]
        v[k] = -((off if k in (2, 5) else lin) + 1)
        over = _inv(*v)
        assert dll.him_canvas_warp_affine(*[dict(good, inv=ctypes.addressof(over))[a] for a in order]) == E_INVALID
        assert b'coefficient' in dll.him_last_error()


# ------------------------------------------------------------------------------------------------- wrappers, host side
def test_ops_wrappers_refuse_bad_arguments_before_any_device_work():
    """Every refusal is a ValueError raised on the host: the planes here are host tensors, refused last."""
    lab = torch.zeros(1, 1, 8, 9)
    amap = ops.affine_map((0, 0, 4, 4), angle=30)
    good = dict(id=3, amap=amap, cls=5, new_id=1003)
    place_bad = [dict(id='a'), dict(id=True), dict(amap=None), dict(amap=(amap.inv, amap.fwd, amap.dst_box, amap.src_box)),
                 dict(amap=amap._replace(inv=amap.inv[:5])), dict(amap=amap._replace(inv=amap.inv + (0,))),
                 dict(amap=amap._replace(inv=None)), dict(amap=amap._replace(inv=(1 << 31,) + amap.inv[1:])),
                 dict(amap=amap._replace(inv=(1.5,) + amap.inv[1:])), dict(amap=amap._replace(dst_box=(5, 1, 5, 7))),
                 dict(amap=amap._replace(src_box=(0, 0, 0, 4))), dict(amap=amap._replace(src_box=(0, 0, 40, 4))),
                 dict(cls=None), dict(new_id=1.5), dict(protect=(70000,)), dict(protect=3), dict()]
    for kw in place_bad:
        kw = dict(good, **kw)
        with pytest.raises(ValueError):
            ops.layout_place_affine(lab, lab, lab, kw.pop('id'), kw.pop('amap'), kw.pop('cls'), kw.pop('new_id'), **kw)
    assert list(inspect.signature(ops.layout_place_affine).parameters) == ['label_dst', 'inst_dst', 'inst_src', 'id', 'amap',
                                                                           'cls', 'new_id', 'protect']
    img = torch.zeros(1, 3, 8, 9)
    for amap_, window in ((None, (0, 0, 4, 4)), (amap, (0, 0, 4)), (amap, (0, 0, 0, 4)), (amap, (0, 0, 4, 2049)),
                          (amap, (0.5, 0, 4, 4)), (amap, (1 << 21, 0, 4, 4)), (amap, None)):
        with pytest.raises(ValueError):
            ops.canvas_warp_affine(img, amap_, window)
    assert list(inspect.signature(ops.canvas_warp_affine).parameters) == ['src', 'amap', 'window']
    region = torch.zeros(8, 9, dtype=torch.uint8)
    canvas = torch.zeros(1, 3, 8, 9)
    clone_bad = [dict(amap=None), dict(amap=ops.affine_map((0, 0, 4, 4), shift=(40, 0))), dict(mixed=1), dict(rtol=0.0),
                 dict(rtol=1.0), dict(rtol='x'), dict(max_iter=0), dict(max_iter=1.5), dict(max_iter=(1 << 20) + 1),
                 dict(src=canvas)]
    for kw in clone_bad:
        kw = dict(dict(src=img, amap=amap), **kw)
        with pytest.raises(ValueError):
            ops.canvas_clone_region_affine(kw.pop('src'), kw.pop('amap'), canvas, region, **kw)
    assert list(inspect.signature(ops.canvas_clone_region_affine).parameters) == ['src', 'amap', 'canvas', 'region', 'mixed',
                                                                                  'rtol', 'max_iter']


def test_joint_inference_adds_the_affine_edits_and_keeps_the_others():
    from neurips18_hierchical_image_manipulation_amd.models import joint_inference_model as jm
    ji = jm.JointInference
    lead = ['label_original', 'inst_original', 'img_original', 'opt']
    for name, first in (('transform_object', ['obj']), ('rotate_object', ['obj', 'angle']), ('flip_object', ['obj', 'axis']),
                        ('move_object', ['obj', 'dst_box']), ('rescale_object', ['obj', 'scale']), ('remove_object', ['obj'])):
        prm = inspect.signature(getattr(ji, name)).parameters
        assert list(prm)[:1 + len(first) + 4] == ['self'] + first + lead, name
    prm = inspect.signature(ji.transform_object).parameters
    want = dict(angle=0.0, scale=1.0, shear=0.0, flip='', shift=(0, 0), fill=None, things=None, protect=(), new_id=None,
                feather=None, reach=0, profile='smooth', seamless=False, keep_appearance=False, mixed=False)
    assert list(prm)[6:] == list(want)
    for k, default in want.items():
        assert prm[k].kind is inspect.Parameter.KEYWORD_ONLY and prm[k].default == default, k
    assert list(inspect.signature(ji.move_object).parameters)[7:] == ['fill', 'things', 'protect', 'new_id', 'feather', 'reach',
                                                                      'profile', 'seamless', 'keep_appearance', 'mixed']
    # refused on the host before any device work (self is never touched)
    obj = (7, {'bbox': [3, 4, 10, 12], 'cls': 26})
    for kw in (dict(angle=float('nan')), dict(scale=5), dict(shear=3), dict(flip='q'), dict(seamless=1),
               dict(mixed=True), dict(keep_appearance='yes')):
        with pytest.raises(ValueError):
            ji.transform_object(None, obj, None, None, None, None, **kw)
    with pytest.raises(ValueError):
        ji.transform_object(None, (7, {'cls': 1}), None, None, None, None)
