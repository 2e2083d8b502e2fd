"""not gpu: the host side of the layout edits -- the brute-force oracle of tests/layout_edit_fixture.py on 5 x 7 planes
whose answers are written out here, the C ABI's declarations, exports and signatures, the refusals the library makes
before it launches anything (the aliasing refusal among them) and the argument checks of the ``ops`` wrappers and of the
``JointInference`` helpers."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import layout_edit_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_WORKSPACE = -1, -2


def _plane(rows):
    return np.array([[int(c) for c in r] for r in rows], np.int64)


# ------------------------------------------------------------------------------------------- the oracle, by hand (5 x 7)
def test_oracle_erase_fills_from_the_nearest_allowed_class_and_jumps_a_forbidden_one():
    label = _plane(['1111222',
                    '1199322',
                    '1199322',
                    '1111222',
                    '1111222'])
    inst = label.copy()
    inst[label == 9] = 50
    # class 3 touches the object on its right but is not a filler: the fill jumps over it to class 2
    lo, io, ch, st = fx.erase(label, inst, id=50, fill=(1, 2), n_class=10)
    want = _plane(['1111222',
                   '1111322',
                   '1111322',
                   '1111222',
                   '1111222'])
    # (1,3): class 1 at (0,3) and (1,1)... distance 1 to (0,3); class 2 at (1,5) is 2 away.  (1,2): (0,2) / (1,1) both at
    # distance 1, the smaller index (0,2) wins: the same class here, another instance id below
    assert np.array_equal(lo, want) and np.array_equal(io, want)
    assert st == [4, 35 - 4 - 2, 4, 0] and np.array_equal(ch, (label == 9).astype(np.uint8))
    lo3, _, _, st3 = fx.erase(label, inst, id=50, fill=(3,), n_class=10)
    assert (lo3[label == 9] == 3).all() and st3 == [4, 2, 4, 0]
    # the windowed search gives the same answer, whatever margin it starts from
    for m in (1, 2, 50):
        assert np.array_equal(fx.erase(label, inst, id=50, fill=(2,), n_class=10, window=m)[0],
                              fx.erase(label, inst, id=50, fill=(2,), n_class=10)[0])


def test_oracle_tie_takes_the_smallest_flat_index():
    label = _plane(['0000000',
                    '0040000',
                    '0507000',
                    '0060000',
                    '0000000'])
    inst = label.copy()
    inst[2, 2] = 77                                     # a one-pixel object between four different neighbours
    label[2, 2] = 8
    lo, io, ch, st = fx.erase(label, inst, id=77, fill=(4, 5, 6, 7), n_class=9)
    assert lo[2, 2] == 4 and io[2, 2] == 4              # (1,2) < (2,1) < (2,3) < (3,2)
    assert st == [1, 4, 1, 0] and ch.sum() == 1
    lo, _, _, _ = fx.erase(label, inst, id=77, fill=(5, 6, 7), n_class=9)
    assert lo[2, 2] == 5
    lo, _, _, _ = fx.erase(label, inst, id=77, fill=(6, 7), n_class=9)
    assert lo[2, 2] == 7                                # (2,3) before (3,2)


def test_oracle_empty_sets_and_out_of_range_labels():
    label = _plane(['1111111'] * 5)
    inst = label.copy()
    inst[1:3, 2:4] = 30
    lo, io, ch, st = fx.erase(label, inst, id=30, fill=(2,), n_class=4)          # no seed: copies, flag
    assert np.array_equal(lo, label) and np.array_equal(io, inst) and not ch.any() and st == [4, 0, 0, fx.NO_SEED]
    lo, io, ch, st = fx.erase(label, inst, id=31, fill=(1,), n_class=4)          # empty region: copies
    assert np.array_equal(lo, label) and np.array_equal(io, inst) and st == [0, 35, 0, 0]
    label[1, 2], label[0, 0] = 9, 9                                              # outside [0, 4): in R, and a non-seed
    lo, io, ch, st = fx.erase(label, inst, id=30, fill=(1,), n_class=4)
    assert lo[1, 2] == 9 and io[1, 2] == 30 and (io[[1, 2, 2], [3, 2, 3]] == 1).all()
    assert st == [4, 35 - 4 - 1, 0, fx.CLASS_RANGE]
    region = np.zeros((5, 7), np.uint8)
    region[4, 6] = 3
    lo, io, _, st = fx.erase(label, inst, region=region, fill=(1,), n_class=4)
    assert st[0] == 1 and np.array_equal(lo, label)


def test_oracle_place_is_pillows_nearest_resize_clipped_and_protected():
    src = np.zeros((5, 7), np.int64)
    src[1:4, 2:5] = [[40, 40, 0], [40, 41, 40], [0, 40, 40]]                     # 41: a second instance inside the box
    label = _plane(['2222222'] * 5)
    label[:, 5] = 6
    inst = label.copy()
    lo, io, ch, st, mask = fx.place(label, inst, src, 40, (2, 1, 5, 4), (3, 2, 9, 8), 7, 90, protect=(6,))
    up = np.array([[1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 0, 0], [1, 1, 0, 0, 1, 1],
                   [1, 1, 0, 0, 1, 1], [0, 0, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1]], bool)
    assert np.array_equal(mask, up)                                              # a 2x upscale doubles every pixel
    want = np.zeros((5, 7), bool)
    want[2:5, 3:7] = up[:3, :4]
    blocked = want & (label == 6)
    want &= label != 6
    assert np.array_equal(ch, want.astype(np.uint8)) and (lo[want] == 7).all() and (io[want] == 90).all()
    assert np.array_equal(lo[~want], label[~want]) and st[:2] == [int(want.sum()), int(blocked.sum())]
    assert st[2:] == [3, 2, 6, 4] and blocked.sum() == 2
    _, _, ch, st, _ = fx.place(label, inst, src, 99, (2, 1, 5, 4), (0, 0, 3, 3), 7, 90)
    assert not ch.any() and st == [0, 0] + fx.EMPTY_BOX


# --------------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_library_exports_the_entry_points_with_the_ctypes_signatures():
    from neurips18_hierchical_image_manipulation_amd import _cabi, ops
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        header = f.read()
    for decl in (r'^size_t him_layout_erase_workspace\(int H, int W\);', r'^int him_layout_erase\(', r'^int him_layout_place\(',
                 r'^#define HIM_LAYOUT_NO_SEED 1$', r'^#define HIM_LAYOUT_CLASS_RANGE 2$'):
        assert re.search(decl, header, flags=re.M), decl
    assert os.path.isfile(_cabi.LIB_PATH), 'libhim_hip.so not built'
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    plain = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in ('him_layout_erase_workspace', 'him_layout_erase', 'him_layout_place'):
        assert name in _cabi.EXPORTS and hasattr(dll, name), name
        ret, params = re.search(r'^(\w+) %s\(([^)]*)\);' % name, plain, flags=re.M | re.S).groups()
        res, args = _cabi._SIGS[name]
        assert res is (ctypes.c_size_t if ret == 'size_t' else ctypes.c_int)
        want = []
        for prm in params.split(','):
            prm = ' '.join(prm.split())
            want.append(ctypes.c_void_p if '*' in prm else ctypes.c_size_t if prm.startswith('size_t') else ctypes.c_int)
        assert list(args) == want, name
    assert (ops.LAYOUT_NO_SEED, ops.LAYOUT_CLASS_RANGE) == (fx.NO_SEED, fx.CLASS_RANGE)


def test_library_refuses_bad_arguments_before_any_launch():
    """Nothing below reaches a launch: the addresses are never dereferenced on the host, and every call is refused."""
    from neurips18_hierchical_image_manipulation_amd import _cabi
    dll = _cabi.lib._load()
    ws_fn = dll.him_layout_erase_workspace
    H, W = 64, 96
    need = int(ws_fn(H, W))
    assert need % 16 == 0 and need >= H * W * (1 + 4 + 4) + int(dll.him_edt_workspace(1, H, W))
    for shape in ((0, 8), (8, 0), (-1, 8), (16385, 8), (8, 16385)):
        assert int(ws_fn(*shape)) == 0, shape
    assert int(ws_fn(16384, 16384)) > 0
    p, step = 1 << 24, 1 << 20                          # aligned, non-null, far apart; never read
    order = ['label', 'label_kind', 'inst', 'inst_kind', 'region', 'id', 'H', 'W', 'fill', 'n_class', 'label_out', 'inst_out',
             'changed', 'status', 'ws', 'ws_bytes', 'stream']
    good = dict(label=p, label_kind=3, inst=p + step, inst_kind=1, region=0, id=5, H=H, W=W, fill=p + 2 * step, n_class=35,
                label_out=p + 3 * step, inst_out=p + 4 * step, changed=p + 5 * step, status=p + 6 * step, ws=p + 7 * step,
                ws_bytes=need, stream=0)
    bad = [('label', 0), ('inst', 0), ('fill', 0), ('label_out', 0), ('inst_out', 0), ('changed', 0), ('status', 0),
           ('label_kind', 4), ('inst_kind', -1), ('H', 0), ('W', 16385), ('n_class', 0), ('n_class', 65537),
           ('label', p + 2), ('inst_out', p + 4 * step + 1), ('ws', p + 7 * step + 8),
           ('label_out', p), ('label_out', p + H * W * 4 - 4), ('inst_out', p + step), ('changed', p + 3 * step),
           ('changed', p + step + H * W * 4 - 1), ('region', p + 5 * step)]
    for name, value in bad:
        rc = dll.him_layout_erase(*[dict(good, **{name: value})[k] for k in order])
        assert rc == E_INVALID, (name, value, rc)
        assert b'layout_erase' in dll.him_last_error(), (name, dll.him_last_error())
    for over in (dict(ws=0), dict(ws_bytes=need - 1)):
        assert dll.him_layout_erase(*[dict(good, **over)[k] for k in order]) == E_WORKSPACE, over

    order = ['inst_src', 'inst_kind', 'Hs', 'Ws', 'id', 'sx0', 'sy0', 'sx1', 'sy1', 'xs', 'ys', 'label_dst', 'label_kind',
             'inst_dst', 'Hd', 'Wd', 'dx0', 'dy0', 'dx1', 'dy1', 'cls', 'new_id', 'protect', 'n_class', 'changed', 'status',
             'stream']
    good = dict(inst_src=p, inst_kind=1, Hs=H, Ws=W, id=5, sx0=3, sy0=4, sx1=20, sy1=30, xs=p + step, ys=p + 2 * step,
                label_dst=p + 3 * step, label_kind=0, inst_dst=p + 4 * step, Hd=H, Wd=W, dx0=-5, dy0=-6, dx1=40, dy1=50, cls=7,
                new_id=1005, protect=0, n_class=0, changed=p + 5 * step, status=p + 6 * step, stream=0)
    bad = [('inst_src', 0), ('xs', 0), ('ys', 0), ('label_dst', 0), ('inst_dst', 0), ('status', 0), ('inst_kind', 4),
           ('label_kind', -1), ('Hs', 0), ('Wd', 16385), ('sx0', -1), ('sx1', W + 1), ('sy1', 4), ('sy1', H + 1), ('dx1', -5),
           ('dy1', -7), ('dx0', -(1 << 20) - 1), ('dy1', (1 << 20) + 1), ('cls', 256), ('cls', -1), ('protect', p + 7 * step),
           ('inst_src', p + 1), ('xs', p + step + 2),
           # the aliasing refusal: the source plane is a destination plane, or reaches into one
           ('inst_src', p + 4 * step), ('inst_src', p + 3 * step), ('inst_src', p + 4 * step - 4), ('inst_src', p + 5 * step),
           ('inst_dst', p + 3 * step), ('changed', p + 4 * step + 8)]
    for name, value in bad:
        rc = dll.him_layout_place(*[dict(good, **{name: value})[k] for k in order])
        assert rc == E_INVALID, (name, value, rc)
        assert b'layout_place' in dll.him_last_error(), (name, dll.him_last_error())
    assert dll.him_layout_place(*[dict(good, inst_kind=0, new_id=256)[k] for k in order]) == E_INVALID
    assert dll.him_layout_place(*[dict(good, inst_kind=3, inst_src=p, new_id=(1 << 24) + 1)[k] for k in order]) == E_INVALID
    assert b'overlaps' in (dll.him_layout_place(*[dict(good, inst_src=p + 4 * step)[k] for k in order]),
                           dll.him_last_error())[1]


# ------------------------------------------------------------------------------------------------- wrappers, host side
def test_ops_wrappers_refuse_bad_arguments_before_any_device_work():
    """Every refusal is a ValueError raised on the host: the planes here are host tensors, refused last."""
    from neurips18_hierchical_image_manipulation_amd import ops
    lab = torch.zeros(1, 1, 8, 9)
    erase_bad = [dict(id=None), dict(id=3, region=torch.zeros(8, 9, dtype=torch.uint8)), dict(id=2.0), dict(id=True),
                 dict(id=3, n_class=0), dict(id=3, n_class=65537), dict(id=3, fill=(35,)), dict(id=3, fill=(-1,)),
                 dict(id=3, fill=5), dict(id=3)]
    for kw in erase_bad:
        kw = dict(dict(fill=(1, 2), n_class=35), **kw)
        with pytest.raises(ValueError):
            ops.layout_erase(lab, lab, kw.pop('id'), **kw)
    with pytest.raises(TypeError):
        ops.layout_erase(lab, lab, 3)                                            # fill and n_class are required
    good = dict(id=3, src_box=(0, 0, 4, 4), dst_box=(1, 1, 6, 7), cls=5, new_id=1003)
    place_bad = [dict(id='a'), dict(src_box=(0, 0, 0, 4)), dict(src_box=(0, 0, 4)), dict(dst_box=(5, 1, 5, 7)),
                 dict(dst_box=(0, 0, 1 << 21, 4)), dict(src_box=(0.5, 0, 4, 4)), dict(cls=None), dict(new_id=1.5),
                 dict(protect=(70000,)), dict(protect=3), dict()]
    for kw in place_bad:
        kw = dict(good, **kw)
        with pytest.raises(ValueError):
            ops.layout_place(lab, lab, lab, kw.pop('id'), kw.pop('src_box'), kw.pop('dst_box'), kw.pop('cls'),
                             kw.pop('new_id'), **kw)
    assert list(inspect.signature(ops.layout_erase).parameters) == ['label', 'inst', 'id', 'region', 'fill', 'n_class']
    assert list(inspect.signature(ops.layout_place).parameters) == ['label_dst', 'inst_dst', 'inst_src', 'id', 'src_box',
                                                                    'dst_box', 'cls', 'new_id', 'protect']


def test_joint_inference_keeps_its_methods_and_adds_the_three_edits():
    from neurips18_hierchical_image_manipulation_amd.models import joint_inference_model as jm
    ji = jm.JointInference
    assert list(inspect.signature(ji.gen_image).parameters) == ['self', 'bbox_sampled', 'img_original', 'label_generated',
                                                                'opt']
    lead = ['label_original', 'inst_original', 'img_original', 'opt']
    for name, first in (('remove_object', ['obj']), ('move_object', ['obj', 'dst_box']), ('rescale_object', ['obj', 'scale'])):
        prm = inspect.signature(getattr(ji, name)).parameters
        assert list(prm)[:1 + len(first) + 4] == ['self'] + first + lead, name
    rm = inspect.signature(ji.remove_object).parameters
    for k, default in (('fill', None), ('feather', None), ('reach', 0), ('profile', 'smooth')):
        assert rm[k].kind is inspect.Parameter.KEYWORD_ONLY and rm[k].default == default
    assert jm.edit_object(('1004', {'bbox': [3, 4, 10, 12], 'cls': 26})) == (1004, [3, 4, 10, 12], 26)
    assert jm.edit_object({'id': 7, 'bbox': (3, 4, 10, 12), 'cls': 2}) == (7, [3, 4, 10, 12], 2)
    for bad in (None, ('x', {}), {'bbox': [1, 2, 3, 4], 'cls': 1}, (5, {'bbox': [4, 4, 3, 9], 'cls': 1})):
        with pytest.raises(ValueError):
            jm.edit_object(bad)
    assert jm.scaled_box([10, 20, 19, 39], 1) == [10, 20, 19, 39]
    assert jm.scaled_box([10, 20, 19, 39], 2) == [5, 10, 24, 49]                 # 10 x 20 -> 20 x 40 about (15, 30)
    assert jm.scaled_box([10, 20, 19, 39], 0.5) == [12, 25, 16, 34]
    assert jm.scaled_box([0, 0, 2, 2], 0.01) == [1, 1, 1, 1]
    for bad in (0, -1, float('nan'), float('inf'), 'x', True):
        with pytest.raises(ValueError):
            jm.scaled_box([0, 0, 2, 2], bad)
