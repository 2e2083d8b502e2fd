"""-m gpu: him_layout_erase and him_layout_place at the C ABI inside tests/abi_harness.py's guarded arena, bit for bit
against the brute-force oracle of tests/layout_edit_fixture.py, for every plane kind (uint8 / int32 / int64 / fp32, and
the fp32 label + int32 instance pair the joint edit uses).

Arena: every buffer of a call is a view in ONE allocation between 64 KiB bands; NaN bands beside the inputs, 0xA5 bands
beside outputs, status and workspace, compared bit for bit afterwards; outputs and workspace are pre-filled with 0xFF
bytes, so a pixel the call forgets shows; the inputs are compared with what went in.

Shapes: 1 x 9 and 9 x 1 planes, 37 x 53, and 67 x 261 -- each side just past the transform's blocks (csrc/him_edt.hip:
256 columns per row-pass step, 64 rows per column-pass chunk, 64 x 32 tiles), with regions across those seams."""
import numpy as np
import pytest
import torch

import abi_harness as ah
import layout_edit_fixture as fx
from neurips18_hierchical_image_manipulation_amd import ops
from neurips18_hierchical_image_manipulation_amd.data import resample

pytestmark = pytest.mark.gpu

KINDS = [(0, 0), (1, 1), (2, 2), (3, 3), (3, 1)]                     # (label kind, instance kind)
KIND_IDS = ['u8', 'i32', 'i64', 'f32', 'f32+i32']
SEAM = (67, 261)
N_CLASS = 12
FILL = tuple(range(10))                                              # 10 and 11 are never fillers
OBJ, OTHER = 200, 201                                                # instance ids a uint8 plane holds


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _as_floats(raw):
    raw = raw + b'\xff' * (-len(raw) % 4)
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy().view(np.float32))


def _bytes(view, n):
    return bytes(view.contiguous().view(torch.uint8).cpu().numpy()[:n])


def _out(ar, name, dtype, shape):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer(_bytes(ar.t[name], n), dtype).reshape(shape).copy()


def _finish(lib, ar, rc, expect, raws):
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.him_last_error())
    bad = ar.guard_failures()
    assert not bad, '; '.join(bad)
    for k, raw in raws.items():
        assert _bytes(ar.t[k], len(raw)) == raw, 'input %s was written' % k


# ------------------------------------------------------------------------------------------------------------- erase
def call_erase(label, inst, kinds, id=0, region=None, fill=FILL, n_class=N_CLASS):
    lib = ah.raw_lib()
    lk, ik = kinds
    H, W = label.shape
    lab, ins = label.astype(fx.NP_KINDS[lk]), inst.astype(fx.NP_KINDS[ik])
    raws = {'label': lab.tobytes(), 'inst': ins.tobytes(), 'fill': fx.bit_table(fill, n_class).tobytes()}
    if region is not None:
        raws['region'] = np.ascontiguousarray(region, np.uint8).tobytes()
    specs = {k: ('in', _as_floats(v)) for k, v in raws.items()}
    nws = int(lib.him_layout_erase_workspace(H, W))
    specs.update(label_out=('ws', lab.nbytes), inst_out=('ws', ins.nbytes), changed=('ws', H * W), status=('ws', 16),
                 ws=('ws', nws))
    ar = ah.Arena('cuda', specs)
    rc = lib.him_layout_erase(ar.ptr('label'), lk, ar.ptr('inst'), ik, ar.ptr('region'), id, H, W, ar.ptr('fill'), n_class,
                              ar.ptr('label_out'), ar.ptr('inst_out'), ar.ptr('changed'), ar.ptr('status'), ar.ptr('ws'),
                              nws, _stream())
    _finish(lib, ar, rc, 0, raws)
    return (_out(ar, 'label_out', lab.dtype, (H, W)), _out(ar, 'inst_out', ins.dtype, (H, W)),
            _out(ar, 'changed', np.uint8, (H, W)), _out(ar, 'status', np.int32, (4,)).tolist(), lab, ins)


def _base(shape, seed):
    return fx.canvas(shape[0], shape[1], seed, n_class=10, block=3)


def _obj(label, inst, mask, cls=11, id=OBJ):
    assert mask.any()
    return fx.add_object(label, inst, mask, cls, id)


def case_thin(shape):
    label, inst = _base(shape, 1)
    m = np.zeros(shape, bool)
    m.reshape(-1)[3:6] = True
    return dict(zip(('label', 'inst'), _obj(label, inst, m)), id=OBJ)


def case_borders(shape):
    H, W = shape
    label, inst = _base(shape, 2)
    m = np.zeros(shape, bool)
    m[:H // 2 + 1, :W // 3 + 1] = True                                # the top and the left canvas border
    m &= ~fx.ellipse(H, W, H // 2, W // 3, 4, 5)
    return dict(zip(('label', 'inst'), _obj(label, inst, m)), id=OBJ)


def case_hole(shape):
    H, W = shape
    label, inst = _base(shape, 3)
    cy, cx = (62, 255) if shape == SEAM else (H // 2, W // 2)         # across column 256 and row 64, cut by the border
    m = fx.ellipse(H, W, cy, cx, 12, 15) & ~fx.ellipse(H, W, cy, cx, 4, 6)
    return dict(zip(('label', 'inst'), _obj(label, inst, m)), id=OBJ)


def case_excluded(shape):
    H, W = shape
    label, inst = _base(shape, 4)
    cy, cx = (60, 250) if shape == SEAM else (H // 2, W // 2)
    band = fx.ellipse(H, W, cy, cx, 11, 13)
    label[band], inst[band] = 10, 10                                  # class 10 is not a filler: the fill jumps over it
    other = fx.ellipse(H, W, cy + 9, cx + 8, 3, 3)
    label[other], inst[other] = 11, OTHER                             # nor is a neighbouring object
    return dict(zip(('label', 'inst'), _obj(label, inst, fx.ellipse(H, W, cy, cx, 6, 8))), id=OBJ)


def case_tie(shape):
    H, W = shape
    cy, cx = (61, 255) if shape == SEAM else (H // 2, W // 2)
    label = np.full(shape, 10, np.int64)
    inst = label.copy()
    for k, (dy, dx) in enumerate(((-3, 0), (0, -3), (0, 3), (3, 0), (-5, -5), (5, 5))):
        label[cy + dy, cx + dx] = inst[cy + dy, cx + dx] = 1 + k      # four equidistant seeds of four classes, two more
    m = np.zeros(shape, bool)
    m[cy - 1:cy + 2, cx - 1:cx + 2] = True
    return dict(zip(('label', 'inst'), _obj(label, inst, m)), id=OBJ)


def case_no_seed(shape):
    return dict(case_thin(shape) if min(shape) == 1 else case_hole(shape), fill=())


def case_no_region(shape):
    return dict(case_hole(shape), id=OTHER + 1)


def case_range(shape):
    c = case_excluded(shape)
    H, W = shape
    cy, cx = (60, 250) if shape == SEAM else (H // 2, W // 2)
    c['label'][cy - 2:cy + 1, cx - 20:cx + 1] = 13                    # outside [0, 12): partly in the region, partly not
    c['label'][0, 0] = 12
    return c


def case_region_plane(shape):
    c = case_hole(shape)
    region = (c['inst'] == OBJ).astype(np.uint8) * 7
    region[1, 1:4] = 1
    c['inst'][c['inst'] == OBJ] = 11                                  # the instance plane no longer tells
    return dict(c, region=region, id=0)


ERASE_CASES = [(case_thin, (1, 9)), (case_thin, (9, 1)), (case_no_seed, (1, 9))] + \
    [(f, s) for s in ((37, 53), SEAM) for f in (case_borders, case_hole, case_excluded, case_tie, case_no_seed,
                                                 case_no_region, case_range, case_region_plane)]
_WANT = {}                                                           # the oracle's answer per case, computed once


@pytest.mark.parametrize('kinds', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('case', ERASE_CASES, ids=lambda c: '%s-%dx%d' % (c[0].__name__[5:], c[1][0], c[1][1]))
def test_erase_against_the_oracle(case, kinds):
    build, shape = case
    c = build(shape)
    args = dict(id=c.get('id', 0), region=c.get('region'), fill=c.get('fill', FILL), n_class=N_CLASS)
    key = (build.__name__, shape)
    if key not in _WANT:
        _WANT[key] = fx.erase(c['label'], c['inst'], **args)
    w_label, w_inst, w_changed, w_status = _WANT[key]
    label_out, inst_out, changed, status, lab, ins = call_erase(c['label'], c['inst'], kinds, **args)
    print(key, kinds, 'status', status, 'oracle', w_status)
    assert status == w_status
    assert np.array_equal(label_out, w_label.astype(lab.dtype)) and label_out.dtype == lab.dtype
    assert np.array_equal(inst_out, w_inst.astype(ins.dtype)) and inst_out.dtype == ins.dtype
    assert np.array_equal(changed, w_changed)
    # what each case is about did happen
    name = build.__name__
    if name == 'case_no_seed':
        assert status[3] == fx.NO_SEED and status[1] == 0 and status[0] > 0 and not changed.any()
        assert label_out.tobytes() == lab.tobytes() and inst_out.tobytes() == ins.tobytes()
    elif name == 'case_no_region':
        assert status[0] == 0 and status[3] == 0 and label_out.tobytes() == lab.tobytes()
    elif name == 'case_range':
        assert status[3] == fx.CLASS_RANGE and (label_out[c['label'] >= N_CLASS] == lab[c['label'] >= N_CLASS]).all()
        assert ((c['inst'] == OBJ) & (c['label'] >= N_CLASS)).any()
    elif name == 'case_tie':
        cy, cx = (61, 255) if shape == SEAM else (shape[0] // 2, shape[1] // 2)
        assert label_out[cy, cx] == 1 and label_out[cy + 1, cx] == 4 and label_out[cy, cx + 1] == 3
    else:
        assert status[3] == 0 and status[2] > 0 and not (inst_out == OBJ).any() if 'region' not in c else status[2] > 0
    if name == 'case_excluded':
        assert not np.isin(label_out[c['inst'] == OBJ], (10, 11)).any()


# ------------------------------------------------------------------------------------------------------------- place
def call_place(c, kinds, alias=None, expect=0):
    lib = ah.raw_lib()
    lk, ik = kinds
    lab, ins = c['label'].astype(fx.NP_KINDS[lk]), c['inst'].astype(fx.NP_KINDS[ik])
    src = c['src'].astype(fx.NP_KINDS[ik])
    (Hs, Ws), (Hd, Wd) = src.shape, lab.shape
    sx0, sy0, sx1, sy1 = c['src_box']
    dx0, dy0, dx1, dy1 = c['dst_box']
    protect = c.get('protect', ())
    n_class = max(protect) + 1 if protect else 0
    raws = {'src': src.tobytes(), 'xs': np.ascontiguousarray(resample.nearest_table(sx1 - sx0, dx1 - dx0), np.int32).tobytes(),
            'ys': np.ascontiguousarray(resample.nearest_table(sy1 - sy0, dy1 - dy0), np.int32).tobytes()}
    if protect:
        raws['protect'] = fx.bit_table(protect, n_class).tobytes()
    specs = {k: ('in', _as_floats(v)) for k, v in raws.items()}
    specs.update(label=('ws', lab.nbytes), inst=('ws', ins.nbytes), changed=('ws', Hd * Wd), status=('ws', 24))
    ar = ah.Arena('cuda', specs)
    for name, a in (('label', lab), ('inst', ins), ('changed', np.zeros((Hd, Wd), np.uint8))):
        ar.t[name][:a.nbytes].copy_(torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()))
    rc = lib.him_layout_place(ar.ptr(alias or 'src'), ik, Hs, Ws, c['id'], sx0, sy0, sx1, sy1, ar.ptr('xs'), ar.ptr('ys'),
                              ar.ptr('label'), lk, ar.ptr('inst'), Hd, Wd, dx0, dy0, dx1, dy1, c['cls'], c['new_id'],
                              ar.ptr('protect'), n_class, ar.ptr('changed'), ar.ptr('status'), _stream())
    _finish(lib, ar, rc, expect, raws)
    status = _out(ar, 'status', np.int32, (6,))
    if expect != 0:
        assert (status.view(np.uint8) == ah.NAN_BYTE).all()          # a refused call wrote nothing, not even the status
        assert _bytes(ar.t['label'], lab.nbytes) == lab.tobytes() and _bytes(ar.t['inst'], ins.nbytes) == ins.tobytes()
        return None
    return (_out(ar, 'label', lab.dtype, (Hd, Wd)), _out(ar, 'inst', ins.dtype, (Hd, Wd)),
            _out(ar, 'changed', np.uint8, (Hd, Wd)), status.tolist())


def _source(shape, box, seed):
    """An instance plane with object OBJ inside ``box`` [x0, y0, x1, y1) and a second instance OTHER across it."""
    H, W = shape
    x0, y0, x1, y1 = box
    _, inst = _base(shape, seed)
    g = np.random.default_rng(seed)
    blob = np.zeros(shape, bool)
    blob[y0:y1, x0:x1] = g.random((y1 - y0, x1 - x0)) < 0.7
    blob[y0, x0:x1] = blob[y1 - 1, x0:x1] = True
    inst[blob] = OBJ
    second = np.zeros(shape, bool)
    if y1 - y0 > 1:
        second[y0 + (y1 - y0) // 2, x0:x1] = True
    else:
        second[y0:y1, x0 + (x1 - x0) // 2] = True
    inst[second] = OTHER                                             # inside the box, must not be copied
    return inst


def _place_case(dst_shape, src_shape, src_box, dst_box, seed, protect=()):
    label, inst = _base(dst_shape, seed + 50)
    if protect:
        label[:, dst_shape[1] // 2 - 1:dst_shape[1] // 2 + 2] = protect[0]   # a protected stripe across the destination
        inst[:] = label
    return dict(label=label, inst=inst, src=_source(src_shape, src_box, seed), id=OBJ, src_box=src_box, dst_box=dst_box,
                cls=11, new_id=150, protect=protect)


PLACE_CASES = {
    'up-2.6x2.4': _place_case((37, 53), (37, 53), (5, 6, 16, 13), (12, 9, 41, 26), 1),
    'down-0.4': _place_case((37, 53), (67, 261), (200, 20, 231, 43), (20, 10, 33, 19), 2),
    'clipped-top-left': _place_case((37, 53), (37, 53), (5, 6, 16, 13), (-9, -6, 20, 11), 3),
    'clipped-bottom-right': _place_case(SEAM, (37, 53), (3, 3, 30, 30), (240, 50, 283, 91), 4),
    'protected': _place_case((37, 53), (37, 53), (5, 6, 16, 13), (12, 9, 41, 26), 5, protect=(6,)),
    'one-pixel-wide': _place_case((37, 53), (37, 53), (7, 4, 8, 21), (30, 2, 37, 35), 6),
    'tile-seam': _place_case(SEAM, SEAM, (100, 10, 171, 41), (30, 20, 131, 60), 7, protect=(3,)),
    'thin-1x9': _place_case((1, 9), (1, 9), (2, 0, 5, 1), (1, 0, 8, 1), 8),
    'thin-9x1': _place_case((9, 1), (9, 1), (0, 2, 1, 5), (0, 1, 1, 8), 9),
    'outside': _place_case((37, 53), (37, 53), (5, 6, 16, 13), (60, 9, 80, 26), 10),
}
_PLACE_WANT = {}


@pytest.mark.parametrize('kinds', KINDS, ids=KIND_IDS)
@pytest.mark.parametrize('name', list(PLACE_CASES))
def test_place_against_the_oracle(name, kinds):
    c = PLACE_CASES[name]
    if name not in _PLACE_WANT:
        _PLACE_WANT[name] = fx.place(c['label'], c['inst'], c['src'], c['id'], c['src_box'], c['dst_box'], c['cls'],
                                     c['new_id'], c['protect'])
    w_label, w_inst, w_changed, w_status, mask = _PLACE_WANT[name]
    label_out, inst_out, changed, status = call_place(c, kinds)
    print(name, kinds, 'status', status, 'oracle', w_status, 'mask pixels', int(mask.sum()))
    assert status == w_status
    assert np.array_equal(label_out, w_label.astype(label_out.dtype))
    assert np.array_equal(inst_out, w_inst.astype(inst_out.dtype))
    assert np.array_equal(changed, w_changed)
    sx0, sy0, sx1, sy1 = c['src_box']
    assert (c['src'][sy0:sy1, sx0:sx1] == OTHER).any() and not (inst_out == OTHER).any()
    if name == 'outside':
        assert status == [0, 0] + fx.EMPTY_BOX and label_out.tobytes() == c['label'].astype(label_out.dtype).tobytes()
        return
    assert status[0] > 0 and status[0] + status[1] <= int(mask.sum())
    if name.startswith('clipped'):
        assert status[0] + status[1] < int(mask.sum())               # part of the mask fell off the canvas
    elif not c['protect']:
        assert status[0] == int(mask.sum())                          # Pillow's own pixel count
    if c['protect']:
        assert status[1] > 0 and (label_out[c['label'] == c['protect'][0]] == c['protect'][0]).all()
    # the reported box is the row inst_summary builds from the result
    rows = ops.inst_summary(torch.from_numpy(inst_out.astype(np.int32)).cuda(), torch.from_numpy(label_out.astype(np.int32)).cuda(),
                            min_id=c['new_id'])
    assert rows.shape[0] == 1 and rows[0].tolist() == [c['new_id']] + status[2:6] + [status[0], c['cls']]


@pytest.mark.parametrize('kinds', KINDS, ids=KIND_IDS)
def test_place_refuses_a_source_that_is_a_destination_plane(kinds):
    c = dict(PLACE_CASES['up-2.6x2.4'])
    assert call_place(c, kinds, alias='inst', expect=ah.E_INVALID) is None
    assert b'overlaps' in ah.raw_lib().him_last_error()
