"""gpu: the ADE20K segmentation decode on the device against the reference's files (tests/golden/preprocess_ade.json and
.npz, written by the live reference from tests/preprocess_ade_fixture.py) and, for shapes the reference was not run on,
against the fixture's numpy restatement (which tests/golden/make_golden_preprocess_ade.py checked against the reference
on every golden case).  Integer results: every comparison is for equality.  The C-ABI calls run inside
tests/abi_harness.py's guarded arena: guard bands in front of and behind the input, every output and the workspace."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import abi_harness as ah
import data_fixture
import preprocess_ade_fixture as fx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'preprocess_ade.json')) as _f:
    GOLD = json.load(_f)
PLANES = np.load(os.path.join(ROOT, 'tests', 'golden', 'preprocess_ade.npz'))
CASES = fx.golden_cases()
NAMES = fx.objectnames()
FILL = 0xFF                                                  # ah.NAN_BYTE: what the arena leaves in a fresh buffer


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _prefix(i):
    return 'bedroom_%05d' % (i + 1)


def _check_binding(seg):
    """``ops.ade_decode`` with and without the class plane equals the restatement; returns the restatement."""
    from neurips18_hierchical_image_manipulation_amd import ops
    cls, label, inst, rows = fx.restate(seg)
    got_label, got_inst, got_rows = ops.ade_decode(_dev(seg), fx.KEEP)
    assert got_rows.dtype == np.int32 and got_rows.shape == rows.shape, (got_rows.shape, rows.shape)
    assert np.array_equal(got_rows, rows)
    assert got_label.dtype == torch.uint8 and got_label.is_cuda and np.array_equal(got_label.cpu().numpy(), label)
    assert got_inst.dtype == torch.uint8 and np.array_equal(got_inst.cpu().numpy(), inst)
    l2, i2, r2, c2 = ops.ade_decode(_dev(seg), fx.KEEP, want_cls=True)
    assert c2.dtype == torch.uint16 and np.array_equal(c2.cpu().numpy(), cls)
    assert torch.equal(l2, got_label) and torch.equal(i2, got_inst) and np.array_equal(r2, rows)
    return cls, label, inst, rows


class Guarded(object):
    """The images, their outputs, keep, status, table and workspace of him_ade_decode calls in ONE guarded allocation.
    Every image has output planes of exactly its own size, so a write one pixel past a plane lands in a band.  ``shift``
    moves the base of ``seg`` by that many BYTES off its 256-byte aligned start (the element path)."""

    def __init__(self, images, shift=0, keep=fx.KEEP):
        self.lib = ah.raw_lib()
        self.nws = int(self.lib.him_ade_decode_workspace())
        self.images = {k: np.ascontiguousarray(v) for k, v in images.items()}
        self.shift, self.keep = shift, list(keep)
        specs = {}
        for name, a in self.images.items():
            px = a.shape[0] * a.shape[1]
            specs['seg_' + name] = ('ws', a.nbytes + shift)
            specs['cls_' + name] = ('ws', 2 * px)
            specs['label_' + name] = ('ws', px)
            specs['inst_' + name] = ('ws', px)
        specs['keep'] = ('ws', 2 * max(len(self.keep), 1))
        specs['status'] = ('ws', 8)
        specs['table'] = ('ws', 256 * 7 * 4)
        specs['ws'] = ('ws', self.nws)
        self.ar = ah.Arena('cuda', specs)
        for name, a in self.images.items():
            self.ar.t['seg_' + name][shift:shift + a.nbytes].copy_(torch.from_numpy(a.reshape(-1)))
        if self.keep:
            self.ar.t['keep'].copy_(torch.from_numpy(np.array(self.keep, np.uint16).view(np.uint8)))

    def call(self, name, want_cls=True):
        """Returns (rc, status (2,), table (256, 7), cls or None, label, inst); asserts the bands and the input."""
        a, ar = self.images[name], self.ar
        H, W, pb = a.shape
        for out in ('cls_', 'label_', 'inst_'):
            ar.t[out + name].fill_(FILL)
        ar.t['table'].fill_(FILL)                            # rows the call does not write read as -1
        ar.t['status'].fill_(FILL)
        rc = self.lib.him_ade_decode(ar.ptr('seg_' + name) + self.shift, H, W, pb, ar.ptr('keep'), len(self.keep),
                                     ar.ptr('cls_' + name) if want_cls else 0, ar.ptr('label_' + name),
                                     ar.ptr('inst_' + name), ar.ptr('status'), ar.ptr('table'), ar.ptr('ws'), self.nws,
                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        bad = ar.guard_failures()
        assert not bad, '; '.join(bad)
        for other, b in self.images.items():                 # the inputs are read, never written
            assert bytes(ar.t['seg_' + other][self.shift:self.shift + b.nbytes].cpu().numpy()) == b.tobytes(), other
        raw_cls = ar.t['cls_' + name].cpu().numpy()
        if not want_cls:
            assert (raw_cls == FILL).all(), 'cls_out was NULL, yet the class plane of the arena was written'
        status = ar.t['status'].cpu().numpy().view(np.int32)
        table = ar.t['table'].cpu().numpy().view(np.int32).reshape(256, 7)
        return (rc, status, table, raw_cls.view(np.uint16).reshape(H, W) if want_cls else None,
                ar.t['label_' + name].cpu().numpy().reshape(H, W), ar.t['inst_' + name].cpu().numpy().reshape(H, W))

    def check(self, name, want_cls=True):
        """One call against the restatement of the image (with this arena's keep list)."""
        rc, status, table, cls, label, inst = self.call(name, want_cls)
        assert rc == 0, self.lib.him_last_error()
        w_cls, w_label, w_inst, w_rows = fx.restate(self.images[name], self.keep)
        n = int(status[0])
        assert n == len(w_rows) and int(status[1]) == 0, (name, status)
        assert (table[n:] == -1).all(), 'rows behind the last rank were written'
        assert np.array_equal(table[:n], w_rows), name
        assert np.array_equal(label, w_label) and np.array_equal(inst, w_inst), name
        if want_cls:
            assert np.array_equal(cls, w_cls), name
        return table[:n].tobytes() + label.tobytes() + inst.tobytes()


def test_every_golden_case_through_the_binding_equals_the_reference():
    from neurips18_hierchical_image_manipulation_amd import preprocess_ade
    for i, (tag, seg, lines) in enumerate(CASES):
        cls, label, inst, rows = _check_binding(seg)
        assert np.array_equal(label, PLANES['label_' + _prefix(i)]) and np.array_equal(inst, PLANES['inst_' + _prefix(i)])
        info = preprocess_ade.rows_to_info(seg.shape[0], seg.shape[1], rows, fx.names_of(lines), NAMES, image=tag)
        assert json.dumps(info) == GOLD['json'][_prefix(i)], tag
    assert len(fx.restate(CASES[4][1])[3]) == 256            # case c: the full table went through


def test_convert_writes_the_reference_files(tmp_path):
    from neurips18_hierchical_image_manipulation_amd import preprocess_ade
    root = str(tmp_path / 'ade20k')
    listed = fx.write_raw_tree(root, CASES)
    assert preprocess_ade.convert(root) == len(CASES)
    for folder, names in GOLD['files'].items():
        assert sorted(os.listdir(os.path.join(root, folder))) == names, folder
    for i, (jpg, seg, lines) in enumerate(listed):
        p = _prefix(i)
        with open(os.path.join(root, 'val_bbox', p + '_gtFine_instanceIds.json'), 'rb') as f:
            assert f.read() == GOLD['json'][p].encode(), p
        for sub, suf, key in (('val_label', '_gtFine_labelIds.png', 'label_'), ('val_inst', '_gtFine_instanceIds.png', 'inst_')):
            with Image.open(os.path.join(root, sub, p + suf)) as im:
                assert im.mode == 'L' and np.array_equal(np.array(im), PLANES[key + p]), (sub, p)
        with open(jpg, 'rb') as f, open(os.path.join(root, 'val_img', p + '_leftImg8bit.png'), 'rb') as g:
            assert f.read() == g.read()


def test_main_converts_with_the_default_split(tmp_path, capsys):
    from neurips18_hierchical_image_manipulation_amd import preprocess_ade
    root = str(tmp_path / 'ade20k')
    fx.write_raw_tree(root, CASES[:2])
    preprocess_ade.main(['--dataroot', root])
    assert 'converted 2 images' in capsys.readouterr().out
    assert sorted(os.listdir(os.path.join(root, 'val_bbox'))) == GOLD['files']['val_bbox'][:2]
    assert os.listdir(os.path.join(root, 'train_bbox')) == []


@pytest.mark.parametrize('shape', [(1, 1), (1, 67), (67, 1)])
def test_degenerate_shapes_equal_the_restatement(shape):
    seg, _ = fx.synth(61, shape[0], shape[1], 3, min_side=1)
    _check_binding(seg)
    Guarded({'a': seg}).check('a')


def test_one_instance_covering_the_plane():
    """64 x 512 under one B value: every wave takes the whole-wave update."""
    rng = np.random.RandomState(62)
    seg = np.zeros((64, 512, 3), np.uint8)
    fx.paint(seg, rng, np.ones((64, 512), bool), fx.KEEP[2], 9)
    rows = _check_binding(seg)[3]
    assert np.array_equal(rows, [[0, 9, 0, 0, 511, 63, 64 * 512]])
    Guarded({'a': seg}).check('a')


def test_ade_sized_image_equals_the_restatement():
    seg, lines = fx.synth(63, 512, 683, 40, kinds='ellipse')
    rows = _check_binding(seg)[3]
    assert len(rows) >= 30 and int(rows[1:, 6].max()) > 64 * 16 * 4
    Guarded({'a': seg}).check('a')


def test_raw_call_in_guarded_buffers_with_and_without_the_class_plane():
    g = Guarded({'a': CASES[1][1], 'c': CASES[4][1]})
    with_cls = g.check('a', want_cls=True)
    without = g.check('a', want_cls=False)                   # asserts the class plane of the arena stays untouched
    assert with_cls == without
    g.check('c', want_cls=False)                             # 256 ranks: the whole table
    g.check('c', want_cls=True)
    assert len(fx.restate(CASES[1][1])[3]) < 8               # ... and 'a' leaves all rows but a few untouched (checked)
    # an empty keep list, and one that repeats an entry (the C ABI takes the first position; the binding refuses it)
    Guarded({'a': CASES[1][1]}, keep=[]).check('a')
    rc, status, table, cls, label, inst = Guarded({'a': CASES[0][1]}, keep=[165, fx.KEEP[0], 165, fx.KEEP[0]]).call('a')
    assert rc == 0 and (label[cls == fx.KEEP[0]] == 2).all() and (label[cls == 165] == 1).all()
    assert (cls == fx.KEEP[0]).any() and (label[(cls != fx.KEEP[0]) & (cls != 165)] == 0).all()


def test_four_byte_pixels():
    from neurips18_hierchical_image_manipulation_amd import ops
    rng = np.random.RandomState(64)
    for tag, seg, _ in CASES[:4]:
        rgba = np.concatenate([seg, rng.randint(0, 256, seg.shape[:2] + (1,)).astype(np.uint8)], axis=2)
        cls, label, inst, rows = fx.restate(seg)
        got = ops.ade_decode(_dev(rgba), fx.KEEP, want_cls=True)
        assert np.array_equal(got[0].cpu().numpy(), label) and np.array_equal(got[1].cpu().numpy(), inst), tag
        assert np.array_equal(got[2], rows) and np.array_equal(got[3].cpu().numpy(), cls), tag
        for shift in (0, 1):
            Guarded({'a': rgba}, shift=shift).check('a')


@pytest.mark.parametrize('width', [1, 15, 16, 17, 67])
def test_widths_around_the_group_size_on_both_paths(width):
    """Aligned bases take whole 16-pixel groups as 16-byte words and the last partial group byte by byte; a base shifted
    by one byte takes every pixel byte by byte.  Both give the same bytes."""
    seg, _ = fx.synth(65 + width, 9, width, 4, min_side=1)
    aligned = Guarded({'a': seg}).check('a')
    shifted = Guarded({'a': seg}, shift=1).check('a')
    assert aligned == shifted
    _check_binding(seg)


def test_base_shifted_by_one_byte_through_the_binding():
    from neurips18_hierchical_image_manipulation_amd import ops
    tag, seg, _ = CASES[2]
    flat = torch.zeros(seg.size + 1, dtype=torch.uint8, device='cuda')
    view = flat[1:].view(seg.shape)
    view.copy_(_dev(seg))
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    cls, label, inst, rows = fx.restate(seg)
    got = ops.ade_decode(view, fx.KEEP, want_cls=True)
    assert np.array_equal(got[0].cpu().numpy(), label) and np.array_equal(got[1].cpu().numpy(), inst)
    assert np.array_equal(got[2], rows) and np.array_equal(got[3].cpu().numpy(), cls)
    with pytest.raises(ValueError, match='ade_decode: seg must be a contiguous'):
        ops.ade_decode(_dev(seg)[:, ::2], fx.KEEP)
    with pytest.raises(ValueError, match='ade_decode: seg is torch.int32'):
        ops.ade_decode(_dev(seg).to(torch.int32), fx.KEEP)


def test_one_workspace_serves_different_images_in_any_order():
    a, b = CASES[0][1], CASES[4][1]                          # 37 x 301 with 6 ranks, 16 x 16 with 256
    assert a.shape != b.shape
    g = Guarded({'a': a, 'b': b})
    for order in ('ab', 'ba', 'aab'):
        for which in order:
            g.check(which)


def test_same_image_three_times_gives_identical_bytes():
    seg, _ = fx.synth(66, 200, 333, 30, kinds='ellipse')
    g = Guarded({'a': seg})
    runs = [g.check('a') for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


def test_loadAde20K_and_ade_info_equal_the_files(tmp_path):
    from neurips18_hierchical_image_manipulation_amd import preprocess_ade
    listed = fx.write_raw_tree(str(tmp_path), CASES)
    for i, (jpg, seg, lines) in enumerate(listed):
        om, oi, objects = preprocess_ade.loadAde20K(jpg)
        cls = fx.restate(seg)[0]
        assert om.is_cuda and om.dtype == torch.uint16 and np.array_equal(om.cpu().numpy(), cls)
        assert oi.is_cuda and np.array_equal(oi.cpu().numpy(), PLANES['inst_' + _prefix(i)])
        assert objects['class'] == fx.names_of(lines)
        assert objects['instancendx'] == [n for n, level, _ in lines if level == 0]
        assert sorted(objects) == ['class', 'corrected_raw_name', 'instancendx', 'iscrop', 'listattributes']
        info = preprocess_ade.ade_info(_dev(seg), fx.names_of(lines), NAMES)
        assert info == json.loads(GOLD['json'][_prefix(i)]) and json.dumps(info) == GOLD['json'][_prefix(i)]


def test_converted_tree_opens_through_the_loader(tmp_path):
    from neurips18_hierchical_image_manipulation_amd import preprocess_ade
    from neurips18_hierchical_image_manipulation_amd.data.data_loader import CreateDataLoader
    from neurips18_hierchical_image_manipulation_amd.options import MaskToImageTrainOptions
    root = str(tmp_path / 'ade20k')
    cases = fx.loader_cases()
    fx.write_raw_tree(root, cases)
    assert preprocess_ade.convert(root, n_val=1) == 4
    for sub in ('img', 'label', 'inst', 'bbox'):
        assert len(os.listdir(os.path.join(root, 'train_' + sub))) == 3 and len(os.listdir(os.path.join(root, 'val_' + sub))) == 1
    for i, (tag, seg, lines) in enumerate(cases):
        phase = 'val' if i == 0 else 'train'
        with open(os.path.join(root, phase + '_bbox', _prefix(i) + '_gtFine_instanceIds.json')) as f:
            info = json.load(f)
        assert info == fx.rows_to_info(seg.shape[0], seg.shape[1], fx.restate(seg)[3], fx.names_of(lines), NAMES)
        boxes = [o['bbox'] for o in info['objects'].values()]
        assert boxes and all(b[2] - b[0] >= 16 and b[3] - b[1] >= 16 for b in boxes), tag
    argv = data_fixture.loader_argv(root, 'ade', 64, ['--contextMargin', '2.0', '--min_box_size', '16',
                                                       '--max_box_size', '64'])
    opt = MaskToImageTrainOptions().parse(save=False, default_args=argv)
    loader = CreateDataLoader(opt)
    assert len(loader) == 3
    batches = list(loader.load_data())
    assert [int(b['image'].shape[0]) for b in batches] == [2, 1]
    for b in batches:
        assert b['image'].is_cuda and tuple(b['image'].shape[1:]) == (3, 64, 64)
        assert tuple(b['label'].shape)[0] == b['image'].shape[0] and bool(torch.isfinite(b['image']).all())
        assert bool(torch.isfinite(b['label']).all())
