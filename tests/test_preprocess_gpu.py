"""gpu: the instance-box summary on the device against the reference's files (tests/golden/preprocess_city.json, written
by the live reference from tests/preprocess_fixture.py) and, at full size, against the fixture's numpy restatement (which
tests/golden/make_golden_preprocess.py checked against the reference on every fixture pair).  Integer results: every
comparison is for equality.  The C-ABI calls run inside tests/abi_harness.py's guarded arena: guard bands in front of and
behind both planes, the status record, the table and the workspace."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import abi_harness as ah
import data_fixture
import preprocess_fixture as fx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'preprocess_city.json')) as _f:
    GOLD = json.load(_f)

OVERFLOW, ID_RANGE, CLS_RANGE = 1, 2, 4
INST_KIND = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.int16): 1, np.dtype(np.int32): 2,
             np.dtype(np.int64): 3}
CLS_KIND = {np.dtype(np.uint8): 0, np.dtype(np.int32): 1, np.dtype(np.int64): 2, np.dtype(np.float32): 3}


def _pairs():
    return [(c + '/' + s, i, l) for c, s, i, l in fx.pairs()]


def _golden_rows(stem):
    """(n, 6) id, xmin, ymin, xmax, ymax, cls of a golden file, in file order."""
    objects = json.loads(GOLD[stem + '_gtFine_instanceIds'])['objects']
    return np.array([[int(k)] + v['bbox'] + [v['cls']] for k, v in objects.items()], dtype=np.int64).reshape(-1, 6)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded(object):
    """Planes, status, table and workspace of one or more him_inst_summary calls in ONE guarded allocation.  ``shift``
    moves a plane's base by that many ELEMENTS off its 256-byte aligned start (the element path)."""

    def __init__(self, planes, max_objects, shift=0):
        self.lib = ah.raw_lib()
        self.max_objects = max_objects
        self.nws = int(self.lib.him_inst_summary_workspace(8, 8, max_objects))
        specs, self.planes = {}, {}
        for name, a in planes.items():
            a = np.ascontiguousarray(a)
            specs[name] = ('ws', a.nbytes + shift * a.itemsize)
            self.planes[name] = (a, shift * a.itemsize)
        specs['status'] = ('ws', 8)
        specs['table'] = ('ws', max_objects * 7 * 4)
        specs['ws'] = ('ws', self.nws)
        self.ar = ah.Arena('cuda', specs)
        for name, (a, off) in self.planes.items():
            self.ar.t[name][off:off + a.nbytes].copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))

    def call(self, inst, cls, min_id=1000):
        """Returns (rc, count, flags, table (max_objects, 7) int32 as it stands); asserts the bands."""
        (ia, ioff), (ca, coff) = self.planes[inst], self.planes[cls]
        H, W = ia.shape
        ar = self.ar
        ar.t['table'].fill_(0xFF)                            # rows the call does not write read as -1
        rc = self.lib.him_inst_summary(ar.ptr(inst) + ioff, INST_KIND[ia.dtype], ar.ptr(cls) + coff, CLS_KIND[ca.dtype],
                                       H, W, min_id, self.max_objects, ar.ptr('status'), ar.ptr('table'), ar.ptr('ws'),
                                       self.nws, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        bad = ar.guard_failures()
        assert not bad, '; '.join(bad)
        for name, (a, off) in self.planes.items():          # the inputs are read, never written
            assert bytes(ar.t[name][off:off + a.nbytes].cpu().numpy()) == a.tobytes(), name
        status = ar.t['status'].cpu().numpy().view(np.int32)
        table = ar.t['table'].cpu().numpy().view(np.int32).reshape(self.max_objects, 7)
        return rc, int(status[0]), int(status[1]), table

    def rows(self, inst, cls, min_id=1000):
        rc, count, flags, table = self.call(inst, cls, min_id)
        assert rc == 0, self.lib.him_last_error()
        assert flags == 0 and count <= self.max_objects, (count, flags)
        assert (table[count:] == -1).all(), 'rows behind the last object were written'
        return table[:count].astype(np.int64)


def _inst_variants(inst):
    out = [inst.astype(np.int32), inst.astype(np.int64)]
    if inst.dtype == np.uint8:
        out.insert(0, inst)
    out += [inst.astype(np.uint16), inst.astype(np.uint16).view(np.int16)]      # int16 bits are read as unsigned
    return out


def _cls_variants(label):
    return [label, label.astype(np.int32), label.astype(np.int64), label.astype(np.float32)]


@pytest.mark.parametrize('index', range(7))
def test_every_fixture_pair_equals_the_reference_for_every_input_kind(index):
    from neurips18_hierchical_image_manipulation_amd import ops
    name, inst, label = _pairs()[index]
    want = _golden_rows(os.path.basename(name))
    full = fx.restate(inst, label)
    assert np.array_equal(full[:, [0, 1, 2, 3, 4, 6]], want)
    seen = set()
    for iv in _inst_variants(inst):
        for cv in _cls_variants(label):
            got = ops.inst_summary(_dev(iv), _dev(cv))
            assert got.dtype == np.int32 and got.shape == (len(want), 7), (iv.dtype, cv.dtype, got.shape)
            assert np.array_equal(got, full), (name, iv.dtype, cv.dtype)
            seen.add((iv.dtype, cv.dtype))
    assert len(seen) >= 16
    if inst.dtype == np.uint8:                               # ADE-style planes: small ids, a lower threshold
        low = fx.restate(inst, label, min_id=100)
        assert len(low) == 2
        assert np.array_equal(ops.inst_summary(_dev(inst), _dev(label), min_id=100), low)
        assert np.array_equal(ops.inst_summary(_dev(inst), _dev(label), min_id=0), fx.restate(inst, label, min_id=0))


def test_full_size_pair_equals_the_restatement():
    from neurips18_hierchical_image_manipulation_amd import ops
    inst, label = fx.synth_pair(21, 1024, 2048, 90)
    want = fx.restate(inst, label)
    assert len(want) >= 60 and int(want[:, 5].max()) > 64 * 8 * 4
    assert np.array_equal(ops.inst_summary(_dev(inst), _dev(label)), want)
    g = Guarded({'inst': inst, 'cls': label}, max_objects=128)
    assert np.array_equal(g.rows('inst', 'cls'), want)
    # a plane that is one object: every wave takes the whole-wave update
    one = np.full((64, 512), 26007, np.uint16)
    assert np.array_equal(ops.inst_summary(_dev(one), _dev(np.full((64, 512), 26, np.uint8))),
                          np.array([[26007, 0, 0, 511, 63, 64 * 512, 26]]))


@pytest.mark.parametrize('index', [0, 1, 3, 4, 6])
def test_element_path_misaligned_bases_and_odd_widths(index):
    name, inst, label = _pairs()[index]
    want = fx.restate(inst, label)
    for shift in (0, 1):
        for iv, cv in ((inst, label), (inst.astype(np.int32), label.astype(np.float32)),
                       (inst.astype(np.int64), label.astype(np.int64))):
            g = Guarded({'inst': iv, 'cls': cv}, max_objects=64, shift=shift)
            assert np.array_equal(g.rows('inst', 'cls'), want), (name, shift, iv.dtype)


def test_misaligned_view_through_the_binding():
    from neurips18_hierchical_image_manipulation_amd import ops
    _, inst, label = _pairs()[0]
    H, W = inst.shape
    assert W % 8 == 0
    flat_i = torch.zeros(H * W + 1, dtype=torch.int16, device='cuda')      # 16 bits, read as unsigned
    flat_c = torch.zeros(H * W + 1, dtype=torch.uint8, device='cuda')
    vi, vc = flat_i[1:].view(H, W), flat_c[1:].view(H, W)
    vi.copy_(_dev(inst.view(np.int16)))
    vc.copy_(_dev(label))
    assert vi.data_ptr() % 16 != 0 and vi.is_contiguous()
    assert np.array_equal(ops.inst_summary(vi, vc), fx.restate(inst, label))
    assert np.array_equal(ops.inst_summary(vi, _dev(label)), fx.restate(inst, label))


def test_one_workspace_serves_different_images_in_any_order():
    a_inst, a_cls = fx.synth_pair(31, 96, 160, 30)
    b_inst, b_cls = fx.synth_pair(32, 50, 383, 40)
    want_a, want_b = fx.restate(a_inst, a_cls), fx.restate(b_inst, b_cls)
    assert len(want_a) != len(want_b) and set(want_a[:, 0]) != set(want_b[:, 0])
    g = Guarded({'ai': a_inst, 'ac': a_cls, 'bi': b_inst, 'bc': b_cls}, max_objects=64)
    for order in ('ab', 'ba', 'aab', 'bba'):
        for which in order:
            got = g.rows(which + 'i', which + 'c')
            assert np.array_equal(got, want_a if which == 'a' else want_b), (order, which)


def test_same_image_twice_gives_identical_bytes():
    inst, label = fx.synth_pair(33, 256, 512, 60)
    g = Guarded({'inst': inst, 'cls': label}, max_objects=96)
    runs = []
    for _ in range(3):
        rc, count, flags, table = g.call('inst', 'cls')
        assert rc == 0 and flags == 0
        runs.append((count, table.tobytes()))
    assert runs[0] == runs[1] == runs[2]
    assert np.array_equal(np.frombuffer(runs[0][1], np.int32).reshape(-1, 7)[:runs[0][0]], fx.restate(inst, label))


def test_overflow_and_values_outside_the_domains_raise():
    from neurips18_hierchical_image_manipulation_amd import ops
    _, inst, label = _pairs()[0]
    n = len(fx.restate(inst, label))
    with pytest.raises(ValueError, match='max_objects=5'):
        ops.inst_summary(_dev(inst), _dev(label), max_objects=5)
    assert len(ops.inst_summary(_dev(inst), _dev(label), max_objects=n)) == n          # exactly full is not an overflow
    wide = inst.astype(np.int32)
    wide[3, 5] = 70000
    with pytest.raises(ValueError, match='instance id outside'):
        ops.inst_summary(_dev(wide), _dev(label))
    neg = inst.astype(np.int64)
    neg[0, 0] = -1
    with pytest.raises(ValueError, match='instance id outside'):
        ops.inst_summary(_dev(neg), _dev(label))
    for bad_cls in (label.astype(np.int32), label.astype(np.float32)):
        bad_cls = bad_cls.copy()
        bad_cls[7, 9] = 256 if bad_cls.dtype == np.int32 else 3.5
        with pytest.raises(ValueError, match='class value outside'):
            ops.inst_summary(_dev(inst), _dev(bad_cls))
    assert np.array_equal(ops.inst_summary(_dev(inst), _dev(label)), fx.restate(inst, label))   # the cache is unharmed
    # the same through the guarded arena: the status bits, and nothing outside the table is written
    g = Guarded({'inst': inst, 'cls': label, 'wide': wide}, max_objects=5)
    rc, count, flags, _ = g.call('inst', 'cls')
    assert rc == 0 and count == n and flags == OVERFLOW
    rc, count, flags, _ = g.call('wide', 'cls')
    assert rc == 0 and flags & ID_RANGE and flags & OVERFLOW
    g = Guarded({'inst': inst, 'cls': label, 'wide': wide}, max_objects=64)
    rc, count, flags, _ = g.call('wide', 'cls')
    assert rc == 0 and flags == ID_RANGE
    assert np.array_equal(g.rows('inst', 'cls'), fx.restate(inst, label))               # and the next call is clean


def test_construct_box_writes_the_reference_bytes(tmp_path, capsys):
    from neurips18_hierchical_image_manipulation_amd import preprocess
    src, dst = str(tmp_path / 'gtFine'), str(tmp_path / 'bbox')
    os.makedirs(dst)
    listed = fx.write_tree(src)
    preprocess.construct_box(src, fx.INST_PATTERN, fx.CLS_PATTERN, dst)
    assert sorted(os.listdir(dst)) == sorted(s + '.json' for s in GOLD)
    for stem, _, _ in listed:
        with open(os.path.join(dst, stem + '.json'), 'rb') as f:
            assert f.read() == GOLD[stem].encode(), stem
    assert capsys.readouterr().out.count('wrote a bbox summary of ') == len(GOLD)


def test_inst_info_on_device_tensors_equals_the_file():
    from neurips18_hierchical_image_manipulation_amd import preprocess
    for name, inst, label in _pairs():
        want = json.loads(GOLD[os.path.basename(name) + '_gtFine_instanceIds'])
        assert preprocess.inst_info(_dev(inst.astype(np.int32))[None, None], _dev(label.astype(np.float32))[None, None]) == want
        assert preprocess.inst_info(_dev(inst.astype(np.float32))[None], _dev(label)[None]) == want
        assert preprocess.inst_info(_dev(inst), _dev(label)) == want


def test_preprocessed_directory_opens_through_the_loader(tmp_path):
    """A raw tree (leftImg8bit/, gtFine/) through ``main``: folders, copies and box files; then the loader reads it."""
    from neurips18_hierchical_image_manipulation_amd import preprocess
    from neurips18_hierchical_image_manipulation_amd.data.data_loader import CreateDataLoader
    from neurips18_hierchical_image_manipulation_amd.options import MaskToImageTrainOptions
    staged, root = str(tmp_path / 'staged'), str(tmp_path / 'cityscape')
    data_fixture.write_dataset(staged, 'city')
    for phase in ('train', 'val'):
        os.makedirs(os.path.join(root, 'leftImg8bit', phase))
        os.makedirs(os.path.join(root, 'gtFine', phase))
    maps = {}
    for i, stem in enumerate(sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(staged, 'train_label')))):
        city = 'ulm' if i % 2 else 'jena'
        for d in (os.path.join(root, 'leftImg8bit', 'train', city), os.path.join(root, 'gtFine', 'train', city)):
            os.makedirs(d, exist_ok=True)
        new = '%s_%06d_000019' % (city, i)
        shutil.copy(os.path.join(staged, 'train_img', stem + '.png'),
                    os.path.join(root, 'leftImg8bit', 'train', city, new + '_leftImg8bit.png'))
        shutil.copy(os.path.join(staged, 'train_label', stem + '.png'),
                    os.path.join(root, 'gtFine', 'train', city, new + '_gtFine_labelIds.png'))
        shutil.copy(os.path.join(staged, 'train_inst', stem + '.png'),
                    os.path.join(root, 'gtFine', 'train', city, new + '_gtFine_instanceIds.png'))
        from PIL import Image
        maps[new] = (np.array(Image.open(os.path.join(staged, 'train_inst', stem + '.png'))),
                     np.array(Image.open(os.path.join(staged, 'train_label', stem + '.png'))))
    preprocess.main(['--dataroot', root])
    for sub in ('img', 'label', 'inst', 'bbox'):
        assert len(os.listdir(os.path.join(root, 'train_' + sub))) == 4 and os.listdir(os.path.join(root, 'val_' + sub)) == []
    for new, (inst, label) in maps.items():
        with open(os.path.join(root, 'train_bbox', new + '_gtFine_instanceIds.json')) as f:
            text = f.read()
        assert text == json.dumps(fx.rows_to_info(inst.shape[0], inst.shape[1], fx.restate(inst, label))), new
        assert len(json.loads(text)['objects']) >= 1
    argv = data_fixture.loader_argv(root, 'city', 64, ['--contextMargin', '3.0', '--min_box_size', '16',
                                                        '--max_box_size', '96'])
    opt = MaskToImageTrainOptions().parse(save=False, default_args=argv)
    loader = CreateDataLoader(opt)
    assert len(loader) == 4
    batches = list(loader.load_data())
    assert len(batches) == 2
    for b in batches:
        assert b['image'].is_cuda and tuple(b['image'].shape) == (2, 3, 64, 64)
        assert tuple(b['label'].shape)[0] == 2 and bool(torch.isfinite(b['image']).all())
