"""gpu: the instance labelling of layouts on the device against the numpy reference of tests/ccl_fixture.py on the same
plane.  Integer results: every comparison is for equality.  The C-ABI calls run inside tests/abi_harness.py's guarded
arena: guard bands in front of and behind the class planes, the thing table, the instance planes, the status record and
the workspace.  Shapes are worded in the kernel's tile of 32 x 64 pixels and its rank chunks of 2048 pixels."""
import json
import os

import numpy as np
import pytest
import torch

import abi_harness as ah
import ccl_fixture as fx

pytestmark = pytest.mark.gpu

E_INVALID, E_WORKSPACE = -1, -2
CLS_KIND = {np.dtype(np.uint8): 0, np.dtype(np.int32): 1, np.dtype(np.int64): 2, np.dtype(np.float32): 3}
CANARY = -1515870811                    # 0xA5A5A5A5: what a cell of inst_out / status holds before the call


class Guarded(object):
    """A batch of class planes, the thing table, inst_out, status and the workspace of him_label_instances in ONE guarded
    allocation.  ``shift`` moves the batch's base by that many ELEMENTS off its 256-byte aligned start."""

    def __init__(self, planes, things, shift=0):
        self.lib = ah.raw_lib()
        a = np.ascontiguousarray(planes)
        self.a = a if a.ndim == 3 else a[None]
        self.B, self.H, self.W = self.a.shape
        self.off = shift * self.a.itemsize
        self.things = things
        self.nws = int(self.lib.him_label_instances_workspace(self.B, self.H, self.W))
        assert self.nws > 0
        specs = {'cls': ('ws', self.a.nbytes + self.off), 'thing': ('ws', 256), 'inst': ('ws', self.a.size * 4),
                 'status': ('ws', 8 * self.B), 'ws': ('ws', self.nws)}
        self.ar = ah.Arena('cuda', specs)
        self.ar.t['cls'][self.off:self.off + self.a.nbytes].copy_(torch.from_numpy(self.a.reshape(-1).view(np.uint8)))
        self.ar.t['thing'].copy_(torch.from_numpy(fx.thing_table(things)))

    def raw(self, connectivity=4, min_area=1, base_id=1000, max_objects=1024, **over):
        """One call; returns (rc, inst (B,H,W) int32, status (B,2)) and asserts the bands and the inputs."""
        ar = self.ar
        ar.t['inst'].fill_(0xA5)
        ar.t['status'].fill_(0xA5)
        args = dict(cls=ar.ptr('cls') + self.off, cls_kind=CLS_KIND[self.a.dtype], B=self.B, H=self.H, W=self.W,
                    thing=ar.ptr('thing'), connectivity=connectivity, min_area=min_area, base_id=base_id,
                    max_objects=max_objects, inst_out=ar.ptr('inst'), status=ar.ptr('status'), ws=ar.ptr('ws'),
                    ws_bytes=self.nws, stream=torch.cuda.current_stream().cuda_stream)
        args.update(over)
        rc = self.lib.him_label_instances(*[args[k] for k in (
            'cls', 'cls_kind', 'B', 'H', 'W', 'thing', 'connectivity', 'min_area', 'base_id', 'max_objects', 'inst_out',
            'status', 'ws', 'ws_bytes', 'stream')])
        torch.cuda.synchronize()
        bad = ar.guard_failures()
        assert not bad, '; '.join(bad)
        assert bytes(ar.t['cls'][self.off:self.off + self.a.nbytes].cpu().numpy()) == self.a.tobytes()
        assert bytes(ar.t['thing'].cpu().numpy()) == fx.thing_table(self.things).tobytes()
        inst = ar.t['inst'].cpu().numpy().view(np.int32).reshape(self.B, self.H, self.W).copy()
        status = ar.t['status'].cpu().numpy().view(np.int32).reshape(self.B, 2).copy()
        return rc, inst, status

    def check(self, connectivity=4, min_area=1, base_id=1000, max_objects=1024):
        """The call equals the reference on every plane (inst_out only where no flag is set); returns (inst, status)."""
        rc, inst, status = self.raw(connectivity, min_area, base_id, max_objects)
        assert rc == 0, self.lib.him_last_error()
        for b in range(self.B):
            want, count, flags = fx.label_reference(self.a[b], self.things, connectivity, min_area, base_id, max_objects)
            assert (int(status[b, 0]), int(status[b, 1])) == (count, flags), (b, status[b], count, flags)
            if flags == 0:
                diff = np.argwhere(inst[b] != want)
                assert len(diff) == 0, 'plane %d: %d pixels differ, first at %s: got %d, want %d' % (
                    b, len(diff), diff[0], inst[b][tuple(diff[0])], want[tuple(diff[0])])
        return inst, status


@pytest.mark.parametrize('transpose', (False, True))
@pytest.mark.parametrize('shape', ((67, 131), (97, 193)))
def test_serpentine_through_every_tile_border(shape, transpose):
    g = Guarded(fx.serpentine(shape[0], shape[1], transpose=transpose), fx.CITY_THINGS)
    for conn in (4, 8):
        _, status = g.check(conn)
        assert status.tolist() == [[1, 0]]


def test_combs_join_only_in_the_next_tile_row_and_nothing_joins_through_stuff():
    g = Guarded(fx.comb(), fx.CITY_THINGS)
    for conn in (4, 8):
        assert g.check(conn)[1].tolist() == [[10, 0]]
    g = Guarded(fx.split_by_stuff_line(), fx.CITY_THINGS)
    for conn in (4, 8):
        assert g.check(conn)[1].tolist() == [[4, 0]]


def test_checkerboard_dense_ranks_and_overflow():
    g = Guarded(fx.checkerboard(), (24, 25))
    inst, status = g.check(4, max_objects=4096)
    assert status.tolist() == [[2145, 0]]
    assert np.array_equal(inst[0].reshape(-1), 1000 + np.arange(2145))          # every pixel its own object, in raster order
    _, status = g.check(4, max_objects=1024)
    assert status.tolist() == [[2145, fx.OVERFLOW]]                               # the true count all the same
    _, status = g.check(4, max_objects=4096, base_id=65535 - 2143)
    assert status.tolist() == [[2145, fx.OVERFLOW]]                               # the ids would pass 65535
    _, status = g.check(8)
    assert status.tolist() == [[2, 0]]


@pytest.mark.parametrize('anti', (False, True))
def test_diagonal_stair_across_tile_corners(anti):
    plane = fx.stair(anti=anti)
    g = Guarded(plane, fx.CITY_THINGS)
    assert g.check(8)[1].tolist() == [[1, 0]]
    assert g.check(4)[1].tolist() == [[int((plane == 28).sum()), 0]]


def test_min_area_threshold_is_inclusive():
    plane = fx.blobs(7)
    g = Guarded(plane, fx.CITY_THINGS)
    inst, status = g.check(4, min_area=7)
    assert status.tolist() == [[4, 0]]
    assert (inst[0][2, 3:9] == 24).all() and (inst[0][30:34, 20] == 25).all()    # dropped blobs keep their class
    assert inst[0][5, 60] == 1000 and inst[0][9, 10] == 1001 and inst[0][20, 70] == 1002 and inst[0][31, 40] == 1003
    assert g.check(4, min_area=8)[1].tolist() == [[2, 0]]
    assert g.check(4, min_area=6)[1].tolist() == [[5, 0]]
    for m in (1, 0, -5):
        assert g.check(8, min_area=m)[1].tolist() == [[6, 0]]


def test_no_things_and_all_things_on_a_noisy_layout():
    plane = fx.coarse_layout()
    assert plane.shape == (256, 512) and plane.max() == 34
    g = Guarded(plane, ())
    inst, status = g.check(8)
    assert status.tolist() == [[0, 0]] and np.array_equal(inst[0], plane.astype(np.int32))
    g = Guarded(plane, tuple(range(35)))
    for conn in (4, 8):
        inst, status = g.check(conn, max_objects=65536)
        assert status[0, 1] == 0 and status[0, 0] > 512 and inst.min() >= 1000


@pytest.mark.parametrize('shape', ((1, 1), (1, 300), (300, 1)))
def test_degenerate_planes(shape):
    rng = np.random.RandomState(shape[1])
    plane = rng.choice(np.array([24, 25, fx.STUFF], np.uint8), size=shape)
    g = Guarded(plane, (24, 25))
    for conn in (4, 8):
        g.check(conn)
    g = Guarded(np.full(shape, 24, np.uint8), (24,))
    assert g.check(4)[1].tolist() == [[1, 0]]


@pytest.mark.parametrize('dtype', (np.uint8, np.int32, np.int64, np.float32))
def test_every_class_kind_and_a_shifted_base(dtype):
    plane = fx.coarse_layout(70, 131, seed=5, salt=0.05).astype(dtype)
    for shift in (0, 1):
        g = Guarded(plane, fx.CITY_THINGS, shift=shift)
        for conn in (4, 8):
            g.check(conn, min_area=3)


def test_classes_outside_the_domain_set_the_flag():
    base = fx.coarse_layout(40, 70, seed=2).astype(np.int32)
    for dtype, value in ((np.float32, 3.5), (np.int32, 256), (np.int32, -1), (np.int64, 1 << 40), (np.float32, np.nan)):
        plane = base.astype(dtype)
        plane[33, 65] = value
        good = base.astype(dtype)
        g = Guarded(np.stack([good, plane, good]), fx.CITY_THINGS)
        inst, status = g.check(4)
        assert status[:, 1].tolist() == [0, fx.CLS_RANGE, 0], (dtype, value)       # and the planes around it are right


def test_planes_of_a_batch_are_numbered_independently():
    planes = np.stack([fx.coarse_layout(70, 140, seed=s, salt=0.03) for s in (1, 2)] + [fx.comb()])
    g = Guarded(planes, fx.CITY_THINGS)
    for conn in (4, 8):
        inst, status = g.check(conn)
        assert (status[:, 0] > 1).all() and (status[:, 1] == 0).all()
        for b in range(3):
            ids = np.unique(inst[b][inst[b] >= 1000])
            assert ids.tolist() == list(range(1000, 1000 + int(status[b, 0])))


def test_same_call_twice_is_identical_and_the_workspace_needs_no_clearing():
    a, b = fx.coarse_layout(97, 193, seed=8, salt=0.05), fx.serpentine(97, 193)
    g = Guarded(a, fx.CITY_THINGS)
    first, st1 = g.check(8)
    second, st2 = g.check(8)
    assert first.tobytes() == second.tobytes() and st1.tobytes() == st2.tobytes()
    g.a = b[None]                                          # another plane through the same arena and workspace
    g.ar.t['cls'][:b.nbytes].copy_(torch.from_numpy(b.reshape(-1)))
    assert g.check(8)[1].tolist() == [[1, 0]]
    g.ar.t['ws'].fill_(0x5A)                               # and whatever the workspace holds
    assert g.check(4)[1].tolist() == [[1, 0]]


def test_binding_shapes_dtypes_counts_and_errors():
    from neurips18_hierchical_image_manipulation_amd import ops
    planes = np.stack([fx.coarse_layout(70, 131, seed=s, salt=0.03) for s in (3, 4, 5)])
    want = [fx.label_reference(p, fx.CITY_THINGS, 8, 2) for p in planes]
    dev = torch.from_numpy(planes).cuda()
    for t in (dev, dev[:, None], dev.to(torch.int32), dev.to(torch.int64)[:, None], dev.float()):
        inst, counts = ops.label_instances(t, ops.CITYSCAPES_THINGS, connectivity=8, min_area=2)
        assert inst.dtype == torch.int32 and inst.shape == t.shape and inst.is_cuda
        assert counts.tolist() == [w[1] for w in want]
        assert np.array_equal(inst.reshape(3, 70, 131).cpu().numpy(), np.stack([w[0] for w in want]))
    one, counts = ops.label_instances(dev[1], ops.CITYSCAPES_THINGS, connectivity=8, min_area=2)
    assert one.shape == (70, 131) and counts.tolist() == [want[1][1]] and np.array_equal(one.cpu().numpy(), want[1][0])
    view = dev[:, 3:, 5:]                                  # a non-contiguous view
    inst, counts = ops.label_instances(view, range(24, 34))
    for b in range(3):
        w = fx.label_reference(planes[b, 3:, 5:], fx.CITY_THINGS)
        assert np.array_equal(inst[b].cpu().numpy(), w[0]) and counts[b] == w[1]
    inst, counts, st = ops.label_instances_launch(dev, ops.CITYSCAPES_THINGS, 8, 2)
    assert counts.is_cuda and counts.cpu().tolist() == [w[1] for w in want] and st['out'].shape == (3, 2)
    with pytest.raises(ValueError, match='plane 0: 2145 objects'):
        ops.label_instances(torch.from_numpy(fx.checkerboard()).cuda(), (24, 25))
    bad = dev.to(torch.int32).clone()
    bad[2, 0, 0] = 300
    with pytest.raises(ValueError, match='plane 2: a class value outside 0..255'):
        ops.label_instances(bad, ops.CITYSCAPES_THINGS)
    for kw in (dict(connectivity=6), dict(base_id=255), dict(max_objects=0), dict(max_objects=65537)):
        with pytest.raises(ValueError, match='label_instances'):
            ops.label_instances(dev, ops.CITYSCAPES_THINGS, **kw)
    with pytest.raises(ValueError, match='label_instances'):
        ops.label_instances(dev.to(torch.int16), ops.CITYSCAPES_THINGS)


def test_layout_info_on_rectangles_and_ells():
    from neurips18_hierchical_image_manipulation_amd import preprocess
    plane, rows = fx.rects_and_ells()
    label = torch.from_numpy(plane).cuda().float()[None, None]      # as the joint edit keeps its canvases
    inst, info = preprocess.layout_info(label, fx.CITY_THINGS)
    assert inst.shape == label.shape and inst.dtype == torch.int32
    assert np.array_equal(inst[0, 0].cpu().numpy(), fx.label_reference(plane, fx.CITY_THINGS)[0])
    want = {'imgHeight': 72, 'imgWidth': 150,
            'objects': {str(int(r[0])): {'bbox': [int(v) for v in r[1:5]], 'cls': int(r[6])} for r in rows}}
    assert info == want and list(info['objects']) == [str(int(r[0])) for r in rows]
    assert preprocess.inst_info(inst, label) == want                # the component plane reproduces the table
    assert preprocess.layout_objects(info) == [{'bbox': [int(v) for v in r[1:5]], 'cls': int(r[6])} for r in rows]
    _, small = preprocess.layout_info(label, fx.CITY_THINGS, connectivity=8, min_area=100)
    assert list(small['objects']) == ['1000', '1001'] and small['objects']['1000']['cls'] == 24
    assert small['objects']['1001']['bbox'] == [100, 20, 129, 35]


def test_refusals_write_nothing():
    g = Guarded(fx.coarse_layout(40, 70, seed=2), fx.CITY_THINGS)
    ws0 = g.ar.t['ws'].clone()
    bad = [('cls', 0), ('thing', 0), ('inst_out', 0), ('status', 0), ('ws', 0), ('connectivity', 5), ('connectivity', 0),
           ('B', 0), ('H', 0), ('W', -1), ('H', 1 << 26), ('base_id', 255), ('max_objects', 0), ('max_objects', 65537),
           ('cls_kind', 4), ('cls_kind', -1), ('ws', g.ar.ptr('ws') + 4), ('ws_bytes', g.nws - 1), ('ws_bytes', 0)]
    for name, value in bad:
        rc, inst, status = g.raw(**{name: value})
        assert rc == (E_WORKSPACE if name == 'ws_bytes' else E_INVALID), (name, value, rc)
        assert g.lib.him_last_error(), name
        assert (inst == CANARY).all() and (status == CANARY).all(), name
        assert torch.equal(g.ar.t['ws'], ws0), name
    g.check(8)                                             # and the next call is clean


def test_command_line_writes_a_folder_the_loader_reads(tmp_path, capsys):
    from PIL import Image
    from neurips18_hierchical_image_manipulation_amd import preprocess_labels
    from neurips18_hierchical_image_manipulation_amd.data.data_loader import CreateDataLoader
    from neurips18_hierchical_image_manipulation_amd.options import MaskToImageTrainOptions
    import data_fixture
    root = str(tmp_path / 'labels_only')
    os.makedirs(os.path.join(root, 'train_label'))
    os.makedirs(os.path.join(root, 'train_img'))
    maps = {}
    for i, (h, w) in enumerate(((96, 160), (70, 131), (128, 128))):
        plane = fx.coarse_layout(h, w, classes=20, cell=16, seed=20 + i, salt=0.0)
        plane[10:40, 20:60] = 26                           # objects the sampler can pick
        plane[50:66, 70:120] = 24
        plane[5:8, 100:103] = 25                           # 9 pixels: stays stuff under --min_area 10
        maps['map_%d' % i] = plane
        Image.fromarray(plane, 'L').save(os.path.join(root, 'train_label', 'map_%d.png' % i))
        photo = np.random.RandomState(i).randint(0, 256, (h, w, 3)).astype(np.uint8)
        Image.fromarray(photo, 'RGB').save(os.path.join(root, 'train_img', 'map_%d.png' % i))
    things = tuple(range(24, 34))
    preprocess_labels.main(['--dataroot', root, '--things', ','.join(str(c) for c in things), '--connectivity', '8',
                            '--min_area', '10'])
    assert capsys.readouterr().out.count('labelled ') == 3
    assert not os.path.exists(os.path.join(root, 'val_inst'))
    assert sorted(os.listdir(os.path.join(root, 'train_inst'))) == ['map_0.png', 'map_1.png', 'map_2.png']
    assert sorted(os.listdir(os.path.join(root, 'train_bbox'))) == ['map_0.json', 'map_1.json', 'map_2.json']
    for stem, plane in maps.items():
        want, count, flags = fx.label_reference(plane, things, 8, 10)
        assert flags == 0 and count == 2
        with Image.open(os.path.join(root, 'train_inst', stem + '.png')) as im:
            assert im.mode == 'I;16'
            got = np.array(im)
        assert got.dtype == np.uint16 and np.array_equal(got, want.astype(np.uint16)), stem
        with open(os.path.join(root, 'train_bbox', stem + '.json')) as f:
            info = json.load(f)
        assert info == {'imgHeight': plane.shape[0], 'imgWidth': plane.shape[1],
                        'objects': {'1000': {'bbox': [20, 10, 59, 39], 'cls': 26},
                                    '1001': {'bbox': [70, 50, 119, 65], 'cls': 24}}}, stem
    argv = data_fixture.loader_argv(root, 'city', 64, ['--contextMargin', '3.0', '--min_box_size', '16',
                                                        '--max_box_size', '96'])
    loader = CreateDataLoader(MaskToImageTrainOptions().parse(save=False, default_args=argv))
    assert len(loader) == 3
    import random
    random.seed(11)
    np.random.seed(11)
    picked = set()
    for i in range(3):
        for _ in range(4):                                 # an object, or (with prob_bg) a background box
            rec = loader.dataset.host_record(i)
            assert (rec['cls'], rec['params']['bbox_inst_id']) in ((26, 1000), (24, 1001), (34, None))
            assert rec['inst'].size and rec['label'].size
            picked.add(rec['params']['bbox_inst_id'])
    assert picked & {1000, 1001}
