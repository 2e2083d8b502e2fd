"""not gpu: the host side of the instance labelling of layouts -- the numpy reference of tests/ccl_fixture.py on planes
whose answer is written out here (and against scipy.ndimage.label where scipy is installed), the C ABI's declarations
and exports, the object-list helpers of ``preprocess`` and the argument checks the library makes before it launches
anything."""
import ctypes
import os
import re

import numpy as np
import pytest

import ccl_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_WORKSPACE = -1, -2
S = fx.STUFF


def test_reference_labels_hand_drawn_planes():
    things = (24, 25)
    plane = np.array([[24, 24, S, 25, 25],
                      [S, 24, S, 25, S],
                      [24, S, 24, S, 25],
                      [24, S, 24, 24, 25]], np.uint8)
    inst4 = np.array([[1000, 1000, S, 1001, 1001],
                      [S, 1000, S, 1001, S],
                      [1002, S, 1003, S, 1004],
                      [1002, S, 1003, 1003, 1004]], np.int32)
    got, count, flags = fx.label_reference(plane, things, 4)
    assert np.array_equal(got, inst4) and (count, flags) == (5, 0)
    # 8-connectivity: (1,1)-(2,0) and (1,1)-(2,2) join the 24s; (1,3)-(2,4) joins the 25s
    inst8 = np.where(plane == 24, 1000, np.where(plane == 25, 1001, S)).astype(np.int32)
    got, count, flags = fx.label_reference(plane, things, 8)
    assert np.array_equal(got, inst8) and (count, flags) == (2, 0)
    # min_area 3 under 4-connectivity drops the two two-pixel components and renumbers without a gap
    drop = inst4.copy()
    drop[inst4 == 1002] = 24
    drop[inst4 == 1003] = 1002
    drop[inst4 == 1004] = 25
    got, count, flags = fx.label_reference(plane, things, 4, min_area=3)
    assert np.array_equal(got, drop) and (count, flags) == (3, 0)
    # a class that is no thing keeps its id; another base id; an empty list of things returns the plane
    got, count, _ = fx.label_reference(plane, (25,), 4, base_id=300)
    want = plane.astype(np.int32)
    want[inst4 == 1001] = 300
    want[inst4 == 1004] = 301
    assert np.array_equal(got, want) and count == 2
    got, count, flags = fx.label_reference(plane, (), 8)
    assert np.array_equal(got, plane.astype(np.int32)) and (count, flags) == (0, 0)


def test_reference_numbers_by_first_pixel_and_keeps_classes_apart():
    # a "U" whose first pixel comes before the blob it encloses; two classes side by side never join
    plane = np.array([[26, S, 27, S, 26],
                      [26, S, 27, S, 26],
                      [26, 26, 26, 26, 26]], np.uint8)
    want = np.array([[1000, S, 1001, S, 1000],
                     [1000, S, 1001, S, 1000],
                     [1000, 1000, 1000, 1000, 1000]], np.int32)
    for conn in (4, 8):
        got, count, flags = fx.label_reference(plane, (26, 27), conn)
        assert np.array_equal(got, want) and (count, flags) == (2, 0), conn


def test_reference_flags():
    plane = fx.checkerboard(5, 5)
    _, count, flags = fx.label_reference(plane, (24, 25), 4, max_objects=24)
    assert (count, flags) == (25, fx.OVERFLOW)
    _, count, flags = fx.label_reference(plane, (24, 25), 4, base_id=65535 - 23, max_objects=64)
    assert (count, flags) == (25, fx.OVERFLOW)
    _, count, flags = fx.label_reference(plane, (24, 25), 4, base_id=65535 - 24, max_objects=25)
    assert (count, flags) == (25, 0)
    for bad in (np.array([[3.5, 1.0]], np.float32), np.array([[256, 1]], np.int32), np.array([[-1, 1]], np.int64)):
        assert fx.label_reference(bad, (1,), 4)[2] == fx.CLS_RANGE


def test_generated_planes_have_the_structure_the_gpu_cases_rely_on():
    for H, W in ((67, 131), (97, 193)):
        for transpose in (False, True):
            p = fx.serpentine(H, W, transpose=transpose)
            for conn in (4, 8):
                inst, count, _ = fx.label_reference(p, fx.CITY_THINGS, conn)
                assert count == 1 and ((inst == 1000) == (p == 26)).all()
    board = fx.checkerboard()
    assert fx.label_reference(board, (24, 25), 4, max_objects=4096)[1] == 33 * 65 == 2145
    assert fx.label_reference(board, (24, 25), 8)[1] == 2
    for anti in (False, True):
        st = fx.stair(anti=anti)
        n = int((st == 28).sum())
        assert fx.label_reference(st, fx.CITY_THINGS, 8)[1] == 1 and fx.label_reference(st, fx.CITY_THINGS, 4)[1] == n > 90
    split = fx.split_by_stuff_line()
    assert fx.label_reference(split, fx.CITY_THINGS, 8)[1] == 4 and fx.label_reference(split, fx.CITY_THINGS, 4)[1] == 4
    cb = fx.comb()
    assert fx.label_reference(cb, fx.CITY_THINGS, 4)[1] == 2 + 8
    inst, count, _ = fx.label_reference(fx.blobs(7), fx.CITY_THINGS, 4, min_area=7)
    assert count == 4 and sorted(np.unique(inst[inst >= 1000]).tolist()) == [1000, 1001, 1002, 1003]
    assert fx.label_reference(fx.blobs(7), fx.CITY_THINGS, 4, min_area=1)[1] == 6
    plane, rows = fx.rects_and_ells()
    inst, count, _ = fx.label_reference(plane, fx.CITY_THINGS, 4)
    assert count == len(rows)
    for r in rows:
        ys, xs = np.nonzero(inst == r[0])
        assert [xs.min(), ys.min(), xs.max(), ys.max(), len(xs)] == r[1:6].tolist() and (plane[ys, xs] == r[6]).all()


def test_reference_partition_equals_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    structs = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}
    planes = [fx.coarse_layout(64, 96, seed=3, salt=0.1), fx.checkerboard(), fx.serpentine(67, 131), fx.comb(),
              fx.stair(), fx.stair(anti=True), fx.split_by_stuff_line()]
    for plane in planes:
        things = tuple(int(c) for c in np.unique(plane) if c not in (fx.STUFF, fx.STUFF2))
        for conn in (4, 8):
            inst, count, _ = fx.label_reference(plane, things, conn, max_objects=65536, base_id=256)
            total = 0
            for c in things:
                lab, n = ndimage.label(plane == c, structure=structs[conn])
                total += n
                sel = plane == c
                assert fx.partition_equal(inst[sel], lab[sel]), (c, conn)
            assert count == total
            stuff = ~np.isin(plane, things)
            assert (inst[stuff] == plane[stuff]).all()


def test_header_declares_and_library_exports_the_entry_points():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        header = f.read()
    assert re.search(r'^int him_label_instances\(', header, flags=re.M)
    assert re.search(r'^size_t him_label_instances_workspace\(', header, flags=re.M)
    assert re.search(r'^#define HIM_CCL_OVERFLOW 1$', header, flags=re.M)
    assert re.search(r'^#define HIM_CCL_CLS_RANGE 2$', header, flags=re.M)
    assert os.path.isfile(_cabi.LIB_PATH), 'libhim_hip.so not built'
    dll = ctypes.CDLL(_cabi.LIB_PATH)
    for name in ('him_label_instances', 'him_label_instances_workspace'):
        assert name in _cabi.EXPORTS and hasattr(dll, name), name


def test_layout_objects_round_trip():
    from neurips18_hierchical_image_manipulation_amd import preprocess
    rows = np.array([[1000, 5, 4, 19, 9, 90, 26], [1001, 60, 6, 69, 49, 440, 24], [1002, 100, 20, 129, 35, 168, 33]],
                    np.int32)
    info = preprocess.rows_to_info(72, 150, rows)
    assert list(info['objects']) == ['1000', '1001', '1002']
    objects = preprocess.layout_objects(info)
    assert objects == [{'bbox': [5, 4, 19, 9], 'cls': 26}, {'bbox': [60, 6, 69, 49], 'cls': 24},
                       {'bbox': [100, 20, 129, 35], 'cls': 33}]
    assert all(type(v) is int for o in objects for v in o['bbox'] + [o['cls']])
    assert preprocess.layout_objects(preprocess.rows_to_info(8, 8, np.zeros((0, 7), np.int32))) == []
    assert callable(preprocess.layout_info)


def test_argument_checks_return_before_any_launch():
    """Nothing below reaches a launch: the pointers are never dereferenced on the host, and every call is refused."""
    from neurips18_hierchical_image_manipulation_amd import _cabi
    dll = _cabi.lib._load()
    ws_fn, fn = dll.him_label_instances_workspace, dll.him_label_instances
    need = int(ws_fn(2, 1024, 2048))
    assert need >= 2 * 2 * 1024 * 2048 * 4 and need % 16 == 0
    assert int(ws_fn(0, 8, 8)) == 0 and int(ws_fn(1, 0, 8)) == 0 and int(ws_fn(1, 8, -1)) == 0
    assert int(ws_fn(1, 1 << 16, 1 << 15)) == 0 and int(ws_fn(1, 1, 1)) >= 16
    p = 1 << 20                                             # a 16-byte aligned non-null address, never read
    order = ['cls', 'cls_kind', 'B', 'H', 'W', 'thing', 'connectivity', 'min_area', 'base_id', 'max_objects', 'inst_out',
             'status', 'ws', 'ws_bytes', 'stream']
    good = dict(cls=p, cls_kind=0, B=2, H=1024, W=2048, thing=p, connectivity=4, min_area=1, base_id=1000,
                max_objects=1024, inst_out=p, status=p, ws=p, ws_bytes=need, stream=0)
    bad = [('cls', 0), ('thing', 0), ('inst_out', 0), ('status', 0), ('ws', 0), ('connectivity', 6), ('connectivity', 0),
           ('B', 0), ('H', 0), ('W', -3), ('H', 1 << 30), ('base_id', 255), ('base_id', -1), ('max_objects', 0),
           ('max_objects', 65537), ('cls_kind', 4), ('cls_kind', -1), ('ws', p + 4)]
    for name, value in bad:
        args = dict(good, **{name: value})
        rc = fn(*[args[k] for k in order])
        assert rc == E_INVALID, (name, value, rc)
        assert b'label_instances' in dll.him_last_error(), (name, dll.him_last_error())
    for short in (need - 1, 0):
        assert fn(*[dict(good, ws_bytes=short)[k] for k in order]) == E_WORKSPACE
        assert b'label_instances' in dll.him_last_error()
    with pytest.raises(_cabi.HimError, match='label_instances'):
        _cabi.lib.him_label_instances(*[dict(good, connectivity=5)[k] for k in order])


def test_binding_refuses_host_tensors_and_bad_arguments():
    import torch
    from neurips18_hierchical_image_manipulation_amd import ops
    assert ops.CITYSCAPES_THINGS == tuple(range(24, 34))
    with pytest.raises(ValueError, match='device tensor'):
        ops.label_instances(torch.zeros(4, 4, dtype=torch.uint8), ops.CITYSCAPES_THINGS)
    with pytest.raises(ValueError, match='outside 0..255'):
        ops.label_instances_launch(torch.zeros(4, 4, dtype=torch.uint8), (300,))


def test_command_line_parses_the_class_list():
    from neurips18_hierchical_image_manipulation_amd import preprocess_labels
    assert preprocess_labels.parse_things('24,25, 26') == (24, 25, 26) and preprocess_labels.parse_things('') == ()
    with pytest.raises(ValueError):
        preprocess_labels.parse_things('24,256')
