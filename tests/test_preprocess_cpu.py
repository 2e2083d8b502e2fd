"""not gpu: the host side of the preprocessing step -- the C ABI's declarations, the reference's signatures
(tests/golden/preprocess_api.json, recorded from the live reference by tests/golden/make_golden_preprocess.py), the JSON
writer against the reference's bytes (tests/golden/preprocess_city.json) and the argument checks the library makes
before it launches anything."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import preprocess_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
E_INVALID = -1


def _golden_texts():
    with open(os.path.join(GOLD, 'preprocess_city.json')) as f:
        return json.load(f)


def test_header_declares_and_cabi_lists_the_entry_points():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        header = f.read()
    assert re.search(r'^int him_inst_summary\(', header, flags=re.M)
    assert re.search(r'^size_t him_inst_summary_workspace\(', header, flags=re.M)
    for name in ('him_inst_summary', 'him_inst_summary_workspace'):
        assert name in _cabi.EXPORTS


def test_signatures_follow_the_reference():
    from neurips18_hierchical_image_manipulation_amd import preprocess
    with open(os.path.join(GOLD, 'preprocess_api.json')) as f:
        api = json.load(f)['signatures']
    assert sorted(api) == ['construct_box', 'copy_file']
    for name, params in api.items():
        mine = inspect.signature(getattr(preprocess, name)).parameters
        names = list(mine)
        assert names[:len(params)] == [p[0] for p in params], (name, names)
        for pname, default in params:
            assert default is None and mine[pname].default is inspect.Parameter.empty, (name, pname)
        for extra in names[len(params):]:               # appended parameters are optional
            assert mine[extra].default is not inspect.Parameter.empty, (name, extra)
    assert callable(preprocess.inst_info) and callable(preprocess.main)
    assert list(inspect.signature(preprocess.inst_info).parameters)[:2] == ['inst', 'label']
    assert inspect.signature(preprocess.inst_info).parameters['min_id'].default == 1000


def test_fixture_restatement_reproduces_the_golden_files(tmp_path):
    """The fixture the golden files were made from is the fixture the tests build, and the numpy restatement (checked
    against the live reference when the golden files were written) still yields those files."""
    gold = _golden_texts()
    listed = fx.write_tree(str(tmp_path))
    assert sorted(gold) == sorted(s for s, _, _ in listed)
    for stem, inst, label in listed:
        assert json.dumps(fx.rows_to_info(inst.shape[0], inst.shape[1], fx.restate(inst, label))) == gold[stem], stem
    widths = {i.shape[1] for _, i, _ in listed}
    assert {1, 383} <= widths and 1 in {i.shape[0] for _, i, _ in listed}
    assert any(i.dtype == np.uint8 for _, i, _ in listed) and any(json.loads(t)['objects'] == {} for t in gold.values())
    assert '65535' in json.loads(gold['aachen_000001_000019_gtFine_instanceIds'])['objects']


def test_json_writer_produces_the_golden_bytes(tmp_path):
    """A hand-made table through the module's writer: the reference's bytes (key order, separators, plain ints)."""
    from neurips18_hierchical_image_manipulation_amd import preprocess
    rows = np.array([[1000, 60, 33, 64, 35, 15, 9], [24001, 17, 10, 17, 10, 1, 24], [25002, 30, 20, 301, 46, 42, 25],
                     [26003, 0, 0, 382, 63, 890, 26], [27004, 100, 30, 101, 30, 2, 27], [31005, 200, 50, 201, 51, 4, 31],
                     [65535, 370, 5, 379, 8, 40, 33]], dtype=np.int32)
    path = str(tmp_path / 'edge.json')
    preprocess.write_info(path, preprocess.rows_to_info(64, 383, rows))
    with open(path, 'rb') as f:
        got = f.read()
    assert got == _golden_texts()['aachen_000001_000019_gtFine_instanceIds'].encode()
    preprocess.write_info(path, preprocess.rows_to_info(np.int64(48), np.int32(80), np.zeros((0, 7), np.int32)))
    with open(path, 'rb') as f:
        assert f.read() == _golden_texts()['aachen_000002_000019_gtFine_instanceIds'].encode()


def test_copy_file_follows_the_glob(tmp_path, capsys):
    from neurips18_hierchical_image_manipulation_amd import preprocess
    src, dst = tmp_path / 'src', tmp_path / 'dst'
    for city, name in (('b', 'b_1_x.png'), ('a', 'a_2_x.png'), ('a', 'a_1_x.png'), ('a', 'a_1_y.png')):
        (src / city).mkdir(parents=True, exist_ok=True)
        (src / city / name).write_bytes(name.encode())
    dst.mkdir()
    preprocess.copy_file(str(src), '*_x.png', str(dst))
    assert sorted(os.listdir(str(dst))) == ['a_1_x.png', 'a_2_x.png', 'b_1_x.png']
    assert (dst / 'a_2_x.png').read_bytes() == b'a_2_x.png'
    lines = capsys.readouterr().out.splitlines()
    assert [os.path.basename(l.split(' to ')[0]) for l in lines] == ['a_1_x.png', 'a_2_x.png', 'b_1_x.png']


def test_argument_checks_return_invalid_before_any_launch():
    """Nothing below reaches a launch: the pointers are never dereferenced on the host, and every call is refused."""
    from neurips18_hierchical_image_manipulation_amd import _cabi
    dll = _cabi.lib._load()
    ws_fn, fn = dll.him_inst_summary_workspace, dll.him_inst_summary
    need = int(ws_fn(1024, 2048, 1024))
    assert need >= 4 * (5 * 65536 + 65536 + 1024 * 256)
    assert int(ws_fn(0, 8, 8)) == 0 and int(ws_fn(8, 8, 0)) == 0 and int(ws_fn(8, 8, 65537)) == 0
    p = 1 << 20                                             # a 16-byte aligned non-null address, never read
    good = dict(inst=p, inst_kind=1, cls=p, cls_kind=0, H=1024, W=2048, min_id=1000, max_objects=1024, status=p, table=p,
                ws=p, ws_bytes=need, stream=0)
    order = ['inst', 'inst_kind', 'cls', 'cls_kind', 'H', 'W', 'min_id', 'max_objects', 'status', 'table', 'ws',
             'ws_bytes', 'stream']
    bad = [('H', 0), ('W', -3), ('H', 1 << 30), ('inst', 0), ('cls', 0), ('status', 0), ('table', 0), ('ws', 0),
           ('inst_kind', 4), ('inst_kind', -1), ('cls_kind', 4), ('cls_kind', -1), ('max_objects', 0),
           ('max_objects', 65537), ('ws_bytes', need - 1), ('ws_bytes', 0), ('ws', p + 4)]
    for name, value in bad:
        args = dict(good, **{name: value})
        rc = fn(*[args[k] for k in order])
        assert rc == E_INVALID, (name, value, rc)
        assert b'inst_summary' in dll.him_last_error(), (name, dll.him_last_error())
    with pytest.raises(_cabi.HimError, match='inst_summary'):
        _cabi.lib.him_inst_summary(*[dict(good, ws_bytes=need - 1)[k] for k in order])


def test_binding_refuses_host_tensors_and_bad_kinds():
    import torch
    from neurips18_hierchical_image_manipulation_amd import ops
    with pytest.raises(ValueError, match='device tensor'):
        ops.inst_summary(torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.uint8))
