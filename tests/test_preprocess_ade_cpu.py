"""not gpu: the host side of the ADE20K preprocessing step -- the C ABI's declarations and the argument checks the
library makes before it launches anything, the binding's own checks, the attribute and index readers on fabricated files,
and the box writer against the reference's bytes (tests/golden/preprocess_ade.json, written by the live reference from
tests/preprocess_ade_fixture.py through tests/golden/make_golden_preprocess_ade.py)."""
import json
import os
import re

import numpy as np
import pytest

import preprocess_ade_fixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
E_INVALID = -1


@pytest.fixture(scope='module')
def gold():
    with open(os.path.join(GOLD, 'preprocess_ade.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def cases():
    return fx.golden_cases()


def test_header_declares_and_library_exports_the_entry_points():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        header = f.read()
    assert re.search(r'^int him_ade_decode\(', header, flags=re.M)
    assert re.search(r'^size_t him_ade_decode_workspace\(void\);', header, flags=re.M)
    dll = _cabi.lib._load()
    for name in ('him_ade_decode', 'him_ade_decode_workspace'):
        assert name in _cabi.EXPORTS and getattr(dll, name)
    need = int(dll.him_ade_decode_workspace())
    assert need >= 4 * 5 * 256 and need % 16 == 0


def test_argument_checks_return_invalid_before_any_launch():
    """Nothing below reaches a launch: the pointers are never dereferenced on the host, and every call is refused."""
    from neurips18_hierchical_image_manipulation_amd import _cabi
    dll = _cabi.lib._load()
    fn = dll.him_ade_decode
    need = int(dll.him_ade_decode_workspace())
    p = 1 << 20                                             # a 16-byte aligned non-null address, never read
    good = dict(seg=p, H=512, W=683, pixel_bytes=3, keep=p, n_keep=48, cls_out=0, label_out=p, inst_out=p, status=p,
                table=p, ws=p, ws_bytes=need, stream=0)
    order = ['seg', 'H', 'W', 'pixel_bytes', 'keep', 'n_keep', 'cls_out', 'label_out', 'inst_out', 'status', 'table',
             'ws', 'ws_bytes', 'stream']
    bad = [('H', 0), ('W', -3), ('H', 1 << 30), ('seg', 0), ('keep', 0), ('label_out', 0), ('inst_out', 0),
           ('status', 0), ('table', 0), ('ws', 0), ('pixel_bytes', 2), ('pixel_bytes', 5), ('pixel_bytes', 1),
           ('n_keep', -1), ('n_keep', 256), ('ws_bytes', need - 1), ('ws_bytes', 0), ('ws', p + 4), ('ws', p + 8)]
    for name, value in bad:
        args = dict(good, **{name: value})
        rc = fn(*[args[k] for k in order])
        assert rc == E_INVALID, (name, value, rc)
        assert b'ade_decode' in dll.him_last_error(), (name, dll.him_last_error())
    with pytest.raises(_cabi.HimError, match='ade_decode'):
        _cabi.lib.him_ade_decode(*[dict(good, ws_bytes=need - 1)[k] for k in order])


def test_binding_refuses_host_tensors_and_bad_keep_lists():
    import torch
    from neurips18_hierchical_image_manipulation_amd import ops
    seg = torch.zeros(4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match='ade_decode: seg must be a device tensor'):
        ops.ade_decode(seg, fx.KEEP)
    with pytest.raises(ValueError, match='ade_decode: seg must be a device tensor'):
        ops.ade_decode_launch(seg.numpy(), fx.KEEP)
    for keep, why in (([2978, 165, 2978], 'duplicate'), ([2978, 2, 165], r'lies in 1\.\.3'), ([100, 1], r'lies in 1\.\.2'),
                      ([70000], 'outside 0..65535'), ([-1], 'outside 0..65535'), (list(range(1000, 1256)), 'at most 255'),
                      (['bed'], 'sequence of class ids'), (7, 'sequence of class ids')):
        with pytest.raises(ValueError, match='ade_decode: .*' + why):      # keep is checked first: no device is needed
            ops.ade_decode(seg, keep)
    assert ops._ade_keep(fx.KEEP) == tuple(fx.KEEP) and ops._ade_keep([]) == () and ops._ade_keep([0, 3]) == (0, 3)


def test_sorted_50_is_the_reference_list(gold):
    from neurips18_hierchical_image_manipulation_amd import preprocess_ade
    assert preprocess_ade.SORTED_50 == gold['sorted_50'] and len(preprocess_ade.SORTED_50) == 48
    assert len(set(gold['sorted_50'])) == 48 and not any(1 <= k <= 48 for k in gold['sorted_50'])
    assert [s['matches'] for s in gold['substitutions']] == [1, 1, 1]


def test_parse_atr_and_load_index_on_fabricated_files(tmp_path, cases):
    from neurips18_hierchical_image_manipulation_amd import preprocess_ade
    listed = fx.write_raw_tree(str(tmp_path), cases[:3])
    for jpg, _, lines in listed:
        assert any(level > 0 for _, level, _ in lines)                  # part lines are present and passed over
        assert preprocess_ade.parse_atr(jpg.replace('.jpg', '_atr.txt')) == fx.names_of(lines)
    assert any(',' in n for _, _, lines in listed for n in fx.names_of(lines))
    filenames, folders, names = preprocess_ade.load_index(str(tmp_path / 'index_ade20k.mat'))
    assert filenames == ['ADE_train_00000001.jpg', 'ADE_train_00009999.jpg', 'ADE_train_00000002.jpg',
                         'ADE_train_00000003.jpg']
    assert folders == [fx.FOLDER, fx.OTHER_FOLDER, fx.FOLDER, fx.FOLDER]
    assert names == fx.objectnames() and all(type(n) is str for n in names + filenames + folders)
    rel = preprocess_ade.bedroom_files(filenames, folders)
    assert rel == [os.path.join('images', 'training', 'b', 'bedroom', 'ADE_train_%08d.jpg' % k) for k in (1, 2, 3)]
    assert [os.path.join(str(tmp_path), r) for r in rel] == [jpg for jpg, _, _ in listed]


def test_restatement_and_writer_reproduce_every_golden_text(tmp_path, gold, cases):
    """The fixture the golden files were made from is the fixture the tests build; its numpy restatement (checked against
    the live reference when the golden files were written) through the package's ``rows_to_info`` and default
    ``json.dump`` gives the reference's bytes, and its planes are the reference's PNGs."""
    from neurips18_hierchical_image_manipulation_amd import preprocess_ade
    planes = np.load(os.path.join(GOLD, 'preprocess_ade.npz'))
    names = fx.objectnames()
    assert gold['cases'] == [tag for tag, _, _ in cases] == ['a0', 'a1', 'a2', 'b', 'c', 'd', 'e', 'f']
    for i, (tag, seg, lines) in enumerate(cases):
        prefix = 'bedroom_%05d' % (i + 1)
        cls, label, inst, rows = fx.restate(seg)
        assert np.array_equal(label, planes['label_' + prefix]) and np.array_equal(inst, planes['inst_' + prefix]), tag
        info = preprocess_ade.rows_to_info(seg.shape[0], seg.shape[1], rows, fx.names_of(lines), names, image=tag)
        path = str(tmp_path / 'box.json')
        with open(path, 'w') as f:
            json.dump(info, f)
        with open(path, 'rb') as f:
            assert f.read() == gold['json'][prefix].encode(), tag
        assert info == fx.rows_to_info(seg.shape[0], seg.shape[1], rows, fx.names_of(lines), names)
        assert info == preprocess_ade.rows_to_info(seg.shape[0], seg.shape[1], rows.astype(np.int32), fx.names_of(lines),
                                                   preprocess_ade._name_ids(names))
    by_tag = {tag: json.loads(gold['json']['bedroom_%05d' % (i + 1)]) for i, (tag, _, _) in enumerate(cases)}
    assert [len(by_tag[t]['objects']) for t in ('a0', 'a1', 'a2')] == [5, 4, 3]          # a1 drops its two unkept classes
    assert sorted(by_tag['b']['objects']) == ['1', '2', '3']                             # rank 0 (B = 7) is skipped
    assert len(fx.restate(cases[4][1])[3]) == 256                                        # c: a full table
    assert by_tag['d']['objects'] == {'1': {'bbox': [10, 1, 162, 5], 'cls': 6}, '2': {'bbox': [11, 6, 263, 12], 'cls': 10}}
    cls_e, label_e = fx.restate(cases[6][1])[:2]
    assert cls_e[3, 4] == 12 * 256 + 7 and label_e[3, 4] == 0 and cls_e[0, 0] == fx.KEEP[0] and label_e[0, 0] == 1
    cls_f, label_f = fx.restate(cases[7][1])[:2]
    assert cls_f[2, 3] == 5 and label_f[2, 3] == 0 and cls_f[10, 20] == 48 and label_f[10, 20] == 0


def test_a_name_the_index_does_not_hold_raises(cases):
    from neurips18_hierchical_image_manipulation_amd import preprocess_ade
    tag, seg, lines = cases[0]
    rows = fx.restate(seg)[3]
    names = fx.names_of(lines)
    names[1] = 'no such object'
    with pytest.raises(ValueError, match=r"ADE_train_7\.jpg: object name 'no such object'"):
        preprocess_ade.rows_to_info(seg.shape[0], seg.shape[1], rows, names, fx.objectnames(), image='ADE_train_7.jpg')
    with pytest.raises(ValueError, match='no part-level-0 line'):
        preprocess_ade.rows_to_info(seg.shape[0], seg.shape[1], rows, names[:1], fx.objectnames())
    # the first occurrence of a repeated name decides, as the reference's scan does
    twice = ['object 10', 'object 10']
    assert preprocess_ade._name_ids(twice) == {'object 10': 1}


def test_split_and_file_naming_on_a_file_list(gold):
    from neurips18_hierchical_image_manipulation_amd import preprocess_ade as pa
    got = pa.output_names(153)
    assert got[0] == ('val', 'bedroom_00001') and got[149] == ('val', 'bedroom_00150')
    assert got[150] == ('train', 'bedroom_00151') and got[152] == ('train', 'bedroom_00153')
    assert pa.output_names(3, n_val=1) == [('val', 'bedroom_00001'), ('train', 'bedroom_00002'), ('train', 'bedroom_00003')]
    assert pa.output_names(2, n_val=0) == [('train', 'bedroom_00001'), ('train', 'bedroom_00002')]
    sufs = {'bbox': pa.BBOX_SUF, 'img': pa.IMG_SUF, 'label': pa.LABEL_SUF, 'inst': pa.INST_SUF}
    for sub, suf in sufs.items():                                        # the reference's own names for the 8 cases
        assert gold['files']['val_' + sub] == [prefix + suf for _, prefix in pa.output_names(8)]
        assert gold['files']['train_' + sub] == []


def test_load_index_names_scipy_when_it_is_missing(monkeypatch, tmp_path):
    import builtins
    from neurips18_hierchical_image_manipulation_amd import preprocess_ade
    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.split('.')[0] == 'scipy':
            raise ImportError('No module named scipy')
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, '__import__', no_scipy)
    with pytest.raises(ImportError, match='needs SciPy'):
        preprocess_ade.load_index(str(tmp_path / 'index_ade20k.mat'))
