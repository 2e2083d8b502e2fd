"""tests/golden/preprocess_city.json and tests/golden/preprocess_api.json.

preprocess_city.json: for every pair of tests/preprocess_fixture.py, the exact text the live reference's
``preprocess_city.construct_box`` writes into ``<stem>.json``.  The reference is imported as it stands (with
``sys.dont_write_bytecode`` set, so nothing is written into its tree).  One thing is handed to it: a ``json`` whose
``dump`` converts numpy integers to Python ints -- under Python 3 ``json.dump`` refuses the ``np.int64`` box corners the
script collects (Python 2 took them for ints).  The conversion changes no number and no byte of the layout.

preprocess_api.json: the parameter lists of ``construct_box`` and ``copy_file``.

The script also asserts that ``preprocess_fixture.restate`` (one sort, reduceat, a 256-bin count and two order
statistics per object) yields the reference's text on every fixture pair, so the tests may use it in the reference's
place at sizes the reference is too slow for.  Build container only.

    python tests/golden/make_golden_preprocess.py
"""
import importlib
import inspect
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))
from oracle import ref_shim                                              # noqa: E402
import preprocess_fixture as fx                                          # noqa: E402


class _Py3Encoder(json.JSONEncoder):
    def default(self, o):
        if isinstance(o, np.integer):
            return int(o)
        return json.JSONEncoder.default(self, o)


def _json_for_python3():
    shim = types.ModuleType('json')
    shim.__dict__.update({k: v for k, v in json.__dict__.items() if not k.startswith('__')})
    shim.dump = lambda obj, fp, **kw: json.dump(obj, fp, cls=_Py3Encoder, **kw)
    return shim


def _sig(fn):
    return [[p.name, None if p.default is inspect.Parameter.empty else p.default]
            for p in inspect.signature(fn).parameters.values()]


def main():
    sys.dont_write_bytecode = True
    assert ref_shim.available(), 'reference checkout not present'
    sys.path.insert(0, ref_shim.REF)
    ref = importlib.import_module('preprocess_city')
    ref.json = _json_for_python3()
    texts = {}
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, 'gtFine'), os.path.join(d, 'bbox')
        os.makedirs(dst)
        listed = fx.write_tree(src)
        stdout, sys.stdout = sys.stdout, io.StringIO()
        try:
            ref.construct_box(src, fx.INST_PATTERN, fx.CLS_PATTERN, dst)
        finally:
            sys.stdout = stdout
        assert sorted(os.listdir(dst)) == sorted(s + '.json' for s, _, _ in listed)
        for stem, inst, label in listed:
            with open(os.path.join(dst, stem + '.json')) as f:
                texts[stem] = f.read()
            mine = json.dumps(fx.rows_to_info(inst.shape[0], inst.shape[1], fx.restate(inst, label)))
            assert mine == texts[stem], 'the restatement departs from the reference on %s' % stem
    n_obj = {s: len(json.loads(t)['objects']) for s, t in texts.items()}
    with open(os.path.join(HERE, 'preprocess_city.json'), 'w') as f:
        json.dump(texts, f, indent=1, sort_keys=True)
        f.write('\n')
    with open(os.path.join(HERE, 'preprocess_api.json'), 'w') as f:
        json.dump({'signatures': {'construct_box': _sig(ref.construct_box), 'copy_file': _sig(ref.copy_file)}}, f,
                  indent=1, sort_keys=True)
        f.write('\n')
    print('preprocess_city.json: %d files, objects per file %s; the restatement equals the reference on all of them'
          % (len(texts), n_obj))


if __name__ == '__main__':
    main()
