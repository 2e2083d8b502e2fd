"""tests/golden/preprocess_ade.json and tests/golden/preprocess_ade.npz.

The live reference's ``preprocess_ade.py`` is run, as a script, on the golden cases of tests/preprocess_ade_fixture.py
(a raw tree fabricated in a temporary directory: ``.jpg``, ``_seg.png``, ``_atr.txt`` files and an ``index_ade20k.mat``).
The script is Python 2; three things are handed to it so that it runs here with Python 2's results:

* the three ``/`` that Python 2 evaluates as integer divisions are replaced by ``//`` (each text must occur exactly once;
  the texts and their match counts are recorded);
* a ``scipy.misc`` whose ``imread`` is ``np.array(Image.open(path))`` (SciPy removed its own);
* an ``imageio`` whose ``imwrite`` writes ``floor(a * 255 + 0.499999999)`` as bytes through Pillow (imageio's
  conversion of a float plane in [0, 1]).

Nothing is written into the reference's tree (``sys.dont_write_bytecode``) and none of its text is kept.

preprocess_ade.json: the JSON text of every box file, the output file names per folder, the reference's ``sorted_50`` and
the substitutions.  preprocess_ade.npz: the decoded label and instance PNGs.  The script also asserts that the fixture's
``restate`` / ``rows_to_info`` yield the reference's planes and texts on every case.  Build container only.

    python tests/golden/make_golden_preprocess_ade.py
"""
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))
from oracle import ref_shim                                              # noqa: E402
import preprocess_ade_fixture as fx                                      # noqa: E402

SUBSTITUTIONS = [("R.astype('uint16') / 10", "R.astype('uint16') // 10"),
                 ('round(w / 100)', 'round(w // 100)'),
                 ('round(h / 100)', 'round(h // 100)')]
FOLDERS = ['%s_%s' % (p, s) for p in ('train', 'val') for s in ('bbox', 'img', 'label', 'inst')]


def _stubs():
    import scipy
    misc = types.ModuleType('scipy.misc')
    misc.imread = lambda path: np.array(Image.open(path))
    imageio = types.ModuleType('imageio')

    def imwrite(path, a):
        Image.fromarray(np.floor(np.asarray(a) * 255 + 0.499999999).astype(np.uint8)).save(path)
    imageio.imwrite = imwrite
    sys.modules['scipy.misc'] = misc
    scipy.misc = misc
    sys.modules['imageio'] = imageio


def run_reference(workdir):
    """Execute the reference script with ``__name__ == '__main__'`` from ``workdir`` (which holds datasets/ade20k/);
    returns its globals and the substitution record."""
    with open(os.path.join(ref_shim.REF, 'preprocess_ade.py')) as f:
        text = f.read()
    record = []
    for old, new in SUBSTITUTIONS:
        n = text.count(old)
        assert n == 1, '%r occurs %d times in the reference script' % (old, n)
        text = text.replace(old, new)
        record.append({'old': old, 'new': new, 'matches': n})
    _stubs()
    scope = {'__name__': '__main__'}
    cwd, stdout = os.getcwd(), sys.stdout
    os.chdir(workdir)
    sys.stdout = io.StringIO()
    try:
        exec(compile(text, 'preprocess_ade.py', 'exec'), scope)
    finally:
        sys.stdout = stdout
        os.chdir(cwd)
    return scope, record


def main():
    sys.dont_write_bytecode = True
    assert ref_shim.available(), 'reference checkout not present'
    cases = fx.golden_cases()
    names = fx.objectnames()
    gold, planes = {'json': {}, 'files': {}}, {}
    with tempfile.TemporaryDirectory() as d:
        root = os.path.join(d, 'datasets', 'ade20k')
        listed = fx.write_raw_tree(root, cases)
        scope, gold['substitutions'] = run_reference(d)
        gold['sorted_50'] = [int(k) for k in scope['sorted_50']]
        assert gold['sorted_50'] == list(fx.KEEP), 'the package keeps other classes than the reference'
        for folder in FOLDERS:
            gold['files'][folder] = sorted(os.listdir(os.path.join(root, folder)))
        assert all(len(gold['files']['val_' + s]) == len(cases) for s in ('bbox', 'img', 'label', 'inst'))
        for i, ((tag, seg, lines), (jpg, _, _)) in enumerate(zip(cases, listed)):
            prefix = 'bedroom_%05d' % (i + 1)
            with open(os.path.join(root, 'val_bbox', prefix + '_gtFine_instanceIds.json')) as f:
                gold['json'][prefix] = f.read()
            label = np.array(Image.open(os.path.join(root, 'val_label', prefix + '_gtFine_labelIds.png')))
            inst = np.array(Image.open(os.path.join(root, 'val_inst', prefix + '_gtFine_instanceIds.png')))
            with open(jpg, 'rb') as f, open(os.path.join(root, 'val_img', prefix + '_leftImg8bit.png'), 'rb') as g:
                assert f.read() == g.read()
            _, my_label, my_inst, rows = fx.restate(seg)
            assert label.dtype == np.uint8 and np.array_equal(label, my_label), 'label planes differ on %s' % tag
            assert inst.dtype == np.uint8 and np.array_equal(inst, my_inst), 'instance planes differ on %s' % tag
            mine = json.dumps(fx.rows_to_info(seg.shape[0], seg.shape[1], rows, fx.names_of(lines), names))
            assert mine == gold['json'][prefix], 'the restatement departs from the reference on %s:\n%s\n%s' % (
                tag, mine, gold['json'][prefix])
            planes['label_' + prefix], planes['inst_' + prefix] = label, inst
    gold['cases'] = [tag for tag, _, _ in cases]
    with open(os.path.join(HERE, 'preprocess_ade.json'), 'w') as f:
        json.dump(gold, f, indent=1, sort_keys=True)
        f.write('\n')
    np.savez_compressed(os.path.join(HERE, 'preprocess_ade.npz'), **planes)
    print('preprocess_ade.json: %d cases, objects per file %s; the restatement equals the reference on all of them'
          % (len(cases), {p: len(json.loads(t)['objects']) for p, t in gold['json'].items()}))


if __name__ == '__main__':
    main()
