"""tests/golden/vis_api.json and tests/golden/vis_cases.npz.

vis_api.json: the parameter lists of the live reference's util/util.py helpers, of ``util.html.HTML``'s and
``util.visualizer.Visualizer``'s methods; ``labelcolormap(N)`` for N in {2, 8, 35, 36, 49, 151}; the ``loss_log.txt`` line
its ``print_current_errors`` writes for tests/vis_fixture.py's errors.  ``dominate`` and ``scipy.misc`` do not exist
here: stub modules stand in for them (only signatures are read from the two modules that import them).

vis_cases.npz: what ``tensor2im`` / ``tensor2label`` / ``tensor2seglabel`` / ``Colorize`` return for the seeded inputs of
tests/vis_fixture.py.  Outputs only; the inputs are rebuilt from the seeds.  Build container only (oracle/ref_shim.py).

    python tests/golden/make_golden_vis.py
"""
import importlib
import inspect
import io
import json
import os
import sys
import tempfile
import types
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))
from oracle import ref_shim                                              # noqa: E402
import vis_fixture                                                       # noqa: E402


def _sig(fn):
    out = []
    for p in inspect.signature(fn).parameters.values():
        d = None if p.default is inspect.Parameter.empty else p.default
        out.append([p.name, repr(d) if d is not None and not isinstance(d, (int, float, str, bool)) else d])
    return out


def _stubs():
    for name in ('dominate', 'dominate.tags', 'scipy.misc'):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    if 'scipy' not in sys.modules:
        sys.modules['scipy'] = types.ModuleType('scipy')
    sys.modules['scipy'].misc = sys.modules['scipy.misc']
    sys.modules['dominate'].tags = sys.modules['dominate.tags']


def api(util):
    _stubs()
    html = importlib.import_module('util.html')
    vis = importlib.import_module('util.visualizer')
    sigs = {n: _sig(getattr(util, n)) for n in ('tensor2im', 'tensor2label', 'tensor2seglabel', 'labelcolormap',
                                                 'save_image', 'mkdirs', 'mkdir', 'load_script_to_opt')}
    sigs['Colorize.__init__'] = _sig(util.Colorize.__init__)
    sigs['Colorize.__call__'] = _sig(util.Colorize.__call__)
    for m in ('__init__', 'get_image_dir', 'add_header', 'add_table', 'add_images', 'save'):
        sigs['HTML.' + m] = _sig(getattr(html.HTML, m))
    for m in ('__init__', 'display_current_results', 'plot_current_errors', 'print_current_errors', 'save_images'):
        sigs['Visualizer.' + m] = _sig(getattr(vis.Visualizer, m))
    call = vis_fixture.LOG_CALL
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, 'n'))
        opt = types.SimpleNamespace(tf_log=False, isTrain=False, no_html=True, display_winsize=256, name='n',
                                    checkpoints_dir=d)
        v = vis.Visualizer(opt)
        stdout, sys.stdout = sys.stdout, io.StringIO()
        try:
            v.print_current_errors(call['epoch'], call['i'], OrderedDict((k, x) for k, x in call['errors']), call['t'])
        finally:
            sys.stdout = stdout
        with open(os.path.join(d, 'n', 'loss_log.txt')) as f:
            lines = f.read().split('\n')
    assert lines[0].startswith('================ Training Loss (') and lines[-1] == '' and len(lines) == 3
    out = {'signatures': sigs, 'labelcolormap': {str(n): util.labelcolormap(n).tolist() for n in (2, 8, 35, 36, 49, 151)},
           'loss_log_header_prefix': '================ Training Loss (', 'loss_log_header_suffix': ') ================',
           'loss_log_line': lines[1]}
    with open(os.path.join(HERE, 'vis_api.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


def cases(util):
    import torch
    out = {}
    for name, (fn, inp, kw) in vis_fixture.CASES.items():
        if fn == 'Colorize':
            got = util.Colorize(**kw)(torch.from_numpy(inp))
            assert got.dtype == torch.uint8
            out[name] = got.numpy()
            continue
        arg = [torch.from_numpy(a) for a in inp] if isinstance(inp, list) else torch.from_numpy(inp)
        got = getattr(util, fn)(arg, **kw)
        if isinstance(got, list):
            for i, g in enumerate(got):
                out['%s_%d' % (name, i)] = g
        else:
            out[name] = got
    for k, v in out.items():
        assert v.dtype == np.uint8, (k, v.dtype)
    # the rounding-edge case tells the reference's order of operations from the single fused multiply-add
    x = vis_fixture.rounding_edge_values().astype(np.float64)
    fma = np.clip((x * 127.5 + 127.5).astype(np.float32), 0, 255).astype(np.uint8).transpose(1, 2, 0)
    n_fma = int((fma != out['im_edge']).sum())
    assert n_fma > 0, 'the rounding-edge case does not tell the single-FMA form apart'
    two = np.clip((x.astype(np.float32) + np.float32(1)) * np.float32(127.5), 0, 255).astype(np.uint8).transpose(1, 2, 0)
    assert np.array_equal(two, out['im_edge'])
    path = os.path.join(HERE, 'vis_cases.npz')
    np.savez_compressed(path, **out)
    print('vis_cases.npz: %d arrays, %d bytes; single-FMA form differs in %d of %d edge values'
          % (len(out), os.path.getsize(path), n_fma, fma.size))


if __name__ == '__main__':
    ref_shim.install()
    live = importlib.import_module('util.util')
    api(live)
    cases(live)
