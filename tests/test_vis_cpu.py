"""Host side of the visualisation path: the reference's signatures and colour tables (tests/golden/vis_api.json, recorded
from the live reference by tests/golden/make_golden_vis.py), the Visualizer's files / page / log line, the HTML writer,
and the C ABI's declarations.  Nothing here touches the device: the pictures handed in are numpy arrays."""
import argparse
import inspect
import json
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
from PIL import Image

import vis_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'vis_api.json')) as _f:
    API = json.load(_f)


def _modules():
    from neurips18_hierchical_image_manipulation_amd.util import html, util, visualizer
    return util, html, visualizer


def test_signatures_follow_the_reference():
    util, html, visualizer = _modules()
    assert len(API['signatures']) == 21
    for name, params in API['signatures'].items():
        if '.' in name:
            cls, meth = name.split('.')
            fn = getattr({'Colorize': util.Colorize, 'HTML': html.HTML, 'Visualizer': visualizer.Visualizer}[cls], meth)
        else:
            fn = getattr(util, name)
        mine = inspect.signature(fn).parameters
        names = list(mine)
        assert names[:len(params)] == [p[0] for p in params], '%s%s: here %s' % (name, params, names)
        for pname, default in params:
            d = mine[pname].default
            if default is None:
                assert d is inspect.Parameter.empty, (name, pname)
            elif isinstance(default, str) and default.startswith('<class'):
                assert repr(d) == default, (name, pname, d)
            else:
                assert d == default and type(d) is type(default), (name, pname, d)
        for extra in names[len(params):]:          # appended parameters are optional
            assert mine[extra].default is not inspect.Parameter.empty, (name, extra)


@pytest.mark.parametrize('n', [2, 8, 35, 36, 49, 151])
def test_labelcolormap_equals_the_reference_tables(n):
    util, _, _ = _modules()
    got = util.labelcolormap(n)
    want = np.array(API['labelcolormap'][str(n)], dtype=np.uint8)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


def test_colorize_keeps_the_first_n_rows():
    import torch
    util, _, _ = _modules()
    c = util.Colorize(35)
    assert c.cmap.dtype == torch.uint8 and tuple(c.cmap.shape) == (35, 3)
    assert np.array_equal(c.cmap.numpy(), np.array(API['labelcolormap']['35'], dtype=np.uint8)[:35])
    assert tuple(util.Colorize().cmap.shape) == (35, 3) and tuple(util.Colorize(8).cmap.shape) == (8, 3)


def _opt(d, **over):
    return argparse.Namespace(**dict(dict(tf_log=False, isTrain=True, no_html=False, display_winsize=256, name='exp',
                                          checkpoints_dir=str(d)), **over))


def _picture(seed, h=12, w=20):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _page(path):
    """(headers, rows) of an index.html: rows = per table, the (href, src, width, text) of its cells, in page order."""
    with open(path) as f:
        text = f.read()
    headers = re.findall(r'<h3>(.*?)</h3>', text)
    rows = []
    for table in re.findall(r'<table.*?</table>', text, flags=re.S):
        assert len(re.findall(r'<tr>', table)) == 1
        rows.append(re.findall(r'<a href="([^"]*)"><img style="width:(\d+)px" src="([^"]*)"></a>.*?<p>(.*?)</p>', table,
                               flags=re.S))
    return text, headers, rows


def test_print_current_errors_appends_the_reference_line(tmp_path, capsys):
    _, _, visualizer = _modules()
    os.makedirs(os.path.join(str(tmp_path), 'exp'))
    v = visualizer.Visualizer(_opt(tmp_path, isTrain=False))
    call = vis_fixture.LOG_CALL
    v.print_current_errors(call['epoch'], call['i'], OrderedDict((k, x) for k, x in call['errors']), call['t'])
    with open(os.path.join(str(tmp_path), 'exp', 'loss_log.txt')) as f:
        lines = f.read().split('\n')
    assert len(lines) == 3 and lines[2] == ''
    assert lines[0].startswith(API['loss_log_header_prefix']) and lines[0].endswith(API['loss_log_header_suffix'])
    assert lines[1] == API['loss_log_line']
    assert API['loss_log_line'] in capsys.readouterr().out
    assert 'G_GAN_Feat' not in lines[1]                        # the zero entry is left out
    assert v.plot_current_errors({'G_GAN': 1.0}, 5) is None
    assert not os.path.exists(os.path.join(str(tmp_path), 'exp', 'web'))      # isTrain=False: no page


def test_no_html_flag_and_tf_log(tmp_path):
    _, _, visualizer = _modules()
    os.makedirs(os.path.join(str(tmp_path), 'exp'))
    v = visualizer.Visualizer(_opt(tmp_path, no_html=True))
    v.display_current_results(OrderedDict([('a', _picture(0))]), 1, 10)
    assert not os.path.exists(os.path.join(str(tmp_path), 'exp', 'web'))
    with pytest.raises(NotImplementedError, match='TensorFlow 1'):
        visualizer.Visualizer(_opt(tmp_path, tf_log=True))


def test_display_current_results_writes_files_and_page(tmp_path):
    _, _, visualizer = _modules()
    os.makedirs(os.path.join(str(tmp_path), 'exp'))
    v = visualizer.Visualizer(_opt(tmp_path))
    web = os.path.join(str(tmp_path), 'exp', 'web')
    assert os.path.isdir(os.path.join(web, 'images'))
    visuals = OrderedDict([('input_label', _picture(1)), ('pyramid', [_picture(2, 6, 10), _picture(3, 3, 5)]),
                           ('synthesized_image', _picture(4))])
    for epoch in (1, 2):
        v.display_current_results(visuals, epoch, epoch * 100)
    names = ['epoch%.3d_input_label.jpg', 'epoch%.3d_pyramid_0.jpg', 'epoch%.3d_pyramid_1.jpg',
             'epoch%.3d_synthesized_image.jpg']
    sizes = [(20, 12), (10, 6), (5, 3), (20, 12)]
    for epoch in (1, 2):
        for n, size in zip(names, sizes):
            with Image.open(os.path.join(web, 'images', n % epoch)) as im:
                assert im.size == size and im.format == 'JPEG'
    text, headers, rows = _page(os.path.join(web, 'index.html'))
    assert '<meta content="5" http-equiv="refresh">' in text and 'Experiment name = exp' in text
    assert headers == ['epoch [2]', 'epoch [1]'] and len(rows) == 2
    for epoch, row in zip((2, 1), rows):
        assert [c[0] for c in row] == ['images/' + n % epoch for n in names]
        assert [c[2] for c in row] == [c[0] for c in row] and all(c[1] == '256' for c in row)
        assert [c[3] for c in row] == ['input_label', 'pyramid0', 'pyramid1', 'synthesized_image']
        for c in row:
            assert os.path.isfile(os.path.join(web, c[0])) and os.path.isfile(os.path.join(web, c[2]))


def test_display_current_results_splits_ten_or_more(tmp_path):
    _, _, visualizer = _modules()
    os.makedirs(os.path.join(str(tmp_path), 'exp'))
    v = visualizer.Visualizer(_opt(tmp_path))
    web = os.path.join(str(tmp_path), 'exp', 'web')
    visuals = OrderedDict(('v%02d' % i, _picture(10 + i, 4, 6)) for i in range(11))
    v.display_current_results(visuals, 1, 1)
    _, headers, rows = _page(os.path.join(web, 'index.html'))
    assert headers == ['epoch [1]'] and [len(r) for r in rows] == [6, 5]        # int(round(11 / 2.0)) = 6
    assert [c[0] for r in rows for c in r] == ['images/epoch001_v%02d.jpg' % i for i in range(11)]
    assert all(os.path.isfile(os.path.join(web, c[0])) for r in rows for c in r)
    v.display_current_results(OrderedDict(list(visuals.items())[:9]), 1, 2)
    assert [len(r) for r in _page(os.path.join(web, 'index.html'))[2]] == [9]


def test_save_images_and_html(tmp_path):
    _, html, visualizer = _modules()
    os.makedirs(os.path.join(str(tmp_path), 'exp'))
    v = visualizer.Visualizer(_opt(tmp_path, isTrain=False, display_winsize=300))
    web = os.path.join(str(tmp_path), 'results', 'val')
    page = html.HTML(web, 'Experiment = <Joint & Co>, Phase = val')
    assert page.get_image_dir() == os.path.join(web, 'images') and os.path.isdir(page.get_image_dir())
    for i in range(2):
        visuals = OrderedDict([('input_image_patch', _picture(i)), ('predicted_label_canvas', _picture(5 + i, 16, 32))])
        v.save_images(page, visuals, ['/data/val/%05d.png' % i])
    page.add_header('a < b')
    page.save()
    text, headers, rows = _page(os.path.join(web, 'index.html'))
    assert 'http-equiv' not in text                                            # refresh = 0
    assert '<title>Experiment = &lt;Joint &amp; Co&gt;, Phase = val</title>' in text
    assert headers == ['00000', '00001', 'a &lt; b'] and len(rows) == 2
    for i, row in enumerate(rows):
        assert [c[0] for c in row] == ['images/%05d_input_image_patch.jpg' % i, 'images/%05d_predicted_label_canvas.jpg' % i]
        assert [c[3] for c in row] == ['input_image_patch', 'predicted_label_canvas'] and all(c[1] == '300' for c in row)
        for c, size in zip(row, [(20, 12), (32, 16)]):
            assert c[2] == c[0]
            with Image.open(os.path.join(web, c[0])) as im:
                assert im.size == size
    assert text.index('<h3>00000</h3>') < text.index('00000_input_image_patch') < text.index('<h3>00001</h3>')


def test_html_defaults(tmp_path):
    _, html, _ = _modules()
    page = html.HTML(os.path.join(str(tmp_path), 'w'), 't', refresh=7)
    page.add_images(['a.jpg'], ['x & y'], ['b.jpg'])
    page.save()
    text, _, rows = _page(os.path.join(str(tmp_path), 'w', 'index.html'))
    assert rows == [[('images/b.jpg', '512', 'images/a.jpg', 'x &amp; y')]]
    assert '<meta content="7" http-equiv="refresh">' in text and '<table border="1"' in text


def test_save_image_and_mkdirs(tmp_path):
    util, _, _ = _modules()
    a, b = os.path.join(str(tmp_path), 'a', 'b'), os.path.join(str(tmp_path), 'c')
    util.mkdirs([a, b])
    util.mkdirs(a)
    util.mkdir(b)
    assert os.path.isdir(a) and os.path.isdir(b)
    pic = _picture(9)
    util.save_image(pic, os.path.join(a, 'p.png'))
    with Image.open(os.path.join(a, 'p.png')) as im:
        assert np.array_equal(np.asarray(im), pic)


def test_header_declares_and_cabi_lists_the_entry_points():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        header = f.read()
    for name in ('him_tensor2im_bytes', 'him_label2color_bytes', 'him_seglabel_bytes'):
        assert re.search(r'^int %s\(' % name, header, flags=re.M), name
        assert name in _cabi.EXPORTS


def test_converters_refuse_what_the_kernels_do_not_take():
    """Argument checks run before anything touches the device."""
    import torch
    from neurips18_hierchical_image_manipulation_amd import ops
    for bad in (torch.zeros(2, 4, 4), torch.zeros(4, 4), torch.zeros(1, 3, 4, 4), torch.zeros(3, 4, 4, dtype=torch.float64),
                torch.zeros(3, 0, 4)):
        with pytest.raises(ValueError):
            ops.tensor2im_bytes(bad)
    with pytest.raises(ValueError):
        ops.label2color_bytes(torch.zeros(4, 4), 35)
    with pytest.raises(ValueError):
        ops.label2color_bytes(torch.zeros(1, 4, 4, dtype=torch.int32), 35)
    with pytest.raises(ValueError):
        ops.label2color_bytes(torch.zeros(5, 4, 4, dtype=torch.int64), 35)
    with pytest.raises(ValueError):
        ops.seglabel_bytes(torch.zeros(4, 4))
