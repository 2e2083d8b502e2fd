"""tensor2im / tensor2label / tensor2seglabel on the MI355X: every recorded case of the live reference
(tests/golden/vis_cases.npz) bit for bit, full-size and odd-size tensors against a host restatement of the three formulas
(which must itself reproduce the recorded cases first), no host synchronisation in the device passes, the models'
``get_current_visuals(as_images=True)`` and the loop body of vis_joint_inference.py with this package's classes.
Integer results of exactly specified fp32 steps: no tolerance anywhere."""
import argparse
import json
import os
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch
from PIL import Image

import joint_fixture
import vis_fixture

gpu = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
with open(os.path.join(GOLDEN, 'vis_api.json')) as _f:
    TABLES = {int(n): np.array(t, dtype=np.uint8) for n, t in json.load(_f)['labelcolormap'].items()}


# -- the host restatement of the three formulas (numpy; the colour tables are the recorded reference tables) --------
def ref_tensor2im(x, normalize=True):
    x = np.asarray(x, dtype=np.float32)
    if x.shape[0] == 1:
        x = np.repeat(x, 3, axis=0)
    v = (x + np.float32(1)) / np.float32(2) * np.float32(255) if normalize else x * np.float32(255)
    assert v.dtype == np.float32
    return np.ascontiguousarray(np.clip(v, 0, 255).astype(np.uint8).transpose(1, 2, 0))


def ref_label2color(x, n):
    x = np.asarray(x)
    table = TABLES[n][:n]
    if x.shape[0] > 1:
        lab = np.argmax(x, axis=0).astype(np.int64)          # first = lowest channel of the maximum
        valid = lab < n
    else:
        f = x[0].astype(np.float64)
        valid = (f == np.floor(f)) & (f >= 0) & (f < n)
        lab = np.where(valid, f, 0).astype(np.int64)
    out = np.zeros(lab.shape + (3,), np.uint8)
    out[valid] = table[lab[valid]]
    return out


def ref_seglabel(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32).transpose(1, 2, 0).astype(np.uint8))


def _recorded():
    return np.load(os.path.join(GOLDEN, 'vis_cases.npz'))


def _restate(fn, inp, kw):
    if fn == 'tensor2im' or (fn == 'tensor2label' and kw.get('n_label') == 0):
        return ref_tensor2im(inp, kw.get('normalize', True))
    if fn == 'tensor2label':
        return ref_label2color(inp, kw['n_label'])
    if fn == 'Colorize':
        return ref_label2color(inp, kw['n']).transpose(2, 0, 1)
    return ref_seglabel(inp)


def _check_restatement():
    g = _recorded()
    seen = 0
    for name, (fn, inp, kw) in vis_fixture.CASES.items():
        pairs = [('%s_%d' % (name, i), a) for i, a in enumerate(inp)] if isinstance(inp, list) else [(name, inp)]
        for key, a in pairs:
            got, want = _restate(fn, a, kw), g[key]
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), key
            seen += 1
    assert seen == len(g.files) == 15


def test_host_restatement_reproduces_the_recorded_cases():
    _check_restatement()


@pytest.fixture(scope='module')
def restatement():
    """The full-size tests compare against the restatement: it has to reproduce the live reference first."""
    _check_restatement()


def _util():
    from neurips18_hierchical_image_manipulation_amd.util import util
    return util


def _same(got, want, what=''):
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, \
        (what, getattr(got, 'dtype', None), getattr(got, 'shape', None), want.dtype, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, '%s: %d values differ, first at %s: %r vs %r' % (what, len(bad), bad[0].tolist(),
                                                                         got[tuple(bad[0])], want[tuple(bad[0])])


class _no_sync(object):
    def __enter__(self):
        torch.cuda.set_sync_debug_mode('error')

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(0)


# -- 1. the recorded cases ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name', list(vis_fixture.CASES))
@pytest.mark.parametrize('where', ['device', 'host'])
def test_recorded_case(name, where):
    util = _util()
    g = _recorded()
    fn, inp, kw = vis_fixture.CASES[name]

    def tensor(a):
        t = torch.from_numpy(a)
        return t.to(DEV) if where == 'device' else t

    if fn == 'Colorize':
        got = util.Colorize(**kw)(tensor(inp))
        assert isinstance(got, torch.ByteTensor) and not got.is_cuda
        _same(got.numpy(), g[name], name)
        return
    if isinstance(inp, list):
        got = getattr(util, fn)([tensor(a) for a in inp], **kw)
        assert isinstance(got, list) and len(got) == len(inp)
        for i, p in enumerate(got):
            _same(p, g['%s_%d' % (name, i)], '%s[%d]' % (name, i))
        return
    _same(getattr(util, fn)(tensor(inp), **kw), g[name], name)


# -- 2. full sizes and odd shapes against the restatement -------------------------------------------------------------
def _ids(seed, h, w, hi=41):
    return np.random.RandomState(seed).randint(0, hi, size=(1, h, w))


@gpu
@pytest.mark.parametrize('dtype', ['float32', 'uint8', 'int64'])
def test_id_canvas_full_size(restatement, dtype):
    from neurips18_hierchical_image_manipulation_amd import ops
    ids = _ids(31, 1024, 2048).astype(dtype)
    if dtype == 'float32':
        ids[0, 100, 200:260] += np.float32(0.25)            # non-integer ids stay black
        ids[0, 7, 9] = -1.0
    if dtype == 'int64':
        ids[0, 3, 5], ids[0, 3, 6], ids[0, 3, 7] = -1, 2 ** 32 + 3, 2 ** 40
    t = torch.from_numpy(ids).to(DEV)
    with _no_sync():
        dev = ops.label2color_bytes(t, 35)
    assert dev.dtype == torch.uint8 and dev.is_cuda and tuple(dev.shape) == (1024, 2048, 3)
    _same(dev.cpu().numpy(), ref_label2color(ids, 35), dtype)
    _same(_util().tensor2label(t, 35), ref_label2color(ids, 35), dtype)


@gpu
@pytest.mark.parametrize('shape', [(35, 256, 256), (35, 512, 1024), (35, 129, 257), (35, 33, 65), (2, 1, 1), (151, 5, 3)])
def test_scores_against_restatement(restatement, shape):
    from neurips18_hierchical_image_manipulation_amd import ops
    x = np.random.RandomState(shape[1]).randn(*shape).astype(np.float32)
    x[:, 0, 0] = x[:, 0, 0].max()                           # one all-tie pixel: the lowest channel
    n = {35: 35, 2: 2, 151: 151}[shape[0]]
    t = torch.from_numpy(x).to(DEV)
    with _no_sync():
        dev = ops.label2color_bytes(t, n)
    _same(dev.cpu().numpy(), ref_label2color(x, n), str(shape))
    # more score channels than table rows: the upper channels are out of range -> black
    if shape[0] == 35:
        _same(_util().tensor2label(t, 8), ref_label2color(x, 8), 'n=8 %s' % (shape,))


@gpu
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('shape', [(3, 1024, 2048), (3, 33, 65), (1, 1, 1), (3, 1, 1), (1, 129, 257), (3, 2, 2)])
def test_image_against_restatement(restatement, shape, normalize):
    from neurips18_hierchical_image_manipulation_amd import ops
    lo, hi = (-1.2, 1.2) if normalize else (-0.1, 1.1)
    x = np.random.RandomState(shape[2] + normalize).uniform(lo, hi, size=shape).astype(np.float32)
    edge = vis_fixture.rounding_edge_values().reshape(-1)
    k = min(edge.size, x.size)
    x.reshape(-1)[:k] = edge[:k] if normalize else (edge[:k] + np.float32(1)) / np.float32(2)
    t = torch.from_numpy(x).to(DEV)
    with _no_sync():
        dev = ops.tensor2im_bytes(t, normalize)
    assert dev.dtype == torch.uint8 and tuple(dev.shape) == (shape[1], shape[2], 3)
    _same(dev.cpu().numpy(), ref_tensor2im(x, normalize), str(shape))
    _same(_util().tensor2im(t, np.uint8, normalize), ref_tensor2im(x, normalize), str(shape))


@gpu
@pytest.mark.parametrize('shape', [(1, 33, 65), (2, 9, 11), (3, 64, 96), (4, 16, 16), (7, 5, 13), (3, 1, 1), (19, 32, 32)])
def test_seglabel_against_restatement(restatement, shape):
    from neurips18_hierchical_image_manipulation_amd import ops
    x = np.random.RandomState(sum(shape)).uniform(0, 255.999, size=shape).astype(np.float32)
    x.reshape(-1)[:2] = (0.0, 255.0)
    t = torch.from_numpy(x).to(DEV)
    with _no_sync():
        dev = ops.seglabel_bytes(t)
    assert tuple(dev.shape) == (shape[1], shape[2], shape[0])
    _same(dev.cpu().numpy(), ref_seglabel(x), str(shape))
    _same(_util().tensor2seglabel(t), ref_seglabel(x), str(shape))


@gpu
def test_non_contiguous_and_misaligned_inputs(restatement):
    from neurips18_hierchical_image_manipulation_amd import ops
    rs = np.random.RandomState(5)
    batch = rs.uniform(-1, 1, size=(2, 5, 40, 52)).astype(np.float32)
    t = torch.from_numpy(batch).to(DEV)
    _same(ops.tensor2im_bytes(t[1, 1:4]).cpu().numpy(), ref_tensor2im(batch[1, 1:4]), 'channel slice')
    _same(ops.tensor2im_bytes(t[0][:3]).cpu().numpy(), ref_tensor2im(batch[0, :3]), '[0] slice')
    _same(ops.tensor2im_bytes(t[0, :3, ::2, 1::3]).cpu().numpy(), ref_tensor2im(batch[0, :3, ::2, 1::3]), 'strided')
    _same(ops.label2color_bytes(t[1], 8).cpu().numpy(), ref_label2color(batch[1], 8), 'scores [1]')
    # a contiguous view that starts 4 bytes past a 16-byte boundary: the element-load path
    flat = torch.from_numpy(rs.uniform(-1, 1, size=(1 + 3 * 8 * 12,)).astype(np.float32)).to(DEV)
    view = flat[1:].view(3, 8, 12)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    _same(ops.tensor2im_bytes(view).cpu().numpy(), ref_tensor2im(view.cpu().numpy()), 'misaligned')
    _same(ops.label2color_bytes(view, 8).cpu().numpy(), ref_label2color(view.cpu().numpy(), 8), 'misaligned scores')
    _same(ops.seglabel_bytes(view.abs() * 200).cpu().numpy(), ref_seglabel((view.abs() * 200).cpu().numpy()), 'seg')


@gpu
def test_runs_on_the_current_stream_only(restatement):
    """A side stream's passes are ordered behind that stream's producer, and the host copy waits for that stream."""
    x = np.random.RandomState(8).uniform(-1, 1, size=(3, 256, 512)).astype(np.float32)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.from_numpy(x).pin_memory().to(DEV, non_blocking=True)
        got = _util().tensor2im(t)
        lab = _util().tensor2label(t, 49)
    _same(got, ref_tensor2im(x), 'side stream')
    _same(lab, ref_label2color(x, 49), 'side stream label')


# -- 3. LabelCond -----------------------------------------------------------------------------------------------------
@gpu
def test_labelcond_is_coloured_from_its_ids(restatement):
    from neurips18_hierchical_image_manipulation_amd import ops
    ids = _ids(41, 64, 96, 35).astype(np.float32)
    label = torch.from_numpy(ids[None]).to(DEV)
    edges = (torch.rand(1, 1, 64, 96, device=DEV) > 0.8).float()
    for dense in (None, edges):
        cond = ops.LabelCond(label, 35, dense)
        with _no_sync():
            got = ops.label2color_bytes(cond, 35)
        assert cond._full is None and cond._pooled is None and not cond._made      # nothing was materialised
        _same(got.cpu().numpy(), ref_label2color(ids, 35), 'LabelCond')
        _same(_util().tensor2label(cond, 35), ref_label2color(ids, 35), 'LabelCond via util')
        assert cond._full is None
        full = cond.full()[0]
        assert tuple(full.shape) == (35 + (0 if dense is None else 1), 64, 96)
        assert torch.equal(ops.label2color_bytes(full, 35), got)
    # the table of an n_label is uploaded once per device and reused
    dev = torch.cuda.current_device()
    assert ops._COLOR_TABLES[(dev, 35)][0].data_ptr() == ops._color_table(label.device, 35).data_ptr()


# -- 4. the models ----------------------------------------------------------------------------------------------------
KEYS = ['input_label', 'input_image', 'real_image', 'synthesized_image']


def _check_visuals(model, label_nc, H, W):
    util = _util()
    plain = model.get_current_visuals()
    assert list(plain.keys()) == KEYS
    for k, v in plain.items():
        assert torch.is_tensor(v) and not v.is_cuda and v.dtype == torch.float32 and tuple(v.shape[1:]) == (H, W), k
    assert plain['input_label'].shape[0] >= label_nc and plain['synthesized_image'].shape[0] == 3
    images = model.get_current_visuals(as_images=True)
    assert list(images.keys()) == KEYS
    want = OrderedDict([('input_label', ref_label2color(plain['input_label'].numpy(), label_nc))] +
                       [(k, ref_tensor2im(plain[k].numpy())) for k in KEYS[1:]])
    for k in KEYS:
        _same(images[k], want[k], k)
    _same(util.tensor2label(plain['input_label'], label_nc), want['input_label'], 'tensor2label of the float tensor')
    _same(util.tensor2im(plain['synthesized_image']), want['synthesized_image'], 'tensor2im of the float tensor')
    assert len(np.unique(images['input_label'].reshape(-1, 3), axis=0)) > 3      # a real label picture, not a blank


@gpu
@pytest.mark.parametrize('no_instance', [True, False])
def test_get_current_visuals_as_images(tmp_path, restatement, no_instance):
    from neurips18_hierchical_image_manipulation_amd import synth
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    flags = dict(model='pix2pixHD_condImg', netG='global', ngf=16, ndf=8, n_downsample_global=2, n_blocks_global=1,
                 num_D=1, n_layers_D=2, label_nc=35, no_instance=no_instance, no_vgg_loss=True)
    torch.manual_seed(3)
    model = create_model(dict(flags, gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp_path), name='v'))
    batch = synth.make_batch(0, 0, 2, 32, 64)
    model.optimize_parameters(batch)
    _check_visuals(model, 35, 32, 64)
    fake = model.inference(batch['label'], batch['inst'], batch['image'], batch['mask_in'], batch['mask_out'])
    assert tuple(fake.shape) == (2, 3, 32, 64)
    _check_visuals(model, 35, 32, 64)
    _same(model.get_current_visuals(as_images=True)['synthesized_image'], ref_tensor2im(fake[0].cpu().numpy()), 'fake')


# -- 5. the loop body of vis_joint_inference.py -----------------------------------------------------------------------
@gpu
def test_joint_inference_result_page(tmp_path, restatement):
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    from neurips18_hierchical_image_manipulation_amd.models.joint_inference_model import JointInference
    from neurips18_hierchical_image_manipulation_amd.options import BoxToMaskTestOptions, MaskToImageTestOptions
    from neurips18_hierchical_image_manipulation_amd.util import html
    from neurips18_hierchical_image_manipulation_amd.util.util import load_script_to_opt
    from neurips18_hierchical_image_manipulation_amd.util.visualizer import Visualizer
    util = _util()
    fs = 64
    b2m = joint_fixture.with_flags(joint_fixture.BOX2MASK_FLAGS, fineSize=fs, checkpoints_dir=str(tmp_path))
    m2i = joint_fixture.with_flags(joint_fixture.MASK2IMAGE_FLAGS, fineSize=fs, checkpoints_dir=str(tmp_path), ngf=16)
    sb, sm = joint_fixture.script_pair(str(tmp_path), True, b2m, m2i)
    for path, cls, extra in ((sb, BoxToMaskTestOptions, dict(use_gan=True)), (sm, MaskToImageTestOptions, {})):
        torch.manual_seed(12)
        m = create_model(dict(vars(load_script_to_opt(path, cls)), isTrain=True, **extra))
        if cls is BoxToMaskTestOptions:
            m.netG.load_state_dict(joint_fixture.box2mask_state(m.netG.state_dict(), 31))
        m.save('latest')
    model = JointInference(argparse.Namespace(maskgen_script=sb, imggen_script=sm, gpu_ids=[0]))
    opt_maskgen, opt_pix2pix = model.opt_maskgen, model.opt_imggen
    visualizer = Visualizer(opt_maskgen)
    web_dir = os.path.join(str(tmp_path), 'results', 'test_joint_inference', 'val')
    webpage = html.HTML(web_dir, 'Experiment = %s, Phase = %s' % ('Joint Inference', 'val'))
    handed = []
    names = ['input_image_patch', 'predicted_label_patch', 'predicted_image_patch', 'GT_label_canvas',
             'predicted_label_canvas', 'GT_image_canvas', 'predicted_image_canvas']
    for i, case in enumerate(('interior', 'edge')):
        c = joint_fixture.CASES[case]
        label, photo = joint_fixture.canvases(c['seed'])
        label_orig, img_orig = torch.from_numpy(label).to(DEV), torch.from_numpy(photo).to(DEV)
        np.random.seed(c['seed'])
        random.seed(c['seed'])
        layout, layout_dict, _ = model.gen_layout(c['bbox'], label_orig, opt_maskgen)
        image, test_dict, img_generated = model.gen_image(c['bbox'], img_orig, layout, opt_pix2pix)
        visuals = OrderedDict([
            ('input_image_patch', util.tensor2im(test_dict['image'][0])),
            ('predicted_label_patch', util.tensor2label(test_dict['label'][0], opt_maskgen.label_nc)),
            ('predicted_image_patch', util.tensor2im(img_generated[0])),
            ('GT_label_canvas', util.tensor2label(label_orig[0], opt_maskgen.label_nc)),
            ('predicted_label_canvas', util.tensor2label(layout[0], opt_maskgen.label_nc)),
            ('GT_image_canvas', util.tensor2im(img_orig[0], normalize=False)),
            ('predicted_image_canvas', util.tensor2im(image[0], normalize=False))])
        visualizer.save_images(webpage, visuals, ['%05d' % i])
        want = OrderedDict([
            ('input_image_patch', ref_tensor2im(test_dict['image'][0].cpu().numpy())),
            ('predicted_label_patch', ref_label2color(test_dict['label'][0].cpu().numpy(), 35)),
            ('predicted_image_patch', ref_tensor2im(img_generated[0].cpu().numpy())),
            ('GT_label_canvas', ref_label2color(label[0], 35)),
            ('predicted_label_canvas', ref_label2color(layout[0].cpu().numpy(), 35)),
            ('GT_image_canvas', ref_tensor2im(photo[0], False)),
            ('predicted_image_canvas', ref_tensor2im(image[0].cpu().numpy(), False))])
        assert list(visuals) == names
        for k in names:
            _same(visuals[k], want[k], '%s %s' % (case, k))
        assert visuals['predicted_label_canvas'].shape == (1024, 2048, 3) and visuals['input_image_patch'].shape == (fs, fs, 3)
        assert (visuals['predicted_label_canvas'] != visuals['GT_label_canvas']).any()        # the edit shows
        handed.append(visuals)
    webpage.save()
    with open(os.path.join(web_dir, 'index.html')) as f:
        text = f.read()
    at = -1
    for i, visuals in enumerate(handed):
        for k in names:
            rel = 'images/%05d_%s.jpg' % (i, k)
            assert text.count('href="%s"' % rel) == 1 and text.count('src="%s"' % rel) == 1
            assert text.index(rel) > at
            at = text.index(rel)
            with Image.open(os.path.join(web_dir, rel)) as im:
                assert im.size == visuals[k].shape[1::-1] and im.mode == 'RGB'
    assert sorted(os.listdir(os.path.join(web_dir, 'images'))) == sorted('%05d_%s.jpg' % (i, k) for i in range(2) for k in names)
    assert text.count('<h3>') == 2 and '<h3>00000</h3>' in text and '<h3>00001</h3>' in text
