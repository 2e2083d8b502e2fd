"""Joint box -> layout -> image edit on the MI355X: the resize-and-compose kernel of evaluate(target_size) against torch
CPU, the canvas crop / paste against Pillow (the reference's crop_canvas / paste_canvas are ToPILImage -> Image.crop ->
Image.resize -> ToTensor), and the public JointInference path built from script files and checkpoints."""
import argparse
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import joint_fixture
from neurips18_hierchical_image_manipulation_amd import ops
from neurips18_hierchical_image_manipulation_amd.models import create_model
from neurips18_hierchical_image_manipulation_amd.models.joint_inference_model import JointInference
from neurips18_hierchical_image_manipulation_amd.options import BoxToMaskTestOptions, MaskToImageTestOptions
from neurips18_hierchical_image_manipulation_amd.util import data_util
from neurips18_hierchical_image_manipulation_amd.util.util import load_script_to_opt

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# -- host references ------------------------------------------------------------------------------------------------
def to_pil_bytes(planes, pre=0):
    """ToPILImage of (C,H,W) fp32 host planes: mul(255).byte() in fp32 (after /255 or (v+1)/2)."""
    v = planes.astype(np.float32)
    if pre == 1:
        v = v / np.float32(255)
    elif pre == 2:
        v = (v + np.float32(1)) / np.float32(2)
    b = (v * np.float32(255)).astype(np.int32).astype(np.uint8)
    return b[0] if b.shape[0] == 1 else np.ascontiguousarray(b.transpose(1, 2, 0))


def pil_resize(b, box, size, method):
    im = Image.fromarray(b, 'L' if b.ndim == 2 else 'RGB')
    if box is not None:
        im = im.crop(box)
    return np.asarray(im.resize(size, method))


def compose_ref(comb, obj, label, mask, cls, background, align):
    """Reference TwoStreamAE_mask.py:318-335 on the CPU: upsample, then compose."""
    H, W = label.shape[-2:]
    if not background:
        p = F.interpolate(obj, size=(H, W), mode='bilinear', align_corners=align)
        return torch.where(p > 0.5, torch.full_like(label, float(cls)), label), (p - 0.5).abs()
    p = F.interpolate(comb, size=(H, W), mode='bilinear', align_corners=align)
    onehot = F.one_hot(label.long()[:, 0], comb.shape[1]).permute(0, 3, 1, 2).float()
    blend = p * mask + (1 - mask) * onehot
    top2 = blend.topk(2, dim=1).values
    return blend.max(1, keepdim=True)[1], (top2[:, 0:1] - top2[:, 1:2])


# -- 1. resize-and-compose ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('align', [False, True])
@pytest.mark.parametrize('lo,hi', [((16, 16), (37, 23)), ((64, 64), (29, 51)), ((8, 8), (1, 1)), ((32, 32), (97, 64)),
                                   ((64, 64), (64, 64))])
@pytest.mark.parametrize('background', [False, True])
def test_resize_compose_matches_torch(lo, hi, align, background):
    g = torch.Generator().manual_seed(hash((lo, hi, align, background)) % 1000)
    C = 35
    comb = torch.softmax(torch.randn(1, C, *lo, generator=g) * 3, 1)
    obj = torch.rand(1, 1, *lo, generator=g)
    label = torch.randint(0, C, (1, 1, *hi), generator=g).float()
    mask = torch.zeros(1, 1, *hi)
    mask[..., hi[0] // 4:hi[0] - hi[0] // 4 + 1, hi[1] // 5:] = 1
    cls = C - 1 if background else 26
    got = ops.resize_compose(comb.to(DEV), obj.to(DEV), label.to(DEV), mask.to(DEV), cls, background, align).cpu()
    want, margin = compose_ref(comb, obj, label, mask, cls, background, align)
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape)
    sure = margin > 1e-5
    assert bool((got[sure] == want[sure]).all())
    assert int(sure.sum()) >= 0.95 * got.numel()


# -- 2. canvas crop -------------------------------------------------------------------------------------------------
def _canvases(H, W, seed=0):
    rs = np.random.RandomState(seed)
    label = rs.randint(0, 35, size=(H // 8 + 1, W // 8 + 1)).repeat(8, 0).repeat(8, 1)[:H, :W].astype(np.float32)
    photo = rs.randint(0, 256, size=(3, H, W)).astype(np.float32) / np.float32(255)
    return label[None, None], photo[None]


@pytest.mark.parametrize('box', [(40, 20, 141, 95), (-13, -7, 60, 50), (150, 80, 230, 131), (0, 0, 200, 120)])
def test_canvas_crop_bit_exact_vs_pillow(box):
    label, photo = _canvases(120, 200)
    got_l = ops.canvas_crop_nearest(torch.from_numpy(label).to(DEV), box, 64, 64, pre=1).cpu().numpy()
    want_l = pil_resize(to_pil_bytes(label[0], 1), box, (64, 64), Image.NEAREST).astype(np.float32)
    assert np.array_equal(got_l[0, 0], want_l)
    got_p = ops.canvas_crop_bicubic(torch.from_numpy(photo).to(DEV), box, 64, 64, normalize=True).cpu().numpy()
    want_p = pil_resize(to_pil_bytes(photo[0]), box, (64, 64), Image.BICUBIC).transpose(2, 0, 1).astype(np.float32)
    want_p = ((want_p / np.float32(255)) - np.float32(0.5)) / np.float32(0.5)
    assert np.array_equal(got_p[0], want_p)


class _Opt(argparse.Namespace):
    pass


def _opt(fs=64, margin=2.0):
    return _Opt(fineSize=fs, contextMargin=margin, resize_or_crop='select_region', isTrain=False, no_flip=False)


def test_crop_canvas_matches_pillow_and_draws_like_upstream():
    label, photo = _canvases(1024, 2048, 1)
    lab, ph = torch.from_numpy(label).to(DEV), torch.from_numpy(photo).to(DEV)
    bbox = {'cls': 26, 'bbox': [1900, 900, 2040, 1010]}
    np.random.seed(3)
    random.seed(3)
    torch.cuda.set_sync_debug_mode('error')
    try:
        d = data_util.crop_canvas(bbox, lab, _opt(), img_original=ph, transform_img=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    after = (np.random.uniform(), random.random())
    np.random.seed(3)
    random.seed(3)
    random.random()                            # get_transform_params' flip draw
    ratio = np.random.uniform(low=1.2, high=1.5)
    assert after == (np.random.uniform(), random.random())
    from neurips18_hierchical_image_manipulation_amd.data import resample
    from neurips18_hierchical_image_manipulation_amd.data.base_dataset import get_transform_params, get_soft_bbox
    random.seed(3)
    params = get_transform_params((2048, 1024), config={'prob_flip': 0.0, 'fineSize': 64, 'img_to_obj_ratio': 2.0,
                                                          'patch_to_obj_ratio': 1.2}, bbox=bbox, random_crop=False)
    box = resample.pil_crop_box(params['crop_pos'])
    want_l = pil_resize(to_pil_bytes(label[0], 1), box, (64, 64), Image.NEAREST).astype(np.float32)
    assert np.array_equal(d['label'].cpu().numpy()[0, 0], want_l)
    ob = get_soft_bbox(np.array(params['bbox_in_context']), 64, 64, ratio)
    assert d['output_bbox'].tolist() == list(ob)
    ib = [int(v) for v in params['bbox_in_context']]
    m_in = np.zeros((64, 64), np.float32)
    m_in[ib[1]:ib[3], ib[0]:ib[2]] = 1
    assert np.array_equal(d['mask_in'].cpu().numpy()[0, 0], m_in)
    assert np.array_equal(d['mask_ctx_in'].cpu().numpy()[0, 0], (1 - m_in) * want_l + m_in * 26)
    want_p = pil_resize(to_pil_bytes(photo[0]), box, (64, 64), Image.BICUBIC).transpose(2, 0, 1).astype(np.float32)
    want_p = ((want_p / np.float32(255)) - np.float32(0.5)) / np.float32(0.5) * (1 - m_in)
    assert np.array_equal(d['image'].cpu().numpy()[0], want_p)
    x1, y1, x2, y2 = d['crop_pos'].tolist()
    assert np.array_equal(d['label_orig'].cpu().numpy(), label[:, :, y1:y2 + 1, x1:x2 + 1])
    assert d['cls'].tolist() == [26] and d['output_bbox_global'].dtype == torch.float64
    assert tuple(d['mask_out_orig'].shape) == tuple(d['label_orig'].shape)


# -- 3. canvas paste ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('glob,patch_box', [((1900.7, 950.2, 2100.3, 1100.9), (3, 5, 64, 64)),     # clamps + x4 == fs
                                            ((100.2, 200.9, 180.5, 290.1), (10, 12, 50, 44))])
def test_paste_canvas_bit_exact_vs_pillow(glob, patch_box):
    _, photo = _canvases(1024, 2048, 2)
    rs = np.random.RandomState(4)
    patch = np.tanh(rs.randn(1, 3, 64, 64).astype(np.float32) * 2)
    info = {'output_bbox_global': torch.tensor(glob, dtype=torch.float64), 'output_bbox': torch.tensor(patch_box)}
    ph, pt = torch.from_numpy(photo).to(DEV), torch.from_numpy(patch).to(DEV)
    before = ph.clone()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out_a = data_util.paste_canvas(ph, (pt + 1) / 2, info, method=Image.BICUBIC, is_img=True)
        out_b = data_util._paste_image(ph, pt, info, 2)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(ph, before)
    x1, y1 = max(0, int(glob[0])), max(0, int(glob[1]))
    x2, y2 = min(2047, int(glob[2])), min(1023, int(glob[3]))
    x3, y3, x4, y4 = patch_box
    src = to_pil_bytes(((patch[0] + np.float32(1)) / np.float32(2))[:, y3:y4 + 1, x3:x4 + 1])
    rec = np.asarray(Image.fromarray(src, 'RGB').resize([x2 - x1 + 1, y2 - y1 + 1], Image.BICUBIC))
    want = photo.copy()
    want[0, :, y1:y2 + 1, x1:x2 + 1] = rec.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    assert np.array_equal(out_a.cpu().numpy(), want)
    assert np.array_equal(out_b.cpu().numpy(), want)


def test_paste_canvas_label_window():
    label, _ = _canvases(1024, 2048, 5)
    lab = torch.from_numpy(label).to(DEV)
    gen = torch.randint(0, 35, (1, 1, 90, 70), device=DEV)
    info = {'crop_pos': torch.tensor([1978, 934, 2047, 1023])}
    with _no_sync():
        out = data_util.paste_canvas(lab, gen, info, resize=False)
    want = label.copy()
    want[0, :, 934:1024, 1978:2048] = gen.cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), want) and torch.equal(lab.cpu(), torch.from_numpy(label))


# -- 4 / 5. evaluate(target_size) and the public path ---------------------------------------------------------------
def _scripts(tmp_path, fs=64):
    b2m = joint_fixture.with_flags(joint_fixture.BOX2MASK_FLAGS, fineSize=fs, checkpoints_dir=str(tmp_path))
    m2i = joint_fixture.with_flags(joint_fixture.MASK2IMAGE_FLAGS, fineSize=fs, checkpoints_dir=str(tmp_path), ngf=16)
    sb, sm = joint_fixture.script_pair(str(tmp_path), True, b2m, m2i)
    for path, cls, seed in ((sb, BoxToMaskTestOptions, 11), (sm, MaskToImageTestOptions, 12)):
        opt = vars(load_script_to_opt(path, cls))
        torch.manual_seed(seed)
        model = create_model(dict(opt, isTrain=True, use_gan=True))
        model.save('latest')
    return sb, sm


def test_box2mask_test_time_load_needs_checkpoint(tmp_path):
    sb, _ = joint_fixture.script_pair(str(tmp_path), True,
                                      joint_fixture.with_flags(joint_fixture.BOX2MASK_FLAGS, checkpoints_dir=str(tmp_path)))
    with pytest.raises(AssertionError):
        create_model(load_script_to_opt(sb, BoxToMaskTestOptions))


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _golden(name):
    return np.load(os.path.join(GOLDEN, 'joint_%s.npz' % name))


def _check_crop(tag, d, g, canvas):
    """Every crop_canvas output against the live reference's (tests/golden/joint_<case>.npz)."""
    for k in ('label', 'mask_ctx_in', 'mask_in', 'mask_out', 'mask_ctx_in_orig', 'mask_out_orig'):
        assert d[k].dtype == torch.float32 and d[k].is_cuda, k
        assert np.array_equal(d[k].cpu().numpy(), g['%s_%s' % (tag, k)].astype(np.float32)), '%s %s' % (tag, k)
    for k in ('crop_pos', 'cls', 'output_bbox', 'output_bbox_global'):
        want = g['%s_%s' % (tag, k)]
        assert d[k].dtype == torch.from_numpy(want).dtype and np.array_equal(d[k].numpy(), want), '%s %s' % (tag, k)
    x1, y1, x2, y2 = d['crop_pos'].tolist()
    assert tuple(d['label_orig'].shape) == tuple(g[tag + '_label_orig_shape'])
    assert np.array_equal(d['label_orig'].cpu().numpy(), canvas[:, :, max(0, y1):y2 + 1, max(0, x1):x2 + 1])


def _check_image(d, g):
    b = g['c2_image_bytes'].astype(np.float32)
    want = ((b / np.float32(255)) - np.float32(0.5)) / np.float32(0.5) * (1 - g['c2_mask_in'].astype(np.float32))
    assert np.array_equal(d['image'].cpu().numpy(), want)


def _box2mask(tmp_path, c):
    model = create_model(dict(model='AE_maskgen_twostream', gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp_path),
                              name='t', ndf=16, fineSize=c['fineSize']))
    model.netG.load_state_dict(joint_fixture.box2mask_state(model.netG.state_dict(), c['wseed']))
    return model


def _evaluate_input(d):
    return {'label_map': d['label'], 'mask_ctx_in': d['mask_ctx_in'], 'mask_out': d['mask_out'], 'mask_in': d['mask_in'],
            'cls': d['cls'], 'label_map_orig': d['label_orig'], 'mask_ctx_in_orig': d['mask_ctx_in_orig'],
            'mask_out_orig': d['mask_out_orig']}


def _check_layout(ev, d, g, cls):
    want = g['evaluate']
    assert ev.dtype == (torch.int64 if cls == 34 else torch.float32) and tuple(ev.shape) == want.shape
    sure = g['evaluate_sure']
    assert sure.mean() > 0.99
    assert np.array_equal(ev.cpu().numpy()[sure], want[sure].astype(ev.cpu().numpy().dtype))
    # the edit is not a no-op: the reference changed this many pixels, and so does the build
    assert int(g['evaluate_changed']) >= joint_fixture.MIN_CHANGED
    assert int((ev.float() != d['label_orig']).sum()) >= joint_fixture.MIN_CHANGED


@pytest.mark.parametrize('name', list(joint_fixture.CASES))
def test_joint_steps_match_reference_fixture(tmp_path, name):
    """gen_layout -> gen_image step by step against the live reference: both crops (every output, bit-exact), the
    layout of evaluate(target_size) (equal wherever the reference's decision margin is above 1e-4), the label paste and
    the image paste fed the reference's layout / the seeded generated patch (bit-exact, rest of the canvas untouched)."""
    c = joint_fixture.CASES[name]
    g = _golden(name)
    fs, cls = c['fineSize'], c['bbox']['cls']
    model = _box2mask(tmp_path, c)
    label, photo = joint_fixture.canvases(c['seed'])
    lab, ph = torch.from_numpy(label).to(DEV), torch.from_numpy(photo).to(DEV)
    opt = joint_fixture.crop_opt(fs)
    np.random.seed(c['seed'])
    random.seed(c['seed'])
    with _no_sync():
        d1 = data_util.crop_canvas(c['bbox'], lab, opt)
    _check_crop('c1', d1, g, label)
    ev = model.evaluate(_evaluate_input(d1), target_size=tuple(d1['label_orig'].shape[2:4]))
    _check_layout(ev, d1, g, cls)
    ref_ev = torch.from_numpy(g['evaluate'].astype(np.int64 if cls == 34 else np.float32)).to(DEV)
    with _no_sync():
        lc = data_util.paste_canvas(lab, ref_ev, d1, resize=False)
    x1, y1, x2, y2 = d1['crop_pos'].tolist()
    want = label.copy()
    want[0, :, y1:y2 + 1, x1:x2 + 1] = g['evaluate'][0].astype(np.float32)
    assert np.array_equal(lc.cpu().numpy(), want) and torch.equal(lab.cpu(), torch.from_numpy(label))
    pt = torch.from_numpy(joint_fixture.generated_patch(c['seed'], fs)).to(DEV)
    with _no_sync():
        d2 = data_util.crop_canvas(c['bbox'], lc, opt, img_original=ph, transform_img=True)
        ic = data_util.paste_canvas(ph, (pt + 1) / 2, d2, method=Image.BICUBIC, is_img=True)
    _check_crop('c2', d2, g, want)
    _check_image(d2, g)
    x1, y1, x2, y2 = g['paste_box'].tolist()
    want = photo.copy()
    want[0, :, y1:y2 + 1, x1:x2 + 1] = g['paste_window'].astype(np.float32) / np.float32(255)
    assert np.array_equal(ic.cpu().numpy(), want) and torch.equal(ph.cpu(), torch.from_numpy(photo))


class _no_sync(object):
    """The canvas code under torch.cuda.set_sync_debug_mode('error'): no host round trip."""

    def __enter__(self):
        torch.cuda.set_sync_debug_mode('error')

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(0)


def test_joint_inference_end_to_end(tmp_path):
    """The public path: script files + checkpoints saved by the build's own save() -> JointInference loads both
    generators (their weights are the saved ones) -> gen_layout on the 'interior' case reproduces the live reference's
    crop and layout; the image window of gen_image is Pillow's paste of the generator's own output, and everything
    outside the windows is the input canvas."""
    c, g = joint_fixture.CASES['interior'], _golden('interior')
    fs = c['fineSize']
    b2m = joint_fixture.with_flags(joint_fixture.BOX2MASK_FLAGS, fineSize=fs, checkpoints_dir=str(tmp_path))
    m2i = joint_fixture.with_flags(joint_fixture.MASK2IMAGE_FLAGS, fineSize=fs, checkpoints_dir=str(tmp_path), ngf=16)
    sb, sm = joint_fixture.script_pair(str(tmp_path), True, b2m, m2i)
    saved = {}
    for key, path, cls, extra in (('b2m', sb, BoxToMaskTestOptions, dict(use_gan=True)), ('m2i', sm, MaskToImageTestOptions, {})):
        torch.manual_seed(12)
        m = create_model(dict(vars(load_script_to_opt(path, cls)), isTrain=True, **extra))
        if key == 'b2m':
            m.netG.load_state_dict(joint_fixture.box2mask_state(m.netG.state_dict(), c['wseed']))
        saved[key] = {k: v.detach().cpu().clone() for k, v in m.netG.state_dict().items()}
        m.save('latest')
    ji = JointInference(argparse.Namespace(maskgen_script=sb, imggen_script=sm, gpu_ids=[0]))
    assert not ji.G_box2mask.isTrain and not ji.G_mask2img.isTrain
    for key, net in (('b2m', ji.G_box2mask.netG), ('m2i', ji.G_mask2img.netG)):
        sd = net.state_dict()
        assert set(sd) == set(saved[key]) and all(torch.equal(sd[k].cpu(), v) for k, v in saved[key].items()), key
    label, photo = joint_fixture.canvases(c['seed'])
    lab, ph = torch.from_numpy(label).to(DEV), torch.from_numpy(photo).to(DEV)
    np.random.seed(c['seed'])
    random.seed(c['seed'])
    canvas_l, d1, gen_l = ji.gen_layout(c['bbox'], lab, ji.opt_maskgen)
    _check_crop('c1', d1, g, label)
    _check_layout(gen_l, d1, g, c['bbox']['cls'])
    x1, y1, x2, y2 = d1['crop_pos'].tolist()
    want = label.copy()
    want[0, :, y1:y2 + 1, x1:x2 + 1] = gen_l.float().cpu().numpy()[0]
    assert np.array_equal(canvas_l.cpu().numpy(), want) and torch.equal(lab.cpu(), torch.from_numpy(label))
    # gen_image crops with the mask2image options (--contextMargin 3), as vis_joint_inference.py passes them; the
    # fixture's second crop uses the box2mask margin, so the window here is checked against Pillow instead
    canvas_i, d2, gen_i = ji.gen_image(c['bbox'], ph, canvas_l, ji.opt_imggen)
    assert tuple(gen_i.shape) == (1, 3, fs, fs)
    x1, y1, x2, y2 = [int(v) for v in d2['output_bbox_global'].int()]
    x1, y1, x2, y2 = max(0, x1), max(0, y1), min(2047, x2), min(1023, y2)
    x3, y3, x4, y4 = [int(v) for v in d2['output_bbox']]
    src = to_pil_bytes(gen_i.cpu().numpy()[0][:, y3:y4 + 1, x3:x4 + 1], 2)
    rec = np.asarray(Image.fromarray(src, 'RGB').resize([x2 - x1 + 1, y2 - y1 + 1], Image.BICUBIC))
    exp = photo.copy()
    exp[0, :, y1:y2 + 1, x1:x2 + 1] = rec.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    got = canvas_i.cpu().numpy()
    bad = np.argwhere(got != exp)
    assert bad.size == 0, '%d pixels differ, first %s: %r vs %r' % (len(bad), bad[:3].tolist(), got[tuple(bad[0])],
                                                                    exp[tuple(bad[0])])
    assert torch.equal(ph.cpu(), torch.from_numpy(photo))


def test_normalize_input_matches_totensor():
    """normalize_input of an RGB photo and a mode-'L' label map: (3,H,W) ToTensor (optionally Normalize) and (1,H,W)
    ToTensor * 255 (the ids), as upstream -- the caller adds the batch axis."""
    rs = np.random.RandomState(9)
    img = rs.randint(0, 256, size=(24, 40, 3)).astype(np.uint8)
    ids = rs.randint(0, 35, size=(24, 40)).astype(np.uint8)
    ji = JointInference.__new__(JointInference)
    for norm in (False, True):
        t_img, t_lab = ji.normalize_input(Image.fromarray(img, 'RGB'), Image.fromarray(ids, 'L'), normalize_image=norm)
        want = img.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
        if norm:
            want = (want - np.float32(0.5)) / np.float32(0.5)
        assert tuple(t_img.shape) == (3, 24, 40) and np.array_equal(t_img.cpu().numpy(), want)
        assert tuple(t_lab.shape) == (1, 24, 40) and np.array_equal(t_lab.cpu().numpy()[0], ids.astype(np.float32))


def test_evaluate_target_size_needs_original_maps(tmp_path):
    sb, _ = _scripts(tmp_path)
    m = create_model(load_script_to_opt(sb, BoxToMaskTestOptions))
    d = {k: torch.zeros(1, 1, 64, 64, device=DEV) for k in ('label_map', 'mask_ctx_in', 'mask_out', 'mask_in')}
    d['cls'] = torch.tensor([26])
    with pytest.raises(KeyError):
        m.evaluate(d, target_size=(100, 90))
    d.update(label_map_orig=torch.zeros(1, 1, 100, 90, device=DEV), mask_ctx_in_orig=torch.zeros(1, 1, 100, 90, device=DEV),
             mask_out_orig=torch.ones(1, 1, 100, 90, device=DEV))
    assert tuple(m.evaluate(d, target_size=(100, 90)).shape) == (1, 1, 100, 90)
    with pytest.raises(ValueError):
        m.evaluate(d, target_size=(64, 64))


def test_resize_compose_refuses_mismatched_shapes():
    comb, obj = torch.rand(1, 35, 8, 8, device=DEV), torch.rand(1, 1, 8, 8, device=DEV)
    label = torch.zeros(1, 1, 20, 30, device=DEV)
    with pytest.raises(ops.HimError):
        ops.resize_compose(comb, obj, label, torch.zeros(1, 1, 20, 29, device=DEV), 34, True)
    with pytest.raises(ops.HimError):
        ops.resize_compose(comb, torch.rand(1, 1, 8, 9, device=DEV), label, None, 26, False)
