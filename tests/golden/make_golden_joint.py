"""tests/golden/joint_api.json and tests/golden/joint_<case>.npz.

joint_api.json: what the live reference's joint-inference helpers produce on the host -- the options
``load_script_to_opt`` (util/util.py) reads from the two pretrained test scripts, in the one-line and the multi-line
form, with each parser (options/box2mask_test_options.py, options/mask2image_test_options.py), and the parameter lists
of ``JointInference``'s methods, ``crop_canvas`` and ``paste_canvas``.  Build container only (oracle/ref_shim.py).
Data only: option values, names and defaults.

joint_<case>.npz (cases in tests/joint_fixture.py): the live reference's gen_layout -> gen_image steps on a seeded
1024 x 2048 canvas -- crop_canvas, TwoStreamAE_mask.evaluate(target_size) with the margins of its decisions, the label
paste, the second crop_canvas with the photo, and the image paste of a seeded stand-in for the mask2image output.  Windows
only; the canvases, boxes and weights are rebuilt from seeds.  Two shims for today's torch, kept in this file:
torchvision's ToPILImage (mul(255).byte(), mode L / RGB), and ``cls`` handed to evaluate as (-1, 1) as torch 0.3's
``[0].unsqueeze(0)`` produced it.

    python tests/golden/make_golden_joint.py
"""
import importlib
import inspect
import io
import json
import math
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..', '..')))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, '..')))
from oracle import ref_shim                                              # noqa: E402
import joint_fixture                                                     # noqa: E402


def _json(v):
    if isinstance(v, float) and math.isinf(v):
        return 'inf'
    return v


def _sig(fn):
    out = []
    for p in inspect.signature(fn).parameters.values():
        d = None if p.default is inspect.Parameter.empty else p.default
        out.append([p.name, repr(d) if d is not None and not isinstance(d, (int, float, str, bool)) else d])
    return out


def main():
    ref_shim.install()
    util = importlib.import_module('util.util')
    b2m = importlib.import_module('options.box2mask_test_options').BoxToMaskTestOptions
    m2i = importlib.import_module('options.mask2image_test_options').MaskToImageTestOptions
    opts = {}
    with tempfile.TemporaryDirectory() as d:
        for multiline in (False, True):
            sb, sm = joint_fixture.script_pair(d, multiline)
            for key, path, cls in (('box2mask', sb, b2m), ('mask2image', sm, m2i)):
                stdout, sys.stdout = sys.stdout, io.StringIO()
                try:
                    o = util.load_script_to_opt(path, cls)
                finally:
                    sys.stdout = stdout
                opts['%s_%s' % (key, 'multi' if multiline else 'one')] = {k: _json(v) for k, v in sorted(vars(o).items())}
    du = importlib.import_module('util.data_util')
    ji = importlib.import_module('models.joint_inference_model').JointInference
    sigs = {'crop_canvas': _sig(du.crop_canvas), 'paste_canvas': _sig(du.paste_canvas),
            'load_script_to_opt': _sig(util.load_script_to_opt)}
    for m in ('__init__', 'sample_bbox', 'sample_window', 'normalize_input', 'gen_layout', 'gen_image'):
        sigs['JointInference.' + m] = _sig(getattr(ji, m))
    with open(os.path.join(HERE, 'joint_api.json'), 'w') as f:
        json.dump({'opts': opts, 'signatures': sigs}, f, indent=1, sort_keys=True)
        f.write('\n')


def _install_to_pil():
    import numpy as np
    import torchvision.transforms as tvt
    from PIL import Image

    class ToPILImage(object):
        def __call__(self, t):
            b = t.mul(255).byte().numpy()
            return Image.fromarray(b[0], 'L') if b.shape[0] == 1 else Image.fromarray(b.transpose(1, 2, 0).copy(), 'RGB')

    tvt.ToPILImage = ToPILImage


def _u8(t):
    import numpy as np
    a = t.detach().numpy() if hasattr(t, 'detach') else np.asarray(t)
    assert np.array_equal(a, np.round(a)) and a.min() >= 0 and a.max() < 256
    return a.astype(np.uint8)


def cases():
    import random
    import numpy as np
    import torch
    from PIL import Image
    ref_shim.install()
    _install_to_pil()
    du = importlib.import_module('util.data_util')
    for name, c in joint_fixture.CASES.items():
        fs = c['fineSize']
        ref = ref_shim.box2mask_trainer(ndf=16, fineSize=fs)
        ref.netG.load_state_dict(joint_fixture.box2mask_state(ref.netG.state_dict(), c['wseed']))
        label, photo = (torch.from_numpy(a) for a in joint_fixture.canvases(c['seed']))
        opt = joint_fixture.crop_opt(fs)
        np.random.seed(c['seed'])
        random.seed(c['seed'])
        out = {}
        with torch.no_grad():
            d1 = du.crop_canvas(c['bbox'], label, opt)
            e_in = {'label_map': d1['label'], 'mask_ctx_in': d1['mask_ctx_in'], 'mask_out': d1['mask_out'],
                    'mask_in': d1['mask_in'], 'cls': d1['cls'].view(-1, 1), 'label_map_orig': d1['label_orig'],
                    'mask_ctx_in_orig': d1['mask_ctx_in_orig'], 'mask_out_orig': d1['mask_out_orig']}
            ev = ref.evaluate(e_in, target_size=tuple(d1['label_orig'].size()[2:4]))
            # the margins of evaluate's decisions: |p - .5| of the resized object probability, or top-1 minus runner-up
            # of the background blend
            gt, ctx, gm, cls1h, oc = ref.encode_input(d1['label'], d1['mask_ctx_in'], d1['mask_out'], d1['mask_in'],
                                                     e_in['cls'])
            _, comb, _, obj = ref.netG.forward(ref.construct_input_cond(oc, ctx), cls1h)
            obj = ref.mask_variable(obj, gm)
            gt_o, _, gm_o, _, _ = ref.encode_input(d1['label_orig'], d1['mask_ctx_in_orig'], d1['mask_out_orig'], None,
                                                   e_in['cls'])
            us = torch.nn.Upsample(tuple(d1['label_orig'].size()[2:4]), mode='bilinear')
            if c['bbox']['cls'] == 34:
                top = ref.postprocess_output(us(comb), gm_o, gt_o).topk(2, dim=1).values
                margin = top[:, :1] - top[:, 1:2]
            else:
                margin = (us(obj) - 0.5).abs()
            lc = du.paste_canvas(label, ev.float(), d1, resize=False)
            d2 = du.crop_canvas(c['bbox'], lc, opt, img_original=photo, transform_img=True)
            patch = torch.from_numpy(joint_fixture.generated_patch(c['seed'], fs))
            ic = du.paste_canvas(photo, (patch + 1) / 2, d2, method=Image.BICUBIC, is_img=True)
        for tag, d in (('c1', d1), ('c2', d2)):
            for k in ('label', 'mask_ctx_in', 'mask_in', 'mask_out', 'mask_ctx_in_orig', 'mask_out_orig'):
                out['%s_%s' % (tag, k)] = _u8(d[k])
            for k in ('crop_pos', 'cls', 'output_bbox', 'output_bbox_global'):
                out['%s_%s' % (tag, k)] = d[k].numpy()
            out[tag + '_label_orig_shape'] = np.array(d['label_orig'].shape)
        img = d2['image'].numpy()
        out['c2_image_bytes'] = np.round((img * np.float32(0.5) + np.float32(0.5)) * 255).astype(np.uint8)
        assert ev.dtype == (torch.int64 if c['bbox']['cls'] == 34 else torch.float32)
        out['evaluate'] = _u8(ev)
        out['evaluate_sure'] = (margin > 1e-4).numpy()
        out['evaluate_changed'] = np.array(int((ev.float() != d1['label_orig']).sum()))
        x1, y1, x2, y2 = [int(v) for v in d2['output_bbox_global'].int()]
        x1, y1, x2, y2 = max(0, x1), max(0, y1), min(2047, x2), min(1023, y2)
        out['paste_box'] = np.array([x1, y1, x2, y2])
        out['paste_window'] = _u8(torch.round(ic[0, :, y1:y2 + 1, x1:x2 + 1] * 255))
        assert np.array_equal(ic.numpy()[0, :, y1:y2 + 1, x1:x2 + 1], out['paste_window'].astype(np.float32) / np.float32(255))
        assert int(out['evaluate_changed']) >= joint_fixture.MIN_CHANGED, (name, int(out['evaluate_changed']))
        path = os.path.join(HERE, 'joint_%s.npz' % name)
        np.savez_compressed(path, **out)
        print(name, 'changed', int(out['evaluate_changed']), 'sure %.4f' % out['evaluate_sure'].mean(),
              'crop', d1['crop_pos'].tolist(), 'out', d2['output_bbox'].tolist(), 'paste', out['paste_box'].tolist(),
              '%d bytes' % os.path.getsize(path))


if __name__ == '__main__':
    main()
    cases()
