#!/usr/bin/env python
"""One joint box -> layout -> image edit on a 1024 x 2048 canvas with the architectures of the pretrained Cityscapes
test scripts (fineSize 256; seeded weights saved as checkpoints and loaded through JointInference's own constructor).
Prints one JSON line: median ms per edit over --edits edits after --warmup, the median HIP-event time of each stage
(crop, box2mask forward, resize-compose, label paste, crop, mask2image forward, image paste) and the share of the edit
spent outside the two generator forwards.  Not the bench.py line."""
import argparse
import json
import os
import random
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
import numpy as np
import torch

import joint_fixture
from neurips18_hierchical_image_manipulation_amd import ops
from neurips18_hierchical_image_manipulation_amd.models import create_model
from neurips18_hierchical_image_manipulation_amd.models.joint_inference_model import JointInference
from neurips18_hierchical_image_manipulation_amd.options import BoxToMaskTestOptions, MaskToImageTestOptions
from neurips18_hierchical_image_manipulation_amd.util import data_util
from neurips18_hierchical_image_manipulation_amd.util.util import load_script_to_opt

STAGES = ['crop_layout', 'box2mask_forward', 'resize_compose', 'label_paste', 'crop_image', 'mask2image_forward',
          'image_paste']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--edits', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix='joint_bench_')
    b2m = joint_fixture.with_flags(joint_fixture.BOX2MASK_FLAGS, checkpoints_dir=d)
    m2i = joint_fixture.with_flags(joint_fixture.MASK2IMAGE_FLAGS, checkpoints_dir=d)
    sb, sm = joint_fixture.script_pair(d, True, b2m, m2i)
    for path, cls, seed, extra in ((sb, BoxToMaskTestOptions, 1, dict(use_gan=True)), (sm, MaskToImageTestOptions, 2, {})):
        torch.manual_seed(seed)
        create_model(dict(vars(load_script_to_opt(path, cls)), isTrain=True, **extra)).save('latest')
    ji = JointInference(argparse.Namespace(maskgen_script=sb, imggen_script=sm, gpu_ids=[0]))

    rs = np.random.RandomState(0)
    label = rs.randint(0, 35, size=(129, 257)).repeat(8, 0).repeat(8, 1)[:1024, :2048].astype(np.float32)
    lab = torch.from_numpy(label)[None, None].cuda()
    ph = torch.from_numpy(rs.randint(0, 256, size=(1, 3, 1024, 2048)).astype(np.float32) / np.float32(255)).cuda()
    boxes = [{'cls': 26, 'bbox': [700, 380, 980, 600]}, {'cls': 24, 'bbox': [1500, 500, 1640, 820]}]

    ev = {}
    mark = lambda k: ev.setdefault(k, torch.cuda.Event(enable_timing=True)).record()  # noqa: E731
    compose = ops.resize_compose

    def timed_compose(*args, **kw):
        mark('b2m_end')
        out = compose(*args, **kw)
        mark('compose_end')
        return out

    ops.resize_compose = timed_compose
    G = ji.G_mask2img
    infer = G.inference

    def timed_inference(*args, **kw):
        mark('crop2_end')
        out = infer(*args, **kw)
        mark('m2i_end')
        return out

    G.inference = timed_inference
    np.random.seed(0)
    random.seed(0)
    rows = []
    for i in range(a.warmup + a.edits):
        ev.clear()
        bbox = ji.sample_bbox(boxes, ji.opt_maskgen)
        mark('start')
        inp = data_util.crop_canvas(bbox, lab, ji.opt_maskgen)
        mark('crop1_end')
        gen = ji.G_box2mask.evaluate({
            'label_map': inp['label'], 'mask_ctx_in': inp['mask_ctx_in'], 'mask_out': inp['mask_out'],
            'mask_in': inp['mask_in'], 'cls': inp['cls'], 'label_map_orig': inp['label_orig'],
            'mask_ctx_in_orig': inp['mask_ctx_in_orig'], 'mask_out_orig': inp['mask_out_orig']},
            target_size=tuple(inp['label_orig'].shape[2:4]))
        canvas_l = data_util.paste_canvas(lab, gen, inp, resize=False)
        mark('paste1_end')
        ji.gen_image(bbox, ph, canvas_l, ji.opt_imggen)
        mark('end')
        torch.cuda.synchronize()
        if i < a.warmup:
            continue
        t = lambda x, y: ev[x].elapsed_time(ev[y])  # noqa: E731
        rows.append([t('start', 'end'), t('start', 'crop1_end'), t('crop1_end', 'b2m_end'), t('b2m_end', 'compose_end'),
                     t('compose_end', 'paste1_end'), t('paste1_end', 'crop2_end'), t('crop2_end', 'm2i_end'),
                     t('m2i_end', 'end')])
    med = np.median(np.array(rows), axis=0)
    stages = {k: round(float(v), 4) for k, v in zip(STAGES, med[1:])}
    fwd = stages['box2mask_forward'] + stages['mask2image_forward']
    print(json.dumps({'metric': 'joint_edit_ms', 'median_ms_per_edit': round(float(med[0]), 4), 'edits': a.edits,
                      'warmup': a.warmup, 'canvas': [1024, 2048], 'fineSize': 256, 'stage_median_ms': stages,
                      'outside_forwards_share': round(float((med[0] - fwd) / med[0]), 4),
                      'device': torch.cuda.get_device_name(0)}))


if __name__ == '__main__':
    main()
