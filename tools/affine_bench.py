"""Timing of the affine layout edits: profiles/affine_bench.json.  Reports only; nothing is asserted on a
time, and there is no gate: nothing before this warps or rotates anything.

Two objects on a 1024 x 2048 canvas pair and photograph, a 128 x 128 and a 401 x 397 box (composite_bench's joint-edit
window) filled by an ellipse, each at 0 and at 30 degrees.  Between two HIP events, the median of ``--reps`` measurements
after 5 warm-up calls, all in one process; a kernel of a few microseconds is shorter than the events' own cost, so every
entry point is measured twice: one call between the events (``single``) and 100 back-to-back calls between them
divided by 100 (``per_call``, launch overhead included, the figure to quote):

  place_affine_ms   him_layout_place_affine (status init + the tile kernel), fp32 label + fp32 instance planes
  warp_affine_ms    him_canvas_warp_affine over the destination box
  place_ms          for context, at 0 degrees: the separable him_layout_place with resident index tables
  crop_bicubic_ms   for context, at 0 degrees: ops.canvas_crop_bicubic of the same box at the same size (table upload,
                    window bytes, both passes), the patch the separable clone uses

and one whole ``JointInference.transform_object(angle=30, keep_appearance=True)`` on the tiny seeded models of
tests/joint_fixture.py.  Clocks are left as found and nothing is set on the device.

    python tools/affine_bench.py [--reps 20] [--out profiles/affine_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HC, WC = 1024, 2048
BATCH = 100
# name -> source box [x0, y0, x1, y1)
OBJECTS = {'128x128': (900, 400, 1028, 528), '401x397': (813, 307, 1210, 708)}


def edit_context(torch, np, reps, timed):
    """One whole transform_object(keep_appearance=True) on the tiny models (the scene of tests/test_layout_edit_gpu.py)."""
    import random
    import tempfile
    import joint_fixture
    import layout_edit_fixture as lf
    from neurips18_hierchical_image_manipulation_amd import preprocess
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    from neurips18_hierchical_image_manipulation_amd.models.joint_inference_model import JointInference
    from neurips18_hierchical_image_manipulation_amd.options import BoxToMaskTestOptions, MaskToImageTestOptions
    from neurips18_hierchical_image_manipulation_amd.util.util import load_script_to_opt
    tmp = tempfile.mkdtemp(prefix='affine_bench')
    c = joint_fixture.CASES['interior']
    b2m = joint_fixture.with_flags(joint_fixture.BOX2MASK_FLAGS, fineSize=c['fineSize'], checkpoints_dir=tmp)
    m2i = joint_fixture.with_flags(joint_fixture.MASK2IMAGE_FLAGS, fineSize=c['fineSize'], checkpoints_dir=tmp, ngf=16)
    sb, sm = joint_fixture.script_pair(tmp, True, b2m, m2i)
    for path, cls, extra in ((sb, BoxToMaskTestOptions, dict(use_gan=True)), (sm, MaskToImageTestOptions, {})):
        torch.manual_seed(12)
        create_model(dict(vars(load_script_to_opt(path, cls)), isTrain=True, **extra)).save('latest')
    ji = JointInference(argparse.Namespace(maskgen_script=sb, imggen_script=sm, gpu_ids=[0]))
    label, photo = joint_fixture.canvases(c['seed'])
    label = label.copy()
    inst = label.copy()
    H, W = label.shape[2:]
    mask = lf.ellipse(H, W, 380, 800, 24, 36)
    label[0, 0][mask], inst[0, 0][mask] = 26, 26001
    lab, ins, ph = (torch.from_numpy(a).cuda() for a in (label, inst, photo))
    obj = [item for item in preprocess.inst_info(ins, lab)['objects'].items() if item[0] == '26001'][0]
    out = {}
    for name, kw in (('transform_object_repaint_ms', {}), ('transform_object_keep_appearance_ms', dict(keep_appearance=True))):
        def edit():
            np.random.seed(9)
            random.seed(9)
            return ji.transform_object(obj, lab, ins, ph, ji.opt_imggen, angle=30, shift=(150, 40), feather=6, reach=2, **kw)
        report = edit()[4]
        out[name] = timed(edit, reps)
        if kw:
            out['clone_status'] = report['passes'][1]['clone']
            out['place'] = report['place']
    out['object_box'] = [int(v) for v in obj[1]['bbox']]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'affine_bench.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    from composite_bench import timed
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd._cabi import lib
    assert torch.cuda.is_available(), 'affine_bench needs the GPU'
    g = np.random.default_rng(0)
    photo = torch.from_numpy((g.integers(0, 256, size=(1, 3, HC, WC)) / np.float32(255)).astype(np.float32)).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def both(fn):
        def batch():
            for _ in range(BATCH):
                fn()
        t = timed(batch, args.reps)
        return {'single': timed(fn, args.reps), 'per_call': {k: round(v / BATCH, 5) for k, v in t.items()}}

    objects = {}
    for name, box in OBJECTS.items():
        x0, y0, x1, y1 = box
        h, w = y1 - y0, x1 - x0
        yy, xx = np.mgrid[0:h, 0:w]
        inst = np.zeros((HC, WC), np.float32)
        inst[y0:y1, x0:x1][((yy - (h - 1) / 2.0) / (h / 2.0)) ** 2 + ((xx - (w - 1) / 2.0) / (w / 2.0)) ** 2 <= 1.0] = 26001
        src = torch.from_numpy(inst).cuda()
        label = torch.zeros((HC, WC), dtype=torch.float32, device='cuda')
        inst_dst = torch.zeros((HC, WC), dtype=torch.float32, device='cuda')
        changed = torch.zeros((HC, WC), dtype=torch.uint8, device='cuda')
        status = torch.empty(6, dtype=torch.int32, device='cuda')
        per = {}
        for angle in (0, 30):
            amap = ops.affine_map(box, angle=angle, shift=(-300, 100))
            inv = (ctypes.c_longlong * 6)(*amap.inv)
            dx0, dy0, dx1, dy1 = amap.dst_box
            H, W = dy1 - dy0, dx1 - dx0
            P = torch.empty((1, 3, H, W), dtype=torch.float32, device='cuda')

            def place_affine():
                lib.him_layout_place_affine(src.data_ptr(), 3, HC, WC, 26001, x0, y0, x1, y1, ctypes.addressof(inv),
                                            label.data_ptr(), 3, inst_dst.data_ptr(), HC, WC, dx0, dy0, dx1, dy1, 26, 26001, 0,
                                            0, changed.data_ptr(), status.data_ptr(), st)

            def warp_affine():
                lib.him_canvas_warp_affine(photo.data_ptr(), HC, WC, ctypes.addressof(inv), dx0, dy0, H, W, P.data_ptr(), st)

            # results first: the kernel-level calls equal the ops path, twice
            want = ops.layout_place_affine(label.clone().zero_(), inst_dst.clone().zero_(), src, 26001, amap, 26, 26001)
            label.zero_(), inst_dst.zero_(), changed.zero_()
            place_affine()
            assert torch.equal(label, want[0]) and torch.equal(changed, want[2]) and torch.equal(status, want[3])
            warp_affine()
            assert torch.equal(P, ops.canvas_warp_affine(photo, amap, (dx0, dy0, H, W)))
            row = {'dst_box': list(amap.dst_box), 'window': [H, W], 'placed': status.tolist()[0],
                   'place_affine_ms': both(place_affine), 'warp_affine_ms': both(warp_affine),
                   'warp_bytes_written': 3 * 4 * H * W}
            if angle == 0:
                xs, ys = ops._layout_index(w, W, src.device), ops._layout_index(h, H, src.device)

                def place():
                    lib.him_layout_place(src.data_ptr(), 3, HC, WC, 26001, x0, y0, x1, y1, xs.data_ptr(), ys.data_ptr(),
                                         label.data_ptr(), 3, inst_dst.data_ptr(), HC, WC, dx0, dy0, dx1, dy1, 26, 26001, 0, 0,
                                         changed.data_ptr(), status.data_ptr(), st)
                keep = (label.clone(), changed.clone(), status.clone())
                place()
                assert torch.equal(label, keep[0]) and torch.equal(changed, keep[1]) and torch.equal(status, keep[2])
                row['place_ms'] = both(place)
                row['crop_bicubic_ms'] = {'single': timed(lambda: ops.canvas_crop_bicubic(photo, box, H, W, normalize=False),
                                                          args.reps)}
            per['%d_degrees' % angle] = row
        objects[name] = per
    out = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'warmup': 5, 'batch': BATCH, 'canvas': [HC, WC],
           'objects': objects,
           'note': ('event-timed medians after 5 warm-up calls, one process; single = one call between the events, per_call = '
                    '%d back-to-back calls between them over %d; no hardware counters were collected, no kernel was timed '
                    'alone, no LDS-staged variant and no other tile shape was built' % (BATCH, BATCH))}

    def write():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write('\n')
    write()
    out['tiny_models_context'] = edit_context(torch, np, args.reps, timed)
    write()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
