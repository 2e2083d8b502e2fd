"""Timing of the region Poisson clone: profiles/region_clone_bench.json.  Reports only; nothing is asserted
on a time, and there is no gate: nothing before this clones a region.

Three regions on a 1024 x 2048 photo canvas, default options (rtol 1e-7, cap 6 (H + W)): an ellipse filling a 128 x 128
window, an ellipse filling a 401 x 397 window (composite_bench's joint-edit window), and the full 401 x 397 window.
Between two HIP events, the median of ``--reps`` calls after 5 warm-up calls, all in one process:

  solve_ms        him_region_poisson_solve on a resident workspace: 2 max_iter + 2 launches, those after the stop return
                  at once
  solve_live_ms   the same with max_iter = the iterations the solve ran: only the launches that work
  apply_ms        him_region_poisson_apply
  clone_ms        the whole ops.canvas_clone_region call (table upload, both bicubic passes, solve, apply)
  iterations, us_per_iteration (solve_live_ms over iterations), launches_per_iteration (2: dir and upd)

For context, in the same run: the second ``_repaint`` pass of ``JointInference.move_object`` on the tiny seeded models
of tests/joint_fixture.py, which ``keep_appearance=True`` replaces by a clone.  Clocks are left as found and nothing is
set on the device.

    python tools/region_clone_bench.py [--reps 20] [--out profiles/region_clone_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HC, WC = 1024, 2048
# name -> (x0, y0, H, W, ellipse or full)
REGIONS = {'ellipse_128x128': (900, 400, 128, 128, True), 'ellipse_401x397': (813, 307, 401, 397, True),
           'full_401x397': (813, 307, 401, 397, False)}


def repaint_context(torch, np, reps, timed):
    """The parent's second repaint of a moved object on the tiny models (the scene of tests/test_layout_edit_gpu.py)."""
    import random
    import tempfile
    import joint_fixture
    import layout_edit_fixture as lf
    from neurips18_hierchical_image_manipulation_amd import ops, preprocess
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    from neurips18_hierchical_image_manipulation_amd.models.joint_inference_model import JointInference
    from neurips18_hierchical_image_manipulation_amd.options import BoxToMaskTestOptions, MaskToImageTestOptions
    from neurips18_hierchical_image_manipulation_amd.util.util import load_script_to_opt
    tmp = tempfile.mkdtemp(prefix='region_clone_bench')
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
    x0, y0, x1, y1 = obj[1]['bbox']
    dst = [x0 + 150, y0 + 40, x1 + 150, y1 + 40]
    out = {}
    for name, kw in (('move_object_repaint_ms', {}), ('move_object_keep_appearance_ms', dict(keep_appearance=True))):
        def edit():
            np.random.seed(9)
            random.seed(9)
            return ji.move_object(obj, dst, lab, ins, ph, ji.opt_imggen, feather=6, reach=2, **kw)
        report = edit()[4]
        out[name] = timed(edit, reps)
        if kw:
            out['clone_status'] = report['passes'][1]['clone']
    # the second repaint alone, on the canvases the edit leaves
    label_c, _, img_c, _, report = ji.move_object(obj, dst, lab, ins, ph, ji.opt_imggen, feather=6, reach=2)

    def second():
        np.random.seed(9)
        random.seed(9)
        ji._repaint(report['place'][2:6], 26, img_c, lab, label_c, ji.opt_imggen, 6, 2, 'smooth')
    out['second_repaint_ms'] = timed(second, reps)
    out['object_box'] = [int(v) for v in obj[1]['bbox']]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'region_clone_bench.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    from composite_bench import timed
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd._cabi import lib
    assert torch.cuda.is_available(), 'region_clone_bench needs the GPU'
    g = np.random.default_rng(0)
    photo = torch.from_numpy((g.integers(0, 256, size=(1, 3, HC, WC)) / np.float32(255)).astype(np.float32)).cuda()
    src = torch.from_numpy((g.integers(0, 256, size=(1, 3, HC, WC)) / np.float32(255)).astype(np.float32)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    regions = {}
    for name, (x0, y0, H, W, ellipse) in REGIONS.items():
        yy, xx = np.mgrid[0:H, 0:W]
        R = (((yy - (H - 1) / 2.0) / (H / 2.0)) ** 2 + ((xx - (W - 1) / 2.0) / (W / 2.0)) ** 2 <= 1.0) if ellipse \
            else np.ones((H, W), bool)
        plane = np.zeros((HC, WC), np.uint8)
        plane[y0:y0 + H, x0:x0 + W] = R
        plane, window = torch.from_numpy(plane).cuda(), torch.from_numpy(R.astype(np.uint8)).cuda()
        src_box, dst_box = (100, 200, 100 + W, 200 + H), (x0, y0, x0 + W, y0 + H)
        P = ops.canvas_crop_bicubic(src, src_box, H, W, normalize=False)
        u, status, resid = ops.region_poisson_solve(photo, x0, y0, P, window)
        ws = ops._SCRATCH['region_poisson_solve', photo.device.index].buf
        stat = status.tolist()
        iters, cap = stat[3], 6 * (H + W)
        work = photo.clone()

        def solve(max_iter):
            lib.him_region_poisson_solve(photo.data_ptr(), HC, WC, x0, y0, H, W, P.data_ptr(), window.data_ptr(), 0, 1e-7,
                                         max_iter, u.data_ptr(), status.data_ptr(), resid.data_ptr(), ws.data_ptr(),
                                         ws.numel(), st)

        def apply():
            lib.him_region_poisson_apply(P.data_ptr(), u.data_ptr(), window.data_ptr(), work.data_ptr(), HC, WC, x0, y0, H,
                                         W, st)

        # results first: two solves give the same bits, and the kernel-level calls equal the ops path
        keep = u.clone()
        solve(cap)
        assert torch.equal(u, keep) and status.tolist() == stat and stat[4] == 0
        apply()
        want, _, _ = ops.canvas_clone_region(src, src_box, photo.clone(), dst_box, plane)
        assert torch.equal(work, want)
        times = {'solve_ms': timed(lambda: solve(cap), args.reps), 'solve_live_ms': timed(lambda: solve(iters), args.reps),
                 'apply_ms': timed(apply, args.reps),
                 'clone_ms': timed(lambda: ops.canvas_clone_region(src, src_box, work, dst_box, plane), args.reps)}
        regions[name] = {'origin': [x0, y0], 'window': [H, W], 'unknowns': stat[1], 'dropped_on_ring': stat[2],
                         'iterations': iters, 'cap': cap, 'resid': resid.tolist(), 'launches_per_iteration': 2,
                         'launches_per_solve': 2 * cap + 2, 'times': times,
                         'us_per_iteration': round(times['solve_live_ms']['median'] * 1e3 / max(iters, 1), 3),
                         'vector_bytes': 3 * 8 * H * W}
    out = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'warmup': 5, 'canvas': [HC, WC], 'rtol': 1e-7,
           'regions': regions,
           'note': ('event-timed medians of single calls after 5 warm-up calls, one process; solve_ms enqueues the launches of '
                    'the whole cap, solve_live_ms those of the iterations run; no hardware counters were collected and no '
                    'kernel was timed alone')}

    def write():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write('\n')
    write()
    out['tiny_models_context'] = repaint_context(torch, np, args.reps, timed)
    write()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
