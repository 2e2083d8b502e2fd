"""Timing of the feathered canvas composite: profiles/composite_bench.json.  Reports only; nothing is asserted on a time.

One joint-edit-sized paste: a 1024 x 2048 photo canvas, a 401 x 397 window at an unaligned origin, fed from a 256 x 256
generator patch (upscaling, ksize 5), the label edit a filled ellipse of about a tenth of the window plus scattered
pixels.  Between two HIP events, the median of ``--reps`` calls after 5 warm-up calls, all in one process:

  hard_v_ms        him_canvas_paste_bicubic_v alone (tmp and tables already on the device): the existing hard paste
  blend_v_ms       him_canvas_paste_blend_v alone on the same tmp and tables, with dist2 and a matte: the comparable figure
  blend_v_border_ms  the same without dist2 (border term only), still writing the matte
  changed_ms       him_canvas_changed over the window
  edt_ms           ops.distance_transform of the changed plane (three launches, its own output allocation)
  paste_hard_ms / paste_blend_ms   the whole ops.canvas_paste_bicubic / ops.canvas_paste_blend call (table upload,
                   window bytes, horizontal pass, vertical pass) -- what a caller pays per paste

Bytes of the blended vertical pass are counted from the matte it wrote: 4 (dist2) + 4 (matte) per window pixel, 12 written
per pixel with alpha > 0, 12 read per pixel with 0 < alpha < 1, plus tmp once (rows x W x 3; the overlapping taps of
neighbouring rows are counted once).  The hard pass: 12 written per pixel plus tmp once.  Clocks are left as found and
nothing is set on the device.

    python tools/composite_bench.py [--reps 20] [--out profiles/composite_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.3e12
HC, WC, X0, Y0, H, W, PATCH = 1024, 2048, 813, 307, 401, 397, 256
FEATHER, REACH = 8, 4


def timed(fn, reps, warmup=5):
    import torch
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return {'min': round(min(out), 4), 'median': round(statistics.median(out), 4), 'max': round(max(out), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'composite_bench.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd._cabi import lib
    from neurips18_hierchical_image_manipulation_amd.data import resample
    assert torch.cuda.is_available(), 'composite_bench needs the GPU'
    g = np.random.default_rng(0)
    photo = torch.from_numpy(g.random((1, 3, HC, WC), dtype=np.float32)).cuda()
    patch = torch.from_numpy(g.random((1, 3, PATCH, PATCH), dtype=np.float32)).cuda()
    before = np.kron(g.integers(0, 35, size=(HC // 32, WC // 32)), np.ones((32, 32), np.int64)).astype(np.float32)
    after = before.copy()
    yy, xx = np.mgrid[0:H, 0:W]
    edit = ((yy - H * 0.5) / (H * 0.22)) ** 2 + ((xx - W * 0.45) / (W * 0.15)) ** 2 <= 1
    edit |= g.random((H, W)) < 0.0005
    after[Y0:Y0 + H, X0:X0 + W][edit] += 1
    lb, la = torch.from_numpy(before)[None, None].cuda(), torch.from_numpy(after)[None, None].cuda()
    box = (0, 0, PATCH, PATCH)
    st = torch.cuda.current_stream().cuda_stream

    # the vertical passes alone: tmp from the shared horizontal pass, tables resident
    fx_, nx, wx, ksx = resample.bicubic_tables(PATCH, W)
    fy, ny, wy, ksy = resample.bicubic_tables(PATCH, H)
    buf, (o, p, r, afx, anx, awx, afy, any_, awy) = ops._scratch_and_tables(
        PATCH * PATCH * 3, [np.zeros(1, np.int64), np.array([PATCH], np.int32), np.array([PATCH], np.int32), fx_, nx, wx,
                            fy, ny, wy], photo.device)
    lib.him_canvas_window_bytes(patch.data_ptr(), 3, PATCH, PATCH, 0, 0, PATCH, PATCH, 0, buf.data_ptr(), st)
    tmp = torch.empty((PATCH, W, 3), dtype=torch.uint8, device=photo.device)
    lib.him_data_bicubic_h(buf.data_ptr(), o, p, r, afx, anx, awx, ksx, tmp.data_ptr(), PATCH, 1, W, st)
    changed = ops.canvas_changed(lb, la, X0, Y0, H, W)
    dist2 = ops.distance_transform(changed, rule='nonzero')[0]
    matte = torch.empty((H, W), dtype=torch.float32, device=photo.device)
    work = photo.clone()

    def hard_v():
        lib.him_canvas_paste_bicubic_v(tmp.data_ptr(), afy, any_, awy, ksy, work.data_ptr(), HC, WC, X0, Y0, H, W, st)

    def blend_v(d2=dist2):
        lib.him_canvas_paste_blend_v(tmp.data_ptr(), afy, any_, awy, ksy, work.data_ptr(), HC, WC, X0, Y0, H, W,
                                     0 if d2 is None else d2.data_ptr(), FEATHER, REACH, 1, matte.data_ptr(), st)

    # results first: the kernel-level calls equal the ops path, and alpha == 1 pixels equal the hard paste
    hard_v()
    want_hard = ops.canvas_paste_bicubic(patch, box, photo.clone(), X0, Y0, H, W)
    assert torch.equal(work, want_hard)
    work.copy_(photo)
    blend_v()
    want_blend, want_matte = ops.canvas_paste_blend(patch, box, photo.clone(), X0, Y0, H, W, feather=FEATHER, reach=REACH,
                                                    dist2=dist2, profile='smooth', want_matte=True)
    assert torch.equal(work, want_blend) and torch.equal(matte, want_matte[0, 0])
    n = H * W
    n_one, n_zero = int((matte == 1).sum()), int((matte == 0).sum())
    n_mid = n - n_one - n_zero
    one = (matte == 1)[None].expand(3, H, W)
    assert torch.equal(want_blend[0, :, Y0:Y0 + H, X0:X0 + W][one], want_hard[0, :, Y0:Y0 + H, X0:X0 + W][one])
    tmp_bytes = PATCH * W * 3
    bytes_hard = n * 12 + tmp_bytes
    bytes_blend = n * 8 + (n_one + n_mid) * 12 + n_mid * 12 + tmp_bytes

    res = {
        'hard_v_ms': timed(hard_v, args.reps), 'blend_v_ms': timed(blend_v, args.reps),
        'blend_v_border_ms': timed(lambda: blend_v(None), args.reps),
        'changed_ms': timed(lambda: ops.canvas_changed(lb, la, X0, Y0, H, W), args.reps),
        'edt_ms': timed(lambda: ops.distance_transform(changed, rule='nonzero'), args.reps),
        'paste_hard_ms': timed(lambda: ops.canvas_paste_bicubic(patch, box, work, X0, Y0, H, W), args.reps),
        'paste_blend_ms': timed(lambda: ops.canvas_paste_blend(patch, box, work, X0, Y0, H, W, feather=FEATHER, reach=REACH,
                                                               dist2=dist2, profile='smooth', want_matte=True), args.reps),
    }
    out = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'warmup': 5,
           'shape': {'canvas': [HC, WC], 'window': [H, W], 'origin': [X0, Y0], 'patch': PATCH, 'ksize': int(ksy),
                     'feather': FEATHER, 'reach': REACH, 'profile': 'smooth'},
           'pixels': {'window': n, 'changed': int(changed.sum()), 'alpha_one': n_one, 'alpha_zero': n_zero,
                      'alpha_between': n_mid},
           'bytes': {'hard_v': bytes_hard, 'blend_v': bytes_blend},
           'hbm_floor_ms': {'hard_v': round(bytes_hard / HBM_BYTES_PER_S * 1e3, 6),
                            'blend_v': round(bytes_blend / HBM_BYTES_PER_S * 1e3, 6)},
           'times': res,
           'blend_v_over_hard_v': round(res['blend_v_ms']['median'] / res['hard_v_ms']['median'], 3),
           'note': ('event-timed medians of single calls after 5 warm-up calls, one process; *_v = the vertical-pass call '
                    'alone on resident tmp and tables, paste_* = the whole ops call including the pinned table upload and '
                    'its allocations; bytes counted from the matte as the module docstring says; hbm_floor = those bytes '
                    'at 6.3 TB/s')}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
