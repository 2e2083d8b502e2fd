"""Timing of panoptic matching: profiles/panoptic_bench.json.  Reports only; nothing is asserted on a time.

The device call alone (``ops.panoptic_match``: seven launches, no copy, no synchronisation) between two HIP events, median
of ``--reps`` calls after 3 warm-up calls, on 8 x 256 x 512 Cityscapes-like synthetic layouts (the planes of
tools/ccl_bench.py: coarse-grid stuff classes plus a few hundred blobs of thing classes); the prediction is the ground
truth moved by 2 pixels.  Segment ids come from ``ops.label_instances`` (8-connected), classes are uint8, ids int32.

Next to it, on the same planes:

  confusion_ms       ``ops.confusion`` of the two class planes (the region measure: one read of both planes)
  hbm_floor_ms       reading the four planes once at 6.3 TB/s (the achievable HBM rate of the MI355X); the kernel reads
                     them twice and clears and walks its tables, none of which is in this floor
  host_ref_ms        the numpy restatement of tests/panoptic_fixture.py (wall clock, one run)

The device result is compared with the reference before anything is timed.  Clocks are left as found and nothing is set
on the device.

    python tools/panoptic_bench.py [--reps 20] [--out profiles/panoptic_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'panoptic_bench.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    import ccl_bench
    import panoptic_fixture as fx
    from neurips18_hierchical_image_manipulation_amd import ops
    B, H, W, n_class = 8, 256, 512, 35
    gt_cls = ccl_bench.layouts(B, H, W, seed=B)
    pred_cls = np.stack([fx.shifted(p, 2, 2) for p in gt_cls])
    g_cls, p_cls = torch.from_numpy(gt_cls).cuda(), torch.from_numpy(pred_cls).cuda()
    g_seg = ops.label_instances(g_cls, ccl_bench.THINGS, connectivity=8)[0]
    p_seg = ops.label_instances(p_cls, ccl_bench.THINGS, connectivity=8)[0]
    t0 = time.perf_counter()
    want = fx.match_reference(p_seg.cpu().numpy(), pred_cls, g_seg.cpu().numpy(), gt_cls, n_class)
    host_ms = (time.perf_counter() - t0) * 1e3
    counts, iou, status, _ = ops.panoptic_match(p_seg, p_cls, g_seg, g_cls, n_class)
    assert np.array_equal(counts.cpu().numpy(), want[0]) and np.array_equal(status.cpu().numpy(), want[2])
    assert np.allclose(iou.cpu().numpy(), want[1], rtol=1e-12, atol=0)
    ms = ccl_bench.timed(lambda: ops.panoptic_match(p_seg, p_cls, g_seg, g_cls, n_class), args.reps)
    ms_rows = ccl_bench.timed(lambda: ops.panoptic_match(p_seg, p_cls, g_seg, g_cls, n_class, want_matches=True), args.reps)
    conf = ccl_bench.timed(lambda: ops.confusion(p_cls, g_cls, n_class), args.reps)
    floor_ms = gt_cls.size * (1 + 1 + 4 + 4) / HBM_BYTES_PER_S * 1e3
    st = status.cpu().numpy()
    out = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'shape': '%dx%dx%d' % (B, H, W),
           'panoptic_match_ms': ms, 'panoptic_match_with_rows_ms': ms_rows, 'confusion_ms': conf,
           'panoptic_over_confusion': round(ms['median'] / conf['median'], 2), 'hbm_floor_ms': round(floor_ms, 5),
           'host_ref_ms': round(host_ms, 2), 'segments_gt': [int(v) for v in st[:, 0]],
           'segments_pred': [int(v) for v in st[:, 1]], 'tp_fp_fn': [int(v) for v in want[0].sum(0)],
           'note': ('event-timed medians of single ops.panoptic_match calls (uint8 classes, int32 ids, max_segments 1024) '
                    'after 3 warm-up calls; each call also allocates its small outputs through the caching allocator; '
                    'confusion = ops.confusion of the two class planes; hbm_floor = the four planes read once at 6.3 TB/s; '
                    'host_ref = numpy restatement of tests/panoptic_fixture.py, one run')}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
