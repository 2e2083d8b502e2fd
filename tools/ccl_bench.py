"""Timing of the instance labelling of layouts: profiles/ccl_bench.json.  Reports only; nothing is asserted on a time.

The device call alone (``ops.label_instances_launch``: seven launches, no copy, no synchronisation) between two HIP events,
median of ``--reps`` calls after 3 warm-up calls, on Cityscapes-like synthetic layouts -- coarse-grid class ids upsampled
to the plane, as ``synth`` builds its labels, plus a few hundred small blobs of thing classes:

  1x1024x2048      one full-size plane
  8x256x512        a batch of training-size planes

Next to the device time:

  hbm_floor_ms     reading the classes once and writing the int32 ids once at 6.3 TB/s (the achievable HBM rate of the
                   MI355X); the workspace traffic of the seven launches is NOT in this floor
  host_ref_ms      the numpy reference labeller of tests/ccl_fixture.py on the same planes (wall clock, one run)

The device result is compared with the reference before anything is timed.  Clocks are left as found and nothing is set
on the device.

    python tools/ccl_bench.py [--reps 20] [--out profiles/ccl_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HBM_BYTES_PER_S = 6.3e12
THINGS = tuple(range(24, 34))


def layouts(B, H, W, seed, blobs=300, cell=32):
    """(B, H, W) uint8: stuff classes 0..23 on a coarse grid, ``blobs`` rectangles of thing classes per plane."""
    import numpy as np
    rng = np.random.RandomState(seed)
    out = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        coarse = rng.randint(0, 24, ((H + cell - 1) // cell, (W + cell - 1) // cell))
        out[b] = np.kron(coarse, np.ones((cell, cell), np.int64))[:H, :W]
        for _ in range(blobs):
            h, w = int(rng.randint(2, max(H // 16, 3))), int(rng.randint(2, max(W // 16, 3)))
            y, x = int(rng.randint(0, H - h)), int(rng.randint(0, W - w))
            out[b, y:y + h, x:x + w] = THINGS[rng.randint(len(THINGS))]
    return out


def timed(fn, reps):
    import torch
    for _ in range(3):
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ccl_bench.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    import ccl_fixture
    from neurips18_hierchical_image_manipulation_amd import ops
    out = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'cases': {}}
    for name, (B, H, W) in (('1x1024x2048', (1, 1024, 2048)), ('8x256x512', (8, 256, 512))):
        planes = layouts(B, H, W, seed=B)
        dev = torch.from_numpy(planes).cuda()
        case = {}
        for conn in (4, 8):
            t0 = time.perf_counter()
            want = [ccl_fixture.label_reference(p, THINGS, conn, max_objects=65536) for p in planes]
            host_ms = (time.perf_counter() - t0) * 1e3
            inst, counts = ops.label_instances(dev, THINGS, connectivity=conn, max_objects=65536)
            assert counts.tolist() == [w[1] for w in want]
            assert np.array_equal(inst.cpu().numpy(), np.stack([w[0] for w in want]))
            ms = timed(lambda: ops.label_instances_launch(dev, THINGS, conn, 1, 1000, 65536), args.reps)
            floor_ms = planes.size * (1 + 4) / HBM_BYTES_PER_S * 1e3
            case['connectivity_%d' % conn] = {
                'label_instances_ms': ms, 'hbm_floor_ms': round(floor_ms, 5),
                'kernel_over_hbm_floor': round(ms['median'] / floor_ms, 2), 'host_ref_ms': round(host_ms, 2),
                'host_ref_over_kernel': round(host_ms / ms['median'], 1), 'objects': [int(c) for c in counts]}
        out['cases'][name] = case
    out['note'] = ('event-timed medians of single label_instances_launch calls (uint8 classes, things 24..33, min_area 1) '
                   'after 3 warm-up calls; each call also allocates its int32 output through the caching allocator; '
                   'hbm_floor = classes read once + int32 ids written once at 6.3 TB/s, workspace traffic not included; '
                   'host_ref = numpy run-based union-find of tests/ccl_fixture.py, one run')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
