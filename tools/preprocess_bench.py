"""Timing of the Cityscapes box pass: profiles/preprocess_bench.json.

A seeded directory of 32 synthetic 1024x2048 instance / label pairs (40-100 elliptical instances each: disconnected
parts and mixed classes under one id included, tests/preprocess_fixture.py) in the raw Cityscapes layout, then, each as
min / median / max over the 32 pairs:

  (a) device_pass_ms      him_inst_summary alone, between two HIP events, planes already on the device
  (b) construct_box_ms    preprocess.construct_box per image, wall clock: decode, upload, device pass, JSON file
  (c) numpy_restatement_ms  the tests' numpy restatement of the reference's loop on the decoded arrays, same host
  (d) png_decode_ms       decoding the two PNGs alone (one thread)

Warm-up calls come first; clocks are left as found and nothing is set on the device.

    python tools/preprocess_bench.py [--pairs 32] [--out profiles/preprocess_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import preprocess_fixture as fx                                          # noqa: E402


def mmm(values):
    return {'min': round(min(values), 4), 'median': round(statistics.median(values), 4), 'max': round(max(values), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'preprocess_bench.json'))
    args = ap.parse_args()
    import torch
    from PIL import Image
    from neurips18_hierchical_image_manipulation_amd import ops, preprocess
    H, W = 1024, 2048
    rng = np.random.RandomState(2024)
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, 'gtFine'), os.path.join(d, 'bbox')
        os.makedirs(dst)
        files, n_obj = [], []
        for i in range(args.pairs):
            inst, label = fx.synth_pair(1000 + i, H, W, int(rng.randint(40, 101)), max_axis=120)
            city = os.path.join(src, 'city%d' % (i % 4))
            os.makedirs(city, exist_ok=True)
            stem = 'city%d_%06d_000019' % (i % 4, i)
            paths = (os.path.join(city, stem + '_gtFine_instanceIds.png'), os.path.join(city, stem + '_gtFine_labelIds.png'))
            Image.fromarray(inst).save(paths[0])
            Image.fromarray(label, 'L').save(paths[1])
            files.append(paths)
        files.sort()
        # (d) decode alone and (c) the restatement, on the decoded arrays
        decode_ms, numpy_ms, decoded, wanted = [], [], [], []
        preprocess._decode_pair(*files[0])
        for paths in files:
            t0 = time.perf_counter()
            pair = preprocess._decode_pair(*paths)
            decode_ms.append((time.perf_counter() - t0) * 1e3)
            decoded.append(pair)
        fx.restate(*decoded[0])
        for inst, label in decoded:
            t0 = time.perf_counter()
            rows = fx.restate(inst, label)
            numpy_ms.append((time.perf_counter() - t0) * 1e3)
            wanted.append(rows)
            n_obj.append(len(rows))
        # (a) the device pass between events
        dev = [(torch.from_numpy(i).cuda(), torch.from_numpy(l).cuda()) for i, l in decoded]
        for i, l in dev[:4]:
            ops.inst_summary(i, l, max_objects=preprocess.MAX_OBJECTS)
        device_ms = []
        for (i, l), want in zip(dev, wanted):
            best = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.inst_summary_launch(i, l, max_objects=preprocess.MAX_OBJECTS)
                e1.record()
                e1.synchronize()
                best.append(e0.elapsed_time(e1))
            device_ms.append(statistics.median(best))
            assert np.array_equal(ops.inst_summary(i, l, max_objects=preprocess.MAX_OBJECTS), want)
        del dev
        # (b) construct_box, wall clock per image (a warm-up pass over the directory first)
        box_ms = []
        stdout = sys.stdout
        for rep in range(4):
            sys.stdout = open(os.devnull, 'w')
            try:
                t0 = time.perf_counter()
                preprocess.construct_box(src, fx.INST_PATTERN, fx.CLS_PATTERN, dst)
                if rep:                                  # the first pass over the directory is the warm-up
                    box_ms.append((time.perf_counter() - t0) * 1e3 / len(files))
            finally:
                sys.stdout.close()
                sys.stdout = stdout
        # per-image times of a pass with the pool idle between images are not separable from the overlap; the figure per
        # image is the directory's wall clock over its image count, for each of the three passes
        for (ipath, _), want in zip(files, wanted):
            with open(os.path.join(dst, os.path.splitext(os.path.basename(ipath))[0] + '.json')) as f:
                assert f.read() == json.dumps(fx.rows_to_info(H, W, want))
    out = {'shape': [H, W], 'pairs': len(files), 'objects_per_pair': mmm(n_obj), 'device': torch.cuda.get_device_name(0),
           'decode_threads': preprocess.DECODE_THREADS,
           'device_pass_ms': mmm(device_ms), 'construct_box_ms_per_image': mmm(box_ms),
           'construct_box_passes': len(box_ms), 'numpy_restatement_ms': mmm(numpy_ms), 'png_decode_ms': mmm(decode_ms),
           'note': 'device_pass: median of 5 event-timed launches per pair, then min/median/max over pairs; '
                   'construct_box: wall clock of a whole pass over the directory divided by the image count, '
                   'min/median/max over the passes; numpy_restatement and png_decode: one thread, per pair'}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out))
    assert out['construct_box_ms_per_image']['max'] < out['numpy_restatement_ms']['min'], 'construct_box is not below numpy'


if __name__ == '__main__':
    main()
