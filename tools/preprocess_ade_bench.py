"""Timing of the ADE20K preprocessing step: profiles/preprocess_ade_bench.json.

A seeded raw tree of 16 synthetic 512x683 ``_seg.png`` files with about 40 elliptical instances each
(tests/preprocess_ade_fixture.py), then, each as min / median / max over the images:

  (a) device_call_ms        him_ade_decode alone (three launches), between two HIP events, bytes already on the device:
                            on the vector path (aligned base), on the element path (the same bytes at a base shifted by
                            one byte), and for both with 20 calls queued back to back between the events (per call)
  (b) convert_ms_per_image  preprocess_ade.convert per image, wall clock: PNG decode, attribute file, upload, device
                            call, copy back, two PNGs, the JPEG copy and the JSON file
  (c) numpy_restatement_ms  the tests' numpy restatement of the reference's decode, relabel and box loops plus the box
                            dict, on the decoded bytes, same host, one thread
  (d) png_decode_ms         decoding the _seg.png alone (one thread)

Warm-up calls come first; clocks are left as found and nothing is set on the device.  Nothing is asserted on the times.

    python tools/preprocess_ade_bench.py [--images 16] [--out profiles/preprocess_ade_bench.json]
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
import preprocess_ade_fixture as fx                                      # noqa: E402

QUEUED = 20


def mmm(values):
    return {'min': round(min(values), 4), 'median': round(statistics.median(values), 4), 'max': round(max(values), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=16)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'preprocess_ade_bench.json'))
    args = ap.parse_args()
    import torch
    from neurips18_hierchical_image_manipulation_amd import ops, preprocess_ade
    H, W = 512, 683
    names = fx.objectnames()
    cases = [('s%d' % i, ) + fx.synth(2000 + i, H, W, 40, kinds='ellipse') for i in range(args.images)]
    with tempfile.TemporaryDirectory() as d:
        root = os.path.join(d, 'ade20k')
        listed = fx.write_raw_tree(root, cases)
        # (d) decode alone and (c) the restatement on the decoded bytes
        decode_ms, numpy_ms, wanted, n_inst = [], [], [], []
        preprocess_ade._read_seg(listed[0][0].replace('.jpg', '_seg.png'))
        fx.restate(cases[0][1])
        for jpg, seg, lines in listed:
            t0 = time.perf_counter()
            got = preprocess_ade._read_seg(jpg.replace('.jpg', '_seg.png'))
            decode_ms.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(got, seg)
            t0 = time.perf_counter()
            cls, label, inst, rows = fx.restate(seg)
            info = fx.rows_to_info(H, W, rows, fx.names_of(lines), names)
            numpy_ms.append((time.perf_counter() - t0) * 1e3)
            wanted.append((label, inst, rows, info))
            n_inst.append(len(rows) - 1)
        # (a) the device call between events: aligned base (vector path) and a base shifted by one byte (element path)
        device_ms = {'vector': [], 'element': [], 'vector_queued': [], 'element_queued': []}
        for (tag, seg, lines), (label, inst, rows, _) in zip(cases, wanted):
            aligned = torch.from_numpy(seg).cuda()
            flat = torch.zeros(seg.size + 1, dtype=torch.uint8, device='cuda')
            shifted = flat[1:].view(seg.shape)
            shifted.copy_(aligned)
            assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 1
            for path, t in (('vector', aligned), ('element', shifted)):
                got = ops.ade_decode(t, fx.KEEP)                        # warm-up, and the result is the restatement's
                assert np.array_equal(got[0].cpu().numpy(), label) and np.array_equal(got[1].cpu().numpy(), inst)
                assert np.array_equal(got[2], rows)
                for key, calls in ((path, 1), (path + '_queued', QUEUED)):
                    times = []
                    for _ in range(5):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(calls):
                            ops.ade_decode_launch(t, fx.KEEP)
                        e1.record()
                        e1.synchronize()
                        times.append(e0.elapsed_time(e1) / calls)
                    device_ms[key].append(statistics.median(times))
        # (b) convert, wall clock per image (the first pass over the tree is the warm-up)
        convert_ms = []
        for rep in range(4):
            t0 = time.perf_counter()
            n = preprocess_ade.convert(root, n_val=2)
            if rep:
                convert_ms.append((time.perf_counter() - t0) * 1e3 / n)
        for i, (label, inst, rows, info) in enumerate(wanted):
            phase, prefix = preprocess_ade.output_names(len(wanted), 2)[i]
            with open(os.path.join(root, phase + '_bbox', prefix + preprocess_ade.BBOX_SUF)) as f:
                assert f.read() == json.dumps(info)
    out = {'shape': [H, W], 'images': len(cases), 'instances_per_image': mmm(n_inst),
           'device': torch.cuda.get_device_name(0), 'decode_threads': preprocess_ade.DECODE_THREADS,
           'device_call_ms': {k: mmm(v) for k, v in device_ms.items()}, 'queued_calls': QUEUED,
           'convert_ms_per_image': mmm(convert_ms), 'convert_passes': len(convert_ms),
           'numpy_restatement_ms': mmm(numpy_ms), 'png_decode_ms': mmm(decode_ms),
           'note': 'device_call: median of 5 event-timed repetitions per image, then min/median/max over images; *_queued: '
                   '%d calls queued between the two events, per call; element: the same bytes at a base shifted by one '
                   'byte; convert: wall clock of a whole pass over the tree divided by the image count, min/median/max '
                   'over the passes; numpy_restatement and png_decode: one thread, per image' % QUEUED}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
