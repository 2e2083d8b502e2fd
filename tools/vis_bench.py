#!/usr/bin/env python
"""Cost of turning the tensors of one joint edit (1024 x 2048 canvas, 256 x 256 patch: seven pictures) and of one C2
training step (512 x 256, 35 classes: four pictures) into pictures.  Three columns per picture:

  device_ms   the HIP pass alone between HIP events (median), with the bytes it moves and the rate next to the 6.3 TB/s
              the project takes as achievable HBM rate.  For the small patches this is launch-bound: the rate is not a
              bandwidth figure there.
  util_ms     the whole util.tensor2im / tensor2label call, byte copy to the host included: wall clock, min / median / max
  parent_ms   the same picture by the means the package had before: the float .cpu() copy get_current_visuals() makes,
              then the same formula in plain numpy / torch on the host.  min / median / max.

The condition is util_ms < parent_ms for every picture.  Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch

from neurips18_hierchical_image_manipulation_amd import ops
from neurips18_hierchical_image_manipulation_amd.util import util

HBM_TBS = 6.3


def host_tensor2im(t, normalize):
    a = t.cpu().float().numpy()
    if a.shape[0] == 1:
        a = np.repeat(a, 3, axis=0)
    a = np.transpose(a, (1, 2, 0))
    a = (a + 1) / 2.0 * 255.0 if normalize else a * 255.0
    return np.clip(a, 0, 255).astype(np.uint8)


def host_tensor2label(t, n, table):
    a = t.cpu().float()
    if a.shape[0] > 1:
        a = a.max(0, keepdim=True)[1]
    a = a.numpy()[0]
    valid = (a >= 0) & (a < n) & (a == np.floor(a))
    return table[np.where(valid, a, n).astype(np.int64)]


def stats(v):
    v = np.array(v) * 1e3
    return {'min': round(float(v.min()), 4), 'median': round(float(np.median(v)), 4), 'max': round(float(v.max()), 4)}


def wall(fn, calls, warmup):
    out = []
    for i in range(warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i >= warmup:
            out.append(dt)
    return stats(out)


def device_ms(fn, calls, warmup):
    out = []
    for i in range(warmup + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return round(float(np.median(out)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert a.calls >= 20
    g = torch.Generator().manual_seed(0)
    dev = 'cuda'

    def image(h, w, lo, hi):
        return (torch.rand(3, h, w, generator=g) * (hi - lo) + lo).to(dev)

    def ids(h, w):
        return torch.randint(0, 35, (1, h, w), generator=g).float().to(dev)

    cond = ops.LabelCond(ids(256, 512)[None], 35, None)
    onehot = cond.full()[0]         # what the parent's get_current_visuals copies: materialised once, outside the timing
    cond_ids = ops.LabelCond(cond.label, 35, None)
    table = np.concatenate([util.labelcolormap(35)[:35], np.zeros((1, 3), np.uint8)])
    rows = [
        ('joint/input_image_patch', 'im', image(256, 256, -1, 1), True),
        ('joint/predicted_label_patch', 'label', ids(256, 256), None),
        ('joint/predicted_image_patch', 'im', image(256, 256, -1, 1), True),
        ('joint/GT_label_canvas', 'label', ids(1024, 2048), None),
        ('joint/predicted_label_canvas', 'label', ids(1024, 2048), None),
        ('joint/GT_image_canvas', 'im', image(1024, 2048, 0, 1), False),
        ('joint/predicted_image_canvas', 'im', image(1024, 2048, 0, 1), False),
        ('c2/input_label', 'labelcond', onehot, None),
        ('c2/input_image', 'im', image(256, 512, -1, 1), True),
        ('c2/real_image', 'im', image(256, 512, -1, 1), True),
        ('c2/synthesized_image', 'im', image(256, 512, -1, 1), True),
    ]
    result = []
    for name, kind, t, normalize in rows:
        if kind == 'im':
            dev_fn = lambda: ops.tensor2im_bytes(t, normalize)                       # noqa: E731
            util_fn = lambda: util.tensor2im(t, np.uint8, normalize)                 # noqa: E731
            parent_fn = lambda: host_tensor2im(t, normalize)                         # noqa: E731
            moved = t.numel() * 4 + t.shape[1] * t.shape[2] * 3
        elif kind == 'label':
            dev_fn = lambda: ops.label2color_bytes(t, 35)                            # noqa: E731
            util_fn = lambda: util.tensor2label(t, 35)                               # noqa: E731
            parent_fn = lambda: host_tensor2label(t, 35, table)                      # noqa: E731
            moved = t.numel() * 4 + t.shape[1] * t.shape[2] * 3
        else:
            dev_fn = lambda: ops.label2color_bytes(cond_ids, 35)                     # noqa: E731
            util_fn = lambda: util.tensor2label(cond_ids, 35)                        # noqa: E731
            parent_fn = lambda: host_tensor2label(t, 35, table)                      # noqa: E731
            moved = t.shape[1] * t.shape[2] * (4 + 3)
        assert np.array_equal(util_fn(), parent_fn()), name
        d = device_ms(dev_fn, a.calls, a.warmup)
        u, p = wall(util_fn, a.calls, a.warmup), wall(parent_fn, a.calls, a.warmup)
        result.append({'visual': name, 'shape': list(t.shape), 'device_ms': d, 'bytes_moved': int(moved),
                       'device_tb_per_s': round(moved / (d * 1e-3) / 1e12, 4), 'util_ms': u, 'parent_ms': p,
                       'util_faster': bool(u['median'] < p['median'])})
    props = torch.cuda.get_device_properties(0)
    line = {'metric': 'vis_ms', 'calls': a.calls, 'warmup': a.warmup, 'hbm_tb_per_s_taken_as_achievable': HBM_TBS,
            'device': torch.cuda.get_device_name(0), 'compute_units': props.multi_processor_count,
            'clock_rate_khz_as_found': getattr(props, 'clock_rate', None), 'host_threads': torch.get_num_threads(),
            'all_util_faster': all(r['util_faster'] for r in result), 'visuals': result}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
