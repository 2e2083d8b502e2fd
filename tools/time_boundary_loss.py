"""Cost of the boundary-weighted and surface losses at the box2mask benchmark shape (256x256, batch 32):
the training step with the three settings unset and set, and the new loss calls alone next to the unweighted ones.

    python tools/time_boundary_loss.py [--steps 30] [--warmup 5] [--out FILE]

Prints one JSON object; times are medians over ``--steps`` repetitions measured with device events after ``--warmup``
untimed ones (the step: wall clock around ``--steps`` steps, as bench.py does)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurips18_hierchical_image_manipulation_amd import ops, synth  # noqa: E402
from neurips18_hierchical_image_manipulation_amd.models import create_model  # noqa: E402

B, H, W, C = 32, 256, 256, 35


def step_ms(steps, warmup, **settings):
    model = create_model(dict(model='AE_maskgen_twostream', gpu_ids=[0], isTrain=True, checkpoints_dir='/tmp/him_bench',
                              name='time_boundary', batchSize=B, **settings))
    model.netG.load_state_dict(synth.init_state_dict(model.netG.state_dict(), 1))
    model.netD.load_state_dict(synth.init_state_dict(model.netD.state_dict(), 2))
    batches = [{k: v.cuda() for k, v in synth.make_box2mask_batch(s, 0, B, H, W).items()} for s in range(4)]

    def step(i):
        b = batches[i % 4]
        return model.forward(b['label'], None, b['mask_ctx_in'], None, b['mask_out'], b['mask_obj_inst'], b['cls'], b['mask_in'])

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(warmup + i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def call_us(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return round(statistics.median(times), 2)


def calls(steps, warmup):
    b = {k: v.cuda() for k, v in synth.make_box2mask_batch(0, 0, B, H, W).items()}
    label, gate, t = b['label'].float().contiguous(), b['mask_out'].float().contiguous(), b['mask_obj_inst'].float().contiguous()
    logp = torch.log_softmax(torch.randn(B, C, H, W, device='cuda'), 1).requires_grad_(True)
    p = (torch.rand(B, 1, H, W, device='cuda') * 0.98 + 0.01).requires_grad_(True)
    d2, od2, sd = ops.boundary_dist2(label), ops.boundary_dist2(t), ops.surface_dists(t)
    out = {}

    def both(name, fn, leaf):
        out[name + '_fwd_us'] = call_us(fn, steps, warmup)
        loss = fn()
        out[name + '_bwd_us'] = call_us(lambda: torch.autograd.grad(loss, leaf, retain_graph=True), steps, warmup)

    both('masked_nll', lambda: ops.masked_nll(logp, label, gate), logp)
    both('boundary_weighted_nll', lambda: ops.boundary_weighted_nll(logp, label, gate, 4.0, 5.0, dist2=d2), logp)
    both('bce_mean', lambda: ops.bce_mean(p, t), p)
    both('boundary_weighted_bce', lambda: ops.boundary_weighted_bce(p, t, 4.0, 5.0, dist2=od2), p)
    both('l1_mean', lambda: ops.l1_mean(p, t), p)
    both('boundary_weighted_l1', lambda: ops.boundary_weighted_l1(p, t, 4.0, 5.0, dist2=od2), p)
    both('surface_loss', lambda: ops.surface_loss(p, t, dists=sd), p)
    out['boundary_dist2_label_us'] = call_us(lambda: ops.boundary_dist2(label), steps, warmup)
    out['boundary_dist2_object_us'] = call_us(lambda: ops.boundary_dist2(t), steps, warmup)
    out['surface_dists_us'] = call_us(lambda: ops.surface_dists(t), steps, warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'shape': '%dx%dx%d, %d classes' % (B, H, W, C), 'device': torch.cuda.get_device_name(0),
           'step_ms_default': round(step_ms(a.steps, a.warmup), 3),
           'step_ms_boundary_weight_4_surface_weight_1': round(step_ms(a.steps, a.warmup, boundary_weight=4.0, surface_weight=1.0), 3),
           'step_ms_default_again': round(step_ms(a.steps, a.warmup), 3),
           'calls (event-timed, launch overhead of the autograd wrapper included)': calls(a.steps, a.warmup)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
