"""Timing of the evaluation metrics: profiles/metrics_bench.json.

Each device call alone between two HIP events (median of ``--reps`` launches after warm-up), at 3x1024x2048 whole image
and at 3x256x256 with a box:

  (a) image_metrics_ms       him_image_metrics (SSIM + squared / absolute error sums), without the map
  (b) confusion_ms           him_confusion, n = 35, int64 prediction against fp32 ground truth
  (c) torch_ssim_ms          the same SSIM written with torch's GPU operators (depthwise conv2d with the Gaussian over the
                             five moment planes), as a yardstick only
  (d) torch_bincount_ms      the same matrix as torch.bincount(gt * n + pred)
  (e) hbm_floor_ms           reading the two images once at 6.3 TB/s (the achievable HBM rate of the MI355X)
  (f) evaluate_mask2image    share of the loop's wall clock outside the generator forward, tiny generator at 256x256

Clocks are left as found and nothing is set on the device.

    python tools/metrics_bench.py [--reps 20] [--out profiles/metrics_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.3e12


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


def torch_ssim(a, b, win, L):
    """SSIM summed over the valid windows with torch operators: the preset's bytes, five depthwise convolutions."""
    import torch
    import torch.nn.functional as F
    qa = ((a + 1) / 2 * 255).clamp(0, 255).trunc()
    qb = ((b + 1) / 2 * 255).clamp(0, 255).trunc()
    C = a.shape[1]
    x = torch.cat([qa, qb, qa * qa, qb * qb, qa * qb], 1)
    k = (win[:, None] * win[None, :]).expand(5 * C, 1, 11, 11).contiguous()
    m = F.conv2d(x, k, groups=5 * C)
    mu_a, mu_b, eaa, ebb, eab = m.split(C, 1)
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    s = (2 * mu_a * mu_b + c1) * (2 * (eab - mu_a * mu_b) + c2) / \
        ((mu_a * mu_a + mu_b * mu_b + c1) * (eaa - mu_a * mu_a + ebb - mu_b * mu_b + c2))
    d = qa - qb
    return s.double().sum((2, 3)), (d * d).double().sum((2, 3)), d.abs().double().sum((2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'metrics_bench.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    from neurips18_hierchical_image_manipulation_amd import ops, synth
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    from neurips18_hierchical_image_manipulation_amd.util import metrics
    g = np.exp(-((np.arange(11, dtype=np.float64) - 5.0) ** 2) / 4.5)
    win = torch.from_numpy((g / g.sum()).astype(np.float32)).cuda()
    gen = torch.Generator(device='cuda').manual_seed(7)
    out = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'cases': {}}
    preset = dict(scale=127.5, offset=127.5, quantize=True, data_range=255.0)
    for name, (H, W, box) in (('3x1024x2048', (1024, 2048, None)), ('3x256x256_box', (256, 256, (64, 64, 191, 191)))):
        a = torch.rand((1, 3, H, W), device='cuda', generator=gen) * 2 - 1
        b = (a + (torch.rand((1, 3, H, W), device='cuda', generator=gen) - 0.5) * 0.3).clamp(-1, 1)
        dbox = None if box is None else torch.tensor([box], dtype=torch.int32, device='cuda')
        ca, cb = (a, b) if box is None else (a[:, :, box[1]:box[3] + 1, box[0]:box[2] + 1].contiguous(),
                                             b[:, :, box[1]:box[3] + 1, box[0]:box[2] + 1].contiguous())
        mine = timed(lambda: ops.image_metrics(a, b, box=dbox, **preset), args.reps)
        theirs = timed(lambda: torch_ssim(ca, cb, win, 255.0), args.reps)
        sums, _ = ops.image_metrics(a, b, box=dbox, **preset)
        ts, tq, ta = torch_ssim(ca, cb, win, 255.0)
        agree = float(((sums[0, :, 0] - ts[0]).abs() / ts[0].abs()).max())
        assert agree < 1e-4 and torch.equal(sums[0, :, 2], tq[0]) and torch.equal(sums[0, :, 3], ta[0]), agree
        n = 35
        gt = torch.randint(0, n, (1, 1, H, W), device='cuda', generator=gen).float()
        pred = torch.where(torch.rand((1, 1, H, W), device='cuda', generator=gen) < 0.8, gt.long(),
                           torch.randint(0, n, (1, 1, H, W), device='cuda', generator=gen))
        conf = timed(lambda: ops.confusion(pred, gt, n), args.reps)
        binc = timed(lambda: torch.bincount((gt.long() * n + pred).reshape(-1), minlength=n * n), args.reps)
        assert torch.equal(ops.confusion(pred, gt, n)[0].reshape(-1),
                           torch.bincount((gt.long() * n + pred).reshape(-1), minlength=n * n))
        read = ca.numel() * 4 * 2
        floor_ms = read / HBM_BYTES_PER_S * 1e3
        out['cases'][name] = {
            'image_metrics_ms': mine, 'torch_ssim_ms': theirs, 'hbm_floor_ms': round(floor_ms, 5),
            'torch_over_kernel': round(theirs['median'] / mine['median'], 2),
            'kernel_over_hbm_floor': round(mine['median'] / floor_ms, 2),
            'ssim_sum_rel_diff_vs_torch': agree, 'confusion_ms': conf, 'torch_bincount_ms': binc,
            'bincount_over_kernel': round(binc['median'] / conf['median'], 2)}
    # (f) the evaluation loop: wall clock of evaluate_mask2image against the generator forward alone
    flags = dict(model='pix2pixHD_condImg', netG='global', ngf=16, ndf=8, n_downsample_global=3, n_blocks_global=3, num_D=2,
                 n_layers_D=3, label_nc=35, no_instance=True)
    model = create_model(dict(flags, gpu_ids=[0], isTrain=True, checkpoints_dir='/tmp/him_metrics_bench', name='m'))
    model.netG.load_state_dict(synth.init_state_dict(model.netG.state_dict(), 1))
    data = [{k: v.cuda() for k, v in synth.make_batch(i, 0, 1, 256, 256).items()} for i in range(16)]

    def forward_only():
        for d in data:
            model.inference(d['label'], d['inst'], d['image'], d['mask_in'], d['mask_out'])
        torch.cuda.synchronize()

    def with_metrics():
        metrics.evaluate_mask2image(model, data, len(data)).summary()

    for fn in (forward_only, with_metrics):
        fn()
    walls = {}
    for name, fn in (('forward_only', forward_only), ('evaluate_mask2image', with_metrics)):
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3 / len(data))
        walls[name] = round(statistics.median(ts), 4)
    out['evaluate_mask2image'] = dict(ms_per_sample=walls, samples=len(data), shape=[256, 256],
                                      share_outside_forward=round(1 - walls['forward_only'] / walls['evaluate_mask2image'], 4))
    out['note'] = ('event-timed medians of single calls after 3 warm-up calls; torch_ssim / torch_bincount are yardsticks '
                   'written with torch GPU operators, on the cropped tensors for the box case; hbm_floor = both images '
                   'read once at 6.3 TB/s')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
