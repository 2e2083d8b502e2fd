"""Cost of the differentiable discriminator augmentation on one MI355X.

Part 1, the passes alone at the C2 discriminator input (B, 41, 256, 512: 35 one-hot + 3 condition + 3 image channels),
timed between HIP events and interleaved sample by sample (A B C A B C ...), median of ``--samples`` with min..max:
    copy      him_copy_channels moving the same tensor: one read + one write, the yardstick
    fwd       him_diffaug_fwd, policy colour | translation | cutout, a drawn table
    bwd       him_diffaug_bwd, every channel
    bwd_img   him_diffaug_bwd, the three image channels only (what the generator's path runs)
    fwd_geo   him_diffaug_fwd, translation | cutout only (no reduction launches)
``ratio`` = copy / pass.  Part 2 (``--step``): the C2 training step with --diffaug color,translation,cutout against the
step with it off, ``--steps`` steps each, timed per step between events on the main stream, in the order off / on / off.

Prints ONE JSON line and, with ``--out``, appends it to that file (a JSON list).  There is no CPU path."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch  # noqa: E402


def _stat(v, nbytes=None):
    med = statistics.median(v)
    out = dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4))
    if nbytes:
        out['gb_per_s'] = round(nbytes / med / 1e6, 1)
    return out


def passes(args):
    import bench
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd._cabi import lib
    wl = bench.WORKLOADS['c2']
    B, H, W = wl['bs'], wl['H'], wl['W']
    C = wl['label_nc'] + 3 + 3
    c0 = C - 3
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, C, H, W, device=dev, generator=gen)
    y = torch.empty_like(x)
    yi = torch.empty(B, 3, H, W, device=dev)
    table, ch, cw = ops.diffaug_draw(B, H, W, 0, 0, 0, 7, device=dev)
    nb = int(lib.him_diffaug_ws(B, H, W))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()      # noqa: E731
    full = 2 * x.numel() * 4
    forms = {
        'copy': (lambda: lib.him_copy_channels(P(x), C, 0, P(y), C, 0, C, B, H * W, 0, 0, 0, st), full),
        'fwd': (lambda: lib.him_diffaug_fwd(P(x), P(table), P(y), B, C, c0, H, W, ch, cw, 7, P(ws), nb, st), full),
        'bwd': (lambda: lib.him_diffaug_bwd(P(x), P(table), P(y), B, C, c0, H, W, ch, cw, 7, 0, C, P(ws), nb, st), full),
        'bwd_img': (lambda: lib.him_diffaug_bwd(P(x), P(table), P(yi), B, C, c0, H, W, ch, cw, 7, c0, 3, P(ws), nb, st),
                    3 * yi.numel() * 4),
        'fwd_geo': (lambda: lib.him_diffaug_fwd(P(x), P(table), P(y), B, C, c0, H, W, ch, cw, 6, 0, 0, st), full),
    }
    for _ in range(args.warmup):
        for fn, _n in forms.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(args.samples):
        for name, (fn, _n) in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    out = dict(shape=[B, C, H, W], c0=c0, cutout=[ch, cw], ws_bytes=nb, samples=args.samples,
               table=table.cpu().tolist())
    for name, (_fn, nbytes) in forms.items():
        out[name] = _stat(ms[name], nbytes)
    for name in ('fwd', 'bwd', 'fwd_geo'):
        out[name]['ratio_to_copy'] = round(out['copy']['median_ms'] / out[name]['median_ms'], 4)
    return out


def step_times(policy, args):
    import bench
    from neurips18_hierchical_image_manipulation_amd import synth
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    wl = bench.WORKLOADS['c2']
    bs, H, W = wl['bs'], wl['H'], wl['W']
    dev = torch.device('cuda', 0)
    model = create_model(dict(wl['flags'], gpu_ids=[0], isTrain=True, checkpoints_dir='/tmp/him_bench', name='diffaug_bench',
                              batchSize=bs, diffaug=policy))
    model.netG.load_state_dict(synth.init_state_dict(model.netG.state_dict(), 1))
    model.netD.load_state_dict(synth.init_state_dict(model.netD.state_dict(), 2))
    batches = [{k: v.to(dev) for k, v in synth.make_batch(s, 0, bs, H, W, wl['label_nc'], wl['color']).items()}
               for s in range(4)]
    for i in range(args.warmup):
        model.optimize_parameters(batches[i % 4])
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    marks[0].record()
    for i in range(args.steps):
        model.optimize_parameters(batches[i % 4])
        marks[i + 1].record()
    torch.cuda.synchronize()
    v = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
    total = marks[0].elapsed_time(marks[-1]) / args.steps
    del model
    torch.cuda.empty_cache()
    return dict(policy=policy, mean_ms=round(total, 3), **_stat(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--step', action='store_true', help='also time the C2 training step with the policy off / on / off')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('diffaug_bench needs the MI355X: there is no CPU path')
    out = dict(tool='diffaug_bench', device=torch.cuda.get_device_name(0), passes=passes(args))
    if args.step:
        out['step'] = [step_times(p, args) for p in ('', 'color,translation,cutout', '')]
    print(json.dumps(out), flush=True)
    if args.out:
        rows = []
        if os.path.isfile(args.out):
            with open(args.out) as f:
                rows = json.load(f)
        rows.append(out)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
