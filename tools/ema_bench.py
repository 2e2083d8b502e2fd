"""Cost of the generator weight EMA on one MI355X (DESIGN.md "Generator weight EMA").

``--part adam``: the generator's optimizer step at the C2 generator arena's real size, three forms timed between HIP events
and interleaved sample by sample (A B C A B C ...), median of ``--samples`` each after warm-up:
    adam          him_adam_step                         28 B per parameter
    fused         him_adam_ema_step                     36 B per parameter
    two_launch    him_adam_step, then him_ema_update    40 B per parameter
``--part step --ema_decay D``: the full C2 training step with the step loop of bench.py (resident batches, warm-up, host
clock around ``--steps`` steps ending in a device synchronise), ``--windows`` timed windows in one process.

Each invocation prints ONE JSON line and, with ``--out``, appends it to that file (a JSON list): run the legs as separate
processes in A/B order, each under its own time limit.  There is no CPU path: without a device the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch  # noqa: E402


def c2_model(ema_decay):
    import bench
    from neurips18_hierchical_image_manipulation_amd import synth
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    wl = bench.WORKLOADS['c2']
    model = create_model(dict(wl['flags'], gpu_ids=[0], isTrain=True, checkpoints_dir='/tmp/him_bench', name='ema_bench',
                              batchSize=wl['bs'], ema_decay=ema_decay))
    model.netG.load_state_dict(synth.init_state_dict(model.netG.state_dict(), 1))
    model.netD.load_state_dict(synth.init_state_dict(model.netD.state_dict(), 2))
    model.optimizer_G.reset_ema()
    return model, wl


def part_adam(args):
    from neurips18_hierchical_image_manipulation_amd._cabi import lib
    from neurips18_hierchical_image_manipulation_amd.models.Pix2Pix_NET import GlobalGenerator
    import bench
    f = bench.WORKLOADS['c2']['flags']
    net = GlobalGenerator(f['label_nc'] + 3, 3, f['ngf'], f['n_downsample_global'], f['n_blocks_global'], 'instance',
                          'reflect', False)
    n = sum((p.numel() + 63) // 64 * 64 for p in net.parameters())       # FlatArena's padded total
    del net
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    p, g, m, ema = (torch.randn(n, device=dev, generator=gen) * s for s in (0.02, 1e-3, 1e-3, 0.02))
    v = torch.rand(n, device=dev, generator=gen) * 1e-6
    st = torch.cuda.current_stream().cuda_stream
    hp = (2e-4, 0.5, 0.999, 1e-8)
    P = lambda t: t.data_ptr()      # noqa: E731
    forms = {
        'adam': lambda k: lib.him_adam_step(P(p), P(g), P(m), P(v), n, *hp, k, st),
        'fused': lambda k: lib.him_adam_ema_step(P(p), P(g), P(m), P(v), P(ema), n, *hp, k, 0.999, st),
        'two_launch': lambda k: (lib.him_adam_step(P(p), P(g), P(m), P(v), n, *hp, k, st),
                                 lib.him_ema_update(P(ema), P(p), n, 0.999, st)),
    }
    k = 1
    for _ in range(args.warmup):
        for fn in forms.values():
            fn(k)
            k += 1
    torch.cuda.synchronize()
    ms = {name: [] for name in forms}
    for _ in range(args.samples):
        for name, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(k)
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
            k += 1
    out = dict(part='adam', device=torch.cuda.get_device_name(0), n_params_padded=n, samples=args.samples,
               bytes_per_param=dict(adam=28, fused=36, two_launch=40))
    for name, v_ in ms.items():
        q = statistics.quantiles(v_, n=4)
        med = statistics.median(v_)
        bpp = out['bytes_per_param'][name]
        out[name] = dict(median_ms=round(med, 4), q1_ms=round(q[0], 4), q3_ms=round(q[2], 4), min_ms=round(min(v_), 4),
                         max_ms=round(max(v_), 4), gb_per_s=round(bpp * n / med / 1e6, 1))
    return out


def part_step(args):
    model, wl = c2_model(args.ema_decay)
    from neurips18_hierchical_image_manipulation_amd import synth
    dev = model.device
    batches = [{k: v.to(dev) for k, v in synth.make_batch(s, 0, wl['bs'], wl['H'], wl['W'], wl['label_nc'], wl['color']).items()}
               for s in range(4)]
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream(dev))
    for b in batches:
        b['ready_event'] = ready
    i = 0
    for _ in range(args.warmup):
        model.optimize_parameters(batches[i % 4])
        i += 1
    windows = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            model.optimize_parameters(batches[i % 4])
            i += 1
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / args.steps * 1e3)
    return dict(part='step', device=torch.cuda.get_device_name(0), workload='c2', ema_decay=args.ema_decay,
                ema_buffer=model.optimizer_G.ema is not None, steps=args.steps, warmup=args.warmup,
                ms_per_step_windows=[round(w, 3) for w in windows], ms_per_step_median=round(statistics.median(windows), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['adam', 'step'], required=True)
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--ema_decay', type=float, default=0.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ema_bench needs the MI355X: there is no CPU path')
    out = (part_adam if args.part == 'adam' else part_step)(args)
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
