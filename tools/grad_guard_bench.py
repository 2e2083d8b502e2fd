"""Cost of the gradient guard on one MI355X (DESIGN.md "Gradient guard").

The optimizer step at the C2 generator's and discriminator's real arena sizes (FlatArena's padded totals, with their real
segment tables), three forms timed between HIP events and interleaved sample by sample (A B C A B C ...), median of
``--samples`` each after warm-up:
    adam      him_adam_step                                28 B per parameter
    guarded   him_grad_stats, then him_adam_guarded_step   32 B per parameter + two small launches
    stats     him_grad_stats alone                          4 B per parameter
Expectation from the bytes moved: guarded = 32 / 28 of adam.

Prints ONE JSON line and, with ``--out``, appends it to that file (a JSON list).  There is no CPU path: without a device
the tool fails."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch  # noqa: E402


def c2_tables():
    """{'G': (offsets, sizes, total), 'D': ...} of the C2 workload's two arenas, from the module definitions alone."""
    import bench
    from neurips18_hierchical_image_manipulation_amd.models.Discriminator_NET import MultiscaleDiscriminator
    from neurips18_hierchical_image_manipulation_amd.models.Pix2Pix_NET import GlobalGenerator
    from neurips18_hierchical_image_manipulation_amd.options import complete
    opt = complete(dict(bench.WORKLOADS['c2']['flags']))
    in_nc = opt.label_nc + 3
    netG = GlobalGenerator(in_nc, 3, opt.ngf, opt.n_downsample_global, opt.n_blocks_global, 'instance', 'reflect', False)
    d_nc = in_nc + opt.output_nc + (0 if opt.no_instance else 1)
    netD = MultiscaleDiscriminator(d_nc, opt.ndf, opt.n_layers_D, opt.norm, opt.no_lsgan, opt.num_D,
                                   not opt.no_ganFeat_loss)
    out = {}
    for tag, net in (('G', netG), ('D', netD)):
        sizes = [p.numel() for p in net.parameters()]
        offsets, off = [], 0
        for n in sizes:
            offsets.append(off)
            off += (n + 63) // 64 * 64
        out[tag] = (offsets, sizes, off)
    return out


def measure(tag, offsets, sizes, n, args):
    from neurips18_hierchical_image_manipulation_amd._cabi import lib
    from neurips18_hierchical_image_manipulation_amd.optim import guard_tables
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    p, g, m = (torch.randn(n, device=dev, generator=gen) * s for s in (0.02, 1e-3, 1e-3))
    v = torch.rand(n, device=dev, generator=gen) * 1e-6
    seg, work = guard_tables(offsets, sizes, n)
    seg_dev = torch.tensor(seg, dtype=torch.int64).to(dev)
    seg_out = torch.zeros(len(seg), 2, dtype=torch.float64, device=dev)
    stt = torch.zeros(8, dtype=torch.float64, device=dev)
    ws_bytes = int(lib.him_grad_stats_ws(n, len(seg)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    hp = (2e-4, 0.5, 0.999, 1e-8)
    P = lambda t: t.data_ptr()      # noqa: E731
    stats = lambda: lib.him_grad_stats(P(g), n, P(seg_dev), len(seg), P(seg_out), P(stt), 1e30, P(ws), ws_bytes, st)  # noqa: E731
    forms = {
        'adam': lambda k: lib.him_adam_step(P(p), P(g), P(m), P(v), n, *hp, k, st),
        'guarded': lambda k: (stats(), lib.him_adam_guarded_step(P(p), P(g), P(m), P(v), 0, n, *hp, k, 0.0, P(stt), st)),
        'stats': lambda k: stats(),
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
    bpp = dict(adam=28, guarded=32, stats=4)
    out = dict(arena=tag, n_params_padded=n, segments=len(seg), chunks=len(work), ws_bytes=ws_bytes, samples=args.samples,
               bytes_per_param=bpp, nonfinite=float(stt[1]), clip_coef=float(stt[3]))
    for name, v_ in ms.items():
        q = statistics.quantiles(v_, n=4)
        med = statistics.median(v_)
        out[name] = dict(median_ms=round(med, 4), q1_ms=round(q[0], 4), q3_ms=round(q[2], 4), min_ms=round(min(v_), 4),
                         max_ms=round(max(v_), 4), gb_per_s=round(bpp[name] * n / med / 1e6, 1))
    out['guarded_over_adam'] = round(out['guarded']['median_ms'] / out['adam']['median_ms'], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('grad_guard_bench needs the MI355X: there is no CPU path')
    out = dict(tool='grad_guard_bench', device=torch.cuda.get_device_name(0),
               arenas=[measure(tag, *t, args) for tag, t in c2_tables().items()])
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
