"""Times the calls of the feature-space set metrics between HIP events at an evaluation size of 5000 descriptors of 512
features per set (relu5_1 of VGG19): him_kid_sums on 100 subsets of 1000 rows, him_feat_moments on the whole set and on
one batch of 16 rows, him_feat_pool on a batch of relu5_1 maps.  The KID workload is counted in full
-- 100 subsets x 3 blocks x 1000^2 pairs x 512 x 2 = 0.307 TFLOP of fp64 products, the symmetric halves included
although the kernel skips them -- and its floor is that count over the fp64 matrix peak of the MI355X (78.6
TFLOP/s, AMD's published figure).  Writes profiles/featdist_bench.json.  Needs the MI355X; nothing is promised in
advance."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neurips18_hierchical_image_manipulation_amd import ops  # noqa: E402
from neurips18_hierchical_image_manipulation_amd.util import metrics  # noqa: E402

FP64_MATRIX_FLOPS = 78.6e12       # MI355X peak, v_mfma_f64_16x16x4_f64


def timed(fn, reps):
    """Milliseconds per call, each call alone between two events."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=5000)
    ap.add_argument('--dim', type=int, default=512)
    ap.add_argument('--subsets', type=int, default=100)
    ap.add_argument('--subset-size', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'featdist_bench.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'featdist_bench needs the GPU'
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((a.rows, a.dim), generator=g, device=dev).abs()
    y = torch.randn((a.rows, a.dim), generator=g, device=dev).abs() * 1.1
    m = min(a.subset_size, a.rows)
    ix = torch.from_numpy(metrics.kid_subsets(0, 0, a.rows, a.subsets, m)).to(dev)
    iy = torch.from_numpy(metrics.kid_subsets(0, 1, a.rows, a.subsets, m)).to(dev)
    res = dict(device=torch.cuda.get_device_name(0), rows=a.rows, dim=a.dim, n_subsets=a.subsets, subset_size=m)
    res['kid_sums'] = timed(lambda: ops.kid_sums(x, y, ix, iy), a.reps)
    out, status = ops.kid_sums(x, y, ix, iy)
    again, _ = ops.kid_sums(x, y, ix, iy)
    res['kid_status'] = int(status.item())
    res['kid_bit_identical'] = bool(torch.equal(out, again))
    est = (out[:, 0] + out[:, 1]) / (m * (m - 1.0)) - 2.0 * out[:, 2] / (m * float(m))
    res['kid_mean'] = float(est.mean())
    flop = a.subsets * 3.0 * m * m * a.dim * 2.0
    res['kid_counted_tflop'] = flop / 1e12
    res['kid_executed_tflop'] = a.subsets * (2.0 * (m * m / 2.0) + m * m) * a.dim * 2.0 / 1e12   # about: half of xx and yy
    res['kid_floor_ms'] = flop / FP64_MATRIX_FLOPS * 1e3
    res['kid_floor_over_time'] = res['kid_floor_ms'] / res['kid_sums']['median_ms']
    res['kid_counted_tflops'] = flop / 1e12 / (res['kid_sums']['median_ms'] * 1e-3)
    s, q = ops.feat_moment_buffers(a.dim, dev)
    res['feat_moments_all_rows'] = timed(lambda: ops.feat_moments(x, 0, a.rows, s, q), a.reps)
    res['feat_moments_16_rows'] = timed(lambda: ops.feat_moments(x, 0, 16, s, q), a.reps)
    maps = torch.rand((16, a.dim, 16, 32), generator=g, device=dev)
    feat = torch.empty((16, a.dim), device=dev)
    res['feat_pool_16x%dx16x32' % a.dim] = timed(lambda: ops.feat_pool(maps, feat, 0), a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
