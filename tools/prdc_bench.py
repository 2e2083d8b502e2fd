"""Times the two calls of the k-nearest-neighbour measures (precision, recall, density, coverage) between HIP events at
an evaluation size of 5000 descriptors of 512 features per set (relu5_1 of VGG19) with k = 5: him_knn_radii on one set
and him_knn_membership of one set against the other, each call alone, median of 5.  The workload is counted in full --
rows^2 pairs x 512 x 2 = 0.0256 TFLOP of fp64 products per call, the self pairs included -- and its floor is that count
over the fp64 matrix peak of the MI355X (78.6 TFLOP/s, AMD's published figure).  Also records that two identical calls
gave identical bits, and the four measures of the two random sets.  Writes profiles/prdc_bench.json.  Needs the MI355X;
nothing is promised in advance."""
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
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'prdc_bench.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'prdc_bench needs the GPU'
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    real = torch.randn((a.rows, a.dim), generator=g, device=dev).abs()
    fake = torch.randn((a.rows, a.dim), generator=g, device=dev).abs() * 1.02
    res = dict(device=torch.cuda.get_device_name(0), rows=a.rows, dim=a.dim, nearest_k=a.k)
    flop = float(a.rows) * a.rows * a.dim * 2.0
    res['counted_tflop_per_call'] = flop / 1e12
    res['floor_ms_per_call'] = flop / FP64_MATRIX_FLOPS * 1e3
    r2, status = ops.knn_radii(real, a.k)
    again, _ = ops.knn_radii(real, a.k)
    res['knn_radii'] = timed(lambda: ops.knn_radii(real, a.k), a.reps)
    res['knn_radii_bit_identical'] = bool(torch.equal(r2, again))
    rows, cols, _ = ops.knn_membership(fake, real, r2, status=status)
    rows2, cols2, _ = ops.knn_membership(fake, real, r2)
    res['knn_membership'] = timed(lambda: ops.knn_membership(fake, real, r2), a.reps)
    res['knn_membership_rows_only'] = timed(lambda: ops.knn_membership(fake, real, r2, want_cols=False), a.reps)
    res['knn_membership_bit_identical'] = bool(torch.equal(rows, rows2) and torch.equal(cols, cols2))
    res['status'] = int(status.item())
    for name in ('knn_radii', 'knn_membership'):
        res[name + '_floor_over_time'] = res['floor_ms_per_call'] / res[name]['median_ms']
        res[name + '_counted_tflops'] = flop / 1e12 / (res[name]['median_ms'] * 1e-3)
    fd = metrics.FeatureDistance(nearest_k=a.k).add_features(fake, real)
    res['prdc_total'] = timed(lambda: fd.prdc(), a.reps)                 # two radii and two membership calls
    res['prdc'] = {key: float(v) for key, v in fd.prdc().items()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
