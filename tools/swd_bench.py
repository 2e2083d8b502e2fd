"""Times the calls of the sliced Wasserstein distance one by one between HIP events at the C2 evaluation size (500 images
of 3 x 256 x 512, 128 patches per image and level, 512 directions: 64000 descriptors per set and level), times
torch.sort on the same projected matrix, and computes the HBM floor of reading and writing the keys once per pass of a
four-pass (8-bit digit) radix sort.  Writes profiles/swd_bench.json.  Needs the MI355X; nothing is promised in advance."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neurips18_hierchical_image_manipulation_amd import ops  # noqa: E402
from neurips18_hierchical_image_manipulation_amd.util import metrics  # noqa: E402

HBM_BYTES_PER_S = 8.0e12          # MI355X peak


def timed(fn, reps, setup=None):
    """Milliseconds per call, each call alone between two events; ``setup`` runs untimed before every call."""
    for _ in range(2):
        if setup:
            setup()
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        if setup:
            setup()
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
    ap.add_argument('--images', type=int, default=500)
    ap.add_argument('--batch', type=int, default=20)
    ap.add_argument('--patches', type=int, default=128)
    ap.add_argument('--dirs', type=int, default=512)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'swd_bench.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'swd_bench needs the GPU'
    dev = torch.device('cuda:0')
    C, H, W = 3, 256, 512
    N = a.images * a.patches
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand((a.batch, C, H, W), generator=g, device=dev) * 2 - 1
    res = dict(device=torch.cuda.get_device_name(0), images=a.images, batch=a.batch, C=C, H=H, W=W, n_patches=a.patches,
               n_dirs=a.dirs, descriptors_per_set=N)
    res['lap_pyramid_batch'] = timed(lambda: ops.lap_pyramid(x), a.reps)
    laps = ops.lap_pyramid(x)
    res['levels'] = len(laps)
    pos = metrics.swd_positions(0, 0, a.batch, a.patches, H, W, device=dev)
    desc = torch.empty((N, 49 * C), device=dev)
    stats, status = ops.swd_stats(C, dev), torch.zeros(1, dtype=torch.int32, device=dev)
    res['swd_gather_batch_level0'] = timed(lambda: ops.swd_gather(laps[0], pos, desc, 0, stats, status), a.reps)
    desc.copy_(torch.randn(desc.shape, generator=g, device=dev))
    d = desc.double().reshape(N, C, 49)
    stats = torch.stack([d.sum((0, 2)), (d * d).sum((0, 2)), d.amin((0, 2)), d.amax((0, 2))], 1).contiguous()
    del d
    dirs = metrics.swd_tables(0, C, a.dirs, dev)
    res['swd_project'] = timed(lambda: ops.swd_project(desc, stats, dirs), a.reps)
    proj, _ = ops.swd_project(desc, stats, dirs)
    keys = proj.clone()
    res['sort_segments'] = timed(lambda: ops.sort_segments(keys), a.reps, setup=lambda: keys.copy_(proj))
    res['torch_sort'] = timed(lambda: torch.sort(proj, dim=1), a.reps)
    keys.copy_(proj)
    ops.sort_segments(keys)
    res['sort_equals_torch_sort'] = bool(torch.equal(keys, torch.sort(proj, dim=1)[0]))
    other = torch.sort(proj * 1.1 + 0.05, dim=1)[0].contiguous()
    dsum = torch.empty(a.dirs, dtype=torch.float64, device=dev)
    mean = torch.empty((), dtype=torch.float64, device=dev)
    from neurips18_hierchical_image_manipulation_amd._cabi import lib
    st = torch.cuda.current_stream().cuda_stream
    res['swd_distance'] = timed(lambda: lib.him_swd_distance(keys.data_ptr(), N, other.data_ptr(), N, a.dirs, dsum.data_ptr(),
                                                             mean.data_ptr(), st), a.reps)
    nbytes = a.dirs * N * 4
    res['sort_keys_bytes'] = nbytes
    res['radix_hbm_floor_ms'] = 4 * 2 * nbytes / HBM_BYTES_PER_S * 1e3
    res['sort_over_torch_sort'] = res['sort_segments']['median_ms'] / res['torch_sort']['median_ms']
    res['sort_over_floor'] = res['sort_segments']['median_ms'] / res['radix_hbm_floor_ms']
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
