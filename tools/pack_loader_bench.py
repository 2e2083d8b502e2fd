"""PNG loader against the packed, device-resident loader on a synthetic Cityscapes-sized tree (2048x1024, written with
tests/data_fixture.py's generator into a temporary directory): batches/s of select_region at fineSize 256, batch 8, the
host time a batch costs the trainer's process, the run-list gather against the raw gather on the same windows between
HIP events, the one-time upload of the pack, and the pack's size with the maps raw and as run lists.

    python tools/pack_loader_bench.py [--images 96] [--png_images 1536] [--out profiles/pack_loader_bench.json]

Every loader is timed inside ONE pass over its split (a new pass starts the PNG loader's worker processes again, which
is no part of a steady state), and the rate is images / wall time after the warm-up; the median interval is kept beside
it.  The PNG loader keeps workers x prefetch (2) batches in flight, 32 at --nThreads 16, so its split is a tree of links
to the same files several times that long (--png_images / 8 batches); the pack is written from the first --images.

The synthetic PNGs decode faster than real Cityscapes / ADE20K files (flat regions, noise photographs): the PNG
loader's numbers are an upper bound for a real tree."""
import argparse
import json
import os
import random
import shutil
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import data_fixture as fx
from neurips18_hierchical_image_manipulation_amd import preprocess_pack as pk
from neurips18_hierchical_image_manipulation_amd.data import device as dv
from neurips18_hierchical_image_manipulation_amd.data import packed_dataset as pd
from neurips18_hierchical_image_manipulation_amd.data.data_loader import CreateDataLoader
from neurips18_hierchical_image_manipulation_amd.options import MaskToImageTrainOptions

FINE, BATCH, WARM, DISTINCT = 256, 8, 5, 8
STEP_IMAGES_PER_S = 160.0          # what the training step consumes per GPU (README, round 6)


FOLDERS = (('_label', 'png'), ('_inst', 'png'), ('_img', 'png'), ('_bbox', 'json'))


def write_tree(root, images):
    """DISTINCT generated 2048x1024 samples; the rest of the split are links to them (the loaders open every name)."""
    fx.SETS['city2k'] = dict(fx.SETS['city'], sizes=[(2048, 1024)] * DISTINCT)
    fx.write_dataset(root, 'city2k')
    for sub, ext in FOLDERS:
        for i in range(DISTINCT, images):
            os.symlink('sample_%02d.%s' % (i % DISTINCT, ext), os.path.join(root, 'train' + sub, 'sample_%02d.%s' % (i, ext)))


def link_tree(root, source, images):
    """A split of ``images`` names, every one a link to one of ``source``'s DISTINCT generated files."""
    for sub, ext in FOLDERS:
        os.makedirs(os.path.join(root, 'train' + sub))
        for i in range(images):
            os.symlink(os.path.join(source, 'train' + sub, 'sample_%02d.%s' % (i % DISTINCT, ext)),
                       os.path.join(root, 'train' + sub, 'sample_%04d.%s' % (i, ext)))


def options(root, threads, packed=None):
    argv = fx.loader_argv(root, 'city2k', FINE, ['--contextMargin', '3.0', '--batchSize', str(BATCH), '--nThreads',
                                                 str(threads)])
    argv.remove('--serial_batches')
    opt = MaskToImageTrainOptions().parse(save=False, default_args=argv)
    if packed:
        opt.packed_dataroot = packed
    return opt


def run_loader(opt, passes=1):
    """``passes`` over the split (one, wherever worker processes would start again): images / wall time after WARM
    batches (the rate a training run sees), the median batch interval (consumer: a device synchronise) and the host time per batch spent in this process inside the dataset's
    two stages (the PNG loader's host stage runs in the workers unless --nThreads is 0)."""
    random.seed(1)
    np.random.seed(1)
    loader = CreateDataLoader(opt)
    ds = loader.dataset
    spent = [0.0]

    def timed(fn):
        def call(*a):
            t = time.perf_counter()
            out = fn(*a)
            spent[0] += time.perf_counter() - t
            return out
        return call
    ds.assemble, ds.host_record = timed(ds.assemble), timed(ds.host_record)
    if isinstance(ds, pd.PackedSegmentationDataset):
        ds.store.base(dv.device())                            # the one-time upload is measured on its own
    stamps, host = [], []
    for _ in range(passes):
        for batch in loader.load_data():
            torch.cuda.synchronize()
            stamps.append(time.perf_counter())
            host.append(spent[0])
    assert len(stamps) >= 30 + WARM + 1, 'the split is too short for 30 timed batches'
    gaps = np.diff(stamps)[WARM:]
    host = np.diff(host)[WARM:]
    rate = BATCH * len(gaps) / (stamps[-1] - stamps[WARM])
    return {'batches': int(len(gaps)), 'images_per_s': rate, 'batches_per_s': rate / BATCH,
            'batch_ms_mean': float(np.mean(gaps)) * 1e3, 'batch_ms_median': float(np.median(gaps)) * 1e3,
            'batch_ms_p10_p90': [float(np.percentile(gaps, 10)) * 1e3, float(np.percentile(gaps, 90)) * 1e3],
            'batch_ms_max': float(gaps.max()) * 1e3, 'images_per_s_from_median': BATCH / float(np.median(gaps)),
            'host_ms_per_batch_in_trainer_process': float(np.median(host)) * 1e3,
            'reaches_step_rate': bool(rate >= STEP_IMAGES_PER_S)}


def time_gather(plan, kind, dtype, iters=200):
    """Microseconds per launch, ``iters`` launches back to back between two HIP events (tables staged once)."""
    dev = dv.device()
    dst = torch.empty((len(plan.ids), 1, FINE, FINE), dtype=dtype, device=dev)

    def body(base, stream):
        for _ in range(20):
            plan.run(base, dst, kind, stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            plan.run(base, dst, kind, stream)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3
    return dv.run_plans(dev, [plan], body), dst


def kernels(root, raw_pack):
    """him_data_nearest_rle on the run-list pack against him_data_nearest on the raw pack, same windows, same tables."""
    ds = CreateDataLoader(options(root, 0, packed=root)).dataset
    random.seed(2)
    np.random.seed(2)
    recs = [ds.host_record(i) for i in range(BATCH)]
    ids, flips = [r['image_id'] for r in recs], [r['flip'] for r in recs]
    raw = pd.PackedStore(raw_pack)
    out = {'windows': [list(r['label']) for r in recs]}
    for t, key in (('label', 'label'), ('inst', 'inst'), ('label', 'label_obj')):
        boxes = [r[key] for r in recs]
        rle = pd.MapPlanRLE(ds.store, t, ids, boxes, FINE, FINE, flips)
        ref = pd.ResidentMapPlan(raw, t, ids, boxes, FINE, FINE, flips)
        kind, dtype = dv._MAP_OUT['float' if rle.dtype == np.uint8 else 'int32']
        samples = {'rle': [], 'raw': []}
        for _ in range(3):                                    # alternate the two
            us, a = time_gather(rle, kind, dtype)
            samples['rle'].append(us)
            us, b = time_gather(ref, kind, dtype)
            samples['raw'].append(us)
        assert torch.equal(a, b), key
        out[key] = {'him_data_nearest_rle_us': float(np.median(samples['rle'])),
                    'him_data_nearest_us': float(np.median(samples['raw'])), 'samples_us': samples}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=96)
    ap.add_argument('--png_images', type=int, default=1536)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pack_loader_bench.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    tmp = tempfile.mkdtemp(prefix='pack_bench_')
    try:
        root = os.path.join(tmp, 'city2k')
        write_tree(root, args.images)
        png_root = os.path.join(tmp, 'city2k_links')
        link_tree(png_root, root, args.png_images)
        t = time.perf_counter()
        packed = pk.pack_split(root, 'train')
        pack_s = time.perf_counter() - t
        raw = pk.pack_split(root, 'train', out=os.path.join(tmp, 'raw.himpack'), force_raw=pk.MAP_TYPES)
        result = {'device': torch.cuda.get_device_name(0), 'images': args.images, 'png_images': args.png_images, 'distinct_images': DISTINCT,
                  'image_size': [2048, 1024], 'fineSize': FINE, 'batchSize': BATCH,
                  'step_images_per_s': STEP_IMAGES_PER_S, 'pack_write_s': pack_s,
                  'pack': {k: packed[k] for k in ('label', 'inst', 'file_bytes', 'data_bytes')},
                  'pack_bytes_maps_raw': raw['data_bytes'], 'pack_bytes_maps_run_lists': packed['data_bytes']}
        store = pd.PackedStore(packed['path'])
        torch.cuda.synchronize()
        t = time.perf_counter()
        store.base(dv.device())
        torch.cuda.synchronize()
        up = time.perf_counter() - t
        result['upload'] = {'seconds': up, 'bytes': store.data_bytes, 'GB_per_s': store.data_bytes / up / 1e9}
        del store
        result['packed_loader'] = run_loader(options(root, 0, packed=root), passes=4)   # in-process: a new pass starts nothing
        result['png_loader'] = {}
        for threads in (4, 8, 16):
            result['png_loader']['nThreads_%d' % threads] = run_loader(options(png_root, threads))
            print(threads, result['png_loader']['nThreads_%d' % threads], flush=True)
        result['kernels'] = kernels(root, raw['path'])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == '__main__':
    main()
