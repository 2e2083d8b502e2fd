"""-m gpu: the packed, device-resident dataset.  ``him_data_nearest_rle`` at the C ABI between guard bands against
``device.resize_maps`` (the PNG loader's gather, itself tested against Pillow) on the decoded windows; whole batches of
the packed loader against the PNG loader's for the same files and seeds, key by key; one trainer step from each."""
import json
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import abi_harness as ah
import data_fixture as fx
from util import load_golden

pytestmark = pytest.mark.gpu

SRC_H, SRC_W = 37, 53
# (x0, y0, w, h) inside the 53 x 37 source: 19 x 23 scaled down, origin inside a run; 8 x 8 scaled up, reaching the last
# column; the whole image
WINDOWS = [(7, 5, 19, 23), (SRC_W - 8, 11, 8, 8), (0, 0, SRC_W, SRC_H)]
IMAGE_OF = [0, 1, 0]                                         # two images in the store: sample 1 reads the second
OUT_KINDS = {'float': 0, 'unit': 1, 'uint8': 2, 'int32': 3}
CHECKER_ROW, SINGLE_ROWS = 12, (15, 21)                      # rows every output size of the kernel test reads (_case asserts it)
_REF = {}


def _source(dtype, seed):
    """Runs of 5 columns (so x0 = 7 starts inside one), the last column a run of its own, row 12 a 1-pixel checkerboard
    (53 runs: the search at full depth, no neighbour shares a run), rows 15 and 21 a single run each.  The three rows
    lie inside the windows, so the mid-run origin, the last column and the flipped tables cross them."""
    rng = np.random.RandomState(seed)
    hi = 250 if dtype == np.uint8 else (40000 if dtype == np.uint16 else 100000)
    a = np.repeat(rng.randint(1, hi, (SRC_H, SRC_W // 5 + 1)), 5, axis=1)[:, :SRC_W]
    a[:, -1] = rng.randint(1, hi, SRC_H)
    a[CHECKER_ROW] = 1 + (np.arange(SRC_W) % 2) * (hi - 2)
    a[SINGLE_ROWS[0]] = hi - 3
    a[SINGLE_ROWS[1]] = 2
    if dtype == np.int32:
        a[24:28, 10:30] = -7                                 # mode 'I' files may hold negative values
    return a.astype(dtype)


def _layout(arrays):
    """The arrays back to back, each 16-byte aligned: (bytes, offsets)."""
    at, size = [], 0
    for a in arrays:
        size += (-size) % 16
        at.append(size)
        size += a.nbytes
    buf = np.zeros(size + (-size) % 16, np.uint8)
    for o, a in zip(at, arrays):
        buf[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return buf, at


def _case(dtype, flips, H, W):
    """Store bytes, table bytes and their offsets, and the expected (B,1,H,W) per output kind (computed once)."""
    from neurips18_hierchical_image_manipulation_amd.data import device as dv
    from neurips18_hierchical_image_manipulation_amd.data import resample
    from neurips18_hierchical_image_manipulation_amd.preprocess_pack import rle_rows
    key = (np.dtype(dtype).name, tuple(flips), H, W)
    if key in _REF:
        return _REF[key]
    images = [_source(dtype, 1), _source(dtype, 2)]
    runs = [rle_rows(a) for a in images]
    store, at = _layout([v for r in runs for v in (r.row_start, r.run_x, r.run_v)])
    sixteen = dtype == np.uint16                              # mode I;16: Pillow's generic-transform table
    B = len(WINDOWS)
    xt, yt = np.empty((B, W), np.int32), np.empty((B, H), np.int32)
    for b, (x0, y0, w, h) in enumerate(WINDOWS):
        x = resample.nearest_table(w, W, sixteen)
        xt[b] = x[::-1] if flips[b] else x
        yt[b] = resample.nearest_table(h, H, sixteen)
        assert CHECKER_ROW in y0 + yt[b], (b, H, 'no output reads the checkerboard row')
    read = set(np.concatenate([w[1] + yt[b] for b, w in enumerate(WINDOWS)]).tolist())
    assert set(SINGLE_ROWS) <= read, (H, 'no output reads the single-run rows')
    per_row = [np.diff(r.row_start) for r in runs]
    assert all(n[CHECKER_ROW] == SRC_W and n[SINGLE_ROWS[0]] == n[SINGLE_ROWS[1]] == 1 for n in per_row)
    if sixteen and (H, W) == (13, 15):                        # here mode I;16's table is another one than the 8-bit table:
        w1 = WINDOWS[1][2]                                    # with the checkerboard row every column shows it
        assert not np.array_equal(resample.nearest_table(w1, W, True), resample.nearest_table(w1, W, False))
    offs = np.array([at[3 * i:3 * i + 3] for i in IMAGE_OF], np.int64)
    origin = np.array([w[:2] for w in WINDOWS], np.int32)
    tabs, tat = _layout([offs[:, 0], offs[:, 1], offs[:, 2], origin[:, 0], origin[:, 1], xt, yt])
    windows = [np.ascontiguousarray(images[i][y0:y0 + h, x0:x0 + w]) for i, (x0, y0, w, h) in zip(IMAGE_OF, WINDOWS)]
    want = {out: dv.resize_maps(windows, H, W, list(flips), out).cpu() for out in OUT_KINDS}
    _REF[key] = (store, tabs, tat, want, runs, at)
    return _REF[key]


def _arena(store, tabs, dst_bytes):
    ar = ah.Arena('cuda', {'store': ('ws', len(store)), 'tabs': ('ws', len(tabs)), 'dst': ('ws', dst_bytes)})
    ar.t['store'].copy_(torch.from_numpy(store))
    ar.t['tabs'].copy_(torch.from_numpy(tabs))
    return ar


def _call(lib, ar, tat, **over):
    """The call on the arena's store and tables; ``over`` gives dst, dst_kind, B, H, W and replaces any other argument."""
    a = dict(base=ar.ptr('store'))
    a.update({n: ar.ptr('tabs') + o for n, o in zip(('row_off', 'runx_off', 'runv_off', 'x0', 'y0', 'xtab', 'ytab'), tat)})
    a.update(over)
    rc = lib.him_data_nearest_rle(a['base'], a['row_off'], a['runx_off'], a['runv_off'], a['x0'], a['y0'], a['xtab'],
                                  a['ytab'], a['dst'], a['dst_kind'], a['B'], a['H'], a['W'],
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('flips', [(False, False, False), (True, False, True)], ids=['noflip', 'flip'])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.int32], ids=['u8', 'u16', 'i32'])
def test_kernel_equals_the_raw_gather(dtype, flips):
    """3 source kinds x 4 output kinds; 16 x 16 outputs (whole vector stores), the same shifted by one element (element
    stores on a misaligned destination) and 13 x 15 outputs (a ragged last group)."""
    lib = ah.raw_lib()
    B = len(WINDOWS)
    for H, W, shift in ((16, 16, 0), (16, 16, 1), (13, 15, 0)):
        store, tabs, tat, want, _, _ = _case(dtype, flips, H, W)
        for out, kind in OUT_KINDS.items():
            tdtype = want[out].dtype
            n = B * H * W * tdtype.itemsize
            ar = _arena(store, tabs, n + 16)
            rc = _call(lib, ar, tat, dst=ar.ptr('dst') + shift * tdtype.itemsize, dst_kind=kind, B=B, H=H, W=W)
            assert rc == 0, (out, lib.him_last_error())
            assert not ar.guard_failures(), ar.guard_failures()
            raw = ar.t['dst'].cpu()
            got = raw[shift * tdtype.itemsize:shift * tdtype.itemsize + n].view(tdtype).view(B, 1, H, W)
            assert torch.equal(got, want[out]), (np.dtype(dtype).name, out, H, W, shift,
                                                 (got != want[out]).nonzero()[:4].tolist())
            rest = torch.cat([raw[:shift * tdtype.itemsize], raw[shift * tdtype.itemsize + n:]])
            assert bool((rest == ah.NAN_BYTE).all()), 'bytes of the buffer outside the destination were written'


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['u8', 'u16'])
def test_device_nearest_rle_runs_the_same_gather(dtype):
    """``data.device.nearest_rle`` (the tensor-level binding) on the kernel test's store and tables, every output kind."""
    from neurips18_hierchical_image_manipulation_amd.data import device as dv
    B, H, W = len(WINDOWS), 13, 15
    store, tabs, tat, want, _, _ = _case(dtype, (True, False, True), H, W)
    dev = torch.device('cuda')
    part = lambda i, n, t: torch.from_numpy(tabs[tat[i]:tat[i] + n * np.dtype(t).itemsize].view(t).copy()).to(dev)  # noqa: E731
    args = [torch.from_numpy(store).to(dev)] + [part(i, B, np.int64) for i in range(3)] + \
           [part(3, B, np.int32), part(4, B, np.int32), part(5, B * W, np.int32).view(B, W), part(6, B * H, np.int32).view(B, H)]
    for out in OUT_KINDS:
        dst = torch.empty((B, 1, H, W), dtype=want[out].dtype, device=dev)
        assert dv.nearest_rle(*args, dst, out=out) is dst
        assert torch.equal(dst.cpu(), want[out]), out
    with pytest.raises(ValueError, match='do not fit'):
        dv.nearest_rle(*args, torch.empty((B, 1, H, W + 1), device=dev))
    with pytest.raises(ValueError, match='contiguous'):
        dv.nearest_rle(*args, torch.empty((B, 1, H, W), dtype=torch.int32, device=dev))


def test_refused_calls_write_nothing_and_an_empty_row_reads_zero():
    lib = ah.raw_lib()
    B, H, W = len(WINDOWS), 16, 16
    store, tabs, tat, want, runs, at = _case(np.uint8, (False, False, False), H, W)
    ar = _arena(store, tabs, B * H * W * 4)
    for over in (dict(dst_kind=4), dict(dst_kind=-1), dict(B=0), dict(H=-2), dict(W=0), dict(xtab=0), dict(base=0),
                 dict(dst=0), dict(y0=0)):
        good = dict(dst=ar.ptr('dst'), dst_kind=0, B=B, H=H, W=W)
        assert _call(lib, ar, tat, **dict(good, **over)) == ah.E_INVALID, over
        assert b'data_nearest_rle' in lib.him_last_error()
    assert not ar.guard_failures() and bool((ar.t['dst'] == ah.NAN_BYTE).all())
    # rows 5..36 of the first image lose their runs (row_start repeats): samples 0 and 2 read zeros there, sample 1
    # (the second image) is untouched
    broken = store.copy()
    rs = broken[at[0]:at[0] + 4 * (SRC_H + 1)].view(np.int32)
    rs[6:] = rs[5]
    ar = _arena(broken, tabs, B * H * W * 4)
    assert _call(lib, ar, tat, dst=ar.ptr('dst'), dst_kind=0, B=B, H=H, W=W) == 0 and not ar.guard_failures()
    got = ar.t['dst'].cpu().view(torch.float32).view(B, 1, H, W)
    assert torch.equal(got[1], want['float'][1]) and float(got[0].abs().sum()) == 0
    ytab = tabs[tat[6]:tat[6] + 4 * B * H].view(np.int32).reshape(B, H)
    zero = torch.from_numpy(ytab[2] >= 5)
    assert torch.equal(got[2, 0][~zero], want['float'][2, 0][~zero]) and float(got[2, 0][zero].abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------------
def _opt(root, name, fine, extra=(), packed=None, load_image=True):
    from neurips18_hierchical_image_manipulation_amd.options import MaskToImageTrainOptions
    opt = MaskToImageTrainOptions().parse(save=False, default_args=fx.loader_argv(root, name, fine, extra))
    opt.load_image = load_image
    if packed:
        opt.packed_dataroot = packed
    return opt


def _inst16(root):
    """The ADE fixture with its instance maps rewritten as 16-bit files (ids above 255)."""
    folder = os.path.join(root, 'train_inst')
    for fn in sorted(os.listdir(folder)):
        a = np.asarray(Image.open(os.path.join(folder, fn))).astype(np.uint16)
        Image.fromarray(np.where(a > 0, a + 300, 0).astype(np.uint16)).save(os.path.join(folder, fn))


FINE = 64                                                    # the smallest fineSize of tests/test_data_gpu.py
CITY = ['--contextMargin', '3.0', '--min_box_size', '16', '--max_box_size', '96', '--prob_bg', '0.3']
ADE = ['--contextMargin', '2.0', '--min_box_size', '16', '--max_box_size', '64', '--prob_bg', '0.5']
BATCH_CASES = {
    'city_region': ('city', CITY, None),
    'ade_region': ('ade', ADE, None),
    'ade_region_inst16': ('ade', ADE, _inst16),
    'city_scale_width': ('city', ['--resize_or_crop', 'scale_width', '--loadSize', '128', '--min_box_size', '16',
                                  '--max_box_size', '96'], None),
    'city_none_bs1': ('city', ['--resize_or_crop', 'none', '--batchSize', '1', '--min_box_size', '16',
                               '--max_box_size', '96'], None),
}


def _batches(opt, seed):
    from neurips18_hierchical_image_manipulation_amd.data.data_loader import CreateDataLoader
    random.seed(seed)
    np.random.seed(seed)
    loader = CreateDataLoader(opt)
    out = [b for b in loader.load_data()]
    torch.cuda.synchronize()
    return loader, out


def _assert_equal_batches(png, packed):
    assert len(png) == len(packed) > 0
    for a, b in zip(png, packed):
        assert set(a) == set(b), set(a) ^ set(b)
        for k, v in a.items():
            if torch.is_tensor(v):
                assert v.dtype == b[k].dtype and v.shape == b[k].shape and b[k].is_cuda, k
                assert torch.equal(v, b[k]), (k, int((v != b[k]).sum()))
            else:
                assert v == b[k], k


def _compare(tmp_path, case, with_images, force_raw=()):
    from neurips18_hierchical_image_manipulation_amd import preprocess_pack as pk
    from neurips18_hierchical_image_manipulation_amd.data import packed_dataset as pd
    name, extra, rewrite = BATCH_CASES[case]
    root = str(tmp_path / name)
    fx.write_dataset(root, name)
    if rewrite:
        rewrite(root)
    pk.pack_split(root, 'train', with_images=with_images, force_raw=force_raw)
    for seed in (11, 12):                                     # 2 x 2 batches of 2 (4 of 1): flips and background boxes occur
        _, png = _batches(_opt(root, name, FINE, extra, load_image=with_images), seed)
        loader, packed = _batches(_opt(root, name, FINE, extra, packed=root, load_image=with_images), seed)
        assert isinstance(loader.dataset, pd.PackedSegmentationDataset)
        assert loader.host_loader.num_workers == 0
        _assert_equal_batches(png, packed)
        assert ('image' in png[0]) == with_images
    return png, loader


@pytest.mark.parametrize('with_images', [True, False], ids=['photos', 'maps_only'])
@pytest.mark.parametrize('case', sorted(BATCH_CASES))
def test_packed_batches_equal_the_png_loaders(case, with_images, tmp_path):
    png, loader = _compare(tmp_path, case, with_images)
    store = loader.dataset.store
    assert store.raw == {'label': False, 'inst': False} and len(store._dev) == 1      # run lists, uploaded once
    if case == 'ade_region_inst16':
        assert png[0]['inst'].dtype == torch.int32             # 16-bit files: the int32 * 255 path
    if case == 'ade_region':
        assert png[0]['inst'].dtype == torch.float32
    if case == 'city_region':
        assert png[0]['inst'].dtype == torch.int32 and png[0]['label'].shape == (2, 1, FINE, FINE)
    if case == 'city_none_bs1':
        assert png[0]['label'].shape == (1, 1, 256, 512)


def test_packed_batches_with_the_label_maps_stored_raw(tmp_path):
    _, loader = _compare(tmp_path, 'city_region', True, force_raw=('label',))
    assert loader.dataset.store.raw == {'label': True, 'inst': False}


def test_workers_are_not_started_and_a_pack_too_large_is_refused(tmp_path, monkeypatch):
    from neurips18_hierchical_image_manipulation_amd import preprocess_pack as pk
    from neurips18_hierchical_image_manipulation_amd.data import packed_dataset as pd
    from neurips18_hierchical_image_manipulation_amd.data.data_loader import CreateDataLoader
    root = str(tmp_path / 'city')
    fx.write_dataset(root, 'city')
    pk.pack_split(root, 'train')
    loader = CreateDataLoader(_opt(root, 'city', FINE, CITY + ['--nThreads', '4'], packed=root))
    assert loader.host_loader.num_workers == 0
    monkeypatch.setattr(pd, 'MAX_FREE_SHARE', 1e-9)
    with pytest.raises(RuntimeError, match='PNG loader'):
        next(iter(loader.load_data()))


def test_a_trainer_step_from_either_loader_gives_the_same_losses(tmp_path):
    from neurips18_hierchical_image_manipulation_amd import preprocess_pack as pk
    from neurips18_hierchical_image_manipulation_amd import synth
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    flags = json.loads(str(load_golden('tiny_global')['flags']))
    root = str(tmp_path / 'city')
    fx.write_dataset(root, 'city')
    pk.pack_split(root, 'train')
    losses = []
    for packed in (None, root):
        _, batches = _batches(_opt(root, 'city', FINE, CITY, packed=packed), 21)
        model = create_model(dict(flags, gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp_path / 'ck'), name='t'))
        model.netG.load_state_dict(synth.init_state_dict(model.netG.state_dict(), 1))
        model.netD.load_state_dict(synth.init_state_dict(model.netD.state_dict(), 2))
        got = model.optimize_parameters(batches[0])
        losses.append({k: float(v) for k, v in got.items()})
    assert losses[0] and all(np.isfinite(v) for v in losses[0].values())
    assert losses[0] == losses[1]
