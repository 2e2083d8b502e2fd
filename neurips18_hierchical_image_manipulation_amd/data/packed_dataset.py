"""The segmentation datasets fed from a pack that lives in GPU memory (``preprocess_pack.py`` writes it).

``PackedStore`` uploads the photographs and the label / instance maps of a split once; after that the host stage of a
sample is the reference's random draws and a few integers (an image id and window boxes): no file is opened, nothing is
decoded and no image crosses to the device per batch.  ``PackedSegmentationDataset.assemble`` gathers the windows
straight out of the resident store: maps kept as run lists through ``him_data_nearest_rle``, maps kept raw and the
photographs through the kernels of the PNG loader with ``offs`` / ``pitch`` pointing into the store.  The batch
dictionary equals the PNG loader's for the same seeds.

Selected by ``opt.packed_dataroot = <pack file, or the folder that holds <phase>.himpack>`` (an attribute, like
``compact_labels``; there is no parser flag).  The host stage then runs in the trainer's process: no worker processes
start and ``--nThreads`` is ignored.  Under ``dist.py`` every rank holds its own copy of the store.
"""
import json
import os

import numpy as np
import torch

from .. import preprocess_pack as pk
from .._cabi import lib
from . import device as dv
from . import resample
from .base_dataset import get_soft_bbox, get_transform_params
from .segmentation_dataset import CLASSES, DATASETS, SegmentationDataset

# The store may take at most this share of the memory that is free when it is uploaded: the rest is the trainer's
# (weights, activations, workspaces are allocated after the loader is created).  A pack above it is refused; the
# fallback is the PNG loader, there is no partial residency.
MAX_FREE_SHARE = 0.5
BOUNCE_BYTES = 64 << 20        # pinned bounce buffer of the one-time upload; the file itself is never pinned


class PackedStore(object):
    """A pack's index on the host and, from the first ``base()`` on, its data region in device memory."""

    def __init__(self, path):
        self.path = path
        self.header, self.index = pk.read_index(path)
        self.raw = self.header['raw']
        self.with_images = self.header['with_images']
        self.info = [json.loads(e['bbox']) for e in self.index]       # parsed once; the samplers only read it
        self.data_bytes = self.header['data'][1]
        self._dev = {}

    def __len__(self):
        return len(self.index)

    def base(self, dev):
        """Device address of the data region (uploaded on first use)."""
        buf = self._dev.get(dev)
        if buf is None:
            buf = self._dev[dev] = self._upload(dev)
        return buf.data_ptr()

    def _upload(self, dev):
        free, _ = torch.cuda.mem_get_info(dev)
        if self.data_bytes > MAX_FREE_SHARE * free:
            raise RuntimeError('the pack %s needs %d bytes of device memory, more than %d%% of the %d bytes free: use '
                               'the PNG loader (leave opt.packed_dataroot unset)'
                               % (self.path, self.data_bytes, int(MAX_FREE_SHARE * 100), free))
        buf = torch.empty(max(self.data_bytes, 16), dtype=torch.uint8, device=dev)
        chunk = min(BOUNCE_BYTES, max(self.data_bytes, 16))
        bounce = [torch.empty(chunk, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        ready = [None, None]
        stream = torch.cuda.current_stream(dev)
        with open(self.path, 'rb') as f:
            f.seek(self.header['data'][0])
            at, i = 0, 0
            while at < self.data_bytes:
                n = min(chunk, self.data_bytes - at)
                if ready[i] is not None:
                    ready[i].synchronize()                            # the copy that last read this buffer is done
                got = f.readinto(memoryview(bounce[i].numpy())[:n])
                if got != n:
                    raise IOError('%s ends inside its data region' % self.path)
                buf[at:at + n].copy_(bounce[i][:n], non_blocking=True)
                ready[i] = torch.cuda.Event()
                ready[i].record(stream)
                at, i = at + n, i ^ 1
        stream.synchronize()
        return buf


class _Windows(object):
    """What the resident plans share: the store, the image id and the (x0, y0, x1, y1) box of every sample."""

    def init_windows(self, store, ids, boxes):
        self.store, self.ids, self.boxes = store, ids, boxes

    def shape(self, b):
        x0, y0, x1, y1 = self.boxes[b]
        return y1 - y0, x1 - x0

    def source(self, base):
        return self.store.base(dv.device())


class ResidentMapPlan(_Windows, dv.MapPlan):
    """MapPlan over windows of a map type the pack stores raw: only offsets and pitches are staged."""

    def __init__(self, store, map_type, ids, boxes, H, W, flips):
        # not MapPlan.__init__: that one types the batch from the pixel arrays it is given (and converts them where
        # they differ); here the index says what the files held
        self.init_windows(store, ids, boxes)
        self.map_type, self.H, self.W, self.flips = map_type, H, W, flips
        kinds = {store.index[i][map_type + '_kind'] for i in ids}
        if len(kinds) != 1:           # the writer stores a type of several bit depths as run lists
            raise ValueError('raw %s maps of several bit depths in one pack: use the PNG loader' % map_type)
        self.kind = kinds.pop()
        self.dtype = np.dtype(pk.KIND_DTYPES[self.kind])
        self.sixteen = [self.kind == 1] * len(ids)

    def place(self, st, b):
        e = self.store.index[self.ids[b]]
        x0, y0 = self.boxes[b][:2]
        return e[self.map_type][0] + (y0 * e['w'] + x0) * self.dtype.itemsize, e['w']


class MapPlanRLE(_Windows, dv.MapPlan):
    """MapPlan over windows of a map type the pack stores as run lists (``him_data_nearest_rle``)."""

    def __init__(self, store, map_type, ids, boxes, H, W, flips):
        self.init_windows(store, ids, boxes)
        self.map_type, self.H, self.W, self.flips = map_type, H, W, flips
        kinds = [store.index[i][map_type + '_kind'] for i in ids]
        self.sixteen = [k == 1 for k in kinds]                        # mode I;16 resizes by Pillow's other table
        # as MapPlan types a batch: the files' common type, int32 when they differ
        self.dtype = np.dtype(pk.KIND_DTYPES[kinds[0] if len(set(kinds)) == 1 else 2])

    def stage(self, st):
        B = len(self.ids)
        xt, yt = self.tables(B)
        offs = np.array([self.store.index[i][self.map_type][:3] for i in self.ids], np.int64)
        origin = np.array([box[:2] for box in self.boxes], np.int32)
        self.at = tuple(st.add(a) for a in (offs[:, 0], offs[:, 1], offs[:, 2], origin[:, 0], origin[:, 1], xt, yt))

    def run(self, base, dst, dst_kind, stream):
        lib.him_data_nearest_rle(self.source(base), *[base + a for a in self.at], dst.data_ptr(), dst_kind,
                                 len(self.ids), self.H, self.W, stream)


class ResidentPhotoPlan(_Windows, dv.PhotoPlan):
    """PhotoPlan over windows of the resident photographs."""

    def __init__(self, store, ids, boxes, H, W, flips, normalize):
        dv.PhotoPlan.__init__(self, None, H, W, flips, normalize)     # no host windows: shape / place / source answer
        self.init_windows(store, ids, boxes)

    def place(self, st, b):
        e = self.store.index[self.ids[b]]
        x0, y0 = self.boxes[b][:2]
        return e['photo'] + (y0 * e['w'] + x0) * 3, e['w']


class _Size(object):
    """The one attribute of a PIL image ``ImageTransform.window_and_size`` reads."""

    def __init__(self, size):
        self.size = size


def pack_path(opt):
    where = opt.packed_dataroot
    return os.path.join(where, opt.phase + '.himpack') if os.path.isdir(where) else where


class PackedSegmentationDataset(SegmentationDataset):
    def initialize(self, opt):
        self._configure(opt)
        if getattr(opt, 'load_raw', False):
            raise ValueError('load_raw returns the files as PIL decodes them: use the PNG loader (leave '
                             'opt.packed_dataroot unset)')
        self.load_raw = False
        self.store = PackedStore(pack_path(opt))
        if self.load_image and not self.store.with_images:
            raise ValueError('%s was packed with --with_images 0 but the options ask for photographs'
                             % self.store.path)
        index = self.store.index
        self.A_paths = [e['label_path'] for e in index]
        self.inst_paths = [e['inst_path'] for e in index]
        if self.store.with_images:
            self.B_paths = [e['image_path'] for e in index]
        self.dataset_size = len(index)

    def name(self):
        return 'PackedSegmentationDataset'

    def get_raw_inputs(self, index):
        raise ValueError('a packed dataset holds no PIL images: use the PNG loader (leave opt.packed_dataroot unset)')

    def _inside(self, box, e):
        assert 0 <= box[0] < box[2] <= e['w'] and 0 <= box[1] < box[3] <= e['h'], \
            'window %s leaves the %dx%d image: the reference\'s samplers clamp it' % (box, e['w'], e['h'])
        return tuple(int(v) for v in box)

    def host_record(self, index):
        """The PNG loader's host stage without the files: the same calls and random draws in the same order; windows
        as (x0, y0, x1, y1) boxes into image ``index`` of the store."""
        e = self.store.index[index]
        full = _Size((e['w'], e['h']))
        params = get_transform_params(full.size, self.store.info[index], self.class_of_interest, self.config,
                                      random_crop=self.opt.random_crop)
        ctx = dv.ImageTransform(self.opt, params, 0, False, True, True)
        rec = {'params': params, 'flip': ctx.flipped(), 'label_path': e['label_path'], 'inst_path': e['inst_path'],
               'image_id': index}
        box, rec['size'] = ctx.window_and_size(full)
        box = self._inside(box if box is not None else (0, 0, e['w'], e['h']), e)
        rec['label'] = rec['inst'] = box
        if self.load_image:
            rec['image'] = box
            rec['image_path'] = e['image_path']
        if self.config['preprocess_option'] == 'select_region':
            rec['label_obj'] = self._inside(resample.pil_crop_box(params['crop_object_pos']), e)
            size = rec['size'][0]
            ratio = np.random.uniform(low=self.config['min_ctx_ratio'], high=self.config['max_ctx_ratio'])
            rec['input_bbox'] = np.array(params['bbox_in_context'])
            rec['output_bbox'] = np.array(get_soft_bbox(rec['input_bbox'], size, size, ratio))
            cls = params['bbox_cls']
            rec['cls'] = cls if cls is not None else self.opt.label_nc - 1
        return rec

    def _map_plan(self, records, key, H, W, flips):
        map_type = 'inst' if key == 'inst' else 'label'               # 'label_obj' is a window of the label map
        plan = ResidentMapPlan if self.store.raw[map_type] else MapPlanRLE
        return plan(self.store, map_type, [r['image_id'] for r in records], [r[key] for r in records], H, W, flips)

    def _photo_plan(self, records, key, H, W, flips):
        return ResidentPhotoPlan(self.store, [r['image_id'] for r in records], [r[key] for r in records], H, W, flips,
                                 True)


def _packed_with_classes(loader):
    """The packed twin of ``DATASETS[loader]``: same classes of interest, same shown name."""
    def initialize(self, opt):
        PackedSegmentationDataset.initialize(self, opt)
        self.class_of_interest = list(CLASSES[loader])
    png = DATASETS[loader]
    return type('Packed' + png.__name__, (PackedSegmentationDataset,),
                {'initialize': initialize, 'name': png.name, '__doc__': 'packed twin of %s' % png.__name__})


PACKED_DATASETS = {loader: _packed_with_classes(loader) for loader in DATASETS}
