"""Pack one split of a segmentation dataset into a single file that ``data/packed_dataset.py`` keeps resident on the GPU.

    python -m neurips18_hierchical_image_manipulation_amd.preprocess_pack --dataroot D --phase train
                                                                          [--out FILE] [--with_images 0|1]

The ``<phase>_label``, ``<phase>_inst``, ``<phase>_bbox`` and (``--with_images 1``) ``<phase>_img`` folders are read
once, in the sorted order ``SegmentationDataset.initialize`` uses.  Photographs are stored as raw RGB bytes; the label
and the instance maps are piecewise constant and are stored as per-row run lists, which ``him_data_nearest_rle`` reads
directly.  A map type whose run lists would not be smaller than its raw bytes over the whole split is stored raw
instead (per pack and per type, never per image, so that a batch is uniform).  Layout: INTEGRATION.md "Packed dataset".
"""
import argparse
import collections
import json
import os
import shutil
import struct
import tempfile

import numpy as np
from PIL import Image

from .data import device as dv
from .data.image_folder import make_dataset

MAGIC = b'HIMPACK1'
VERSION = 1
# magic, version, images, with_images, label stored raw, inst stored raw, reserved; then 10 unsigned 64-bit words:
# index offset / bytes, data offset / bytes, and offset / bytes (relative to the data offset) of the photo, label and
# inst sections
HEADER = struct.Struct('<8s6I10Q')
HEADER_BYTES = 128
ALIGN = 16
MAP_TYPES = ('label', 'inst')
KIND_NAMES = ('uint8', 'uint16', 'int32')
KIND_DTYPES = (np.uint8, np.uint16, np.int32)

Runs = collections.namedtuple('Runs', 'row_start run_x run_v width dtype')


def rle_rows(a):
    """Per-row run lists of a 2-D integer map: ``row_start[H+1]`` (the runs of row r are ``[row_start[r],
    row_start[r+1])``), ``run_x[n]`` (first column of each run) and ``run_v[n]`` (its value), all int32.  A run starts
    wherever the value changes within a row, and every row starts one at column 0."""
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError('rle_rows takes a non-empty 2-D map, got shape %s' % (a.shape,))
    starts = np.ones(a.shape, np.bool_)
    starts[:, 1:] = a[:, 1:] != a[:, :-1]
    ys, xs = np.nonzero(starts)                               # row-major: rows ascending, columns ascending inside
    row_start = np.zeros(a.shape[0] + 1, np.int32)
    np.cumsum(starts.sum(axis=1), out=row_start[1:])
    return Runs(row_start, xs.astype(np.int32), a[ys, xs].astype(np.int32), a.shape[1], a.dtype)


def unrle_rows(runs):
    """The map ``rle_rows`` encoded, in its dtype."""
    row_start, run_x, run_v, width, dtype = runs
    ends = np.empty(len(run_x), np.int64)
    ends[:-1] = run_x[1:]
    ends[np.asarray(row_start[1:], np.int64) - 1] = width     # the last run of every row ends with the row
    return np.repeat(run_v, ends - run_x).reshape(len(row_start) - 1, width).astype(dtype)


def _pad(f):
    gap = (-f.tell()) % ALIGN
    if gap:
        f.write(b'\0' * gap)
    return f.tell()


def _put(f, array):
    at = _pad(f)
    f.write(np.ascontiguousarray(array).tobytes())
    return at


def pack_split(dataroot, phase='train', out=None, with_images=True, force_raw=()):
    """Write the pack of ``<dataroot>/<phase>_*`` to ``out`` (default ``<dataroot>/<phase>.himpack``) and return a
    summary: the path, the image count and, per map type, the raw and the run-list size and which was stored.
    ``force_raw``: map types stored raw whatever their sizes (tests, measurements)."""
    out = out or os.path.join(dataroot, phase + '.himpack')
    folder = lambda suffix: sorted(make_dataset(os.path.join(dataroot, phase + suffix)))
    paths = {'label': folder('_label'), 'inst': folder('_inst'), 'bbox': folder('_bbox')}
    if with_images:
        paths['image'] = folder('_img')
    n = len(paths['label'])
    if n == 0 or any(len(v) != n for v in paths.values()):
        raise ValueError('%s/%s_*: the folders must hold the same, non-zero number of files (%s)'
                         % (dataroot, phase, {k: len(v) for k, v in paths.items()}))
    for t in force_raw:
        if t not in MAP_TYPES:
            raise ValueError('force_raw: unknown map type %r' % (t,))
    where = os.path.dirname(os.path.abspath(out))
    entries = []
    tmp = {(t, form): tempfile.TemporaryFile(dir=where) for t in MAP_TYPES for form in ('rle', 'raw')}
    kinds = {t: set() for t in MAP_TYPES}
    try:
        with open(out, 'wb') as f:
            f.write(b'\0' * HEADER_BYTES)
            photo_at = f.tell()
            for i in range(n):
                e = {'label_path': paths['label'][i], 'inst_path': paths['inst'][i]}
                with open(paths['bbox'][i], 'r') as jf:
                    e['bbox'] = jf.read()
                for t in MAP_TYPES:
                    a = dv.map_bytes(Image.open(paths[t][i]))
                    if t == 'label':
                        e['h'], e['w'] = int(a.shape[0]), int(a.shape[1])
                    elif a.shape != (e['h'], e['w']):
                        raise ValueError('%s: %s, but its label map is %s' % (paths[t][i], a.shape, (e['h'], e['w'])))
                    e[t + '_kind'] = dv._KIND_OF_DTYPE[a.dtype]
                    kinds[t].add(e[t + '_kind'])
                    runs = rle_rows(a)
                    e[t + '_rle'] = [_put(tmp[t, 'rle'], runs.row_start), _put(tmp[t, 'rle'], runs.run_x),
                                     _put(tmp[t, 'rle'], runs.run_v), int(len(runs.run_x))]
                    e[t + '_raw'] = _put(tmp[t, 'raw'], a)
                if with_images:
                    e['image_path'] = paths['image'][i]
                    photo = np.asarray(Image.open(paths['image'][i]).convert('RGB'))
                    if photo.shape != (e['h'], e['w'], 3):
                        raise ValueError('%s: %s, but its label map is %s' % (paths['image'][i], photo.shape,
                                                                              (e['h'], e['w'])))
                    e['photo'] = _put(f, photo) - photo_at
                entries.append(e)
            sections = [(0, _pad(f) - photo_at)]
            summary = {'path': out, 'images': n, 'with_images': bool(with_images)}
            stored_raw = {}
            for t in MAP_TYPES:
                sizes = {form: _pad(tmp[t, form]) for form in ('rle', 'raw')}
                mixed = len(kinds[t]) > 1                     # run values are int32 whatever the file's mode was
                if t in force_raw and mixed:
                    raise ValueError('%s maps of several bit depths can only be stored as run lists' % t)
                stored_raw[t] = t in force_raw or (sizes['rle'] >= sizes['raw'] and not mixed)
                form = 'raw' if stored_raw[t] else 'rle'
                at = _pad(f)
                tmp[t, form].seek(0)
                shutil.copyfileobj(tmp[t, form], f, 1 << 24)
                sections.append((at - photo_at, f.tell() - at))
                summary[t] = {'raw_bytes': sizes['raw'], 'rle_bytes': sizes['rle'], 'stored': form}
                print('%s maps: raw %d bytes, run lists %d bytes -> stored %s'
                      % (t, sizes['raw'], sizes['rle'], 'raw' if stored_raw[t] else 'as run lists'))
                for e in entries:
                    rle, raw = e.pop(t + '_rle'), e.pop(t + '_raw')
                    e[t] = [raw + sections[-1][0]] if stored_raw[t] else [v + sections[-1][0] for v in rle[:3]] + rle[3:]
            data_bytes = _pad(f) - photo_at
            index = json.dumps(entries).encode('utf-8')
            index_at = f.tell()
            f.write(index)
            total = f.tell()
            f.seek(0)
            f.write(HEADER.pack(MAGIC, VERSION, n, int(bool(with_images)), int(stored_raw['label']),
                                int(stored_raw['inst']), 0, index_at, len(index), photo_at, data_bytes,
                                *[v for s in sections for v in s]))
    finally:
        for t in tmp.values():
            t.close()
    summary['file_bytes'] = total
    summary['data_bytes'] = data_bytes
    print('%s: %d images, %d bytes (%d resident)' % (out, n, total, data_bytes))
    return summary


def read_index(path):
    """(header dict, list of per-image entries) of a pack.  An entry holds ``h``, ``w``, ``label_kind`` / ``inst_kind``
    (0 uint8 / 1 uint16 / 2 int32, as ``data.device.map_bytes`` types the file), the path strings, ``bbox`` (the JSON
    text of the annotation file, verbatim), ``photo`` (byte offset in the data region) and per map type ``[row_start,
    run_x, run_v offsets, runs]`` or, for a type stored raw, ``[offset]``."""
    with open(path, 'rb') as f:
        head = f.read(HEADER_BYTES)
        if len(head) < HEADER_BYTES or head[:8] != MAGIC:
            raise ValueError('%s is not a dataset pack' % path)
        v = HEADER.unpack(head[:HEADER.size])
        if v[1] != VERSION:
            raise ValueError('%s: pack version %d, this reader knows %d' % (path, v[1], VERSION))
        header = {'images': v[2], 'with_images': bool(v[3]), 'raw': {'label': bool(v[4]), 'inst': bool(v[5])},
                  'index': (v[7], v[8]), 'data': (v[9], v[10]),
                  'sections': {'photo': (v[11], v[12]), 'label': (v[13], v[14]), 'inst': (v[15], v[16])}}
        f.seek(v[7])
        entries = json.loads(f.read(v[8]).decode('utf-8'))
    if len(entries) != header['images']:
        raise ValueError('%s: the index lists %d images, the header %d' % (path, len(entries), header['images']))
    return header, entries


def read_map(path, header, entry, map_type):
    """One map of a pack as the array ``map_bytes`` gave the writer (host side: tests and tools)."""
    dtype = KIND_DTYPES[entry[map_type + '_kind']]
    h, w = entry['h'], entry['w']
    with open(path, 'rb') as f:
        def load(at, count, dt):
            f.seek(header['data'][0] + at)
            return np.frombuffer(f.read(count * np.dtype(dt).itemsize), dt)
        where = entry[map_type]
        if header['raw'][map_type]:
            return load(where[0], h * w, dtype).reshape(h, w)
        return unrle_rows(Runs(load(where[0], h + 1, np.int32), load(where[1], where[3], np.int32),
                               load(where[2], where[3], np.int32), w, dtype))


def read_photo(path, header, entry):
    with open(path, 'rb') as f:
        f.seek(header['data'][0] + entry['photo'])
        return np.frombuffer(f.read(entry['h'] * entry['w'] * 3), np.uint8).reshape(entry['h'], entry['w'], 3)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--dataroot', required=True)
    ap.add_argument('--phase', default='train')
    ap.add_argument('--out', default=None, help='pack file (default <dataroot>/<phase>.himpack)')
    ap.add_argument('--with_images', type=int, choices=(0, 1), default=1, help='0: maps and boxes only (box2mask)')
    args = ap.parse_args(argv)
    pack_split(args.dataroot, args.phase, args.out, bool(args.with_images))


if __name__ == '__main__':
    main()
