"""ADE20K preprocessing: turn the bedroom scenes of a raw ADE20K download (``index_ade20k.mat``, ``images/...`` with the
``.jpg``, ``_seg.png`` and ``_atr.txt`` files) into the ``<phase>_img / _label / _inst / _bbox`` folders the loader reads
(upstream's ``preprocess_ade.py``), with the per-pixel work on the device: one ``ops.ade_decode`` call per image instead
of a full-plane compare per kept class and three per instance.

    python -m neurips18_hierchical_image_manipulation_amd.preprocess_ade --dataroot datasets/ade20k

The box files are byte-identical to upstream's and the label / instance PNGs decode to upstream's planes.  One stated
departure: an object name that ``index_ade20k.mat`` does not list raises ``ValueError`` (upstream carries the previous
object's id over, or dies on the first object).
"""
import argparse
import json
import os
from concurrent.futures import ThreadPoolExecutor
from shutil import copyfile

import numpy as np
from PIL import Image

DECODE_THREADS = 4      # PNG decoding leaves the interpreter lock; a fixed, small pool (never sized by the host's CPU count)
PREFETCH = 4            # images decoded ahead of the device pass
BEDROOM = 'images/training/b/bedroom'
BBOX_SUF, IMG_SUF = '_gtFine_instanceIds.json', '_leftImg8bit.png'
LABEL_SUF, INST_SUF = '_gtFine_labelIds.png', '_gtFine_instanceIds.png'

# the 48 object classes upstream keeps ("top 50 most occurring"), as 1-based positions in the index file's objectnames
SORTED_50 = [2978, 165, 976, 2684, 1395, 447, 1735, 3055, 1869, 687, 689, 774, 471, 350, 491, 1564, 2178, 236, 2932, 530,
             57, 2985, 1910, 978, 2243, 1451, 2982, 266, 894, 2730, 2329, 2733, 1981, 2676, 212, 1702, 724, 2473, 146, 571,
             1930, 206, 2046, 2850, 249, 2586, 943, 480]


def _atr_objects(path):
    """``[(instance number, name)]`` of the part-level-0 lines of an ``_atr.txt`` file, in file order."""
    out = []
    with open(path, 'r') as f:
        for line in f:
            c = line.split('# ')
            if int(c[1]) == 0:
                out.append((int(c[0]), c[3].strip()))
    return out


def parse_atr(path):
    """The object class names of an ``_atr.txt`` file: fields separated by ``'# '``, field 1 the part level, field 3 the
    name; the names of the lines with part level 0, in file order.  Instance rank ``r >= 1`` bears name ``r - 1``."""
    return [name for _, name in _atr_objects(path)]


def load_index(path):
    """``(filenames, folders, objectnames)`` of an ``index_ade20k.mat`` as plain lists of ``str``."""
    try:
        import scipy.io
    except ImportError as e:
        raise ImportError('preprocess_ade.load_index needs SciPy (scipy.io.loadmat) to read %s: %s' % (path, e))
    index = scipy.io.loadmat(path)['index'][0, 0]
    return tuple([str(cell[0]) for cell in index[k][0]] for k in (0, 1, 6))


def _read_seg(path):
    """A ``_seg.png`` as contiguous (H, W, 3 or 4) bytes."""
    with Image.open(path) as im:
        a = np.array(im)
    if a.ndim != 3 or a.shape[2] not in (3, 4) or a.dtype != np.uint8:
        raise ValueError('%s: an 8-bit RGB(A) picture is expected, got shape %s %s' % (path, a.shape, a.dtype))
    return np.ascontiguousarray(a)


def _read_pair(file):
    return _read_seg(file.replace('.jpg', '_seg.png')), parse_atr(file.replace('.jpg', '_atr.txt'))


def _device(device):
    import torch
    return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def loadAde20K(file, device=None):
    """``(ObjectClassMasks, ObjectInstanceMasks, objects)`` of ``<file>.jpg``'s ``_seg.png`` and ``_atr.txt``, as
    upstream names them: the raw classes ``(R // 10) * 256 + G`` (uint16) and the instance ranks (uint8), both (H, W)
    planes on the device, and the dict of the part-level-0 lines (upstream fills every list but ``instancendx`` with the
    names; so does this)."""
    import torch
    from . import ops
    seg = _read_seg(file.replace('.jpg', '_seg.png'))
    lines = _atr_objects(file.replace('.jpg', '_atr.txt'))
    _, inst, _, cls = ops.ade_decode(torch.from_numpy(seg).to(_device(device)), SORTED_50, want_cls=True)
    instancendx, names = [n for n, _ in lines], [name for _, name in lines]
    objects = {'instancendx': instancendx, 'class': list(names), 'corrected_raw_name': list(names), 'iscrop': list(names),
               'listattributes': list(names)}
    return cls, inst, objects


def rows_to_info(H, W, rows, names, objectnames, keep=SORTED_50, image=None):
    """The dict upstream dumps, from ``ops.ade_decode``'s rows.  Rank 0 (the lowest B value, zero or not) is no object;
    rank ``r`` bears ``names[r - 1]``, whose 1-based position in ``objectnames`` (a list, or a ready name -> position
    dict) must be in ``keep`` for the object to be written, ``cls`` its 1-based position there.  The box is the 1-based
    inclusive extremes widened by ``max(extent // 100, 1)`` per axis and clamped to ``[1, W] x [1, H]``.  A name that
    ``objectnames`` does not hold raises ``ValueError`` naming ``image``."""
    ids = objectnames if isinstance(objectnames, dict) else _name_ids(objectnames)
    where = {int(k): j + 1 for j, k in reversed(list(enumerate(keep)))}        # the first position wins, as a scan would
    H, W = int(H), int(W)
    objects = {}
    for row in rows:
        r = int(row[0])
        if r == 0:
            continue
        if r - 1 >= len(names):
            raise ValueError('%s: instance %d has no part-level-0 line in the attribute file (%d lines)'
                             % (image or 'image', r, len(names)))
        obj_id = ids.get(names[r - 1])
        if obj_id is None:
            raise ValueError('%s: object name %r of instance %d is not among the index file\'s objectnames'
                             % (image or 'image', names[r - 1], r))
        if obj_id not in where:
            continue
        x1, y1, x2, y2 = int(row[2]) + 1, int(row[3]) + 1, int(row[4]) + 1, int(row[5]) + 1
        margin_x, margin_y = max((x2 - x1) // 100, 1), max((y2 - y1) // 100, 1)
        objects[str(r)] = {'bbox': [max(x1 - margin_x, 1), max(y1 - margin_y, 1), min(x2 + margin_x, W),
                                    min(y2 + margin_y, H)], 'cls': where[obj_id]}
    return {'imgHeight': H, 'imgWidth': W, 'objects': objects}


def _name_ids(objectnames):
    """name -> 1-based position of its first occurrence (upstream scans the list and stops at the first match)."""
    ids = {}
    for k, name in enumerate(objectnames):
        ids.setdefault(name, k + 1)
    return ids


def ade_info(seg, names, objectnames):
    """The box table of a ``_seg.png`` that is already on the device as a (H, W, 3|4) uint8 tensor.  Writes no file."""
    from . import ops
    _, _, rows = ops.ade_decode(seg, SORTED_50)
    return rows_to_info(seg.shape[0], seg.shape[1], rows, names, objectnames)


def bedroom_files(filenames, folders):
    """The index entries whose folder, without its first component, is the bedroom scene, in index order: their paths
    relative to the data root."""
    out = []
    for name, folder in zip(filenames, folders):
        parts = folder.split('/')[1:]
        if '/'.join(parts) == BEDROOM:
            out.append(os.path.join(*(parts + [name])))
    return out


def output_names(n, n_val=150):
    """``[(phase, prefix)]`` of ``n`` images: ``bedroom_%05d`` counted from 1, the first ``n_val`` to ``val``."""
    return [('val' if i < n_val else 'train', 'bedroom_%05d' % (i + 1)) for i in range(n)]


def _save_plane(path, plane):
    Image.fromarray(plane).save(path)                    # a 2-D uint8 array: mode 'L'


def convert(dataroot, n_val=150, device=None):
    """Upstream's main loop over ``<dataroot>/index_ade20k.mat``: for every bedroom image the ``.jpg`` copied to
    ``<phase>_img``, the label and instance planes as 8-bit PNGs in ``<phase>_label`` / ``<phase>_inst`` and the box table
    in ``<phase>_bbox``.  ``_seg.png`` and ``_atr.txt`` files are read on a small thread pool a few images ahead, so
    decoding overlaps the device pass and the writing of the image in hand.  Returns the number of images written."""
    import torch
    from . import ops
    device = _device(device)
    for phase in ('train', 'val'):
        for sub in ('bbox', 'img', 'label', 'inst'):
            os.makedirs(os.path.join(dataroot, '%s_%s' % (phase, sub)), exist_ok=True)
    filenames, folders, objectnames = load_index(os.path.join(dataroot, 'index_ade20k.mat'))
    ids = _name_ids(objectnames)
    files = [os.path.join(dataroot, f) for f in bedroom_files(filenames, folders)]
    targets = output_names(len(files), n_val)
    with ThreadPoolExecutor(max_workers=DECODE_THREADS) as pool:
        pending = [pool.submit(_read_pair, f) for f in files[:PREFETCH]]
        saves = []
        for i, file in enumerate(files):
            seg, names = pending.pop(0).result()
            if i + PREFETCH < len(files):
                pending.append(pool.submit(_read_pair, files[i + PREFETCH]))
            label, inst, rows = ops.ade_decode(torch.from_numpy(seg).to(device), SORTED_50)
            H, W = seg.shape[:2]
            info = rows_to_info(H, W, rows, names, ids, image=file)
            planes = ops.bytes_to_host(torch.stack((label, inst)))
            phase, prefix = targets[i]
            with open(os.path.join(dataroot, phase + '_bbox', prefix + BBOX_SUF), 'w') as f:
                json.dump(info, f)
            copyfile(file, os.path.join(dataroot, phase + '_img', prefix + IMG_SUF))
            saves.append(pool.submit(_save_plane, os.path.join(dataroot, phase + '_label', prefix + LABEL_SUF), planes[0]))
            saves.append(pool.submit(_save_plane, os.path.join(dataroot, phase + '_inst', prefix + INST_SUF), planes[1]))
            while len(saves) > 2 * PREFETCH:
                saves.pop(0).result()
        for s in saves:
            s.result()
    return len(files)


def main(argv=None):
    parser = argparse.ArgumentParser(description='Convert the bedroom scenes of a raw ADE20K download for the loader.')
    parser.add_argument('--dataroot', default='datasets/ade20k',
                        help='holds index_ade20k.mat and images/; the <phase>_* folders are created inside it')
    opt = parser.parse_args(argv)
    n = convert(opt.dataroot)
    print('converted %d images under %s' % (n, opt.dataroot))


if __name__ == '__main__':
    main()
