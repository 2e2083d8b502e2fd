"""Seeded instance / label pairs in the raw Cityscapes layout (``<root>/<city>/<stem>_gtFine_{instanceIds,labelIds}.png``)
for the preprocessing step, and the numpy restatement of the reference's ``construct_box`` the tests compare against at
sizes the reference is too slow for.  The golden generator (tests/golden/make_golden_preprocess.py, run where the
reference is present) and the tests (run anywhere) build byte-identical files from the same seeds; the generator also
asserts that ``restate`` reproduces the reference on every pair below."""
import os

import numpy as np
from PIL import Image

INST_PATTERN, CLS_PATTERN = '*_gtFine_instanceIds.png', '*_gtFine_labelIds.png'
THING_CLASSES = [24, 25, 26, 27, 28, 31, 32, 33]
COLUMNS = ('id', 'xmin', 'ymin', 'xmax', 'ymax', 'count', 'cls')


def _ellipse(H, W, cx, cy, a, b):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((xx - cx) / float(a)) ** 2 + ((yy - cy) / float(b)) ** 2 <= 1.0


def synth_pair(seed, H, W, n_inst, max_axis=None):
    """(inst uint16, label uint8): blocky background whose instance id is its class (ids below 1000, as Cityscapes stores
    stuff classes) and ``n_inst`` elliptical instances ``cls * 1000 + k``; every fourth has a second, separate blob, every
    third carries two classes under one id.  Later ellipses cover earlier ones."""
    rng = np.random.RandomState(seed)
    gh, gw = max(H // 32, 1), max(W // 32, 1)
    coarse = rng.randint(0, 23, (gh, gw)).astype(np.uint8)
    label = np.kron(coarse, np.ones((H // gh + 1, W // gw + 1), np.uint8))[:H, :W].copy()
    inst = label.astype(np.uint16)
    max_axis = max_axis or max(min(H, W) // 6, 2)
    for k in range(n_inst):
        cls = THING_CLASSES[rng.randint(len(THING_CLASSES))]
        iid = cls * 1000 + k
        blobs = 2 if k % 4 == 3 else 1
        for _ in range(blobs):
            a, b = rng.randint(1, max_axis + 1), rng.randint(1, max_axis + 1)
            cx, cy = rng.randint(0, W), rng.randint(0, H)
            x0, x1, y0, y1 = max(cx - a, 0), min(cx + a + 1, W), max(cy - b, 0), min(cy + b + 1, H)
            m = _ellipse(y1 - y0, x1 - x0, cx - x0, cy - y0, a, b)           # inside its bounding window only
            wi, wl = inst[y0:y1, x0:x1], label[y0:y1, x0:x1]
            wi[m] = iid
            wl[m] = cls
            if k % 3 == 2:                           # a second class under the same id (the median decides)
                part = m & (np.arange(x0, x1)[None, :] % 5 < rng.randint(1, 4))
                wl[part] = THING_CLASSES[rng.randint(len(THING_CLASSES))]
    return inst, label


def _edge_pair():
    """64 x 383: the hand-placed corner cases."""
    H, W = 64, 383
    label = np.full((H, W), 7, np.uint8)
    inst = np.full((H, W), 7, np.uint16)             # id 7 < 1000: never an object
    inst[0, :], inst[H - 1, :], inst[:, 0], inst[:, W - 1] = 26003, 26003, 26003, 26003    # touches all four borders
    label[inst == 26003] = 26
    inst[10, 17], label[10, 17] = 24001, 24                                  # one pixel
    inst[20:24, 30:37], label[20:24, 30:37] = 25002, 25                      # two separate blobs
    inst[40:47, 300:302], label[40:47, 300:302] = 25002, 25
    inst[30, 100:102] = 27004                                                # two pixels, classes c and c + 1
    label[30, 100], label[30, 101] = 27, 28
    inst[50:52, 200:202] = 31005                                             # four pixels, 2 / 2 split
    label[50, 200:202], label[51, 200:202] = 31, 32
    inst[5:9, 370:380], label[5:9, 370:380] = 65535, 33                      # the largest 16-bit id
    inst[12:15, 50:60], label[12:15, 50:60] = 999, 11                        # just below the threshold
    inst[33:36, 60:65] = 1000                                                # the smallest object id; 3 classes, odd count
    label[33, 60:65], label[34, 60:65], label[35, 60:65] = 3, 9, 200
    return inst, label


def pairs():
    """[(city, stem, inst, label)]: inst uint16 (written as a 16-bit PNG) or uint8 (written in ``L`` mode), label uint8."""
    out = [('aachen', 'aachen_000000_000019', ) + synth_pair(11, 96, 160, 30),
           ('aachen', 'aachen_000001_000019', ) + _edge_pair()]
    H, W = 48, 80
    stuff = np.kron(np.arange(6, dtype=np.uint8).reshape(2, 3), np.ones((24, 27), np.uint8))[:H, :W].copy()
    out.append(('aachen', 'aachen_000002_000019', stuff.astype(np.uint16), stuff))              # no instance at all
    inst, label = synth_pair(12, 37, 1, 0)
    inst[3:9, 0], label[3:9, 0] = 24000, 24
    inst[20, 0], label[20, 0] = 33001, 33
    out.append(('bonn', 'bonn_000000_000019', inst, label))                                      # width 1
    inst, label = synth_pair(13, 1, 53, 0)
    inst[0, 0:4], label[0, 0:4] = 26000, 26
    inst[0, 40:53], label[0, 40:53] = 28001, 28
    label[0, 45:53] = 27
    out.append(('bonn', 'bonn_000001_000019', inst, label))                                      # height 1
    inst, label = synth_pair(14, 40, 72, 0)
    inst8 = (inst % 7).astype(np.uint8)
    inst8[_ellipse(40, 72, 20, 20, 9, 6)] = 200
    inst8[_ellipse(40, 72, 50, 12, 5, 8)] = 255
    out.append(('bonn', 'bonn_000002_000019', inst8, label))                                     # an L-mode instance file
    out.append(('cologne', 'cologne_000000_000019', ) + synth_pair(15, 50, 383, 24))             # odd width, many
    return out


def write_tree(root):
    """Write every pair under ``root``; returns [(json stem, inst, label)] in the order ``construct_box`` visits them."""
    listed = []
    for city, stem, inst, label in pairs():
        os.makedirs(os.path.join(root, city), exist_ok=True)
        Image.fromarray(inst).save(os.path.join(root, city, stem + '_gtFine_instanceIds.png'))
        Image.fromarray(label, 'L').save(os.path.join(root, city, stem + '_gtFine_labelIds.png'))
        listed.append((os.path.join(city, stem), stem + '_gtFine_instanceIds', inst, label))
    return [(s, i, l) for _, s, i, l in sorted(listed, key=lambda t: t[0])]


def restate(inst, label, min_id=1000):
    """The reference's per-instance loop (np.where -> min / max, int(np.median(classes))) as one sort, reduceat and a
    256-bin count per object: (n, 7) int64 rows (id, xmin, ymin, xmax, ymax, count, cls) in ascending id order."""
    inst = np.asarray(inst).astype(np.int64)
    lab = np.asarray(label).astype(np.int64).ravel()
    H, W = inst.shape
    flat = inst.ravel()
    order = np.argsort(flat, kind='stable')
    ids, start, counts = np.unique(flat[order], return_index=True, return_counts=True)
    ys, xs = order // W, order % W
    xmin, xmax = np.minimum.reduceat(xs, start), np.maximum.reduceat(xs, start)
    ymin, ymax = np.minimum.reduceat(ys, start), np.maximum.reduceat(ys, start)
    lab = lab[order]
    rows = []
    for i, iid in enumerate(ids):
        if iid < min_id:
            continue
        n = int(counts[i])
        cum = np.cumsum(np.bincount(lab[start[i]:start[i] + n], minlength=256))
        lo = int(np.searchsorted(cum, (n - 1) // 2, side='right'))      # the two middle order statistics
        hi = int(np.searchsorted(cum, n // 2, side='right'))
        rows.append((int(iid), int(xmin[i]), int(ymin[i]), int(xmax[i]), int(ymax[i]), n, (lo + hi) // 2))
    return np.array(rows, dtype=np.int64).reshape(-1, 7)


def rows_to_info(H, W, rows):
    """The dict the reference dumps, from rows."""
    return {'imgHeight': int(H), 'imgWidth': int(W),
            'objects': {str(int(r[0])): {'bbox': [int(r[1]), int(r[2]), int(r[3]), int(r[4])], 'cls': int(r[6])}
                        for r in rows}}
