"""Brute-force restatement of the layout edits (include/him.h "Layout edits") in numpy, and seeded canvas builders.

``erase``: for every region pixel the squared distance to EVERY seed, the smallest distance, among equal ones the
smallest ``y * W + x`` -- O(|R| * |S|), no transform, no separable pass.  ``window`` restricts the seeds to a window
around the region and PROVES that no seed outside it can win (every distance found is below the distance to the
window's nearest side that has canvas behind it); without the proof it doubles the margin.  That keeps a 1024 x 2048
canvas affordable and changes no result.

``place``: Pillow's own ``Image.resize(NEAREST)`` of the cropped mask, pasted with plain slicing.
"""
import numpy as np
from PIL import Image

NO_SEED, CLASS_RANGE = 1, 2
EMPTY_BOX = [2 ** 31 - 1, 2 ** 31 - 1, -1, -1]
NP_KINDS = (np.uint8, np.int32, np.int64, np.float32)          # kind 0..3 of the C ABI


def class_of(label, n_class):
    """The class id per pixel, -1 where the value lies outside [0, n_class) or is not integral."""
    lab = np.asarray(label)
    f = lab.astype(np.float64)
    ok = (f >= 0) & (f < n_class) & (f == np.trunc(f))
    return np.where(ok, f, -1).astype(np.int64)


def bit_table(classes, n_class):
    words = np.zeros((n_class + 31) // 32, np.uint32)
    for c in classes:
        assert 0 <= c < n_class
        words[c >> 5] |= np.uint32(1 << (c & 31))
    return words


def _nearest_seed(py, px, sy, sx, W):
    """Per region pixel the (distance^2, flat index) of the winning seed; seeds given by coordinate arrays."""
    flat = sy.astype(np.int64) * W + sx
    best_d = np.empty(len(py), np.int64)
    best_i = np.empty(len(py), np.int64)
    step = max(1, (1 << 22) // max(len(sy), 1))
    for a in range(0, len(py), step):
        d = (py[a:a + step, None].astype(np.int64) - sy[None]) ** 2 + (px[a:a + step, None].astype(np.int64) - sx[None]) ** 2
        m = d.min(1)
        cand = np.where(d == m[:, None], flat[None], np.iinfo(np.int64).max)      # ties: the smallest y * W + x
        best_d[a:a + step], best_i[a:a + step] = m, cand.min(1)
    return best_d, best_i


def erase(label, inst, id=None, region=None, fill=(), n_class=1, window=None):
    """-> (label_out, inst_out, changed uint8, status [|R|, |S|, changed pixels, flags]).  ``window``: a starting margin
    (pixels) around the region's box for the seed search, see the module text; None searches the whole plane."""
    label, inst = np.asarray(label), np.asarray(inst)
    H, W = label.shape
    R = (np.asarray(region) != 0) if region is not None else (inst == id)
    cls = class_of(label, n_class)
    allowed = np.zeros(n_class + 1, bool)
    allowed[list(fill)] = True
    S = ~R & (cls >= 0) & allowed[np.where(cls >= 0, cls, n_class)]
    flags = (CLASS_RANGE if (cls < 0).any() else 0) | (0 if S.any() else NO_SEED)
    label_out, inst_out = label.copy(), inst.copy()
    changed = np.zeros((H, W), np.uint8)
    todo = R & (cls >= 0)
    if S.any() and todo.any():
        py, px = np.nonzero(todo)
        margin = window
        while True:
            if margin is None:
                y0, x0, y1, x1 = 0, 0, H, W
            else:
                y0, x0 = max(py.min() - margin, 0), max(px.min() - margin, 0)
                y1, x1 = min(py.max() + 1 + margin, H), min(px.max() + 1 + margin, W)
            sy, sx = np.nonzero(S[y0:y1, x0:x1])
            if len(sy):
                d, i = _nearest_seed(py, px, sy + y0, sx + x0, W)
                # a seed outside the window is at least this far from the pixel (sides on the canvas edge hide nothing)
                out = np.full(len(py), np.iinfo(np.int64).max, np.int64)
                if y0 > 0:
                    out = np.minimum(out, py - y0 + 1)
                if x0 > 0:
                    out = np.minimum(out, px - x0 + 1)
                if y1 < H:
                    out = np.minimum(out, y1 - py)
                if x1 < W:
                    out = np.minimum(out, x1 - px)
                if (d < out.astype(np.float64) ** 2).all():
                    break
            assert margin is not None
            margin *= 2
        label_out[py, px] = label.reshape(-1)[i]
        inst_out[py, px] = inst.reshape(-1)[i]
        changed = (label_out != label).astype(np.uint8)
    return label_out, inst_out, changed, [int(R.sum()), int(S.sum()), int(changed.sum()), flags]


def resized_mask(mask, dw, dh):
    """Pillow's NEAREST resize of a boolean mask (as an 8-bit image) to (dh, dw)."""
    im = Image.fromarray(mask.astype(np.uint8) * 255, mode='L').resize((dw, dh), Image.NEAREST)
    return np.asarray(im) != 0


def place(label_dst, inst_dst, inst_src, id, src_box, dst_box, cls, new_id, protect=()):
    """-> (label_out, inst_out, changed uint8, status [written, blocked, xmin, ymin, xmax, ymax inclusive], the resized
    mask at the destination box's size, before clipping and protection)."""
    label_out, inst_out = np.asarray(label_dst).copy(), np.asarray(inst_dst).copy()
    Hd, Wd = label_out.shape
    sx0, sy0, sx1, sy1 = src_box
    dx0, dy0, dx1, dy1 = dst_box
    mask = resized_mask(np.asarray(inst_src)[sy0:sy1, sx0:sx1] == id, dx1 - dx0, dy1 - dy0)
    full = np.zeros((Hd, Wd), bool)
    cx0, cy0, cx1, cy1 = max(dx0, 0), max(dy0, 0), min(dx1, Wd), min(dy1, Hd)
    if cx1 > cx0 and cy1 > cy0:
        full[cy0:cy1, cx0:cx1] = mask[cy0 - dy0:cy1 - dy0, cx0 - dx0:cx1 - dx0]
    prot = np.zeros((Hd, Wd), bool)
    if len(protect):
        c = class_of(label_out, max(protect) + 1)
        prot = np.isin(c, list(protect))
    write, blocked = full & ~prot, full & prot
    label_out[write] = cls
    inst_out[write] = new_id
    box = list(EMPTY_BOX)
    if write.any():
        ys, xs = np.nonzero(write)
        box = [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]
    return label_out, inst_out, write.astype(np.uint8), [int(write.sum()), int(blocked.sum())] + box, mask


# ---------------------------------------------------------------------------------------------------- seeded builders
def canvas(H, W, seed, n_class=12, block=3):
    """A label plane of ``block``-sized patches of classes 0..n_class-1 and an instance plane equal to it (stuff)."""
    g = np.random.default_rng(seed)
    lab = g.integers(0, n_class, size=(H // block + 1, W // block + 1)).repeat(block, 0).repeat(block, 1)[:H, :W]
    return lab.astype(np.int64), lab.astype(np.int64).copy()


def add_object(label, inst, mask, cls, id):
    label[mask] = cls
    inst[mask] = id
    return label, inst


def ellipse(H, W, cy, cx, ry, rx):
    y, x = np.mgrid[0:H, 0:W]
    return ((y - cy) / float(ry)) ** 2 + ((x - cx) / float(rx)) ** 2 <= 1.0
