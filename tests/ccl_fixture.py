"""Integer numpy restatement of include/him.h "Instance labelling of layouts" and the deterministic planes the CCL
tests run on (helper module like preprocess_fixture.py; imports nothing from the package).

``label_reference`` is a union-find over the row runs of a plane: runs come from one vectorised compare, the pairs of
runs that touch across two rows from shifted compares, and only the distinct pairs go through the (Python) union loop.
A run's number grows with the raster index of its first pixel, so the smallest run of a component starts at the
component's first pixel, which is what orders the instance ids."""
import numpy as np

OVERFLOW, CLS_RANGE = 1, 2
TILE_H, TILE_W = 32, 64                # the kernel's tile; the cases below are worded in it
STUFF, STUFF2 = 7, 21                  # classes the tests never list as things
CITY_THINGS = tuple(range(24, 34))


def thing_table(things):
    t = np.zeros(256, np.uint8)
    for c in things:
        t[int(c)] = 1
    return t


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def label_reference(cls, things, connectivity=4, min_area=1, base_id=1000, max_objects=1024):
    """-> (inst int32 (H,W), count, flags) of ONE plane; ``cls`` any integer or float array."""
    assert connectivity in (4, 8)
    a = np.asarray(cls)
    H, W = a.shape
    if a.dtype.kind == 'f':
        ok = (a >= 0) & (a < 256) & (a == np.floor(a))
    else:
        ok = (a >= 0) & (a < 256)
    flags = 0 if ok.all() else CLS_RANGE
    c = np.where(ok, a, 0).astype(np.int64)
    tc = np.where(ok & (thing_table(things)[c] != 0), c, -1)
    start = np.ones((H, W), bool)
    start[:, 1:] = tc[:, 1:] != tc[:, :-1]
    run = (np.cumsum(start.reshape(-1)) - 1).reshape(H, W)
    nruns = int(run[-1, -1]) + 1
    pairs = []
    shifts = [(slice(None), slice(None))] if connectivity == 4 else \
        [(slice(None), slice(None)), (slice(1, None), slice(None, -1)), (slice(None, -1), slice(1, None))]
    for lo, up in shifts:                                   # lower row's columns, upper row's columns
        low_c, up_c = tc[1:, lo], tc[:-1, up]
        touch = (low_c == up_c) & (low_c >= 0)
        pairs.append(run[1:, lo][touch] * nruns + run[:-1, up][touch])
    keys = np.unique(np.concatenate(pairs)) if pairs else np.zeros(0, np.int64)
    parent = list(range(nruns))
    for k in keys.tolist():
        ra, rb = _find(parent, k // nruns), _find(parent, k % nruns)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.array([_find(parent, r) for r in range(nruns)], np.int64)
    run_thing = np.zeros(nruns, bool)
    run_thing[run[tc >= 0]] = True
    comp = root[run]                                        # per pixel: the component's smallest run
    area = np.bincount(comp[tc >= 0], minlength=nruns)
    kept = run_thing & (root == np.arange(nruns)) & (area >= max(int(min_area), 1))
    rank = np.cumsum(kept) - 1
    count = int(kept.sum())
    inst = np.where((tc >= 0) & kept[comp], base_id + rank[comp], np.where(ok, a, -1).astype(np.int64))
    if count > max_objects or base_id + count - 1 > 65535:
        flags |= OVERFLOW
    return inst.astype(np.int32), count, flags


def partition_equal(a, b):
    """Two label planes cut the pixels into the same sets (label values aside)."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    pa = np.unique(np.stack([a, b]), axis=1)
    return len(np.unique(pa[0])) == pa.shape[1] and len(np.unique(pa[1])) == pa.shape[1]


# ---- planes -----------------------------------------------------------------------------------------------------------
def serpentine(H, W, cls=26, transpose=False):
    """One component that winds through the whole plane: every second line is full, the lines between hold one joining
    pixel at alternating ends."""
    if transpose:
        return np.ascontiguousarray(serpentine(W, H, cls).T)
    p = np.full((H, W), STUFF, np.uint8)
    p[0::2] = cls
    for y in range(1, H, 2):
        p[y, W - 1 if (y // 2) % 2 == 0 else 0] = cls
    return p


def comb(H=70, W=140, cls=25):
    """Teeth that hang down from above: they lie side by side in tile row 0 and meet only through a bar in tile row 1
    (rows >= 32); a second comb stands upright with its bar in tile row 0."""
    p = np.full((H, W), STUFF, np.uint8)
    for x in range(2, 60, 4):
        p[3:40, x] = cls                                    # teeth across the border at row 32
    p[40, 2:59] = cls                                       # the bar, in the next tile row
    for x in range(70, 136, 6):
        p[10:50, x] = cls + 1
    p[10, 70:131] = cls + 1                                 # bar above, teeth reach down over the border
    for x in range(3, 60, 8):
        p[50:66, x] = cls                                   # loose teeth: one component each
    return p


def split_by_stuff_line(H=70, W=140, cls=27):
    """Two slabs of one class on both sides of a tile border, separated by a one-pixel line of stuff on the border's
    first row / column: nothing may join through it."""
    p = np.full((H, W), cls, np.uint8)
    p[TILE_H, :] = STUFF                                    # row 32: first row of tile row 1
    p[:, TILE_W] = STUFF2                                   # column 64: first column of tile column 1
    p[TILE_H - 1, TILE_W - 1] = STUFF                       # and no way round the corner diagonally
    return p


def checkerboard(H=33, W=65, a=24, b=25):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy + xx) % 2 == 0, a, b).astype(np.uint8)


def stair(H=100, W=200, cls=28, anti=False):
    """One pixel per row on a diagonal through tile corners: x = y + 32 steps (31,63) -> (32,64) and (95,127) ->
    (96,128); the anti-diagonal x = 95 - y steps (31,64) -> (32,63), the up-right neighbour across a corner."""
    p = np.full((H, W), STUFF, np.uint8)
    for y in range(H):
        x = (TILE_W + TILE_H - 1 - y) if anti else (TILE_W - TILE_H + y)
        if 0 <= x < W:
            p[y, x] = cls
    return p


def blobs(min_area=7, H=40, W=90):
    """Row blobs of min_area - 1, min_area and min_area + 1 pixels of thing classes, first the small one."""
    p = np.full((H, W), STUFF, np.uint8)
    p[2, 3:3 + min_area - 1] = 24
    p[5, 60:60 + min_area] = 24                             # straddles column 64
    p[9:11, 10:10 + (min_area + 1) // 2] = 26               # two rows: (min_area + 1) // 2 * 2 pixels
    p[30:34, 20] = 25                                       # 4 pixels across row 32: dropped for min_area 7
    p[31:35, 40:42] = 25                                    # 8 pixels across row 32: kept
    p[20, 70:70 + min_area - 1] = 31
    p[21, 70 + min_area - 2] = 31                           # min_area pixels in an L
    return p


def coarse_layout(H=256, W=512, classes=35, cell=16, seed=0, salt=0.02):
    """A Cityscapes-like plane: a coarse grid of random classes upsampled by ``cell``, with salt noise."""
    rng = np.random.RandomState(seed)
    coarse = rng.randint(0, classes, size=((H + cell - 1) // cell, (W + cell - 1) // cell))
    p = np.kron(coarse, np.ones((cell, cell), np.int64))[:H, :W]
    noise = rng.rand(H, W) < salt
    p = np.where(noise, rng.randint(0, classes, size=(H, W)), p)
    return p.astype(np.uint8)


def rects_and_ells(H=72, W=150):
    """Known rectangles and L-shapes; returns (plane, expected rows id, xmin, ymin, xmax, ymax, count, cls) for things =
    CITY_THINGS, 4-connectivity, min_area 1."""
    p = np.full((H, W), STUFF, np.uint8)
    p[40:, :] = STUFF2
    rows = []
    p[4:10, 5:20] = 26                                      # first pixel (4,5)
    rows.append([1000, 5, 4, 19, 9, 6 * 15, 26])
    p[6:50, 60:70] = 24                                     # first pixel (6,60): across both tile borders
    rows.append([1001, 60, 6, 69, 49, 44 * 10, 24])
    p[20:36, 100:104] = 33                                  # an L: upright 16 x 4 and a foot 4 x 30
    p[32:36, 100:130] = 33
    rows.append([1002, 100, 20, 129, 35, 16 * 4 + 4 * 30 - 4 * 4, 33])
    p[60:70, 30:33] = 26                                    # a second object of class 26, an L mirrored
    p[67:70, 10:33] = 26
    rows.append([1003, 10, 60, 32, 69, 10 * 3 + 3 * 23 - 3 * 3, 26])
    return p, np.array(rows, np.int64)
