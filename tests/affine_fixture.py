"""Numpy restatement of include/him.h "Affine layout edits" (helper module, not a conftest; it never imports the
package's kernels or ``ops``: a map enters as its six integers).

The map is integer arithmetic, restated here in int64: ``uv`` (U, V), ``nearest`` ((U + 2^23) >> 24, floor), ``split``
(integer part and the exact fraction).  ``place`` restates the mask / protect / status semantics of
him_layout_place_affine as plain loops over the destination box.  ``warp`` is the bicubic sample in float64 with
clamped taps, written as the double sum over the 16 products (the device sums separably), with Keys' polynomial in its
expanded textbook form (the device evaluates it by Horner's rule).

Bound of ``warp_bound`` (derived, not measured).  The device computes weights and sums in fp64 and narrows once.  Per
output element, with ref the float64 sample here, S = sum |wy_j| |wx_i| |v_ji| and A = sum |v_ji| over the 16 taps,
e64 = 2^-53:
  weights   the fraction t and the four distances are exact.  One 1-D weight is a cubic in d <= 2 with intermediate values
            <= 18; three roundings propagated through the remaining multiplications by d give <= 44 e64 < 2^-47 on
            either side, 2^-46 between the two.  A product wy wx (|w| <= 1) then differs by <= 2^-44 between the sides:
            2^-44 A over the taps.
  sums      8 fused multiply-adds on the device, 16 products and 16 additions here, every partial sum <= S in magnitude:
            <= 32 e64 S.
  narrowing half an fp32 ulp of the fp64 result: <= 2^-24 (|ref| + the terms above), or 2^-150 below the normal range.
  bound = 2^-24 |ref| + 2^-149 + (1 + 2^-24) (32 e64 S + 2^-44 A).
On a map with zero fractions the weights are exactly (0, 1, 0, 0) on both sides and the result is the source value."""
import numpy as np

FRAC = 24
ONE = 1 << FRAC
HALF = 1 << (FRAC - 1)
MAX_LINEAR, MAX_OFFSET = 1 << 30, 1 << 52
EMPTY_BOX = [2 ** 31 - 1, 2 ** 31 - 1, -1, -1]
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53


def uv(inv, x, y):
    """(U, V) int64 at the destination indices ``x``, ``y`` (arrays broadcast against each other)."""
    a00, a01, a02, a10, a11, a12 = (np.int64(v) for v in inv)
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    return a00 * x + a01 * y + a02, a10 * x + a11 * y + a12


def nearest(inv, x, y):
    """The nearest source pixel (xs, ys): floor((U + 2^23) / 2^24), the one tie rule."""
    U, V = uv(inv, x, y)
    return (U + HALF) >> FRAC, (V + HALF) >> FRAC


def split(inv, x, y):
    """(ix, tx, iy, ty): floor(U / 2^24) and the fraction as float64 (a multiple of 2^-24, exact)."""
    U, V = uv(inv, x, y)
    return U >> FRAC, (U & (ONE - 1)).astype(np.float64) / ONE, V >> FRAC, (V & (ONE - 1)).astype(np.float64) / ONE


def keys(t):
    """Keys' cubic, a = -0.5, at the distances 1 + t, t, 1 - t, 2 - t -> array (4,) + t.shape."""
    t = np.asarray(t, np.float64)

    def near(d):
        return 1.5 * d ** 3 - 2.5 * d ** 2 + 1.0

    def far(d):
        return -0.5 * d ** 3 + 2.5 * d ** 2 - 4.0 * d + 2.0
    return np.stack([far(1.0 + t), near(t), near(1.0 - t), far(2.0 - t)])


def class_of(label, n_class):
    f = np.asarray(label).astype(np.float64)
    ok = (f >= 0) & (f < n_class) & (f == np.trunc(f))
    return np.where(ok, f, -1).astype(np.int64)


def mask(inst_src, id, src_box, dst_box, inv):
    """The resampled mask over the destination box (dy1 - dy0, dx1 - dx0), before clipping and protection: one pixel
    at a time."""
    sx0, sy0, sx1, sy1 = src_box
    dx0, dy0, dx1, dy1 = dst_box
    src = np.asarray(inst_src)
    out = np.zeros((dy1 - dy0, dx1 - dx0), bool)
    for y in range(dy0, dy1):
        for x in range(dx0, dx1):
            xs, ys = nearest(inv, x, y)
            if sx0 <= xs < sx1 and sy0 <= ys < sy1 and src[ys, xs] == id:
                out[y - dy0, x - dx0] = True
    return out


def place(label_dst, inst_dst, inst_src, id, src_box, dst_box, inv, cls, new_id, protect=()):
    """-> (label_out, inst_out, changed uint8, status [written, blocked, xmin, ymin, xmax, ymax inclusive], mask)."""
    label_out, inst_out = np.asarray(label_dst).copy(), np.asarray(inst_dst).copy()
    Hd, Wd = label_out.shape
    dx0, dy0, dx1, dy1 = dst_box
    m = mask(inst_src, id, src_box, dst_box, inv)
    cls_now = class_of(label_out, max(protect) + 1) if len(protect) else None
    changed = np.zeros((Hd, Wd), np.uint8)
    written = blocked = 0
    box = list(EMPTY_BOX)
    for y in range(max(dy0, 0), min(dy1, Hd)):
        for x in range(max(dx0, 0), min(dx1, Wd)):
            if not m[y - dy0, x - dx0]:
                continue
            if cls_now is not None and cls_now[y, x] in protect:
                blocked += 1
                continue
            label_out[y, x], inst_out[y, x], changed[y, x] = cls, new_id, 1
            written += 1
            box = [min(box[0], x), min(box[1], y), max(box[2], x), max(box[3], y)]
    return label_out, inst_out, changed, [written, blocked] + box, m


def taps(inv, window, Hs, Ws):
    """Clamped tap indices and weights of every pixel of the ``window`` (x0, y0, H, W): (cx (4,H,W), cy (4,H,W), wx
    (4,H,W), wy (4,H,W)); tap k is source index i - 1 + k."""
    x0, y0, H, W = window
    y, x = np.mgrid[y0:y0 + H, x0:x0 + W]
    ix, tx, iy, ty = split(inv, x, y)
    k = np.arange(-1, 3, dtype=np.int64)[:, None, None]
    return np.clip(ix[None] + k, 0, Ws - 1), np.clip(iy[None] + k, 0, Hs - 1), keys(tx), keys(ty)


def warp(src, inv, window):
    """-> (ref (3,H,W) float64, S (3,H,W), A (3,H,W)) for ``src`` (3,Hs,Ws)."""
    src = np.asarray(src)
    cx, cy, wx, wy = taps(inv, window, src.shape[1], src.shape[2])
    s64 = src.astype(np.float64)
    ref = np.zeros((3,) + cx.shape[1:])
    S, A = np.zeros_like(ref), np.zeros_like(ref)
    for j in range(4):
        for i in range(4):
            v = s64[:, cy[j], cx[i]]
            w = wy[j] * wx[i]
            ref += w[None] * v
            S += np.abs(w)[None] * np.abs(v)
            A += np.abs(v)
    return ref, S, A


def warp_bound(ref, S, A):
    return EPS32 * np.abs(ref) + 2.0 ** -149 + (1 + EPS32) * (32 * EPS64 * S + 2.0 ** -44 * A)


def reads(inv, window, Hs, Ws, py, px):
    """(H,W) bool: the outputs whose 16 clamped taps include the source pixel (py, px)."""
    cx, cy, _, _ = taps(inv, window, Hs, Ws)
    return (cx == px).any(0) & (cy == py).any(0)


# ---------------------------------------------------------------------------------------------------- seeded builders
def blob(h=37, w=53):
    """A blob with a hole and a one-pixel spur, touching the box's four sides; no symmetry a wrong map would keep."""
    y, x = np.mgrid[0:h, 0:w]
    m = ((y - h * 0.45) / (h * 0.40)) ** 2 + ((x - w * 0.40) / (w * 0.33)) ** 2 <= 1.0
    m &= ~(((y - h * 0.40) / (h * 0.10)) ** 2 + ((x - w * 0.35) / (w * 0.08)) ** 2 <= 1.0)
    m[h // 2, w // 2:] = True
    m[0, :w // 3] = m[h - 1, w // 2:] = True
    m[:, 0] |= (y[:, 0] % 3 == 0)
    m[h - 3:, w - 1] = True
    return m


def picture(seed, H, W):
    """(3,H,W) float32 in [0,1) with full mantissas."""
    return np.random.default_rng(seed).random((3, H, W), dtype=np.float32)
