"""Helper module (like util.py; not a conftest): a numpy restatement of include/him.h "Set-level metrics" -- the
Laplacian pyramid, the patch descriptors, the normalisation, the projection, the key order of the sort and the sliced
Wasserstein distance -- in float64, with ``dtype=np.float32`` giving the fp32 twin that measures ``e32``; the comparison
helpers of the GPU tests; seeded inputs.  Written from the definition, element by element where that is the clearest
form: the pyramid inserts its zeros and mirrors its borders literally."""
import json
import math
import os

import numpy as np

PATCH, PP = 7, 49
LDS_MAX = 8192                      # HIM_SORT_LDS_MAX of include/him.h
ZERO_DEVIATION = 1
EPS32 = 2.0 ** -24
K5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def n_levels(H, W, want=None):
    m, l = min(H, W), 0
    while (m >> l) >= 16:
        l += 1
    return l if want is None or want <= 0 or want > l else want


def mirror(i, n):
    """Index i of a line of n cells continued as d c b | a b c d | c b a."""
    if n == 1:
        return 0
    p = 2 * n - 2
    i %= p
    return i if i < n else p - i


def filter5(x, axis, gain=1.0, border=mirror):
    """The five-tap filter along ``axis`` in x's own dtype, borders by ``border``."""
    n = x.shape[axis]
    out = np.zeros_like(x)
    k = (K5 * gain).astype(x.dtype)
    for t in range(5):
        idx = np.array([border(i + t - 2, n) for i in range(n)])
        out = out + k[t] * np.take(x, idx, axis=axis)
    return out


def down(x, border=mirror):
    return filter5(filter5(x, -1, 1.0, border), -2, 1.0, border)[..., ::2, ::2]


def up(x, gain=2.0, border=mirror):
    z = np.zeros(x.shape[:-2] + (2 * x.shape[-2], 2 * x.shape[-1]), x.dtype)
    z[..., ::2, ::2] = x
    return filter5(filter5(z, -1, gain, border), -2, gain, border)


def pyramid(x, levels=None, dtype=np.float64, border=mirror, up_gain=2.0):
    """(laplacian levels, gaussian levels) of x (B, C, H, W), finest first; ``up_gain`` per direction."""
    g = [np.asarray(x).astype(dtype)]
    L = n_levels(x.shape[-2], x.shape[-1], levels)
    for _ in range(L - 1):
        g.append(down(g[-1], border))
    lap = [g[i] - up(g[i + 1], up_gain, border) for i in range(L - 1)] + [g[-1]]
    return lap, g


def clamp_positions(pos, h, w):
    """(clamped table, number of corners that moved)."""
    p = np.asarray(pos).astype(np.int64)
    c = np.stack([np.clip(p[..., 0], 0, h - PATCH), np.clip(p[..., 1], 0, w - PATCH)], -1)
    return c, int((c != p).any(-1).sum())


def gather(level, pos):
    """Rows (B * n, 49 C) of ``level`` (B, C, h, w), channel-major, in level's dtype, and the clamp count."""
    B, C, h, w = level.shape
    c, moved = clamp_positions(pos, h, w)
    rows = np.empty((B, c.shape[1], C * PP), level.dtype)
    for b in range(B):
        for p in range(c.shape[1]):
            y, x = c[b, p]
            rows[b, p] = level[b, :, y:y + PATCH, x:x + PATCH].reshape(-1)
    return rows.reshape(-1, C * PP), moved


def channel_stats(desc, C, ddof=0):
    """mean and deviation (C,) in float64 over all rows and the 49 positions; ddof = 0 is the definition."""
    d = np.asarray(desc, np.float64).reshape(len(desc), C, PP)
    return d.mean((0, 2)), d.std((0, 2), ddof=ddof)


def normalise(desc, C, dtype=np.float64, ddof=0):
    mean, std = channel_stats(desc, C, ddof)
    d = np.asarray(desc).astype(dtype).reshape(len(desc), C, PP)
    with np.errstate(divide='ignore', invalid='ignore'):
        z = (d - mean.astype(dtype)[None, :, None]) / std.astype(dtype)[None, :, None]
    if (std == 0).any():
        z = np.full_like(z, np.nan)
    return z.reshape(len(desc), C * PP)


def directions(seed, C, n_dirs):
    """(49 C, n_dirs) fp32: util.metrics.swd_tables restated."""
    d = np.random.RandomState(int(seed) & 0x7fffffff).randn(n_dirs, PP * C)
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    return np.ascontiguousarray(d.T).astype(np.float32)


def positions(seed, index, B, n, h, w, level=0, which=0):
    out = np.empty((B, n, 2), np.int32)
    for b in range(B):
        rs = np.random.RandomState([int(seed) & 0x7fffffff, which, level, index + b])
        out[b, :, 0] = rs.randint(0, h - 6, n)
        out[b, :, 1] = rs.randint(0, w - 6, n)
    return out


def project(desc, C, dirs, dtype=np.float64, ddof=0):
    """(n_dirs, N) projections of the normalised rows, in ``dtype``."""
    return (normalise(desc, C, dtype, ddof) @ np.asarray(dirs).astype(dtype)).T.copy()


def sort_keys(bits):
    """The unsigned keys whose order is the sort's order, from uint32 bit patterns."""
    b = np.asarray(bits, np.uint32)
    return np.where(b >> 31, b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000)).astype(np.uint32)


def key_sort(x):
    """fp32 array (..., N) sorted along the last axis in the sign-fixed key order, as uint32 bit patterns; NaN count."""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32)
    order = np.argsort(sort_keys(bits), axis=-1, kind='stable')
    nans = int(((bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)).sum())
    return np.take_along_axis(bits, order, -1), nans


def distance(pa, pb):
    """(level distance, per-direction sums) of two (n_dirs, N) projection arrays (sorted here, plain float order)."""
    a, b = np.sort(np.asarray(pa, np.float64), -1), np.sort(np.asarray(pb, np.float64), -1)
    s = np.abs(a - b).sum(-1)
    return float(s.sum() / a.size), s


def swd(fake, real, n_patches, n_dirs, levels=None, seed=0, same_positions=False, dtype=np.float64):
    """Per level: dict(dist, proj_a, proj_b) of two sets (N, C, H, W), the whole definition end to end."""
    N, C, H, W = fake.shape
    dirs = directions(seed, C, n_dirs)
    out = []
    pyr = [pyramid(x, levels, dtype)[0] for x in (fake, real)]
    for l in range(len(pyr[0])):
        proj = []
        for which in (0, 1):
            lv = pyr[which][l]
            pos = positions(seed, 0, N, n_patches, lv.shape[-2], lv.shape[-1], l, 0 if same_positions else which)
            proj.append(project(gather(lv, pos)[0], C, dirs, dtype))
        out.append(dict(dist=distance(*proj)[0], proj_a=proj[0], proj_b=proj[1]))
    return out


# ------------------------------------------------------------------------------------------------ comparison helpers
def direct_limit(e32):
    return max(8.0 * e32, 16.0 * EPS32)


def scaled_err(got, ref64, scale=None):
    r = np.asarray(ref64, np.float64)
    g = np.asarray(got, np.float64)
    scale = float(np.abs(r).max()) if scale is None else float(scale)
    err = np.abs(g - r)
    if not np.isfinite(err).all():
        return float('inf')
    return float(err.max()) / max(scale, 1e-300) if err.size else 0.0


def check_direct(case, tensor, got, ref64, ref32, rows=None, scale=None):
    """max|got - ref64| / max|ref64| <= max(8 e32, 16 2^-24); the row is recorded before the assertion."""
    err, e32 = scaled_err(got, ref64, scale), scaled_err(ref32, ref64, scale)
    lim = direct_limit(e32)
    if rows is not None:
        rows.append(dict(case=case, tensor=tensor, err=err, e32=e32, ratio=err / e32 if e32 > 0 else None, limit=lim))
    assert err <= lim, '%s %s: error %.3e > limit %.3e (e32 %.3e)' % (case, tensor, err, lim, e32)
    return err, e32


def check_sorted_bits(case, got, given, got_nans=None, rows=None):
    """``got`` (the kernel's output) must hold exactly the bits of the key-sort of ``given`` (the kernel's input)."""
    want, nans = key_sort(given)
    gb = np.ascontiguousarray(got, np.float32).view(np.uint32)
    same = gb.shape == want.shape and bool((gb == want).all())
    if rows is not None:
        rows.append(dict(case=case, tensor='keys', err=0.0 if same else 1.0, e32=0.0, ratio=None, limit=0.0))
    assert same, '%s: sorted bits differ at %s' % (case, np.argwhere(gb != want)[:4].tolist() if gb.shape == want.shape else 'shape')
    if got_nans is not None:
        assert int(got_nans) == nans, '%s: %d NaNs counted, %d present' % (case, int(got_nans), nans)


def check_sum(case, tensor, got, terms, rows=None):
    """A double sum of ``terms`` against math.fsum within count * 2^-53 * sum|x|."""
    t = np.asarray(terms, np.float64).reshape(-1)
    want, lim = math.fsum(t), len(t) * 2.0 ** -53 * math.fsum(np.abs(t))
    err = abs(float(got) - want)
    if rows is not None:
        rows.append(dict(case=case, tensor=tensor, err=err, e32=None, ratio=None, limit=lim))
    assert err <= lim, '%s %s: |%r - %r| = %.3e > %.3e' % (case, tensor, float(got), want, err, lim)


class RowFile(object):
    """``rows`` of the checks above that goes straight to a .jsonl file: a line is on disk before its assertion runs."""

    def __init__(self, path):
        self.path = path

    def append(self, row):
        os.makedirs(os.path.dirname(self.path), exist_ok=True)
        with open(self.path, 'a') as f:
            f.write(json.dumps(row) + '\n')


# ---------------------------------------------------------------------------------------------------- seeded inputs
def images(seed, B, C, H, W):
    """fp32 images in about [-1, 1]: smooth structure plus noise, so that every pyramid level carries signal."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.sin(yy[None, None] * g.uniform(0.05, 0.4, (B, C, 1, 1)) + xx[None, None] * g.uniform(0.05, 0.4, (B, C, 1, 1)))
    return (0.6 * base + 0.3 * g.standard_normal((B, C, H, W))).astype(np.float32)


SORT_KINDS = ('random', 'sorted', 'reversed', 'equal', 'duplicates', 'zeros', 'infinities', 'nans')


def sort_input(kind, seed, S, N):
    g = np.random.default_rng(seed)
    x = g.standard_normal((S, N)).astype(np.float32)
    if kind == 'sorted':
        x = np.sort(x, -1)
    elif kind == 'reversed':
        x = np.sort(x, -1)[:, ::-1].copy()
    elif kind == 'equal':
        x[:] = np.float32(1.5)
    elif kind == 'duplicates':
        x = g.integers(-3, 4, (S, N)).astype(np.float32)
    elif kind == 'zeros':
        x = np.where(g.random((S, N)) < 0.5, np.float32(0.0), -np.float32(0.0)).astype(np.float32)
        x[:, ::3] = g.standard_normal((S, len(range(0, N, 3)))).astype(np.float32)
    elif kind == 'infinities':
        x[g.random((S, N)) < 0.2] = np.inf
        x[g.random((S, N)) < 0.2] = -np.inf
    elif kind == 'nans':
        bits = x.view(np.uint32)
        bits[g.random((S, N)) < 0.05] = 0x7FC00000
        bits[g.random((S, N)) < 0.03] = 0xFFC00001
        bits[g.random((S, N)) < 0.02] = 0x7F800123
        x[g.random((S, N)) < 0.05] = np.inf
    return np.ascontiguousarray(x)
