"""Numpy float64 restatement of include/him.h "Seamless canvas composite" (helper module, not a conftest; it never imports
the package's kernels).

``dense_membrane`` solves the DEFINING equations with numpy.linalg.solve and is the authority.  ``transform_membrane``
restates the direct solver (closed-form bases, eigenvalue division) for shapes the dense solve cannot reach; its keyword
arguments ``dirichlet_everywhere`` / ``normalise`` / ``drop_corner`` / ``wrong_lambda`` -- and ``clamp`` of ``composite``
-- exist for the planted defects of tests/test_seamless_cpu.py: their defaults are the contract.  The matte is
composite_fixture's, not restated.

Bounds of ``compare`` (all derived, none measured):
  membrane  |m - m64| <= 2^-23 max|g|: m is stored in fp32 and |m| <= max|g| by the discrete maximum principle, so its
            rounding is at most 2^-24 max|g|; doubled for the fp64 solve's own error.
  residual  of the defining equations, evaluated in float64 on the stored fp32 membrane: <= 8 2^-24 max|g| (deg <= 4
            roundings of the centre plus one per neighbour).
  ring      m == float32(g) bit for bit.
  canvas    outside the window, on the ring and where alpha == 0: the input's bits.  alpha == 1: |canvas - v64| <=
            4 2^-24 with v64 = clamp(P + m64, 0, 1): 2 2^-24 from m (max|g| <= 1 for canvases in [0,1]), the fp32 add and the
            clamp at most 2^-24, one to spare.  0 < alpha < 1: composite_fixture's bound max(8 e32, 16 2^-24) max|c64| plus
            alpha 3 2^-24 for v's own error above."""
import numpy as np

import composite_fixture as cf

LINEAR, SMOOTH = cf.LINEAR, cf.SMOOTH
EPS32 = 2.0 ** -24
NO_SIDE = 1
MAX_N = 2048


def sides(Hc, Wc, x0, y0, H, W):
    """(l, r, t, b): a side is counted when canvas lies beyond it."""
    return int(x0 > 0), int(x0 + W < Wc), int(y0 > 0), int(y0 + H < Hc)


def sides_mask(flags):
    l, r, t, b = flags
    return l | r << 1 | t << 2 | b << 3


def interior(H, W, flags):
    l, r, t, b = flags
    return slice(t, H - b), slice(l, W - r)


def ring_mask(H, W, flags):
    m = np.ones((H, W), bool)
    m[interior(H, W, flags)] = False
    return m


def window_for(ny, nx, flags, margin=3):
    """(Hc, Wc, x0, y0, H, W) of a window whose interior is ny x nx and whose counted sides are ``flags``."""
    l, r, t, b = flags
    H, W = ny + t + b, nx + l + r
    x0, y0 = (margin if l else 0), (margin if t else 0)
    return y0 + H + (margin if b else 0), x0 + W + (margin if r else 0), x0, y0, H, W


ALL_SIDE_SETS = [(s & 1, s >> 1 & 1, s >> 2 & 1, s >> 3 & 1) for s in range(1, 16)]


# ------------------------------------------------------------------------------------------------- defining equations
def _neighbour_sum(m):
    """(sum of the 4-neighbours inside the plane, their number) per pixel of (..., H, W)."""
    s, deg = np.zeros_like(m), np.zeros(m.shape[-2:], np.float64)
    s[..., 1:, :] += m[..., :-1, :]
    deg[1:, :] += 1
    s[..., :-1, :] += m[..., 1:, :]
    deg[:-1, :] += 1
    s[..., :, 1:] += m[..., :, :-1]
    deg[:, 1:] += 1
    s[..., :, :-1] += m[..., :, 1:]
    deg[:, :-1] += 1
    return s, deg


def residual(m, flags):
    """deg(p) m(p) - sum of m over N(p), at the interior pixels of a window plane (..., H, W) whose ring holds g: the
    defining equations say 0."""
    m = np.asarray(m, np.float64)
    s, deg = _neighbour_sum(m)
    H, W = m.shape[-2:]
    iy, ix = interior(H, W, flags)
    return (deg * m - s)[..., iy, ix]


def dense_membrane(g, flags):
    """The authority: g (..., H, W) float64, read on the ring only -> m (..., H, W) with m = g on the ring and the
    solution of the defining equations inside; no side counted: zeros."""
    g = np.asarray(g, np.float64)
    H, W = g.shape[-2:]
    if not any(flags):
        return np.zeros_like(g)
    ring = ring_mask(H, W, flags)
    iy, ix = interior(H, W, flags)
    ny, nx = iy.stop - iy.start, ix.stop - ix.start
    idx = -np.ones((H, W), np.int64)
    idx[iy, ix] = np.arange(ny * nx).reshape(ny, nx)
    A = np.zeros((ny * nx, ny * nx))
    rhs = np.zeros(g.shape[:-2] + (ny * nx,))
    for y in range(iy.start, iy.stop):
        for x in range(ix.start, ix.stop):
            p = idx[y, x]
            for qy, qx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if not (0 <= qy < H and 0 <= qx < W):
                    continue                                  # beyond an uncounted side: the neighbour does not exist
                A[p, p] += 1
                if ring[qy, qx]:
                    rhs[..., p] += g[..., qy, qx]
                else:
                    A[p, idx[qy, qx]] -= 1
    sol = np.linalg.solve(A, rhs.reshape(-1, ny * nx).T).T.reshape(g.shape[:-2] + (ny, nx))
    m = np.where(ring, g, 0.0)
    m[..., iy, ix] = sol
    return m


# ---------------------------------------------------------------------------------------------------- direct solver
def second_difference(n, lo, hi):
    """The 1-D operator of the defining equations on n interior pixels: 2 on the diagonal, 1 at a Neumann end."""
    L = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    if not lo:
        L[0, 0] -= 1
    if not hi:
        L[n - 1, n - 1] -= 1
    return L


def basis(n, lo, hi, normalise=True):
    """(V (n,n), lam (n,)) of the boundary pair (lo, hi): the table of include/him.h."""
    j, k = np.mgrid[0:n, 0:n].astype(np.float64)
    kk = np.arange(n, dtype=np.float64)
    if lo and hi:
        V, lam = np.sin(np.pi * (k + 1) * (j + 1) / (n + 1)), 2 - 2 * np.cos(np.pi * (kk + 1) / (n + 1))
    elif not lo and not hi:
        V, lam = np.cos(np.pi * k * (2 * j + 1) / (2 * n)), 2 - 2 * np.cos(np.pi * kk / n)
    else:
        jj = (j + 1) if lo else (n - j)
        V, lam = np.sin(np.pi * (2 * k + 1) * jj / (2 * n + 1)), 2 - 2 * np.cos(np.pi * (2 * kk + 1) / (2 * n + 1))
    if normalise:
        V = V / np.sqrt((V * V).sum(0, keepdims=True))
    return V, lam


def transform_membrane(g, flags, dirichlet_everywhere=False, normalise=True, drop_corner=False, wrong_lambda=False):
    """The direct solver in float64: m = Vy (Bh / (lamy_i + lamx_j)) Vx^T, Bh = Vy^T B Vx."""
    g = np.asarray(g, np.float64)
    H, W = g.shape[-2:]
    if not any(flags):
        return np.zeros_like(g)
    l, r, t, b = flags
    iy, ix = interior(H, W, flags)
    ny, nx = iy.stop - iy.start, ix.stop - ix.start
    B = np.zeros(g.shape[:-2] + (ny, nx))
    if t:
        B[..., 0, :] += g[..., 0, ix]
    if b:
        B[..., ny - 1, :] += g[..., H - 1, ix]
    if drop_corner:                                            # the columns overwrite what the rows left in the corners
        if l:
            B[..., :, 0] = g[..., iy, 0]
        if r:
            B[..., :, nx - 1] = g[..., iy, W - 1]
    else:
        if l:
            B[..., :, 0] += g[..., iy, 0]
        if r:
            B[..., :, nx - 1] += g[..., iy, W - 1]
    py, px = ((1, 1), (1, 1)) if dirichlet_everywhere else ((t, b), (l, r))
    Vy, lamy = basis(ny, *py, normalise=normalise)
    Vx, lamx = basis(nx, *px, normalise=normalise)
    if wrong_lambda:
        lamx = basis(nx, *((0, 0) if tuple(px) == (1, 1) else (1, 1)))[1]
    Bh = Vy.T @ B @ Vx
    sol = Vy @ (Bh / (lamy[:, None] + lamx[None, :])) @ Vx.T
    m = np.where(ring_mask(H, W, flags), g, 0.0)
    m[..., iy, ix] = sol
    return m


def boundary_values(O, P, x0, y0):
    """g = O - P over the window in float64 (read on the ring only) of O (3,Hc,Wc) and P (3,H,W) float32."""
    H, W = P.shape[-2:]
    return O[:, y0:y0 + H, x0:x0 + W].astype(np.float64) - P.astype(np.float64)


def membrane(O, P, x0, y0, method=None):
    """m64 (3,H,W) and max|g| over the ring.  ``method``: 'dense', 'transform' or None (dense while it is small)."""
    Hc, Wc = O.shape[-2:]
    H, W = P.shape[-2:]
    flags = sides(Hc, Wc, x0, y0, H, W)
    g = boundary_values(O, P, x0, y0)
    ring = ring_mask(H, W, flags)
    gmax = float(np.abs(g[:, ring]).max()) if ring.any() else 0.0
    if method is None:
        iy, ix = interior(H, W, flags)
        method = 'dense' if (iy.stop - iy.start) * (ix.stop - ix.start) <= 1400 else 'transform'
    m = dense_membrane(g, flags) if method == 'dense' else transform_membrane(g, flags)
    return m, gmax


# --------------------------------------------------------------------------------------------------------- composite
def alpha_of(Hc, Wc, x0, y0, H, W, feather, reach, dist2, profile, dtype):
    if feather is None:
        return np.ones((H, W), dtype)
    return cf.matte(Hc, Wc, x0, y0, H, W, feather, reach, dist2, profile, dtype)


def composite(O, P, m, x0, y0, alpha, dtype=np.float64, clamp=True):
    """The canvas (3,Hc,Wc) in ``dtype``: on the interior O + alpha (v - O), v = clamp(P + m, 0, 1) (alpha == 1: v,
    alpha == 0: O); the ring and everything outside the window keep O."""
    dt = np.dtype(dtype)
    Hc, Wc = O.shape[-2:]
    H, W = P.shape[-2:]
    flags = sides(Hc, Wc, x0, y0, H, W)
    out = O.astype(dt).copy()
    o = out[:, y0:y0 + H, x0:x0 + W]
    v = P.astype(dt) + np.asarray(m).astype(dt)
    if clamp:
        v = np.minimum(np.maximum(v, dt.type(0)), dt.type(1))
    a = np.asarray(alpha).astype(dt)[None]
    new = np.where(a == 1, v, np.where(a == 0, o, o + a * (v - o)))
    inside = ~ring_mask(H, W, flags)
    o[:, inside] = new[:, inside]
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(got_m, got_canvas, got_matte, O, P, x0, y0, feather=None, reach=0, dist2=None, profile=SMOOTH, m64=None,
            rows=None, case=''):
    """Every check of a seamless paste -> list of failures (empty: it is the contract's result).  ``got_m`` (3,H,W) fp32,
    ``got_canvas`` (3,Hc,Wc) fp32 or None (membrane only), ``got_matte`` (H,W) or None.  ``m64``: the float64 membrane
    (None: ``membrane``'s).  ``rows`` (a list) receives one dict per bounded tensor, before anything is judged."""
    bad = []
    Hc, Wc = O.shape[-2:]
    H, W = P.shape[-2:]
    flags = sides(Hc, Wc, x0, y0, H, W)
    ring = ring_mask(H, W, flags)
    inside = ~ring
    g = boundary_values(O, P, x0, y0)
    if m64 is None:
        m64, gmax = membrane(O, P, x0, y0)
    else:
        gmax = float(np.abs(g[:, ring]).max()) if ring.any() else 0.0
    gm = np.asarray(got_m).reshape(3, H, W)

    def row(tensor, error, limit, elements):
        if rows is not None:
            rows.append(dict(case=case, tensor=tensor, elements=int(elements), error=float(error), limit=float(limit),
                             ratio=(float(error) / float(limit) if limit > 0 else None)))
        if not error <= limit:
            bad.append('%s %s: error %.3e > limit %.3e' % (case, tensor, error, limit))

    if not np.isfinite(gm).all():
        bad.append('%s: membrane not finite' % case)
        return bad
    if not np.array_equal(_bits(gm)[:, ring], _bits(g.astype(np.float32))[:, ring]):
        bad.append('%s: membrane differs from float32(g) on the ring' % case)
    err = float(np.abs(gm.astype(np.float64) - m64)[:, inside].max())
    row('membrane', err, 2 * EPS32 * gmax, 3 * inside.sum())
    res = float(np.abs(residual(gm, flags)).max()) if any(flags) else 0.0
    row('residual', res, 8 * EPS32 * gmax, 3 * inside.sum())
    if got_canvas is None:
        return bad

    got = np.asarray(got_canvas).reshape(3, Hc, Wc)
    if not np.isfinite(got).all():
        bad.append('%s: canvas not finite' % case)
        return bad
    a64 = alpha_of(Hc, Wc, x0, y0, H, W, feather, reach, dist2, profile, np.float64)
    a32 = alpha_of(Hc, Wc, x0, y0, H, W, feather, reach, dist2, profile, np.float32)
    if feather is None:
        zero, one = np.zeros((H, W), bool), np.ones((H, W), bool)
    else:
        zero, one = cf.alpha_sets(Hc, Wc, x0, y0, H, W, feather, reach, dist2)
    if got_matte is not None:
        mt = np.asarray(got_matte).reshape(H, W)
        if not np.array_equal(mt == 0, zero) or not np.array_equal(mt == 1, one):
            bad.append('%s: the sets {alpha == 0} / {alpha == 1} differ from the integer decisions' % case)
        mid = ~zero & ~one
        e32 = cf.rel_err(a32[mid], a64[mid])
        row('matte', cf.rel_err(mt[mid], a64[mid]), max(cf.FACTOR * e32, cf.FLOOR), mid.sum())
    keep = np.ones((Hc, Wc), bool)
    keep[y0:y0 + H, x0:x0 + W] = ring | zero
    if not np.array_equal(_bits(got)[:, keep], _bits(O)[:, keep]):
        bad.append('%s: canvas changed outside the window, on the ring or where alpha == 0' % case)
    gw = got[:, y0:y0 + H, x0:x0 + W].astype(np.float64)
    c64 = composite(O, P, m64, x0, y0, a64, np.float64)[:, y0:y0 + H, x0:x0 + W]
    full = inside & one
    if full.any():
        row('canvas_alpha1', np.abs(gw - c64)[:, full].max(), 4 * EPS32, 3 * full.sum())
    mid = inside & ~zero & ~one
    if mid.any():
        c32 = composite(O, P, m64.astype(np.float32), x0, y0, a32, np.float32)[:, y0:y0 + H, x0:x0 + W]
        e32 = cf.rel_err(c32[:, mid], c64[:, mid])
        scale = float(np.abs(c64[:, mid]).max())
        slack = (np.abs(gw - c64) - a64[None] * 3 * EPS32)[:, mid].max()
        row('canvas_ramp', max(float(slack), 0.0), max(cf.FACTOR * e32, cf.FLOOR) * scale, 3 * mid.sum())
    return bad
