"""Numpy restatement of include/him.h "Feathered canvas composite" (helper module, not a conftest; it never imports the
package's kernels).  The matte's DECISIONS (which window side counts, inside / outside a ramp) are integer comparisons
and come out as exact sets; the values strictly inside a ramp and the blended canvas are computed in ``dtype``: float64
is the reference, float32 (every operation rounded on its own, the kernel's order) the yardstick whose own error e32
sizes the bound max(8 * e32, 16 * 2^-24) of tests/README.md.  Squared distances come from edt_fixture's brute force.  P,
the value the hard paste writes, is an INPUT here: the tests take it from the existing paste.

The keyword arguments ``sides`` / ``combine`` / ``metric`` / ``use_reach`` / ``wrap32`` exist for the planted defects of
tests/test_composite_cpu.py: their defaults are the contract."""
import numpy as np

import edt_fixture

LINEAR, SMOOTH = 0, 1
PROFILES = {'linear': LINEAR, 'smooth': SMOOTH}
NONE = edt_fixture.NONE
FACTOR, FLOOR = 8.0, 16 * 2.0 ** -24
NO_SIDE = 2 ** 40                       # d_b where no window side has canvas behind it


def changed(before, after, x0, y0, H, W):
    """him_canvas_changed: (H,W) uint8 of two (Hc,Wc) id planes."""
    return (before[y0:y0 + H, x0:x0 + W] != after[y0:y0 + H, x0:x0 + W]).astype(np.uint8)


def dist2_of(changed_plane, metric='euclid'):
    """him_edt under HIM_EDT_NONZERO over the changed plane: int32 (H,W), NONE everywhere without a changed pixel."""
    return edt_fixture.edt(np.asarray(changed_plane) != 0, metric=metric)[0]


def border_distance(Hc, Wc, x0, y0, H, W, sides='inner'):
    """int64 (H,W): d_b, the minimum over the window sides that are NOT on the canvas edge (``sides='all'``: over all
    four, the planted defect) of the pixel's distance to the first pixel outside; NO_SIDE where no side counts."""
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    d = np.full((H, W), NO_SIDE, np.int64)
    every = sides == 'all'
    if every or x0 > 0:
        d = np.minimum(d, x + 1)
    if every or x0 + W < Wc:
        d = np.minimum(d, W - x)
    if every or y0 > 0:
        d = np.minimum(d, y + 1)
    if every or y0 + H < Hc:
        d = np.minimum(d, H - y)
    return d


def _wrap32(v):
    return int(np.int64(v).astype(np.int32))


def _terms(Hc, Wc, x0, y0, H, W, feather, reach, dist2, dtype, sides='inner', use_reach=True, wrap32=False):
    """(t_b, t_o) in ``dtype`` and, per term, the integer decisions (is0, is1) they were built from."""
    dt = np.dtype(dtype).type
    db = border_distance(Hc, Wc, x0, y0, H, W, sides)
    tb = np.ones((H, W), dt)
    ramp = db < feather
    tb[ramp] = db[ramp].astype(dt) / dt(feather)
    b0, b1 = np.zeros((H, W), bool), ~ramp
    to = np.ones((H, W), dt)
    o0, o1 = np.zeros((H, W), bool), np.ones((H, W), bool)
    if dist2 is not None:
        d2 = np.asarray(dist2).astype(np.int64).reshape(H, W)
        r = reach if use_reach else 0
        r2, out2 = r * r, (r + feather) * (r + feather)
        if wrap32:                      # the squares held in 32-bit words
            r2, out2 = _wrap32(r2), _wrap32(out2)
        o1 = (d2 != NONE) & (d2 <= r2)
        o0 = (d2 == NONE) | ((d2 >= out2) & ~o1)
        mid = ~o0 & ~o1
        to[o0] = 0
        to[mid] = dt(1) - (np.sqrt(d2[mid].astype(dt)) - dt(r)) / dt(feather)
    return tb, to, (b0, b1), (o0, o1)


def matte(Hc, Wc, x0, y0, H, W, feather, reach=0, dist2=None, profile=SMOOTH, dtype=np.float64, combine='min', **defects):
    """alpha (H,W) in ``dtype``."""
    dt = np.dtype(dtype).type
    tb, to, _, _ = _terms(Hc, Wc, x0, y0, H, W, feather, reach, dist2, dtype, **defects)
    t = np.minimum(tb, to) if combine == 'min' else tb * to
    if profile == SMOOTH:
        t = (t * t) * (dt(3) - dt(2) * t)
    return t.astype(dt)


def alpha_sets(Hc, Wc, x0, y0, H, W, feather, reach=0, dist2=None):
    """The exact sets ({alpha == 0}, {alpha == 1}) as bool (H,W), from the integer decisions alone (either profile)."""
    _, _, (b0, b1), (o0, o1) = _terms(Hc, Wc, x0, y0, H, W, feather, reach, dist2, np.float64)
    return b0 | o0, b1 & o1


def composite(O, P, x0, y0, alpha, dtype=np.float64):
    """The canvas (3,Hc,Wc) in ``dtype`` after the blended paste of P (3,H,W) over O (3,Hc,Wc) with alpha (H,W):
    alpha == 1 -> P, alpha == 0 -> O, otherwise O + alpha * (P - O)."""
    dt = np.dtype(dtype)
    H, W = alpha.shape
    out = O.astype(dt).copy()
    o = out[:, y0:y0 + H, x0:x0 + W]
    p = P.astype(dt)
    a = alpha.astype(dt)[None]
    o[...] = np.where(a == 1, p, np.where(a == 0, o, o + a * (p - o)))
    return out


def max_step(canvas):
    """The largest difference between 4-neighbours of a (C,H,W) canvas."""
    c = np.asarray(canvas, np.float64)
    dx = np.abs(np.diff(c, axis=2)).max() if c.shape[2] > 1 else 0.0
    dy = np.abs(np.diff(c, axis=1)).max() if c.shape[1] > 1 else 0.0
    return float(max(dx, dy))


def rel_err(got, ref):
    """Maximum error over the maximum of |ref| (tests/README.md); 0 for an empty selection."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    err = np.abs(got - ref)
    if not np.isfinite(err).all():
        return float('inf')
    return float(err.max()) / max(float(np.abs(ref).max()), 1e-30)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(got_canvas, got_matte, O, P, Hc, Wc, x0, y0, H, W, feather, reach=0, dist2=None, profile=SMOOTH, rows=None,
            case=''):
    """Every check of a blended paste -> list of failures (empty: it is the contract's result).  The sets {alpha == 0} and
    {alpha == 1} equal the integer decisions'; on them the canvas is O / P bit for bit; outside the window it is O bit for
    bit; elsewhere matte and canvas are within max(8 * e32, 16 * 2^-24) of float64.  ``got_matte`` may be None.  ``rows``
    (a list) receives one dict per bounded tensor, before anything is judged."""
    bad = []
    zero, one = alpha_sets(Hc, Wc, x0, y0, H, W, feather, reach, dist2)
    a64 = matte(Hc, Wc, x0, y0, H, W, feather, reach, dist2, profile, np.float64)
    a32 = matte(Hc, Wc, x0, y0, H, W, feather, reach, dist2, profile, np.float32)
    assert np.array_equal(a64 == 0, zero) and np.array_equal(a64 == 1, one), 'fixture: sets and values disagree'
    mid = ~zero & ~one
    checks = []
    if got_matte is not None:
        gm = np.asarray(got_matte).reshape(H, W)
        if not np.array_equal(gm == 0, zero):
            bad.append('%s: {alpha == 0} differs at %d pixels' % (case, int(((gm == 0) != zero).sum())))
        if not np.array_equal(gm == 1, one):
            bad.append('%s: {alpha == 1} differs at %d pixels' % (case, int(((gm == 1) != one).sum())))
        checks.append(('matte', gm[mid], a64[mid], a32[mid]))
    got = np.asarray(got_canvas)
    win = np.zeros((Hc, Wc), bool)
    win[y0:y0 + H, x0:x0 + W] = True
    if not np.array_equal(_bits(got)[:, ~win], _bits(O)[:, ~win]):
        bad.append('%s: canvas changed outside the window' % case)
    gw = got[:, y0:y0 + H, x0:x0 + W]
    if not np.array_equal(_bits(gw)[:, zero], _bits(O[:, y0:y0 + H, x0:x0 + W])[:, zero]):
        bad.append('%s: canvas differs from the original where alpha == 0' % case)
    if not np.array_equal(_bits(gw)[:, one], _bits(P)[:, one]):
        bad.append('%s: canvas differs from the hard paste where alpha == 1' % case)
    c64 = composite(O, P, x0, y0, a64, np.float64)[:, y0:y0 + H, x0:x0 + W]
    c32 = composite(O, P, x0, y0, a32, np.float32)[:, y0:y0 + H, x0:x0 + W]
    checks.append(('canvas', gw[:, mid], c64[:, mid], c32[:, mid]))
    for name, g, r64, r32 in checks:
        err, e32 = rel_err(g, r64), rel_err(r32, r64)
        limit = max(FACTOR * e32, FLOOR)
        if rows is not None:
            rows.append(dict(case=case, tensor=name, elements=int(np.asarray(r64).size), error=err, e32=e32,
                             ratio=(err / e32 if e32 > 0 else None), limit=limit))
        if not err <= limit:
            bad.append('%s %s: error %.3e > limit %.3e (e32 %.3e)' % (case, name, err, limit, e32))
    return bad
