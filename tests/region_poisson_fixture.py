"""Numpy float64 restatement of include/him.h "Region Poisson clone" (helper module, not a conftest; it never imports the
package's kernels).

``system`` assembles the DEFINING equations of the correction u = f - P as a dense float64 matrix, ``dense`` solves them
with numpy.linalg.solve and is the authority.  ``cg`` restates conjugate gradients and returns its iteration count.  The
keyword arguments ``omega_extra`` / ``all_dirichlet`` / ``deg4`` / ``no_abs`` of ``system`` and ``clamp`` of ``composite``
exist for the planted defects of tests/test_region_poisson_cpu.py: their defaults are the contract.

Bounds of ``compare`` (all derived, none measured).  A (n x n) and b are the fixture's, u_d the result under test on
Omega, u* the dense solve, e64 = 2^-53, e32 = 2^-24, lam = the smallest eigenvalue of A (eigvalsh), K the iterations the
status reports, per channel:

  eval      a residual b - A u evaluated in float64: a row has at most 5 integer coefficients of magnitude <= 4 (their
            products are exact), so at most 6 additions: <= 6 e64 (8 max|u| + max|b|) per row; taken as
            16 e64 (8 max|u| + max|b|) sqrt(n) in the 2-norm.
  u         ||u_d - u*||_inf <= ||u_d - u*||_2 <= ||A^-1|| ||A (u_d - u*)||_2 <= (||r_true||_2 + ||r_dense||_2 + 2 eval) / lam
            with r_true = b - A u_d and r_dense = b - A u* (the dense solve's own error enters through its residual).
  residual  the solver stops on its RECURSIVE residual r_K with ||r_K|| <= rtol ||b||; r_true differs from it by the
            drift g_K = (b - A u_K) - r_K.  One step rounds u_{k+1} = fma(alpha, p, u_k) (|du| <= e64 |u_{k+1}|) and
            r_{k+1} = fma(-alpha, Ap, r_k) (<= e64 |r_{k+1}|) with Ap carrying at most 6 e64 (|A||p|) per row, so
            ||g_{k+1}|| <= ||g_k|| + e64 (||A|| ||u_{k+1}|| + ||r_{k+1}|| + 6 ||A|| ||alpha p||).  ||A|| <= 8;
            with U >= every ||u_k||_2 and >= ||u*||_2: ||alpha p|| = ||u_{k+1} - u_k|| <= 2 U and
            ||r_{k+1}|| <= ||A|| (||u*|| + ||u_{k+1}||) + ||g|| ~ 16 U: 120 e64 U per step.  CG from u_0 = 0 decreases the
            energy norm of the error, so ||u_k||_A <= 2 ||u*||_A and U = 2 sqrt(u* . b / lam) serves.  g_0 is the
            difference of two float64 evaluations of b (at most 8 terms of magnitude <= 2 per row, any order):
            <= 128 e64 sqrt(n).  Hence ||r_true||_2 <= rtol ||b||_2 + e64 (120 K U + 128 sqrt(n)) + eval.
  canvas    |canvas - clamp(P + u*)| <= the bound of u + e32 max|P + u*| (the one fp32 rounding of the final sum; the
            clamp is 1-Lipschitz); outside Omega the canvas keeps the input's bits; u is exactly 0 outside Omega."""
import numpy as np

import seamless_fixture as sf

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
EMPTY, SINGULAR, MAX_ITER_HIT, NONFINITE = 1, 2, 4, 8
MAX_N = 2048
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1))          # up, down, left, right


def default_cap(H, W):
    return 6 * (H + W)


def omega_of(region, flags):
    """(Omega (H,W) bool, region pixels dropped on the ring)."""
    R = np.asarray(region) != 0
    ring = sf.ring_mask(R.shape[0], R.shape[1], flags)
    return R & ~ring, int((R & ring).sum())


def system(O, P, x0, y0, region, mixed=False, omega_extra=None, all_dirichlet=False, deg4=False, no_abs=False):
    """The equations of the correction: dict(A (n,n), b (3,n), omega (H,W) bool, idx (H,W), flags, dropped, singular)."""
    Hc, Wc = O.shape[-2:]
    H, W = P.shape[-2:]
    flags = sf.sides(Hc, Wc, x0, y0, H, W)
    om, dropped = omega_of(region, (1, 1, 1, 1) if all_dirichlet else flags)
    if omega_extra is not None:
        om = om | omega_extra
    O64 = O[:, y0:y0 + H, x0:x0 + W].astype(np.float64)
    P64 = P.astype(np.float64)
    n = int(om.sum())
    idx = -np.ones((H, W), np.int64)
    idx[om] = np.arange(n)
    A, b = np.zeros((n, n)), np.zeros((3, n))
    for y, x in np.argwhere(om):
        p = idx[y, x]
        for dy, dx in NEIGHBOURS:
            qy, qx = y + dy, x + dx
            if not (0 <= qy < H and 0 <= qx < W):
                if deg4:
                    A[p, p] += 1
                continue                                       # beyond an uncounted side: the neighbour does not exist
            A[p, p] += 1
            if om[qy, qx]:
                A[p, idx[qy, qx]] -= 1
            else:
                b[:, p] += O64[:, qy, qx] - P64[:, qy, qx]
            if mixed:
                dO, dP = O64[:, y, x] - O64[:, qy, qx], P64[:, y, x] - P64[:, qy, qx]
                take = (dO > dP) if no_abs else (np.abs(dO) > np.abs(dP))      # strictly: ties take the patch
                b[:, p] += np.where(take, dO - dP, 0.0)
    return dict(A=A, b=b, omega=om, idx=idx, flags=flags, dropped=dropped, n=n, H=H, W=W,
                singular=bool(n == H * W and not any(flags)))


def scatter(s, v):
    """(3,n) values on Omega -> (3,H,W) planes, 0 elsewhere."""
    out = np.zeros((3, s['H'], s['W']))
    out[:, s['omega']] = v
    return out


def dense(s):
    """The authority: u (3,H,W) float64, 0 outside Omega; the singular system and the empty set give zeros."""
    if s['n'] == 0 or s['singular']:
        return np.zeros((3, s['H'], s['W']))
    return scatter(s, np.linalg.solve(s['A'], s['b'].T).T)


def cg(s, rtol, max_iter=None):
    """Conjugate gradients as the library runs them (u_0 = 0, stop r.r <= rtol^2 b.b per channel, b.b == 0: no step)
    -> (u (3,H,W), iterations per channel)."""
    A = s['A']
    cap = default_cap(s['H'], s['W']) if max_iter is None else max_iter
    out, its = np.zeros((3, s['n'])), []
    for c in range(3):
        b = s['b'][c]
        u, r, p = np.zeros_like(b), b.copy(), b.copy()
        rr, bb, k = float(b @ b), float(b @ b), 0
        while k < cap and not rr <= rtol * rtol * bb and not s['singular']:
            Ap = A @ p
            pap = float(p @ Ap)
            if not pap > 0:
                break
            alpha = rr / pap
            u, r = u + alpha * p, r - alpha * Ap
            new = float(r @ r)
            p, rr, k = r + (new / rr) * p, new, k + 1
        out[c] = u
        its.append(k)
    return scatter(s, out), its


def composite(O, P, u, x0, y0, omega, clamp=True, dtype=np.float64):
    """The canvas (3,Hc,Wc): clamp(P + u, 0, 1) on Omega, O everywhere else."""
    H, W = P.shape[-2:]
    out = O.astype(dtype).copy()
    v = P.astype(np.float64) + u
    if clamp:
        v = np.minimum(np.maximum(v, 0.0), 1.0)
    win = out[:, y0:y0 + H, x0:x0 + W]
    win[:, omega] = v[:, omega].astype(dtype)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(got_u, got_canvas, got_status, O, P, x0, y0, region, mixed, rtol, s=None, u64=None, rows=None, case=''):
    """Every check of a region clone that is expected to have converged -> list of failures (empty: the contract's
    result).  ``got_u`` (3,H,W) float64, ``got_canvas`` (3,Hc,Wc) float32 or None, ``got_status`` the 8 ints.  ``s`` /
    ``u64``: ``system`` / ``dense`` of the same inputs when the caller has them.  ``rows`` (a list) receives one dict per
    bounded quantity, before anything is judged."""
    bad = []
    s = system(O, P, x0, y0, region, mixed) if s is None else s
    u64 = dense(s) if u64 is None else u64
    om, n, H, W = s['omega'], s['n'], s['H'], s['W']
    gu = np.asarray(got_u, np.float64).reshape(3, H, W)
    st = [int(v) for v in got_status]

    def row(tensor, error, limit):
        if rows is not None:
            rows.append(dict(case=case, tensor=tensor, error=float(error), limit=float(limit),
                             ratio=(float(error) / float(limit) if limit > 0 else None)))
        if not error <= limit:
            bad.append('%s %s: error %.3e > limit %.3e' % (case, tensor, error, limit))

    want_flags = (EMPTY if n == 0 else 0) | (SINGULAR if s['singular'] else 0)
    if st[:3] != [sf.sides_mask(s['flags']), n, s['dropped']] or st[4] != want_flags or st[5:] != [0, 0, 0]:
        bad.append('%s: status %s, expected [%d, %d, %d, K, %d, 0, 0, 0]' % (case, st, sf.sides_mask(s['flags']), n,
                                                                             s['dropped'], want_flags))
    if not np.isfinite(gu).all():
        bad.append('%s: u not finite' % case)
        return bad
    if gu[:, ~om].any():
        bad.append('%s: u is not 0 outside Omega' % case)
    ubound = np.zeros(3)
    if n and not s['singular']:
        A, b = s['A'], s['b']
        lam = float(np.linalg.eigvalsh(A)[0])
        ud, us = gu[:, om], u64[:, om]
        r_true, r_dense = b - ud @ A, b - us @ A
        K = st[3]
        for c in range(3):
            ev = 16 * EPS64 * (8 * max(np.abs(ud[c]).max(), np.abs(us[c]).max()) + np.abs(b[c]).max()) * np.sqrt(n)
            U = 2 * np.sqrt(max(float(us[c] @ b[c]), 0.0) / lam)
            drift = EPS64 * (120 * K * U + 128 * np.sqrt(n))
            nr = float(np.linalg.norm(r_true[c]))
            row('residual[%d]' % c, nr, rtol * float(np.linalg.norm(b[c])) + drift + ev)
            ubound[c] = (nr + float(np.linalg.norm(r_dense[c])) + 2 * ev) / lam
            row('u[%d]' % c, np.abs(ud[c] - us[c]).max(), ubound[c])
    elif gu.any():
        bad.append('%s: u must be 0 (empty or singular system)' % case)
    if got_canvas is None:
        return bad
    got = np.asarray(got_canvas)
    Hc, Wc = O.shape[-2:]
    if not np.isfinite(got).all():
        bad.append('%s: canvas not finite' % case)
        return bad
    keep = np.ones((Hc, Wc), bool)
    keep[y0:y0 + H, x0:x0 + W] = ~om
    if not np.array_equal(_bits(got)[:, keep], _bits(O)[:, keep]):
        bad.append('%s: canvas changed outside Omega' % case)
    if n:
        want = composite(O, P, u64, x0, y0, om)[:, y0:y0 + H, x0:x0 + W]
        gw = got[:, y0:y0 + H, x0:x0 + W].astype(np.float64)
        v = P.astype(np.float64) + u64
        for c in range(3):
            row('canvas[%d]' % c, np.abs(gw[c] - want[c])[om].max(), ubound[c] + EPS32 * np.abs(v[c][om]).max())
    return bad


# ----------------------------------------------------------------------------------------------- hand-written answers
def hand_cases():
    """5 x 7 windows whose corrections are written down by hand -> [(name, O, P, x0, y0, region, mixed, {(y, x): u (3,)})].
    Every value is a multiple of 1/64 below 1/2, so O = P + G is exact in fp32 and G = O - P exact in float64.
    Every system has lam >= 2 (diagonal >= 2 more than the off-diagonal row sum, or a 1 x 1 system) and ||b||_2 <= 4, so a
    solve to rtol is within rtol ||b|| / lam <= 2 rtol of these answers (plus float64 rounding: HAND_SLACK)."""
    H, W, Hc, Wc = 5, 7, 9, 11
    g = np.random.default_rng(7)
    P = (g.integers(0, 32, size=(3, H, W)) / 64.0).astype(np.float32)
    G = (g.integers(1, 32, size=(3, H, W)) / 64.0)
    Obase = (g.integers(0, 64, size=(3, Hc, Wc)) / 64.0).astype(np.float32)

    def photo(x0, y0, win):
        O = Obase.copy()
        O[:, y0:y0 + H, x0:x0 + W] = win.astype(np.float32)
        return O

    def reg(*pix):
        R = np.zeros((H, W), np.uint8)
        for y, x in pix:
            R[y, x] = 1
        return R

    cases = []
    O = photo(2, 2, P + G)
    # one pixel, four Dirichlet neighbours: 4 u = the sum of G over them
    cases.append(('one_pixel', O, P, 2, 2, reg((2, 3)), False,
                  {(2, 3): (G[:, 1, 3] + G[:, 3, 3] + G[:, 2, 2] + G[:, 2, 4]) / 4}))
    # two neighbours a = (2,3), b = (2,4): 4 ua - ub = sa, 4 ub - ua = sb  ->  ua = (4 sa + sb) / 15, ub = (sa + 4 sb) / 15
    sa, sb = G[:, 1, 3] + G[:, 3, 3] + G[:, 2, 2], G[:, 1, 4] + G[:, 3, 4] + G[:, 2, 5]
    cases.append(('two_pixels', O, P, 2, 2, reg((2, 3), (2, 4)), False,
                  {(2, 3): (4 * sa + sb) / 15, (2, 4): (sa + 4 * sb) / 15}))
    # the window in the canvas corner: top and left are not counted (Neumann).  (0,3) has three neighbours, the corner
    # pixel (0,0) two; they do not touch each other
    O = photo(0, 0, P + G)
    cases.append(('canvas_corner', O, P, 0, 0, reg((0, 3), (0, 0)), False,
                  {(0, 3): (G[:, 1, 3] + G[:, 0, 2] + G[:, 0, 4]) / 3, (0, 0): (G[:, 1, 0] + G[:, 0, 1]) / 2}))
    # mixed, a flat patch: every pair takes the photograph's gradient (a zero gradient ties and takes the patch's, also
    # zero), so 4 f(p) - sum O(q) = sum (O(p) - O(q)): f(p) = O(p), u = O(p) - P(p)
    flat = np.full((3, H, W), 0.5, np.float32)
    O = photo(2, 2, P + G)
    cases.append(('mixed_flat_patch', O, flat, 2, 2, reg((2, 3)), True,
                  {(2, 3): O[:, 4, 5].astype(np.float64) - 0.5}))
    return cases


HAND_SLACK = 64 * EPS64


# ---------------------------------------------------------------------------------------------------- seeded builders
def blob_region(H=37, W=53):
    """A blob with a hole, a separate island, a one-pixel-wide spur, and pixels on the window's four borders (whichever
    of them is a counted side drops them, the others keep them)."""
    y, x = np.mgrid[0:H, 0:W]
    R = ((y - 17) / 11.0) ** 2 + ((x - 20) / 15.0) ** 2 <= 1.0
    R &= ~(((y - 16) / 3.0) ** 2 + ((x - 18) / 4.0) ** 2 <= 1.0)          # the hole
    R |= ((y - 28) / 4.0) ** 2 + ((x - 45) / 5.0) ** 2 <= 1.0             # the island
    R[17, 35:50] = True                                                   # the spur, one pixel wide
    R[0:7, 20] = True                                                     # up to the top border
    R[17, 0:6] = True                                                     # to the left border
    R[28:H, 45] = True                                                    # down to the bottom border
    R[28, 45:W] = True                                                    # to the right border
    return R.astype(np.uint8)


def band_region(H=67, W=261, half=3.6):
    """A diagonal band from corner to corner: crosses the 64-column tiles, the 4-row chunks and column 256."""
    y, x = np.mgrid[0:H, 0:W]
    return (np.abs(y - x * (H - 1.0) / (W - 1.0)) <= half).astype(np.uint8)


def scene(seed, Hc, Wc, H, W, quant=True):
    """(O (3,Hc,Wc), P (3,H,W)) float32 in [0,1]; P on byte / 255 values as a paste writes them."""
    g = np.random.default_rng(seed)
    O = g.random((3, Hc, Wc), dtype=np.float32)
    P = (g.integers(0, 256, size=(3, H, W)) / np.float32(255)).astype(np.float32) if quant \
        else g.random((3, H, W), dtype=np.float32)
    return O, P
