"""Restatement of include/him.h "Boundary-weighted and surface losses" in plain torch (helper module, not a conftest; it
never imports the package's kernels).  Distances come from tests/edt_fixture.py: its brute-force transform on small
planes, and an exact separable one here for planes the brute force cannot hold (the CPU tests compare the two).  Every
loss takes ``dtype``: float64 is the reference, float32 the yard-stick whose own error against float64 sets the bound
of the GPU tests (abi_harness.Bound.limit).  The keyword arguments ``denominator`` / ``exponent`` / ``none`` /
``phi_sign`` / ``use_gate`` exist for the planted defects of tests/test_boundary_loss_cpu.py: their defaults are the
contract."""
import math

import numpy as np
import torch

import edt_fixture as ef

NONE = ef.NONE
F32, F64 = torch.float32, torch.float64
AMP_SIGMA = [(0.0, 5.0), (4.0, 1.0), (10.0, 0.5), (1.0, 1000.0)]
SHAPES = [(1, 1), (1, 9), (7, 5), (17, 33), (64, 64), (96, 160)]
BRUTE_MAX = 2500          # edt_fixture's own limit on the pixels of a plane


# -------------------------------------------------------------------------------------------------------- distances
def edt_separable(seed):
    """Exact squared distances (int32 (H,W)) of a boolean seed plane: the nearest seed of every row first, then the
    minimum over rows of (y - y')^2 + that.  O(H W (H + W)) cells of int64, no approximation."""
    H, W = seed.shape
    if not seed.any():
        return np.full((H, W), NONE, np.int32)
    big = np.int64(1) << 40
    xs = np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2                                   # [x, x']
    row = np.where(seed[:, None, :], dx2[None], big).min(-1)                # [y', x]
    ys = np.arange(H, dtype=np.int64)
    dy2 = (ys[:, None] - ys[None, :]) ** 2                                   # [y, y']
    return (dy2[:, :, None] + row[None]).min(1).astype(np.int32)


def edt_plane(seed):
    return ef.edt(seed)[0] if seed.size <= BRUTE_MAX else edt_separable(seed)


def boundary_d2(planes):
    """int32 (B,H,W): one HIM_EDT_ANY_BOUNDARY job per sample over the whole id plane (B,H,W) or (B,1,H,W)."""
    a = np.asarray(planes)
    a = a.reshape(a.shape[0], a.shape[-2], a.shape[-1])
    return np.stack([edt_plane(ef.seeds(a[b], 0, ef.ANY_BOUNDARY)) for b in range(a.shape[0])])


def surface_d2(t):
    """(d2_fg, d2_bg): HIM_EDT_EQUALS 1 and HIM_EDT_EQUALS 0 over the 0/1 planes."""
    a = np.asarray(t)
    a = a.reshape(a.shape[0], a.shape[-2], a.shape[-1])
    return (np.stack([edt_plane(ef.seeds(a[b], 1, ef.EQUALS)) for b in range(a.shape[0])]),
            np.stack([edt_plane(ef.seeds(a[b], 0, ef.EQUALS)) for b in range(a.shape[0])]))


def _d2(d2):
    return torch.as_tensor(np.asarray(d2)).to(torch.int64)


# ---------------------------------------------------------------------------------------------------------- weight
def weight(d2, amp, sigma, dtype, exponent='d2', none='one'):
    """w = 1 + amp * exp(-d2 / (2 sigma^2)); exactly 1 where d2 == NONE."""
    d2 = _d2(d2)
    d = d2.to(dtype)
    if exponent == 'd':                       # planted defect: the distance, not its square
        d = d.sqrt()
    w = 1 + amp * torch.exp(-d / (2 * sigma * sigma))
    if none == 'exp':                         # planted defect: NONE run through exp (2^31 - 1 as a distance)
        return w
    return torch.where(d2 == NONE, torch.ones_like(w), w)


# ---------------------------------------------------------------------------------------------------------- losses
def bw_nll(logp, label, mask, d2, amp, sigma, dtype=F64, g=1.0, denominator='sum_w', **wkw):
    """{'loss', 'sum_w', 'dlogp'} of him_bw_nll_fwd / _bwd.  logp (B,C,H,W), label / mask (B,1,H,W), d2 (B,H,W)."""
    lp = logp.to(dtype)
    B, C, H, W = lp.shape
    ids = label.reshape(B, H, W).to(torch.int64)                   # the kernel's (int) cast: towards zero
    valid = (mask.reshape(B, H, W) >= 0.5) & (ids >= 0) & (ids < C)
    w = torch.where(valid, weight(d2, amp, sigma, dtype, **wkw), torch.zeros((), dtype=dtype))
    picked = lp.gather(1, ids.clamp(0, C - 1)[:, None])[:, 0]
    zero = torch.zeros((), dtype=dtype)
    sum_w = w.sum()
    den = valid.to(dtype).sum() if denominator == 'count' else sum_w      # 'count': planted defect
    loss = torch.where(valid, w * -picked, zero).sum() / den
    dl = torch.zeros_like(lp)
    dl.scatter_(1, ids.clamp(0, C - 1)[:, None], (-g * w / den)[:, None])
    dl = torch.where(valid[:, None], dl, zero)
    return {'loss': loss, 'sum_w': sum_w, 'dlogp': dl}


def pair_term(p, t, kind):
    if kind == 'l1':
        return (p - t).abs()
    return -(t * torch.log(p).clamp(min=-100) + (1 - t) * torch.log(1 - p).clamp(min=-100))


def bw_pair(p, t, d2, amp, sigma, kind, dtype=F64, g=1.0, denominator='sum_w', **wkw):
    """{'loss', 'sum_w', 'dp'} of him_bw_pair_fwd / _bwd.  p, t (B,1,H,W), d2 (B,H,W), kind 'bce' | 'l1'.  The derivative
    is the one the unweighted kernels use: (p - t) / max(p (1 - p), 1e-12) and sign(p - t)."""
    pp, tt = p.to(dtype), t.to(dtype)
    w = weight(d2, amp, sigma, dtype, **wkw).reshape(pp.shape)
    sum_w = w.sum()
    den = torch.tensor(float(pp.numel()), dtype=dtype) if denominator == 'count' else sum_w
    loss = (w * pair_term(pp, tt, kind)).sum() / den
    if kind == 'l1':
        d = torch.sign(pp - tt)
    else:
        d = (pp - tt) / (pp * (1 - pp)).clamp(min=1e-12)
    return {'loss': loss, 'sum_w': sum_w, 'dp': g * w / den * d}


def phi(t, d2_fg, d2_bg, dtype, phi_sign=1):
    fg, bg = _d2(d2_fg), _d2(d2_bg)
    zero = torch.zeros((), dtype=dtype)
    out = torch.where(fg == NONE, zero, fg.to(dtype).sqrt())
    inn = torch.where(bg == NONE, zero, -bg.to(dtype).sqrt())
    return phi_sign * torch.where(t.reshape(fg.shape) < 0.5, out, inn)


def surface(p, t, d2_fg, d2_bg, dtype=F64, g=1.0, phi_sign=1):
    """{'loss', 'dp'} of him_surface_fwd / _bwd."""
    pp = p.to(dtype)
    B, _, H, W = pp.shape
    f = phi(t, d2_fg, d2_bg, dtype, phi_sign).reshape(pp.shape)
    norm = B * H * W * math.sqrt(H * H + W * W)
    return {'loss': (f * pp).sum() / norm, 'dp': g * f / norm}


def trainer_terms(comb_logp, obj_prob, label, gate, obj_gt, amp, sigma, kind='bce', dtype=F64, use_gate=True, **kw):
    """The three terms of a TwoStreamAE_mask step on given network outputs: the layout loss, the object loss on the
    probability the object loss sees (gated with --use_output_gate) and the surface term on the same probability."""
    p = obj_prob.to(dtype) * gate.to(dtype) if use_gate else obj_prob.to(dtype)     # use_gate False: planted defect
    fg, bg = surface_d2(obj_gt.numpy())
    return {'comb': bw_nll(comb_logp, label, gate, boundary_d2(label.numpy()), amp, sigma, dtype, **kw)['loss'],
            'obj': bw_pair(p, obj_gt, boundary_d2(obj_gt.numpy()), amp, sigma, kind, dtype, **kw)['loss'],
            'surface': surface(p, obj_gt, fg, bg, dtype)['loss']}


# ----------------------------------------------------------------------------------------------------------- planes
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def label_plane(kind, B, C, H, W, seed=0):
    """fp32 ids (B,1,H,W).  'uniform': one class, no boundary anywhere; 'checker': every pixel a boundary (ids 0 / 1: with
    C = 1 half of them out of range); 'object': one rectangle of class 1 (255 with C = 1) on class 0, pixel (0, 0) kept at
    0; 'ignore': blocks of valid ids with 255, C and C + 3 among them."""
    ys, xs = torch.arange(H)[:, None], torch.arange(W)[None, :]
    if kind == 'uniform':
        lab = torch.zeros(B, H, W)
    elif kind == 'checker':
        lab = ((ys + xs) % 2).float().expand(B, H, W).clone()
    elif kind == 'object':
        lab = torch.zeros(B, H, W)
        for b in range(B):
            lab[b, H // 4:max(H // 4 + 1, 3 * H // 4), W // 3:max(W // 3 + 1, 2 * W // 3 + b)] = 1 if C > 1 else 255
        lab[:, 0, 0] = 0
    elif kind == 'ignore':
        ids = list(range(min(C, 4))) + [255, C, C + 3]
        lab = torch.from_numpy(ef.blocky(seed + 11, B, H, W, ids, cell=3, salt=0.05)).float()
        lab[:, 0, 0] = 0                                     # one valid position whatever the draw
    else:
        raise ValueError(kind)
    return lab[:, None].contiguous()


def mask_plane(kind, B, H, W):
    """The gate (B,1,H,W): a box that leaves a margin, the whole plane for the tiny shapes."""
    m = torch.zeros(B, 1, H, W)
    m[:, :, H // 8:H - H // 8, W // 8:W - W // 8] = 1
    if kind == 'ignore':
        m[:] = 1                                             # the out-of-range ids sit on valid-mask positions
    return m


def object_plane(kind, B, H, W):
    """The 0/1 instance mask (B,1,H,W): 'empty', 'full', 'checker', 'object' (a rectangle, one pixel at 1x1)."""
    if kind == 'empty' or kind == 'uniform':
        return torch.zeros(B, 1, H, W)
    if kind == 'full':
        return torch.ones(B, 1, H, W)
    return (label_plane(kind, B, 2, H, W) > 0.5).float()


def prob_plane(B, H, W, seed=1, clamp=False):
    """Probabilities in (0, 1); ``clamp``: a sprinkle of exact 0 and 1 (the BCE clamp at -100)."""
    p = torch.rand(B, 1, H, W, generator=_gen(seed)) * 0.98 + 0.01
    if clamp:
        r = torch.rand(B, 1, H, W, generator=_gen(seed + 1))
        p = torch.where(r < 0.15, torch.zeros(()), torch.where(r > 0.85, torch.ones(()), p))
    return p.contiguous()


def logp_planes(B, C, H, W, seed=2):
    return torch.log_softmax(torch.randn(B, C, H, W, generator=_gen(seed)) * 2, 1).contiguous()


_D2_CACHE = {}


def cached_d2(what, kind, B, C, H, W):
    """Distances of the generated planes, computed once per (plane, shape) and shared between the tests."""
    key = (what, kind, B, C, H, W)
    if key not in _D2_CACHE:
        if what == 'label':
            _D2_CACHE[key] = boundary_d2(label_plane(kind, B, C, H, W).numpy())
        elif what == 'object':
            _D2_CACHE[key] = boundary_d2(object_plane(kind, B, H, W).numpy())
        else:
            _D2_CACHE[key] = surface_d2(object_plane(kind, B, H, W).numpy())
    return _D2_CACHE[key]
