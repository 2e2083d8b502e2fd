"""Restatement of the differentiable augmentation (include/him.h, him_diffaug_fwd / him_diffaug_bwd) in torch on the CPU,
written from the formulas, generic in the dtype: float64 is the oracle of the GPU tests, float32 the yardstick ``e32`` of
tests/README.md "How op tests bound errors".  ``backward`` is the adjoint written out by hand; test_diffaug_cpu.py checks
it against torch.autograd of ``forward`` in float64.  Selection is by ``torch.where`` (never a multiplication by a 0/1
mask), so geometric-only rows are copies and +0.0 to the bit in any dtype.  (Helper module like util.py; not a conftest.)"""
import struct

import torch

COLOR, TRANSLATION, CUTOUT = 1, 2, 4


def f32_bits(v):
    """fp32 value -> the int32 holding its bits (the table's first three columns)."""
    return struct.unpack('<i', struct.pack('<f', v))[0]


def bits_f32(i):
    return struct.unpack('<f', struct.pack('<i', i))[0]


def row(b=0.0, a=1.0, k=1.0, ty=0, tx=0, cy=0, cx=0, bits=7):
    return [f32_bits(b), f32_bits(a), f32_bits(k), ty, tx, cy, cx, bits]


def table_tensor(rows):
    return torch.tensor(rows, dtype=torch.int64).to(torch.int32).reshape(-1, 8)


def _geometry(r, H, W, ch, cw, policy):
    """-> (bits, ty, tx, live): live[y, x] = output position (y, x) has its source inside the plane and is not cut."""
    bits = r[7] & policy
    ty, tx = (r[3], r[4]) if bits & TRANSLATION else (0, 0)
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    live = (ys + ty >= 0) & (ys + ty < H) & (xs + tx >= 0) & (xs + tx < W)
    if bits & CUTOUT:
        live = live & ~((ys >= r[5]) & (ys < r[5] + ch) & (xs >= r[6]) & (xs < r[6] + cw))
    return bits, ty, tx, live


def forward(x, rows, ch, cw, c0, policy=7):
    """x (B, C, H, W) of any float dtype -> the augmented tensor in that dtype (differentiable)."""
    B, C, H, W = x.shape
    out = []
    for b in range(B):
        r = rows[b]
        bits, ty, tx, live = _geometry(r, H, W, ch, cw, policy)
        t = x[b]
        if bits & COLOR:
            fb, fa, fk = (bits_f32(v) for v in r[:3])
            img = t[c0:c0 + 3]
            v = img + fb
            p = (v[0] + v[1] + v[2]) / 3
            s = (v - p) * fa + p
            m = img.mean() + fb
            t = torch.cat([t[:c0], (s - m) * fk + m, t[c0 + 3:]], 0)
        ys = (torch.arange(H) + ty).clamp(0, H - 1)
        xs = (torch.arange(W) + tx).clamp(0, W - 1)
        g = t[:, ys][:, :, xs]
        out.append(torch.where(live, g, torch.zeros((), dtype=x.dtype)))
    return torch.stack(out, 0)


def routed(dout, rows, ch, cw, policy=7):
    """g of include/him.h: g[b, c, y', x'] = dout[b, c, y' - ty, x' - tx] where that output position is live, else 0."""
    B, C, H, W = dout.shape
    g = torch.zeros_like(dout)
    for b in range(B):
        bits, ty, tx, live = _geometry(rows[b], H, W, ch, cw, policy)
        d = torch.where(live, dout[b], torch.zeros((), dtype=dout.dtype))
        y0, y1 = max(0, -ty), min(H, H - ty)
        x0, x1 = max(0, -tx), min(W, W - tx)
        if y0 < y1 and x0 < x1:
            g[b, :, y0 + ty:y1 + ty, x0 + tx:x1 + tx] = d[:, y0:y1, x0:x1]
    return g


def backward(dout, rows, ch, cw, c0, policy=7):
    """-> (dx, S): the adjoint of ``forward`` applied to ``dout`` and the per-sample sums S_b (0 for a row without colour)."""
    B, C, H, W = dout.shape
    dx = routed(dout, rows, ch, cw, policy)
    sums = []
    for b in range(B):
        r = rows[b]
        if not (r[7] & policy & COLOR):
            sums.append(torch.zeros((), dtype=dout.dtype))
            continue
        fb, fa, fk = (bits_f32(v) for v in r[:3])
        g = dx[b, c0:c0 + 3].clone()
        S = g.sum()
        ds = fk * g + (1 - fk) * S / (3 * H * W)
        dx[b, c0:c0 + 3] = fa * ds + (1 - fa) * (ds[0] + ds[1] + ds[2]) / 3
        sums.append(S)
    return dx, torch.stack(sums)
