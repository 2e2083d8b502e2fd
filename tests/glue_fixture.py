"""Float64 restatements and deterministic case generators of the pooling, encoding, loss and spectral-norm entry points
(csrc/him_elem.hip, csrc/him_loss.hip, the him_sn_* / him_div_scalar_* part of csrc/him_optim.hip): helper module like
mask_fixture.py, needs neither a GPU nor the library.

Every restatement reads the fp32 tensors the kernel gets and takes ``dtype``: torch.float64 is the reference, the same code
at torch.float32 is the yardstick e32 of tests/README.md.  torch defines the semantics where it has the operation
(F.avg_pool2d(3, 2, 1, count_include_pad=False), F.max_pool2d(k, k) and its autograd routing, F.l1_loss / F.mse_loss with
autograd, scatter_ for the one-hot); the edge map, the colour embedding, the masked image, the slice / blend / tile
kernels, the gates, him_lincomb_* and W / sigma are written out from include/him.h.

Sums: torch's float32 sum is pairwise, the kernels sum per lane and then by tree.  Every restatement of a REDUCED quantity
takes ``order`` in ORDERS -- torch.sum, a strictly sequential sum, 256 strided lanes summed sequentially and combined by a
tree -- all differentiable (``fsum``), none taken from the code under test; ``orders32(f)`` is the list of the three
float32 results whose maximum error is e32.  At float64 the order is torch.sum.
"""
import numpy as np
import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
EPS32 = 2.0 ** -24
FACTOR, FLOOR = 8.0, 16 * EPS32                  # tests/README.md, direct form: error <= max(8 * e32, 16 * 2^-24)
GRID_CAP = 8192 * 256                            # threads of a capped grid-stride launch (gs_grid, the loss backwards, sn dW)
BIG = GRID_CAP + 5                               # a second, partial trip of the grid-stride loop
SIGN_MARGIN = 1e-3                               # a value a sign decision hangs on is exactly 0 or at least this large
SN_EPS = 1e-12
ORDERS = ('torch', 'sequential', 'lanes')


def limit(e32):
    return max(FACTOR * e32, FLOOR)


def rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def uniform(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def randint(lo, hi, *shape, seed=0):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).float()


# ------------------------------------------------------------------------------------------- three summation orders
def _sum_last(x, order):
    """Sum over the last axis of a float tensor in the given order, every addition rounded to x's own precision."""
    if order == 'torch' or x.shape[-1] == 0:
        return x.sum(-1)
    a = x.detach().numpy()
    if order == 'sequential':
        out = np.cumsum(a, axis=-1, dtype=a.dtype)[..., -1]
    else:
        n = a.shape[-1]
        pad = (-n) % 256
        if pad:
            a = np.concatenate([a, np.zeros(a.shape[:-1] + (pad,), a.dtype)], -1)
        lanes = np.cumsum(a.reshape(a.shape[:-1] + (-1, 256)), axis=-2, dtype=a.dtype)[..., -1, :]
        m = 256
        while m > 1:
            m //= 2
            lanes = lanes[..., :m] + lanes[..., m:]
        out = lanes[..., 0]
    return torch.from_numpy(np.ascontiguousarray(out))


class _Sum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, order):
        ctx.n = x.shape[-1]
        return _sum_last(x, order)

    @staticmethod
    def backward(ctx, g):                          # d sum / d x_i = 1 in every order
        return g.unsqueeze(-1).expand(g.shape + (ctx.n,)), None


def fsum(x, order='torch', dim=-1):
    """Differentiable sum over ``dim`` in one of ORDERS."""
    if order == 'torch':
        return x.sum(dim)
    return _Sum.apply(x.movedim(dim, -1).contiguous(), order)


def orders32(f):
    """[f(F32, order) for the three orders]: Checks.row takes the maximum of their errors as e32."""
    return [f(F32, o) for o in ORDERS]


# ----------------------------------------------------------------------------------------------------------- losses
def l1_pair(n, seed=0, relu=False):
    """(a, b): a == b exactly on every third element; elsewhere |a - b| >= 2e-3 (before b is rounded); with ``relu`` a is
    a ReLU output whose positive values are >= 2e-3."""
    a = rand(n, seed=seed)
    if relu:
        a = F.relu(a)
        a[(a > 0) & (a < 2e-3)] = 2e-3
    d = rand(n, seed=seed + 1)
    d = torch.where(d.abs() < 2e-3, torch.where(d < 0, torch.tensor(-2e-3), torch.tensor(2e-3)), d)
    b = a - d
    b[::3] = a[::3]
    return a, b


def sign_margin_ok(v):
    """A value a sign decision hangs on: exactly 0 or at least SIGN_MARGIN in magnitude (asked of float64 AND float32)."""
    return all(bool(((t == 0) | (t.abs() >= SIGN_MARGIN)).all()) for t in (v.double(), v.float()))


def l1_mean(a, b, dtype, order='torch'):
    return (fsum((a.to(dtype) - b.to(dtype)).abs(), order) / a.numel()).reshape(1)


def mse_const(x, target, dtype, order='torch'):
    d = x.to(dtype) - target
    return (fsum(d * d, order) / x.numel()).reshape(1)


def l1_bwd(a, b, g, accumulate, da0, dtype):
    """F.l1_loss's autograd gradient (sign(0) = 0) times g; ``accumulate`` bit 1: gated by a > 0, bit 0: added to da0."""
    x = a.to(dtype).requires_grad_(True)
    (d,) = torch.autograd.grad(F.l1_loss(x, b.to(dtype)), x, torch.tensor(float(g), dtype=dtype))
    if accumulate & 2:
        d = torch.where(a > 0, d, torch.zeros_like(d))
    return da0.to(dtype) + d if accumulate & 1 else d


def mse_bwd(x, target, g, accumulate, dx0, dtype):
    xx = x.to(dtype).requires_grad_(True)
    (d,) = torch.autograd.grad(F.mse_loss(xx, torch.full_like(xx, target)), xx, torch.tensor(float(g), dtype=dtype))
    return dx0.to(dtype) + d if accumulate else d


def lincomb(terms, weights, scale):
    """him_lincomb_fwd in fp32: left to right, every product and every sum rounded on its own."""
    acc = np.float32(0)
    for t, w in zip(terms, weights):
        acc = np.float32(acc + np.float32(np.float32(w) * np.float32(t)))
    return torch.tensor([np.float32(acc * np.float32(scale))])


def lincomb_bwd(g, weights, scale):
    gs = np.float32(np.float32(g) * np.float32(scale))
    return torch.tensor([np.float32(gs * np.float32(w)) for w in weights])


# ------------------------------------------------------------------------------------------------------------ pools
def pool_out(n):
    return (n + 2 - 3) // 2 + 1


def avgpool(x, dtype, dy=None):
    """F.avg_pool2d(3, 2, 1, count_include_pad=False) of (planes, H, W); with ``dy`` its autograd gradient."""
    xx = x.to(dtype).unsqueeze(0).requires_grad_(dy is not None)
    y = F.avg_pool2d(xx, 3, 2, 1, count_include_pad=False)
    if dy is None:
        return y.detach()[0]
    return torch.autograd.grad(y, xx, dy.to(dtype).unsqueeze(0))[0][0]


def maxpool(x, k, dtype, dy=None, relu_gate=False):
    """F.max_pool2d(k, k) of (planes, H, W); with ``dy`` its autograd routing (the first maximum in row-major window order
    wins; rows and columns no window covers get 0), ``relu_gate``: windows whose maximum is not positive pass nothing."""
    xx = x.to(dtype).unsqueeze(0).requires_grad_(dy is not None)
    y = F.max_pool2d(xx, k, k)
    if dy is None:
        return y.detach()[0]
    g = dy.to(dtype).unsqueeze(0)
    if relu_gate:
        g = torch.where(y.detach() > 0, g, torch.zeros_like(g))
    return torch.autograd.grad(y, xx, g)[0][0]


def maxpool_input(planes, H, W, k, seed=1):
    """A ReLU output (ties at 0 inside most windows, equal positive values planted in one) with the first window all
    negative and the second all zero where the plane has two windows."""
    x = F.relu(rand(planes, H, W, seed=seed))
    x[(x > 0) & (x < 2e-3)] = 2e-3                      # the gate's decision (maximum > 0) keeps SIGN_MARGIN
    if H >= k and W >= 2 * k:
        x[0, :k, :k] = -rand(k, k, seed=seed + 1).abs() - 0.5
        x[0, :k, k:2 * k] = 0.0
    if H >= 2 * k and W >= k:
        x[-1, k:2 * k, :k] = 0.75                       # a whole window of equal positive values: the first one wins
    return x


# --------------------------------------------------------------------------------------------------------- encoding
def slice_write(before, c0, value):
    want = before.clone()
    want[:, c0:c0 + value.shape[1]] = value
    return want


def onehot(label, nc, dtype=F32):
    """(B, hw) float ids -> (B, nc, hw) by scatter_; ids outside [0, nc) give all-zero channels."""
    ids = label.long()
    ok = (ids >= 0) & (ids < nc)
    out = torch.zeros(label.shape[0], nc, label.shape[1], dtype=dtype)
    return out.scatter_(1, ids.clamp(0, nc - 1).unsqueeze(1), ok.to(dtype).unsqueeze(1))


def label_map(B, hw, nc, seed=0, strays=True):
    lab = randint(0, nc, B, hw, seed=seed)
    if strays and hw >= 3:
        lab[0, 0], lab[-1, hw // 2], lab[0, -1] = float(nc), 255.0, -1.0
    return lab


def edges(t):
    """oracle.ref_cpu.get_edges on (B, H, W): 1 where a 4-neighbour inside the plane differs."""
    e = torch.zeros_like(t, dtype=torch.bool)
    dx, dy = t[:, :, 1:] != t[:, :, :-1], t[:, 1:, :] != t[:, :-1, :]
    e[:, :, 1:] |= dx
    e[:, :, :-1] |= dx
    e[:, 1:, :] |= dy
    e[:, :-1, :] |= dy
    return e.float()


def inst_map(B, H, W, seed=0):
    """Blocky instance ids: neighbours are equal often enough for both outcomes."""
    return randint(0, 4, B, (H + 1) // 2, (W + 1) // 2, seed=seed).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :H, :W].contiguous()


def masked_image(image, bbox, cls2fill, dtype=F32):
    """data/base_dataset.py get_masked_image per sample: bbox = (wmin, hmin, wmax, hmax), python slice semantics for
    non-negative boxes.  Returns mask (B,1,H,W), object, context."""
    B, C, H, W = image.shape
    mask = torch.zeros(B, 1, H, W, dtype=dtype)
    for b in range(B):
        wmin, hmin, wmax, hmax = (int(v) for v in bbox[b])
        mask[b, 0, hmin:hmax, wmin:wmax] = 1
    img = image.to(dtype)
    return mask, mask * img, (1 - mask) * img + mask * cls2fill


def masked_mean(image, mask, noise, dtype, order='torch'):
    """oracle.ref_cpu.color_embedding on (B,3,hw) / (B,hw): clamp(noise * sum(image * mask) / sum(mask), -1, 1), 0 for an
    empty mask."""
    img, m = image.to(dtype), mask.to(dtype)
    s, cnt = fsum(img * m.unsqueeze(1), order), fsum(m, order).unsqueeze(1)
    e = torch.where(cnt > 0, s / torch.where(cnt > 0, cnt, torch.ones_like(cnt)), torch.zeros_like(s))
    if noise is not None:
        e = e * noise.to(dtype)
    return e.clamp(-1, 1)


MASK_KINDS = ('empty', 'full', 'box', 'fractional')


def mean_mask(kind, B, hw, seed=0):
    if kind == 'empty':
        return torch.zeros(B, hw)
    if kind == 'full':
        return torch.ones(B, hw)
    if kind == 'box':
        m = torch.zeros(B, hw)
        m[:, hw // 4:max(hw // 4 + 1, 3 * hw // 4)] = 1.0
        return m
    return uniform(B, hw, seed=seed)


def tile_embed(emb, mask, dtype=F32):
    return emb.to(dtype).unsqueeze(2) * mask.to(dtype).unsqueeze(1)


def copy_channels(src, cs0, n, mask, mode, dtype=F32):
    v = src.to(dtype)[:, cs0:cs0 + n]
    if mode == 1:
        v = v * mask.to(dtype).unsqueeze(1)
    elif mode == 2:
        v = v * (1 - mask.to(dtype).unsqueeze(1))
    return v


def blend(a, ca0, b, cb0, C, m, dtype=F32):
    mm = m.to(dtype).unsqueeze(1)
    return (1 - mm) * a.to(dtype)[:, ca0:ca0 + C] + mm * b.to(dtype)[:, cb0:cb0 + C]


def box_mask(B, hw, seed=0):
    return (uniform(B, hw, seed=seed) > 0.5).float()


# ---------------------------------------------------------------------------------------------------- spectral norm
def _l2n(x, order):
    return x / (torch.sqrt(fsum(x * x, order)) + SN_EPS)


def sn_chain(W, u, dtype, order='torch', g_sigma=None):
    """s = u W, v = s / (|s| + eps), t = W v, u' = t / (|t| + eps), sigma = u' . t with u a constant and nothing detached;
    with ``g_sigma`` also dW = g_sigma * d sigma / d W by autograd through the whole graph."""
    Wd = W.to(dtype).requires_grad_(g_sigma is not None)
    s = fsum(u.to(dtype).view(-1, 1) * Wd, order, dim=0)
    v = _l2n(s, order)
    t = fsum(Wd * v.view(1, -1), order, dim=1)
    un = _l2n(t, order)
    sigma = fsum(un * t, order).reshape(1)
    out = dict(v=v.detach(), u_out=un.detach(), sigma=sigma.detach())
    if g_sigma is not None:
        (out['dW'],) = torch.autograd.grad(sigma, Wd, torch.tensor([float(g_sigma)], dtype=dtype))
    return out


SN_SHAPES = [(1, 8192), (16, 72), (64, 656), (300, 48), (513, 4100)]


def sn_case(rows, cols, scale=1.0, seed=0):
    return rand(rows, cols, seed=seed + 1, scale=scale * cols ** -0.5), rand(rows, seed=seed + 2)


def div_scalar(W, sigma, dtype):
    return W.to(dtype) / sigma.to(dtype)


def div_scalar_bwd(W, sigma, dout, accumulate, dW0, dtype, order='torch'):
    """dW (+)= dout / sigma, dsigma = -sum(dout * W) / sigma^2."""
    s, d = sigma.to(dtype), dout.to(dtype)
    dW = d / s
    return (dW0.to(dtype) + dW if accumulate else dW), (-fsum(d * W.to(dtype), order) / (s * s)).reshape(1)
