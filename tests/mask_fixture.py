"""Float64 restatements and deterministic case generators of the box2mask building blocks (csrc/him_mask.hip, include/him.h
"box2mask building blocks"): helper module like metrics_fixture.py, needs neither a GPU nor the library.

Every restatement reads the fp32 tensors the kernel gets and takes ``dtype``: torch.float64 is the reference, the same
code at torch.float32 is the yardstick e32 of tests/README.md.  torch's own functions define the semantics where torch has
the operation (F.batch_norm, F.interpolate, F.log_softmax and its backward, F.nll_loss, autograd); the gate combination,
the phase split, the class mask, him_resize_compose and the clamps of torch's BCE are written out.
"""
import numpy as np
import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
EPS32 = 2.0 ** -24
FACTOR, FLOOR = 8.0, 16 * EPS32                  # tests/README.md, direct form: error <= max(8 * e32, 16 * 2^-24)
ACTS = {'none': 0, 'relu': 1, 'lrelu': 2, 'tanh': 3, 'sigmoid': 4}
SLOPE = 0.2
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
GRID_CAP = 8192 * 256                            # threads of a capped grid-stride launch (gs_grid)
LOSS_CAP = 1024 * 256                            # threads of the two loss reductions (LOSS_BLOCKS)
Z_MARGIN = 1e-4                                  # |pre-activation| every relu / lrelu BatchNorm case keeps
MARGIN = 1e-5                                    # him_resize_compose: decisions below this float64 margin are left out
MAX_LEFT_OUT = 0.005                             # ... and at most this share of a case's pixels
BCE_LOG_MIN = -100.0
BCE_DEN_MIN = float(np.float32(1e-12))           # the fp32 constant, so float64 clamps where fp32 does


def limit(e32):
    return max(FACTOR * e32, FLOOR)


def rel_err(got, ref):
    """tests/README.md's metric: maximum error over maximum |ref|; inf when an element is not finite."""
    g, r = torch.as_tensor(got).detach().double().cpu().reshape(-1), torch.as_tensor(ref).detach().double().cpu().reshape(-1)
    if r.numel() == 0:
        return 0.0
    err = (g - r).abs()
    if not bool(torch.isfinite(err).all()):
        return float('inf')
    return float(err.max()) / max(float(r.abs().max()), 1e-30)


def elem_err(got, ref):
    """Maximum per-element relative error; where ref is 0 the value must be 0 as well."""
    g, r = torch.as_tensor(got).detach().double().cpu().reshape(-1), torch.as_tensor(ref).detach().double().cpu().reshape(-1)
    err = (g - r).abs()
    if not bool(torch.isfinite(err).all()) or bool((err[r == 0] != 0).any()):
        return float('inf')
    nz = r != 0
    return float((err[nz] / r[nz].abs()).max()) if bool(nz.any()) else 0.0


def rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def uniform(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def act_fn(z, act):
    return {'none': lambda t: t, 'relu': F.relu, 'lrelu': lambda t: F.leaky_relu(t, SLOPE), 'tanh': torch.tanh,
            'sigmoid': torch.sigmoid}[act](z)


def act_bwd(y, dy, act, dtype):
    """him_act_bwd: the derivative expressed through the activation's OUTPUT."""
    y, dy = y.to(dtype), dy.to(dtype)
    if act == 'relu':
        return torch.where(y > 0, dy, torch.zeros_like(dy))
    if act == 'lrelu':
        return torch.where(y > 0, dy, dy * SLOPE)
    if act == 'tanh':
        return dy * (1 - y * y)
    if act == 'sigmoid':
        return dy * y * (1 - y)
    return dy


# ------------------------------------------------------------------------------------------------------ BatchNorm2d
BN_GENERATORS = ('normal', 'first30', 'first100', 'offset100_first-100', 'const_plus_noise', 'const_channel')
BN_ILL = BN_GENERATORS[1:]


def bn_input(gen, B, C, hw, seed=1):
    """N(0,1) data (B, C, hw); 'first*': only element [0, c, 0] of every channel replaced; 'offset100_first-100': the data
    offset by +100, the first element -100; 'const_plus_noise': 1000 + N(0,1); 'const_channel': channel 1 constant."""
    x = rand(B, C, hw, seed=seed)
    if gen == 'first30':
        x[0, :, 0] = 30.0
    elif gen == 'first100':
        x[0, :, 0] = 100.0
    elif gen == 'offset100_first-100':
        x = x + 100.0
        x[0, :, 0] = -100.0
    elif gen == 'const_plus_noise':
        x = x + 1000.0
    elif gen == 'const_channel':
        x[:, 1] = 0.75
    elif gen != 'normal':
        raise ValueError(gen)
    return x.contiguous()


class BNCase(object):
    """One BatchNorm2d call: act((x - mean) * rstd * gamma + beta) [+ residual] and its backward against ``dy``.  With
    relu / lrelu, beta is searched (0.37, 0.371, ...) per channel until every |pre-activation| exceeds 2 * Z_MARGIN in
    float64 (without gamma / beta: the first data seed that does): the backward's recomputed sign then equals the
    forward's fused one; ``min_abs_z`` records what was reached."""

    def __init__(self, B, C, hw, training, act='none', residual=False, affine=True, running=True, gen='normal'):
        assert running or training
        self.B, self.C, self.hw, self.training, self.act = B, C, hw, bool(training), act
        self.affine, self.running, self.gen = affine, running, gen
        self.x = bn_input(gen, B, C, hw)
        self.rm0 = rand(C, seed=4, scale=0.2) if running else None
        self.rv0 = (1 + rand(C, seed=5, scale=0.1).abs()) if running else None
        self.gamma = (1 + rand(C, seed=2, scale=0.1)) if affine else None
        self.beta = rand(C, seed=3, scale=0.1) if affine else None
        self.residual = rand(B, C, hw, seed=7) if residual else None
        self.dy = rand(B, C, hw, seed=6)
        self.dgamma0, self.dbeta0 = rand(C, seed=8), rand(C, seed=9)      # the prefill of an accumulate != 0 call
        self.min_abs_z = float('inf')
        seed = 1
        while act in ('relu', 'lrelu'):
            mean, rstd = self.stats(F64)
            xhat = (self.x.double() - mean.view(1, -1, 1)) * rstd.view(1, -1, 1)
            if not affine:                          # no beta to choose: the first data seed that keeps the margin
                self.min_abs_z = float(xhat.abs().min())
                if self.min_abs_z > 2 * Z_MARGIN or gen != 'normal':
                    break
                seed += 1
                self.x = bn_input(gen, B, C, hw, seed)
                continue
            g = self.gamma.double()
            best, beta = torch.zeros(C, dtype=F64), torch.zeros(C)
            for k in range(400):
                cand = torch.tensor(0.37 + 0.001 * k, dtype=F32)
                m = (xhat * g.view(1, -1, 1) + cand.double()).abs().amin((0, 2))
                better = (m > best) & (best <= 2 * Z_MARGIN)
                beta = torch.where(better, cand, beta)
                best = torch.where(better, m, best)
                if bool((best > 2 * Z_MARGIN).all()):
                    break
            self.beta, self.min_abs_z = beta, float(best.min())
            break
        self._ref = {}

    def tag(self):
        return 'bn%dx%dx%d|%s|%s|%s%s%s%s' % (self.B, self.C, self.hw, self.gen, 'train' if self.training else 'eval',
                                               self.act, '+res' if self.residual is not None else '',
                                               '' if self.affine else '+noaffine', '' if self.running else '+norun')

    def stats(self, dtype):
        """save_mean, save_rstd as the forward defines them."""
        if self.training:
            x = self.x.to(dtype)
            return x.mean((0, 2)), (x.var((0, 2), unbiased=False) + BN_EPS).rsqrt()
        return self.rm0.to(dtype), (self.rv0.to(dtype) + BN_EPS).rsqrt()

    def ref(self, dtype):
        if dtype not in self._ref:
            x = self.x.to(dtype).clone().requires_grad_(True)
            wrt = [x]
            g = b = None
            if self.affine:
                g, b = self.gamma.to(dtype).clone().requires_grad_(True), self.beta.to(dtype).clone().requires_grad_(True)
                wrt += [g, b]
            rm = self.rm0.to(dtype).clone() if self.running else None
            rv = self.rv0.to(dtype).clone() if self.running else None
            y = act_fn(F.batch_norm(x, rm, rv, g, b, self.training, BN_MOMENTUM, BN_EPS), self.act)
            grads = torch.autograd.grad(y, wrt, self.dy.to(dtype))
            mean, rstd = self.stats(dtype)
            r = {'y': (y + self.residual.to(dtype) if self.residual is not None else y).detach(), 'save_mean': mean,
                 'save_rstd': rstd, 'dx': grads[0]}
            if self.running:
                r['run_mean'], r['run_var'] = rm, rv
            if self.affine:
                r['dgamma'], r['dbeta'] = grads[1], grads[2]
            self._ref[dtype] = r
        return self._ref[dtype]


# ---------------------------------------------------------------------------------------------- bilinear, log-softmax
def upsample2(x, align, dtype, dy=None):
    """(planes, H, W) -> (planes, 2H, 2W); with ``dy`` the gradient with respect to x instead."""
    x = x.to(dtype)[None].clone().requires_grad_(dy is not None)
    y = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=bool(align))
    if dy is None:
        return y[0].detach()
    return torch.autograd.grad(y, x, dy.to(dtype)[None])[0][0]


def log_softmax(x, dtype):
    return F.log_softmax(x.to(dtype), 1)


def log_softmax_bwd(y, dy, dtype):
    """torch's own backward of log_softmax from (dy, y): dy - exp(y) * sum_c dy."""
    return torch.ops.aten._log_softmax_backward_data(dy.to(dtype), y.to(dtype), 1, dtype)


# ------------------------------------------------------------------------------------------------- gate combination
def gate_comb(ctx, p, obj, dtype):
    """comb = (1 - p) * ctx + p * obj, p and obj (B, 1, hw); at float32 every product and the sum round on their own."""
    ctx, p, obj = ctx.to(dtype), p.to(dtype), obj.to(dtype)
    return (1 - p) * ctx + p * obj


def gate_comb_bwd(ctx, p, obj, dout, dtype):
    ctx, p, obj, dout = ctx.to(dtype), p.to(dtype), obj.to(dtype), dout.to(dtype)
    return {'dctx': (1 - p) * dout, 'dobj': p * dout.sum(1, keepdim=True), 'dp': (dout * (obj - ctx)).sum(1, keepdim=True)}


# ------------------------------------------------------------------------------------------------------------ losses
def nll_valid(label, mask, C):
    """A position counts when mask >= 0.5 and the label lies in [0, C)."""
    return (mask >= 0.5) & (label >= 0) & (label < C)


def masked_nll(logp, label, mask, dtype, g=None):
    """logp (B, C, hw), label / mask (B, hw) float -> (loss, count); with ``g`` the gradient g * dloss/dlogp as well."""
    C = logp.shape[1]
    valid = nll_valid(label, mask, C)
    tgt = torch.where(valid, label, torch.full_like(label, -100.0)).long()
    lp = logp.to(dtype).clone().requires_grad_(g is not None)
    loss = F.nll_loss(lp, tgt, ignore_index=-100)
    if g is None:
        return loss.detach(), int(valid.sum())
    return loss.detach(), int(valid.sum()), torch.autograd.grad(loss, lp, torch.as_tensor(g).to(dtype).reshape(()))[0]


def bce_mean(p, t, dtype):
    """nn.BCELoss(): both logarithms clamped at -100."""
    p, t = p.to(dtype), t.to(dtype)
    return -(t * p.log().clamp_min(BCE_LOG_MIN) + (1 - t) * (1 - p).log().clamp_min(BCE_LOG_MIN)).mean()


def bce_mean_bwd(p, t, g, dtype):
    """torch's binary_cross_entropy_backward: g / n * (p - t) / max(p * (1 - p), 1e-12f)."""
    p, t = p.to(dtype), t.to(dtype)
    return float(g) / p.numel() * (p - t) / (p * (1 - p)).clamp_min(BCE_DEN_MIN)


def bce_saturated():
    """64 elements: p in {0, 1, 1e-30, 1 - 2^-24, 0.5} x t in {0, 1}, repeated."""
    ps = torch.tensor([0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24, 0.5], dtype=F32)
    p = ps.repeat_interleave(2).repeat(7)[:64].contiguous()
    t = torch.tensor([0.0, 1.0]).repeat(32)
    return p, t


def nll_case(B, C, hw, kind='random', seed=11):
    """(logp, label, mask).  'random': mask values around 0.5 (0.5 itself, its two fp32 neighbours) among 0 / 1 / uniform
    ones, labels with 255, -1 and C among the valid ids; 'none': no valid position; 'one': exactly one."""
    logp = F.log_softmax(rand(B, C, hw, seed=seed, scale=2.0), 1)
    g = torch.Generator().manual_seed(seed + 1)
    label = torch.randint(0, C, (B, hw), generator=g).float()
    pick = torch.randint(0, 8, (B, hw), generator=g)
    vals = torch.tensor([0.0, 1.0, 0.5, 0.49999997, 0.50000006, 1.0, 0.0, 1.0], dtype=F32)
    mask = torch.where(pick == 7, torch.rand(B, hw, generator=g), vals[pick])
    bad = torch.randint(0, 12, (B, hw), generator=g)
    for k, v in ((0, 255.0), (1, -1.0), (2, float(C))):
        label[bad == k] = v
    if B * hw >= 6:                                 # each edge value certainly once on a counted / ignored position
        fl, fm = label.view(-1), mask.view(-1)
        fm[0:3] = torch.tensor([0.5, 0.49999997, 0.50000006])
        fl[0:3] = 0.0
        fm[3:6] = 1.0
        fl[3:6] = torch.tensor([255.0, -1.0, float(C)])
    if kind == 'none':
        mask = mask.clamp_max(0.49999997)
    elif kind == 'one':
        mask = mask.clamp_max(0.49999997)
        mask.view(-1)[B * hw // 2] = 0.5
        label.view(-1)[B * hw // 2] = float(C - 1)
    elif kind != 'random':
        raise ValueError(kind)
    return logp.contiguous(), label.contiguous(), mask.contiguous()


# ----------------------------------------------------------------------------------------- phase split and class mask
def space_to_batch(x, d):
    """y[(b*d + py)*d + px][c][i][j] = x[b][c][i*d + py][j*d + px]."""
    B, C, H, W = x.shape
    return x.view(B, C, H // d, d, W // d, d).permute(0, 3, 5, 1, 2, 4).reshape(B * d * d, C, H // d, W // d).contiguous()


def batch_to_space(y, d, B):
    _, C, Hd, Wd = y.shape
    return y.view(B, d, d, C, Hd, Wd).permute(0, 3, 4, 1, 5, 2).reshape(B, C, Hd * d, Wd * d).contiguous()


def class_mask(mask, cls, before, NC, c0):
    """dst[b][c0 + c] = mask[b] if c == cls[b] else 0 for c in [0, NC); every other channel of ``before`` stays."""
    out = before.clone()
    for b in range(mask.shape[0]):
        out[b, c0:c0 + NC] = 0.0
        k = int(cls[b])
        if 0 <= k < NC:
            out[b, c0 + k] = mask[b]
    return out


# ------------------------------------------------------------------------------------------------- him_resize_compose
def bilinear_src(out_size, in_size, align, dtype):
    """Source index pair and second weight of every output index, as include/him.h words them (him_upsample2_fwd's)."""
    o = torch.arange(out_size, dtype=dtype)
    if align:
        src = o * (in_size - 1) / (out_size - 1) if out_size > 1 else torch.zeros_like(o)
    else:
        src = ((o + 0.5) * (torch.tensor(float(in_size), dtype=dtype) / torch.tensor(float(out_size), dtype=dtype)) - 0.5)
        src = src.clamp_min(0)
    i0 = src.long().clamp_max(in_size - 1)
    return i0, (i0 + 1).clamp_max(in_size - 1), src - i0.to(dtype)


def resize(p, H, W, align, dtype):
    """(C, h, w) -> (C, H, W): h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11)."""
    p = p.to(dtype)
    y0, y1, wy = bilinear_src(H, p.shape[1], align, dtype)
    x0, x1, wx = bilinear_src(W, p.shape[2], align, dtype)
    wy, wx = wy.view(1, -1, 1), wx.view(1, 1, -1)
    top = (1 - wx) * p[:, y0][:, :, x0] + wx * p[:, y0][:, :, x1]
    bot = (1 - wx) * p[:, y1][:, :, x0] + wx * p[:, y1][:, :, x1]
    return (1 - wy) * top + wy * bot


def resize_compose(src, label, mask, cls, background, align, dtype=F64):
    """him_resize_compose -> (dst, margin): object branch dst f32 = resized obj > .5 ? cls : label, margin |obj - .5|;
    background branch dst i64 = argmax_c (resized p_c * m + (1 - m) * [label == c]), the first index wins, margin = the gap
    between the two largest channel values."""
    H, W = label.shape
    v = resize(src, H, W, align, dtype)
    if not background:
        return torch.where(v[0] > 0.5, torch.full_like(label, float(cls)), label), (v[0] - 0.5).abs()
    C = src.shape[0]
    m = mask.to(dtype)
    onehot = (label.view(1, H, W) == torch.arange(C, dtype=label.dtype).view(C, 1, 1)).to(dtype)
    val = v * m + (1 - m) * onehot
    dst = torch.from_numpy(np.argmax(val.numpy(), axis=0))               # numpy: the first of equal maxima
    top = val.topk(min(2, C), dim=0).values
    return dst, (top[0] - top[1]) if C > 1 else torch.ones(H, W, dtype=dtype)


RESIZE_SHAPES = [((1, 1), (3, 5)), ((8, 8), (16, 16)), ((16, 12), (37, 50)), ((64, 64), (128, 128))]
RESIZE_C = 35


def resize_case(lo, hi, background, seed=21):
    """(src, label, mask, cls): uniform object probabilities / a softmax of N(0, 2) logits; the mask mixes 0, 1 and
    uniform values."""
    (h, w), (H, W) = lo, hi
    g = torch.Generator().manual_seed(seed + h + W)
    label = torch.randint(0, RESIZE_C, (H, W), generator=g).float()
    if not background:
        return torch.rand(1, h, w, generator=g), label, None, 7
    src = F.softmax(torch.randn(RESIZE_C, h, w, generator=g) * 2.0, 0)
    pick = torch.randint(0, 4, (H, W), generator=g)
    mask = torch.where(pick == 0, torch.zeros(H, W), torch.where(pick == 3, torch.rand(H, W, generator=g), torch.ones(H, W)))
    return src.contiguous(), label, mask.contiguous(), RESIZE_C - 1


def resize_tie_case():
    """Channels 3 and 7 hold the same, largest values and the mask is 1: index 3 must win everywhere."""
    src, label, mask, cls = resize_case((8, 8), (16, 16), True)
    src = src * 0.25
    src[3] = src[7] = 0.5 + 0.25 * uniform(8, 8, seed=5)
    return src.contiguous(), label, torch.ones_like(mask), cls
