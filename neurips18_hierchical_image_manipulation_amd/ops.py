"""torch.autograd bindings of the HIP kernels (the only place the C ABI is called from).

PyTorch supplies device memory, the current HIP stream and the autograd tape; every arithmetic op of
the hot path below is a hand-written gfx950 kernel in libhim_hip.so.  Nothing here runs on the CPU and
nothing falls back: a non-CUDA tensor raises.

Weight gradients: parameters that live in a flat gradient arena (``optim.FlatArena``) carry
``_him_direct_grad = True``; their wgrad kernels accumulate straight into ``param.grad`` (which is a view
of the arena, zeroed by ``zero_grad``) and autograd receives ``None`` -- no per-parameter add pass and no
bucket copies for the RCCL all-reduce.
"""
import collections
import contextlib
import ctypes
import os
import threading

import torch

from ._cabi import (lib, HimAlgo, HimConv2d, HimDeconv2d, HimResBlock, ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID,
                    PAD_ZERO, PAD_REFLECT, HimError, ONEHOT_PART_IDS, ONEHOT_PART_DENSE)

ACTS = {'none': ACT_NONE, 'relu': ACT_RELU, 'lrelu': ACT_LRELU, 'tanh': ACT_TANH, 'sigmoid': ACT_SIGMOID}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise HimError('HIP op called with a non-GPU tensor: the product path has no CPU fallback')
        if t.dtype != torch.float32:
            raise HimError('HIP ops are fp32 only, got %s' % t.dtype)
        if not t.is_contiguous():
            raise HimError('HIP ops need contiguous NCHW tensors')


def _p(t):
    return 0 if t is None else t.data_ptr()


def _ws(nbytes, like):
    n = max((int(nbytes) + 3) // 4, 1)
    return torch.empty(n, dtype=torch.float32, device=like.device)


def _direct(p):
    return getattr(p, '_him_direct_grad', False) and p.grad is not None


from .config import SCHED

_STREAMS = {}           # (name, device) -> torch.cuda.Stream, created on first use


def _named_stream(name, device):
    s = _STREAMS.get((name, device))
    if s is None:
        s = _STREAMS[name, device] = torch.cuda.Stream(device=device)
    return s


# Weight gradients that go straight into a gradient arena are not needed by anything until the optimizer / the
# all-reduce, so they run on a SIDE stream next to the data-gradient chain: the two MFMA kernels of a layer fill each
# other's partial last waves (every launch here has an imperfect tile count for 256 CUs).  ``join_side_stream`` makes
# the current stream wait for them (called by FusedAdam.step / zero_grad and the reducer).
def _side_stream(device):
    return _named_stream('side', device)


def _opt_stream(device):
    """Stream of the generator's optimizer step (runs next to the discriminator's backward)."""
    return _named_stream('opt', device)


def _vgg_stream(device):
    """Stream of the VGG(fake) forward / backward (next to the discriminator passes on the fake image)."""
    return _named_stream('vgg', device)


def _real_stream(device):
    """Stream of everything that depends only on the REAL image (its discriminator pass, its VGG features) and of that
    branch's backward.  Not the weight-gradient stream: the branch's data-gradient chain must not queue behind the
    generator's last weight gradients at the end of the step (r03b trace: 4 ms of idle main stream)."""
    return _named_stream('real', device)


def _d_opt_stream(device):
    """Stream of the discriminator's gradient exchange + optimizer step in data-parallel runs (hidden under the NEXT
    step's input encoding and generator forward)."""
    return _named_stream('d_opt', device)


def _side_streams(device=None):
    """(device, side stream) of every device that has one (``device``: that one only)."""
    return [(dev, s) for (name, dev), s in _STREAMS.items() if name == 'side' and (device is None or dev == device)]


# Weight-gradient routing: by default every weight gradient goes to the one side stream.  A trainer may route the weight
# gradients ISSUED FROM a given stream to another one for the duration of a backward pass (``route_wgrads``): during
# loss_D.backward() the fake-image branch (data gradients on the main stream) and the real-image branch (data gradients
# on the side stream, where its forward ran) then each get a weight-gradient stream of their own instead of queueing all
# of D's weight gradients behind the generator's on the single side stream.
_WGRAD_ROUTE = {}      # cuda_stream handle of the issuing stream -> torch.cuda.Stream that takes its weight gradients
# device -> {routed stream handle: event recorded behind the LAST weight-gradient launch routed there}.  Joins wait for
# the EVENT, not for the stream: a routed stream (the VGG stream) goes on to carry other work, and neither the optimizers
# nor the reducers should wait for that (an entry whose launches have finished costs a join nothing).
_WGRAD_USED = {}


class route_wgrads(object):
    """Route the weight gradients issued from the given streams; restores the previous routes on exit (nestable)."""

    def __init__(self, routes):
        self.routes = {src.cuda_stream: dst for src, dst in routes.items()}

    def __enter__(self):
        self.saved = {k: _WGRAD_ROUTE.get(k) for k in self.routes}
        _WGRAD_ROUTE.update(self.routes)

    def __exit__(self, *a):
        for k, prev in self.saved.items():
            if prev is None:
                _WGRAD_ROUTE.pop(k, None)
            else:
                _WGRAD_ROUTE[k] = prev
        return False


def wgrad_waitables(device):
    """What a consumer of ``device``'s weight gradients must wait for: the side stream, and the event behind the last
    launch on every stream weight gradients were routed to.  -> (streams, events)"""
    return ([s for _, s in _side_streams(device)], list(_WGRAD_USED.get(device, {}).values()))


def join_side_stream(device=None):
    for dev, s in _side_streams(device):
        torch.cuda.current_stream(dev).wait_stream(s)
    for dev, used in _WGRAD_USED.items():
        if device is None or dev == device:
            cur = torch.cuda.current_stream(dev)
            for ev in used.values():
                cur.wait_event(ev)


class _wgrad_stream(object):
    """Context: run the enclosed launches on the weight-gradient stream (the side stream, or the stream the issuing stream
    is routed to), after everything enqueued so far on the current one."""

    def __init__(self, *tensors, weight=None):
        self.tensors = [t for t in tensors if t is not None]
        self.weight = weight

    def __enter__(self):
        self.on = SCHED.wgrad_stream
        if not self.on:
            return None
        dev = self.tensors[0].device
        main = torch.cuda.current_stream(dev)
        side = _WGRAD_ROUTE.get(main.cuda_stream)
        alt = getattr(self.weight, '_him_wgrad_alt', None)
        if side is None and ((alt == 'tail' and SCHED.g_tail_wgrad_alt) or (alt == 'head' and SCHED.g_head_wgrad_alt)):
            # the LAST weight gradients of a chain-shaped generator's backward (its down-convolutions): on the VGG stream
            # (idle since VGG's backward) next to the ResnetBlock stack's weight-gradient GEMMs still queued on the
            # weight-gradient stream, instead of behind them (Pix2PixHDModel_condImg marks the weights)
            side = _vgg_stream(dev)
        self.routed = side is not None
        if side is None:
            side = _side_stream(dev)
        self.side, self.dev = side, dev
        side.wait_stream(main)
        for t in self.tensors:
            t.record_stream(side)
        self.ctx = torch.cuda.stream(side)
        self.ctx.__enter__()
        return side

    def __exit__(self, *a):
        if self.on:
            if self.routed:
                ev = torch.cuda.Event()
                ev.record(self.side)
                _WGRAD_USED.setdefault(self.dev, {})[self.side.cuda_stream] = ev
            self.ctx.__exit__(*a)
        return False


# Run-time gradient routing for graphs that are shared between the generator loss and the discriminator loss (the
# fake-image discriminator pass is computed ONCE, see Pix2PixHDModel_condImg.forward): ids of weights whose weight
# gradient / whose layer-input gradient must not be computed during the current backward.
SKIP_WGRAD = set()
SKIP_DGRAD = set()


class _GradSwitch(torch.autograd.Function):
    """Identity whose backward passes the gradient only while ``state['open']`` is true."""

    @staticmethod
    def forward(ctx, x, state):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        ctx.state = state
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.state['open']:
            return None, None
        # everything downstream of this node (the discriminator) has finished its part of this backward pass: a trainer
        # may hang work on that moment (Pix2PixHDModel_condImg: D's Adam step, whose weights nobody reads any more)
        cb = ctx.state.pop('on_open_backward', None)
        if cb is not None:
            cb()
        return g, None


def _wkey(w):
    """Routing key of a weight tensor: the id of the PARAMETER it was derived from (spectral-norm layers hand the conv a
    fresh W / sigma tensor every forward and tag it with ``_him_wkey``), else its own id."""
    return getattr(w, '_him_wkey', id(w))


def grad_switch(x, state):
    return _GradSwitch.apply(x, state)


def _notify(p):
    """Tell the data-parallel reducer (if any) that this parameter's gradient for the step is final."""
    r = getattr(p, '_him_reducer', None)
    if r is not None:
        r.on_param(p)


# ------------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------------
# Kernel selection (include/him.h "Algorithm selection"): the library keeps no global state -- every descriptor carries a
# HimAlgo.  This module keeps ONE current HimAlgo per host thread (``current_algo``): the process default is read from
# the HIM_* environment once at import through ``him_algo_from_env`` (tools/ A/B runs; an empty environment = the
# defaults), ``algo_scope`` / ``set_winograd_min_channels`` change the calling thread's copy.
_ALGO_TLS = threading.local()
_ALGO_DEFAULT = None


def _default_algo():
    global _ALGO_DEFAULT
    if _ALGO_DEFAULT is None:
        a = HimAlgo()
        lib.him_algo_from_env(ctypes.byref(a))
        _ALGO_DEFAULT = a
    return _ALGO_DEFAULT


def current_algo():
    """The calling thread's HimAlgo (a live object: descriptors COPY it when they are built)."""
    a = getattr(_ALGO_TLS, 'algo', None)
    if a is None:
        a = _ALGO_TLS.algo = HimAlgo.from_buffer_copy(_default_algo())
    return a


def resolved_algo(algo=None):
    """dict of the concrete values a HimAlgo selects (zeros replaced by the library's defaults) -- for reports."""
    out = HimAlgo()
    lib.him_algo_resolve(ctypes.byref(algo if algo is not None else current_algo()), ctypes.byref(out))
    return out.as_dict()


@contextlib.contextmanager
def algo_scope(**fields):
    """Temporarily override fields of the calling thread's HimAlgo, e.g. ``algo_scope(wino_min_c=-1)`` (direct form),
    ``algo_scope(ksplit_max=4)``, ``algo_scope(disable=ALGO_NO_FEWCH_MFMA)``."""
    a = current_algo()
    saved = HimAlgo.from_buffer_copy(a)
    try:
        for k, v in fields.items():
            setattr(a, k, v)
        yield a
    finally:
        ctypes.memmove(ctypes.byref(a), ctypes.byref(saved), ctypes.sizeof(HimAlgo))


def _conv_desc(x, w, stride, pad, pad_mode, act, slope, frozen=False):
    B, Cin, H, W = x.shape
    Cout, Cin2, KH, KW = w.shape
    if Cin2 != Cin:
        raise HimError('conv2d: weight expects %d input channels, got %d' % (Cin2, Cin))
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    d = HimConv2d(B, Cin, H, W, Cout, KH, KW, stride, pad, pad_mode, OH, OW, act, slope, current_algo())
    if frozen:
        d.algo.disable |= _ALGO_FROZEN
    return d


_ALGO_FROZEN = 1 << 9


# Weight panels: the MFMA kernels read the weights regrouped (include/him.h "Weight panels").  Weights change once
# per optimizer step, so the panel of every nn.Parameter is cached on the parameter and rebuilt (a) by
# FusedAdam.step() right after the update -- on the optimizer's stream, under the other network's backward -- or (b)
# lazily when the parameter's version counter / storage moved (load_state_dict, torch optimizers).  Code that writes
# weights behind torch's back (raw pointers, ``p.data.copy_``) must call ``invalidate_panels``.
PANEL_FWD, PANEL_BWD_DATA = 0, 1


class _Panel(object):
    __slots__ = ('buf', 'nbytes', 'desc', 'is_deconv', 'kind', 'token', 'event', 'stream_id')


def _panel_token(w):
    return (w._version, w.data_ptr(), getattr(w, '_him_gen', 0))


def _build_panel(w, e):
    fn = lib.him_deconv2d_panel_build if e.is_deconv else lib.him_conv2d_panel_build
    fn(ctypes.byref(e.desc), e.kind, _p(w), _p(e.buf), e.nbytes, _stream())
    e.token = _panel_token(w)
    e.event = torch.cuda.Event()
    e.event.record(torch.cuda.current_stream())
    e.stream_id = _stream()


_PANEL_KEYS = {}     # (descriptor bytes, kind asked for, is_deconv) -> (cache key, panel bytes, kind of the panel that serves it)


def _panel(w, d, kind, is_deconv):
    """Device pointer of the cached panel of parameter ``w`` for descriptor ``d`` (0: use the plain entry point)."""
    if not SCHED.panel_cache or not isinstance(w, torch.nn.Parameter):
        return 0
    cache = w.__dict__.get('_him_panels')
    if cache is None:
        cache = w.__dict__['_him_panels'] = {}
    # every descriptor field the panel LAYOUT can depend on (include/him.h "Weight panels": Winograd eligibility needs
    # pad 1 + planes >= 2x2 + an unchanged plane size for the data gradient; tiny heads switch on the output size)
    # ... and the HimAlgo the panel is built with (Winograd thresholds decide the layout)
    # The layout is the LIBRARY's choice for this descriptor (him_conv2d_panel_layout: implicit GEMM / Winograd F(2x2) /
    # fused Winograd / F(4x4)) and depends on batch and plane size, not on the weight alone: the same frozen VGG weight on
    # the last, smaller batch of an epoch leaves F(4x4) (a 36-position panel read as a 16-position one).
    #  the two size / layout queries are ctypes calls; their answer is a pure function of (descriptor, kind):
    # memoised per descriptor bytes so a cache hit stays pure Python on the launch path
    mk = (bytes(d), kind, is_deconv)
    hit = _PANEL_KEYS.get(mk)
    if hit is None:
        if kind == PANEL_BWD_DATA and not is_deconv and lib.him_conv2d_bwd_data_shares_fwd_panel(ctypes.byref(d)):
            kind = PANEL_FWD        # separate-transform Winograd layers: ONE panel per weight serves both directions
        nbytes = int((lib.him_deconv2d_panel_bytes if is_deconv else lib.him_conv2d_panel_bytes)(ctypes.byref(d), kind))
        if is_deconv:
            key = (kind, d.stride, d.pad, d.out_pad, nbytes, bytes(d.algo))
        else:
            key = (kind, int(lib.him_conv2d_panel_layout(ctypes.byref(d), kind)), nbytes, d.stride, d.pad, d.pad_mode,
                   d.H >= 2 and d.W >= 2, d.OH == d.H and d.OW == d.W,
                   d.B * d.OH * d.OW < 131072, d.B * d.Cin * d.H * d.W < (1 << 29), d.B * d.Cout * d.H * d.W < (1 << 29),
                   bytes(d.algo))
        if len(_PANEL_KEYS) > 4096:
            _PANEL_KEYS.clear()
        hit = _PANEL_KEYS[mk] = (key, nbytes, kind)
    key, nbytes, kind = hit
    e = cache.get(key)
    if e is None:
        e = cache[key] = _Panel()
        e.kind, e.is_deconv = kind, is_deconv
        e.desc = type(d).from_buffer_copy(d)
        e.nbytes = nbytes
        e.buf = torch.empty(e.nbytes // 4, dtype=torch.float32, device=w.device) if e.nbytes else None
        e.token = None
    if e.buf is None:
        return 0
    if e.token != _panel_token(w):
        _build_panel(w, e)
    if e.stream_id != _stream():
        torch.cuda.current_stream().wait_event(e.event)
    return e.buf.data_ptr()


def refresh_panels(params):
    """Rebuild the cached panels of ``params`` on the current stream (called by FusedAdam.step after the update)."""
    for p in params:
        p._him_gen = getattr(p, '_him_gen', 0) + 1
        cache = p.__dict__.get('_him_panels')
        if cache:
            for e in cache.values():
                if e.buf is not None:
                    _build_panel(p, e)


def invalidate_panels(params):
    for p in params:
        p._him_gen = getattr(p, '_him_gen', 0) + 1


def set_winograd_min_channels(c):
    """3x3 stride-1 convs with >= c channels on both sides run as Winograd F(2x2,3x3); c <= 0: EVERY Winograd form off.
    Sets ``current_algo().wino_min_c`` of the calling thread (cached panels are keyed by the HimAlgo they were built
    with); returns the previous setting (0 = the library default, 256)."""
    a = current_algo()
    prev = int(a.wino_min_c)
    a.wino_min_c = -1 if c <= 0 else (0 if int(c) == 256 else int(c))
    return prev if prev != 0 else 256


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad, pad_mode, act, slope, premasked=False, gate_dx=False):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        x = x.contiguous()
        _chk(x, w, b)
        d = _conv_desc(x, w, stride, pad, pad_mode, act, slope, frozen=bool(getattr(w, '_him_frozen', False)))
        if premasked and act != ACT_RELU:
            raise HimError('conv2d: only a ReLU gate can be applied by the producers of the output gradient')
        ctx.premasked, ctx.gate_dx = bool(premasked), bool(gate_dx)
        y = torch.empty((d.B, d.Cout, d.OH, d.OW), dtype=torch.float32, device=x.device)
        nb = lib.him_conv2d_fwd_ws(ctypes.byref(d))
        ws = _ws(nb, x)
        pan = _panel(w, d, PANEL_FWD, False)
        keep = None
        if pan and SCHED.keep_wino_input and ctx.needs_input_grad[1] and _direct(w):
            # separate-transform Winograd layer whose weight gradient will be taken: keep the transformed input
            nk = int(lib.him_conv2d_fwd_keep_bytes(ctypes.byref(d)))
            if nk:
                keep = torch.empty(nk // 4, dtype=torch.float32, device=x.device)
        if keep is not None:
            lib.him_conv2d_fwd_panel_keep(ctypes.byref(d), _p(x), pan, _p(b), _p(y), _p(keep), _p(ws), nb, _stream())
        elif pan:
            lib.him_conv2d_fwd_panel(ctypes.byref(d), _p(x), pan, _p(b), _p(y), _p(ws), nb, _stream())
        else:
            lib.him_conv2d_fwd(ctypes.byref(d), _p(x), _p(w), _p(b), _p(y), _p(ws), nb, _stream())
        ctx.d = d
        ctx.x, ctx.w, ctx.b, ctx.keep = x, w, b, keep
        ctx.gslice = getattr(x, '_him_grad_slice', None)
        # the OUTPUT must go through save_for_backward: a plain ctx attribute closes a tensor -> grad_fn -> ctx -> tensor
        # cycle through C++ that no collector sees, and with it the whole upstream graph of every step leaks
        ctx.save_for_backward(y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 10
        d, x, w, b = ctx.d, ctx.x, ctx.w, ctx.b
        dy = dy.contiguous()
        st = _stream()
        if d.act != ACT_NONE and not ctx.premasked:
            dz = torch.empty_like(dy)
            lib.him_act_bwd(_p(ctx.saved_tensors[0]), _p(dy), _p(dz), dy.numel(), d.act, d.slope, st)
        else:
            dz = dy
        dx = dw = db = None
        gs = ctx.gslice
        if ctx.needs_input_grad[0] and _wkey(w) not in SKIP_DGRAD and gs is not None and gs[1] <= 4 < d.Cin:
            # only channels [c0, c0+n) of the input can use a gradient (first PatchGAN conv: the image channels behind
            # 35..70 channels of data): data gradient of the n-channel weight slice (tiny-M kernel), zeros elsewhere
            c0, n = gs
            d2 = HimConv2d.from_buffer_copy(d)
            d2.Cin = n
            dxs = torch.empty((d.B, n, d.H, d.W), dtype=torch.float32, device=x.device)
            wsl = w.detach()[:, c0:c0 + n].contiguous()
            nb = lib.him_conv2d_bwd_data_ws(ctypes.byref(d2))
            ws = _ws(nb, x)
            lib.him_conv2d_bwd_data(ctypes.byref(d2), _p(dz), _p(wsl), _p(dxs), _p(ws), nb, st)
            dx = torch.zeros_like(x)
            lib.him_copy_channels(_p(dxs), n, 0, _p(dx), d.Cin, c0, n, d.B, d.H * d.W, 0, 0, 0, st)
        elif ctx.needs_input_grad[0] and _wkey(w) not in SKIP_DGRAD:
            dx = torch.empty_like(x)
            nb = lib.him_conv2d_bwd_data_ws(ctypes.byref(d))
            ws = _ws(nb, x)
            pan = _panel(w, d, PANEL_BWD_DATA, False)
            if ctx.gate_dx:     # x is a ReLU output whose consumers apply its gate: dx = (x > 0) * dgrad
                lib.him_conv2d_bwd_data_gated(ctypes.byref(d), _p(dz), 0 if pan else _p(w), pan or 0, _p(x), _p(dx),
                                              _p(ws), nb, st)
            elif pan:
                lib.him_conv2d_bwd_data_panel(ctypes.byref(d), _p(dz), pan, _p(dx), _p(ws), nb, st)
            else:
                lib.him_conv2d_bwd_data(ctypes.byref(d), _p(dz), _p(w), _p(dx), _p(ws), nb, st)
        skip_w = _wkey(w) in SKIP_WGRAD
        need_w = ctx.needs_input_grad[1] and not skip_w
        need_b = b is not None and ctx.needs_input_grad[2] and not skip_w
        if need_w or need_b:
            nb = lib.him_conv2d_bwd_weight_ws(ctypes.byref(d))
            if need_w and _direct(w) and (not need_b or _direct(b)):
                with _wgrad_stream(x, dz, ctx.keep, weight=w):
                    ws = _ws(nb, x)
                    if ctx.keep is not None:
                        lib.him_conv2d_bwd_weight_kept(ctypes.byref(d), _p(ctx.keep), _p(dz), _p(w.grad),
                                                       _p(b.grad) if need_b else 0, 1, _p(ws), nb, _stream())
                    else:
                        lib.him_conv2d_bwd_weight(ctypes.byref(d), _p(x), _p(dz), _p(w.grad),
                                                  _p(b.grad) if need_b else 0, 1, _p(ws), nb, _stream())
                    _notify(w)
                    if need_b:
                        _notify(b)
            else:
                ws = _ws(nb, x)
                dw = torch.empty_like(w) if need_w else None
                db = torch.empty_like(b) if need_b else None
                lib.him_conv2d_bwd_weight(ctypes.byref(d), _p(x), _p(dz), _p(dw), _p(db), 0, _p(ws), nb, st)
        ctx.keep = None
        return dx, dw, db, None, None, None, None, None, None, None


class _OneHotConv2d(torch.autograd.Function):
    """conv2d over [one-hot(label) | dense channels] evaluated from the label ids (include/him.h "One-hot stems")."""

    @staticmethod
    def forward(ctx, x, label, n_onehot, w, b, pad, pad_mode, act, slope, stride=1, dense_only=False):
        """``dense_only``: ``x`` holds only the dense channels (B, Cin - n_onehot, H, W) -- or is None when there are none --
        instead of the (B, Cin, H, W) concatenation with the materialised one-hot block (``LabelCond`` inputs)."""
        ctx.set_materialize_grads(False)
        label = label.contiguous()
        if x is not None:
            x = x.contiguous()
        _chk(x, label, w, b)
        d = _ids_conv_desc(label, w, stride, pad, pad_mode, act, slope)
        if dense_only and (0 if x is None else x.shape[1]) != d.Cin - n_onehot:
            raise HimError('one-hot conv: %d dense channels given, the weight expects %d'
                           % (0 if x is None else x.shape[1], d.Cin - n_onehot))
        y = torch.empty((d.B, d.Cout, d.OH, d.OW), dtype=torch.float32, device=label.device)
        nb = lib.him_conv2d_onehot_fwd_ws(ctypes.byref(d), n_onehot)
        ws = _ws(nb, label)
        fn = lib.him_conv2d_onehot_fwd_dense if dense_only else lib.him_conv2d_onehot_fwd
        fn(ctypes.byref(d), _p(label), n_onehot, _p(x), _p(w), _p(b), _p(y), _p(ws), nb, _stream())
        ctx.d, ctx.n_onehot, ctx.dense_only = d, n_onehot, bool(dense_only)
        ctx.x, ctx.label, ctx.w, ctx.b = x, label, w, b
        ctx.save_for_backward(y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 11
        if ctx.needs_input_grad[0]:
            raise HimError('one-hot stem conv has no data gradient (its input is data)')
        d, x, label, w, b = ctx.d, ctx.x, ctx.label, ctx.w, ctx.b
        bw = lib.him_conv2d_onehot_bwd_weight_dense if ctx.dense_only else lib.him_conv2d_onehot_bwd_weight
        dy = dy.contiguous()
        st = _stream()
        if d.act != ACT_NONE:
            dz = torch.empty_like(dy)
            lib.him_act_bwd(_p(ctx.saved_tensors[0]), _p(dy), _p(dz), dy.numel(), d.act, d.slope, st)
        else:
            dz = dy
        dw = db = None
        skip_w = _wkey(w) in SKIP_WGRAD
        need_w = ctx.needs_input_grad[3] and not skip_w
        need_b = b is not None and ctx.needs_input_grad[4] and not skip_w
        if need_w or need_b:
            nb = lib.him_conv2d_onehot_bwd_weight_ws(ctypes.byref(d), ctx.n_onehot)
            if need_w and _direct(w) and (not need_b or _direct(b)):
                # the range the early Adam pieces must leave alone: the weight's slot and, when the bias gradient is live
                # (dead_bias_skip off, BatchNorm in eval mode), the bias slot behind it -- run_bias_grad writes b.grad in
                # the SAME launches as w.grad, i.e. after the two events below (the early step_range(hi, total)
                # read a zeroed / partial b.grad).  A bias slot that is not the weight's neighbour: no split.
                stem_range = tuple(w._him_arena_range) if hasattr(w, '_him_arena_range') else None
                if stem_range is not None and need_b:
                    br = getattr(b, '_him_arena_range', None)
                    if br is not None and 0 <= br[0] - stem_range[1] < 64:
                        stem_range = (stem_range[0], br[1])
                    elif br is not None and 0 <= stem_range[0] - br[1] < 64:
                        stem_range = (br[0], stem_range[1])
                    else:
                        stem_range = None
                if SCHED.adam_split_stem and SCHED.wgrad_stream and stem_range is not None:
                    # A generator stem is the LAST node of a chain-shaped generator's backward pass: what the streams hold
                    # at this moment is every data gradient (current stream) and every OTHER weight gradient (weight-gradient
                    # stream) of the network.  A trainer may start the optimizer step of everything else behind these two
                    # events, next to this layer's own weight gradient (Pix2PixHDModel_condImg.optimize_parameters).
                    dev = label.device
                    cur = torch.cuda.current_stream(dev)
                    side = _WGRAD_ROUTE.get(cur.cuda_stream) or _side_stream(dev)
                    ev_main, ev_side = torch.cuda.Event(), torch.cuda.Event()
                    ev_main.record(cur)
                    ev_side.record(side)
                    _STEM_PRE[dev] = (ev_main, ev_side, stem_range, id(w))
                fork = SCHED.stem_wgrad_fork and SCHED.wgrad_stream and d.Cin > ctx.n_onehot
                if fork:
                    # the dense channels' slice (an MFMA weight gradient) + the bias gradient on THIS stream -- it has just
                    # delivered dz and, for a generator stem, has nothing left to do -- next to the label-id slice (run-length
                    # kernel, LDS-bound, 1.1 ms at C2) on the weight-gradient stream: disjoint elements of w.grad, disjoint
                    # workspace regions, a workspace each (a block of the other stream's pool may still be in use there)
                    ws_d = _ws(nb, label)
                    lib.him_conv2d_onehot_bwd_weight_part(ctypes.byref(d), _p(label), ctx.n_onehot, _p(x), int(ctx.dense_only),
                                                          _p(dz), _p(w.grad), _p(b.grad) if need_b else 0, 1, _p(ws_d), nb,
                                                          ONEHOT_PART_DENSE, st)
                    dense_done = torch.cuda.Event()
                    dense_done.record(torch.cuda.current_stream(label.device))
                with _wgrad_stream(x, dz, label):
                    ws = _ws(nb, label)
                    if fork:
                        lib.him_conv2d_onehot_bwd_weight_part(ctypes.byref(d), _p(label), ctx.n_onehot, _p(x),
                                                              int(ctx.dense_only), _p(dz), _p(w.grad), 0, 1, _p(ws), nb,
                                                              ONEHOT_PART_IDS, _stream())
                        torch.cuda.current_stream(label.device).wait_event(dense_done)   # w.grad is final behind BOTH parts
                    else:
                        bw(ctypes.byref(d), _p(label), ctx.n_onehot, _p(x), _p(dz), _p(w.grad),
                           _p(b.grad) if need_b else 0, 1, _p(ws), nb, _stream())
                    _notify(w)
                    if need_b:
                        _notify(b)
            else:
                ws = _ws(nb, label)
                dw = torch.empty_like(w) if need_w else None
                db = torch.empty_like(b) if need_b else None
                bw(ctypes.byref(d), _p(label), ctx.n_onehot, _p(x), _p(dz), _p(dw), _p(db), 0, _p(ws), nb, st)
        return None, None, None, dw, db, None, None, None, None, None, None


_STEM_PRE = {}      # device -> (event on the data-gradient stream, event on the weight-gradient stream, arena range, id(weight))


def take_stem_pre(device):
    """The events recorded in front of the LAST one-hot stem weight gradient on ``device`` (see _OneHotConv2d.backward), once."""
    return _STEM_PRE.pop(device, None)


def _ids_conv_desc(label, w, stride, pad, pad_mode, act, slope):
    """HimConv2d of a convolution whose input is [one-hot(label) | dense]: the weight names the channel count."""
    B, _, H, W = label.shape
    Cout, Cin, KH, KW = w.shape
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    return HimConv2d(B, Cin, H, W, Cout, KH, KW, stride, pad, pad_mode, OH, OW, act, slope, current_algo())


class LabelCond(object):
    """The reference's ``encode_input`` result [one-hot(label) | dense channels] (pix2pixHD_condImg_model.py:144-174 + the
    cat at :204) kept as what it is made from: the (B,1,H,W) id map and the few dense channels (edges, (1-mask)*image, colour
    embedding).  Consumers that can read ids do -- the generators' stems and (round 5) the first PatchGAN convolution
    (``_OneHotConv2d``), the pooled discriminator scales (``pooled``: 3x3 class counts) -- so the one-hot block (147 MB at
    512x256 bs 8) is neither written nor copied into the discriminator inputs; anything else calls ``full()`` (materialised
    once, cached)."""

    def __init__(self, label, n_onehot, dense=None):
        if dense is not None and dense.shape[1] == 0:
            dense = None
        self.label, self.n_onehot, self.dense = label, int(n_onehot), dense
        self._full = self._pooled = None
        self._made = {}      # 'full' / 'pooled' -> (stream that materialised it, event behind its kernels)

    @property
    def n_dense(self):
        return 0 if self.dense is None else self.dense.shape[1]

    @property
    def shape(self):
        B, _, H, W = self.label.shape
        return torch.Size((B, self.n_onehot + self.n_dense, H, W))

    @property
    def device(self):
        return self.label.device

    is_cuda, requires_grad = True, False

    def dim(self):
        return 4

    def detach(self):
        return self

    def contiguous(self):
        return self

    def record_stream(self, stream):
        for t in (self.label, self.dense, self._full, self._pooled):
            if t is not None:
                t.record_stream(stream)

    def _made_on(self, what, t):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._made[what] = (_stream(), ev)
        return t

    def _cross_stream(self, what, t):
        """A cache hit from a stream other than the one that materialised ``t`` (the first caller is the real-image
        side stream when the discriminator input is not split): order the reader behind the producer and tell the caching
        allocator about the second user -- the model's own record_stream calls ran before the buffer existed."""
        made = self._made.get(what)
        if made is not None and made[0] != _stream():
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(made[1])
            t.record_stream(cur)
        return t

    def full(self):
        """The (B, n_onehot + n_dense, H, W) tensor itself (him_onehot + one channel copy), cached."""
        if self._full is not None:
            return self._cross_stream('full', self._full)
        if self._full is None:
            B, C, H, W = self.shape
            buf = torch.empty((B, C, H, W), dtype=torch.float32, device=self.device)
            st = _stream()
            lib.him_onehot(_p(self.label), _p(buf), B, self.n_onehot, C, 0, H * W, st)
            if self.dense is not None:
                lib.him_copy_channels(_p(self.dense), self.n_dense, 0, _p(buf), C, self.n_onehot, self.n_dense, B, H * W,
                                      0, 0, 0, st)
            self._full = self._made_on('full', mark_onehot(buf, self.label, self.n_onehot))
        return self._full

    def slice(self, c0, n):
        """Channels [c0, c0 + n): a ``LabelCond`` while the slice still starts with the whole one-hot block, a tensor else."""
        if c0 == 0 and n >= self.n_onehot:
            k = n - self.n_onehot
            if k == self.n_dense:
                return self
            return LabelCond(self.label, self.n_onehot, slice_channels(self.dense, 0, k) if k else None)
        if c0 >= self.n_onehot:
            return slice_channels(self.dense, c0 - self.n_onehot, n)
        return slice_channels(self.full(), c0, n)

    def pooled(self):
        """AvgPool2d(3, 2, 1, count_include_pad=False) of the whole thing (reference Discriminator_NET.py:31-32, LocalEnhancer
        Pix2Pix_NET.py:50-53): the one-hot channels as class counts of the 3x3 windows straight from the ids
        (him_onehot_pool3s2, bit-identical to pooling the one-hot), the dense channels through the ordinary pool."""
        if self._pooled is not None:
            return self._cross_stream('pooled', self._pooled)
        if self._pooled is None:
            with torch.no_grad():
                B, C, H, W = self.shape
                OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
                out = torch.empty((B, C, OH, OW), dtype=torch.float32, device=self.device)
                st = _stream()
                lib.him_onehot_pool3s2(_p(self.label), _p(out), B, self.n_onehot, C, 0, H, W, OH, OW, st)
                if self.dense is not None:
                    pd = avgpool3s2(self.dense)
                    lib.him_copy_channels(_p(pd), self.n_dense, 0, _p(out), C, self.n_onehot, self.n_dense, B, OH * OW,
                                          0, 0, 0, st)
                self._pooled = self._made_on('pooled', out)
        return self._pooled


def mark_onehot(x, label, n_onehot):
    """Declare that channels [0, n_onehot) of ``x`` are the one-hot encoding of the id map ``label`` (B,1,H,W): the
    first convolution applied to ``x`` may then be evaluated from the ids (``_OneHotConv2d``)."""
    x._him_onehot = (label, int(n_onehot))
    return x


def conv2d(x, w, b=None, stride=1, pad=0, pad_mode='zero', act='none', slope=0.2, grad_premasked=False, gate_dx=False):
    """act(conv2d(pad(x), w) + b); pad_mode 'reflect' == nn.ReflectionPad2d(pad) + Conv2d(padding=0).

    ReLU chains (VGG) can move every activation backward into the kernel that PRODUCES the gradient: with
    ``grad_premasked`` the caller guarantees that every consumer of this layer's output multiplies the gradient it
    sends back by (output > 0) -- this layer then skips its own ReLU backward pass; ``gate_dx`` makes this layer such a
    consumer for its input (dx = (x > 0) * dgrad, in the data-gradient kernel's epilogue)."""
    if isinstance(x, LabelCond):
        pm = PAD_REFLECT if pad_mode == 'reflect' else PAD_ZERO
        d = _ids_conv_desc(x.label, w, stride, pad, pm, ACTS[act], float(slope))
        if SCHED.onehot_stem and w.shape[1] == x.shape[1] and lib.him_conv2d_onehot_fwd_ws(ctypes.byref(d), x.n_onehot):
            return _OneHotConv2d.apply(x.dense, x.label, x.n_onehot, w, b, pad, pm, ACTS[act], float(slope), int(stride), True)
        x = x.full()
    oh = getattr(x, '_him_onehot', None) if SCHED.onehot_stem else None
    if oh is not None and stride == 1 and not x.requires_grad:
        label, n_onehot = oh
        pm = PAD_REFLECT if pad_mode == 'reflect' else PAD_ZERO
        d = _conv_desc(x, w, 1, pad, pm, ACTS[act], float(slope))
        if lib.him_conv2d_onehot_fwd_ws(ctypes.byref(d), n_onehot):
            return _OneHotConv2d.apply(x, label, n_onehot, w, b, pad, pm, ACTS[act], float(slope))
    return _Conv2d.apply(x, w, b, stride, pad, PAD_REFLECT if pad_mode == 'reflect' else PAD_ZERO, ACTS[act],
                         float(slope), bool(grad_premasked), bool(gate_dx))


class CondImage(object):
    """Discriminator input handed over in two parts: ``cond`` (B,Cc,H,W: data, never differentiated -- one-hot labels,
    edges, the conditioning image) and ``image`` (B,Ci,H,W: the real / generated picture).  The reference concatenates
    them (pix2pixHD_condImg_model.py:176-182) and pools the 41-channel tensor per scale; kept apart, the pooled condition
    is computed once per step for all passes (``cond_pyramid``), and the gradient of the first PatchGAN conv comes back as
    Ci channels instead of a zero-filled (Cc+Ci)-channel tensor that the pooling / cat backward would walk again."""

    def __init__(self, cond, image):
        self.cond, self.image = cond, image

    def cat(self):
        cond = self.cond.full() if isinstance(self.cond, LabelCond) else self.cond
        return cat_channels([cond, self.image])


def cond_pyramid(cond, levels, prefill=0, image_channels=3):
    """[cond, pool(cond), pool(pool(cond)), ...] (AvgPool2d(3, 2, 1, count_include_pad=False)), cached on the tensor.
    ``prefill``: per level, that many (B, Cc + image_channels, H, W) input buffers of the first PatchGAN conv with the
    condition already copied in (``_CondImageConv2d`` takes one per pass and adds only the image channels): the 164 MB
    condition copy of the fake-image pass sat on the main stream between the generator's last conv and the first
    discriminator conv; filled here -- at the start of the step, next to the previous step's Adam pass -- it is off the
    critical path."""
    pyr = getattr(cond, '_him_pyramid', None)
    if pyr is None or len(pyr) < levels:
        with torch.no_grad():
            pyr = [cond.detach()]
            while len(pyr) < levels:
                # a LabelCond's next level comes from the ids (3x3 class counts); from there on the levels are tensors
                pyr.append(pyr[-1].pooled() if isinstance(pyr[-1], LabelCond) else avgpool3s2(pyr[-1]))
            if prefill > 0 and SCHED.d_prefill_cond:
                st = _stream()
                for c in pyr:
                    if isinstance(c, LabelCond):
                        # scale 0 reads the ids: the buffers hold [dense condition channels | image slot] only
                        B, _, H, W = c.shape
                        Cd, bufs = c.n_dense, []
                        for _ in range(prefill):
                            x = torch.empty((B, Cd + image_channels, H, W), dtype=torch.float32, device=c.device)
                            if Cd:
                                lib.him_copy_channels(_p(c.dense), Cd, 0, _p(x), Cd + image_channels, 0, Cd, B, H * W, 0, 0,
                                                      0, st)
                            bufs.append(x)
                        c._him_prefilled = bufs
                        continue
                    B, Cc, H, W = c.shape
                    bufs = []
                    for _ in range(prefill):
                        x = torch.empty((B, Cc + image_channels, H, W), dtype=torch.float32, device=c.device)
                        lib.him_copy_channels(_p(c), Cc, 0, _p(x), Cc + image_channels, 0, Cc, B, H * W, 0, 0, 0, st)
                        bufs.append(x)
                    c._him_prefilled = bufs
        cond._him_pyramid = pyr
    return pyr


class _CondImageConv2d(torch.autograd.Function):
    """act(conv2d([cond | image], w) + b), zero padding; gradient to ``image`` (and the parameters) only."""

    @staticmethod
    def forward(ctx, cond, image, w, b, stride, pad, act, slope):
        ctx.set_materialize_grads(False)
        cond, image = cond.contiguous(), image.contiguous()
        _chk(cond, image, w, b)
        B, Cc, H, W = cond.shape
        Ci = image.shape[1]
        if image.shape[0] != B or tuple(image.shape[2:]) != (H, W):
            raise HimError('cond/image conv: shapes %s and %s do not stack' % (tuple(cond.shape), tuple(image.shape)))
        st = _stream()
        pre = getattr(cond, '_him_prefilled', None)
        if pre and tuple(pre[-1].shape) == (B, Cc + Ci, H, W):
            x = pre.pop()                  # condition channels filled by cond_pyramid at the start of the step
            x.record_stream(torch.cuda.current_stream(x.device))
        else:
            x = torch.empty((B, Cc + Ci, H, W), dtype=torch.float32, device=cond.device)
            lib.him_copy_channels(_p(cond), Cc, 0, _p(x), Cc + Ci, 0, Cc, B, H * W, 0, 0, 0, st)
        lib.him_copy_channels(_p(image), Ci, 0, _p(x), Cc + Ci, Cc, Ci, B, H * W, 0, 0, 0, st)
        d = _conv_desc(x, w, stride, pad, PAD_ZERO, act, slope)
        y = torch.empty((d.B, d.Cout, d.OH, d.OW), dtype=torch.float32, device=x.device)
        nb = lib.him_conv2d_fwd_ws(ctypes.byref(d))
        ws = _ws(nb, x)
        pan = _panel(w, d, PANEL_FWD, False)
        if pan:
            lib.him_conv2d_fwd_panel(ctypes.byref(d), _p(x), pan, _p(b), _p(y), _p(ws), nb, st)
        else:
            lib.him_conv2d_fwd(ctypes.byref(d), _p(x), _p(w), _p(b), _p(y), _p(ws), nb, st)
        ctx.d, ctx.Cc, ctx.Ci = d, Cc, Ci
        ctx.x, ctx.w, ctx.b = x, w, b
        ctx.save_for_backward(y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 8
        d, x, w, b, Cc, Ci = ctx.d, ctx.x, ctx.w, ctx.b, ctx.Cc, ctx.Ci
        dy = dy.contiguous()
        st = _stream()
        if d.act != ACT_NONE:
            dz = torch.empty_like(dy)
            lib.him_act_bwd(_p(ctx.saved_tensors[0]), _p(dy), _p(dz), dy.numel(), d.act, d.slope, st)
        else:
            dz = dy
        dimg = dw = db = None
        if ctx.needs_input_grad[1] and _wkey(w) not in SKIP_DGRAD:
            d2 = HimConv2d.from_buffer_copy(d)
            d2.Cin = Ci
            dimg = torch.empty((d.B, Ci, d.H, d.W), dtype=torch.float32, device=x.device)
            wsl = w.detach()[:, Cc:].contiguous()
            nb = lib.him_conv2d_bwd_data_ws(ctypes.byref(d2))
            ws = _ws(nb, x)
            lib.him_conv2d_bwd_data(ctypes.byref(d2), _p(dz), _p(wsl), _p(dimg), _p(ws), nb, st)
        skip_w = _wkey(w) in SKIP_WGRAD
        need_w = ctx.needs_input_grad[2] and not skip_w
        need_b = b is not None and ctx.needs_input_grad[3] and not skip_w
        if need_w or need_b:
            nb = lib.him_conv2d_bwd_weight_ws(ctypes.byref(d))
            if need_w and _direct(w) and (not need_b or _direct(b)):
                with _wgrad_stream(x, dz, weight=w):
                    ws = _ws(nb, x)
                    lib.him_conv2d_bwd_weight(ctypes.byref(d), _p(x), _p(dz), _p(w.grad),
                                              _p(b.grad) if need_b else 0, 1, _p(ws), nb, _stream())
                    _notify(w)
                    if need_b:
                        _notify(b)
            else:
                ws = _ws(nb, x)
                dw = torch.empty_like(w) if need_w else None
                db = torch.empty_like(b) if need_b else None
                lib.him_conv2d_bwd_weight(ctypes.byref(d), _p(x), _p(dz), _p(dw), _p(db), 0, _p(ws), nb, st)
        return None, dimg, dw, db, None, None, None, None


class _IdsCondImageConv2d(torch.autograd.Function):
    """act(conv2d([one-hot(label) | dense condition | image], w) + b), zero padding, with the one-hot block read from the
    ids (reference: the first nn.Conv2d of every NLayerDiscriminator, Discriminator_NET.py:71-74, on the concatenation of
    pix2pixHD_condImg_model.py:176-186): forward = table lookups + the (dense condition | image) channels as an ordinary
    few-channel conv; weight gradient = run-length sums over the label rows + the few-channel weight gradient; data gradient
    to the image channels only (the 3-channel weight slice, as ``_CondImageConv2d``)."""

    @staticmethod
    def forward(ctx, cond, image, w, b, stride, pad, act, slope):
        ctx.set_materialize_grads(False)
        image = image.contiguous()
        _chk(image, w, b)
        B, _, H, W = cond.shape
        Cd, Ci, NC = cond.n_dense, image.shape[1], cond.n_onehot
        if image.shape[0] != B or tuple(image.shape[2:]) != (H, W):
            raise HimError('cond/image conv: shapes %s and %s do not stack' % (tuple(cond.shape), tuple(image.shape)))
        st = _stream()
        pre = getattr(cond, '_him_prefilled', None)
        if pre and tuple(pre[-1].shape) == (B, Cd + Ci, H, W):
            x = pre.pop()                  # dense condition channels filled by cond_pyramid at the start of the step
            x.record_stream(torch.cuda.current_stream(x.device))
        else:
            x = torch.empty((B, Cd + Ci, H, W), dtype=torch.float32, device=image.device)
            if Cd:
                lib.him_copy_channels(_p(cond.dense), Cd, 0, _p(x), Cd + Ci, 0, Cd, B, H * W, 0, 0, 0, st)
        lib.him_copy_channels(_p(image), Ci, 0, _p(x), Cd + Ci, Cd, Ci, B, H * W, 0, 0, 0, st)
        label = cond.label
        d = _ids_conv_desc(label, w, stride, pad, PAD_ZERO, act, slope)
        y = torch.empty((d.B, d.Cout, d.OH, d.OW), dtype=torch.float32, device=x.device)
        nb = lib.him_conv2d_onehot_fwd_ws(ctypes.byref(d), NC)
        ws = _ws(nb, x)
        lib.him_conv2d_onehot_fwd_dense(ctypes.byref(d), _p(label), NC, _p(x), _p(w), _p(b), _p(y), _p(ws), nb, st)
        ctx.d, ctx.NC, ctx.Cc, ctx.Ci = d, NC, NC + Cd, Ci
        ctx.x, ctx.label, ctx.w, ctx.b = x, label, w, b
        ctx.save_for_backward(y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 8
        d, x, label, w, b, Cc, Ci = ctx.d, ctx.x, ctx.label, ctx.w, ctx.b, ctx.Cc, ctx.Ci
        dy = dy.contiguous()
        st = _stream()
        if d.act != ACT_NONE:
            dz = torch.empty_like(dy)
            lib.him_act_bwd(_p(ctx.saved_tensors[0]), _p(dy), _p(dz), dy.numel(), d.act, d.slope, st)
        else:
            dz = dy
        dimg = dw = db = None
        if ctx.needs_input_grad[1] and _wkey(w) not in SKIP_DGRAD:
            d2 = HimConv2d.from_buffer_copy(d)
            d2.Cin = Ci
            dimg = torch.empty((d.B, Ci, d.H, d.W), dtype=torch.float32, device=x.device)
            wsl = w.detach()[:, Cc:].contiguous()
            nb = lib.him_conv2d_bwd_data_ws(ctypes.byref(d2))
            ws = _ws(nb, x)
            lib.him_conv2d_bwd_data(ctypes.byref(d2), _p(dz), _p(wsl), _p(dimg), _p(ws), nb, st)
        skip_w = _wkey(w) in SKIP_WGRAD
        need_w = ctx.needs_input_grad[2] and not skip_w
        need_b = b is not None and ctx.needs_input_grad[3] and not skip_w
        if need_w or need_b:
            nb = lib.him_conv2d_onehot_bwd_weight_ws(ctypes.byref(d), ctx.NC)
            if need_w and _direct(w) and (not need_b or _direct(b)):
                with _wgrad_stream(x, dz, label):
                    ws = _ws(nb, x)
                    lib.him_conv2d_onehot_bwd_weight_dense(ctypes.byref(d), _p(label), ctx.NC, _p(x), _p(dz), _p(w.grad),
                                                           _p(b.grad) if need_b else 0, 1, _p(ws), nb, _stream())
                    _notify(w)
                    if need_b:
                        _notify(b)
            else:
                ws = _ws(nb, x)
                dw = torch.empty_like(w) if need_w else None
                db = torch.empty_like(b) if need_b else None
                lib.him_conv2d_onehot_bwd_weight_dense(ctypes.byref(d), _p(label), ctx.NC, _p(x), _p(dz), _p(dw), _p(db), 0,
                                                       _p(ws), nb, st)
        return None, dimg, dw, db, None, None, None, None


def cond_image_conv2d(cond, image, w, b=None, stride=1, pad=0, act='none', slope=0.2):
    """The first PatchGAN convolution on a ``CondImage`` pair (see there)."""
    if isinstance(cond, LabelCond):
        d = _ids_conv_desc(cond.label, w, stride, pad, PAD_ZERO, ACTS[act], float(slope))
        if (SCHED.d_from_ids and w.shape[1] == cond.shape[1] + image.shape[1]
                and lib.him_conv2d_onehot_fwd_ws(ctypes.byref(d), cond.n_onehot)):
            return _IdsCondImageConv2d.apply(cond, image, w, b, stride, pad, ACTS[act], float(slope))
        cond = cond.full()
    return _CondImageConv2d.apply(cond, image, w, b, stride, pad, ACTS[act], float(slope))


class _Deconv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad, out_pad, act, slope):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        x = x.contiguous()
        _chk(x, w, b)
        B, Cin, H, W = x.shape
        Cin2, Cout, KH, KW = w.shape
        if Cin2 != Cin:
            raise HimError('deconv2d: weight expects %d input channels, got %d' % (Cin2, Cin))
        OH = (H - 1) * stride - 2 * pad + KH + out_pad
        OW = (W - 1) * stride - 2 * pad + KW + out_pad
        d = HimDeconv2d(B, Cin, H, W, Cout, KH, KW, stride, pad, out_pad, OH, OW, act, slope, current_algo())
        y = torch.empty((B, Cout, OH, OW), dtype=torch.float32, device=x.device)
        nb = lib.him_deconv2d_fwd_ws(ctypes.byref(d))
        ws = _ws(nb, x)
        pan = _panel(w, d, PANEL_FWD, True)
        if pan:
            lib.him_deconv2d_fwd_panel(ctypes.byref(d), _p(x), pan, _p(b), _p(y), _p(ws), nb, _stream())
        else:
            lib.him_deconv2d_fwd(ctypes.byref(d), _p(x), _p(w), _p(b), _p(y), _p(ws), nb, _stream())
        ctx.d = d
        ctx.x, ctx.w, ctx.b = x, w, b
        ctx.gslice = getattr(x, '_him_grad_slice', None)
        # the OUTPUT must go through save_for_backward: a plain ctx attribute closes a tensor -> grad_fn -> ctx -> tensor
        # cycle through C++ that no collector sees, and with it the whole upstream graph of every step leaks
        ctx.save_for_backward(y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 8
        d, x, w, b = ctx.d, ctx.x, ctx.w, ctx.b
        dy = dy.contiguous()
        st = _stream()
        if d.act != ACT_NONE:
            dz = torch.empty_like(dy)
            lib.him_act_bwd(_p(ctx.saved_tensors[0]), _p(dy), _p(dz), dy.numel(), d.act, d.slope, st)
        else:
            dz = dy
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            nb = lib.him_deconv2d_bwd_data_ws(ctypes.byref(d))
            ws = _ws(nb, x)
            pan = _panel(w, d, PANEL_BWD_DATA, True)
            if pan:
                lib.him_deconv2d_bwd_data_panel(ctypes.byref(d), _p(dz), pan, _p(dx), _p(ws), nb, st)
            else:
                lib.him_deconv2d_bwd_data(ctypes.byref(d), _p(dz), _p(w), _p(dx), _p(ws), nb, st)
        need_w = ctx.needs_input_grad[1]
        need_b = b is not None and ctx.needs_input_grad[2]
        if need_w or need_b:
            nb = lib.him_deconv2d_bwd_weight_ws(ctypes.byref(d))
            if need_w and _direct(w) and (not need_b or _direct(b)):
                with _wgrad_stream(x, dz, weight=w):
                    ws = _ws(nb, x)
                    lib.him_deconv2d_bwd_weight(ctypes.byref(d), _p(x), _p(dz), _p(w.grad),
                                                _p(b.grad) if need_b else 0, 1, _p(ws), nb, _stream())
                    _notify(w)
                    if need_b:
                        _notify(b)
            else:
                ws = _ws(nb, x)
                dw = torch.empty_like(w) if need_w else None
                db = torch.empty_like(b) if need_b else None
                lib.him_deconv2d_bwd_weight(ctypes.byref(d), _p(x), _p(dz), _p(dw), _p(db), 0, _p(ws), nb, st)
        return dx, dw, db, None, None, None, None, None


def conv_transpose2d(x, w, b=None, stride=2, pad=1, out_pad=1, act='none', slope=0.2):
    return _Deconv2d.apply(x, w, b, stride, pad, out_pad, ACTS[act], float(slope))


# ------------------------------------------------------------------------------------------------
# ResnetBlock with both InstanceNorms fused into the Winograd transforms (include/him.h "ResnetBlock")
# ------------------------------------------------------------------------------------------------
class _ResBlock(torch.autograd.Function):
    """out = x + IN(conv3(refpad(relu(IN(conv3(refpad(x)))))))  (reference models/layer_util.py:333-378) as ONE node:
    7 launches forward (two input transforms -- the second normalises on load --, two batched GEMMs, two output
    transforms that reduce the plane statistics), no normalised intermediate in HBM; backward applies the ReLU gate and
    the InstanceNorm backward inside the data gradient's output transform and adds the skip gradient in the last one.
    The conv biases feed an InstanceNorm (zero true gradient): they take part in the forward only."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, eps):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        _chk(x, w1, b1, w2, b2)
        B, Cn, H, W = x.shape
        d = HimResBlock(B, Cn, H, W, eps, current_algo())
        cd = _conv_desc(x, w1, 1, 1, PAD_REFLECT, ACT_NONE, 0.0)
        p1, p2 = _panel(w1, cd, PANEL_FWD, False), _panel(w2, cd, PANEL_FWD, False)
        if not p1 or not p2:
            raise HimError('fused ResnetBlock needs cached weight panels (nn.Parameter weights)')
        y1, y2, out = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        st1 = torch.empty(2 * B * Cn, dtype=torch.float32, device=x.device)
        st2 = torch.empty_like(st1)
        nb = lib.him_resblock_ws(ctypes.byref(d))
        ws = _ws(nb, x)
        lib.him_resblock_fwd(ctypes.byref(d), _p(x), p1, _p(b1), p2, _p(b2), _p(y1), _p(st1), _p(y2), _p(st2), _p(out),
                             _p(ws), nb, _stream())
        ctx.d, ctx.cd = d, cd
        ctx.x, ctx.w1, ctx.w2 = x, w1, w2
        ctx.save_for_backward(y1, st1, y2, st2)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 6
        g = g.contiguous()
        d, cd, x, w1, w2 = ctx.d, ctx.cd, ctx.x, ctx.w1, ctx.w2
        y1, st1, y2, st2 = ctx.saved_tensors
        q1, q2 = _panel(w1, cd, PANEL_BWD_DATA, False), _panel(w2, cd, PANEL_BWD_DATA, False)
        dy2, dy1 = torch.empty_like(x), torch.empty_like(x)
        dx = torch.empty_like(x)
        nb = lib.him_resblock_ws(ctypes.byref(d))
        ws = _ws(nb, x)
        lib.him_resblock_bwd_data(ctypes.byref(d), _p(g), _p(y1), _p(st1), _p(y2), _p(st2), q1, q2, _p(dy2), _p(dy1), _p(dx),
                                  _p(ws), nb, _stream())
        dws = [None, None]
        nbw = lib.him_resblock_bwd_weight_ws(ctypes.byref(d))
        for i, (w, src, stat, dy) in enumerate(((w2, y1, st1, dy2), (w1, x, None, dy1))):
            which = 2 - i
            if not ctx.needs_input_grad[1 if which == 1 else 3] or _wkey(w) in SKIP_WGRAD:
                continue
            if _direct(w):
                with _wgrad_stream(src, dy, stat):
                    wsw = _ws(nbw, x)
                    lib.him_resblock_bwd_weight(ctypes.byref(d), which, _p(src), _p(stat), _p(dy), _p(w.grad), 1, _p(wsw), nbw,
                                                _stream())
                    _notify(w)
            else:
                wsw = _ws(nbw, x)
                dw = torch.empty_like(w)
                lib.him_resblock_bwd_weight(ctypes.byref(d), which, _p(src), _p(stat), _p(dy), _p(dw), 0, _p(wsw), nbw, _stream())
                dws[which - 1] = dw
        return (dx if ctx.needs_input_grad[0] else None), dws[0], None, dws[1], None, None


# Off by default since round 3's 64x128 conv tiles: inside the multi-stream step the layer-by-layer block is 0.4 ms
# faster (59.6 vs 60.0 ms, three repetitions each, profiles/r03_tile_shape_ab.txt) although the fused unit launches
# fewer kernels and moves fewer bytes; HIM_RESBLOCK_FUSED=1 turns it on, tests/test_ops_gpu.py keeps it pinned.


def resblock_supported(x, w1, w2):
    """True when ``resnet_block`` can take (x, w1, w2): CUDA fp32, nn.Parameter weights (cached panels) and a shape in
    the separate-transform Winograd range (him_resblock_supported)."""
    if not (SCHED.resblock_fused and SCHED.panel_cache and x.is_cuda and x.dim() == 4 and isinstance(w1, torch.nn.Parameter)
            and isinstance(w2, torch.nn.Parameter)):
        return False
    B, Cn, H, W = x.shape
    if tuple(w1.shape) != (Cn, Cn, 3, 3) or tuple(w2.shape) != (Cn, Cn, 3, 3):
        return False
    return bool(lib.him_resblock_supported(ctypes.byref(HimResBlock(B, Cn, H, W, 1e-5, current_algo()))))


def resnet_block(x, w1, b1, w2, b2, eps=1e-5):
    """x + IN(conv3x3(refpad(relu(IN(conv3x3(refpad(x), w1, b1)))), w2, b2)) with the norms fused into the convolutions'
    Winograd transforms; b1 / b2 (in front of an InstanceNorm: zero true gradient) are used as data."""
    return _ResBlock.apply(x, w1, None if b1 is None else b1.detach(), w2, None if b2 is None else b2.detach(), float(eps))


# ------------------------------------------------------------------------------------------------
# instance norm (+activation, +residual)
# ------------------------------------------------------------------------------------------------
class _InstNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, act, slope, eps):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        x = x.contiguous()
        if residual is not None:
            residual = residual.contiguous()
        _chk(x, residual)
        B, Cn, H, W = x.shape
        planes, hw = B * Cn, H * W
        y = torch.empty_like(x)
        mean = torch.empty(planes, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        lib.him_instnorm_fwd(_p(x), _p(residual), _p(y), _p(mean), _p(rstd), planes, hw, eps, act, slope, _stream())
        ctx.x, ctx.mean, ctx.rstd = x, mean, rstd
        ctx.cfg = (planes, hw, act, slope)
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 5
        dy = dy.contiguous()
        planes, hw, act, slope = ctx.cfg
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(ctx.x)
            lib.him_instnorm_bwd(_p(ctx.x), _p(ctx.mean), _p(ctx.rstd), _p(dy), _p(dx), planes, hw, act, slope,
                                 _stream())
        dres = dy if (ctx.has_res and ctx.needs_input_grad[1]) else None
        return dx, dres, None, None, None


class _Conv2dIN(torch.autograd.Function):
    """act(InstanceNorm2d(conv2d(pad(x), w) + b)) [+ residual] through him_conv2d_in_act_fwd (include/him.h): taken for
    the descriptors whose forward is a split-K launch -- the InstanceNorm kernel reads the split-K slabs, the finish pass
    disappears; outputs bit-identical to conv2d + instance_norm.  Backward = InstanceNorm backward, then _Conv2d's."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, pad_mode, eps, act, slope, residual):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        if residual is not None:
            residual = residual.contiguous()
        _chk(x, w, b, residual)
        d = _conv_desc(x, w, stride, pad, pad_mode, ACT_NONE, 0.0)
        y = torch.empty((d.B, d.Cout, d.OH, d.OW), dtype=torch.float32, device=x.device)
        z = torch.empty_like(y)
        planes, hw = d.B * d.Cout, d.OH * d.OW
        mean = torch.empty(planes, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        nb = lib.him_conv2d_fwd_ws(ctypes.byref(d))
        ws = _ws(nb, x)
        pan = _panel(w, d, PANEL_FWD, False)
        lib.him_conv2d_in_act_fwd(ctypes.byref(d), _p(x), 0 if pan else _p(w), pan or 0, _p(b), _p(y), _p(residual), _p(z),
                                  _p(mean), _p(rstd), eps, act, slope, _p(ws), nb, _stream())
        # the fields _Conv2d.backward reads
        ctx.d, ctx.x, ctx.w, ctx.b, ctx.keep = d, x, w, b, None
        ctx.premasked, ctx.gate_dx = False, False
        ctx.gslice = getattr(x, '_him_grad_slice', None)
        ctx.cfg = (planes, hw, act, slope)
        ctx.has_res = residual is not None
        ctx.save_for_backward(y, mean, rstd)
        return z

    @staticmethod
    def backward(ctx, dz):
        if dz is None:
            return (None,) * 10
        dz = dz.contiguous()
        y, mean, rstd = ctx.saved_tensors
        planes, hw, act, slope = ctx.cfg
        dy = torch.empty_like(y)
        lib.him_instnorm_bwd(_p(y), _p(mean), _p(rstd), _p(dz), _p(dy), planes, hw, act, slope, _stream())
        dx, dw, db = _Conv2d.backward(ctx, dy)[:3]
        dres = dz if (ctx.has_res and ctx.needs_input_grad[9]) else None
        return dx, dw, db, None, None, None, None, None, None, dres


def conv2d_in_act(x, w, b=None, stride=1, pad=0, pad_mode='zero', eps=1e-5, act='none', slope=0.2, residual=None):
    """act(InstanceNorm2d(affine=False)(conv2d(pad(x), w) + b)) [+ residual]: ONE library call
    (him_conv2d_in_act_fwd) where the convolution is a split-K launch, conv2d + instance_norm otherwise."""
    pm = PAD_REFLECT if pad_mode == 'reflect' else PAD_ZERO
    if (SCHED.conv_in_fused and not isinstance(x, LabelCond) and getattr(x, '_him_onehot', None) is None
            and not getattr(w, '_him_frozen', False)):
        d = _conv_desc(x, w, stride, pad, pm, ACT_NONE, 0.0)
        if lib.him_conv2d_in_act_fused(ctypes.byref(d)):
            return _Conv2dIN.apply(x, w, b, stride, pad, pm, float(eps), ACTS[act], float(slope), residual)
    return instance_norm(conv2d(x, w, b, stride, pad, pad_mode, 'none', slope), residual, act, slope, eps)


def instance_norm(x, residual=None, act='none', slope=0.2, eps=1e-5):
    """act(InstanceNorm2d(affine=False)(x)) [+ residual]."""
    return _InstNorm.apply(x, residual, ACTS[act], float(slope), float(eps))


# ------------------------------------------------------------------------------------------------
# box2mask building blocks: BatchNorm2d, stand-alone activation, bilinear x2, channel log-softmax, mask losses
# ------------------------------------------------------------------------------------------------
class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, gamma, beta, run_mean, run_var, training, momentum, eps, act, slope):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        if residual is not None:
            residual = residual.contiguous()
        _chk(x, residual, gamma, beta, run_mean, run_var)
        B, Cn, H, W = x.shape
        y = torch.empty_like(x)
        mean = torch.empty(Cn, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        nb = lib.him_batchnorm_ws(Cn)
        ws = _ws(nb, x)
        lib.him_batchnorm_fwd(_p(x), _p(residual), _p(gamma), _p(beta), _p(run_mean), _p(run_var), _p(y), _p(mean),
                              _p(rstd), B, Cn, H * W, eps, momentum, 1 if training else 0, act, slope, _p(ws), nb, _stream())
        ctx.x, ctx.gamma, ctx.beta, ctx.mean, ctx.rstd = x, gamma, beta, mean, rstd
        ctx.cfg = (B, Cn, H * W, bool(training), act, slope)
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * 11
        dy = dy.contiguous()
        B, Cn, hw, training, act, slope = ctx.cfg
        x, gamma, beta = ctx.x, ctx.gamma, ctx.beta
        need_x = ctx.needs_input_grad[0]
        need_g = gamma is not None and ctx.needs_input_grad[2]
        need_b = beta is not None and ctx.needs_input_grad[3]
        dx = torch.empty_like(x) if need_x else None
        nb = lib.him_batchnorm_ws(Cn)
        ws = _ws(nb, x)
        direct = need_g and need_b and _direct(gamma) and _direct(beta)
        if direct:
            dg, db = gamma.grad, beta.grad
        else:
            dg = torch.empty_like(gamma) if need_g else None
            db = torch.empty_like(beta) if need_b else None
        lib.him_batchnorm_bwd(_p(x), _p(gamma), _p(beta), _p(ctx.mean), _p(ctx.rstd), _p(dy), _p(dx), _p(dg), _p(db), B, Cn,
                              hw, 1 if training else 0, act, slope, 1 if direct else 0, _p(ws), nb, _stream())
        if direct:
            _notify(gamma)
            _notify(beta)
            dg = db = None
        dres = dy if (ctx.has_res and ctx.needs_input_grad[1]) else None
        return dx, dres, dg, db, None, None, None, None, None, None, None


def batch_norm(x, gamma, beta, run_mean, run_var, training=True, momentum=0.1, eps=1e-5, act='none', slope=0.2,
               residual=None):
    """act(BatchNorm2d(x)) [+ residual]; training mode updates run_mean / run_var in place (torch semantics)."""
    return _BatchNorm.apply(x, residual, gamma, beta, run_mean, run_var, bool(training), float(momentum), float(eps),
                            ACTS[act], float(slope))


class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act, slope):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        _chk(x)
        y = torch.empty_like(x)
        lib.him_act_fwd(_p(x), _p(y), x.numel(), act, slope, _stream())
        ctx.cfg = (act, slope)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None, None, None
        dy = dy.contiguous()
        (y,) = ctx.saved_tensors
        dz = torch.empty_like(dy)
        lib.him_act_bwd(_p(y), _p(dy), _p(dz), dy.numel(), ctx.cfg[0], ctx.cfg[1], _stream())
        return dz, None, None


def activation(x, act, slope=0.2):
    """stand-alone nn.ReLU / LeakyReLU / Tanh / Sigmoid (out of place)."""
    return _Act.apply(x, ACTS[act], float(slope))


class _Upsample2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, align):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        _chk(x)
        B, Cn, H, W = x.shape
        y = torch.empty((B, Cn, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
        lib.him_upsample2_fwd(_p(x), _p(y), B * Cn, H, W, align, _stream())
        ctx.cfg = (B * Cn, H, W, align)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None, None
        dy = dy.contiguous()
        planes, H, W, align = ctx.cfg
        dx = torch.empty((dy.shape[0], dy.shape[1], H, W), dtype=torch.float32, device=dy.device)
        lib.him_upsample2_bwd(_p(dy), _p(dx), planes, H, W, align, _stream())
        return dx, None


def upsample_bilinear2(x, align_corners=False):
    """nn.Upsample(scale_factor=2, mode='bilinear')."""
    return _Upsample2.apply(x, 1 if align_corners else 0)


class _LogSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        _chk(x)
        B, Cn, H, W = x.shape
        y = torch.empty_like(x)
        lib.him_logsoftmax_fwd(_p(x), _p(y), B, Cn, H * W, _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None
        dy = dy.contiguous()
        (y,) = ctx.saved_tensors
        B, Cn, H, W = y.shape
        dx = torch.empty_like(y)
        lib.him_logsoftmax_bwd(_p(y), _p(dy), _p(dx), B, Cn, H * W, _stream())
        return dx


def log_softmax_channels(x):
    """nn.LogSoftmax(dim=1) on a (B,C,H,W) tensor."""
    return _LogSoftmax.apply(x)


class _GateComb(torch.autograd.Function):
    """(1 - p) * ctx + p * obj, p and obj (B,1,H,W) broadcast over ctx's channels (MaskTwoStreamConv_NET.py:213-221)."""

    @staticmethod
    def forward(ctx_, ctx, p, obj):
        ctx, p, obj = ctx.contiguous(), p.contiguous(), obj.contiguous()
        _chk(ctx, p, obj)
        B, C, H, W = ctx.shape
        if p.shape != (B, 1, H, W) or obj.shape != (B, 1, H, W):
            raise ValueError('gate_comb: gate / object logits must be (B,1,H,W)')
        out = torch.empty_like(ctx)
        lib.him_gate_comb_fwd(_p(ctx), _p(p), _p(obj), _p(out), B, C, H * W, _stream())
        ctx_.save_for_backward(ctx, p, obj)
        return out

    @staticmethod
    def backward(ctx_, dout):
        ctx, p, obj = ctx_.saved_tensors
        dout = dout.contiguous()
        B, C, H, W = ctx.shape
        dctx, dp, dobj = torch.empty_like(ctx), torch.empty_like(p), torch.empty_like(obj)
        lib.him_gate_comb_bwd(_p(ctx), _p(p), _p(obj), _p(dout), _p(dctx), _p(dp), _p(dobj), B, C, H * W, _stream())
        return dctx, dp, dobj


def gate_comb(ctx_logit, gate, obj_logit):
    return _GateComb.apply(ctx_logit, gate, obj_logit)


class _MaskedNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, label, mask):
        ctx.set_materialize_grads(False)
        logp, label, mask = logp.contiguous(), label.contiguous(), mask.contiguous()
        _chk(logp, label, mask)
        B, Cn, H, W = logp.shape
        out2 = torch.empty(2, dtype=torch.float32, device=logp.device)
        nb = lib.him_mask_loss_ws()
        ws = _ws(nb, logp)
        lib.him_masked_nll_fwd(_p(logp), _p(label), _p(mask), _p(out2), B, Cn, H * W, _p(ws), nb, _stream())
        ctx.label, ctx.mask, ctx.count, ctx.shape = label, mask, out2[1:2], (B, Cn, H, W)
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        B, Cn, H, W = ctx.shape
        g = g.contiguous()
        d = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        lib.him_masked_nll_bwd(_p(ctx.label), _p(ctx.mask), _p(g), _p(ctx.count), _p(d), B, Cn, H * W, _stream())
        return d, None, None


def masked_nll(logp, label, mask):
    """MaskReconLoss: NLLLoss2d(ignore_index) of log-probabilities (B,C,H,W) against the id map ``label`` (B,1,H,W or
    B,H,W, ids as floats) with the positions where ``mask`` < 0.5 ignored; mean over the valid positions."""
    return _MaskedNLL.apply(logp, label.detach(), mask.detach())


class _BCEMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t):
        ctx.set_materialize_grads(False)
        p, t = p.contiguous(), t.contiguous()
        _chk(p, t)
        if p.shape != t.shape:
            raise HimError('bce: shape mismatch %s vs %s' % (tuple(p.shape), tuple(t.shape)))
        out = torch.empty((), dtype=torch.float32, device=p.device)
        nb = lib.him_mask_loss_ws()
        ws = _ws(nb, p)
        lib.him_bce_mean_fwd(_p(p), _p(t), p.numel(), _p(out), _p(ws), nb, _stream())
        ctx.p, ctx.t = p, t
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        g = g.contiguous()
        dp = torch.empty_like(ctx.p)
        lib.him_bce_mean_bwd(_p(ctx.p), _p(ctx.t), ctx.p.numel(), _p(g), _p(dp), _stream())
        return dp, None


def bce_mean(p, t):
    """nn.BCELoss()(p, t.detach())."""
    return _BCEMean.apply(p, t.detach())


class _SpaceBatch(torch.autograd.Function):
    """inverse = 0: (B,C,H,W) -> (B*d*d, C, H/d, W/d) phase images; inverse = 1: back.  A permutation: its adjoint is its
    inverse."""

    @staticmethod
    def forward(ctx, x, d, inverse):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        _chk(x)
        if inverse:
            Bd, Cn, Hd, Wd = x.shape
            B, H, W = Bd // (d * d), Hd * d, Wd * d
            y = torch.empty((B, Cn, H, W), dtype=torch.float32, device=x.device)
        else:
            B, Cn, H, W = x.shape
            y = torch.empty((B * d * d, Cn, H // d, W // d), dtype=torch.float32, device=x.device)
        lib.him_space_to_batch(_p(x), _p(y), B, Cn, H, W, d, inverse, _stream())
        ctx.cfg = (d, inverse)
        return y

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        d, inverse = ctx.cfg
        return _SpaceBatch.apply(g, d, 0 if inverse else 1), None, None


def dilated_conv3x3(x, w, dilation):
    """nn.Conv2d(k=3, stride=1, padding=dilation, dilation=dilation, bias=False) (reference conv3x3,
    models/layer_util.py:254-256) = the plain pad-1 conv on the dilation^2 phase images of x."""
    d = int(dilation)
    if d == 1:
        return conv2d(x, w, None, 1, 1, 'zero', 'none')
    if x.shape[2] % d or x.shape[3] % d:
        raise HimError('dilated conv: plane %dx%d is not divisible by the dilation %d' % (x.shape[2], x.shape[3], d))
    return _SpaceBatch.apply(conv2d(_SpaceBatch.apply(x, d, 0), w, None, 1, 1, 'zero', 'none'), d, 1)


def lr_control(loss_d_real, loss_d_fake, margin=0.3):
    """(g_lr, d_lr) device scalars in {0., 1.} (reference models/Discriminator_NET.py:190-211), no host read-back."""
    a, b = loss_d_real.detach().reshape(1).contiguous(), loss_d_fake.detach().reshape(1).contiguous()
    _chk(a, b)
    out = torch.empty(2, dtype=torch.float32, device=a.device)
    lib.him_lr_control(_p(a), _p(b), float(margin), _p(out), _stream())
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------
# pooling
# ------------------------------------------------------------------------------------------------
class _AvgPool3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        x = x.contiguous()
        _chk(x)
        B, Cn, H, W = x.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = torch.empty((B, Cn, OH, OW), dtype=torch.float32, device=x.device)
        lib.him_avgpool3s2_fwd(_p(x), _p(y), B * Cn, H, W, OH, OW, _stream())
        ctx.shape = (B, Cn, H, W, OH, OW)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None
        B, Cn, H, W, OH, OW = ctx.shape
        dy = dy.contiguous()
        dx = torch.empty((B, Cn, H, W), dtype=torch.float32, device=dy.device)
        lib.him_avgpool3s2_bwd(_p(dy), _p(dx), B * Cn, H, W, OH, OW, _stream())
        return dx


def avgpool3s2(x):
    """nn.AvgPool2d(3, stride=2, padding=1, count_include_pad=False)."""
    if isinstance(x, LabelCond):
        return x.pooled()
    y = _AvgPool3s2.apply(x)
    gs = getattr(x, '_him_grad_slice', None)
    if gs is not None:
        y._him_grad_slice = gs      # channel-wise op: the same slice is the only one that needs a gradient
    return y


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, relu_gate=False):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        x = x.contiguous()
        _chk(x)
        B, Cn, H, W = x.shape
        y = torch.empty((B, Cn, H // k, W // k), dtype=torch.float32, device=x.device)
        lib.him_maxpool_fwd(_p(x), _p(y), B * Cn, H, W, k, _stream())
        ctx.x, ctx.k, ctx.relu_gate = x, k, bool(relu_gate)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None, None, None
        x, k = ctx.x, ctx.k
        B, Cn, H, W = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        (lib.him_maxpool_relu_bwd if ctx.relu_gate else lib.him_maxpool_bwd)(_p(x), _p(dy), _p(dx), B * Cn, H, W, k,
                                                                            _stream())
        return dx, None, None


def maxpool(x, k, relu_gate=False):
    """``relu_gate``: x is the output of a ReLU layer that was told its gradient arrives gated (conv2d's
    ``grad_premasked``): the pool's backward applies (x > 0) to what it routes."""
    return _MaxPool.apply(x, int(k), bool(relu_gate))


# ------------------------------------------------------------------------------------------------
# channel plumbing: cat / slice / mask-multiply / blend
# ------------------------------------------------------------------------------------------------
class _CatMask(torch.autograd.Function):
    """out = cat(f_i(mask) * tensor_i, dim=1); mask (B,1,H,W) or None; mode 0 none, 1 mask, 2 (1-mask) -- one int for every
    tensor or a tuple with one mode per tensor."""

    @staticmethod
    def forward(ctx, mask, mode, *ts):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        ts = [t.contiguous() for t in ts]
        _chk(mask, *ts)
        B, _, H, W = ts[0].shape
        Ctot = sum(t.shape[1] for t in ts)
        out = torch.empty((B, Ctot, H, W), dtype=torch.float32, device=ts[0].device)
        modes = tuple(mode) if isinstance(mode, (tuple, list)) else (mode,) * len(ts)
        if len(modes) != len(ts):
            raise ValueError('cat_channels: %d mask modes for %d tensors' % (len(modes), len(ts)))
        st, c0 = _stream(), 0
        for t, md in zip(ts, modes):
            lib.him_copy_channels(_p(t), t.shape[1], 0, _p(out), Ctot, c0, t.shape[1], B, H * W, _p(mask), md, 0, st)
            c0 += t.shape[1]
        ctx.mask, ctx.modes = mask, modes
        ctx.chs = [t.shape[1] for t in ts]
        return out

    @staticmethod
    def backward(ctx, dout):
        if dout is None:
            return (None,) * (2 + len(ctx.chs))
        dout = dout.contiguous()
        B, Ctot, H, W = dout.shape
        st, c0, grads = _stream(), 0, []
        for i, ch in enumerate(ctx.chs):
            if ctx.needs_input_grad[2 + i]:
                g = torch.empty((B, ch, H, W), dtype=torch.float32, device=dout.device)
                lib.him_copy_channels(_p(dout), Ctot, c0, _p(g), ch, 0, ch, B, H * W, _p(ctx.mask), ctx.modes[i], 0, st)
                grads.append(g)
            else:
                grads.append(None)
            c0 += ch
        return (None, None) + tuple(grads)


def cat_channels(tensors, mask=None, mask_mode=0):
    """cat(tensors, 1), optionally times the mask (mode 1) or its complement (mode 2); ``mask_mode`` may hold one mode per
    tensor (the 'concat' feature fusion: cat((1-m)*ctx, m*obj))."""
    tensors = [t.full() if isinstance(t, LabelCond) else t for t in tensors]
    if mask is None:
        mask_mode = 0
    elif isinstance(mask_mode, (tuple, list)):
        mask_mode = tuple(int(m) for m in mask_mode)
    else:
        mask_mode = int(mask_mode)
    out = _CatMask.apply(mask, mask_mode, *tensors)
    need = [bool(t.requires_grad) for t in tensors]
    if torch.is_grad_enabled() and any(need) and not all(need):
        # only a channel slice of this tensor can receive a gradient (discriminator input = [data | image]): consumers
        # may restrict their data gradient to it (``_Conv2d.backward``)
        c, lo, hi = 0, None, 0
        for t, n in zip(tensors, need):
            if n:
                lo = c if lo is None else lo
                hi = c + t.shape[1]
            c += t.shape[1]
        out._him_grad_slice = (lo, hi - lo)
    return out


def mul_mask(x, mask):
    """x * mask.repeat(1, C, 1, 1)."""
    return _CatMask.apply(mask, 1, x)


class _DiffAugment(torch.autograd.Function):
    """him_diffaug_fwd / him_diffaug_bwd (include/him.h): colour -> translation -> cutout with one table row per sample."""

    @staticmethod
    def forward(ctx, x, table, ch, cw, c0, policy):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        x = x.contiguous()
        _chk(x)
        B, C, H, W = x.shape
        _chk_table(table, B)
        y = torch.empty_like(x)
        nb = int(lib.him_diffaug_ws(B, H, W)) if policy & 1 else 0
        ws = _ws(nb, x) if nb else None
        lib.him_diffaug_fwd(_p(x), table.data_ptr(), _p(y), B, C, c0, H, W, ch, cw, policy, _p(ws), nb, _stream())
        ctx.table, ctx.args = table, (B, C, c0, H, W, ch, cw, policy)
        ctx.gslice = getattr(x, '_him_grad_slice', None)
        return y

    @staticmethod
    def backward(ctx, dout):
        if dout is None:
            return (None,) * 6
        B, C, c0, H, W, ch, cw, policy = ctx.args
        dout = dout.contiguous()
        nb = int(lib.him_diffaug_ws(B, H, W)) if policy & 1 else 0
        ws = _ws(nb, dout) if nb else None
        st = _stream()
        gs = ctx.gslice
        if gs is not None and gs[1] < C:
            # only channels [g0, g0+n) of the input can use a gradient (the image behind the condition): those alone are
            # computed, zeros elsewhere -- what such an input receives from ``_Conv2d.backward`` too
            g0, n = gs
            dxs = torch.empty((B, n, H, W), dtype=torch.float32, device=dout.device)
            lib.him_diffaug_bwd(_p(dout), ctx.table.data_ptr(), _p(dxs), B, C, c0, H, W, ch, cw, policy, g0, n, _p(ws), nb, st)
            dx = torch.zeros_like(dout)
            lib.him_copy_channels(_p(dxs), n, 0, _p(dx), C, g0, n, B, H * W, 0, 0, 0, st)
        else:
            dx = torch.empty_like(dout)
            lib.him_diffaug_bwd(_p(dout), ctx.table.data_ptr(), _p(dx), B, C, c0, H, W, ch, cw, policy, 0, C, _p(ws), nb, st)
        return dx, None, None, None, None, None


def _chk_table(table, B):
    if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.int32 and table.is_contiguous()
            and tuple(table.shape) == (B, 8)):
        raise HimError('diff_augment: the parameter table must be a contiguous int32 (B, 8) GPU tensor')


def diff_augment(x, table, ch, cw, c0, policy=7):
    """DiffAugment of the dense discriminator input ``x`` (B,C,H,W): channels [c0, c0+3) are the image, the others only
    move with it.  ``table``: int32 (B,8) from ``diffaug_draw``; ``policy`` masks the rows' own bits."""
    if isinstance(x, (LabelCond, CondImage)):
        raise HimError('diff_augment works on the dense concatenated discriminator input')
    y = _DiffAugment.apply(x, table, int(ch), int(cw), int(c0), int(policy) & 7)
    gs = getattr(x, '_him_grad_slice', None)
    if gs is not None:
        y._him_grad_slice = gs      # channel-wise op: the same slice is the only one that needs a gradient
    return y


def diffaug_draw(B, H, W, seed, step, sample0, policy, ratio_translation=0.125, ratio_cutout=0.5, device=None, out=None):
    """-> (table, ch, cw): the int32 (B,8) parameter table drawn ON THE DEVICE on the current stream (no host copy, no
    synchronisation) and the cutout size of the call; ``augment.draw`` gives the same integers on the host."""
    table = out if out is not None else torch.empty((int(B), 8), dtype=torch.int32,
                                                     device=device if device is not None else torch.device('cuda'))
    _chk_table(table, int(B))
    ch, cw = ctypes.c_int(0), ctypes.c_int(0)
    with torch.cuda.device(table.device):
        lib.him_diffaug_draw(table.data_ptr(), int(B), int(H), int(W), int(seed), int(step), int(sample0), int(policy),
                             float(ratio_translation), float(ratio_cutout), ctypes.byref(ch), ctypes.byref(cw), _stream())
    return table, ch.value, cw.value


class _Blend(torch.autograd.Function):
    """out = (1-m) * a[:, a0:a0+C] + m * b    (m: (B,1,H,W))."""

    @staticmethod
    def forward(ctx, a, a0, b, m):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        a, b, m = a.contiguous(), b.contiguous(), m.contiguous()
        _chk(a, b, m)
        B, Cn, H, W = b.shape
        out = torch.empty_like(b)
        lib.him_blend(_p(a), a.shape[1], a0, _p(b), Cn, 0, _p(m), _p(out), B, Cn, H * W, _stream())
        ctx.m, ctx.a0, ctx.Ca = m, a0, a.shape[1]
        return out

    @staticmethod
    def backward(ctx, dout):
        if dout is None:
            return None, None, None, None
        dout = dout.contiguous()
        B, Cn, H, W = dout.shape
        st = _stream()
        da = db = None
        if ctx.needs_input_grad[0]:
            if ctx.Ca == Cn:
                da = torch.empty_like(dout)
            else:
                da = torch.zeros((B, ctx.Ca, H, W), dtype=torch.float32, device=dout.device)
            lib.him_copy_channels(_p(dout), Cn, 0, _p(da), ctx.Ca, ctx.a0, Cn, B, H * W, _p(ctx.m), 2, 0, st)
        if ctx.needs_input_grad[2]:
            db = torch.empty_like(dout)
            lib.him_copy_channels(_p(dout), Cn, 0, _p(db), Cn, 0, Cn, B, H * W, _p(ctx.m), 1, 0, st)
        return da, None, db, None


def blend(a, b, m, a0=0):
    if isinstance(a, LabelCond):
        if a0 >= a.n_onehot:        # the channels read are dense ones (the output gate reads the image out of the G input)
            a, a0 = a.dense, a0 - a.n_onehot
        else:
            a = a.full()
    return _Blend.apply(a, int(a0), b, m)


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        a, b = a.contiguous(), b.contiguous()
        _chk(a, b)
        out = torch.empty_like(a)
        lib.him_add(_p(a), _p(b), _p(out), a.numel(), _stream())
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    return _Add.apply(a, b)


# ------------------------------------------------------------------------------------------------
# input encoding (no gradients)
# ------------------------------------------------------------------------------------------------
def encode_channels(label, inst, image, mask_in, label_nc, use_edges, extra_after=0, color_emb=None, lazy=False):
    """Builds, in ONE (B, Ctot, H, W) buffer and without any torch.cat,
         [ one-hot(label) | edges(inst)? | (1-mask)*image | emb*mask ? ]
    (reference encode_input + the torch.cat at pix2pixHD_condImg_model.py:204).  Returns (buf, n_label, n_cond).
    ``lazy`` (label_nc > 0): ``buf`` is a ``LabelCond`` -- the id map + the dense channels; the one-hot block is written
    only if a consumer asks for it (``LabelCond.full``)."""
    _chk(label, inst, image, mask_in, color_emb)
    B, _, H, W = image.shape
    hw = H * W
    n_label = (label_nc if label_nc else label.shape[1]) + (1 if use_edges else 0)
    n_cond = 3 + (3 if color_emb is not None else 0)
    Ctot = n_label + n_cond
    if lazy and label_nc:
        Cd = Ctot - label_nc
        dense = torch.empty((B, Cd, H, W), dtype=torch.float32, device=image.device)
        st, c = _stream(), 0
        if use_edges:
            lib.him_edges(_p(inst), _p(dense), B, H, W, Cd, 0, st)
            c = 1
        lib.him_copy_channels(_p(image), 3, 0, _p(dense), Cd, c, 3, B, hw, _p(mask_in), 2, 0, st)
        if color_emb is not None:
            lib.him_tile_embed(_p(color_emb), _p(mask_in), _p(dense), B, Cd, c + 3, hw, st)
        return LabelCond(label.contiguous(), label_nc, dense), n_label, n_cond
    buf = torch.empty((B, Ctot, H, W), dtype=torch.float32, device=image.device)
    st = _stream()
    if label_nc:
        lib.him_onehot(_p(label), _p(buf), B, label_nc, Ctot, 0, hw, st)
        c = label_nc
    else:
        c = label.shape[1]
        lib.him_copy_channels(_p(label), c, 0, _p(buf), Ctot, 0, c, B, hw, 0, 0, 0, st)
    if use_edges:
        lib.him_edges(_p(inst), _p(buf), B, H, W, Ctot, c, st)
        c += 1
    lib.him_copy_channels(_p(image), 3, 0, _p(buf), Ctot, c, 3, B, hw, _p(mask_in), 2, 0, st)
    c += 3
    if color_emb is not None:
        lib.him_tile_embed(_p(color_emb), _p(mask_in), _p(buf), B, Ctot, c, hw, st)
    if label_nc:
        mark_onehot(buf, label, label_nc)
    return buf, n_label, n_cond


def slice_channels(x, c0, n):
    """contiguous copy of x[:, c0:c0+n] (no gradient)."""
    if isinstance(x, LabelCond):
        return x.slice(c0, n)
    _chk(x)
    B, Cn, H, W = x.shape
    out = torch.empty((B, n, H, W), dtype=torch.float32, device=x.device)
    lib.him_copy_channels(_p(x), Cn, c0, _p(out), n, 0, n, B, H * W, 0, 0, 0, _stream())
    oh = getattr(x, '_him_onehot', None)
    if oh is not None and c0 == 0 and n >= oh[1]:      # a slice that still starts with the whole one-hot block
        mark_onehot(out, oh[0], oh[1])
    return out


def widen_u8(t):
    """uint8 id map (any shape) on the device -> float32 ids (what every kernel of the path reads)."""
    if not t.is_cuda or t.dtype != torch.uint8:
        raise HimError('widen_u8 needs a uint8 GPU tensor')
    t = t.contiguous()
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    lib.him_u8_to_f32(t.data_ptr(), out.data_ptr(), t.numel(), _stream())
    return out


def get_masked_image(image, bbox, cls2fill=0.0):
    """Batched, on-device ``get_masked_image`` (reference data/base_dataset.py:342-357): ``image`` (B,C,H,W), ``bbox``
    (B,4) = (wmin, hmin, wmax, hmax) -> (mask (B,1,H,W), mask*image, (1-mask)*image + mask*cls2fill)."""
    image = image.contiguous()
    bbox = bbox.to(device=image.device, dtype=torch.float32).contiguous()
    _chk(image, bbox)
    B, Cn, H, W = image.shape
    if tuple(bbox.shape) != (B, 4):
        raise HimError('get_masked_image: bbox must be (B, 4), got %s' % (tuple(bbox.shape),))
    mask = torch.empty((B, 1, H, W), dtype=torch.float32, device=image.device)
    obj, ctx = torch.empty_like(image), torch.empty_like(image)
    lib.him_masked_image(_p(image), _p(bbox), _p(mask), _p(obj), _p(ctx), B, Cn, H, W, float(cls2fill), _stream())
    return mask, obj, ctx


def tile_embedding(embedding, mask_in):
    """(B,K) embedding, (B,1,H,W) mask -> (B,K,H,W) = embedding[b,k] * mask[b,0,y,x]  (``encode_global_embedding``,
    models/pix2pixHD_condImgColor_model.py:147-160); him_tile_embed writes three channels per launch (the colour path's K)."""
    _chk(embedding, mask_in)
    B, K = embedding.shape
    H, W = mask_in.shape[2], mask_in.shape[3]
    if K % 3:
        raise ValueError('tile_embedding: K = %d (the colour embedding has 3 channels per group)' % K)
    out = torch.empty((B, K, H, W), dtype=torch.float32, device=embedding.device)
    mask_in = mask_in.contiguous()
    for k in range(0, K, 3):
        emb = embedding[:, k:k + 3].contiguous()
        lib.him_tile_embed(_p(emb), _p(mask_in), _p(out), B, K, k, H * W, _stream())
    return out


def masked_mean_color(image, obj_mask, noise=None):
    _chk(image, obj_mask, noise)
    B, _, H, W = image.shape
    emb = torch.empty((B, 3), dtype=torch.float32, device=image.device)
    lib.him_masked_mean(_p(image), _p(obj_mask), _p(noise), _p(emb), B, H * W, _stream())
    return emb


# ------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------
class _L1Mean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        a, b = a.contiguous(), b.contiguous()
        _chk(a, b)
        if a.shape != b.shape:
            raise HimError('l1: shape mismatch %s vs %s' % (tuple(a.shape), tuple(b.shape)))
        out = torch.empty((), dtype=torch.float32, device=a.device)
        nb = lib.him_reduce_ws(a.numel())
        ws = _ws(nb, a)
        lib.him_l1_mean_fwd(_p(a), _p(b), a.numel(), _p(out), _p(ws), nb, _stream())
        ctx.a, ctx.b = a, b
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        a, b = ctx.a, ctx.b
        g = g.contiguous()
        da = torch.empty_like(a)
        lib.him_l1_mean_bwd(_p(a), _p(b), a.numel(), _p(g), _p(da), 0, _stream())
        return da, None


def l1_mean(a, b):
    """nn.L1Loss()(a, b.detach())."""
    return _L1Mean.apply(a, b.detach())


class _L1WeightedSum(torch.autograd.Function):
    """sum_i w_i * mean|a_i - b_i| as ONE autograd node: n reductions into a vector, one tiny weighted sum; the backward
    scales the incoming gradient by the weights once and runs the n L1 backward kernels.  Replaces the chain of
    ``loss = loss + w * l1(...) * lambda`` scalar kernels (3 launches forward + 2 backward per term)."""

    @staticmethod
    def forward(ctx, wvec, gate, *tensors):
        ctx.set_materialize_grads(False)
        ctx.gate = bool(gate)
        n = len(tensors) // 2
        a_s = [t.contiguous() for t in tensors[:n]]
        b_s = [t.contiguous() for t in tensors[n:]]
        vals = torch.empty(n, dtype=torch.float32, device=wvec.device)
        st = _stream()
        for a, b in zip(a_s, b_s):
            _chk(a, b)
            if a.shape != b.shape:
                raise HimError('l1: shape mismatch %s vs %s' % (tuple(a.shape), tuple(b.shape)))
        # all pairs in one reduction launch + one finishing launch (per-pair sums as in him_l1_mean_fwd, bit for bit)
        ctx.pa = (ctypes.c_void_p * n)(*[_p(a) for a in a_s])
        ctx.pb = (ctypes.c_void_p * n)(*[_p(b) for b in b_s])
        ctx.pn = (ctypes.c_size_t * n)(*[a.numel() for a in a_s])
        nb = lib.him_l1_multi_ws(n)
        ws = _ws(nb, a_s[0])
        lib.him_l1_multi_fwd(ctx.pa, ctx.pb, ctx.pn, n, _p(vals), _p(ws), nb, st)
        ctx.a_s, ctx.b_s, ctx.wvec = a_s, b_s, wvec
        return (vals * wvec).sum()

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * (2 + 2 * len(ctx.a_s))
        gw = (g * ctx.wvec).contiguous()
        st = _stream()
        grads = [torch.empty_like(a) if ctx.needs_input_grad[2 + i] else None for i, a in enumerate(ctx.a_s)]
        n = len(grads)
        pda = (ctypes.c_void_p * n)(*[_p(da) for da in grads])
        lib.him_l1_multi_bwd(ctx.pa, ctx.pb, ctx.pn, n, _p(gw), pda, 2 if ctx.gate else 0, st)
        return (None, None) + tuple(grads) + (None,) * len(ctx.b_s)


_WVEC_CACHE = {}


def l1_weighted_sum(pairs, weights, gate_relu=False):
    """sum_i weights[i] * nn.L1Loss()(a_i, b_i.detach()) for pairs = [(a_i, b_i), ...].  ``gate_relu``: every a_i is the
    output of a ReLU layer built with ``grad_premasked`` -- the gradients sent back carry the (a_i > 0) gate."""
    dev = pairs[0][0].device
    key = (dev, tuple(float(w) for w in weights))
    wvec = _WVEC_CACHE.get(key)
    if wvec is None:
        wvec = _WVEC_CACHE[key] = torch.tensor(key[1], dtype=torch.float32, device=dev)
    return _L1WeightedSum.apply(wvec, bool(gate_relu), *([a for a, _ in pairs] + [b.detach() for _, b in pairs]))


class _LinComb(torch.autograd.Function):
    """scale * sum_i w_i * t_i over one-element tensors as ONE node / ONE launch each way (him_lincomb_*): the scalar loss
    arithmetic of the trainer, which as torch expressions was ~45 one-element ATen kernels per step."""

    @staticmethod
    def forward(ctx, weights, scale, *terms):
        ctx.set_materialize_grads(False)
        n = len(terms)
        ts = [t.contiguous() for t in terms]
        _chk(*ts)
        if any(t.numel() != 1 for t in ts):
            raise HimError('lincomb: one-element tensors only')
        ctx.weights, ctx.scale, ctx.shapes = tuple(float(w) for w in weights), float(scale), [t.shape for t in ts]
        out = torch.empty((), dtype=torch.float32, device=ts[0].device)
        ptrs = (ctypes.c_void_p * n)(*[_p(t) for t in ts])
        ws = (ctypes.c_float * n)(*ctx.weights)
        lib.him_lincomb_fwd(ptrs, ws, n, ctx.scale, _p(out), _stream())
        return out

    @staticmethod
    def backward(ctx, g):
        n = len(ctx.weights)
        if g is None:
            return (None,) * (n + 2)
        g = g.contiguous()
        need = ctx.needs_input_grad[2:]
        outs = [torch.empty(s, dtype=torch.float32, device=g.device) if nd else None for s, nd in zip(ctx.shapes, need)]
        ptrs = (ctypes.c_void_p * n)(*[_p(o) for o in outs])
        ws = (ctypes.c_float * n)(*ctx.weights)
        lib.him_lincomb_bwd(_p(g), ws, n, ctx.scale, ptrs, _stream())
        return (None, None) + tuple(outs)


def lincomb(terms, weights=None, scale=1.0):
    """scale * (w_0 t_0 + w_1 t_1 + ...), left to right in fp32, over one-element tensors (default weights: 1)."""
    terms = list(terms)
    if not SCHED.lincomb:          # the same expression as a chain of one-element torch ops (A/B switch)
        ws = list(weights) if weights is not None else [1.0] * len(terms)
        acc = 0
        for w, t in zip(ws, terms):
            acc = acc + (t if w == 1.0 else t * w)
        return acc if scale == 1.0 else acc * scale
    ws = tuple(weights) if weights is not None else (1.0,) * len(terms)
    # him_lincomb_* take at most 8 terms per launch: longer sums (--num_D > 8) fold 8 at a time, left to right -- the
    # running sum enters the next launch as its first term with weight 1 (x * 1.0 is exact: same rounding as one chain)
    while len(terms) > 8:
        head = _LinComb.apply(ws[:8], 1.0, *terms[:8])
        terms, ws = [head] + terms[8:], (1.0,) + ws[8:]
    return _LinComb.apply(ws, scale, *terms)


class _MSEConst(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        x = x.contiguous()
        _chk(x)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        nb = lib.him_reduce_ws(x.numel())
        ws = _ws(nb, x)
        lib.him_mse_const_fwd(_p(x), x.numel(), target, _p(out), _p(ws), nb, _stream())
        ctx.x, ctx.t = x, target
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None
        x = ctx.x
        g = g.contiguous()
        dx = torch.empty_like(x)
        lib.him_mse_const_bwd(_p(x), x.numel(), ctx.t, _p(g), _p(dx), 0, _stream())
        return dx, None


def mse_const(x, target):
    """nn.MSELoss()(x, full_like(x, target))."""
    return _MSEConst.apply(x, float(target))


# ------------------------------------------------------------------------------------------------
# spectral norm
# ------------------------------------------------------------------------------------------------
class _SNSigma(torch.autograd.Function):
    @staticmethod
    def forward(ctx, W, u):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        W2 = W.contiguous().view(W.shape[0], -1)
        u = u.detach().clone()      # the layer overwrites its persistent u in place after this call
        _chk(W2, u)
        rows, cols = W2.shape
        v = torch.empty(cols, dtype=torch.float32, device=W.device)
        u_new = torch.empty((1, rows), dtype=torch.float32, device=W.device)
        sigma = torch.empty((1, 1), dtype=torch.float32, device=W.device)
        nb = lib.him_sn_ws(rows, cols)
        ws = _ws(nb, W)
        lib.him_sn_power_iter_fwd(_p(W2), _p(u), rows, cols, _p(v), _p(u_new), _p(sigma), _p(ws), nb, _stream())
        ctx.W, ctx.u, ctx.v = W2, u, v
        ctx.save_for_backward(u_new, sigma)    # outputs: never as plain ctx attributes (uncollectable cycle)
        ctx.shape = W.shape
        ctx.mark_non_differentiable(u_new)
        return sigma, u_new

    @staticmethod
    def backward(ctx, g, _gu):
        if g is None:
            return None, None
        W2 = ctx.W
        rows, cols = W2.shape
        g = g.contiguous()
        dW = torch.empty_like(W2)
        nb = lib.him_sn_ws(rows, cols)
        ws = _ws(nb, W2)
        u_new, sigma = ctx.saved_tensors
        lib.him_sn_power_iter_bwd(_p(W2), _p(ctx.u), _p(ctx.v), _p(u_new), _p(sigma), _p(g), rows, cols,
                                  _p(dW), 0, _p(ws), nb, _stream())
        return dW.view(ctx.shape), None


def sn_max_singular_value(W, u):
    """(sigma (1,1), u' (1,rows)) of models/sn_utils.py:11-25 with Ip = 1; sigma is differentiable in W through
    BOTH normalisations (nothing detached, as in the reference)."""
    return _SNSigma.apply(W, u)


class _DivScalar(torch.autograd.Function):
    @staticmethod
    def forward(ctx, W, sigma):
        ctx.set_materialize_grads(False)   # an undefined gradient stays None: backward returns early
        W = W.contiguous()
        sigma = sigma.contiguous()
        _chk(W, sigma)
        out = torch.empty_like(W)
        lib.him_div_scalar_fwd(_p(W), _p(sigma), _p(out), W.numel(), _stream())
        ctx.W, ctx.sigma = W, sigma
        return out

    @staticmethod
    def backward(ctx, dout):
        if dout is None:
            return None, None
        W, sigma = ctx.W, ctx.sigma
        dout = dout.contiguous()
        dW = torch.empty_like(W)
        dsig = torch.empty_like(sigma)
        ws = _ws(4096, W)
        lib.him_div_scalar_bwd(_p(W), _p(sigma), _p(dout), _p(dW), _p(dsig), W.numel(), 0, _p(ws), 4096, _stream())
        return dW, dsig


def div_scalar(W, sigma):
    return _DivScalar.apply(W, sigma)


# -- plumbing shared by the operators below (none of them is on the training path): cached scratch, status read-back,
# plane check --------------------------------------------------------------------------------------------------------------
_SCRATCH = {}           # (operator, device index) -> _Scratch


class _Scratch(object):
    """The cached workspace of one operator on one device: ONE grow-only byte buffer, whatever shapes the operator is
    called with, so what an operator holds is bounded by its largest call.  ``buf``: the uint8 tensor; ``stream`` /
    ``event``: the stream of the last use and the event recorded behind it; ``home``: the stream ``buf`` was allocated
    on."""
    __slots__ = ('buf', 'home', 'stream', 'event')

    def __init__(self):
        self.buf = self.home = self.stream = None
        self.event = torch.cuda.Event()

    def __enter__(self):
        return self.buf

    def __exit__(self, *a):
        self.done(self.stream)
        return False

    def done(self, stream):
        """Everything queued on ``stream`` so far is the last use."""
        self.stream = stream
        self.event.record(stream)


def _scratch(tag, nbytes):
    """``with _scratch(tag, nbytes) as ws:`` -- at least ``nbytes`` (and at least one) bytes of the operator ``tag`` on
    the current device, handed over to the current stream: a use on another stream than the last one first waits for the
    event behind that one; leaving the block records the event behind this use.  ``_p(ws)`` and ``ws.numel()`` go to the
    C ABI.  The base is aligned for fp64 (and more): the caching allocator hands out multiples of 512 bytes."""
    key = (tag, torch.cuda.current_device())
    s = _SCRATCH.get(key)
    if s is None:
        s = _SCRATCH[key] = _Scratch()
    cur = torch.cuda.current_stream()
    if s.stream is not None and s.stream != cur:
        cur.wait_event(s.event)
    if s.buf is None or s.buf.numel() < nbytes:
        # the buffer dropped here is safe to reuse: its block returns to the stream it was allocated on, which either
        # ran its last launch or was told about the stream that did (record_stream below)
        s.buf, s.home = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device='cuda'), cur
        assert s.buf.data_ptr() % 16 == 0
    elif cur != s.home:
        # a launch on a stream the allocator does not know of: without this a buffer dropped on growth (or with the
        # cache) could be handed out again on ``home`` while that launch still runs
        s.buf.record_stream(cur)
    s.stream = cur
    return s


def _read_back(tag, st):
    """The host array of the ``out`` tensor of a ``*_launch`` state: one asynchronous copy into its pinned ``host`` twin,
    the operator's event recorded behind it (the next launch, which overwrites ``out``, waits for the copy from whatever
    stream it comes) and one wait on the current stream only."""
    with torch.cuda.device(st['out'].device):
        cur = torch.cuda.current_stream()
        st['host'].copy_(st['out'], non_blocking=True)
        _SCRATCH[tag, torch.cuda.current_device()].done(cur)
        cur.synchronize()
    return st['host'].numpy()


# accepted layouts of ``_planes``: name -> (the shapes as the message lists them, rank of what it returns, whether the
# message shows a refused shape as given or as planes)
_PLANE_LAYOUTS = {'plane': ('one (H, W) plane', 2, True),
                  'hw_first': ('(H, W), (B, H, W) or (B, 1, H, W)', 3, True),
                  'planes': ('(B, H, W), (B, 1, H, W) or (H, W)', 3, False),
                  'nchw': ('(B, 1, H, W), (B, H, W) or (H, W)', 4, False)}


def _planes(op, arg, t, kinds, layout, *, channels=False, max_side=None, single=False):
    """The argument ``arg`` of the operator ``op`` as contiguous planes: a device tensor of a dtype among ``kinds`` in
    one of the shapes of ``layout``, reshaped to (H, W), (B, H, W) or (B, 1, H, W).  ``channels``: (B, C, H, W) passes
    too (scores); ``max_side``: the largest H and W; ``single``: B must be 1 and the plane (H, W) is returned.
    ValueError for anything else."""
    name = '%s: %s' % (op, arg)
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError('%s must be a device tensor' % name)
    if t.dtype not in kinds:
        raise ValueError('%s is %s, accepted: %s' % (name, t.dtype, ' / '.join(str(k) for k in kinds)))
    accepts, rank, got_given = _PLANE_LAYOUTS[layout]
    shape = tuple(t.shape)
    if rank == 2:
        fits, new = len(shape) >= 2 and all(s == 1 for s in shape[:-2]), shape[-2:]
    else:
        fits = len(shape) in (2, 3) or (len(shape) == 4 and (channels or shape[1] == 1))
        lead = (shape[0] if len(shape) > 2 else 1,) + ((shape[1] if len(shape) == 4 else 1,) if rank == 4 else ())
        new = lead + shape[-2:]
    if not fits or 0 in shape or (max_side is not None and max(new[-2:]) > max_side):
        if max_side is not None:
            accepts += ' with H, W <= %d' % max_side
        raise ValueError('%s must be %s, got %s' % (name, accepts, shape if got_given or not fits else new))
    if single and new[0] != 1:
        raise ValueError('%s: one plane at a time (B = 1), got %s' % (op, shape))
    return t.detach().reshape(new[1:] if single else new).contiguous()


# -- joint box -> layout -> image edit: evaluate(target_size) and the canvas crop / paste (include/him.h) ---------------
def resize_compose(comb_prob, obj_prob, label, mask_out, cls, background, align_corners=False):
    """TwoStreamAE_mask.evaluate(target_size)'s tail (reference :318-335) in one kernel at the (H, W) of ``label``
    (1,1,H,W): the object class -> fp32 ``obj_prob`` (1,1,h,w) sampled bilinearly > .5 ? cls : label; the background class
    (``background``) -> int64 arg-max over c of bilinear(comb_prob[c]) * m + (1 - m) * [label == c], m = ``mask_out``."""
    src = comb_prob if background else obj_prob
    label = label.contiguous()
    mask_out = None if mask_out is None else mask_out.contiguous()
    src = src.contiguous()
    _chk(src, label, mask_out)
    if src.dim() != 4 or src.shape[0] != 1 or label.numel() != label.shape[-2] * label.shape[-1]:
        raise HimError('resize_compose: one sample (1,C,h,w) probabilities and a (1,1,H,W) label map')
    _, C, h, w = src.shape
    H, W = label.shape[-2:]
    if background and (mask_out is None or tuple(mask_out.shape) != tuple(label.shape)):
        raise HimError('resize_compose: mask_out %s must have the label map\'s shape %s'
                       % (None if mask_out is None else tuple(mask_out.shape), tuple(label.shape)))
    other = obj_prob if background else comb_prob
    if other is not None and tuple(other.shape[-2:]) != (h, w):
        raise HimError('resize_compose: comb_prob %s and obj_prob %s differ in (h, w)'
                       % (tuple(comb_prob.shape), tuple(obj_prob.shape)))
    dst = torch.empty((1, 1, H, W), dtype=torch.int64 if background else torch.float32, device=label.device)
    lib.him_resize_compose(_p(src) if background else 0, 0 if background else _p(src), C, h, w, _p(label),
                           _p(mask_out) if background else 0, int(cls), 1 if background else 0, _p(dst), H, W,
                           1 if align_corners else 0, _stream())
    return dst


def _align16(n):
    return n + ((-n) % 16)


def _scratch_and_tables(lead, arrays, dev):
    """One device byte buffer: ``lead`` bytes of scratch, then the host ``arrays`` (resampling tables) uploaded with one
    asynchronous copy from pinned memory on the current stream -> (buffer, device address of each array)."""
    import numpy as np
    start = _align16(int(lead))
    at, size = [], start
    for a in arrays:
        at.append(size)
        size = _align16(size + a.nbytes)
    host = torch.empty(max(size - start, 16), dtype=torch.uint8, pin_memory=True)
    view = host.numpy()
    for o, a in zip(at, arrays):
        view[o - start:o - start + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    buf = torch.empty(start + host.numel(), dtype=torch.uint8, device=dev)
    buf[start:].copy_(host, non_blocking=True)
    base = buf.data_ptr()
    return buf, [base + o for o in at]


def _plane_geometry(t, what):
    _chk(t)
    if t.dim() != 4 or t.shape[0] != 1:
        raise HimError('%s: one (1,C,H,W) fp32 tensor, got %s' % (what, tuple(t.shape)))
    return t.shape[1], t.shape[2], t.shape[3]


def canvas_crop_nearest(canvas, box, H, W, pre=1):
    """(1,1,H,W) fp32 ids: ToPILImage of the one-channel ``canvas`` (``pre`` 1: the canvas holds ids and is divided by
    255 first, as tensor2pil does), ``Image.crop(box)`` (integer (x0,y0,x1,y1), may extend past the canvas: zeros),
    ``resize((W,H), NEAREST)``, ToTensor * 255."""
    import numpy as np
    from .data import resample
    C, Hs, Ws = _plane_geometry(canvas, 'canvas_crop_nearest')
    if C != 1:
        raise HimError('canvas_crop_nearest: a label canvas has one channel, got %d' % C)
    x0, y0, x1, y1 = (int(v) for v in box)
    w, h = x1 - x0, y1 - y0
    if w <= 0 or h <= 0:
        raise HimError('canvas_crop_nearest: empty window %s' % (box,))
    buf, (o, p, xt, yt) = _scratch_and_tables(h * w, [np.zeros(1, np.int64), np.array([w], np.int32),
                                                      resample.nearest_table(w, W), resample.nearest_table(h, H)],
                                              canvas.device)
    st = _stream()
    lib.him_canvas_window_bytes(_p(canvas), 1, Hs, Ws, x0, y0, h, w, pre, buf.data_ptr(), st)
    dst = torch.empty((1, 1, H, W), dtype=torch.float32, device=canvas.device)
    lib.him_data_nearest(buf.data_ptr(), o, p, xt, yt, 0, _p(dst), 0, 1, H, W, st)
    return dst


def canvas_crop_bicubic(canvas, box, H, W, normalize=True):
    """(1,3,H,W) fp32: ToPILImage of the RGB ``canvas`` (1,3,Hc,Wc) in [0,1], ``Image.crop(box)`` (zeros outside),
    ``resize((W,H), BICUBIC)``, ToTensor, optionally Normalize((.5,.5,.5),(.5,.5,.5))."""
    return _bicubic(canvas, box, H, W, 0, None, (0, 0), normalize)


def canvas_paste_bicubic(patch, box, canvas, x0, y0, H, W, pre=0):
    """In place: the window ``box`` of ``patch`` (1,3,h,w) (inside it) as ToPILImage bytes of pre(v) (0: v, 2: (v+1)/2),
    ``resize((W,H), BICUBIC)``, ToTensor, written into ``canvas`` (1,3,Hc,Wc) at [y0,y0+H) x [x0,x0+W)."""
    return _bicubic(patch, box, H, W, pre, canvas, (x0, y0), False)


def _bicubic(src, box, H, W, pre, canvas, at, normalize, blend=None):
    import numpy as np
    from .data import resample
    C, Hs, Ws = _plane_geometry(src, 'canvas bicubic')
    if C != 3:
        raise HimError('canvas bicubic: RGB planes, got %d channels' % C)
    x0, y0, x1, y1 = (int(v) for v in box)
    w, h = x1 - x0, y1 - y0
    if w <= 0 or h <= 0 or h > 65535 or H <= 0 or W <= 0:
        raise HimError('canvas bicubic: bad window %s -> %dx%d' % (box, W, H))
    fx, nx, wx, ksx = resample.bicubic_tables(w, W)
    fy, ny, wy, ksy = resample.bicubic_tables(h, H)
    buf, (o, p, r, afx, anx, awx, afy, any_, awy, fl) = _scratch_and_tables(
        h * w * 3, [np.zeros(1, np.int64), np.array([w], np.int32), np.array([h], np.int32), fx, nx, wx, fy, ny, wy,
                    np.zeros(1, np.int32)], src.device)
    st = _stream()
    lib.him_canvas_window_bytes(_p(src), 3, Hs, Ws, x0, y0, h, w, pre, buf.data_ptr(), st)
    tmp = torch.empty((h, W, 3), dtype=torch.uint8, device=src.device)
    lib.him_data_bicubic_h(buf.data_ptr(), o, p, r, afx, anx, awx, ksx, _p(tmp), h, 1, W, st)
    if canvas is None:
        dst = torch.empty((1, 3, H, W), dtype=torch.float32, device=src.device)
        lib.him_data_bicubic_v(_p(tmp), h, afy, any_, awy, ksy, fl, _p(dst), 1 if normalize else 0, 1, H, W, st)
        return dst
    _, Hc, Wc = _plane_geometry(canvas, 'canvas_paste_bicubic')
    if blend is None:
        lib.him_canvas_paste_bicubic_v(_p(tmp), afy, any_, awy, ksy, _p(canvas), Hc, Wc, int(at[0]), int(at[1]), H, W, st)
        return canvas
    dist2, feather, reach, profile, matte = blend
    lib.him_canvas_paste_blend_v(_p(tmp), afy, any_, awy, ksy, _p(canvas), Hc, Wc, int(at[0]), int(at[1]), H, W,
                                 _p(dist2), feather, reach, profile, _p(matte), st)
    return canvas


MATTE_PROFILES = {'linear': 0, 'smooth': 1}
MATTE_MAX_RADIUS = 16384


def matte_args(feather, reach, profile, what):
    """(feather, reach, profile number) of a blended paste, checked on the host: ``feather`` 1..16384 pixels of ramp,
    ``reach`` 0..16384 pixels of full strength around the changed pixels, ``profile`` in ``MATTE_PROFILES``."""
    for name, v, lo in (('feather', feather, 1), ('reach', reach, 0)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= MATTE_MAX_RADIUS:
            raise ValueError('%s: %s must be an int in %d..%d, got %r' % (what, name, lo, MATTE_MAX_RADIUS, v))
    if profile not in MATTE_PROFILES:
        raise ValueError('%s: profile %r (one of %s)' % (what, profile, ', '.join(MATTE_PROFILES)))
    return feather, reach, MATTE_PROFILES[profile]


def canvas_changed(before, after, x0, y0, H, W):
    """(1,H,W) uint8 on the device: 1 where the one-channel fp32 id canvases ``before`` and ``after`` (1,1,Hc,Wc) differ
    inside the window [y0,y0+H) x [x0,x0+W), which must lie inside them -- the seed plane ``distance_transform`` reads
    under ``rule='nonzero'``.  Current stream, no host synchronisation."""
    C, Hc, Wc = _plane_geometry(before, 'canvas_changed')
    if C != 1 or tuple(after.shape) != tuple(before.shape) or after.device != before.device:
        raise HimError('canvas_changed: two (1,1,Hc,Wc) label canvases of one shape on one device, got %s and %s'
                       % (tuple(before.shape), tuple(after.shape)))
    _chk(after)
    x0, y0, H, W = int(x0), int(y0), int(H), int(W)
    if H < 1 or W < 1 or x0 < 0 or y0 < 0 or x0 + W > Wc or y0 + H > Hc:
        raise HimError('canvas_changed: window (%d,%d)+(%d,%d) outside the %dx%d canvas' % (x0, y0, W, H, Wc, Hc))
    changed = torch.empty((1, H, W), dtype=torch.uint8, device=before.device)
    lib.him_canvas_changed(_p(before), _p(after), Hc, Wc, x0, y0, H, W, _p(changed), _stream())
    return changed


def canvas_paste_blend(patch, box, canvas, x0, y0, H, W, pre=0, feather=8, reach=0, dist2=None, profile='smooth',
                       want_matte=False):
    """``canvas_paste_bicubic`` through a matte, in place -> ``(canvas, matte or None)``.  The matte fades over ``feather``
    pixels towards every side of the window that is not on the canvas edge and, with ``dist2`` (int32 (H,W) or (1,H,W):
    ``distance_transform``'s squared distances to the pixels an edit changed), from full strength within ``reach`` pixels
    of them to nothing at ``reach + feather``; ``profile`` 'linear' or 'smooth' (smoothstep).  Where the matte is 1 the
    canvas receives exactly what ``canvas_paste_bicubic`` writes, where it is 0 it keeps its pixel (include/him.h
    "Feathered canvas composite").  ``matte``: (1,1,H,W) fp32.  Current stream, no host synchronisation."""
    feather, reach, profile = matte_args(feather, reach, profile, 'canvas_paste_blend')
    H, W = int(H), int(W)
    if dist2 is not None:
        if not torch.is_tensor(dist2) or not dist2.is_cuda or dist2.dtype != torch.int32 or dist2.device != canvas.device \
                or tuple(dist2.shape) not in ((H, W), (1, H, W)):
            raise HimError('canvas_paste_blend: dist2 must be an int32 (%d,%d) tensor on the canvas device' % (H, W))
        dist2 = dist2.contiguous()
    matte = torch.empty((1, 1, H, W), dtype=torch.float32, device=canvas.device) if want_matte else None
    _bicubic(patch, box, H, W, pre, canvas, (x0, y0), False, (dist2, feather, reach, profile, matte))
    return canvas, matte


# -- seamless (gradient-domain) composite: the membrane of include/him.h "Seamless canvas composite" ---------------------
MEMBRANE_MAX_N, MEMBRANE_NO_SIDE = 2048, 1
_MEMBRANE_BASES = {}    # (n, lo, hi, device index) -> (V, Vt, lam) fp64


def membrane_sides(Hc, Wc, x0, y0, H, W, what='membrane'):
    """(l, r, t, b, ny, nx) of an H x W window at (x0, y0) of an Hc x Wc canvas, checked on the host: a side is counted
    when photograph lies beyond it; the interior left by the counted sides must hold a pixel and at most 2048 per axis."""
    Hc, Wc, x0, y0, H, W = (int(v) for v in (Hc, Wc, x0, y0, H, W))
    if H < 1 or W < 1 or x0 < 0 or y0 < 0 or x0 + W > Wc or y0 + H > Hc:
        raise ValueError('%s: window (%d,%d)+(%d,%d) outside the %dx%d canvas' % (what, x0, y0, W, H, Wc, Hc))
    l, r, t, b = int(x0 > 0), int(x0 + W < Wc), int(y0 > 0), int(y0 + H < Hc)
    ny, nx = H - t - b, W - l - r
    if ny < 1 or nx < 1:
        raise ValueError('%s: a %dx%d window with sides l%d r%d t%d b%d has no interior' % (what, W, H, l, r, t, b))
    if ny > MEMBRANE_MAX_N or nx > MEMBRANE_MAX_N:
        raise ValueError('%s: interior %dx%d above %d pixels per axis' % (what, nx, ny, MEMBRANE_MAX_N))
    return l, r, t, b, ny, nx


def membrane_basis(n, lo, hi, device=None):
    """``(V, Vt, lam)``: the orthonormal eigenbasis (n,n) fp64 of the 1-D second difference on ``n`` pixels with a
    Dirichlet (1) or Neumann (0) end at ``lo`` / ``hi``, its transpose and the eigenvalues (n,), built on the device once
    per ``(n, lo, hi, device)``.  Current stream, no host synchronisation."""
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MEMBRANE_MAX_N:
        raise ValueError('membrane_basis: n must be an int in 1..%d, got %r' % (MEMBRANE_MAX_N, n))
    if lo not in (0, 1) or hi not in (0, 1):
        raise ValueError('membrane_basis: lo and hi are 0 or 1, got %r, %r' % (lo, hi))
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    key = (n, int(lo), int(hi), dev.index if dev.index is not None else torch.cuda.current_device())
    got = _MEMBRANE_BASES.get(key)
    if got is None:
        V = torch.empty((n, n), dtype=torch.float64, device=dev)
        Vt = torch.empty((n, n), dtype=torch.float64, device=dev)
        lam = torch.empty((n,), dtype=torch.float64, device=dev)
        lib.him_membrane_basis(n, int(lo), int(hi), _p(V), _p(Vt), _p(lam), _stream())
        got = _MEMBRANE_BASES[key] = (V, Vt, lam)
    return got


def _membrane_P(P, what):
    if torch.is_tensor(P) and P.dim() == 3:
        P = P[None]
    C, H, W = _plane_geometry(P, what)
    if C != 3:
        raise HimError('%s: P is (1,3,H,W), got %d channels' % (what, C))
    return P, H, W


def membrane_solve(canvas, x0, y0, P):
    """``(m, status)``: the membrane (1,3,H,W) fp32 of the patch ``P`` (1,3,H,W) (what the hard paste would write) in
    the window at ``(x0, y0)`` of the photo ``canvas`` (1,3,Hc,Wc): ``O - P`` on the window's ring, its harmonic extension
    inside, so that ``P + m`` is the Poisson clone.  ``status``: int32 ``[sides mask, ny, nx, flags]`` on the device.
    ValueError before any device work for a window without interior.  Current stream, no host synchronisation."""
    P, H, W = _membrane_P(P, 'membrane_solve')
    C, Hc, Wc = _plane_geometry(canvas, 'membrane_solve')
    if C != 3 or P.device != canvas.device:
        raise HimError('membrane_solve: an RGB canvas and P on one device')
    x0, y0 = int(x0), int(y0)
    l, r, t, b, ny, nx = membrane_sides(Hc, Wc, x0, y0, H, W, 'membrane_solve')
    sides = l | r << 1 | t << 2 | b << 3
    dev = canvas.device
    m = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    if sides == 0:
        lib.him_membrane_solve(_p(canvas), Hc, Wc, x0, y0, H, W, _p(P), 0, 0, 0, 0, 0, 0, _p(m), 0, _p(status), _stream())
        return m, status
    Vy, Vyt, lamy = membrane_basis(ny, t, b, dev)
    Vx, Vxt, lamx = membrane_basis(nx, l, r, dev)
    with _scratch('membrane_solve', lib.him_membrane_ws(H, W, sides)) as ws:
        lib.him_membrane_solve(_p(canvas), Hc, Wc, x0, y0, H, W, _p(P), _p(Vy), _p(Vyt), _p(lamy), _p(Vx), _p(Vxt),
                               _p(lamx), _p(m), _p(ws), _p(status), _stream())
    return m, status


def canvas_seamless_apply(P, m, canvas, x0, y0, *, feather=None, reach=0, dist2=None, profile='smooth', want_matte=False):
    """In place -> ``(canvas, matte or None)``: the window's interior takes ``clamp(P + m, 0, 1)`` through the matte of
    ``canvas_paste_blend`` (``feather=None``: alpha 1); the ring keeps the photograph."""
    P, H, W = _membrane_P(P, 'canvas_seamless_apply')
    _, Hc, Wc = _plane_geometry(canvas, 'canvas_seamless_apply')
    _chk(m)
    if tuple(m.shape) != tuple(P.shape) or m.device != canvas.device or P.device != canvas.device:
        raise HimError('canvas_seamless_apply: P and m are (1,3,H,W) on the canvas device')
    membrane_sides(Hc, Wc, x0, y0, H, W, 'canvas_seamless_apply')
    if feather is None:
        if reach != 0 or dist2 is not None:
            raise ValueError('canvas_seamless_apply: reach / dist2 need feather')
        fe, re_, prof = 0, 0, MATTE_PROFILES.get(profile, 1)
    else:
        fe, re_, prof = matte_args(feather, reach, profile, 'canvas_seamless_apply')
    if dist2 is not None:
        if not torch.is_tensor(dist2) or not dist2.is_cuda or dist2.dtype != torch.int32 or dist2.device != canvas.device \
                or tuple(dist2.shape) not in ((H, W), (1, H, W)):
            raise HimError('canvas_seamless_apply: dist2 must be an int32 (%d,%d) tensor on the canvas device' % (H, W))
        dist2 = dist2.contiguous()
    matte = torch.empty((1, 1, H, W), dtype=torch.float32, device=canvas.device) if want_matte else None
    lib.him_canvas_seamless_apply(_p(P), _p(m), _p(canvas), Hc, Wc, int(x0), int(y0), H, W, _p(dist2), fe, re_, prof,
                                  _p(matte), _stream())
    return canvas, matte


def canvas_paste_seamless(cropped, box, canvas, x0, y0, H, W, pre, *, feather=None, reach=0, dist2=None, profile='smooth',
                          want_matte=False):
    """``canvas_paste_bicubic`` in the gradient domain, in place -> ``(canvas, matte or None, status)``.  P, what the hard
    paste would write, comes from the same horizontal pass and ``him_canvas_paste_bicubic_v`` run into an (H,W) scratch
    canvas; the membrane of ``membrane_solve`` moves it onto the photograph's values along the window's border, and
    ``clamp(P + m, 0, 1)`` enters the window's interior through the matte of ``canvas_paste_blend`` (``feather=None``:
    alpha 1 on the interior).  Options are checked on the host before any device work.  Current stream, no host
    synchronisation."""
    H, W = int(H), int(W)
    membrane_sides(canvas.shape[-2], canvas.shape[-1], x0, y0, H, W, 'canvas_paste_seamless')
    if feather is None:
        if reach != 0 or dist2 is not None:
            raise ValueError('canvas_paste_seamless: reach / dist2 need feather')
        if profile not in MATTE_PROFILES:
            raise ValueError('canvas_paste_seamless: profile %r (one of %s)' % (profile, ', '.join(MATTE_PROFILES)))
    else:
        matte_args(feather, reach, profile, 'canvas_paste_seamless')
    scratch = torch.empty((1, 3, H, W), dtype=torch.float32, device=canvas.device)
    _bicubic(cropped, box, H, W, pre, scratch, (0, 0), False)
    m, status = membrane_solve(canvas, x0, y0, scratch)
    _, matte = canvas_seamless_apply(scratch, m, canvas, x0, y0, feather=feather, reach=reach, dist2=dist2, profile=profile,
                                     want_matte=want_matte)
    return canvas, matte, status


# -- region Poisson clone: include/him.h "Region Poisson clone" -----------------------------------------------------------
REGION_POISSON_MAX_N, REGION_POISSON_MAX_ITER = 2048, 1 << 20
REGION_POISSON_EMPTY, REGION_POISSON_SINGULAR, REGION_POISSON_MAX_ITER_HIT, REGION_POISSON_NONFINITE = 1, 2, 4, 8


def region_poisson_args(H, W, mixed, rtol, max_iter, what='region_poisson'):
    """(mixed 0/1, rtol, max_iter) of a region clone on an H x W window, checked on the host: ``mixed`` a bool, ``rtol``
    a float in (0, 1), ``max_iter`` None (the cap 6 (H + W)) or an int in 1..2^20."""
    H, W = int(H), int(W)
    if not 1 <= H <= REGION_POISSON_MAX_N or not 1 <= W <= REGION_POISSON_MAX_N:
        raise ValueError('%s: window %dx%d outside 1..%d per axis' % (what, W, H, REGION_POISSON_MAX_N))
    if not isinstance(mixed, bool):
        raise ValueError('%s: mixed must be True or False, got %r' % (what, mixed))
    if isinstance(rtol, bool) or not isinstance(rtol, (int, float)) or not 0.0 < float(rtol) < 1.0:
        raise ValueError('%s: rtol must be a number in (0, 1), got %r' % (what, rtol))
    if max_iter is None:
        max_iter = 6 * (H + W)
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or not 1 <= max_iter <= REGION_POISSON_MAX_ITER:
        raise ValueError('%s: max_iter must be None or an int in 1..%d, got %r' % (what, REGION_POISSON_MAX_ITER, max_iter))
    return int(mixed), float(rtol), max_iter


def _region_inside(canvas, x0, y0, H, W, what):
    Hc, Wc, x0, y0 = int(canvas.shape[-2]), int(canvas.shape[-1]), int(x0), int(y0)
    if x0 < 0 or y0 < 0 or x0 + W > Wc or y0 + H > Hc:
        raise ValueError('%s: window (%d,%d)+(%d,%d) outside the %dx%d canvas' % (what, x0, y0, W, H, Wc, Hc))


def _region_window(canvas, x0, y0, H, W, what):
    C, Hc, Wc = _plane_geometry(canvas, what)
    if C != 3:
        raise HimError('%s: an RGB canvas, got %d channels' % (what, C))
    return Hc, Wc, int(x0), int(y0)


def _region_plane(region, H, W, device, what):
    if not torch.is_tensor(region) or not region.is_cuda or region.dtype != torch.uint8 or region.device != device \
            or tuple(region.shape) not in ((H, W), (1, H, W)):
        raise HimError('%s: region must be a uint8 (%d,%d) tensor on the canvas device' % (what, H, W))
    return region.contiguous()


def region_poisson_solve(canvas, x0, y0, P, region, *, mixed=False, rtol=1e-7, max_iter=None):
    """``(u, status, resid)``: the correction ``u`` (1,3,H,W) fp64 that makes ``P + u`` the Poisson clone of the patch
    ``P`` (1,3,H,W) into the photo ``canvas`` (1,3,Hc,Wc) on the pixels of ``region`` (uint8 (H,W), nonzero = clone) of the
    window at ``(x0, y0)``, the photograph being Dirichlet data all around them; ``mixed``: per neighbour pair the stronger
    of the patch's and the photograph's gradient.  Conjugate gradients to ``rtol`` (relative residual), at most
    ``max_iter`` iterations (None: 6 (H + W)).  ``status``: int32 ``[sides mask, |Omega|, region pixels dropped on the
    ring, iterations, flags, 0, 0, 0]``, ``resid``: fp64 (3,), both on the device.  Options are checked on the host before
    any device work.  Current stream, no host synchronisation."""
    what = 'region_poisson_solve'
    mixed, rtol, max_iter = region_poisson_args(P.shape[-2], P.shape[-1], mixed, rtol, max_iter, what)
    _region_inside(canvas, x0, y0, P.shape[-2], P.shape[-1], what)
    P, H, W = _membrane_P(P, what)
    Hc, Wc, x0, y0 = _region_window(canvas, x0, y0, H, W, what)
    if P.device != canvas.device:
        raise HimError('%s: canvas and P on one device' % what)
    dev = canvas.device
    region = _region_plane(region, H, W, dev, what)
    with torch.cuda.device(dev):
        u = torch.empty((1, 3, H, W), dtype=torch.float64, device=dev)
        status = torch.empty(8, dtype=torch.int32, device=dev)
        resid = torch.empty(3, dtype=torch.float64, device=dev)
        with _scratch(what, lib.him_region_poisson_ws(H, W)) as ws:
            lib.him_region_poisson_solve(_p(canvas), Hc, Wc, x0, y0, H, W, _p(P), _p(region), mixed, rtol, max_iter, _p(u),
                                         _p(status), _p(resid), _p(ws), ws.numel(), _stream())
    return u, status, resid


def region_poisson_apply(P, u, region, canvas, x0, y0):
    """In place -> ``canvas``: ``clamp(P + u, 0, 1)`` (one fp32 add) on the region's pixels off the ring; nothing else of
    the canvas is read or written."""
    what = 'region_poisson_apply'
    region_poisson_args(P.shape[-2], P.shape[-1], False, 0.5, None, what)
    _region_inside(canvas, x0, y0, P.shape[-2], P.shape[-1], what)
    P, H, W = _membrane_P(P, what)
    Hc, Wc, x0, y0 = _region_window(canvas, x0, y0, H, W, what)
    if not torch.is_tensor(u) or not u.is_cuda or u.dtype != torch.float64 or u.device != canvas.device \
            or P.device != canvas.device or tuple(u.shape) not in ((3, H, W), (1, 3, H, W)):
        raise HimError('%s: u is fp64 (1,3,%d,%d) and P fp32 on the canvas device' % (what, H, W))
    region = _region_plane(region, H, W, canvas.device, what)
    with torch.cuda.device(canvas.device):
        lib.him_region_poisson_apply(_p(P), _p(u.contiguous()), _p(region), _p(canvas), Hc, Wc, x0, y0, H, W, _stream())
    return canvas


def canvas_clone_region(src, src_box, canvas, dst_box, region, *, mixed=False, rtol=1e-7, max_iter=None):
    """Clone the pixels of ``src`` (1,3,Hs,Ws) inside ``src_box`` into ``canvas`` (1,3,Hc,Wc) at ``dst_box`` (both
    ``[xmin, ymin, xmax, ymax)``, as ``layout_place`` takes them), in place -> ``(canvas, status, resid)``.  P is
    ``canvas_crop_bicubic(src, src_box, dh, dw, normalize=False)`` -- Pillow's resize of the source box to the
    destination's size -- cut to the part of ``dst_box`` inside the canvas; that part is the window.  ``region``: a
    canvas-sized uint8 (Hc,Wc) plane (``layout_place``'s ``changed``), read on the window.  ``src`` must not alias
    ``canvas``.  ``region_poisson_solve`` then ``region_poisson_apply``; options are checked on the host before any device
    work.  Current stream, no host synchronisation."""
    what = 'canvas_clone_region'
    sx0, sy0, sx1, sy1 = _layout_box(src_box, what + ': src_box')
    dx0, dy0, dx1, dy1 = _layout_box(dst_box, what + ': dst_box')
    Hs, Ws = int(src.shape[-2]), int(src.shape[-1])
    if sx0 < 0 or sy0 < 0 or sx1 > Ws or sy1 > Hs:
        raise ValueError('%s: src_box [%d, %d, %d, %d) is not inside the %d x %d source' % (what, sx0, sy0, sx1, sy1, Ws, Hs))
    cx0, cy0, cx1, cy1 = _clone_window(what, src, canvas, (dx0, dy0, dx1, dy1), region, mixed, rtol, max_iter)
    P = canvas_crop_bicubic(src, (sx0, sy0, sx1, sy1), dy1 - dy0, dx1 - dx0, normalize=False)
    P = P[:, :, cy0 - dy0:cy1 - dy0, cx0 - dx0:cx1 - dx0].contiguous()
    return _clone_patch(P, canvas, (cx0, cy0, cx1, cy1), region, mixed, rtol, max_iter)


def _clone_window(what, src, canvas, dst_box, region, mixed, rtol, max_iter):
    """``dst_box`` cut to the canvas -> ``(cx0, cy0, cx1, cy1)``, the window of a region clone, with the solve's options
    and the tensors checked on the host."""
    dx0, dy0, dx1, dy1 = dst_box
    Hc, Wc = int(canvas.shape[-2]), int(canvas.shape[-1])
    cx0, cy0, cx1, cy1 = max(dx0, 0), max(dy0, 0), min(dx1, Wc), min(dy1, Hc)
    if cx1 <= cx0 or cy1 <= cy0:
        raise ValueError('%s: dst_box [%d, %d, %d, %d) does not meet the %d x %d canvas' % (what, dx0, dy0, dx1, dy1, Wc, Hc))
    region_poisson_args(cy1 - cy0, cx1 - cx0, mixed, rtol, max_iter, what)
    if src.data_ptr() == canvas.data_ptr() or src.device != canvas.device:
        raise ValueError('%s: src and canvas are two tensors on one device' % what)
    _plane_geometry(canvas, what)
    if not torch.is_tensor(region) or not region.is_cuda or region.dtype != torch.uint8 or region.device != canvas.device \
            or tuple(region.shape) not in ((Hc, Wc), (1, Hc, Wc)):
        raise HimError('%s: region must be a uint8 (%d,%d) tensor on the canvas device' % (what, Hc, Wc))
    return cx0, cy0, cx1, cy1


def _clone_patch(P, canvas, window, region, mixed, rtol, max_iter):
    """The patch ``P`` of the ``window`` Poisson-cloned into ``canvas`` on the window's pixels of the canvas-sized plane
    ``region`` -> ``(canvas, status, resid)``."""
    cx0, cy0, cx1, cy1 = window
    Hc, Wc = int(canvas.shape[-2]), int(canvas.shape[-1])
    part = region.reshape(Hc, Wc)[cy0:cy1, cx0:cx1].contiguous()
    u, status, resid = region_poisson_solve(canvas, cx0, cy0, P, part, mixed=mixed, rtol=rtol, max_iter=max_iter)
    region_poisson_apply(P, u, part, canvas, cx0, cy0)
    return canvas, status, resid


def canvas_paste_window(src, canvas, x0, y0):
    """In place: canvas[0, :, y0:y0+h, x0:x0+w] = src (1,C,h,w) fp32 or int64 (as fp32)."""
    src = src.contiguous()
    if not src.is_cuda or src.dtype not in (torch.float32, torch.int64) or src.dim() != 4 or src.shape[0] != 1:
        raise HimError('canvas_paste_window: one (1,C,h,w) fp32 / int64 device tensor')
    C, Hc, Wc = _plane_geometry(canvas, 'canvas_paste_window')
    if src.shape[1] != C:
        raise HimError('canvas_paste_window: %d channels into a %d-channel canvas' % (src.shape[1], C))
    lib.him_canvas_paste_window(_p(src), 1 if src.dtype == torch.int64 else 0, C, src.shape[2], src.shape[3],
                                _p(canvas), Hc, Wc, int(x0), int(y0), _stream())
    return canvas


# -- tensors to pictures: util.util.tensor2im / tensor2label / tensor2seglabel on the device (include/him.h) ------------
_COLOR_TABLES = {}      # (device index, n_label) -> (device (n,3) uint8 table, the pinned host copy it was uploaded from)
_ID_DTYPES = {torch.float32: 0, torch.uint8: 1, torch.int64: 2}


def _color_table(device, n_label):
    """``Colorize(n_label)``'s table on ``device``: uploaded once per (device, n) from pinned memory on the current stream
    (no host synchronisation) and ordered before every later reader on another stream by an event."""
    from .util.util import labelcolormap
    n = int(n_label)
    if n <= 0:
        raise ValueError('label2color_bytes: n_label must be positive, got %r' % (n_label,))
    key = (device.index if device.index is not None else torch.cuda.current_device(), n)
    hit = _COLOR_TABLES.get(key)
    if hit is None:
        rows = labelcolormap(n)[:n]
        host = torch.empty((rows.shape[0], 3), dtype=torch.uint8, pin_memory=True)
        host.numpy()[...] = rows
        dev = host.to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        hit = _COLOR_TABLES[key] = (dev, host, ev, _stream())
    elif hit[3] != _stream():
        torch.cuda.current_stream(device).wait_event(hit[2])
    return hit[0]


def _picture_input(t, what, dtypes, channels=None):
    if not torch.is_tensor(t) or t.dim() != 3:
        raise ValueError('%s: a (C, H, W) tensor, got %s' % (what, tuple(t.shape) if torch.is_tensor(t) else type(t)))
    if channels is not None and t.shape[0] not in channels:
        raise ValueError('%s: %s channels, got %d' % (what, ' or '.join(str(c) for c in channels), t.shape[0]))
    if t.dtype not in dtypes:
        raise ValueError('%s: %s tensor, got %s' % (what, ' / '.join(str(d) for d in dtypes), t.dtype))
    if 0 in t.shape:
        raise ValueError('%s: empty tensor %s' % (what, tuple(t.shape)))
    if not t.is_cuda:
        t = t.cuda()       # upstream's callers hand in .cpu() tensors
    return t.detach().contiguous()


def tensor2im_bytes(t, normalize=True):
    """(H, W, 3) uint8 device tensor of a (C, H, W) fp32 image, C = 1 or 3: upstream ``tensor2im``'s bytes (one channel is
    written three times).  Current stream, no host synchronisation."""
    t = _picture_input(t, 'tensor2im_bytes', (torch.float32,), channels=(1, 3))
    C, H, W = t.shape
    with torch.cuda.device(t.device):
        dst = torch.empty((H, W, 3), dtype=torch.uint8, device=t.device)
        lib.him_tensor2im_bytes(_p(t), C, H, W, 1 if normalize else 0, _p(dst), _stream())
    return dst


def label2color_bytes(t, n_label, sample=0):
    """(H, W, 3) uint8 device tensor: upstream ``tensor2label``'s label branch.  ``t`` (C, H, W): C > 1 fp32 scores (the
    label is the channel of the maximum, the lowest on a tie), C = 1 an id map (fp32 / uint8 / int64); or a ``LabelCond``,
    whose id map of batch entry ``sample`` is coloured directly -- the one-hot block is not materialised (its dense
    channels are edge maps / masked images in [-1, 1]: they never beat the 1.0 of the id's own channel under the
    lowest-channel tie rule).  Labels outside [0, n_label) are black."""
    if isinstance(t, LabelCond):
        t = t.label[sample]
    if torch.is_tensor(t) and t.dim() == 3 and t.shape[0] > 1 and t.dtype != torch.float32:
        raise ValueError('label2color_bytes: scores are fp32, got %s' % t.dtype)
    t = _picture_input(t, 'label2color_bytes', tuple(_ID_DTYPES))
    C, H, W = t.shape
    with torch.cuda.device(t.device):
        table = _color_table(t.device, n_label)
        dst = torch.empty((H, W, 3), dtype=torch.uint8, device=t.device)
        lib.him_label2color_bytes(_p(t), _ID_DTYPES[t.dtype], C, H, W, _p(table), table.shape[0], _p(dst), _stream())
    return dst


def seglabel_bytes(t):
    """(H, W, C) uint8 device tensor of a (C, H, W) fp32 tensor with values in [0, 255]: upstream ``tensor2seglabel``."""
    t = _picture_input(t, 'seglabel_bytes', (torch.float32,))
    C, H, W = t.shape
    with torch.cuda.device(t.device):
        dst = torch.empty((H, W, C), dtype=torch.uint8, device=t.device)
        lib.him_seglabel_bytes(_p(t), C, H, W, _p(dst), _stream())
    return dst


def bytes_to_host(dev):
    """The host ``numpy`` copy of a uint8 device tensor: one asynchronous copy into a pinned buffer and a wait on the
    current stream only (other streams keep running; nothing but bytes crosses)."""
    host = torch.empty(dev.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(dev, non_blocking=True)
    torch.cuda.current_stream(dev.device).synchronize()
    return host.numpy().copy()


# -- instance-box summary: preprocess_city.construct_box's per-instance loop in one device call (include/him.h) ---------
_INST_KINDS = {torch.uint8: 0, torch.int16: 1, torch.uint16: 1, torch.int32: 2, torch.int64: 3}
_CLS_KINDS = {torch.uint8: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3}
_INST_FLAGS = ((1, 'more than max_objects=%(max)d objects (%(count)d found)'),
               (2, 'an instance id outside 0..65535'),
               (4, 'a class value outside 0..255 (or not integral)'))
_INST_STATE = {}        # (H, W, max_objects, device index) -> status + table, pinned host copy


def inst_summary_launch(inst, cls, min_id=1000, max_objects=1024):
    """Queue the device pass on the current stream; returns the cached state whose ``out`` tensor (2 status ints, then
    ``max_objects`` rows of 7) the kernels fill.  No copy, no host synchronisation (``inst_summary`` adds both)."""
    inst = _planes('inst_summary', 'inst', inst, _INST_KINDS, 'plane')
    cls = _planes('inst_summary', 'cls', cls, _CLS_KINDS, 'plane')
    if inst.shape != cls.shape or inst.device != cls.device:
        raise ValueError('inst_summary: inst %s on %s and cls %s on %s differ' % (tuple(inst.shape), inst.device,
                                                                                tuple(cls.shape), cls.device))
    H, W = inst.shape
    max_objects = int(max_objects)
    if not 1 <= max_objects <= 65536:
        raise ValueError('inst_summary: max_objects must be in 1..65536, got %d' % max_objects)
    with torch.cuda.device(inst.device):
        key = (H, W, max_objects, torch.cuda.current_device())
        st = _INST_STATE.get(key)
        if st is None:
            st = _INST_STATE[key] = dict(
                out=torch.empty(2 + 7 * max_objects, dtype=torch.int32, device=inst.device),
                host=torch.empty(2 + 7 * max_objects, dtype=torch.int32, pin_memory=True))
        out = st['out']
        with _scratch('inst_summary', lib.him_inst_summary_workspace(H, W, max_objects)) as ws:
            lib.him_inst_summary(_p(inst), _INST_KINDS[inst.dtype], _p(cls), _CLS_KINDS[cls.dtype], H, W, int(min_id),
                                 max_objects, _p(out), _p(out) + 8, _p(ws), ws.numel(), _stream())
    return st


def inst_summary(inst, cls, min_id=1000, max_objects=1024):
    """(n, 7) host ``int32`` rows ``id, xmin, ymin, xmax, ymax, count, cls`` of every instance id >= ``min_id`` of the
    device plane ``inst`` (uint8 / 16-bit read as unsigned / int32 / int64, ids 0..65535), ascending id; the box is
    inclusive, ``cls = int(np.median(cls[inst == id]))`` of the device plane ``cls`` (uint8 / int32 / int64 / integral
    fp32, 0..255) -- what upstream's ``construct_box`` stores per object.  One asynchronous copy of status + table into a
    pinned buffer and one wait on the current stream.  ``ValueError`` names an overflow or a value outside its domain."""
    host = _read_back('inst_summary', inst_summary_launch(inst, cls, min_id, max_objects))
    count, flags = int(host[0]), int(host[1])
    if flags:
        why = [text % dict(max=int(max_objects), count=count) for bit, text in _INST_FLAGS if flags & bit]
        raise ValueError('inst_summary: ' + '; '.join(why))
    return host[2:2 + 7 * count].reshape(count, 7).copy()


# -- instance labelling of layouts: connected components of the classes that have instances (include/him.h) -------------
CITYSCAPES_THINGS = tuple(range(24, 34))
CCL_OVERFLOW, CCL_CLS_RANGE = 1, 2
_CCL_FLAGS = ((CCL_OVERFLOW, 'plane %(plane)d: %(count)d objects, more than max_objects=%(max)d or than the ids '
                             '%(base)d..65535 hold'),
              (CCL_CLS_RANGE, 'plane %(plane)d: a class value outside 0..255 (or not integral)'))
_CCL_STATE = {}         # (B, H, W, device index) -> status, pinned host copy, things -> table


def _ccl_things(things):
    try:
        ids = tuple(sorted(set(int(c) for c in things)))
    except (TypeError, ValueError):
        raise ValueError('label_instances: things must be an iterable of class ids')
    for c in ids:
        if not 0 <= c <= 255:
            raise ValueError('label_instances: thing class %d outside 0..255' % c)
    return ids


def label_instances_launch(label, things, connectivity=4, min_area=1, base_id=1000, max_objects=1024):
    """Queue the labelling of one (H, W) plane or a (B, H, W) / (B, 1, H, W) batch of class planes on the current stream;
    returns ``(inst, counts, state)``: a fresh int32 device tensor of the input's shape, the device view of the per-plane
    object counts and the cached per-shape state whose ``out`` tensor (B rows of count, flags) the kernels fill.  No
    copy, no host synchronisation (``label_instances`` adds both).  ``counts`` and ``out`` are overwritten by the next
    launch of the same batch shape on that device."""
    ids = _ccl_things(things)
    planes = _planes('label_instances', 'label', label, _CLS_KINDS, 'hw_first')
    B, H, W = planes.shape
    if H * W > 0x7fffffff:
        raise ValueError('label_instances: %d x %d pixels (at most 2^31 - 1)' % (H, W))
    connectivity, min_area, base_id, max_objects = int(connectivity), int(min_area), int(base_id), int(max_objects)
    if connectivity not in (4, 8):
        raise ValueError('label_instances: connectivity must be 4 or 8, got %d' % connectivity)
    if base_id < 256:
        raise ValueError('label_instances: base_id must be at least 256, got %d' % base_id)
    if not 1 <= max_objects <= 65536:
        raise ValueError('label_instances: max_objects must be in 1..65536, got %d' % max_objects)
    with torch.cuda.device(planes.device):
        key = (B, H, W, torch.cuda.current_device())
        st = _CCL_STATE.get(key)
        nws = lib.him_label_instances_workspace(B, H, W)
        if nws == 0:
            raise ValueError('label_instances: a batch of %d planes of %d x %d is too large' % (B, H, W))
        if st is None:
            st = _CCL_STATE[key] = dict(
                out=torch.empty((B, 2), dtype=torch.int32, device=planes.device),
                host=torch.empty((B, 2), dtype=torch.int32, pin_memory=True), things={})
        table = st['things'].get(ids)
        if table is None:
            host = torch.zeros(256, dtype=torch.uint8)
            if ids:
                host[list(ids)] = 1
            table = st['things'][ids] = host.to(planes.device)
        inst = torch.empty(label.shape, dtype=torch.int32, device=planes.device)
        with _scratch('label_instances', nws) as ws:
            lib.him_label_instances(_p(planes), _CLS_KINDS[planes.dtype], B, H, W, _p(table), connectivity, min_area,
                                    base_id, max_objects, _p(inst), _p(st['out']), _p(ws), ws.numel(), _stream())
    return inst, st['out'][:, 0], st


def label_instances(label, things, connectivity=4, min_area=1, base_id=1000, max_objects=1024):
    """``(inst, counts)``: the instance plane(s) of the class plane(s) ``label`` (uint8 / int32 / int64 / integral fp32
    device tensor, (H, W), (B, H, W) or (B, 1, H, W)) in the Cityscapes convention, and the host ``int32`` array of the
    objects found per plane.  Every maximal ``connectivity``-connected set of at least ``min_area`` pixels of one class
    of ``things`` is an object; objects of a plane get the ids ``base_id``, ``base_id + 1``, ... in raster order of their
    first pixel, every other pixel keeps its class id.  ``inst`` is int32, of the input's shape, on the device.  One
    asynchronous copy of the status into a pinned buffer and one wait on the current stream.  ``ValueError`` names an
    overflow or a class outside its domain."""
    inst, _, st = label_instances_launch(label, things, connectivity, min_area, base_id, max_objects)
    host = _read_back('label_instances', st).copy()
    why = [text % dict(plane=b, count=int(host[b, 0]), max=int(max_objects), base=int(base_id))
           for b in range(host.shape[0]) for bit, text in _CCL_FLAGS if int(host[b, 1]) & bit]
    if why:
        raise ValueError('label_instances: ' + '; '.join(why))
    return inst, host[:, 0].copy()


# -- ADE20K segmentation decode: preprocess_ade's per-image work in one device call (include/him.h) ---------------------
_ADE_STATE = {}         # device index -> status + table, pinned host copy, keep tuple -> tensor


def _ade_keep(keep):
    """``keep`` as a tuple of ints, checked on the host.  Upstream relabels with one in-place rewrite per entry, in list
    order; that equals a table lookup only when no entry repeats and none lies in 1..len(keep) (a position an earlier
    rewrite produced would be rewritten again)."""
    try:
        ids = tuple(int(k) for k in keep)
    except (TypeError, ValueError):
        raise ValueError('ade_decode: keep must be a sequence of class ids')
    if len(ids) > 255:
        raise ValueError('ade_decode: keep has %d entries (at most 255)' % len(ids))
    for k in ids:
        if not 0 <= k <= 65535:
            raise ValueError('ade_decode: keep entry %d outside 0..65535' % k)
        if 1 <= k <= len(ids):
            raise ValueError('ade_decode: keep entry %d lies in 1..%d, where upstream\'s sequential relabel is not a '
                             'lookup' % (k, len(ids)))
    if len(set(ids)) != len(ids):
        raise ValueError('ade_decode: keep holds a duplicate entry')
    return ids


def _ade_seg(seg):
    if not torch.is_tensor(seg) or not seg.is_cuda:
        raise ValueError('ade_decode: seg must be a device tensor')
    if seg.dtype != torch.uint8:
        raise ValueError('ade_decode: seg is %s, accepted: torch.uint8' % seg.dtype)
    if seg.dim() != 3 or seg.shape[2] not in (3, 4) or 0 in seg.shape or not seg.is_contiguous():
        raise ValueError('ade_decode: seg must be a contiguous (H, W, 3 or 4) tensor, got %s' % (tuple(seg.shape),))
    if seg.shape[0] * seg.shape[1] > 0x7fffffff:
        raise ValueError('ade_decode: %d x %d pixels (at most 2^31 - 1)' % (seg.shape[0], seg.shape[1]))
    return seg.detach()


def ade_decode_launch(seg, keep, want_cls=False):
    """Queue the decode of a (H, W, 3|4) uint8 device tensor on the current stream; returns ``(label, inst, cls or None,
    state)``: fresh (H, W) device planes and the cached per-device state whose ``out`` tensor (2 status ints, then 256
    rows of 7) the kernels fill.  No copy of results, no host synchronisation (``ade_decode`` adds both).  The state is
    ONE per device: the next launch on that device overwrites ``out``, so status and table of a launch must be read (or
    copied on the same stream) before the next one is queued -- two launches queued back to back leave the second image's
    rows.  The planes are fresh tensors per launch and are not affected."""
    ids = _ade_keep(keep)
    seg = _ade_seg(seg)
    H, W, pb = seg.shape
    with torch.cuda.device(seg.device):
        key = torch.cuda.current_device()
        st = _ADE_STATE.get(key)
        if st is None:
            st = _ADE_STATE[key] = dict(
                out=torch.empty(2 + 7 * 256, dtype=torch.int32, device=seg.device),
                host=torch.empty(2 + 7 * 256, dtype=torch.int32, pin_memory=True), keep={})
        kdev = st['keep'].get(ids)
        if kdev is None:
            import numpy as np
            kdev = st['keep'][ids] = torch.from_numpy(np.array(ids if ids else [0], dtype=np.uint16)).to(seg.device)
        label = torch.empty((H, W), dtype=torch.uint8, device=seg.device)
        inst = torch.empty((H, W), dtype=torch.uint8, device=seg.device)
        cls = torch.empty((H, W), dtype=torch.uint16, device=seg.device) if want_cls else None
        out = st['out']
        with _scratch('ade_decode', lib.him_ade_decode_workspace()) as ws:
            lib.him_ade_decode(_p(seg), H, W, pb, _p(kdev), len(ids), _p(cls) if want_cls else 0, _p(label), _p(inst),
                               _p(out), _p(out) + 8, _p(ws), ws.numel(), _stream())
    return label, inst, cls, st


def ade_decode(seg, keep, want_cls=False):
    """``(label, inst, rows[, cls])`` of one ADE20K ``_seg.png`` held as a (H, W, 3|4) uint8 device tensor: ``label`` the
    1-based position of the pixel's class ``(R // 10) * 256 + G`` in ``keep`` (0: not kept), ``inst`` the rank of its B
    value among the image's distinct B values, both (H, W) uint8 device planes; ``rows`` an (n, 7) host ``int32`` array
    ``rank, b, xmin, ymin, xmax, ymax, count`` (inclusive zero-based box), one row per B value in ascending rank; ``cls``
    (``want_cls``) the raw classes as a uint16 device plane.  One asynchronous copy of status + table into a pinned buffer
    and one wait on the current stream.  ``ValueError`` for a ``seg`` or a ``keep`` outside the contract."""
    label, inst, cls, st = ade_decode_launch(seg, keep, want_cls)
    host = _read_back('ade_decode', st)
    count = int(host[0])
    rows = host[2:2 + 7 * count].reshape(count, 7).copy()
    return (label, inst, rows, cls) if want_cls else (label, inst, rows)


# -- evaluation metrics: SSIM / error sums and the confusion matrix in one device call each (include/him.h) -------------
_PRED_KINDS = {torch.uint8: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3}
CONF_SKIPPED, CONF_SATURATED = 1, 2


def _metric_image(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError('image_metrics: %s must be a device tensor' % what)
    if t.dtype != torch.float32:
        raise ValueError('image_metrics: %s is %s, accepted: torch.float32' % (what, t.dtype))
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[1] not in (1, 3) or 0 in t.shape:
        raise ValueError('image_metrics: %s must be (B, 1 or 3, H, W), got %s' % (what, tuple(t.shape)))
    return t.detach().contiguous()


def image_metrics(a, b, *, scale, offset, quantize, data_range, box=None, want_map=False):
    """``(sums, map)`` of two (B, C, H, W) fp32 device batches, C = 1 or 3: ``sums`` (B, C, 5) float64 on the device =
    [sum of SSIM over the windows, windows, sum of squared error, sum of absolute error, pixels] per plane after the
    mapping ``x * scale + offset`` (and ``trunc(clip(., 0, 255))`` with ``quantize``); ``map`` the (B, C, H-10, W-10)
    SSIM map with ``want_map`` (whole-image calls only), else None.  ``box``: (B, 4) int32 device tensor of inclusive
    ``(xmin, ymin, xmax, ymax)``, or None.  Current stream, no host synchronisation."""
    a, b = _metric_image(a, 'a'), _metric_image(b, 'b')
    if a.shape != b.shape or a.device != b.device:
        raise ValueError('image_metrics: a %s on %s and b %s on %s differ' % (tuple(a.shape), a.device, tuple(b.shape),
                                                                              b.device))
    B, C, H, W = a.shape
    if box is not None:
        if not torch.is_tensor(box) or not box.is_cuda or box.dtype != torch.int32 or tuple(box.shape) != (B, 4):
            raise ValueError('image_metrics: box must be a (%d, 4) int32 device tensor' % B)
        if want_map:
            raise ValueError('image_metrics: the map is written for whole-image calls only')
        box = box.contiguous()
    if want_map and (H < 11 or W < 11):
        raise ValueError('image_metrics: no 11x11 window fits a %dx%d image' % (H, W))
    with torch.cuda.device(a.device):
        sums = torch.empty((B, C, 5), dtype=torch.float64, device=a.device)
        smap = torch.empty((B, C, H - 10, W - 10), dtype=torch.float32, device=a.device) if want_map else None
        with _scratch('image_metrics', lib.him_image_metrics_workspace(B, C, H, W)) as ws:
            lib.him_image_metrics(_p(a), _p(b), B, C, H, W, float(scale), float(offset), 1 if quantize else 0,
                                  float(data_range), _p(box), _p(sums), _p(smap), _p(ws), ws.numel(), _stream())
    return sums, smap


def confusion(pred, gt, n, *, mask=None, ignore=-1, per_sample=False, out=None, pred_kind=None):
    """``(counts, status)``: the int64 confusion matrix (B or 1, n, n) of ``pred`` against ``gt`` (row = ground truth,
    column = prediction) and the 2-int status record (skipped pixels, flag bits), both on the device.  ``pred``: uint8 /
    int32 / int64 / integral fp32 ids, or fp32 scores (B, C > 1, H, W) (arg-max, lowest channel on a tie), or with
    ``pred_kind='prob'`` fp32 probabilities thresholded at 0.5.  ``mask``: fp32, pixels count where it is not 0.
    ``out``: the pair an earlier call returned; the call then adds into it.  Current stream, no host synchronisation."""
    gt = _planes('confusion', 'gt', gt, _PRED_KINDS, 'nchw')
    pred = _planes('confusion', 'pred', pred, _PRED_KINDS, 'nchw', channels=True)
    if pred_kind == 'prob':
        kind = 5
    elif pred_kind == 'scores' or (pred_kind is None and pred.dtype == torch.float32 and pred.shape[1] > 1):
        kind = 4
    elif pred_kind in (None, 'ids'):
        kind = _PRED_KINDS[pred.dtype]
    else:
        raise ValueError("confusion: pred_kind %r (None, 'ids', 'scores' or 'prob')" % (pred_kind,))
    if kind in (4, 5) and pred.dtype != torch.float32:
        raise ValueError('confusion: scores and probabilities are fp32, got %s' % pred.dtype)
    if kind != 4 and pred.shape[1] != 1:
        raise ValueError('confusion: id / probability planes have one channel, got %s' % (tuple(pred.shape),))
    B, C, H, W = pred.shape
    if tuple(gt.shape) != (B, 1, H, W) or gt.device != pred.device:
        raise ValueError('confusion: pred %s and gt %s differ' % (tuple(pred.shape), tuple(gt.shape)))
    if mask is not None:
        mask = _planes('confusion', 'mask', mask, (torch.float32,), 'nchw')
        if tuple(mask.shape) != (B, 1, H, W) or mask.device != pred.device:
            raise ValueError('confusion: mask %s does not fit pred %s' % (tuple(mask.shape), tuple(pred.shape)))
    n = int(n)
    if not 1 <= n <= 256:
        raise ValueError('confusion: n must be in 1..256, got %d' % n)
    rows = B if per_sample else 1
    with torch.cuda.device(pred.device):
        if out is None:
            counts = torch.empty((rows, n, n), dtype=torch.int64, device=pred.device)
            status = torch.empty(2, dtype=torch.int32, device=pred.device)
        else:
            counts, status = out
            if counts.dtype != torch.int64 or tuple(counts.shape) != (rows, n, n) or not counts.is_contiguous() \
                    or counts.device != pred.device or status.dtype != torch.int32 or status.numel() != 2:
                raise ValueError('confusion: out must be the (counts (%d, %d, %d) int64, status (2,) int32) pair of an '
                                 'earlier call' % (rows, n, n))
        with _scratch('confusion', lib.him_confusion_workspace(n)) as ws:
            lib.him_confusion(_p(pred), kind, _p(gt), _PRED_KINDS[gt.dtype], _p(mask), B, C, H, W, n, int(ignore),
                              1 if per_sample else 0, 0 if out is None else 1, _p(counts), _p(status), _p(ws),
                              ws.numel(), _stream())
    return counts, status


# -- distance transform and boundary statistics (include/him.h "Distance transform and boundary metrics") --------------
EDT_RULES = {'nonzero': 0, 'equals': 1, 'boundary_of': 2, 'any_boundary': 3}
EDT_NONE, EDT_BAD_JOB, _EDT_MAX_SIDE = 2 ** 31 - 1, 1, 16384


def _edt_jobs(jobs, device, what):
    if not torch.is_tensor(jobs) or not jobs.is_cuda or jobs.dtype != torch.int32 or jobs.dim() != 2 \
            or jobs.shape[1] != 3 or jobs.shape[0] < 1 or jobs.device != device:
        raise ValueError('%s: jobs must be a (K >= 1, 3) int32 tensor on the device of src' % what)
    return jobs.contiguous()


def edt_jobs(B, values, rule, device):
    """The (B * len(values), 3) int32 job table [plane, value, rule] on ``device``, plane-major, built by device ops."""
    rule = EDT_RULES[rule] if isinstance(rule, str) else int(rule)
    n = len(values)
    with torch.cuda.device(device):
        k = torch.arange(B * n, dtype=torch.int32, device=device)
        plane = torch.div(k, n, rounding_mode='floor')
        if list(values) == list(range(values[0], values[0] + n)):
            value = k - plane * n + int(values[0])
        else:
            value = torch.tensor(list(values), dtype=torch.int32).to(device)[(k - plane * n).long()]
        return torch.stack([plane, value, torch.full_like(k, rule)], 1).contiguous()


def distance_transform(src, jobs=None, value=None, rule='nonzero', want_nearest=False):
    """``(dist2, nearest or None, status)`` on the device: for each job the exact squared Euclidean distance (int32,
    (K, H, W)) from every pixel to the nearest seed of the job's plane, the seed's index ``y * W + x`` (the smallest among
    equidistant ones; -1 without a seed) and the (K, 2) record [seed count, flag bits].  ``src``: uint8 / int32 / int64 /
    integral fp32 ids, (B, H, W).  ``jobs``: a (K, 3) int32 device table [plane, value, rule number]; None runs one job
    per plane with ``rule`` in ``EDT_RULES`` and ``value``.  ``EDT_NONE`` marks a job without a seed.  Current stream,
    no host synchronisation, no autograd."""
    src = _planes('distance_transform', 'src', src, _PRED_KINDS, 'planes', max_side=_EDT_MAX_SIDE)
    B, H, W = src.shape
    if jobs is None:
        if rule not in EDT_RULES:
            raise ValueError('distance_transform: rule %r (one of %s)' % (rule, ', '.join(EDT_RULES)))
        jobs = edt_jobs(B, [0 if value is None else int(value)], rule, src.device)
    jobs = _edt_jobs(jobs, src.device, 'distance_transform')
    K = jobs.shape[0]
    with torch.cuda.device(src.device):
        dist2 = torch.empty((K, H, W), dtype=torch.int32, device=src.device)
        nearest = torch.empty((K, H, W), dtype=torch.int32, device=src.device) if want_nearest else None
        status = torch.empty((K, 2), dtype=torch.int32, device=src.device)
        with _scratch('distance_transform', lib.him_edt_workspace(K, H, W)) as ws:
            lib.him_edt(_p(src), _PRED_KINDS[src.dtype], B, H, W, _p(jobs), K, _p(dist2), _p(nearest), _p(status), _p(ws),
                        ws.numel(), _stream())
    return dist2, nearest, status


def boundary_stats(src, jobs, dist2, tol2):
    """``(counts, sumd)`` on the device: per job over its seeds of ``src``, int64 (K, 4) [seeds, seeds with
    ``dist2 <= tol2``, the largest reachable ``dist2`` (-1: none), seeds with ``dist2 == EDT_NONE``] and the float64 (K,)
    sum of ``sqrt(dist2)`` over the reachable seeds, added in a fixed order.  ``dist2``: the (K, H, W) result of
    ``distance_transform`` over the other map with the same job table.  Current stream, no host synchronisation."""
    src = _planes('boundary_stats', 'src', src, _PRED_KINDS, 'planes', max_side=_EDT_MAX_SIDE)
    B, H, W = src.shape
    jobs = _edt_jobs(jobs, src.device, 'boundary_stats')
    K = jobs.shape[0]
    if not torch.is_tensor(dist2) or dist2.dtype != torch.int32 or tuple(dist2.shape) != (K, H, W) \
            or dist2.device != src.device:
        raise ValueError('boundary_stats: dist2 must be a (%d, %d, %d) int32 tensor on the device of src' % (K, H, W))
    tol2 = int(tol2)
    if tol2 < 0:
        raise ValueError('boundary_stats: tol2 must not be negative, got %d' % tol2)
    dist2 = dist2.contiguous()
    with torch.cuda.device(src.device):
        counts = torch.empty((K, 4), dtype=torch.int64, device=src.device)
        sumd = torch.empty(K, dtype=torch.float64, device=src.device)
        with _scratch('boundary_stats', lib.him_boundary_stats_workspace(K, H, W)) as ws:
            lib.him_boundary_stats(_p(src), _PRED_KINDS[src.dtype], B, H, W, _p(jobs), K, _p(dist2), tol2, _p(counts),
                                   _p(sumd), _p(ws), ws.numel(), _stream())
    return counts, sumd


def label_ids(pred, pred_kind):
    """int32 ids (B, H, W) on the device of fp32 scores (B, C, H, W) (``pred_kind='scores'``: the channel of the maximum,
    the lowest on a tie) or probabilities (B, 1, H, W) (``'prob'``: p > 0.5), the rules of ``confusion``."""
    if pred_kind not in ('scores', 'prob'):
        raise ValueError("label_ids: pred_kind %r ('scores' or 'prob')" % (pred_kind,))
    pred = _planes('confusion', 'pred', pred, (torch.float32,), 'nchw', channels=True)
    B, C, H, W = pred.shape
    if pred_kind == 'prob' and C != 1:
        raise ValueError('label_ids: probability planes have one channel, got %s' % (tuple(pred.shape),))
    with torch.cuda.device(pred.device):
        ids = torch.empty((B, H, W), dtype=torch.int32, device=pred.device)
        lib.him_label_ids(_p(pred), 4 if pred_kind == 'scores' else 5, B, C, H, W, _p(ids), _stream())
    return ids


# -- layout edits: take an instance out and fill the hole, write an instance elsewhere (include/him.h "Layout edits") ----
LAYOUT_NO_SEED, LAYOUT_CLASS_RANGE = 1, 2
LAYOUT_MAX_CLASS = 65536
LAYOUT_MAX_COORD = 1 << 20
_LAYOUT_TABLES = {}     # (class ids, n_class, device index) -> device class bit table
_LAYOUT_INDEX = {}      # (source length, destination length, device index) -> device NEAREST index table
_LAYOUT_ID_RANGE = {torch.uint8: (0, 255), torch.int32: (-2 ** 31, 2 ** 31 - 1), torch.int64: (-2 ** 31, 2 ** 31 - 1),
                    torch.float32: (-2 ** 24, 2 ** 24)}


def _layout_int(v, what, lo, hi):
    import numbers
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lo <= int(v) <= hi:
        raise ValueError('%s must be an integer in %d..%d, got %r' % (what, lo, hi, v))
    return int(v)


def _layout_classes(classes, n_class, what):
    try:
        ids = tuple(sorted(set(int(c) for c in classes)))
    except (TypeError, ValueError):
        raise ValueError('%s must be an iterable of class ids' % what)
    for c in ids:
        if not 0 <= c < n_class:
            raise ValueError('%s: class %d outside 0..%d' % (what, c, n_class - 1))
    return ids


def _layout_table(ids, n_class, device):
    """The device bit table of the class ids over [0, n_class): uint32 words, class c is bit c & 31 of word c >> 5."""
    import numpy as np
    key = (ids, n_class, device.index)
    table = _LAYOUT_TABLES.get(key)
    if table is None:
        words = np.zeros((n_class + 31) // 32, np.uint32)
        for c in ids:
            words[c >> 5] |= np.uint32(1 << (c & 31))
        if len(_LAYOUT_TABLES) > 256:
            _LAYOUT_TABLES.clear()
        table = _LAYOUT_TABLES[key] = torch.from_numpy(words.view(np.int32)).to(device)
    return table


def _layout_index(src_len, dst_len, device):
    import numpy as np
    from .data import resample
    key = (src_len, dst_len, device.index)
    tab = _LAYOUT_INDEX.get(key)
    if tab is None:
        if len(_LAYOUT_INDEX) > 256:
            _LAYOUT_INDEX.clear()
        tab = _LAYOUT_INDEX[key] = torch.from_numpy(np.ascontiguousarray(resample.nearest_table(src_len, dst_len),
                                                                         np.int32)).to(device)
    return tab


def _layout_box(box, what):
    try:
        x0, y0, x1, y1 = (v for v in box)
    except (TypeError, ValueError):
        raise ValueError('%s must be [xmin, ymin, xmax, ymax), got %r' % (what, box))
    x0, y0, x1, y1 = (_layout_int(v, what, -LAYOUT_MAX_COORD, LAYOUT_MAX_COORD) for v in (x0, y0, x1, y1))
    if x1 <= x0 or y1 <= y0:
        raise ValueError('%s [%d, %d, %d, %d) is empty' % (what, x0, y0, x1, y1))
    return x0, y0, x1, y1


def layout_erase(label, inst, id=None, *, region=None, fill, n_class):
    """Take the region R out of a (label, inst) canvas pair: ``(label_out, inst_out, changed, status)`` on the device.
    R is ``inst == id`` or, given instead, the nonzero pixels of ``region`` (uint8 / bool, one (H, W) plane).  Every
    pixel of R takes label and instance id of the nearest pixel outside R whose class is in ``fill`` (an iterable of
    class ids below ``n_class``): exact squared Euclidean distance, the smallest ``y * W + x`` among equidistant ones
    (``distance_transform``'s rule; the transform is the same kernel).  Everything else is copied.  ``label`` / ``inst``:
    uint8 / int32 / int64 / integral fp32 device planes, (H, W), (1, H, W) or (1, 1, H, W); the outputs have their dtype
    and shape.  ``changed``: uint8 (H, W), 1 where the label changed.  ``status``: int32 (4,) [|R|, seeds, changed pixels,
    flags]; ``LAYOUT_NO_SEED``: no pixel of an allowed class, the outputs are copies; ``LAYOUT_CLASS_RANGE``: a label
    outside [0, n_class) was seen (never a seed, never rewritten).  Current stream, no host synchronisation, no autograd."""
    if (id is None) == (region is None):
        raise ValueError('layout_erase: give an instance id or a region plane, not both')
    if region is None:
        id = _layout_int(id, 'layout_erase: id', -2 ** 31, 2 ** 31 - 1)
    n_class = _layout_int(n_class, 'layout_erase: n_class', 1, LAYOUT_MAX_CLASS)
    fill = _layout_classes(fill, n_class, 'layout_erase: fill')
    lab = _planes('layout_erase: label', 'src', label, _PRED_KINDS, 'planes', max_side=_EDT_MAX_SIDE, single=True)
    ins = _planes('layout_erase: inst', 'src', inst, _PRED_KINDS, 'planes', max_side=_EDT_MAX_SIDE, single=True)
    if lab.shape != ins.shape or lab.device != ins.device:
        raise ValueError('layout_erase: label %s on %s and inst %s on %s differ' % (tuple(lab.shape), lab.device,
                                                                                 tuple(ins.shape), ins.device))
    H, W = lab.shape
    if region is not None:
        if not torch.is_tensor(region) or not region.is_cuda or region.dtype not in (torch.uint8, torch.bool) or \
                region.device != lab.device or region.numel() != H * W or tuple(region.shape[-2:]) != (H, W):
            raise ValueError('layout_erase: region must be a uint8 / bool (%d, %d) plane on the device of label' % (H, W))
        region = region.detach().contiguous().view(torch.uint8)
        id = 0
    table = _layout_table(fill, n_class, lab.device)
    with torch.cuda.device(lab.device):
        label_out, inst_out = torch.empty_like(lab), torch.empty_like(ins)
        changed = torch.empty((H, W), dtype=torch.uint8, device=lab.device)
        status = torch.empty(4, dtype=torch.int32, device=lab.device)
        with _scratch('layout_erase', lib.him_layout_erase_workspace(H, W)) as ws:
            lib.him_layout_erase(_p(lab), _PRED_KINDS[lab.dtype], _p(ins), _PRED_KINDS[ins.dtype], _p(region), id, H, W,
                                 _p(table), n_class, _p(label_out), _p(inst_out), _p(changed), _p(status), _p(ws),
                                 ws.numel(), _stream())
    return label_out.reshape(label.shape), inst_out.reshape(inst.shape), changed, status


def _layout_place_args(what, label_dst, inst_dst, inst_src, id, src_box, dst_box, cls, new_id, protect):
    """The checked arguments of a place, separable or affine: ``(dst_box, id, src_box, cls, new_id, n_class, protect's
    device table or None, label plane, instance plane, source plane)``; ValueError for anything refused."""
    id = _layout_int(id, what + ': id', -2 ** 31, 2 ** 31 - 1)
    sx0, sy0, sx1, sy1 = _layout_box(src_box, what + ': src_box')
    dst_box = _layout_box(dst_box, what + ': dst_box')
    _layout_int(cls, what + ': cls', -2 ** 31, 2 ** 31 - 1)
    _layout_int(new_id, what + ': new_id', -2 ** 31, 2 ** 31 - 1)
    prot = _layout_classes(protect, LAYOUT_MAX_CLASS, what + ': protect')
    n_class = prot[-1] + 1 if prot else 1
    lab = _planes(what + ': label_dst', 'src', label_dst, _PRED_KINDS, 'planes', max_side=_EDT_MAX_SIDE, single=True)
    ins = _planes(what + ': inst_dst', 'src', inst_dst, _PRED_KINDS, 'planes', max_side=_EDT_MAX_SIDE, single=True)
    src = _planes(what + ': inst_src', 'src', inst_src, _PRED_KINDS, 'planes', max_side=_EDT_MAX_SIDE, single=True)
    if lab.shape != ins.shape or lab.device != ins.device or src.device != lab.device:
        raise ValueError('%s: label_dst %s on %s, inst_dst %s on %s and inst_src on %s differ'
                         % (what, tuple(lab.shape), lab.device, tuple(ins.shape), ins.device, src.device))
    if src.dtype != ins.dtype:
        raise ValueError('%s: inst_src is %s, inst_dst %s' % (what, src.dtype, ins.dtype))
    Hs, Ws = src.shape
    if sx0 < 0 or sy0 < 0 or sx1 > Ws or sy1 > Hs:
        raise ValueError('%s: src_box [%d, %d, %d, %d) is not inside the %d x %d plane' % (what, sx0, sy0, sx1, sy1, Ws, Hs))
    cls = _layout_int(cls, '%s: cls (%s plane)' % (what, lab.dtype), *_LAYOUT_ID_RANGE[lab.dtype])
    new_id = _layout_int(new_id, '%s: new_id (%s plane)' % (what, ins.dtype), *_LAYOUT_ID_RANGE[ins.dtype])
    table = _layout_table(prot, n_class, lab.device) if prot else None
    return dst_box, id, (sx0, sy0, sx1, sy1), cls, new_id, n_class, table, lab, ins, src


def layout_place(label_dst, inst_dst, inst_src, id, src_box, dst_box, cls, new_id, *, protect=()):
    """Write the instance ``id`` of the plane ``inst_src``, cut out by ``src_box`` and resized to ``dst_box`` (both
    ``[xmin, ymin, xmax, ymax)``), onto copies of the pair ``label_dst`` / ``inst_dst``: ``(label_out, inst_out, changed,
    status)`` on the device.  The resized mask is bit-identical to Pillow's ``Image.resize(NEAREST)`` of the cropped mask
    (``data/resample.nearest_table``); ``dst_box`` may hang over the canvas, that part is clipped.  Where the mask is set
    the pixel becomes class ``cls``, instance ``new_id``, except where its current class is in ``protect``: those stay
    in front.  ``changed``: uint8 (H, W), 1 on the written pixels.  ``status``: int32 (6,) [written, blocked, xmin, ymin,
    xmax, ymax of the written pixels, inclusive as ``inst_summary``'s rows; (2^31 - 1, 2^31 - 1, -1, -1) when none].
    Planes as ``layout_erase`` takes them; ``inst_src`` has the dtype of ``inst_dst``.  Current stream, no host
    synchronisation, no autograd."""
    (dx0, dy0, dx1, dy1), id, (sx0, sy0, sx1, sy1), cls, new_id, n_class, table, lab, ins, src = _layout_place_args(
        'layout_place', label_dst, inst_dst, inst_src, id, src_box, dst_box, cls, new_id, protect)
    Hd, Wd = lab.shape
    Hs, Ws = src.shape
    with torch.cuda.device(lab.device):
        xs = _layout_index(sx1 - sx0, dx1 - dx0, lab.device)
        ys = _layout_index(sy1 - sy0, dy1 - dy0, lab.device)
        label_out, inst_out = lab.clone(), ins.clone()
        changed = torch.zeros((Hd, Wd), dtype=torch.uint8, device=lab.device)
        status = torch.empty(6, dtype=torch.int32, device=lab.device)
        lib.him_layout_place(_p(src), _PRED_KINDS[src.dtype], Hs, Ws, id, sx0, sy0, sx1, sy1, _p(xs), _p(ys),
                             _p(label_out), _PRED_KINDS[lab.dtype], _p(inst_out), Hd, Wd, dx0, dy0, dx1, dy1, cls, new_id,
                             _p(table), n_class, _p(changed), _p(status), _stream())
    return label_out.reshape(label_dst.shape), inst_out.reshape(inst_dst.shape), changed, status


# -- affine layout edits: include/him.h "Affine layout edits" ------------------------------------------------------------
AFFINE_FRAC_BITS = 24
AFFINE_MAX_LINEAR, AFFINE_MAX_OFFSET = 1 << 30, 1 << 52
AffineMap = collections.namedtuple('AffineMap', ('inv', 'fwd', 'dst_box', 'src_box'))
AffineMap.__doc__ = """An affine edit of a source box: ``inv``, the six ints [a00, a01, a02, a10, a11, a12] of the inverse
map in units of 2^-24 source pixel as the device takes them; ``fwd``, the float64 2 x 3 forward map (read-only);
``dst_box`` ``[xmin, ymin, xmax, ymax)``: the forward image of the source box's pixel squares, rounded outwards;
``src_box`` as given."""


def _affine_pair(v, what, scalar_ok=False):
    import math
    import numbers
    if scalar_ok and isinstance(v, numbers.Real) and not isinstance(v, bool):
        v = (v, v)
    try:
        a, b = v
        if isinstance(a, bool) or isinstance(b, bool):
            raise TypeError
        a, b = float(a), float(b)
    except (TypeError, ValueError):
        raise ValueError('%s must be %stwo numbers, got %r' % (what, 'a number or ' if scalar_ok else '', v))
    if not (math.isfinite(a) and math.isfinite(b)):
        raise ValueError('%s must be finite, got %r' % (what, v))
    return a, b


def affine_map(src_box, *, angle=0.0, scale=1.0, shear=0.0, flip='', shift=(0, 0), dst_center=None):
    """The ``AffineMap`` that turns the pixels of ``src_box`` (``[xmin, ymin, xmax, ymax)``, as ``layout_place`` takes it)
    about the box's centre: mirror (``flip``, a subset of ``'xy'``: ``'x'`` reverses the columns), scale (a number or
    ``(sx, sy)``), shear (``shear``: the tangent of a horizontal shear, x += shear * y), then rotate by ``angle`` degrees
    counter-clockwise as seen on the picture (y points down: ``Image.rotate``'s sense), and put the centre at
    ``dst_center`` (None: the source box's centre) plus ``shift``.  Pixel index i has its centre at coordinate i.

    When the linear part is a signed permutation matrix (quarter turns and flips, scale 1, shear 0) the centre is snapped
    by at most half a pixel towards +x / +y so that pixel centres land on pixel centres: every fraction of the map is
    zero, the nearest rule meets no tie and the bicubic weights are exactly (0, 1, 0, 0): the edit permutes pixels.

    The device samples points: NEAREST for ids, the 4 x 4 Keys cubic for pixels, with no prefilter.  Below scale 1 this
    aliases, because Pillow's resize widens its support there and this map does not; hence the bound on the minification.
    ValueError: a non-finite parameter, a singular value of the linear part outside [1/4, 4], ``|shear| > 2``, a flip
    that is no subset of ``'xy'``, a destination beyond the coordinates the device accepts."""
    import fractions
    import math
    import numbers
    import numpy as np
    what = 'affine_map'
    sx0, sy0, sx1, sy1 = _layout_box(src_box, what + ': src_box')
    for name, v in (('angle', angle), ('shear', shear)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
            raise ValueError('%s: %s must be a finite number, got %r' % (what, name, v))
    angle, shear = float(angle), float(shear)
    kx, ky = _affine_pair(scale, what + ': scale', scalar_ok=True)
    shx, shy = _affine_pair(shift, what + ': shift')
    if abs(shear) > 2.0:
        raise ValueError('%s: |shear| > 2, got %r' % (what, shear))
    if not isinstance(flip, str) or len(set(flip)) != len(flip) or not set(flip) <= set('xy'):
        raise ValueError("%s: flip must be a subset of 'xy', got %r" % (what, flip))
    quarter = angle % 90.0 == 0.0
    if quarter:
        c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(angle // 90.0) % 4]
    else:
        c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    fx, fy = (-1.0 if 'x' in flip else 1.0), (-1.0 if 'y' in flip else 1.0)
    L = np.array([[c, s], [-s, c]]) @ np.array([[1.0, shear], [0.0, 1.0]]) @ np.diag([kx * fx, ky * fy])
    sv = np.linalg.svd(L, compute_uv=False)
    if not (sv.max() <= 4.0 * (1 + 1e-12) and sv.min() >= 0.25 * (1 - 1e-12)):
        raise ValueError('%s: the singular values %s of the linear part leave [1/4, 4]' % (what, sv.tolist()))
    permutation = quarter and kx == 1.0 and ky == 1.0 and shear == 0.0
    cs = np.array([(sx0 + sx1 - 1) / 2.0, (sy0 + sy1 - 1) / 2.0])
    cd = (cs if dst_center is None else np.array(_affine_pair(dst_center, what + ': dst_center'))) + np.array([shx, shy])
    if permutation:
        L = np.rint(L)                                   # exact already; -0.0 -> a plain zero after the sums below
        t = L @ cs
        cd = t + np.floor(cd - t + 0.5)
        Linv = L.T.copy()
    else:
        det = L[0, 0] * L[1, 1] - L[0, 1] * L[1, 0]
        Linv = np.array([[L[1, 1], -L[0, 1]], [-L[1, 0], L[0, 0]]]) / det
    off = cs - Linv @ cd
    one = float(1 << AFFINE_FRAC_BITS)
    inv = tuple(int(math.floor(float(v) * one + 0.5))
                for v in (Linv[0, 0], Linv[0, 1], off[0], Linv[1, 0], Linv[1, 1], off[1]))
    if max(abs(inv[k]) for k in (0, 1, 3, 4)) > AFFINE_MAX_LINEAR or max(abs(inv[2]), abs(inv[5])) > AFFINE_MAX_OFFSET:
        raise ValueError('%s: the inverse map %s leaves the coefficients the device accepts' % (what, list(inv)))
    fwd = np.concatenate([L, (cd - L @ cs)[:, None]], axis=1) + 0.0
    fwd.setflags(write=False)
    # the destination box from the integer map itself, in exact rationals: the corners of the source box's pixel squares
    # (U in [sx0 - 1/2, sx1 - 1/2) in 2^-24 units) through the inverse of [a00 a01; a10 a11]
    a00, a01, a02, a10, a11, a12 = inv
    det = a00 * a11 - a01 * a10
    half = 1 << (AFFINE_FRAC_BITS - 1)
    xs, ys = [], []
    for U in ((sx0 << AFFINE_FRAC_BITS) - half, (sx1 << AFFINE_FRAC_BITS) - half):
        for V in ((sy0 << AFFINE_FRAC_BITS) - half, (sy1 << AFFINE_FRAC_BITS) - half):
            xs.append(fractions.Fraction(a11 * (U - a02) - a01 * (V - a12), det))
            ys.append(fractions.Fraction(a00 * (V - a12) - a10 * (U - a02), det))
    dx0, dy0 = math.ceil(min(xs)), math.ceil(min(ys))
    dx1, dy1 = max(math.floor(max(xs)) + 1, dx0 + 1), max(math.floor(max(ys)) + 1, dy0 + 1)
    if min(dx0, dy0) < -LAYOUT_MAX_COORD or max(dx1, dy1) > LAYOUT_MAX_COORD:
        raise ValueError('%s: dst_box [%d, %d, %d, %d) beyond +-2^20' % (what, dx0, dy0, dx1, dy1))
    return AffineMap(inv, fwd, (dx0, dy0, dx1, dy1), (sx0, sy0, sx1, sy1))


def _affine_inv(amap, what):
    """The six coefficients of ``amap`` as a host int64 array for the C ABI (the call copies them)."""
    if not isinstance(amap, AffineMap):
        raise ValueError('%s: amap must be the AffineMap ops.affine_map returns, got %r' % (what, type(amap).__name__))
    try:
        n = len(amap.inv)
    except TypeError:
        n = -1
    if n != 6:
        raise ValueError('%s: amap.inv has six coefficients, got %r' % (what, amap.inv))
    inv = tuple(_layout_int(v, what + ': amap.inv', -lim, lim)
                for v, lim in zip(amap.inv, (AFFINE_MAX_LINEAR, AFFINE_MAX_LINEAR, AFFINE_MAX_OFFSET) * 2))
    return (ctypes.c_longlong * 6)(*inv)


def layout_place_affine(label_dst, inst_dst, inst_src, id, amap, cls, new_id, *, protect=()):
    """``layout_place`` through the affine edit ``amap`` (``affine_map``): the instance ``id`` of the plane ``inst_src``
    inside ``amap.src_box``, resampled NEAREST through the inverse map -- destination pixel (x, y) reads the source pixel
    ``((U + 2^23) >> 24, (V + 2^23) >> 24)``, unset when that lies outside the source box -- onto copies of the pair
    ``label_dst`` / ``inst_dst`` over ``amap.dst_box`` (clipped to the canvas).  Everything else, the four results
    ``(label_out, inst_out, changed, status)`` included, as ``layout_place``.  Current stream, no host synchronisation,
    no table upload, no autograd."""
    what = 'layout_place_affine'
    inv = _affine_inv(amap, what)
    (dx0, dy0, dx1, dy1), id, (sx0, sy0, sx1, sy1), cls, new_id, n_class, table, lab, ins, src = _layout_place_args(
        what, label_dst, inst_dst, inst_src, id, amap.src_box, amap.dst_box, cls, new_id, protect)
    Hd, Wd = lab.shape
    Hs, Ws = src.shape
    with torch.cuda.device(lab.device):
        label_out, inst_out = lab.clone(), ins.clone()
        changed = torch.zeros((Hd, Wd), dtype=torch.uint8, device=lab.device)
        status = torch.empty(6, dtype=torch.int32, device=lab.device)
        lib.him_layout_place_affine(_p(src), _PRED_KINDS[src.dtype], Hs, Ws, id, sx0, sy0, sx1, sy1,
                                    ctypes.addressof(inv), _p(label_out), _PRED_KINDS[lab.dtype], _p(inst_out), Hd, Wd,
                                    dx0, dy0, dx1, dy1, cls, new_id, _p(table), n_class, _p(changed), _p(status), _stream())
    return label_out.reshape(label_dst.shape), inst_out.reshape(inst_dst.shape), changed, status


def _affine_window(window, what):
    try:
        x0, y0, H, W = window
    except (TypeError, ValueError):
        raise ValueError('%s: window must be (x0, y0, H, W), got %r' % (what, window))
    x0, y0 = (_layout_int(v, what + ': window origin', -LAYOUT_MAX_COORD, LAYOUT_MAX_COORD) for v in (x0, y0))
    H, W = (_layout_int(v, what + ': window size', 1, REGION_POISSON_MAX_N) for v in (H, W))
    return x0, y0, H, W


def canvas_warp_affine(src, amap, window):
    """``P`` (1,3,H,W) fp32: the RGB planes ``src`` (1,3,Hs,Ws) seen through the affine edit ``amap`` on the ``window``
    ``(x0, y0, H, W)`` of the destination canvas: ``P[0, c, y, x]`` is the bicubic sample (Keys, a = -0.5, 4 x 4 taps
    clamped to the source plane, fp64 weights and sums narrowed once) of channel c at the source point the inverse map
    gives for the destination pixel ``(x0 + x, y0 + y)``.  No 8-bit round trip and no clamp: the cubic's overshoot stays.
    H, W in 1..2048.  Current stream, no host synchronisation, no autograd."""
    what = 'canvas_warp_affine'
    inv = _affine_inv(amap, what)
    x0, y0, H, W = _affine_window(window, what)
    C, Hs, Ws = _plane_geometry(src, what)
    if C != 3 or max(Hs, Ws) > _EDT_MAX_SIDE:
        raise HimError('%s: RGB planes with sides up to %d, got %s' % (what, _EDT_MAX_SIDE, tuple(src.shape)))
    with torch.cuda.device(src.device):
        P = torch.empty((1, 3, H, W), dtype=torch.float32, device=src.device)
        lib.him_canvas_warp_affine(_p(src), Hs, Ws, ctypes.addressof(inv), x0, y0, H, W, _p(P), _stream())
    return P


def canvas_clone_region_affine(src, amap, canvas, region, *, mixed=False, rtol=1e-7, max_iter=None):
    """``canvas_clone_region`` through the affine edit ``amap``: the patch is ``canvas_warp_affine(src, amap, window)``
    with the window = ``amap.dst_box`` cut to the canvas, Poisson-cloned in place into ``canvas`` (1,3,Hc,Wc) on the
    nonzero pixels of the canvas-sized uint8 plane ``region`` (``layout_place_affine``'s ``changed``) -> ``(canvas,
    status, resid)``.  ``region_poisson_solve`` then ``region_poisson_apply``, unchanged; options are checked on the host
    before any device work.  ``src`` must not alias ``canvas``.  Current stream, no host synchronisation."""
    what = 'canvas_clone_region_affine'
    _affine_inv(amap, what)
    dst_box = _layout_box(amap.dst_box, what + ': amap.dst_box')
    cx0, cy0, cx1, cy1 = _clone_window(what, src, canvas, dst_box, region, mixed, rtol, max_iter)
    P = canvas_warp_affine(src, amap, (cx0, cy0, cy1 - cy0, cx1 - cx0))
    return _clone_patch(P, canvas, (cx0, cy0, cx1, cy1), region, mixed, rtol, max_iter)


# -- boundary-weighted and surface losses (include/him.h "Boundary-weighted and surface losses") ------------------------
def _bw_args(what, amp, sigma):
    amp, sigma = float(amp), float(sigma)
    if not (amp >= 0.0 and amp != float('inf')) or not (sigma > 0.0 and sigma != float('inf')):
        raise ValueError('%s: amp >= 0 and sigma > 0, both finite, got amp=%r sigma=%r' % (what, amp, sigma))
    return amp, sigma


def _bw_planes(what, shape, **ts):
    """The named fp32 device tensors of ``shape``, contiguous; ValueError for anything else."""
    out = []
    for name, t in ts.items():
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError('%s: %s must be a device tensor' % (what, name))
        if t.dtype != torch.float32:
            raise ValueError('%s: %s is %s, not float32' % (what, name, t.dtype))
        if tuple(t.shape) != tuple(shape):
            raise ValueError('%s: %s is %s, expected %s' % (what, name, tuple(t.shape), tuple(shape)))
        out.append(t.contiguous())
    return out


def _bw_dist(what, d, shape, device):
    if not torch.is_tensor(d) or not d.is_cuda or d.dtype != torch.int32 or tuple(d.shape) != tuple(shape) \
            or d.device != device:
        raise ValueError('%s: a distance plane must be a %s int32 tensor on the device of the input' % (what, tuple(shape)))
    return d.contiguous()


def boundary_dist2(planes):
    """int32 (B,H,W): squared distance of every pixel to the nearest class boundary of its own id plane (``planes``:
    (B,1,H,W) or (B,H,W) integral ids, fp32 included) -- one 'any_boundary' job per sample over the whole plane;
    ``EDT_NONE`` on a plane of one value."""
    return distance_transform(planes, rule='any_boundary')[0]


def surface_dists(t):
    """``(d2_fg, d2_bg)``, int32 (B,H,W) each: squared distances to the nearest pixel with ``t == 1`` and with ``t == 0``
    of the 0/1 mask ``t`` ((B,1,H,W) or (B,H,W)), two 'equals' jobs per sample in one transform."""
    t = _planes('surface_dists', 'src', t, _PRED_KINDS, 'planes', max_side=_EDT_MAX_SIDE)
    B, H, W = t.shape
    d2 = distance_transform(t, jobs=edt_jobs(B, [0, 1], 'equals', t.device))[0].view(B, 2, H, W)
    return d2[:, 1].contiguous(), d2[:, 0].contiguous()


def _bw_ws(like):
    nb = lib.him_bw_loss_ws()
    return torch.empty(max((int(nb) + 7) // 8, 1), dtype=torch.float64, device=like.device), nb


class _BWNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, label, mask, dist2, amp, sigma):
        ctx.set_materialize_grads(False)
        B, Cn, H, W = logp.shape
        with torch.cuda.device(logp.device):
            out2 = torch.empty(2, dtype=torch.float32, device=logp.device)
            ws, nb = _bw_ws(logp)
            lib.him_bw_nll_fwd(_p(logp), _p(label), _p(mask), _p(dist2), B, Cn, H * W, amp, sigma, _p(out2), _p(ws), nb,
                               _stream())
        ctx.label, ctx.mask, ctx.dist2, ctx.sum_w = label, mask, dist2, out2[1:2]
        ctx.shape, ctx.amp, ctx.sigma = (B, Cn, H, W), amp, sigma
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None, None
        B, Cn, H, W = ctx.shape
        g = g.contiguous()
        with torch.cuda.device(g.device):
            d = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
            lib.him_bw_nll_bwd(_p(ctx.label), _p(ctx.mask), _p(ctx.dist2), _p(g), _p(ctx.sum_w), ctx.amp, ctx.sigma, _p(d),
                               B, Cn, H * W, _stream())
        return d, None, None, None, None, None


def boundary_weighted_nll(logp, label, mask, amp, sigma, dist2=None):
    """``masked_nll`` with the weight ``1 + amp * exp(-d2 / (2 sigma^2))`` on every valid position, d2 the squared
    distance to the nearest class boundary of the ground-truth ``label`` plane (weight 1 on a plane of one class):
    ``sum w * -logp[label] / sum w`` over the positions with ``mask >= 0.5`` and an id in ``0..C-1``.  ``logp`` (B,C,H,W),
    ``label`` / ``mask`` (B,1,H,W); ``dist2``: the int32 (B,H,W) result of ``boundary_dist2(label)`` to share one
    transform, None computes it.  No gradient flows into the targets or through the distances."""
    what = 'boundary_weighted_nll'
    amp, sigma = _bw_args(what, amp, sigma)
    if not torch.is_tensor(logp) or logp.dim() != 4:
        raise ValueError('%s: logp must be a (B, C, H, W) device tensor' % what)
    B, _, H, W = logp.shape
    (logp,) = _bw_planes(what, logp.shape, logp=logp)
    label, mask = _bw_planes(what, (B, 1, H, W), **{k: v.detach() if torch.is_tensor(v) else v
                                                    for k, v in (('label', label), ('mask', mask))})
    dist2 = boundary_dist2(label) if dist2 is None else _bw_dist(what, dist2, (B, H, W), logp.device)
    return _BWNLL.apply(logp, label, mask, dist2, amp, sigma)


class _BWPair(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t, dist2, kind, amp, sigma):
        ctx.set_materialize_grads(False)
        with torch.cuda.device(p.device):
            out2 = torch.empty(2, dtype=torch.float32, device=p.device)
            ws, nb = _bw_ws(p)
            lib.him_bw_pair_fwd(_p(p), _p(t), _p(dist2), p.numel(), kind, amp, sigma, _p(out2), _p(ws), nb, _stream())
        ctx.p, ctx.t, ctx.dist2, ctx.sum_w, ctx.kind, ctx.amp, ctx.sigma = p, t, dist2, out2[1:2], kind, amp, sigma
        return out2[0]

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None, None, None
        g = g.contiguous()
        with torch.cuda.device(g.device):
            dp = torch.empty_like(ctx.p)
            lib.him_bw_pair_bwd(_p(ctx.p), _p(ctx.t), _p(ctx.dist2), ctx.p.numel(), ctx.kind, _p(g), _p(ctx.sum_w), ctx.amp,
                                ctx.sigma, _p(dp), _stream())
        return dp, None, None, None, None, None


def _bw_pair(what, kind, p, t, amp, sigma, dist2):
    amp, sigma = _bw_args(what, amp, sigma)
    if not torch.is_tensor(p) or p.dim() != 4 or p.shape[1] != 1:
        raise ValueError('%s: p must be a (B, 1, H, W) device tensor' % what)
    p, t = _bw_planes(what, p.shape, p=p, t=t.detach() if torch.is_tensor(t) else t)
    B, _, H, W = p.shape
    dist2 = boundary_dist2(t) if dist2 is None else _bw_dist(what, dist2, (B, H, W), p.device)
    return _BWPair.apply(p, t, dist2, kind, amp, sigma)


def boundary_weighted_bce(p, t, amp, sigma, dist2=None):
    """``bce_mean`` with the weight ``1 + amp * exp(-d2 / (2 sigma^2))``, d2 the squared distance to the outline of the
    0/1 mask ``t``: ``sum w * bce / sum w`` over all positions.  ``p``, ``t`` (B,1,H,W); ``dist2``: the int32 (B,H,W)
    result of ``boundary_dist2(t)`` to share one transform, None computes it."""
    return _bw_pair('boundary_weighted_bce', 0, p, t, amp, sigma, dist2)


def boundary_weighted_l1(p, t, amp, sigma, dist2=None):
    """``l1_mean`` with the weight of ``boundary_weighted_bce``."""
    return _bw_pair('boundary_weighted_l1', 1, p, t, amp, sigma, dist2)


class _Surface(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t, d2_fg, d2_bg):
        ctx.set_materialize_grads(False)
        B, _, H, W = p.shape
        with torch.cuda.device(p.device):
            out = torch.empty((), dtype=torch.float32, device=p.device)
            ws, nb = _bw_ws(p)
            lib.him_surface_fwd(_p(p), _p(t), _p(d2_fg), _p(d2_bg), B, H, W, _p(out), _p(ws), nb, _stream())
        ctx.t, ctx.d2_fg, ctx.d2_bg, ctx.shape = t, d2_fg, d2_bg, (B, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        B, H, W = ctx.shape
        g = g.contiguous()
        with torch.cuda.device(g.device):
            dp = torch.empty_like(ctx.t)
            lib.him_surface_bwd(_p(ctx.t), _p(ctx.d2_fg), _p(ctx.d2_bg), B, H, W, _p(g), _p(dp), _stream())
        return dp, None, None, None


def surface_loss(p, t, dists=None):
    """The surface term of Kervadec et al. on the probability ``p`` against the 0/1 mask ``t`` (both (B,1,H,W)):
    ``sum phi * p / (B*H*W * sqrt(H^2 + W^2))`` with phi the signed distance to the outline of ``t`` -- ``+sqrt(d2_fg)``
    outside the mask, ``-sqrt(d2_bg)`` inside, 0 for an empty or a full mask.  Negative where the prediction sits inside
    the mask; lowering it pulls the probability mass towards the mask and lowers the surface distance.  ``dists``: the
    pair of ``surface_dists(t)`` to share one transform, None computes it."""
    what = 'surface_loss'
    if not torch.is_tensor(p) or p.dim() != 4 or p.shape[1] != 1:
        raise ValueError('%s: p must be a (B, 1, H, W) device tensor' % what)
    p, t = _bw_planes(what, p.shape, p=p, t=t.detach() if torch.is_tensor(t) else t)
    B, _, H, W = p.shape
    if dists is None:
        dists = surface_dists(t)
    if not isinstance(dists, (tuple, list)) or len(dists) != 2:
        raise ValueError('%s: dists must be the pair (d2_fg, d2_bg)' % what)
    d2_fg, d2_bg = (_bw_dist(what, d, (B, H, W), p.device) for d in dists)
    return _Surface.apply(p, t, d2_fg, d2_bg)


# -- panoptic matching: segments, overlaps, unique matches, per-class tp / fp / fn (include/him.h "Panoptic matching") ---
PQ_OVERFLOW, PQ_ID_RANGE, PQ_CLS_RANGE, PQ_MIXED, PQ_CCL = 1, 2, 4, 8, 16
_SEG_KINDS = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}


def panoptic_match(pred_seg, pred_cls, gt_seg, gt_cls, n_class, *, mask=None, ignore=-1, max_segments=1024, out=None,
                   want_matches=False):
    """``(counts, iou_sum, status, matches or None)`` on the device: per class the int64 (n_class, 3) tp / fp / fn of the
    predicted segments against the ground-truth ones (matched at IoU > 0.5 within a class, void taken out), the float64
    (n_class,) sum of the matched IoUs, the int32 (B, 4) record [ground-truth segments, predicted segments, flag bits, 0]
    and, with ``want_matches``, the int32 (B, max_segments, 6) rows id, class, area, matched predicted id or -1, inter,
    union of every ground-truth segment.  ``*_seg``: uint8 / int32 / int64 ids 0..65535; ``*_cls``: uint8 / int32 / int64 /
    integral fp32 classes; ``mask``: fp32, void where 0; ``ignore``: a ground-truth class that is void.  ``out``: the
    (counts, iou_sum, status) triple an earlier call returned; the call then adds into it.  Current stream, no host
    synchronisation."""
    pred_seg = _planes('panoptic_match', 'pred_seg', pred_seg, _SEG_KINDS, 'planes')
    pred_cls = _planes('panoptic_match', 'pred_cls', pred_cls, _PRED_KINDS, 'planes')
    gt_seg = _planes('panoptic_match', 'gt_seg', gt_seg, _SEG_KINDS, 'planes')
    gt_cls = _planes('panoptic_match', 'gt_cls', gt_cls, _PRED_KINDS, 'planes')
    B, H, W = pred_seg.shape
    for what, t in (('pred_cls', pred_cls), ('gt_seg', gt_seg), ('gt_cls', gt_cls)):
        if tuple(t.shape) != (B, H, W) or t.device != pred_seg.device:
            raise ValueError('panoptic_match: pred_seg %s and %s %s differ' % (tuple(pred_seg.shape), what, tuple(t.shape)))
    if mask is not None:
        mask = _planes('panoptic_match', 'mask', mask, (torch.float32,), 'planes')
        if tuple(mask.shape) != (B, H, W) or mask.device != pred_seg.device:
            raise ValueError('panoptic_match: mask %s does not fit pred_seg %s' % (tuple(mask.shape), (B, H, W)))
    n_class, max_segments, ignore = int(n_class), int(max_segments), int(ignore)
    if not 1 <= n_class <= 256:
        raise ValueError('panoptic_match: n_class must be in 1..256, got %d' % n_class)
    if not 1 <= max_segments <= 4096:
        raise ValueError('panoptic_match: max_segments must be in 1..4096, got %d' % max_segments)
    if ignore < -1 or H * W > 0x7fffffff or B > 65535:
        raise ValueError('panoptic_match: ignore %d (-1 or a class), planes of %d x %d (at most 2^31 - 1 pixels), batch %d '
                         '(at most 65535)' % (ignore, H, W, B))
    dev = pred_seg.device
    with torch.cuda.device(dev):
        if out is None:
            counts = torch.empty((n_class, 3), dtype=torch.int64, device=dev)
            iou_sum = torch.empty(n_class, dtype=torch.float64, device=dev)
            status = torch.empty((B, 4), dtype=torch.int32, device=dev)
        else:
            counts, iou_sum, status = out[:3]
            ok = all(torch.is_tensor(t) and t.device == dev and t.is_contiguous() for t in (counts, iou_sum, status))
            if not ok or counts.dtype != torch.int64 or tuple(counts.shape) != (n_class, 3) \
                    or iou_sum.dtype != torch.float64 or tuple(iou_sum.shape) != (n_class,) \
                    or status.dtype != torch.int32 or tuple(status.shape) != (B, 4):
                raise ValueError('panoptic_match: out must be the (counts (%d, 3) int64, iou_sum (%d,) float64, status '
                                 '(%d, 4) int32) triple of an earlier call' % (n_class, n_class, B))
        matches = torch.empty((B, max_segments, 6), dtype=torch.int32, device=dev) if want_matches else None
        with _scratch('panoptic_match', lib.him_panoptic_match_workspace(B, max_segments)) as ws:
            lib.him_panoptic_match(_p(pred_seg), _SEG_KINDS[pred_seg.dtype], _p(pred_cls), _PRED_KINDS[pred_cls.dtype],
                                   _p(gt_seg), _SEG_KINDS[gt_seg.dtype], _p(gt_cls), _PRED_KINDS[gt_cls.dtype], _p(mask), B,
                                   H, W, n_class, ignore, max_segments, 0 if out is None else 1, _p(counts), _p(iou_sum),
                                   _p(matches), _p(status), _p(ws), ws.numel(), _stream())
    return counts, iou_sum, status, matches


# -- set-level metrics: Laplacian pyramid, segmented sort, sliced Wasserstein distance (include/him.h "Set-level metrics")
SWD_PATCH, SORT_LDS_MAX, SWD_ZERO_DEVIATION = 7, 8192, 1


def _swd_f32(t, what, dim):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError('%s must be a device tensor' % what)
    if t.dtype != torch.float32 or t.dim() != dim:
        raise ValueError('%s must be a %d-dimensional fp32 tensor, got %s %s' % (what, dim, t.dtype, tuple(t.shape)))
    return t.detach().contiguous()


def lap_levels(H, W, levels=None):
    """The number of pyramid levels of an H x W image: the most that keep min(H, W) >= 16, or ``levels`` if smaller."""
    return int(lib.him_lap_levels(int(H), int(W), 0 if levels is None else int(levels)))


def lap_pyramid(x, levels=None, want_gauss=False):
    """The Laplacian pyramid of a planar fp32 device batch (B, C, H, W), C = 1 or 3: a list of ``levels`` tensors
    (B, C, H >> l, W >> l), finest first, views of one packed buffer; with ``want_gauss`` also the list of the Gaussian
    levels 1 .. levels - 1.  Five-tap binomial filter, mirrored borders; the last level is the Gaussian one.  H and W
    must be divisible by 2^(levels - 1).  Current stream, no host synchronisation, no autograd."""
    x = _swd_f32(x, 'lap_pyramid: x', 4)
    B, C, H, W = x.shape
    L = lap_levels(H, W, levels)
    if levels is not None and int(levels) != L:
        raise ValueError('lap_pyramid: %d levels asked, an image of %d x %d has %d' % (int(levels), H, W, L))
    need = int(lib.him_lap_pyramid_ws(B, C, H, W, L)) if L >= 1 else 0
    if need == 0:
        raise ValueError('lap_pyramid: (B, C, H, W) = %s refused: C is 1 or 3, min(H, W) >= 16, and H and W are '
                         'divisible by 2^(levels - 1)' % (tuple(x.shape),))
    off = [int(lib.him_lap_level_offset(B, C, H, W, l)) for l in range(L + 1)]
    with torch.cuda.device(x.device):
        lap = torch.empty(off[L], dtype=torch.float32, device=x.device)
        gauss = torch.empty(max(off[L] - off[1], 1), dtype=torch.float32, device=x.device) if want_gauss else None
        with _scratch('lap_pyramid', need) as ws:
            lib.him_lap_pyramid(_p(x), B, C, H, W, L, _p(lap), _p(gauss), _p(ws), ws.numel(), _stream())
    laps = [lap[off[l]:off[l + 1]].view(B, C, H >> l, W >> l) for l in range(L)]
    if not want_gauss:
        return laps
    return laps, [gauss[off[l] - off[1]:off[l + 1] - off[1]].view(B, C, H >> l, W >> l) for l in range(1, L)]


def swd_stats(C, device):
    """Fresh channel accumulators of ``swd_gather``: (C, 4) float64 [sum, sum of squares, minimum, maximum]."""
    with torch.cuda.device(device):
        return torch.tensor([[0.0, 0.0, float('inf'), float('-inf')]] * int(C), dtype=torch.float64).to(device)


def swd_gather(level, pos, desc, row0, stats, status):
    """Copies the 7 x 7 x C patches of ``level`` (B, C, h, w) at the corners ``pos`` (B, n, 2) int32 (y, x) into the rows
    ``row0 ...`` of ``desc`` (capacity, 49 C), folds them into ``stats`` (``swd_stats``) and adds the number of clamped
    corners to the int32 ``status[0]``.  Everything on the device and in place; returns the row behind the last one."""
    level = _swd_f32(level, 'swd_gather: level', 4)
    B, C, h, w = level.shape
    if not torch.is_tensor(pos) or pos.dtype != torch.int32 or pos.dim() != 3 or pos.shape[0] != B or pos.shape[2] != 2 \
            or pos.device != level.device:
        raise ValueError('swd_gather: pos must be a (B, n_patches, 2) int32 tensor on the device of level')
    n = pos.shape[1]
    if desc.dtype != torch.float32 or desc.dim() != 2 or desc.shape[1] != 49 * C or not desc.is_contiguous() \
            or desc.device != level.device:
        raise ValueError('swd_gather: desc must be a contiguous (capacity, %d) fp32 tensor on the device of level' % (49 * C))
    if stats.dtype != torch.float64 or tuple(stats.shape) != (C, 4) or not stats.is_contiguous() \
            or status.dtype != torch.int32 or not status.is_cuda:
        raise ValueError('swd_gather: stats must be (C, 4) float64 and status int32, both on the device')
    pos = pos.contiguous()
    with torch.cuda.device(level.device):
        with _scratch('swd_gather', lib.him_swd_gather_ws(B, C)) as ws:
            lib.him_swd_gather(_p(level), B, C, h, w, _p(pos), n, _p(desc), desc.shape[0], int(row0), _p(stats), _p(status),
                               _p(ws), ws.numel(), _stream())
    return int(row0) + B * n


def swd_project(desc, stats, dirs, status=None):
    """``(out, status)``: the (n_dirs, N) fp32 projections of the N rows of ``desc`` (N, 49 C), normalised per channel
    with the mean and population deviation derived on the device from ``stats``, onto the columns of ``dirs``
    (49 C, n_dirs).  ``status[0]`` gains SWD_ZERO_DEVIATION (and ``out`` is NaN) when a channel does not vary."""
    desc, dirs = _swd_f32(desc, 'swd_project: desc', 2), _swd_f32(dirs, 'swd_project: dirs', 2)
    N, K = desc.shape
    if K not in (49, 147) or dirs.shape[0] != K or N < 1:
        raise ValueError('swd_project: desc %s against dirs %s' % (tuple(desc.shape), tuple(dirs.shape)))
    with torch.cuda.device(desc.device):
        out = torch.empty((dirs.shape[1], N), dtype=torch.float32, device=desc.device)
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=desc.device)
        lib.him_swd_project(_p(desc), N, K // 49, _p(stats), _p(dirs), dirs.shape[1], _p(out), _p(status), _stream())
    return out, status


def sort_segments(keys):
    """Sorts every row of the (S, N) (or (N,)) fp32 device tensor ``keys`` in place, ascending in the order of the
    sign-fixed bit pattern (-0 before +0, +inf before NaN); returns ``(keys, status)`` with the int32 ``status[0]`` the
    number of NaNs.  Rows of up to SORT_LDS_MAX keys are sorted in LDS, longer ones by merge passes through the cached
    workspace, at least of the size of ``keys``.  Exact, identical bits from run to run.  Current stream, no host synchronisation."""
    if not torch.is_tensor(keys) or not keys.is_cuda:
        raise ValueError('sort_segments: keys must be a device tensor')
    if keys.dtype != torch.float32 or keys.dim() not in (1, 2) or not keys.is_contiguous() or keys.numel() == 0:
        raise ValueError('sort_segments: keys must be a contiguous, non-empty (S, N) or (N,) fp32 tensor')
    S, N = (1, keys.shape[0]) if keys.dim() == 1 else keys.shape
    if S * N > 2 ** 31 - 1:
        raise ValueError('sort_segments: %d x %d keys, at most 2^31 - 1 per call' % (S, N))
    with torch.cuda.device(keys.device):
        status = torch.empty(1, dtype=torch.int32, device=keys.device)
        with _scratch('sort_segments', lib.him_sort_segments_ws(S, N)) as ws:
            lib.him_sort_segments(_p(keys), S, N, _p(status), _p(ws), ws.numel(), _stream())
    return keys, status


def sliced_wasserstein(desc_a, desc_b, stats_a, stats_b, dirs):
    """One level's sliced Wasserstein distance between two descriptor sets: ``(distance, dir_sums, status)`` on the
    device, a float64 scalar (NaN when a channel of either set does not vary), the (n_dirs,) float64 sums of
    |a_sorted - b_sorted| and the int32 flag word of ``swd_project``.  Both sets must hold the same number of rows."""
    if desc_a.shape[0] != desc_b.shape[0]:
        raise ValueError('sliced_wasserstein: the sets hold %d and %d descriptors' % (desc_a.shape[0], desc_b.shape[0]))
    pa, status = swd_project(desc_a, stats_a, dirs)
    pb, _ = swd_project(desc_b, stats_b, dirs, status)
    sort_segments(pa)
    sort_segments(pb)
    n_dirs, N = pa.shape
    with torch.cuda.device(pa.device):
        dir_sums = torch.empty(n_dirs, dtype=torch.float64, device=pa.device)
        mean = torch.empty((), dtype=torch.float64, device=pa.device)
        lib.him_swd_distance(_p(pa), N, _p(pb), N, n_dirs, _p(dir_sums), _p(mean), _stream())
    return mean, dir_sums, status


# -- feature-space set metrics: descriptor pooling, streaming moments, KID kernel sums (include/him.h "Feature-space set
# metrics")
FEAT_MAX_DIM, KID_BAD_INDEX = 4096, 1


def _feat_matrix(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError('%s must be a device tensor' % what)
    if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.shape[1] < 1:
        raise ValueError('%s must be a contiguous (rows, D) fp32 tensor, got %s %s' % (what, t.dtype, tuple(t.shape)))
    return t.detach()


def feat_pool(x, feat, row0, c0=0):
    """Writes the plane means of the fp32 device feature maps ``x`` (B, C, h, w) to ``feat[row0 + b, c0 + c]`` of the
    contiguous (capacity, D) fp32 device matrix ``feat``, in place: summed in double, rounded once.  Several maps are
    concatenated into one row by one call each with its own ``c0``.  Returns the column behind the last one written.
    Current stream, no host synchronisation, no autograd."""
    x = _swd_f32(x, 'feat_pool: x', 4)
    feat = _feat_matrix(feat, 'feat_pool: feat')
    if feat.device != x.device:
        raise ValueError('feat_pool: feat must be on the device of x')
    B, C, h, w = x.shape
    row0, c0 = int(row0), int(c0)
    if B < 1 or C < 1 or h < 1 or w < 1 or row0 < 0 or row0 + B > feat.shape[0] or c0 < 0 or c0 + C > feat.shape[1]:
        raise ValueError('feat_pool: x %s does not fit rows [%d, %d) and columns [%d, %d) of feat %s'
                         % (tuple(x.shape), row0, row0 + B, c0, c0 + C, tuple(feat.shape)))
    with torch.cuda.device(x.device):
        lib.him_feat_pool(_p(x), B, C, h, w, _p(feat), feat.shape[0], row0, feat.shape[1], c0, _stream())
    return c0 + C


def feat_moment_buffers(D, device):
    """Fresh accumulators of ``feat_moments``: ``(sum (D,), second (D, D))`` float64 zeros on ``device``."""
    D = int(D)
    if D < 1 or D > FEAT_MAX_DIM:
        raise ValueError('feat_moments: D %d outside 1..%d' % (D, FEAT_MAX_DIM))
    with torch.cuda.device(device):
        return torch.zeros(D, dtype=torch.float64, device=device), torch.zeros((D, D), dtype=torch.float64, device=device)


def feat_moments(feat, row0, n, sum, second):
    """Adds the column sums and X^T X of the rows ``row0 .. row0 + n - 1`` of the (rows, D) fp32 device matrix ``feat``
    to the float64 device accumulators ``sum`` (D,) and ``second`` (D, D) (``feat_moment_buffers``), in place; exact
    products on the fp64 matrix instruction, both triangles of ``second`` identical.  Returns ``(sum, second)``."""
    feat = _feat_matrix(feat, 'feat_moments: feat')
    D, row0, n = feat.shape[1], int(row0), int(n)
    if D > FEAT_MAX_DIM:
        raise ValueError('feat_moments: D %d outside 1..%d' % (D, FEAT_MAX_DIM))
    if n < 1 or row0 < 0 or row0 + n > feat.shape[0]:
        raise ValueError('feat_moments: rows [%d, %d) outside feat %s' % (row0, row0 + n, tuple(feat.shape)))
    for t, shape, what in ((sum, (D,), 'sum'), (second, (D, D), 'second')):
        if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() \
                or t.device != feat.device:
            raise ValueError('feat_moments: %s must be a contiguous %s float64 tensor on the device of feat' % (what, shape))
    with torch.cuda.device(feat.device):
        with _scratch('feat_moments', lib.him_feat_moments_ws(n, D)) as ws:
            lib.him_feat_moments(_p(feat), row0, n, D, _p(sum), _p(second), _p(ws), ws.numel(), _stream())
    return sum, second


def kid_sums(x, y, ix, iy, gamma=0.0, coef0=1.0, status=None):
    """``(out, status)``: for every row s of the int32 device index tables ``ix`` / ``iy`` (n_subsets, m) the float64
    sums ``out[s] = [sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j)]`` over the indexed rows
    of the fp32 device matrices ``x`` (nx, D) and ``y`` (ny, D), k(a, b) = (gamma a.b + coef0)^3, ``gamma == 0`` meaning
    1 / D; the diagonal is excluded by position.  Dot products on the fp64 matrix instruction; the Gram matrix is never
    stored.  An index outside its matrix sets KID_BAD_INDEX in the int32 ``status[0]`` and makes its subset NaN."""
    x, y = _feat_matrix(x, 'kid_sums: x'), _feat_matrix(y, 'kid_sums: y')
    if y.device != x.device or y.shape[1] != x.shape[1] or x.shape[0] < 1 or y.shape[0] < 1:
        raise ValueError('kid_sums: x %s and y %s must be non-empty, of one row length and on one device'
                         % (tuple(x.shape), tuple(y.shape)))
    for t in (ix, iy):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError('kid_sums: ix and iy must be device tensors')
        if t.dtype != torch.int32 or t.dim() != 2 or not t.is_contiguous() or t.device != x.device or t.shape != ix.shape:
            raise ValueError('kid_sums: ix and iy must be contiguous (n_subsets, m) int32 tensors of one shape on the '
                             'device of x')
    n_subsets, m = ix.shape
    gamma, coef0 = float(gamma), float(coef0)
    with torch.cuda.device(x.device):
        need = int(lib.him_kid_sums_ws(n_subsets, m))
        if need == 0 or not 0.0 <= gamma < float('inf') or coef0 != coef0 or abs(coef0) == float('inf'):
            raise ValueError('kid_sums: n_subsets %d (1..65535), m %d (2..65536), gamma %r (>= 0), coef0 %r (finite)'
                             % (n_subsets, m, gamma, coef0))
        out = torch.empty((n_subsets, 3), dtype=torch.float64, device=x.device)
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=x.device)
        elif not torch.is_tensor(status) or status.dtype != torch.int32 or not status.is_cuda:
            raise ValueError('kid_sums: status must be an int32 device tensor')
        with _scratch('kid_sums', need) as ws:
            lib.him_kid_sums(_p(x), x.shape[0], _p(y), y.shape[0], x.shape[1], _p(ix), _p(iy), n_subsets, m, gamma, coef0,
                             _p(out), _p(status), _p(ws), ws.numel(), _stream())
    return out, status


# -- k-nearest-neighbour manifold estimates: radii and membership counts (include/him.h, him_knn_radii / him_knn_membership)
KNN_MAX_K, KNN_NONFINITE = 16, 1


def _knn_status(status, device, what):
    if status is None:
        return torch.zeros(1, dtype=torch.int32, device=device)
    if not torch.is_tensor(status) or status.dtype != torch.int32 or not status.is_cuda or status.device != device:
        raise ValueError('%s: status must be an int32 device tensor on the device of the rows' % what)
    return status


def knn_radii(x, k, status=None):
    """``(radii2, status)``: ``radii2[i]``, float64, is the k-th smallest squared Euclidean distance from row i of the
    fp32 device matrix ``x`` (n, D) to its other rows (self excluded by position: a duplicate row is a neighbour at
    distance 0).  Gram form with exact products on the fp64 matrix instruction; the matrix of pairs is never stored;
    identical bits from run to run.  A row with a non-finite feature sets KNN_NONFINITE in the int32 ``status[0]``, has
    the radius NaN and is nobody's neighbour.  ``1 <= k <= KNN_MAX_K``, ``k < n``, ``D <= FEAT_MAX_DIM``.  Current
    stream, no host synchronisation, no autograd."""
    x = _feat_matrix(x, 'knn_radii: x')
    n, D, k = x.shape[0], x.shape[1], int(k)
    if k < 1 or k > KNN_MAX_K or n <= k or D > FEAT_MAX_DIM:
        raise ValueError('knn_radii: k %d (1..%d), x %s (more than k rows, at most %d columns)'
                         % (k, KNN_MAX_K, tuple(x.shape), FEAT_MAX_DIM))
    status = _knn_status(status, x.device, 'knn_radii')
    with torch.cuda.device(x.device):
        radii2 = torch.empty(n, dtype=torch.float64, device=x.device)
        with _scratch('knn_radii', lib.him_knn_radii_ws(n, D, k)) as ws:
            lib.him_knn_radii(_p(x), n, D, k, _p(radii2), _p(status), _p(ws), ws.numel(), _stream())
    return radii2, status


def knn_membership(q, ref, radii2, want_cols=True, status=None):
    """``(row_count, col_count, status)`` of the indicator ``I[j, i] = d2(q_j, ref_i) <= radii2[i]`` between the fp32
    device matrices ``q`` (nq, D) and ``ref`` (nr, D), ``radii2`` (nr,) float64 being the radii of the REFERENCE rows
    (``knn_radii(ref, k)``): ``row_count[j] = sum_i I[j, i]`` (nq,) and ``col_count[i] = sum_j I[j, i]`` (nr,), int32;
    ``col_count`` is None without ``want_cols``.  The arithmetic of ``knn_radii``; the indicator is never stored.  A
    non-finite row sets KNN_NONFINITE in ``status[0]`` and takes part in no true comparison.  Current stream, no host
    synchronisation, no autograd."""
    q, ref = _feat_matrix(q, 'knn_membership: q'), _feat_matrix(ref, 'knn_membership: ref')
    if ref.device != q.device or ref.shape[1] != q.shape[1] or q.shape[0] < 1 or ref.shape[0] < 1 \
            or q.shape[1] > FEAT_MAX_DIM:
        raise ValueError('knn_membership: q %s and ref %s must be non-empty, of one row length (at most %d) and on one '
                         'device' % (tuple(q.shape), tuple(ref.shape), FEAT_MAX_DIM))
    nq, nr, D = q.shape[0], ref.shape[0], q.shape[1]
    if not torch.is_tensor(radii2) or radii2.dtype != torch.float64 or tuple(radii2.shape) != (nr,) \
            or not radii2.is_contiguous() or radii2.device != q.device:
        raise ValueError('knn_membership: radii2 must be a contiguous (%d,) float64 tensor on the device of q' % nr)
    status = _knn_status(status, q.device, 'knn_membership')
    with torch.cuda.device(q.device):
        row_count = torch.empty(nq, dtype=torch.int32, device=q.device)
        col_count = torch.empty(nr, dtype=torch.int32, device=q.device) if want_cols else None
        with _scratch('knn_membership', lib.him_knn_membership_ws(nq, nr, D)) as ws:
            lib.him_knn_membership(_p(q), nq, _p(ref), nr, D, _p(radii2.detach()), _p(row_count), _p(col_count),
                                   _p(status), _p(ws), ws.numel(), _stream())
    return row_count, col_count, status
