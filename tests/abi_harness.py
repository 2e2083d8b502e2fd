"""Direct C-ABI harness of the convolution family (helper module like util.py; not a conftest).

One call = one (descriptor, HimAlgo, pass).  Every buffer of the call lives inside ONE allocation between two guard
bands; after the call the harness checks the return code, the bands, that every output element is finite, and the error
against a float64 CPU reference under the bound of tests/README.md "How op tests bound errors".

The library under check is a PARAMETER (``lib``): any object whose ``him_*`` attributes take the arguments of
include/him.h (pointers as integers) and return the library's return codes.  ``raw_lib()`` is libhim_hip.so without the
raising wrappers of _cabi; tests/test_abi_harness_cpu.py passes CPU stand-ins with planted defects instead, which reach
the arena through ``mem()`` exactly like a kernel would: by address, bands included.
"""
import ctypes
import json
import os

import torch
import torch.nn.functional as F

from neurips18_hierchical_image_manipulation_amd import _cabi
from neurips18_hierchical_image_manipulation_amd._cabi import HimAlgo, HimConv2d, HimDeconv2d

E_INVALID, E_WORKSPACE, E_LAUNCH, E_UNSUPPORTED = -1, -2, -3, -4
PANEL_FWD, PANEL_BWD_DATA = 0, 1

# Guard bands: a multiple of 256 bytes, so that every view keeps the 256-byte alignment a torch allocation has (the
# kernels' 16-byte vector loads and buffer resources assume it); 64 KiB on each side holds a whole stray row of the
# widest tile (256 columns x 64 rows of floats).
GUARD = 64 * 1024
ALIGN = 256
OUT_BYTE = 0xA5          # bands around outputs / workspace: 0xA5A5A5A5 words (finite, -2.9e-16), compared bit for bit
NAN_BYTE = 0xFF          # bands around inputs, fresh outputs, workspace: 0xFFFFFFFF words = NaN
EPS32 = 2.0 ** -24
DIRECT_FACTOR, DIRECT_FLOOR = 8.0, 16 * EPS32      # direct-form bound: max(8 * e32, 16 * 2^-24)
ACTS = {'none': 0, 'relu': 1, 'lrelu': 2, 'tanh': 3}
SLOPE = 0.2


class HarnessFailure(AssertionError):
    pass


def raw_lib():
    """libhim_hip.so with integer return codes (the _cabi wrappers raise instead)."""
    return _cabi.lib._load()


def algo(**fields):
    a = HimAlgo()
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def algo_tag(a):
    return ','.join('%s=%d' % (k, v) for k, v in a.as_dict().items() if v) or 'default'


def mem(ptr, nfloats):
    """HOST memory at ``ptr`` as a float tensor (the CPU stand-ins' way to the arena, bands included)."""
    return torch.frombuffer((ctypes.c_float * nfloats).from_address(ptr), dtype=torch.float32)


class Arena(object):
    """specs: name -> ('in', tensor) | ('out', shape, prefill tensor or None) | ('ws', nbytes).  ``t[name]`` is the view."""

    def __init__(self, device, specs):
        self.device = torch.device(device)
        self.specs = specs
        off, self.span = 0, {}
        for name, s in specs.items():
            nbytes = int(s[1].numel() * 4 if s[0] == 'in' else (torch.Size(s[1]).numel() * 4 if s[0] == 'out' else s[1]))
            off += GUARD
            end = off + nbytes
            self.span[name] = (off, end)
            off = (end + ALIGN - 1) // ALIGN * ALIGN + GUARD     # the band behind begins at the buffer's last byte + 1
        self.raw = torch.empty(off + ALIGN, dtype=torch.uint8, device=self.device)
        self.base = (-self.raw.data_ptr()) % ALIGN
        self.buf = self.raw[self.base:self.base + off]
        self.t, self.bands = {}, []
        prev_end = 0
        names = list(specs)
        for i, name in enumerate(names):
            s = specs[name]
            b0, b1 = self.span[name]
            nxt = self.span[names[i + 1]][0] - GUARD if i + 1 < len(names) else off
            fill = NAN_BYTE if s[0] == 'in' else OUT_BYTE
            for side, lo, hi in (('before', prev_end, b0), ('behind', b1, nxt)):
                self.buf[lo:hi].fill_(fill)
                self.bands.append((name, side, lo, hi, fill))
            prev_end = nxt
            region = self.buf[b0:b1]
            if s[0] == 'ws':
                region.fill_(NAN_BYTE)
                self.t[name] = region
                continue
            view = region.view(torch.float32).view(s[1].shape if s[0] == 'in' else s[1])
            if s[0] == 'in':
                view.copy_(s[1])
            elif s[2] is not None:
                view.copy_(s[2])
            else:
                region.fill_(NAN_BYTE)
            self.t[name] = view

    def ptr(self, name):
        return 0 if name is None or name not in self.t else self.buf.data_ptr() + self.span[name][0]

    def nbytes(self, name):
        return self.span[name][1] - self.span[name][0] if name in self.span else 0

    def guard_failures(self):
        bad = []
        for name, side, lo, hi, fill in self.bands:
            band = self.buf[lo:hi]
            if bool((band == fill).all()):
                continue
            idx = int((band != fill).nonzero()[0])
            edge = (idx - (hi - lo)) if side == 'before' else idx     # bytes relative to the buffer's first / last+1 byte
            w0 = idx // 4 * 4
            word = bytes(band[w0:w0 + 4].cpu().tolist())[::-1].hex()
            bad.append('guard %s %s changed: first byte at %+d from the buffer edge, word 0x%s' % (side, name, edge, word))
        return bad


# ------------------------------------------------------------------------------------------------ metrics and bounds
def ring_mask(shape):
    m = torch.zeros(shape[-2:], dtype=torch.bool)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    return m


def rel_err(got, ref64, mask=None):
    """max|got - ref| over max|ref| (util.report's metric), optionally on the masked elements only, both sides."""
    g, r = got.detach().double().cpu(), ref64.detach().double().cpu()
    if mask is not None:
        g, r = g[..., mask], r[..., mask]
    scale = max(float(r.abs().max()) if r.numel() else 0.0, 1e-30)
    err = (g - r).abs()
    if not bool(torch.isfinite(err).all()):
        return float('inf'), _worst(torch.where(torch.isfinite(err), torch.zeros_like(err), torch.ones_like(err)))
    return (float(err.max()) / scale if err.numel() else 0.0), _worst(err)


def _worst(err):
    if not err.numel():
        return ()
    i, out = int(err.argmax()), []
    for n in reversed(err.shape):
        out.append(i % n)
        i //= n
    return tuple(reversed(out))


def metrics(kind, got, ref64):
    """kind 'plane': (whole tensor, border ring); 'weight': (whole tensor,); 'bias': (per channel,) -- each (error, index)."""
    if kind == 'plane':
        return {'all': rel_err(got, ref64), 'ring': rel_err(got, ref64, ring_mask(ref64.shape))}
    return {'all': rel_err(got, ref64)}


class Bound(object):
    """direct: max(8 * e32, 16 * 2^-24) with e32 = the fp32 CPU result's own error under the same metric.
    fixed(tol): the tolerance the suite already asserts for a Winograd family, applied to float64 and to the ring."""

    def __init__(self, tol=None):
        self.tol = tol

    def limit(self, e32):
        return self.tol if self.tol is not None else max(DIRECT_FACTOR * e32, DIRECT_FLOOR)


DIRECT = Bound()
REPORT = []          # one dict per checked tensor; test modules dump it (dump_report)


def check_tensor(row, what, kind, got, ref64, ref32, bound):
    if not bool(torch.isfinite(got).all()):
        n = int((~torch.isfinite(got)).sum())
        idx = _worst((~torch.isfinite(got)).double().cpu())
        raise HarnessFailure('%s %s: %d output elements are not finite (never written, or computed from a guard value); '
                             'first kind of offender at %s' % (row, what, n, idx))
    m, m32 = metrics(kind, got, ref64), metrics(kind, ref32, ref64)
    for key in m:
        err, idx = m[key]
        e32 = m32[key][0]
        lim = bound.limit(e32)
        REPORT.append({'row': row, 'tensor': what, 'metric': key, 'err': err, 'e32': e32,
                       'ratio': err / e32 if e32 > 0 else None, 'limit': lim})
        if not err <= lim:
            raise HarnessFailure('%s %s [%s]: error %.3e of max|ref64| > bound %.3e (e32 %.3e, ratio %.1f) worst@%s got=%.9e '
                                 'ref=%.9e' % (row, what, key, err, lim, e32, err / max(e32, 1e-30), idx,
                                               float(got.detach().cpu()[idx] if key == 'all' else float('nan')),
                                               float(ref64[idx]) if key == 'all' else float('nan')))


def dump_report(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'a') as f:
        for r in REPORT:
            f.write(json.dumps(r) + '\n')
    del REPORT[:]


# ------------------------------------------------------------------------- guarded calls and per-tensor rows (shared)
def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def max_rel_err(got, ref):
    """tests/README.md's metric as one number: maximum error over maximum |ref|; inf when an element is not finite."""
    g, r = torch.as_tensor(got).detach().double().cpu().reshape(-1), torch.as_tensor(ref).detach().double().cpu().reshape(-1)
    if r.numel() == 0:
        return 0.0
    err = (g - r).abs()
    if not bool(torch.isfinite(err).all()):
        return float('inf')
    return float(err.max()) / max(float(r.abs().max()), 1e-30)


def call(lib, dev, fn, specs, args, expect=0):
    """One guarded call: ``args(P)`` builds the argument list from the arena's address function.  Checks the return
    code, every band and that no input changed; returns the arena."""
    ar = Arena(dev, specs)
    rc = getattr(lib, fn)(*args(ar.ptr))
    _sync(dev)
    assert rc == expect, '%s returned %d, expected %d (%s)' % (fn, rc, expect, lib.him_last_error())
    bad = ar.guard_failures()
    assert not bad, '%s: %s' % (fn, '; '.join(bad))
    for name, s in specs.items():
        if s[0] == 'in':
            assert torch.equal(bits(ar.t[name]), bits(s[1])), '%s wrote its input %s' % (fn, name)
    return ar


def untouched(ar, specs):
    """After a refused call: fresh outputs and the workspace still hold the NaN bytes, prefilled outputs their prefill."""
    for name, s in specs.items():
        if s[0] == 'ws' or (s[0] == 'out' and s[2] is None):
            assert bool((ar.t[name].view(torch.uint8) == NAN_BYTE).all()), name
        elif s[0] == 'out':
            assert torch.equal(bits(ar.t[name]), bits(s[2])), name


class RowLog(object):
    """The rows of one test module; ``flush()`` appends them to ``path`` as JSON lines."""

    def __init__(self, path):
        self.path, self.rows = path, []

    def flush(self):
        if self.rows:
            os.makedirs(os.path.dirname(self.path), exist_ok=True)
            with open(self.path, 'a') as f:
                for r in self.rows:
                    f.write(json.dumps(r) + '\n')
            del self.rows[:]


class Checks(object):
    """Collects the rows of one case in ``log``; ``done()`` flushes, then asserts, after every row has been reported.
    ``ref32`` of ``row`` may be a list of float32 results (several correct summation orders): e32 is their maximum."""

    def __init__(self, case, log, flush=None, metric=max_rel_err, limit=DIRECT.limit):
        self.case, self.failed, self.log = case, [], log
        self.flush, self.metric, self.limit = flush or log.flush, metric, limit

    def row(self, name, got, ref64, ref32, metric=None, lim=None):
        metric = metric or self.metric
        got = got.detach().cpu()
        err = metric(got, ref64)
        e32 = max(metric(r, ref64) for r in (ref32 if isinstance(ref32, (list, tuple)) else [ref32]))
        lim = self.limit(e32) if lim is None else lim
        self.log.rows.append(dict(case=self.case, tensor=name, error=err, e32=e32, ratio=(err / e32 if e32 > 0 else None),
                                  limit=lim))
        print('%s %s: error %.3e e32 %.3e limit %.3e' % (self.case, name, err, e32, lim))
        if not err <= lim:
            self.failed.append('%s %s: error %.3e > limit %.3e (e32 %.3e)' % (self.case, name, err, lim, e32))
        return lim

    def exact(self, name, got, want):
        ok = torch.equal(got.detach().cpu(), want)
        self.log.rows.append(dict(case=self.case, tensor=name, error=0.0 if ok else 1.0, e32=0.0, ratio=None, limit=0.0))
        if not ok:
            self.failed.append('%s %s: not bit-identical to the float32 restatement' % (self.case, name))

    def done(self):
        self.flush()
        assert not self.failed, '; '.join(self.failed)


# ------------------------------------------------------------------------------------------------------- references
def rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def act_fn(y, act):
    return {'none': lambda t: t, 'relu': F.relu, 'lrelu': lambda t: F.leaky_relu(t, SLOPE), 'tanh': torch.tanh}[act](y)


class ConvCase(object):
    """(B, Cin, H, W, Cout, k, stride, pad, pad_mode, act): the CONV_CASES tuple of test_ops_gpu.py."""
    deconv = False

    def __init__(self, case, bias=True):
        self.case = tuple(case)
        self.B, self.Cin, self.H, self.W, self.Cout, self.k, self.s, self.p, self.pm, self.act = case
        self.OH = (self.H + 2 * self.p - self.k) // self.s + 1
        self.OW = (self.W + 2 * self.p - self.k) // self.s + 1
        self.x = rand(self.B, self.Cin, self.H, self.W, seed=1)
        self.w = rand(self.Cout, self.Cin, self.k, self.k, seed=2, scale=(self.Cin * self.k * self.k) ** -0.5)
        self.b = rand(self.Cout, seed=3, scale=0.1) if bias else None
        self.dy = rand(self.B, self.Cout, self.OH, self.OW, seed=4)
        self._ref = {}

    def tag(self):
        return 'x'.join(map(str, self.case))

    def desc(self, a, **over):
        d = HimConv2d(self.B, self.Cin, self.H, self.W, self.Cout, self.k, self.k, self.s, self.p,
                      1 if self.pm == 'reflect' else 0, self.OH, self.OW, ACTS[self.act], SLOPE, a)
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def pre(self, x, w, b):
        p = self.p
        if self.pm == 'reflect':
            x, p = F.pad(x, (p, p, p, p), mode='reflect'), 0
        return F.conv2d(x, w, b, self.s, p)

    def ref(self, dtype, what):
        """'y' (activated) / 'z' (pre-activation) / 'dx' / 'dw' / 'db' of the pre-activation output against dy, computed in
        ``dtype`` on the CPU; each on first use (the full-size shapes only pay for the passes their rows run)."""
        r = self._ref.setdefault(dtype, {})
        if what not in r:
            x, w = self.x.to(dtype), self.w.to(dtype)
            b = self.b.to(dtype) if self.b is not None else None
            dy = self.dy.to(dtype)
            if what in ('y', 'z'):
                with torch.no_grad():
                    r['z'] = self.pre(x, w, b)
                    r['y'] = act_fn(r['z'], self.act)
            elif what == 'dx':
                x.requires_grad_(True)
                (r['dx'],) = torch.autograd.grad(self.pre(x, w, None), x, dy)
            elif what == 'dw':
                w.requires_grad_(True)
                (r['dw'],) = torch.autograd.grad(self.pre(x, w, None), w, dy)
            elif what == 'db':
                r['db'] = dy.sum((0, 2, 3))
        return r[what]

    def ref_nobias(self, dtype):
        with torch.no_grad():
            return act_fn(self.pre(self.x.to(dtype), self.w.to(dtype), None), self.act)


class DeconvCase(ConvCase):
    """(B, Cin, H, W, Cout[, act]): ConvTranspose2d(k3, s2, p1, op1), the DECONV_CASES tuple of test_ops_gpu.py."""
    deconv = True

    def __init__(self, case, act='none', bias=True):
        self.case = tuple(case) + (act,)
        self.B, self.Cin, self.H, self.W, self.Cout = case
        self.k, self.s, self.p, self.op, self.pm, self.act = 3, 2, 1, 1, 'zero', act
        self.OH = (self.H - 1) * 2 - 2 + 3 + 1
        self.OW = (self.W - 1) * 2 - 2 + 3 + 1
        self.x = rand(self.B, self.Cin, self.H, self.W, seed=1)
        self.w = rand(self.Cin, self.Cout, 3, 3, seed=2, scale=(self.Cin * 9) ** -0.5)
        self.b = rand(self.Cout, seed=3, scale=0.1) if bias else None
        self.dy = rand(self.B, self.Cout, self.OH, self.OW, seed=4)
        self._ref = {}

    def tag(self):
        return 'deconv' + 'x'.join(map(str, self.case))

    def desc(self, a, **over):
        d = HimDeconv2d(self.B, self.Cin, self.H, self.W, self.Cout, 3, 3, 2, 1, 1, self.OH, self.OW, ACTS[self.act], SLOPE, a)
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def pre(self, x, w, b):
        return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)


# ------------------------------------------------------------------------------------------------------------ passes
def _stream(device):
    return torch.cuda.current_stream().cuda_stream if torch.device(device).type == 'cuda' else 0


def _sync(device):
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()


def _finish(lib, row, rc, arena, device):
    _sync(device)
    if rc != 0:
        why = lib.him_last_error()
        raise HarnessFailure('%s: return code %d (%s)' % (row, rc, why.decode() if isinstance(why, bytes) else why))
    bad = arena.guard_failures()
    if bad:
        raise HarnessFailure('%s: %s' % (row, '; '.join(bad)))


def run_pass(lib, case, a, what, device='cuda', bound=DIRECT, accumulate=0, bias=True, dbias=True, panel=False,
             check=True):
    """One launch of pass ``what`` in ('fwd', 'bwd_data', 'bwd_weight', 'bwd_data_gated', 'fwd_keep_wgrad', 'in_act')
    through guarded arenas; returns the outputs (CPU tensors) by name.  ``panel``: the *_panel form (panel_build with the
    same HimAlgo first).  ``check=False`` skips the error bounds (guards, return code and finiteness still hold)."""
    pre = 'him_deconv2d_' if case.deconv else 'him_conv2d_'
    d = case.desc(a)
    dref = ctypes.byref(d)
    row = '%s|%s|%s%s%s' % (case.tag(), algo_tag(a), what, '+panel' if panel else '', '+acc' if accumulate else '')
    st = _stream(device)
    f64, f32 = torch.float64, torch.float32
    if what == 'fwd_keep_wgrad':
        panel = True
    use_bias = bias and case.b is not None
    specs, outs = {}, {}
    kind = PANEL_FWD if what in ('fwd', 'fwd_keep_wgrad', 'in_act') else PANEL_BWD_DATA
    npanel = int(getattr(lib, pre + 'panel_bytes')(dref, kind)) if panel else 0
    if panel and npanel == 0:
        return None                                    # the kernel reads raw weights: the plain entry point is the only form
    if what in ('fwd', 'in_act', 'fwd_keep_wgrad'):
        ws_fn = pre + 'fwd_ws'
    elif what in ('bwd_data', 'bwd_data_gated'):
        ws_fn = pre + 'bwd_data_ws'
    else:
        ws_fn = pre + 'bwd_weight_ws'
    nws = int(getattr(lib, ws_fn)(dref))
    xin = F.relu(case.x) if what == 'bwd_data_gated' else case.x     # the gate's tensor is a ReLU output (VGG chain)
    if what in ('fwd', 'in_act', 'fwd_keep_wgrad'):
        specs['x'] = ('in', case.x)
        specs['w'] = ('in', case.w)
        if use_bias:
            specs['bias'] = ('in', case.b)
        specs['y'] = ('out', (case.B, case.Cout, case.OH, case.OW), None)
    elif what in ('bwd_data', 'bwd_data_gated'):
        specs['dy'] = ('in', case.dy)
        specs['w'] = ('in', case.w)
        if what == 'bwd_data_gated':
            specs['x'] = ('in', xin)
        specs['dx'] = ('out', tuple(case.x.shape), None)
    else:
        specs['x'] = ('in', case.x)
        specs['dy'] = ('in', case.dy)
        specs['dw'] = ('out', tuple(case.w.shape), rand(*case.w.shape, seed=7) if accumulate else None)
        if dbias:
            specs['dbias'] = ('out', (case.Cout,), rand(case.Cout, seed=8) if accumulate else None)
    if what == 'in_act':
        specs['z'] = ('out', (case.B, case.Cout, case.OH, case.OW), None)
        specs['mean'] = ('out', (case.B * case.Cout,), None)
        specs['rstd'] = ('out', (case.B * case.Cout,), None)
    nkeep = 0
    if what == 'fwd_keep_wgrad':
        nkeep = int(lib.him_conv2d_fwd_keep_bytes(dref))
        if nkeep == 0:
            return None
        specs['keep'] = ('ws', nkeep)
        specs['dw'] = ('out', tuple(case.w.shape), rand(*case.w.shape, seed=7) if accumulate else None)
        specs['dbias'] = ('out', (case.Cout,), rand(case.Cout, seed=8) if accumulate else None)
        specs['dy'] = ('in', case.dy)
        nws2 = int(lib.him_conv2d_bwd_weight_ws(dref))
        specs['ws2'] = ('ws', nws2)
    if npanel:
        specs['panel'] = ('ws', npanel)
    specs['ws'] = ('ws', nws)
    ar = Arena(device, specs)
    P = ar.ptr
    if npanel:
        rc = getattr(lib, pre + 'panel_build')(dref, kind, P('w'), P('panel'), npanel, st)
        _finish(lib, row + ' panel_build', rc, ar, device)
        ar.t['w'].fill_(float('nan'))                  # the *_panel launch must not read the raw weights any more
    if what == 'fwd':
        if panel:
            rc = getattr(lib, pre + 'fwd_panel')(dref, P('x'), P('panel'), P('bias'), P('y'), P('ws'), nws, st)
        else:
            rc = getattr(lib, pre + 'fwd')(dref, P('x'), P('w'), P('bias'), P('y'), P('ws'), nws, st)
    elif what == 'in_act':
        rc = lib.him_conv2d_in_act_fwd(dref, P('x'), 0 if panel else P('w'), P('panel') if panel else 0, P('bias'), P('y'), 0,
                                       P('z'), P('mean'), P('rstd'), 1e-5, ACTS['relu'], SLOPE, P('ws'), nws, st)
    elif what == 'fwd_keep_wgrad':
        rc = lib.him_conv2d_fwd_panel_keep(dref, P('x'), P('panel'), P('bias'), P('y'), P('keep'), P('ws'), nws, st)
        _finish(lib, row + ' fwd_panel_keep', rc, ar, device)
        ar.t['x'].fill_(float('nan'))                  # bwd_weight_kept reads `keep` in place of x
        rc = lib.him_conv2d_bwd_weight_kept(dref, P('keep'), P('dy'), P('dw'), P('dbias'), accumulate, P('ws2'),
                                            ar.nbytes('ws2'), st)
    elif what == 'bwd_data':
        if panel:
            rc = getattr(lib, pre + 'bwd_data_panel')(dref, P('dy'), P('panel'), P('dx'), P('ws'), nws, st)
        else:
            rc = getattr(lib, pre + 'bwd_data')(dref, P('dy'), P('w'), P('dx'), P('ws'), nws, st)
    elif what == 'bwd_data_gated':
        rc = lib.him_conv2d_bwd_data_gated(dref, P('dy'), 0 if panel else P('w'), P('panel') if panel else 0, P('x'), P('dx'),
                                           P('ws'), nws, st)
    elif what == 'bwd_weight':
        rc = getattr(lib, pre + 'bwd_weight')(dref, P('x'), P('dy'), P('dw'), P('dbias') if dbias else 0, accumulate, P('ws'),
                                              nws, st)
    else:
        raise ValueError(what)
    _finish(lib, row, rc, ar, device)
    if 'y' in specs:
        outs['y'] = ar.t['y'].cpu()
        if check:
            ref = (lambda dt: case.ref(dt, 'y')) if use_bias or case.b is None else case.ref_nobias
            check_tensor(row, 'y', 'plane', outs['y'], ref(f64), ref(f32), bound)
    if what == 'in_act':
        outs['z'] = ar.t['z'].cpu()
        if check:
            zr = {k: F.relu(F.instance_norm(case.ref(dt, 'y'), eps=1e-5)) for k, dt in (('64', f64), ('32', f32))}
            # InstanceNorm divides by the plane's deviation: its error bound is the norm kernels' own (test_instance_norm, 2e-5)
            check_tensor(row, 'z', 'plane', outs['z'], zr['64'], zr['32'], Bound(2e-5))
    if 'dx' in specs:
        outs['dx'] = ar.t['dx'].cpu()
        if check:
            gate = (xin > 0) if what == 'bwd_data_gated' else 1
            check_tensor(row, 'dx', 'plane', outs['dx'], case.ref(f64, 'dx') * gate, case.ref(f32, 'dx') * gate, bound)
    if 'dw' in specs:
        outs['dw'] = ar.t['dw'].cpu()
        base_w = specs['dw'][2]
        if check:
            check_tensor(row, 'dw', 'weight', outs['dw'], case.ref(f64, 'dw') + (0 if base_w is None else base_w.double()),
                         case.ref(f32, 'dw') + (0 if base_w is None else base_w), bound)
        if 'dbias' in specs:
            outs['dbias'] = ar.t['dbias'].cpu()
            base_b = specs['dbias'][2]
            if check:
                check_tensor(row, 'dbias', 'bias', outs['dbias'], case.ref(f64, 'db') + (0 if base_b is None else base_b.double()),
                             case.ref(f32, 'db') + (0 if base_b is None else base_b), bound)
    return outs


def negative_paths(lib, case, a, device='cuda'):
    """No launch: a workspace one byte short -> HIM_E_WORKSPACE, OH / OW off the formula -> HIM_E_INVALID; guards and the
    NaN-filled output stay as they were."""
    d = case.desc(a)
    nws = int(lib.him_conv2d_fwd_ws(ctypes.byref(d)))
    specs = {'x': ('in', case.x), 'w': ('in', case.w), 'y': ('out', (case.B, case.Cout, case.OH, case.OW), None),
             'ws': ('ws', max(nws, 1))}
    ar = Arena(device, specs)
    st = _stream(device)
    results = {}
    if nws > 0:
        results['short'] = lib.him_conv2d_fwd(ctypes.byref(d), ar.ptr('x'), ar.ptr('w'), 0, ar.ptr('y'), ar.ptr('ws'), nws - 1, st)
    bad = case.desc(a, OH=case.OH + 1)
    results['oh'] = lib.him_conv2d_fwd(ctypes.byref(bad), ar.ptr('x'), ar.ptr('w'), 0, ar.ptr('y'), ar.ptr('ws'), nws, st)
    bad = case.desc(a, OW=case.OW - 1)
    results['ow'] = lib.him_conv2d_fwd(ctypes.byref(bad), ar.ptr('x'), ar.ptr('w'), 0, ar.ptr('y'), ar.ptr('ws'), nws, st)
    _sync(device)
    if 'short' in results and results['short'] != E_WORKSPACE:
        raise HarnessFailure('%s: workspace one byte short returned %d, not HIM_E_WORKSPACE' % (case.tag(), results['short']))
    for k in ('oh', 'ow'):
        if results[k] != E_INVALID:
            raise HarnessFailure('%s: descriptor with a wrong %s returned %d, not HIM_E_INVALID' % (case.tag(), k.upper(), results[k]))
    bad = ar.guard_failures()
    if bad or not bool(torch.isnan(ar.t['y']).all()):
        raise HarnessFailure('%s: a refused call wrote memory: %s' % (case.tag(), bad or 'output touched'))


def run_wino_gemm(lib, M, K, N, a, device='cuda', expect_error=False):
    """him_winograd_gemm on its own against a float64 bmm; ``expect_error``: a shape outside K % 16 / N % 128 must be
    refused and write nothing."""
    A, Bm = rand(16, M, K, seed=1, scale=K ** -0.5), rand(16, K, N, seed=2)
    ar = Arena(device, {'a': ('in', A), 'b': ('in', Bm), 'c': ('out', (16, M, N), None)})
    rc = lib.him_winograd_gemm(ar.ptr('a'), ar.ptr('b'), ar.ptr('c'), M, K, N, ctypes.byref(a), _stream(device))
    row = 'wino_gemm %dx%dx%d|%s' % (M, K, N, algo_tag(a))
    if expect_error:
        _sync(device)
        bad = ar.guard_failures()
        if rc == 0 or bad or not bool(torch.isnan(ar.t['c']).all()):
            raise HarnessFailure('%s: outside the contract, yet rc %d, guards %s, output %s' % (
                row, rc, bad or 'intact', 'untouched' if bool(torch.isnan(ar.t['c']).all()) else 'written'))
        return None
    _finish(lib, row, rc, ar, device)
    c = ar.t['c'].cpu()
    check_tensor(row, 'c', 'weight', c, torch.bmm(A.double(), Bm.double()), torch.bmm(A, Bm), DIRECT)
    return c
