"""Flat parameter/gradient arenas and the fused Adam that walks them.

MI355X-first layout: all parameters of one network live in ONE contiguous fp32 buffer (and so do their
gradients, and Adam's two moments).  Consequences:
  * ``optimizer.step()`` is a single HBM-bound kernel over the arena (16 B/param read, 12 B/param written);
  * ``zero_grad()`` is one fill;
  * the data-parallel all-reduce operates on contiguous slices of the gradient arena -- bucket boundaries
    are just offsets, nothing is ever copied in or out of a bucket (see ``dist.py``).
Parameters stay ordinary ``nn.Parameter`` objects (views into the arena), so ``state_dict()`` keys and
tensors are exactly the reference's (``models/base_model.py:46-51`` checkpoint format).
"""
import bisect

import torch

from ._cabi import lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def ema_decay_at(decay, t):
    """Decay of EMA update ``t`` (0-based count of the updates made so far): ``min(decay, (1 + t) / (10 + t))`` in double.
    The ramp lets the first updates forget the initial weights (0.1, 0.18, ... reaches 0.999 at t = 8991)."""
    return min(float(decay), (1.0 + t) / (10.0 + t))


def ema_warm_count(decay):
    """The smallest update count from which ``ema_decay_at`` returns ``decay`` itself."""
    t = 0
    while (1.0 + t) / (10.0 + t) < float(decay):
        t = t * 2 + 1
    lo, hi = t // 2, t
    while lo < hi:
        mid = (lo + hi) // 2
        if (1.0 + mid) / (10.0 + mid) < float(decay):
            lo = mid + 1
        else:
            hi = mid
    return lo


GUARD_CHUNK = 16384      # floats per chunk of him_grad_stats (GS_CHUNK in csrc/him_optim.hip)


def guard_tables(offsets, sizes, total, chunk=GUARD_CHUNK):
    """The segment table handed to ``him_grad_stats`` and the chunk list its summation order is defined by.

    ``seg``: one ``(begin, length)`` per parameter.  ``work``: ``(range, start, length)`` per chunk, in the order the
    kernel numbers them: the arena is cut into the ranges gap 0, parameter 0, gap 1, ..., parameter N-1, tail gap (range
    ``2 i + 1`` is parameter ``i``; gaps are the 256-byte padding and may be empty) and every range into chunks of
    ``chunk`` floats counted from the range's own start.  The library derives the same list on the device from ``seg``
    (the table lives in device memory); here it sizes the workspace check and documents the order."""
    seg, work, at = [], [], 0

    def cut(r, b, e):
        for s in range(b, e, chunk):
            work.append((r, s, min(chunk, e - s)))

    for i, (o, n) in enumerate(zip(offsets, sizes)):
        o, n = int(o), int(n)
        if o < at or n < 0 or o + n > total:
            raise ValueError('parameter %d: [%d, %d) is not a sorted, disjoint sub-range of [0, %d)' % (i, o, o + n, total))
        seg.append((o, n))
        cut(2 * i, at, o)
        cut(2 * i + 1, o, o + n)
        at = o + n
    cut(2 * len(seg), at, int(total))
    return seg, work


class GradGuard(object):
    """Device state of ``FusedAdam.attach_guard``: everything ``him_grad_stats`` writes and the guarded Adam kernel reads."""

    def __init__(self, arena, max_norm, skip_nonfinite):
        dev = arena.data.device
        self.max_norm, self.skip_nonfinite = max_norm, skip_nonfinite
        seg, work = guard_tables(arena.offsets, [p.numel() for p in arena.params], arena.total)
        self.nseg, self.chunks = len(seg), len(work)
        self.seg = torch.tensor(seg, dtype=torch.int64).reshape(-1, 2).to(dev)
        self.seg_out = torch.zeros(self.nseg, 2, dtype=torch.float64, device=dev)
        self.st = torch.zeros(8, dtype=torch.float64, device=dev)           # cumulative slots 4, 5: zeroed once, here
        # clipping without the skip: the Adam kernel reads its flag (slot 1) from a second st whose slot 1 stays zero and
        # whose slot 3 receives the coefficient by a one-element device copy after every stats pass
        self.st_adam = self.st if skip_nonfinite else torch.zeros(8, dtype=torch.float64, device=dev)
        self.ws_bytes = int(lib.him_grad_stats_ws(arena.total, self.nseg))
        if self.ws_bytes < 32 * self.chunks:      # work-list entry + partial, 16 B each
            raise RuntimeError('him_grad_stats_ws(%d, %d) = %d bytes cannot hold %d chunks'
                               % (arena.total, self.nseg, self.ws_bytes, self.chunks))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)


class FlatArena(object):
    def __init__(self, params):
        self.params = [p for p in params]
        dev = self.params[0].device
        sizes = [p.numel() for p in self.params]
        # 64-float (256 B) alignment per tensor keeps every view 16 B aligned for float4 streams
        self.offsets, off = [], 0
        for n in sizes:
            self.offsets.append(off)
            off += (n + 63) // 64 * 64
        self.total = off
        self.data = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(off, dtype=torch.float32, device=dev)
        for p, o in zip(self.params, self.offsets):
            n = p.numel()
            self.data[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.data[o:o + n].view(p.shape)
            p.grad = self.grad[o:o + n].view(p.shape)
            p._him_direct_grad = True
            p._him_arena_range = (o, o + n)

    def rebind(self):
        """Re-attach .grad views (something set them to None) -- keeps the direct-wgrad contract."""
        for p, o in zip(self.params, self.offsets):
            n = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                p.grad = self.grad[o:o + n].view(p.shape)

    def zero_grad(self):
        self.rebind()
        from .ops import join_side_stream
        join_side_stream(self.grad.device)     # no weight-gradient kernel may still be writing
        lib.him_fill(self.grad.data_ptr(), self.total, 0.0, _stream())


class FusedAdam(object):
    """torch.optim.Adam look-alike (``zero_grad/step/param_groups/state_dict``) over a FlatArena.
    Numerics follow torch's single-tensor Adam: lerp first moment, sqrt(v)/sqrt(bc2)+eps, lr/bc1."""

    def __init__(self, params, lr=2e-4, betas=(0.5, 0.999), eps=1e-8, arena=None):
        """``params``: an iterable of Parameters, or torch-style groups ``[{'params': [...], 'lr': ...}, ...]`` (the
        reference freezes the global generator that way, ``models/pix2pixHD_condImg_model.py:122-130``: one group per
        parameter with lr 0 outside the local enhancer).  All groups share ONE arena in the order given; ``step`` runs
        one kernel per maximal contiguous run of parameters with equal hyper-parameters (one launch in the common case)."""
        params = list(params)
        if params and isinstance(params[0], dict):
            groups = [dict(g, params=list(g['params'])) for g in params]
        else:
            groups = [dict(params=params)]
        flat = [p for g in groups for p in g['params']]
        self.arena = arena if arena is not None else FlatArena(flat)
        if [id(p) for p in self.arena.params] != [id(p) for p in flat]:
            raise ValueError('the arena holds a different parameter list than the optimizer was given')
        self.param_groups = []
        for g in groups:
            self.param_groups.append(dict(params=g['params'], lr=g.get('lr', lr), betas=tuple(g.get('betas', betas)),
                                          eps=g.get('eps', eps)))
        self.exp_avg = torch.zeros_like(self.arena.data)
        self.exp_avg_sq = torch.zeros_like(self.arena.data)
        self.step_count = 0
        # weight EMA (attach_ema): off = no buffer, and _adam calls him_adam_step exactly as without the feature
        self.ema = None
        self.ema_decay = 0.0
        self.ema_updates = 0          # EMA updates made so far (the ``t`` of ema_decay_at)
        self._ema_now = 0.0           # the decay of the step in flight: ONE value for all ranges of a step
        self._ema_swapped = False     # inside swap_ema() ... swap_ema(): the arena holds the averaged values
        # gradient guard (attach_guard): off = nothing allocated, and _adam makes exactly the calls above
        self.guard = None

    # ---- gradient guard: global norm, clipping and the non-finite skip, decided on the device -----------------------
    def attach_guard(self, max_norm=0.0, skip_nonfinite=True):
        """From now on every ``step()`` first runs ``him_grad_stats`` over the whole gradient arena and then the guarded
        Adam kernel, which reads the outcome from device memory -- nothing synchronises with the host.

        ``max_norm`` > 0: global-norm clipping by the rule of ``torch.nn.utils.clip_grad_norm_``, applied to the gradient
        as Adam reads it; the ``.grad`` buffers are NOT rewritten (unlike torch).  0 or inf: no clipping.
        ``skip_nonfinite``: a step whose gradient holds an Inf or NaN stores nothing -- parameters, both moments and the
        weight EMA keep their bits.  False: the statistics are still taken, but the kernel is handed a second ``st``
        buffer whose non-finite slot stays zero (only the clip coefficient is copied into it, on the device).

        DEVIATION from ``torch.cuda.amp.GradScaler``: the host cannot know the outcome without a synchronisation, so a
        skipped step KEEPS its step number -- ``step_count`` and ``ema_updates`` count attempts, and the next step's bias
        corrections are those of one step later; ``grad_report()['skipped']`` (slot 5 of ``st``) counts the skips.

        Piecewise steps: the global norm needs every gradient, so with a guard ``step_range`` only records its range
        and ``step()`` updates the whole arena -- bit-identical to a plain guarded ``step()``.

        Data parallel: ``step()`` runs after the reducer has finished, on gradients every rank holds identically, and
        the statistics are a deterministic function of them: the ranks decide alike without another collective."""
        max_norm = float(max_norm)
        if not max_norm >= 0.0:
            raise ValueError('max_norm %r: a value >= 0 (0 = no clipping)' % max_norm)
        if getattr(self, '_done', None) is not None:
            raise RuntimeError('attach_guard inside an open piecewise step')
        self.guard = GradGuard(self.arena, max_norm, bool(skip_nonfinite))
        return self

    def adopt_guard(self, other):
        """Take over ``other``'s guard, counters included (an optimizer rebuilt over the same arena)."""
        if other.guard is not None:
            if other.arena is not self.arena:
                raise ValueError('adopt_guard: the two optimizers walk different arenas')
            self.guard = other.guard
        return self

    def _guard_stats(self):
        a, gd = self.arena, self.guard
        lib.him_grad_stats(a.grad.data_ptr(), a.total, gd.seg.data_ptr(), gd.nseg, gd.seg_out.data_ptr(), gd.st.data_ptr(),
                           gd.max_norm, gd.ws.data_ptr(), gd.ws_bytes, _stream())
        if gd.st_adam is not gd.st:
            gd.st_adam[3:4].copy_(gd.st[3:4])

    def grad_stats(self):
        """``(st, norms)`` on the DEVICE, as the last ``step()`` left them: the 8 doubles of ``him_grad_stats`` and the
        gradient norm of every parameter (arena order).  Reading them on the host synchronises; ``grad_report`` does."""
        if self.guard is None:
            raise RuntimeError('no gradient guard attached (attach_guard)')
        return self.guard.st, self.guard.seg_out[:, 0].sqrt()

    def grad_report(self, network=None):
        """Host dict of the last step's statistics -- THE synchronising call, for print time only.  With ``network``:
        ``per_param`` (norm by parameter name) and ``worst``, the name with the most non-finite elements, else the
        largest norm."""
        st, norms = self.grad_stats()
        st = st.cpu().tolist()
        out = dict(norm=st[2], clip_coef=st[3], nonfinite=int(st[1]), steps=int(st[4]), skipped=int(st[5]))
        if network is not None:
            by_id = {id(p): i for i, p in enumerate(self.arena.params)}
            norms, bad = norms.cpu().tolist(), self.guard.seg_out[:, 1].cpu().tolist()
            names = [(k, by_id[id(p)]) for k, p in network.named_parameters() if id(p) in by_id]
            out['per_param'] = {k: norms[i] for k, i in names}
            if names:
                out['worst'] = max(names, key=lambda ki: (bad[ki[1]], norms[ki[1]]))[0]
        return out

    # ---- exponential moving average of the arena, computed by the Adam kernel itself (him_adam_ema_step) ----
    def attach_ema(self, decay, ema=None, updates=0):
        """From now on every Adam run also averages the elements it updates: ``self.ema`` (one more arena-sized buffer,
        4 B per parameter) starts as a copy of the parameters, or as ``ema`` with ``updates`` updates behind it (a buffer
        handed over from another optimizer over the same arena, or read from a checkpoint)."""
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError('ema decay %r: a value in (0, 1)' % decay)
        if getattr(self, '_done', None) is not None:
            raise RuntimeError('attach_ema inside an open piecewise step')
        if ema is None:
            ema = self.arena.data.clone()
        elif ema.shape != self.arena.data.shape or ema.dtype != torch.float32 or ema.device != self.arena.data.device:
            raise ValueError('the EMA buffer does not match the arena')
        self.ema, self.ema_decay, self.ema_updates = ema, decay, int(updates)
        return self

    def reset_ema(self):
        """Restart the average from the parameters as they are now (they were loaded after the optimizer was built)."""
        if self.ema is not None:
            self.ema.copy_(self.arena.data)
            self.ema_updates = 0

    def adopt_ema(self, other):
        """Take over ``other``'s EMA buffer and update count (an optimizer rebuilt over the same arena)."""
        if other.ema is not None:
            if other.arena is not self.arena:
                raise ValueError('adopt_ema: the two optimizers walk different arenas')
            self.attach_ema(other.ema_decay, other.ema, other.ema_updates)
        return self

    def _ema_open(self):
        if self.ema is not None:
            self._ema_now = ema_decay_at(self.ema_decay, self.ema_updates)
            self.ema_updates += 1

    def _check_live(self):
        if self._ema_swapped:
            raise RuntimeError('the arena holds the averaged weights (inside ema_weights()): no optimizer step here')

    def swap_ema(self):
        """Exchange the parameters and their averages in place (one kernel over the arena, current stream).  The caller
        owns the stream order and the weight panels (see the models' ``ema_weights``); while swapped, stepping raises."""
        if self.ema is None:
            raise RuntimeError('no EMA attached (ema_decay 0)')
        if getattr(self, '_done', None) is not None:
            raise RuntimeError('swap_ema inside an open piecewise step')
        lib.him_swap(self.arena.data.data_ptr(), self.ema.data_ptr(), self.arena.total, _stream())
        self._ema_swapped = not self._ema_swapped

    def ema_state_dict(self, network):
        """``network.state_dict()`` on the host with every arena parameter replaced by its average (buffers: live)."""
        by_id = {id(p): o for p, o in zip(self.arena.params, self.arena.offsets)}
        names = {k: by_id[id(p)] for k, p in network.named_parameters() if id(p) in by_id}
        src = self.arena.data if self._ema_swapped else self.ema
        out = {}
        for k, v in network.state_dict().items():
            if k in names:
                out[k] = src[names[k]:names[k] + v.numel()].view(v.shape).detach().cpu().clone()
            else:
                out[k] = v.detach().cpu().clone()
        return out

    def load_ema_state_dict(self, network, sd):
        """Fill the EMA buffer from a checkpoint with ``network``'s keys (what ``ema_state_dict`` wrote)."""
        by_id = {id(p): o for p, o in zip(self.arena.params, self.arena.offsets)}
        for k, p in network.named_parameters():
            if id(p) in by_id:
                if k not in sd or tuple(sd[k].shape) != tuple(p.shape):
                    raise ValueError('EMA checkpoint: %s is missing or has another shape' % k)
                o = by_id[id(p)]
                self.ema[o:o + p.numel()].copy_(sd[k].reshape(-1))

    def zero_grad(self, set_to_none=False):
        self.arena.zero_grad()

    def _runs(self):
        """[(start, end, lr, b1, b2, eps)] over the arena: contiguous parameters with equal hyper-parameters merged."""
        a = self.arena
        runs, i = [], 0
        for g in self.param_groups:
            n = len(g['params'])
            if n == 0:
                continue
            start = a.offsets[i]
            end = a.offsets[i + n] if i + n < len(a.offsets) else a.total
            hp = (float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']))
            if runs and runs[-1][2:] == hp and runs[-1][1] == start:
                runs[-1] = (runs[-1][0], end) + hp
            else:
                runs.append((start, end) + hp)
            i += n
        return runs

    # ---- one optimizer step in pieces (bucket by bucket, as the gradients become final during the backward pass) ----
    def begin_step(self):
        """Open a step that ``step_range`` will carry out piecewise; ``step()`` closes it (whatever is left)."""
        if getattr(self, '_done', None):
            raise RuntimeError('a piecewise optimizer step is still open (aborted after part of the arena was updated): '
                               'step() completes it')
        self._check_live()
        self.step_count += 1
        self._ema_open()
        self._done = []

    def abort_step(self):
        """An exception between ``begin_step`` and ``step``.  Nothing applied yet: the step is forgotten (count restored,
        the next ``step()`` is a whole step).  Part of the arena already updated: the step STAYS OPEN with its
        coverage -- the next ``step()`` completes the complement under the same step count, so no range is ever updated
        twice by one step and none is skipped; ``begin_step`` refuses to open another step on top of it."""
        done = getattr(self, '_done', None)
        if done is not None and not done:
            self.step_count -= 1
            if self.ema is not None:
                self.ema_updates -= 1
            self._done = None

    def _adam(self, lo, hi):
        a = self.arena
        for (s, e, lr, b1, b2, eps) in self._runs():
            s, e = max(s, lo), min(e, hi)
            if s >= e:
                continue
            if self.guard is not None:      # the kernel reads the skip flag and the clip coefficient from guard.st_adam
                lib.him_adam_guarded_step(a.data.data_ptr() + 4 * s, a.grad.data_ptr() + 4 * s,
                                          self.exp_avg.data_ptr() + 4 * s, self.exp_avg_sq.data_ptr() + 4 * s,
                                          0 if self.ema is None else self.ema.data_ptr() + 4 * s, e - s, lr, b1, b2, eps,
                                          self.step_count, self._ema_now, self.guard.st_adam.data_ptr(), _stream())
            elif self.ema is None:
                lib.him_adam_step(a.data.data_ptr() + 4 * s, a.grad.data_ptr() + 4 * s, self.exp_avg.data_ptr() + 4 * s,
                                  self.exp_avg_sq.data_ptr() + 4 * s, e - s, lr, b1, b2, eps, self.step_count, _stream())
            else:       # the same pass also averages [s, e): every element exactly once per step, as Adam visits it
                lib.him_adam_ema_step(a.data.data_ptr() + 4 * s, a.grad.data_ptr() + 4 * s,
                                      self.exp_avg.data_ptr() + 4 * s, self.exp_avg_sq.data_ptr() + 4 * s,
                                      self.ema.data_ptr() + 4 * s, e - s, lr, b1, b2, eps, self.step_count,
                                      self._ema_now, _stream())

    def _params_in(self, lo, hi):
        a = self.arena
        i = bisect.bisect_left(a.offsets, lo)
        out = []
        while i < len(a.offsets) and a.offsets[i] < hi:
            out.append(a.params[i])
            i += 1
        return out

    def step_range(self, lo, hi):
        """Adam update + panel rebuild of arena elements [lo, hi) on the current stream.  The caller guarantees that their
        gradients are final (and exchanged) and that nothing still reads these parameters (their layers' data gradients
        have run) -- the data-parallel reducer's bucket trigger (dist.GradReducer.bucket_hook)."""
        if getattr(self, '_done', None) is None:
            raise RuntimeError('step_range outside begin_step() ... step()')
        self._check_live()
        if self.guard is not None:
            # the global norm needs EVERY gradient: the range is only recorded, step() updates the whole arena at once
            self._done.append((lo, hi))
            return
        self._adam(lo, hi)
        self._done.append((lo, hi))
        from .ops import refresh_panels
        refresh_panels(self._params_in(lo, hi))

    def step(self):
        a = self.arena
        self._check_live()
        from .ops import join_side_stream, refresh_panels
        join_side_stream(a.grad.device)        # wait for the side-stream weight gradients
        done = getattr(self, '_done', None)
        if done is None:
            self.step_count += 1
            self._ema_open()
            todo = [(0, a.total)]
        else:                                  # close a piecewise step: the complement of what step_range has covered
            todo, at = [], 0
            for lo, hi in sorted(done):
                if lo > at:
                    todo.append((at, lo))
                at = max(at, hi)
            if at < a.total:
                todo.append((at, a.total))
            self._done = None
        if self.guard is not None:
            # One statistics pass over the whole arena, then the guarded kernel over all of it (step_range has applied
            # nothing).  Data parallel: the reducer has finished, every rank holds the same gradients and the statistics
            # are a deterministic function of them, so the ranks take the same decision without another collective.
            todo, done = [(0, a.total)], None
            self._guard_stats()
        for lo, hi in todo:
            self._adam(lo, hi)
        # everything that reads the RAW parameters may start here; every cached weight panel carries its own event
        # (ops._panel waits for it), so a consumer need not wait for the whole rebuild pass below
        self.updated = torch.cuda.Event()
        self.updated.record(torch.cuda.current_stream(a.data.device))
        for lo, hi in todo:                    # regrouped weight panels of the conv kernels follow the update
            refresh_panels(self._params_in(lo, hi) if done is not None else a.params)

    def load_moments(self, exp_avgs, exp_avg_sqs, step):
        """Adopt per-parameter Adam moments (e.g. from a torch.optim.Adam) -- used by checkpoint import and by the
        teacher-forced parity tests."""
        a = self.arena
        for p, o, m, v in zip(a.params, a.offsets, exp_avgs, exp_avg_sqs):
            n = p.numel()
            self.exp_avg[o:o + n].copy_(m.reshape(-1))
            self.exp_avg_sq[o:o + n].copy_(v.reshape(-1))
        self.step_count = int(step)

    def state_dict(self):
        """``torch.optim.Adam.state_dict()`` layout (what the reference's ``save_network_dict`` pickles,
        ``models/base_model.py:52-66``): per-parameter ``step / exp_avg / exp_avg_sq`` keyed by the parameter's index,
        plus ``param_groups`` with index lists -- loadable by a ``torch.optim.Adam`` over the same parameter list."""
        a = self.arena
        state = {}
        if self.step_count > 0:
            for i, (p, o) in enumerate(zip(a.params, a.offsets)):
                n = p.numel()
                state[i] = dict(step=torch.tensor(float(self.step_count)),
                                exp_avg=self.exp_avg[o:o + n].view(p.shape).cpu().clone(),
                                exp_avg_sq=self.exp_avg_sq[o:o + n].view(p.shape).cpu().clone())
        groups, i = [], 0
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != 'params'}
            for k, v in (('weight_decay', 0), ('amsgrad', False), ('maximize', False), ('foreach', None),
                         ('capturable', False), ('differentiable', False), ('fused', None)):
                d.setdefault(k, v)
            d['params'] = list(range(i, i + len(g['params'])))
            i += len(g['params'])
            groups.append(d)
        return dict(state=state, param_groups=groups)

    def load_state_dict(self, sd):
        """Accepts a ``torch.optim.Adam`` state dict (any torch era: ``step`` as int or tensor) or this class's round-1
        flat-arena format (``step / exp_avg / exp_avg_sq`` over the padded arena)."""
        if 'state' in sd:
            a = self.arena
            st = sd['state']
            if len(st) == 0:
                self.exp_avg.zero_()
                self.exp_avg_sq.zero_()
                self.step_count = 0
            else:
                # Parameter ORDER comes from the file's own param_groups: torch >= 1.6 keys the state by index, but the
                # reference's era (torch 0.3 / 0.4) keys it by id(p) -- memory addresses, also listed per group -- whose
                # numeric order says nothing about the parameter order.  A parameter without an entry (never received a
                # gradient) gets zero moments.  DEVIATION from torch, warned about below: torch would start such a
                # parameter at step 0 (bias corrections 1-b1, 1-b2 on its first update); this optimizer has ONE fused step
                # count, so its first update uses the corrections of step N+1 -- (1-b1)/sqrt(1-b2) times smaller.
                order = [pid for g in sd['param_groups'] for pid in g['params']]
                if len(order) != len(a.params):
                    raise ValueError('optimizer state lists %d parameters, the arena holds %d' % (len(order), len(a.params)))
                known = set(order)
                unknown = [k for k in st.keys() if k not in known]
                if unknown:
                    raise ValueError('optimizer state has entries no param_group lists: %s' % unknown[:4])
                ms, vs, steps = [], [], set()
                for pid, p in zip(order, a.params):
                    e = st.get(pid)
                    if e is None:
                        ms.append(torch.zeros(p.shape))
                        vs.append(torch.zeros(p.shape))
                        continue
                    if tuple(e['exp_avg'].shape) != tuple(p.shape):
                        raise ValueError('optimizer state %s: shape %s vs parameter %s'
                                         % (pid, tuple(e['exp_avg'].shape), tuple(p.shape)))
                    ms.append(e['exp_avg'])
                    vs.append(e['exp_avg_sq'])
                    steps.add(int(float(e['step'])))
                if len(steps) != 1:
                    raise ValueError('per-parameter step counts differ (%s): one fused step count only' % sorted(steps))
                missing = sum(1 for pid in order if pid not in st)
                if missing:
                    import warnings
                    warnings.warn('%d of %d parameters have no Adam state in the file: they start from zero moments at the '
                                  'shared step count %d (torch would restart them at step 0)'
                                  % (missing, len(order), next(iter(steps))))
                self.load_moments(ms, vs, steps.pop())
            for g, s in zip(self.param_groups, sd['param_groups']):
                for k in ('lr', 'betas', 'eps'):
                    if k in s:
                        g[k] = tuple(s[k]) if k == 'betas' else s[k]
                if s.get('weight_decay', 0) or s.get('amsgrad', False):
                    raise NotImplementedError('weight_decay / amsgrad are not used by the reference and not supported')
            return
        self.step_count = int(sd['step'])
        self.exp_avg.copy_(sd['exp_avg'])
        self.exp_avg_sq.copy_(sd['exp_avg_sq'])
        for g, s in zip(self.param_groups, sd['param_groups']):
            g.update(s)
