"""Gradient guard, the parts that need no GPU: the three C-ABI entries (exported, declared, bound with matching argument
lists), the two options in the four parsers, the optimizer's off state and argument checks, and the host builder of the
segment / chunk tables against a brute-force enumeration."""
import ctypes
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

# C type -> the ctypes type the binding must use (device pointers travel as integers)
C2CTYPES = {'float*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'void*': ctypes.c_void_p,
            'double*': ctypes.c_void_p, 'const double*': ctypes.c_void_p, 'const long long*': ctypes.c_void_p,
            'size_t': ctypes.c_size_t, 'double': ctypes.c_double, 'int': ctypes.c_int}
ENTRIES = ('him_grad_stats_ws', 'him_grad_stats', 'him_adam_guarded_step')


def _declared(name):
    """(return type, [parameter types]) of ``name`` in include/him.h, comments removed."""
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        src = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    m = re.search(r'\b(int|size_t)\s+%s\s*\(([^)]*)\)\s*;' % name, src)
    assert m, '%s is not declared in include/him.h' % name
    return m.group(1), [' '.join(arg.split()[:-1]) for arg in m.group(2).split(',')]      # drop the parameter names


@pytest.mark.parametrize('name', ENTRIES)
def test_entry_is_exported_declared_and_bound_alike(name):
    from neurips18_hierchical_image_manipulation_amd import _cabi
    assert name in _cabi.EXPORTS
    assert hasattr(ctypes.CDLL(_cabi.LIB_PATH), name), '%s is not exported by the built library' % name
    res, args = _cabi._SIGS[name]
    cres, cargs = _declared(name)
    assert res is C2CTYPES[cres]
    assert args == [C2CTYPES[t] for t in cargs], (name, cargs)


def test_guarded_entry_is_the_fused_entry_plus_the_statistics_pointer():
    fused, guarded = _declared('him_adam_ema_step')[1], _declared('him_adam_guarded_step')[1]
    assert guarded == fused[:-1] + ['const double*'] + fused[-1:]


def test_workspace_size_grows_with_both_arguments_and_holds_the_chunk_list():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    from neurips18_hierchical_image_manipulation_amd.optim import GUARD_CHUNK
    ws = _cabi.lib.him_grad_stats_ws
    assert ws(0, 0) > 0 and ws(GUARD_CHUNK * 10, 0) > ws(0, 0) and ws(0, 5) > ws(0, 0)
    # a chunk's work-list entry and its partial take 16 bytes each; at most n / chunk + 2 nseg + 1 chunks exist
    assert ws(GUARD_CHUNK * 10 + 1, 3) >= 32 * (10 + 7)


@pytest.mark.parametrize('which', ['train', 'test', 'box2mask_train', 'box2mask_test'])
def test_the_two_options_exist_with_their_defaults(which):
    from neurips18_hierchical_image_manipulation_amd import options
    cls = dict(train=options.MaskToImageTrainOptions, test=options.MaskToImageTestOptions,
               box2mask_train=options.BoxToMaskTrainOptions, box2mask_test=options.BoxToMaskTestOptions)[which]
    opt = cls().parse(save=False, default_args=[])
    assert opt.clip_grad_norm == 0.0 and type(opt.clip_grad_norm) is float
    assert opt.skip_nonfinite is False
    opt = cls().parse(save=False, default_args=['--clip_grad_norm', '2.5', '--skip_nonfinite'])
    assert opt.clip_grad_norm == 2.5 and type(opt.clip_grad_norm) is float and opt.skip_nonfinite is True
    assert opt.ema_decay == 0.0 and opt.use_ema is False


def test_complete_fills_the_two_options():
    from neurips18_hierchical_image_manipulation_amd.options import complete
    opt = complete({})
    assert opt.clip_grad_norm == 0.0 and opt.skip_nonfinite is False


class _FakeArena(object):
    """What FusedAdam and the guard read of a FlatArena, on the host (no kernel is launched by the calls below)."""

    def __init__(self):
        import torch
        self.params = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(70))]
        self.offsets, self.total = [0, 64], 192
        self.data, self.grad = torch.zeros(192), torch.zeros(192)


def test_guard_off_allocates_nothing_and_attach_validates():
    from neurips18_hierchical_image_manipulation_amd.optim import FusedAdam
    arena = _FakeArena()
    o = FusedAdam(arena.params, arena=arena)
    assert o.guard is None
    for bad in (-1.0, -1e-30, float('nan')):
        with pytest.raises(ValueError):
            o.attach_guard(bad)
    assert o.guard is None
    with pytest.raises(RuntimeError):
        o.grad_stats()
    o.begin_step()
    with pytest.raises(RuntimeError):
        o.attach_guard(1.0)
    o.abort_step()
    o.attach_guard(1.5, skip_nonfinite=False)
    gd = o.guard
    assert (gd.max_norm, gd.skip_nonfinite, gd.nseg) == (1.5, False, 2)
    assert gd.seg.tolist() == [[0, 3], [64, 70]] and tuple(gd.seg_out.shape) == (2, 2)
    assert tuple(gd.st.shape) == (8,) and not bool(gd.st.any())
    assert gd.st_adam is not gd.st and tuple(gd.st_adam.shape) == (8,)      # clip only: a flag slot that stays zero
    assert gd.ws.numel() == gd.ws_bytes > 0
    assert FusedAdam(arena.params, arena=arena).attach_guard(float('inf')).guard.st_adam is not None
    on = FusedAdam(arena.params, arena=arena).attach_guard(0.0, True)
    assert on.guard.st_adam is on.guard.st
    # a rebuilt optimizer over the same arena takes the guard, counters included, along
    n = FusedAdam(arena.params, arena=arena).adopt_guard(o)
    assert n.guard is gd
    # with a guard step_range only records: no kernel runs on this host arena, the step stays open with its coverage
    o.begin_step()
    o.step_range(0, 64)
    assert o._done == [(0, 64)] and o.step_count == 1
    # the optimizer state keeps torch.optim.Adam's layout
    assert set(o.state_dict()) == {'state', 'param_groups'}


# ---- the host table builder against brute force ------------------------------------------------------------------------
def _brute(sizes, chunk):
    """Element by element: the owner range of every arena element, then maximal runs of (range, chunk index)."""
    offsets, off = [], 0
    for n in sizes:
        offsets.append(off)
        off += (n + 63) // 64 * 64
    total = off
    owner, start = [None] * total, {}
    for i, (o, n) in enumerate(zip(offsets, sizes)):
        for e in range(o, o + n):
            owner[e] = 2 * i + 1
    gap = 0
    for e in range(total):
        if owner[e] is None:
            owner[e] = gap                       # padding: the gap in front of the next parameter
        else:
            gap = owner[e] + 1
        start.setdefault(owner[e], e)            # a range starts at its first element
    work = []
    for e in range(total):
        key = (owner[e], (e - start[owner[e]]) // chunk)
        if work and work[-1][0] == key:
            work[-1][2] += 1
        else:
            work.append([key, e, 1])
    return offsets, total, [(k[0], s, n) for k, s, n in work]


CH = 256      # a small chunk for the enumeration; the builder takes it as a parameter


@pytest.mark.parametrize('sizes', [
    [1, 63, 64, 65],
    [CH - 1, CH, CH + 1],
    [3 * CH + 1],
    [65, 5 * CH + 1, 1, CH - 1, 64, 2 * CH + 1],
])
def test_table_builder_against_brute_force(sizes):
    from neurips18_hierchical_image_manipulation_amd.optim import guard_tables
    offsets, total, ref = _brute(sizes, CH)
    seg, work = guard_tables(offsets, sizes, total, chunk=CH)
    assert seg == list(zip(offsets, sizes))
    assert work == ref
    # every element of the arena is in exactly one chunk, no chunk is longer than the chunk size or empty
    assert sum(n for _, _, n in work) == total and all(0 < n <= CH for _, _, n in work)
    assert [r for r, _, _ in work] == sorted(r for r, _, _ in work)


def test_table_builder_at_the_library_chunk_size_and_its_argument_checks():
    from neurips18_hierchical_image_manipulation_amd.optim import GUARD_CHUNK, guard_tables
    sizes = [GUARD_CHUNK - 1, GUARD_CHUNK, GUARD_CHUNK + 1, 3 * GUARD_CHUNK + 1]
    offsets, total, ref = _brute(sizes, GUARD_CHUNK)
    seg, work = guard_tables(offsets, sizes, total)
    assert work == ref
    per_seg = [sum(1 for r, _, _ in work if r == 2 * i + 1) for i in range(4)]
    assert per_seg == [1, 1, 2, 4]
    assert guard_tables([], [], 0) == ([], [])
    assert guard_tables([], [], 70, chunk=64) == ([], [(0, 0, 64), (0, 64, 6)])
    for bad in (([64, 0], [1, 1], 128), ([0], [65], 64), ([0, 32], [64, 1], 128)):
        with pytest.raises(ValueError):
            guard_tables(*bad)
