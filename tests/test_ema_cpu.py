"""Weight EMA, the parts that need no GPU: the three C-ABI entries (exported, declared, bound with matching argument
lists), the two options in the four parsers, and the host-side decay schedule."""
import ctypes
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))

# C parameter type -> the ctypes type the binding must use
C2CTYPES = {'float*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'size_t': ctypes.c_size_t,
            'double': ctypes.c_double, 'int': ctypes.c_int}
ENTRIES = ('him_adam_ema_step', 'him_ema_update', 'him_swap')


def _declared(name):
    with open(os.path.join(ROOT, 'include', 'him.h')) as f:
        src = f.read()
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, src)
    assert m, '%s is not declared in include/him.h' % name
    out = []
    for arg in m.group(1).split(','):
        words = arg.split()
        out.append(' '.join(words[:-1]))          # drop the parameter name
    return out


@pytest.mark.parametrize('name', ENTRIES)
def test_entry_is_exported_declared_and_bound_alike(name):
    from neurips18_hierchical_image_manipulation_amd import _cabi
    assert name in _cabi.EXPORTS
    assert hasattr(ctypes.CDLL(_cabi.LIB_PATH), name), '%s is not exported by the built library' % name
    res, args = _cabi._SIGS[name]
    assert res is ctypes.c_int
    assert args == [C2CTYPES[t] for t in _declared(name)], (name, _declared(name))


def test_fused_entry_is_the_adam_entry_plus_the_shadow_buffer_and_the_decay():
    adam, fused = _declared('him_adam_step'), _declared('him_adam_ema_step')
    assert fused == adam[:4] + ['float*'] + adam[4:-1] + ['double'] + adam[-1:]


@pytest.mark.parametrize('which', ['train', 'test', 'box2mask_train', 'box2mask_test'])
def test_the_two_options_exist_with_their_defaults(which):
    from neurips18_hierchical_image_manipulation_amd import options
    cls = dict(train=options.MaskToImageTrainOptions, test=options.MaskToImageTestOptions,
               box2mask_train=options.BoxToMaskTrainOptions, box2mask_test=options.BoxToMaskTestOptions)[which]
    opt = cls().parse(save=False, default_args=[])
    assert opt.ema_decay == 0.0 and type(opt.ema_decay) is float
    assert opt.use_ema is False
    opt = cls().parse(save=False, default_args=['--ema_decay', '0.999', '--use_ema'])
    assert opt.ema_decay == 0.999 and opt.use_ema is True


def test_decay_schedule_values():
    """min(decay, (1 + t) / (10 + t)) in double: the ramp at t = 0, 1, 89, the first update at the full decay (8991/9000
    equals 0.999 only up to rounding at t = 8990; at 8991 the ramp is above it)."""
    from neurips18_hierchical_image_manipulation_amd.optim import ema_decay_at, ema_warm_count
    assert ema_decay_at(0.999, 0) == 1.0 / 10.0
    assert ema_decay_at(0.999, 1) == 2.0 / 11.0
    assert ema_decay_at(0.999, 89) == 90.0 / 99.0
    assert ema_decay_at(0.999, 8991) == 0.999
    assert ema_decay_at(0.5, 8) == 0.5 and ema_decay_at(0.5, 7) == 8.0 / 17.0
    t = ema_warm_count(0.999)
    assert ema_decay_at(0.999, t) == 0.999 and (1.0 + (t - 1)) / (10.0 + (t - 1)) < 0.999


class _FakeArena(object):
    """What FusedAdam reads of a FlatArena, on the host (no kernel is launched by the calls below)."""

    def __init__(self):
        import torch
        self.params = [torch.nn.Parameter(torch.zeros(3))]
        self.offsets, self.total = [0], 64
        self.data, self.grad = torch.zeros(64), torch.zeros(64)


def test_ema_off_allocates_nothing_and_attach_validates():
    import torch
    from neurips18_hierchical_image_manipulation_amd.optim import FusedAdam
    arena = _FakeArena()
    o = FusedAdam(arena.params, arena=arena)
    assert o.ema is None and o.ema_decay == 0.0 and o.ema_updates == 0
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError):
            o.attach_ema(bad)
    assert o.ema is None
    o.attach_ema(0.999)
    assert o.ema is not arena.data and torch.equal(o.ema, arena.data)
    # one decay per step, opened once: a forgotten piecewise step also forgets its update count
    o.begin_step()
    assert (o.ema_updates, o._ema_now) == (1, 0.1)
    o.abort_step()
    assert (o.ema_updates, o.step_count) == (0, 0)
    # an optimizer rebuilt over the same arena takes buffer and count along
    o.ema_updates = 7
    n = FusedAdam(arena.params, arena=arena).adopt_ema(o)
    assert n.ema is o.ema and (n.ema_decay, n.ema_updates) == (0.999, 7)
    # the optimizer state keeps torch.optim.Adam's layout: nothing of the EMA in it
    assert set(o.state_dict()) == {'state', 'param_groups'}
    assert not any('ema' in k for g in o.state_dict()['param_groups'] for k in g)


@pytest.mark.parametrize('multiline', [False, True])
def test_a_joint_inference_script_may_carry_use_ema_for_either_model(tmp_path, multiline):
    from neurips18_hierchical_image_manipulation_amd import options
    from neurips18_hierchical_image_manipulation_amd.util.util import load_script_to_opt
    for cls, model in ((options.BoxToMaskTestOptions, 'AE_maskgen_twostream'),
                       (options.MaskToImageTestOptions, 'pix2pixHD_condImg')):
        flags = ['--model %s' % model, '--use_ema', '--name x']
        path = tmp_path / ('%s_%d.sh' % (model, multiline))
        if multiline:
            path.write_text('python test.py \\\n' + ''.join('%s \\\n' % f for f in flags))
        else:
            path.write_text('python test.py ' + ' '.join(flags))
        opt = load_script_to_opt(str(path), cls)
        assert opt.use_ema is True and opt.model == model and opt.name == 'x' and opt.ema_decay == 0.0
