"""The gradient guard through the optimizer and the trainers (--clip_grad_norm / --skip_nonfinite / ``grad_report()``),
on the tiny configurations of the trainer tests.

Everything here is bit for bit: a guard that does not clip (max_norm 1e30) must leave the trajectory of the unguarded
run, whatever schedule cuts the Adam step into pieces (with a guard ``step_range`` defers to ``step()``); a clipped step
equals an unguarded step on gradients scaled by the fp32 coefficient; a skipped step changes nothing.  The reported norm
is bounded like the statistics themselves (tests/test_grad_guard_abi_gpu.py): the sum of squares within count * 2^-53
relative, so the norm within (count / 2 + 2) * 2^-53 (half the sum's error, the square root's rounding, one to spare)."""
import functools
import json
import math

import pytest
import torch

from util import load_golden

pytestmark = pytest.mark.gpu

NAMES = ['G_GAN', 'G_GAN_Feat', 'G_VGG', 'D_real', 'D_fake']
TINY = dict(model='pix2pixHD_condImg', netG='global', ngf=8, ndf=8, n_downsample_global=2, n_blocks_global=2, num_D=2,
            n_layers_D=3, label_nc=35, no_instance=True)
B, H, W = 2, 32, 64
DECAY = 0.999
KEYS = {'G_grad_norm', 'D_grad_norm', 'G_clip_coef', 'D_clip_coef', 'G_skipped', 'D_skipped'}


def build(tmp, **extra):
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    from neurips18_hierchical_image_manipulation_amd import synth
    model = create_model(dict(TINY, gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp), name='t', ema_decay=DECAY, **extra))
    model.netG.load_state_dict(synth.init_state_dict(model.netG.state_dict(), 1))
    model.netD.load_state_dict(synth.init_state_dict(model.netD.state_dict(), 2))
    model.optimizer_G.reset_ema()
    return model


def batch(s, bad=False):
    from neurips18_hierchical_image_manipulation_amd import synth
    b = synth.make_batch(s, 0, B, H, W, 35, False)
    if bad:
        b['image'][0, 0, 0, 0] = float('inf')       # one Inf pixel of the real image: ordinary arithmetic from here on
    return b


def state(model):
    model.sync()
    torch.cuda.synchronize()
    oG, oD = model.optimizer_G, model.optimizer_D
    return [t.clone() for t in (oG.arena.data, oG.exp_avg, oG.exp_avg_sq, oG.ema, oD.arena.data, oD.exp_avg, oD.exp_avg_sq)]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@functools.lru_cache(None)
def three(options=(), sched=()):
    """Three clean steps -> (model, losses, state)."""
    from neurips18_hierchical_image_manipulation_amd import config
    with config.schedule(**dict(sched)):
        m = build('/tmp/him_test_guard', **dict(options))
        losses = []
        for s in range(3):
            ld = m.optimize_parameters(batch(s))
            losses.append([float(ld[k]) for k in NAMES])
        return m, losses, state(m)


def test_flags_off_no_guard_and_the_same_trajectory():
    plain = three()
    off = three((('clip_grad_norm', 0.0), ('skip_nonfinite', False)))
    for m in (plain[0], off[0]):
        assert m.optimizer_G.guard is None and m.optimizer_D.guard is None
        with pytest.raises(RuntimeError):
            m.grad_report()
    assert plain[1] == off[1] and same(plain[2], off[2])


@pytest.mark.parametrize('sched', ['default', 'chunked', 'unsplit'])
def test_a_guard_that_does_not_clip_leaves_the_trajectory(sched):
    """default: Adam split around the stem (begin_step / step_range / step); chunked: the local reducer attached, Adam
    bucket by bucket -- both reach the guard through the deferred step_range; unsplit: one step()."""
    kw = dict(default=(), chunked=(('adam_chunked', True),), unsplit=(('adam_split_stem', False),))[sched]
    plain = three()
    m, losses, st = three((('clip_grad_norm', 1e30),), kw)
    assert m.optimizer_G.guard is not None and m.optimizer_D.guard is not None
    assert m.optimizer_G.guard.skip_nonfinite is False
    if sched == 'chunked':
        assert m.reducer_G is not None
    assert losses == plain[1]
    assert same(st, plain[2]), 'weights, moments or EMA differ from the unguarded run (%s)' % sched
    r = m.grad_report()
    assert set(r) == KEYS
    assert (r['G_clip_coef'], r['D_clip_coef'], r['G_skipped'], r['D_skipped']) == (1.0, 1.0, 0, 0)
    assert m.optimizer_G.grad_report()['steps'] == 3 and m.optimizer_G.step_count == 3


def test_grad_report_against_float64_and_parameter_names():
    m = three((('clip_grad_norm', 1e30),))[0]
    r = m.grad_report()
    for tag, o, net in (('G', m.optimizer_G, m.netG), ('D', m.optimizer_D, m.netD)):
        g = o.arena.grad.double().cpu()             # the last step's gradients are still in the arena
        ref = math.sqrt(math.fsum((g * g).tolist()))
        bound = (g.numel() / 2 + 2) * 2.0 ** -53 * ref
        err = abs(r[tag + '_grad_norm'] - ref)
        print('%s: norm %.17g ref %.17g err %.3e bound %.3e' % (tag, r[tag + '_grad_norm'], ref, err, bound))
        assert ref > 0.0 and err <= bound
        full = o.grad_report(net)
        names = [k for k, _ in net.named_parameters()]
        assert list(full['per_param']) == names and full['worst'] in names
        assert full['per_param'][full['worst']] == max(full['per_param'].values())
        for (k, p), off in zip(net.named_parameters(), o.arena.offsets):
            pg = g[off:off + p.numel()]
            pref = math.sqrt(math.fsum((pg * pg).tolist()))
            assert abs(full['per_param'][k] - pref) <= (p.numel() / 2 + 2) * 2.0 ** -53 * pref, k
        st, norms = o.grad_stats()
        assert st.is_cuda and norms.is_cuda and tuple(st.shape) == (8,) and norms.numel() == len(names)


def test_a_non_finite_batch_is_skipped_and_the_next_step_trains(tmp_path):
    m = build(tmp_path, skip_nonfinite=True)
    assert m.optimizer_G.guard.max_norm == 0.0 and m.optimizer_G.guard.skip_nonfinite is True
    m.optimize_parameters(batch(0))
    before = state(m)
    assert m.grad_report()['G_skipped'] == 0
    m.optimize_parameters(batch(1, bad=True))
    after = state(m)
    assert same(before, after), 'a skipped step changed parameters, moments or the EMA'
    r = m.grad_report()
    assert (r['G_skipped'], r['D_skipped']) == (1, 1) and set(r) == KEYS
    full = m.optimizer_D.grad_report(m.netD)
    assert full['nonfinite'] > 0 and full['steps'] == 2
    # attempts are counted on the host, skips on the device
    assert m.optimizer_G.step_count == 2 and m.optimizer_G.ema_updates == 2
    m.optimize_parameters(batch(2))
    then = state(m)
    assert not torch.equal(then[0], after[0]) and not torch.equal(then[4], after[4])
    assert all(bool(torch.isfinite(t).all()) for t in then)
    assert (m.grad_report()['G_skipped'], m.grad_report()['D_skipped']) == (1, 1)


def test_the_same_batch_without_the_flag_leaves_non_finite_weights(tmp_path):
    """Clipping alone (the statistics run, the kernel reads a flag slot that stays zero): the step is taken."""
    m = build(tmp_path, clip_grad_norm=1e30)
    m.optimize_parameters(batch(0))
    m.optimize_parameters(batch(1, bad=True))
    s = state(m)
    assert not bool(torch.isfinite(s[0]).all()) and not bool(torch.isfinite(s[4]).all())
    r = m.grad_report()
    assert (r['G_skipped'], r['D_skipped']) == (1, 1)       # the statistics still saw it


def test_update_fixed_params_keeps_the_guard(tmp_path):
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    flags = dict(model='pix2pixHD_condImg', netG='local', ngf=8, ndf=8, n_downsample_global=2, n_blocks_global=2,
                 n_local_enhancers=1, n_blocks_local=2, num_D=2, label_nc=35, no_instance=True, niter_fix_global=3)
    m = create_model(dict(flags, gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp_path), name='t', clip_grad_norm=5.0,
                          skip_nonfinite=True))
    gd = m.optimizer_G.guard
    assert gd is not None and (gd.max_norm, gd.skip_nonfinite) == (5.0, True)
    old = m.optimizer_G
    m.update_fixed_params()
    assert m.optimizer_G is not old and m.optimizer_G.guard is gd


# ---- optimizer level ----------------------------------------------------------------------------------------------------
SHAPES = [(3,), (70,), (64,), (10, 100), (20000,)]       # the last one spans two chunks of the statistics pass


def _optimizer(grads=None, ema=True):
    from neurips18_hierchical_image_manipulation_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.1).cuda()) for s in SHAPES]
    o = FusedAdam(params, lr=1e-3)
    if ema:
        o.attach_ema(0.9)
    if grads is not None:
        o.arena.grad.copy_(grads)
    return o


def _opt_state(o):
    torch.cuda.synchronize()
    return [t.clone() for t in (o.arena.data, o.exp_avg, o.exp_avg_sq, o.ema)]


def _grads(total, offsets, step):
    g = torch.zeros(total)
    vals = torch.randn(total, generator=torch.Generator().manual_seed(50 + step))
    for s, o in zip(SHAPES, offsets):
        n = int(torch.Size(s).numel())
        g[o:o + n] = vals[o:o + n]
    return g


def test_optimizer_piecewise_guarded_step_and_clipping_against_prescaled_gradients():
    probe = _optimizer()
    total, offsets = probe.arena.total, probe.arena.offsets
    piece, whole, plain = _optimizer(), _optimizer(), _optimizer()
    cut = offsets[3]
    piece.attach_guard(1.0)
    whole.attach_guard(1.0)
    for step in range(3):
        g = _grads(total, offsets, step)
        max_norm = 0.5 * math.sqrt(math.fsum((g.double() * g.double()).tolist()))      # half the measured norm
        for o in (piece, whole):
            o.guard.max_norm = max_norm
            o.arena.grad.copy_(g)
        piece.begin_step()
        piece.step_range(0, cut)
        assert torch.equal(piece.arena.data, plain.arena.data), 'step_range applied something with a guard attached'
        piece.step_range(cut, total)
        piece.step()
        whole.step()
        st, norms = whole.grad_stats()
        c = float(st[3])
        assert 0.49 < c < 0.51 and float(st[1]) == 0.0
        assert torch.equal(whole.arena.grad.cpu(), g), 'clipping rewrote the gradient arena'
        plain.arena.grad.copy_((g.double() * c).float())          # fl32(g * c): exact product, one rounding
        plain.step()
        a, b, p = _opt_state(piece), _opt_state(whole), _opt_state(plain)
        assert same(a, b), 'step_range + step() differs from a plain guarded step() at step %d' % step
        assert same(b, p), 'a clipped step differs from an unguarded step on pre-scaled gradients at step %d' % step
    assert not torch.equal(whole.arena.data, probe.arena.data)
    assert piece.step_count == whole.step_count == plain.step_count == 3


def test_optimizer_skip_and_clip_only():
    g = _grads(_optimizer().arena.total, _optimizer().arena.offsets, 9)
    bad = g.clone()
    bad[5] = float('nan')
    skip, clip, plain = _optimizer(bad), _optimizer(bad), _optimizer(g)
    start = _opt_state(skip)
    skip.attach_guard(0.0, skip_nonfinite=True)
    skip.step()
    assert same(_opt_state(skip), start) and skip.step_count == 1
    r = skip.grad_report()
    assert (r['nonfinite'], r['steps'], r['skipped'], r['clip_coef']) == (1, 1, 1, 1.0)
    clip.attach_guard(1e30, skip_nonfinite=False)
    clip.step()
    assert not bool(torch.isfinite(clip.arena.data).all())
    assert clip.grad_report()['skipped'] == 1
    # the clean gradient after the skip: the step is taken, with the bias corrections of step 2
    skip.arena.grad.copy_(g)
    skip.step()
    plain.step_count = 1
    plain._ema_open()
    plain.step()
    assert same(_opt_state(skip), _opt_state(plain))
    assert skip.grad_report()['skipped'] == 1 and skip.grad_report()['steps'] == 2


# ---- box2mask -------------------------------------------------------------------------------------------------------------
def _b2m_run(tmp, bad_step=None, **extra):
    from neurips18_hierchical_image_manipulation_amd import synth
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    g = load_golden('box2mask_traj')
    fl = dict(json.loads(str(g['flags'])), isTrain=True, ema_decay=DECAY, **extra)
    model = create_model(dict(fl, model='AE_maskgen_twostream', gpu_ids=[0], checkpoints_dir=str(tmp), name='b'))
    model.netG.load_state_dict(synth.init_state_dict(model.netG.state_dict(), 21))
    model.netD.load_state_dict(synth.init_state_dict(model.netD.state_dict(), 22))
    model.optimizer.reset_ema()
    o, oD = model.optimizer, model.optimizer_D
    trail = []
    for s in range(3):
        b = synth.make_box2mask_batch(s, 0, int(g['B']), int(g['H']), int(g['W']), 35)
        if s == bad_step:
            b['mask_obj_inst'][0, 0, 0, 0] = float('inf')
        model.forward(b['label'], None, b['mask_ctx_in'], None, b['mask_out'], b['mask_obj_inst'], b['cls'], b['mask_in'],
                      eval_mode=False)
        torch.cuda.synchronize()
        trail.append([t.clone() for t in (o.arena.data, o.exp_avg, o.exp_avg_sq, o.ema, oD.arena.data, oD.exp_avg,
                                          oD.exp_avg_sq)])
    return model, trail


def test_box2mask_clip_and_skip(tmp_path):
    plain, ptrail = _b2m_run(tmp_path / 'p')
    assert plain.optimizer.guard is None and plain.optimizer_D.guard is None
    clip, ctrail = _b2m_run(tmp_path / 'c', clip_grad_norm=1e30)
    assert clip.optimizer.guard is not None and clip.optimizer_D.guard is not None
    assert same(ctrail[2], ptrail[2]), 'a guard that does not clip changed the box2mask trajectory'
    r = clip.grad_report()
    assert set(r) == KEYS and (r['G_clip_coef'], r['D_clip_coef'], r['G_skipped'], r['D_skipped']) == (1.0, 1.0, 0, 0)
    assert r['G_grad_norm'] > 0.0 and r['D_grad_norm'] > 0.0
    skip, strail = _b2m_run(tmp_path / 's', bad_step=1, skip_nonfinite=True)
    assert same(strail[0], ptrail[0])
    assert same(strail[1], strail[0]), 'a skipped box2mask step changed parameters, moments or the EMA'
    assert not torch.equal(strail[2][0], strail[1][0]) and not torch.equal(strail[2][4], strail[1][4])
    r = skip.grad_report()
    assert (r['G_skipped'], r['D_skipped']) == (1, 1)
    names = [k for k, _ in skip.netG.named_parameters()]
    assert list(skip.optimizer.grad_report(skip.netG)['per_param']) == names
