"""Generator weight EMA through the trainers (--ema_decay / --use_ema / ``model.ema_weights()``), on the tiny
configurations of the trainer tests.

The average is computed by the Adam kernel in the pass it already makes, so (1) switching it on may change nothing of a
trajectory, (2) every arena element must be averaged exactly once per step whatever schedule cuts the Adam step into
pieces, and (3) the buffer must follow ema' = ema + w (p' - ema) with the decay min(d, (1 + t) / (10 + t)) of update t.
Bound of (3): one step is within 3 * 2^-24 * max|.| of its float64 evaluation (tests/test_ema_abi_gpu.py); the recursion
contracts the carried error, so K steps stay within min(K, 1 / (1 - d)) = K times that."""
import functools
import json
import os

import pytest
import torch

from util import load_golden

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
NAMES = ['G_GAN', 'G_GAN_Feat', 'G_VGG', 'D_real', 'D_fake']
TINY = dict(model='pix2pixHD_condImg', netG='global', ngf=8, ndf=8, n_downsample_global=2, n_blocks_global=2, num_D=2,
            n_layers_D=3, label_nc=35, no_instance=True)
B, H, W = 2, 32, 64
DECAY = 0.999


def build(flags, tmp, **extra):
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    from neurips18_hierchical_image_manipulation_amd import synth
    model = create_model(dict(flags, gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp), name='t', **extra))
    model.netG.load_state_dict(synth.init_state_dict(model.netG.state_dict(), 1))
    model.netD.load_state_dict(synth.init_state_dict(model.netD.state_dict(), 2))
    model.optimizer_G.reset_ema()          # the weights were loaded after the optimizer was built
    return model


def batch(s, flags=TINY, color=False, h=H, w=W):
    from neurips18_hierchical_image_manipulation_amd import synth
    return synth.make_batch(s, 0, B, h, w, flags.get('label_nc', 35), color)


def state(model):
    model.sync()
    torch.cuda.synchronize()
    oG, oD = model.optimizer_G, model.optimizer_D
    return dict(params=[p.detach().clone() for p in list(model.netG.parameters()) + list(model.netD.parameters())],
                moments=[t.clone() for t in (oG.exp_avg, oG.exp_avg_sq, oD.exp_avg, oD.exp_avg_sq)],
                arena=oG.arena.data.clone(), ema=None if oG.ema is None else oG.ema.clone())


def run(decay, steps, tmp='/tmp/him_test_ema', flags=TINY, record=False, color=False, h=H, w=W, **sched):
    from neurips18_hierchical_image_manipulation_amd import config
    with config.schedule(**sched):
        m = build(flags, tmp, ema_decay=decay)
        out = dict(model=m, losses=[], start=m.optimizer_G.arena.data.clone(), trail=[])
        for s in range(steps):
            ld = m.optimize_parameters(batch(s, flags, color, h, w))
            out['losses'].append([float(ld[k]) for k in NAMES])
            if record:
                m.sync()
                out['trail'].append(m.optimizer_G.arena.data.double().cpu())
        out.update(state(m))
    return out


@functools.lru_cache(None)
def five(decay=DECAY, sched='default'):
    from neurips18_hierchical_image_manipulation_amd import config
    kw = dict(default={}, serial=config.SERIAL, chunked=dict(adam_chunked=True), unsplit=dict(adam_split_stem=False))[sched]
    return run(decay, 5, record=(sched == 'default' and decay > 0), **kw)


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_ema_off_allocates_nothing():
    off = five(0.0)
    assert off['model'].optimizer_G.ema is None and off['ema'] is None


def test_ema_on_changes_no_trajectory():
    on, off = five(), five(0.0)
    assert on['losses'] == off['losses']
    assert same(on['params'], off['params']), 'a generator / discriminator parameter differs with the EMA on'
    assert same(on['moments'], off['moments']), 'an Adam moment differs with the EMA on'
    assert not torch.equal(on['ema'], on['arena']) and not torch.equal(on['ema'], on['start'])


@pytest.mark.parametrize('sched', ['serial', 'chunked', 'unsplit'])
def test_each_element_is_averaged_exactly_once_per_step(sched):
    """default: Adam split around the stem (begin_step / step_range / step); serial: one step(); chunked: the local reducer
    attached, Adam bucket by bucket; unsplit: one deferred step()."""
    a, b = five(), five(DECAY, sched)
    if sched == 'chunked':
        assert b['model'].reducer_G is not None
    assert same(a['params'], b['params'])
    assert torch.equal(a['ema'], b['ema']), 'EMA buffers differ between the default schedule and %s' % sched
    assert a['model'].optimizer_G.ema_updates == b['model'].optimizer_G.ema_updates == 5


def test_buffer_follows_the_schedule_rule_in_float64():
    from neurips18_hierchical_image_manipulation_amd.optim import ema_decay_at
    r = five()
    ref = r['start'].double().cpu()
    scale = float(ref.abs().max())
    for t, p in enumerate(r['trail']):
        w = torch.tensor(1.0 - ema_decay_at(DECAY, t), dtype=torch.float64).float().double()
        assert float(w) == pytest.approx(1.0 - (1.0 + t) / (10.0 + t), rel=1e-6)       # the ramp, not 0.999
        ref = ref + w * (p - ref)
        scale = max(scale, float(p.abs().max()))
    err = float((r['ema'].double().cpu() - ref).abs().max())
    bound = 5 * 3 * EPS * scale
    print('5 steps: max error %.3e, bound %.3e' % (err, bound))
    assert err <= bound, (err, bound)


def _infer(model, s=9):
    b = batch(s)
    out = model.inference(b['label'], b['inst'], b['image'], b['mask_in'], b['mask_out']).clone()
    torch.cuda.synchronize()
    return out


def test_checkpoint_context_test_time_load_and_continue_train(tmp_path):
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    from neurips18_hierchical_image_manipulation_amd.util.metrics import evaluate_mask2image
    straight = run(DECAY, 6, tmp=tmp_path / 'straight')
    a = run(DECAY, 5, tmp=tmp_path)
    m = a['model']
    m.save('latest')
    d = tmp_path / 't'
    live, avg = torch.load(str(d / 'latest_net_G.pth')), torch.load(str(d / 'latest_net_G_ema.pth'))
    assert list(live) == list(avg) == list(m.netG.state_dict())
    assert all(live[k].shape == avg[k].shape and live[k].dtype == avg[k].dtype for k in live)
    assert any(not torch.equal(live[k], avg[k]) for k in live)
    # inside the context: inference, visuals and the metrics run on the averaged weights
    outside = _infer(m)
    with m.ema_weights():
        inside = _infer(m)
        assert set(m.get_current_visuals()) == {'input_label', 'input_image', 'real_image', 'synthesized_image'}
        assert evaluate_mask2image(m, [{k: v[:1] for k, v in batch(9).items()}], 1) is not None
        for step in (lambda: m.optimize_parameters(batch(5)), m.backward_G, m.optimizer_G.step):
            with pytest.raises(RuntimeError):
                step()
    assert not torch.equal(inside, outside)
    assert torch.equal(_infer(m), outside)
    with pytest.raises(KeyError):            # the live weights come back when the body raises
        with m.ema_weights():
            raise KeyError('body')
    assert same(state(m)['params'], a['params']) and torch.equal(m.optimizer_G.ema, a['ema'])
    # test time: --use_ema loads the averaged file; a missing one is an error
    test_flags = dict(TINY, gpu_ids=[0], isTrain=False, checkpoints_dir=str(tmp_path), name='t')
    t = create_model(dict(test_flags, use_ema=True))
    assert torch.equal(_infer(t), inside)
    assert torch.equal(_infer(create_model(dict(test_flags))), outside)
    with pytest.raises(RuntimeError):
        create_model(dict(test_flags, use_ema=True, which_epoch='12'))
    # --continue_train: buffer and update count come back (Adam's own state travels as the torch-layout state dicts)
    c = create_model(dict(TINY, gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp_path), name='t', ema_decay=DECAY,
                          continue_train=True))
    assert torch.equal(c.optimizer_G.ema, a['ema']) and c.optimizer_G.ema_updates == 5
    c.optimizer_G.load_state_dict(m.optimizer_G.state_dict())
    c.optimizer_D.load_state_dict(m.optimizer_D.state_dict())
    # the sixth step: after the context (a), after the reload (c), and never interrupted (straight)
    la, lc = m.optimize_parameters(batch(5)), c.optimize_parameters(batch(5))
    sa, sc = state(m), state(c)
    assert [float(la[k]) for k in NAMES] == [float(lc[k]) for k in NAMES] == straight['losses'][5]
    for s in (sa, sc):
        assert same(s['params'], straight['params']), 'the cached weight panels were not rebuilt from the live weights'
        assert torch.equal(s['ema'], straight['ema'])
    # without the file the average starts from the loaded weights
    m.delete_model('latest')
    assert not (d / 'latest_net_G_ema.pth').exists() and not (d / 'latest_net_G.pth').exists()


def test_continue_train_without_the_file_starts_from_the_loaded_weights(tmp_path, capsys):
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    m = run(0.0, 1, tmp=tmp_path)['model']
    m.save('latest')
    c = create_model(dict(TINY, gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp_path), name='t', ema_decay=DECAY,
                          continue_train=True))
    assert 'latest_net_G_ema.pth not found' in capsys.readouterr().out
    assert torch.equal(c.optimizer_G.ema, c.optimizer_G.arena.data) and c.optimizer_G.ema_updates == 0


def test_batchnorm_statistics_in_the_ema_file_are_the_live_ones(tmp_path):
    flags = dict(TINY, norm='batch')
    m = run(DECAY, 2, tmp=tmp_path, flags=flags)['model']
    m.save('latest')
    live, avg = torch.load(str(tmp_path / 't' / 'latest_net_G.pth')), torch.load(str(tmp_path / 't' / 'latest_net_G_ema.pth'))
    params = {k for k, _ in m.netG.named_parameters()}
    stats = [k for k in live if k not in params]
    assert any(k.endswith('running_mean') for k in stats)
    assert list(live) == list(avg) and all(torch.equal(live[k], avg[k]) and live[k].dtype == avg[k].dtype for k in stats)
    assert any(not torch.equal(live[k], avg[k]) for k in params)


def test_frozen_parameters_and_update_fixed_params(tmp_path):
    flags = dict(model='pix2pixHD_condImg', netG='local', ngf=8, ndf=8, n_downsample_global=2, n_blocks_global=2,
                 n_local_enhancers=1, n_blocks_local=2, num_D=2, label_nc=35, no_instance=True, niter_fix_global=3)
    m = run(DECAY, 2, tmp=tmp_path, flags=flags, h=64, w=64)['model']
    o = m.optimizer_G
    moved = 0
    for (k, p), off in zip(m.netG.named_parameters(), o.arena.offsets):
        avg = o.ema[off:off + p.numel()].view(p.shape)
        if k.startswith('model1'):
            moved += int(not torch.equal(avg, p.detach()))
        else:
            assert torch.equal(avg, p.detach()), 'frozen parameter %s: its average left it' % k
    assert moved > 0
    buf, count = o.ema, o.ema_updates
    m.update_fixed_params()
    assert m.optimizer_G is not o and m.optimizer_G.ema is buf and m.optimizer_G.ema_updates == count == 2
    assert m.optimizer_G.ema_decay == DECAY
    m.optimize_parameters(batch(2, flags, h=64, w=64))
    m.sync()
    assert m.optimizer_G.ema_updates == 3


def test_colour_two_stream_model():
    g = load_golden('tiny_color')
    flags = json.loads(str(g['flags']))
    kw = dict(flags=flags, color=True, h=int(g['H']), w=int(g['W']), tmp='/tmp/him_test_ema_color')
    on, off = run(DECAY, 3, **kw), run(0.0, 3, **kw)
    assert on['losses'] == off['losses'] and same(on['params'], off['params']) and same(on['moments'], off['moments'])
    assert on['model'].optimizer_G.ema_updates == 3 and not torch.equal(on['ema'], on['arena'])
    from neurips18_hierchical_image_manipulation_amd import config
    serial = run(DECAY, 3, **dict(kw, **config.SERIAL))
    assert torch.equal(on['ema'], serial['ema'])


# ---- box2mask ---------------------------------------------------------------------------------------------------------
def _b2m(tmp, **extra):
    from neurips18_hierchical_image_manipulation_amd import synth
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    g = load_golden('box2mask_traj')
    fl = dict(json.loads(str(g['flags'])), **extra)
    model = create_model(dict(fl, model='AE_maskgen_twostream', gpu_ids=[0], checkpoints_dir=str(tmp), name='b'))
    return g, fl, model, synth


def _b2m_run(tmp, decay, steps=5):
    g, fl, model, synth = _b2m(tmp, isTrain=True, ema_decay=decay)
    model.netG.load_state_dict(synth.init_state_dict(model.netG.state_dict(), 21))
    model.netD.load_state_dict(synth.init_state_dict(model.netD.state_dict(), 22))
    model.optimizer.reset_ema()
    start = model.optimizer.arena.data.double().cpu()
    losses, trail = [], []
    for s in range(steps):
        b = synth.make_box2mask_batch(s, 0, int(g['B']), int(g['H']), int(g['W']), 35)
        out, _ = model.forward(b['label'], None, b['mask_ctx_in'], None, b['mask_out'], b['mask_obj_inst'], b['cls'],
                               b['mask_in'], eval_mode=False)
        losses.append([float(x.detach().reshape(-1)[0]) if torch.is_tensor(x) else float(x) for x in out])
        torch.cuda.synchronize()
        trail.append(model.optimizer.arena.data.double().cpu())
    o, oD = model.optimizer, model.optimizer_D
    return dict(model=model, losses=losses, start=start, trail=trail, g=g, synth=synth,
                tensors=[t.clone() for t in (o.arena.data, o.exp_avg, o.exp_avg_sq, oD.arena.data, oD.exp_avg, oD.exp_avg_sq)],
                ema=None if o.ema is None else o.ema.clone())


def _b2m_eval(model, g, synth):
    b = synth.make_box2mask_batch(9, 0, int(g['B']), int(g['H']), int(g['W']), 35)
    out = model.forward(b['label'], None, b['mask_ctx_in'], None, b['mask_out'], b['mask_obj_inst'], b['cls'], b['mask_in'],
                        eval_mode=True)
    torch.cuda.synchronize()
    return out['obj_pred_label'].clone()


def test_box2mask_trajectory_average_and_test_time_load(tmp_path):
    from neurips18_hierchical_image_manipulation_amd.optim import ema_decay_at
    on, off = _b2m_run(tmp_path, DECAY), _b2m_run(tmp_path / 'off', 0.0)
    assert off['ema'] is None and on['losses'] == off['losses'] and same(on['tensors'], off['tensors'])
    # every element once per step: the buffer is the float64 recursion over the recorded parameters
    ref, scale = on['start'], float(on['start'].abs().max())
    for t, p in enumerate(on['trail']):
        w = torch.tensor(1.0 - ema_decay_at(DECAY, t), dtype=torch.float64).float().double()
        ref = ref + w * (p - ref)
        scale = max(scale, float(p.abs().max()))
    err = float((on['ema'].double().cpu() - ref).abs().max())
    assert err <= 5 * 3 * EPS * scale, (err, 5 * 3 * EPS * scale)
    m, g, synth = on['model'], on['g'], on['synth']
    m.save('latest')
    d = tmp_path / 'b'
    live, avg = torch.load(str(d / 'latest_net_G.pth')), torch.load(str(d / 'latest_net_G_ema.pth'))
    assert list(live) == list(avg) and list(live['network']) == list(avg['network'])
    for k in live['network']:
        assert list(live['network'][k]) == list(avg['network'][k])
        assert all(live['network'][k][n].shape == avg['network'][k][n].shape and
                   live['network'][k][n].dtype == avg['network'][k][n].dtype for n in live['network'][k])
    outside = _b2m_eval(m, g, synth)
    with m.ema_weights():
        inside = _b2m_eval(m, g, synth)
        with pytest.raises(RuntimeError):
            m.optimizer.step()
    assert not torch.equal(inside, outside) and torch.equal(_b2m_eval(m, g, synth), outside)
    assert torch.equal(_b2m_eval(_b2m(tmp_path, isTrain=False, use_ema=True)[2], g, synth), inside)
    assert torch.equal(_b2m_eval(_b2m(tmp_path, isTrain=False)[2], g, synth), outside)
    m.delete_model('latest')
    assert not os.path.exists(str(d / 'latest_net_G_ema.pth'))
    with pytest.raises(AssertionError):
        _b2m(tmp_path, isTrain=False, use_ema=True)
