"""-m gpu: the boundary-weighted and surface losses through ``ops`` and autograd, ``MaskReconLoss`` and one
``TwoStreamAE_mask`` step, against the float64 restatement of tests/boundary_loss_fixture.py under the bound of
abi_harness (max(8 * e32, 16 * 2^-24), e32 the fp32 restatement's own error)."""
import json
import os

import pytest
import torch

import abi_harness as ah
import boundary_loss_fixture as fx
from boundary_loss_fixture import F32, F64
from test_model_gpu import OUT as REPORT_DIR
from util import load_golden

pytestmark = pytest.mark.gpu
LOG = ah.RowLog(os.path.join(REPORT_DIR, 'boundary_loss_ops_rows.jsonl'))
G = 0.75
B, C, H, W = 3, 5, 17, 33
A, S = 4.0, 1.0


def _ops():
    from neurips18_hierchical_image_manipulation_amd import ops
    return ops


def _nll_inputs():
    return (fx.logp_planes(B, C, H, W), fx.label_plane('ignore', B, C, H, W), fx.mask_plane('ignore', B, H, W),
            fx.cached_d2('label', 'ignore', B, C, H, W))


def _pair_inputs():
    return fx.prob_plane(B, H, W), fx.object_plane('object', B, H, W), fx.cached_d2('object', 'object', B, 2, H, W)


def _grad(loss, leaf):
    (loss * G).backward()
    return leaf.grad.detach().cpu()


def test_ops_forward_and_backward_match_the_fixture_through_autograd():
    ops = _ops()
    ck = ah.Checks('ops', LOG)
    logp, label, mask, d2 = _nll_inputs()
    x = logp.cuda().requires_grad_(True)
    loss = ops.boundary_weighted_nll(x, label.cuda(), mask.cuda(), A, S)
    r64, r32 = (fx.bw_nll(logp, label, mask, d2, A, S, dt, g=G) for dt in (F64, F32))
    ck.row('nll', loss, r64['loss'], r32['loss'])
    ck.row('nll dlogp', _grad(loss, x), r64['dlogp'], r32['dlogp'])
    p, t, od2 = _pair_inputs()
    for kind, fn in (('bce', ops.boundary_weighted_bce), ('l1', ops.boundary_weighted_l1)):
        x = p.cuda().requires_grad_(True)
        loss = fn(x, t.cuda(), A, S)
        r64, r32 = (fx.bw_pair(p, t, od2, A, S, kind, dt, g=G) for dt in (F64, F32))
        ck.row(kind, loss, r64['loss'], r32['loss'])
        ck.row(kind + ' dp', _grad(loss, x), r64['dp'], r32['dp'])
    fg, bg = fx.cached_d2('surface', 'object', B, 2, H, W)
    x = p.cuda().requires_grad_(True)
    loss = ops.surface_loss(x, t.cuda())
    r64, r32 = (fx.surface(p, t, fg, bg, dt, g=G) for dt in (F64, F32))
    ck.row('surface', loss, r64['loss'], r32['loss'])
    ck.row('surface dp', _grad(loss, x), r64['dp'], r32['dp'])
    ck.done()


def test_the_transforms_of_ops_equal_the_fixture():
    ops = _ops()
    _, label, _, d2 = _nll_inputs()
    _, t, od2 = _pair_inputs()
    fg, bg = fx.cached_d2('surface', 'object', B, 2, H, W)
    assert torch.equal(ops.boundary_dist2(label.cuda()).cpu(), torch.from_numpy(d2))
    assert torch.equal(ops.boundary_dist2(t.cuda()).cpu(), torch.from_numpy(od2))
    got = ops.surface_dists(t.cuda())
    assert torch.equal(got[0].cpu(), torch.from_numpy(fg)) and torch.equal(got[1].cpu(), torch.from_numpy(bg))


def test_passed_in_distances_and_the_internal_ones_give_equal_results():
    ops = _ops()
    logp, label, mask, _ = _nll_inputs()
    p, t, _ = _pair_inputs()
    label, mask, t = label.cuda(), mask.cuda(), t.cuda()

    def both(fn, leaf, *rest, **kw):
        out = []
        for extra in ({}, kw):
            x = leaf.cuda().requires_grad_(True)
            loss = fn(x, *rest, **extra)
            out.append((loss.detach().clone(), _grad(loss, x)))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), fn.__name__

    both(lambda x, **k: ops.boundary_weighted_nll(x, label, mask, A, S, **k), logp, dist2=ops.boundary_dist2(label))
    od2 = ops.boundary_dist2(t)
    both(lambda x, **k: ops.boundary_weighted_bce(x, t, A, S, **k), p, dist2=od2)
    both(lambda x, **k: ops.boundary_weighted_l1(x, t, A, S, **k), p, dist2=od2)
    both(lambda x, **k: ops.surface_loss(x, t, **k), p, dists=ops.surface_dists(t))


def test_a_side_stream_gives_the_same_bits():
    ops = _ops()
    logp, label, mask, _ = _nll_inputs()
    p, t, _ = _pair_inputs()
    label, mask, t = label.cuda(), mask.cuda(), t.cuda()

    def run():
        x, q = logp.cuda().requires_grad_(True), p.cuda().requires_grad_(True)
        total = ops.boundary_weighted_nll(x, label, mask, A, S) + ops.boundary_weighted_bce(q, t, A, S) \
            + ops.boundary_weighted_l1(q, t, A, S) + ops.surface_loss(q, t)
        total.backward()
        return total.detach(), x.grad, q.grad

    main = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = run()
    side.synchronize()
    for a, b in zip(main, other):
        assert torch.equal(a, b)


def test_shape_and_dtype_refusals_on_device_tensors():
    ops = _ops()
    p, t, _ = _pair_inputs()
    p, t = p.cuda(), t.cuda()
    with pytest.raises(ValueError):
        ops.boundary_weighted_bce(p, t[:, :, :-1], A, S)
    with pytest.raises(ValueError):
        ops.boundary_weighted_l1(p, t, A, S, dist2=torch.zeros(B, H, W, device='cuda'))          # not int32
    with pytest.raises(ValueError):
        ops.boundary_weighted_bce(p, t, A, S, dist2=torch.zeros(B, H + 1, W, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        ops.surface_loss(p, t, dists=(torch.zeros(B, H, W, dtype=torch.int32, device='cuda'),))
    with pytest.raises(ValueError):
        ops.boundary_weighted_nll(p, t, t.double(), A, S)
    with pytest.raises(ValueError):
        ops.boundary_weighted_bce(p, t, -1.0, S)


def test_mask_recon_loss_with_weight_zero_is_masked_nll_and_with_a_weight_the_weighted_form():
    ops = _ops()
    from neurips18_hierchical_image_manipulation_amd.models.mask_losses import MaskReconLoss
    logp, label, mask, _ = _nll_inputs()
    logp, label, mask = logp.cuda(), label.cuda(), mask.cuda()
    for lab in (label, label[:, 0].long()):
        assert torch.equal(MaskReconLoss()(logp, lab, mask), ops.masked_nll(logp, label, mask))
        assert torch.equal(MaskReconLoss(True, 0.0, 2.0)(logp, lab, mask), ops.masked_nll(logp, label, mask))
        assert torch.equal(MaskReconLoss(True, A, S)(logp, lab, mask), ops.boundary_weighted_nll(logp, label, mask, A, S))
    assert torch.equal(ops.boundary_weighted_nll(logp, label, mask, 0.0, 5.0), ops.boundary_weighted_nll(logp, label, mask, 0.0, 1.0))


# ------------------------------------------------------------------------------------------------- the training step
def _model(tmp, **kw):
    from neurips18_hierchical_image_manipulation_amd import synth
    from neurips18_hierchical_image_manipulation_amd.models import create_model
    g = load_golden('box2mask_traj')
    fl = dict(json.loads(str(g['flags'])), isTrain=True, **kw)
    model = create_model(dict(fl, model='AE_maskgen_twostream', gpu_ids=[0], checkpoints_dir=str(tmp), name='b'))
    model.netG.load_state_dict(synth.init_state_dict(model.netG.state_dict(), 21))
    model.netD.load_state_dict(synth.init_state_dict(model.netD.state_dict(), 22))
    batch = synth.make_box2mask_batch(0, 0, int(g['B']), int(g['H']), int(g['W']), 35)
    return model, batch


def _step(model, b):
    return model.forward(b['label'], None, b['mask_ctx_in'], None, b['mask_out'], b['mask_obj_inst'], b['cls'], b['mask_in'],
                         eval_mode=False)


def test_a_step_with_the_settings_at_zero_is_the_step_without_them(tmp_path, monkeypatch):
    ops = _ops()
    calls = []
    for name in ('boundary_weighted_nll', 'boundary_weighted_bce', 'boundary_weighted_l1', 'surface_loss',
                 'distance_transform'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    plain, batch = _model(tmp_path / 'p')
    zero, _ = _model(tmp_path / 'z', boundary_weight=0.0, boundary_sigma=5.0, surface_weight=0.0)
    assert (zero.boundary_weight, zero.boundary_sigma, zero.surface_weight) == (0.0, 5.0, 0.0)
    assert (plain.boundary_weight, plain.boundary_sigma, plain.surface_weight) == (0.0, 5.0, 0.0)
    out = []
    for m in (plain, zero):
        losses, labels = _step(m, batch)
        torch.cuda.synchronize()
        out.append(([x.clone() if torch.is_tensor(x) else x for x in losses], [x.clone() for x in labels],
                    m.optimizer.arena.grad.clone(), m.optimizer.arena.data.clone(), m.optimizer_D.arena.data.clone()))
        assert m.loss_surface is None
    assert not calls, calls
    (l0, y0, g0, w0, d0), (l1, y1, g1, w1, d1) = out
    assert len(l0) == len(l1) == 6
    for a, b in zip(l0, l1):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    assert all(torch.equal(a, b) for a, b in zip(y0, y1))
    assert torch.equal(g0, g1) and torch.equal(w0, w1) and torch.equal(d0, d1)


@pytest.mark.parametrize('kind', ['bce', 'l1'])
def test_a_step_with_the_settings_set_gives_the_fixtures_losses(tmp_path, kind):
    from neurips18_hierchical_image_manipulation_amd.models.TwoStreamAE_mask import TwoStreamAE_mask
    model, b = _model(tmp_path, boundary_weight=A, boundary_sigma=2.0, surface_weight=0.5, objReconLoss=kind)
    assert (model.boundary_weight, model.boundary_sigma, model.surface_weight) == (A, 2.0, 0.5)
    over = TwoStreamAE_mask(model.opt, boundary_weight=1.0, surface_weight=0.25)      # keywords win over opt
    assert (over.boundary_weight, over.boundary_sigma, over.surface_weight) == (1.0, 2.0, 0.25)
    with pytest.raises(TypeError):
        TwoStreamAE_mask(model.opt, boundary=1.0)
    with pytest.raises(ValueError):
        TwoStreamAE_mask(model.opt, boundary_sigma=0.0)
    before = model.optimizer.arena.data.clone()
    with torch.no_grad():                      # training-mode BatchNorm: the batch alone decides these probabilities
        model.netG.train(True)
        _, comb, _, obj = model.netG(model.encode_cond(b['mask_ctx_in'], b['mask_in'], b['cls']))
        comb, obj = comb.cpu(), obj.cpu()
    losses, labels = _step(model, b)
    torch.cuda.synchronize()
    assert len(losses) == 6 and losses[2] == 0 and len(labels) == 2
    assert all(torch.is_tensor(x) and x.numel() == 1 for i, x in enumerate(losses) if i != 2)
    assert torch.is_tensor(model.loss_surface) and not model.loss_surface.requires_grad
    assert not torch.equal(model.optimizer.arena.data, before) and bool(torch.isfinite(model.optimizer.arena.data).all())
    args = (comb, obj, b['label'].float(), b['mask_out'].float(), b['mask_obj_inst'].float(), A, 2.0, kind)
    assert model.use_output_gate                # the object and surface terms see the GATED probability
    r64, r32 = fx.trainer_terms(*args, dtype=F64), fx.trainer_terms(*args, dtype=F32)
    ck = ah.Checks('step|' + kind, LOG)
    ck.row('comb', losses[0], r64['comb'], r32['comb'])
    ck.row('obj', losses[1], r64['obj'], r32['obj'])
    ck.row('surface', model.loss_surface, r64['surface'], r32['surface'])
    ck.done()
    ungated = fx.trainer_terms(*args, dtype=F64, use_gate=False)
    assert abs(float(ungated['obj']) - float(r64['obj'])) > 1e-3 * abs(float(r64['obj']))
