"""-m gpu: the seamless composite through the Python layers -- ops.membrane_basis / ops.membrane_solve /
ops.canvas_paste_seamless, util.data_util.paste_canvas_seamless, JointInference.gen_image_seamless and the ``seamless``
keyword of the object edits -- against tests/seamless_fixture.py under the rule of tests/test_seamless_abi_gpu.py; the
unset keyword is today's path bit for bit; the constant-offset property on device results; a side stream; a seamless
removal on the tiny models of tests/joint_fixture.py."""
import numpy as np
import pytest
import torch

import composite_fixture as cf
import seamless_fixture as fx
from neurips18_hierchical_image_manipulation_amd import ops
from neurips18_hierchical_image_manipulation_amd.util import data_util
from test_composite_gpu import _labels, _no_sync, _paste_case
from test_layout_edit_gpu import CLS, FEATHER, REACH, _canvas, _near, _oracle_erase, _seed, scene  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _check(m, canvas, matte, photo, P, x0, y0, case, **opts):
    rows = []
    bad = fx.compare(m.cpu().numpy()[0], canvas.cpu().numpy()[0], None if matte is None else matte.cpu().numpy(),
                     photo[0], P, x0, y0, rows=rows, case=case, **opts)
    for r in rows:
        print(r)
    assert not bad, '; '.join(bad)


# (Hc, Wc, x0, y0, H, W), patch box, feather, reach, profile, with labels
OPS_CASES = [((40, 100, 13, 5, 29, 73), (3, 2, 30, 21), None, 0, 'smooth', False),
             ((40, 100, 0, 11, 29, 73), (0, 0, 32, 32), 5, 0, 'linear', True),          # the left side on the canvas edge
             ((80, 300, 9, 6, 67, 261), (2, 0, 28, 32), 6, 0, 'smooth', False)]         # the largest plane: 65 x 259 inside


@pytest.mark.parametrize('case', OPS_CASES, ids=lambda c: 'x'.join(map(str, c[0])))
def test_ops_chain_against_the_fixture(case):
    (Hc, Wc, x0, y0, H, W), box, feather, reach, profile, with_labels = case
    g = np.random.default_rng(H * W)
    photo = g.random((1, 3, Hc, Wc), dtype=np.float32)
    patch = g.random((1, 3, 32, 32), dtype=np.float32)
    ph, pt = torch.from_numpy(photo).to(DEV), torch.from_numpy(patch).to(DEV)
    P = ops.canvas_paste_bicubic(pt, box, ph.clone(), x0, y0, H, W).cpu().numpy()[0, :, y0:y0 + H, x0:x0 + W]
    dist2 = want_d2 = None
    if with_labels:
        before, after = _labels(Hc, Wc, x0, y0, H, W, 3)
        changed = ops.canvas_changed(torch.from_numpy(before).to(DEV), torch.from_numpy(after).to(DEV), x0, y0, H, W)
        dist2 = ops.distance_transform(changed, rule='nonzero')[0]
        want_d2 = cf.dist2_of(cf.changed(before[0, 0], after[0, 0], x0, y0, H, W))
    l, r, t, b, ny, nx = ops.membrane_sides(Hc, Wc, x0, y0, H, W)
    ops.membrane_basis(ny, t, b), ops.membrane_basis(nx, l, r)       # built once; the chain below finds them cached
    Pd = torch.from_numpy(P).to(DEV)[None]
    torch.cuda.synchronize()
    with _no_sync():
        m, status = ops.membrane_solve(ph, x0, y0, Pd)
        canvas, matte, status2 = ops.canvas_paste_seamless(pt, box, ph.clone(), x0, y0, H, W, 0, feather=feather,
                                                           reach=reach, dist2=dist2, profile=profile,
                                                           want_matte=feather is not None)
    assert status.tolist() == status2.tolist() == [fx.sides_mask((l, r, t, b)), ny, nx, 0]
    assert tuple(m.shape) == (1, 3, H, W) and m.dtype == torch.float32
    assert ops.membrane_basis(ny, t, b)[0] is ops.membrane_basis(ny, t, b)[0]               # cached per (n, lo, hi, device)
    _check(m, canvas, None if matte is None else matte[0, 0], photo, P, x0, y0, 'ops', feather=feather, reach=reach,
           dist2=want_d2, profile=cf.PROFILES[profile])


def test_paste_canvas_seamless_against_the_fixture_and_on_a_side_stream():
    photo, patch, info, (Hc, Wc, x0, y0, H, W) = _paste_case()
    before, after = _labels(Hc, Wc, x0, y0, H, W, 8)
    ph, pt = torch.from_numpy(photo).to(DEV), torch.from_numpy(patch).to(DEV)
    lb, la = torch.from_numpy(before).to(DEV), torch.from_numpy(after).to(DEV)
    keep = ph.clone()
    from PIL import Image
    hard = data_util.paste_canvas(ph, (pt + 1) / 2, info, method=Image.BICUBIC, is_img=True)
    P = hard.cpu().numpy()[0, :, y0:y0 + H, x0:x0 + W]
    m, _ = ops.membrane_solve(ph, x0, y0, hard[:, :, y0:y0 + H, x0:x0 + W].contiguous())
    whole = data_util.paste_canvas_seamless(ph, (pt + 1) / 2, info)
    assert info['membrane'].tolist() == [15, H - 2, W - 2, 0]
    both, matte = data_util.paste_canvas_seamless(ph, (pt + 1) / 2, info, feather=7, reach=3, label_before=lb,
                                                  label_after=la, want_matte=True)
    folded = data_util._paste_image_seamless(ph, pt, info, 2, feather=7, reach=3, label_before=lb, label_after=la)
    assert torch.equal(ph, keep) and torch.equal(folded, both)       # the input canvas is cloned, never written
    d2 = cf.dist2_of(cf.changed(before[0, 0], after[0, 0], x0, y0, H, W))
    _check(m, whole, None, photo, P, x0, y0, 'paste alpha 1')
    _check(m, both, matte[0, 0], photo, P, x0, y0, 'paste border and object', feather=7, reach=3, dist2=d2)
    _, want_matte = data_util.paste_canvas_feathered(ph, (pt + 1) / 2, info, feather=7, reach=3, label_before=lb,
                                                     label_after=la, want_matte=True)
    assert torch.equal(matte, want_matte)                            # the matte of the feathered paste, bit for bit
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        half = (pt + 1) / 2
        with _no_sync():
            got, got_m = data_util.paste_canvas_seamless(ph, half, info, feather=7, reach=3, label_before=lb,
                                                         label_after=la, want_matte=True)
    side.synchronize()
    assert torch.equal(got, both) and torch.equal(got_m, matte)


def test_constant_offset_gives_the_photograph_back():
    """A patch that IS the photograph plus 0.25 (values chosen so that the sum is exact in fp32): the membrane is -0.25
    and the seamless paste returns the photograph."""
    Hc, Wc, x0, y0, H, W = 48, 100, 9, 6, 30, 71
    g = np.random.default_rng(1)
    photo = (g.integers(0, 128, size=(1, 3, Hc, Wc)) / np.float32(256)).astype(np.float32)
    ph = torch.from_numpy(photo).to(DEV)
    P = (ph[:, :, y0:y0 + H, x0:x0 + W] + 0.25).contiguous()
    m, _ = ops.membrane_solve(ph, x0, y0, P)
    assert float((m + 0.25).abs().max()) <= 2.0 ** -23 * 0.25
    out, _ = ops.canvas_seamless_apply(P, m, ph.clone(), x0, y0)
    assert float((out - ph).abs().max()) <= 4 * 2.0 ** -24


def test_unset_seamless_is_todays_path_bit_for_bit(scene):  # noqa: F811
    s, ji = scene, scene['ji']
    x0, y0, x1, y1 = s['bbox']
    dst = [x0 + 150, y0 + 40, x0 + 150 + (x1 - x0), y0 + 40 + (y1 - y0)]
    for edit, args in ((ji.remove_object, ()), (ji.move_object, (dst,))):
        results = []
        for kw in ({}, dict(seamless=False)):
            _seed(5)
            results.append(edit(s['obj'], *args, s['lab'], s['ins'], s['ph'], ji.opt_imggen, feather=FEATHER, reach=REACH,
                                **kw))
        for a, b in zip(results[0][:3], results[1][:3]):
            assert torch.equal(a, b)
        for pa, pb in zip(results[0][4]['passes'], results[1][4]['passes']):
            assert 'membrane' not in pa and 'membrane' not in pb and torch.equal(pa['matte'], pb['matte'])
        _seed(5)
        want, _, _ = ji.gen_image_feathered({'bbox': s['bbox'], 'cls': CLS}, s['ph'], results[0][0], ji.opt_imggen,
                                            feather=FEATHER, reach=REACH, label_before=s['lab'])
        if edit == ji.remove_object:
            assert torch.equal(results[0][2], want)


def test_remove_object_seamless(scene):  # noqa: F811
    s, ji = scene, scene['ji']
    want_label = _oracle_erase(s)[0]
    _seed(5)
    _, _, feathered, _, _ = ji.remove_object(s['obj'], s['lab'], s['ins'], s['ph'], ji.opt_imggen, feather=4, reach=2)
    _seed(5)
    label_c, _, img_c, _, report = ji.remove_object(s['obj'], s['lab'], s['ins'], s['ph'], ji.opt_imggen, seamless=True,
                                                    feather=4, reach=2)
    assert np.array_equal(label_c.cpu().numpy()[0, 0], want_label.astype(np.float32))
    d = report['passes'][0]
    status = d['membrane'].tolist()
    matte = d['matte']
    H, W = matte.shape[2:]
    assert status[0] == 15 and status[1:] == [H - 2, W - 2, 0]
    got, photo = img_c.cpu().numpy(), s['photo']
    far = ~_near(want_label != s['label'][0, 0], 2 + 4)
    assert far.any() and np.array_equal(got.view(np.uint32)[0][:, far], photo.view(np.uint32)[0][:, far])
    assert (got != photo).any() and not torch.equal(img_c, feathered)
    assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
    assert torch.equal(s['ph'].cpu(), torch.from_numpy(photo))       # the input canvas is never written
    _seed(5)
    hand, d2, _ = ji.gen_image_seamless({'bbox': s['bbox'], 'cls': CLS}, s['ph'], _canvas(want_label, label_c),
                                        ji.opt_imggen, feather=4, reach=2, label_before=s['lab'])
    assert torch.equal(hand, img_c) and torch.equal(d2['matte'], matte)
    with pytest.raises(ValueError):
        ji.remove_object(s['obj'], s['lab'], s['ins'], s['ph'], ji.opt_imggen, seamless=1)
