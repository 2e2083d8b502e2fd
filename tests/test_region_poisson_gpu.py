"""-m gpu: the region Poisson clone through ``ops`` (solve, apply, ``canvas_clone_region``) against
tests/region_poisson_fixture.py, on a side stream and without host synchronisation, and ``keep_appearance=True`` of
``JointInference.move_object`` / ``rescale_object`` on the tiny models of tests/joint_fixture.py; with the option unset the
edits are today's, bit for bit."""
import numpy as np
import pytest
import torch

import region_poisson_fixture as fx
from neurips18_hierchical_image_manipulation_amd import ops
from neurips18_hierchical_image_manipulation_amd.models.joint_inference_model import scaled_box
from test_composite_gpu import _no_sync
from test_layout_edit_gpu import CLS, FEATHER, OBJ, REACH, _canvas, _near, _oracle_move, _seed, scene  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _blob(x0=9, y0=7, seed=5):
    R = fx.blob_region()
    O, P = fx.scene(seed, 60, 80, 37, 53)
    return O, P, x0, y0, R


@pytest.mark.parametrize('mixed', [False, True])
def test_solve_and_apply_against_the_fixture(mixed):
    O, P, x0, y0, R = _blob()
    canvas = _dev(O)[None]
    u, status, resid = ops.region_poisson_solve(canvas, x0, y0, _dev(P)[None], _dev(R), mixed=mixed, rtol=1e-10)
    assert u.dtype == torch.float64 and tuple(u.shape) == (1, 3, 37, 53) and status.dtype == torch.int32
    assert torch.equal(canvas.cpu(), torch.from_numpy(O)[None])              # the solve does not write the canvas
    out = ops.region_poisson_apply(_dev(P)[None], u, _dev(R), canvas, x0, y0)
    assert out is canvas
    rows = []
    bad = fx.compare(u.cpu().numpy()[0], out.cpu().numpy()[0], status.tolist(), O, P, x0, y0, R, mixed, 1e-10, rows=rows,
                     case='ops mixed%d' % mixed)
    print(rows)
    assert not bad, '; '.join(bad)
    assert float(resid.max()) <= 1e-10 * (1 + 1e-12)
    loose = ops.region_poisson_solve(_dev(O)[None], x0, y0, _dev(P)[None], _dev(R), mixed=mixed)[1].tolist()
    assert 0 < loose[3] < status.tolist()[3] and loose[4] == 0                # the default rtol 1e-7 stops earlier


def _clone_case():
    """A 40 x 60 source box resized to 37 x 53 and cloned at a box that hangs 6 columns over the canvas's left edge."""
    g = np.random.default_rng(3)
    src = (g.integers(0, 256, size=(1, 3, 90, 120)) / np.float32(255)).astype(np.float32)
    O = (g.integers(0, 256, size=(1, 3, 60, 80)) / np.float32(255)).astype(np.float32)
    src_box, dst_box = (30, 20, 90, 60), (-6, 11, 47, 48)
    plane = np.zeros((60, 80), np.uint8)
    plane[11:48, 0:47] = fx.blob_region()[:, 6:]
    plane[3, 70] = 1                                                           # outside the window: never read
    return src, O, src_box, dst_box, plane


def test_canvas_clone_region_against_the_fixture_on_a_side_stream_without_synchronisation():
    src, O, src_box, dst_box, plane = _clone_case()
    s_dev, plane_dev = _dev(src), _dev(plane)
    P = ops.canvas_crop_bicubic(s_dev, src_box, 37, 53, normalize=False)[0, :, :, 6:].contiguous().cpu().numpy()
    canvas, status, resid = ops.canvas_clone_region(s_dev, src_box, _dev(O), dst_box, plane_dev)
    R = plane[11:48, 0:47]
    got = canvas.cpu().numpy()[0]
    bad = fx.compare(ops.region_poisson_solve(_dev(O), 0, 11, _dev(P)[None], _dev(R))[0].cpu().numpy()[0], got,
                     status.tolist(), O[0], P, 0, 11, R, False, 1e-7, case='clone')
    assert not bad, '; '.join(bad)
    assert status.tolist()[0] == 2 | 4 | 8 and (got != O[0]).any()           # the left side is the canvas edge
    mixed, _, _ = ops.canvas_clone_region(s_dev, src_box, _dev(O), dst_box, plane_dev, mixed=True)
    assert not torch.equal(mixed, canvas)
    side = torch.cuda.Stream()
    target, P_dev, R_dev = _dev(O), _dev(P)[None], plane_dev[11:48, 0:47].contiguous()
    spare = target.clone()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with _no_sync():
            again, st2, rs2 = ops.canvas_clone_region(s_dev, src_box, target, dst_box, plane_dev)
            u, _, _ = ops.region_poisson_solve(spare, 0, 11, P_dev, R_dev)
            ops.region_poisson_apply(P_dev, u, R_dev, spare, 0, 11)
    side.synchronize()
    assert torch.equal(again, canvas) and torch.equal(st2, status) and torch.equal(rs2, resid)   # the same bits
    assert torch.equal(spare, canvas)                                          # the two halves by hand are the whole


# ----------------------------------------------------------------------------------------- JointInference on tiny models
def _move(s, dst, seed, **kw):
    _seed(seed)
    return s['ji'].move_object(s['obj'], dst, s['lab'], s['ins'], s['ph'], s['ji'].opt_imggen, feather=FEATHER,
                               reach=REACH, **kw)


def _first_pass(s, dst, seed, photo=None):
    """The oracle's layout after the move and the canvas after the first repaint, done by hand."""
    e_status, want_label, want_inst, changed, p_status, _ = _oracle_move(s, dst)
    after = _canvas(want_label, s['lab'])
    _seed(seed)
    first, _, _ = s['ji'].gen_image_feathered({'bbox': s['bbox'], 'cls': CLS}, s['ph'] if photo is None else photo, after,
                                              s['ji'].opt_imggen, feather=FEATHER, reach=REACH, label_before=s['lab'])
    return want_label, changed, p_status, first


def _check_keep(s, dst, result, seed, mixed):
    label_c, _, img_c, _, report = result
    want_label, changed, p_status, first = _first_pass(s, dst, seed)
    assert np.array_equal(label_c.cpu().numpy()[0, 0], want_label.astype(np.float32)) and report['place'] == p_status
    x0, y0, x1, y1 = s['bbox']
    hand, status, resid = ops.canvas_clone_region(s['ph'], (x0, y0, x1 + 1, y1 + 1), first.clone(),
                                                  (dst[0], dst[1], dst[2] + 1, dst[3] + 1), _dev(changed), mixed=mixed)
    assert torch.equal(img_c, hand)                                            # the second pass IS the clone
    assert len(report['passes']) == 2 and sorted(report['passes'][1]) == ['clone', 'resid']
    clone = report['passes'][1]['clone']
    assert clone == status.tolist() and report['passes'][1]['resid'] == resid.tolist()
    assert clone[1] + clone[2] == p_status[0] and clone[1] > 0 and clone[4] == 0 and clone[3] > 0
    got, photo = img_c.cpu().numpy(), s['photo']
    placed = changed.astype(bool)
    assert (got[0][:, placed] != first.cpu().numpy()[0][:, placed]).any()      # the clone wrote the object's pixels ...
    keep = ~placed
    assert np.array_equal(got[0][:, keep], first.cpu().numpy()[0][:, keep])    # ... and nothing but them
    # outside both windows (the repaint's reach around the changed labels, and the pixels placed, whose label a shrunk
    # object leaves as it was): the photograph
    far = ~_near((want_label != s['label'][0, 0]) | placed, REACH + FEATHER)
    assert far.any() and np.array_equal(got.view(np.uint32)[0][:, far], photo.view(np.uint32)[0][:, far])
    assert torch.equal(s['ph'].cpu(), torch.from_numpy(photo))                 # the input canvas is never written


@pytest.mark.parametrize('mixed', [False, True])
def test_move_object_keeps_the_objects_own_pixels(scene, mixed):  # noqa: F811
    x0, y0, x1, y1 = scene['bbox']
    w, h = x1 - x0 + 1, y1 - y0 + 1
    dst = [x0 + 150, y0 + 40, x0 + 150 + int(w * 1.3) - 1, y0 + 40 + int(h * 0.8) - 1]
    _check_keep(scene, dst, _move(scene, dst, 9, keep_appearance=True, mixed=mixed), 9, mixed)


def test_rescale_object_keeps_the_objects_own_pixels(scene):  # noqa: F811
    s, ji = scene, scene['ji']
    dst = scaled_box(s['bbox'], 0.6)
    _seed(11)
    result = ji.rescale_object(s['obj'], 0.6, s['lab'], s['ins'], s['ph'], ji.opt_imggen, feather=FEATHER, reach=REACH,
                               keep_appearance=True)
    _check_keep(s, dst, result, 11, False)


def test_a_same_size_move_onto_the_same_pixels_returns_them(scene):  # noqa: F811
    """The photograph at the destination equals the source box (bytes / 255: the same-size crop returns them exactly), so
    P == O on the whole window, b == 0, u == 0 and no iteration runs: the canvas takes (float)(P + 0) = the source pixels.
    Bound: one fp32 rounding, 2^-24 (values in [0,1])."""
    s, ji = scene, scene['ji']
    x0, y0, x1, y1 = s['bbox']
    dst = [x0 + 300, y0, x1 + 300, y1]
    photo2 = s['ph'].clone()
    source = s['ph'][:, :, y0:y1 + 1, x0:x1 + 1]
    photo2[:, :, y0:y1 + 1, x0 + 300:x1 + 301] = source
    _seed(13)
    _, _, img_c, _, report = ji.move_object(s['obj'], dst, s['lab'], s['ins'], photo2, ji.opt_imggen, feather=FEATHER,
                                            reach=REACH, keep_appearance=True)
    _, changed, _, first = _first_pass(s, dst, 13, photo=photo2)
    window = (slice(None), slice(None), slice(y0, y1 + 1), slice(x0 + 300, x1 + 301))
    assert torch.equal(first[window], photo2[window]), 'the first repaint must not reach the destination'
    clone = report['passes'][1]['clone']
    assert clone[3] == 0 and clone[4] == 0 and report['passes'][1]['resid'] == [0.0, 0.0, 0.0]
    placed = torch.from_numpy(changed.astype(bool))[y0:y1 + 1, x0 + 300:x1 + 301]
    err = (img_c[window] - source).abs()[0][:, placed.to(DEV)]
    assert err.numel() > 1000 and float(err.max()) <= 2.0 ** -24


def test_unset_option_is_the_parents_path_bit_for_bit(scene):  # noqa: F811
    x0, y0, x1, y1 = scene['bbox']
    dst = [x0 + 150, y0 + 40, x0 + 150 + (x1 - x0), y0 + 40 + (y1 - y0)]
    plain, unset = _move(scene, dst, 5), _move(scene, dst, 5, keep_appearance=False, mixed=False)
    for a, b in zip(plain[:3], unset[:3]):
        assert torch.equal(a, b)
    # the parent's path by hand: two feathered repaints (tests/test_layout_edit_gpu.py::_check_move)
    want_label, _, p_status, first = _first_pass(scene, dst, 5)
    hand, _, _ = scene['ji'].gen_image_feathered({'bbox': p_status[2:6], 'cls': CLS}, first, _canvas(want_label, scene['lab']),
                                                 scene['ji'].opt_imggen, feather=FEATHER, reach=REACH,
                                                 label_before=scene['lab'])
    assert torch.equal(plain[2], hand) and len(plain[4]['passes']) == 2 and 'matte' in plain[4]['passes'][1]
    kept = _move(scene, dst, 5, keep_appearance=True)
    assert not torch.equal(kept[2], plain[2]) and torch.equal(kept[0], plain[0]) and torch.equal(kept[1], plain[1])
