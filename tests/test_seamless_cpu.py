"""CPU: the float64 restatement of the seamless composite (tests/seamless_fixture.py) against its own authority, the
properties of the membrane, the planted defects ``compare`` must catch, and the new interfaces and host refusals."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import seamless_fixture as fx

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
INTERIORS = [(1, 1), (1, 9), (9, 1), (5, 7), (17, 33)]


def _ring_values(seed, H, W):
    return np.random.default_rng(seed).uniform(-1, 1, size=(2, H, W))


@pytest.mark.parametrize('shape', INTERIORS, ids=['%dx%d' % s for s in INTERIORS])
def test_transform_agrees_with_the_dense_solve(shape):
    ny, nx = shape
    worst = 0.0
    for flags in fx.ALL_SIDE_SETS:
        _, _, _, _, H, W = fx.window_for(ny, nx, flags)
        g = _ring_values(ny * 100 + nx + fx.sides_mask(flags), H, W)
        dense, direct = fx.dense_membrane(g, flags), fx.transform_membrane(g, flags)
        worst = max(worst, float(np.abs(dense - direct).max()))
        assert np.abs(fx.residual(dense, flags)).max() <= 1e-13
        ring = fx.ring_mask(H, W, flags)
        assert np.array_equal(dense[:, ring], g[:, ring]) and np.array_equal(direct[:, ring], g[:, ring])
    print('transform vs dense, %dx%d: %.3e' % (ny, nx, worst))
    assert worst <= 1e-12                                     # float64 on at most 561 unknowns with |g| <= 1


@pytest.mark.parametrize('n', [1, 2, 3, 16, 33])
def test_bases_diagonalise_the_second_difference(n):
    for lo, hi in ((1, 1), (0, 0), (1, 0), (0, 1)):
        V, lam = fx.basis(n, lo, hi)
        L = fx.second_difference(n, lo, hi)
        assert np.abs(L @ V - V * lam[None]).max() <= 64 * 2.0 ** -53 * n
        assert np.abs(V.T @ V - np.eye(n)).max() <= 64 * 2.0 ** -53 * n


def test_discrete_maximum_principle():
    for flags in fx.ALL_SIDE_SETS:
        _, _, _, _, H, W = fx.window_for(5, 7, flags)
        g = _ring_values(fx.sides_mask(flags), H, W)
        m = fx.dense_membrane(g, flags)
        ring = fx.ring_mask(H, W, flags)
        for c in range(2):
            lo, hi = g[c][ring].min(), g[c][ring].max()
            assert lo - 1e-13 <= m[c].min() and m[c].max() <= hi + 1e-13


def _scene(seed, ny, nx, flags, offset=None):
    Hc, Wc, x0, y0, H, W = fx.window_for(ny, nx, flags)
    rng = np.random.default_rng(seed)
    O = rng.random((3, Hc, Wc), dtype=np.float32)
    if offset is None:
        P = (rng.integers(0, 256, size=(3, H, W)) / np.float32(255)).astype(np.float32)
    else:
        P = (O[:, y0:y0 + H, x0:x0 + W] + np.float32(offset)).astype(np.float32)
    return O, P, x0, y0


def test_constant_offset_gives_the_photograph_back():
    c = 0.25
    for flags in ((1, 1, 1, 1), (1, 0, 1, 1), (0, 0, 1, 0)):
        O, P, x0, y0 = _scene(3, 6, 9, flags, offset=c)
        O = np.floor(O * 128) / np.float32(256)               # multiples of 1/256 below 1/2: O + c is exact in fp32
        P = (O[:, y0:y0 + P.shape[1], x0:x0 + P.shape[2]] + np.float32(c)).astype(np.float32)
        m64, _ = fx.membrane(O, P, x0, y0, 'dense')
        assert np.abs(m64 + c).max() <= 1e-13
        out = fx.composite(O, P, m64, x0, y0, np.ones(P.shape[1:]), np.float64)
        assert np.abs(out - O).max() <= 1e-13


def test_no_side_counted_gives_zero():
    Hc, Wc, x0, y0, H, W = fx.window_for(4, 6, (0, 0, 0, 0))
    assert (x0, y0, H, W) == (0, 0, Hc, Wc)
    g = _ring_values(1, H, W)
    assert not fx.dense_membrane(g, (0, 0, 0, 0)).any() and not fx.transform_membrane(g, (0, 0, 0, 0)).any()


def _result(O, P, x0, y0, clamp=True, **defect):
    flags = fx.sides(O.shape[1], O.shape[2], x0, y0, P.shape[1], P.shape[2])
    m = fx.transform_membrane(fx.boundary_values(O, P, x0, y0), flags, **defect).astype(np.float32)
    H, W = P.shape[1:]
    canvas = fx.composite(O, P, m, x0, y0, np.ones((H, W), np.float32), np.float32, clamp=clamp)
    return m, canvas


def test_compare_accepts_the_contract_and_catches_planted_defects():
    flags = (1, 0, 1, 1)                                      # the right side is on the canvas edge: Neumann
    O, P, x0, y0 = _scene(11, 9, 12, flags)
    m, canvas = _result(O, P, x0, y0)
    assert canvas.min() >= 0 and canvas.max() <= 1
    assert (P + m).max() > 1 or (P + m).min() < 0, 'the scene must reach the clamp'
    rows = []
    assert fx.compare(m, canvas, None, O, P, x0, y0, rows=rows, case='good') == []
    assert {r['tensor'] for r in rows} == {'membrane', 'residual', 'canvas_alpha1'}
    for defect in (dict(dirichlet_everywhere=True), dict(normalise=False), dict(drop_corner=True),
                   dict(wrong_lambda=True), dict(clamp=False)):
        bad_m, bad_canvas = _result(O, P, x0, y0, **defect)
        assert fx.compare(bad_m, bad_canvas, None, O, P, x0, y0, case=str(defect)), defect
    off = m.copy()
    off[0, 0, 3] = np.nextafter(off[0, 0, 3], np.float32(2))  # one ulp on the ring
    assert fx.compare(off, canvas, None, O, P, x0, y0)
    ring_written = canvas.copy()
    ring_written[1, y0, x0 + 2] = np.nextafter(ring_written[1, y0, x0 + 2], np.float32(2))
    assert fx.compare(m, ring_written, None, O, P, x0, y0)


def test_compare_with_a_matte():
    import composite_fixture as cf
    flags = (1, 1, 1, 1)
    O, P, x0, y0 = _scene(5, 14, 20, flags)
    Hc, Wc = O.shape[1:]
    H, W = P.shape[1:]
    changed = np.zeros((H, W), np.uint8)
    changed[6:9, 8:12] = 1
    d2 = cf.dist2_of(changed)
    m64, _ = fx.membrane(O, P, x0, y0)
    m = m64.astype(np.float32)
    a32 = cf.matte(Hc, Wc, x0, y0, H, W, 4, 2, d2, cf.SMOOTH, np.float32)
    canvas = fx.composite(O, P, m, x0, y0, a32, np.float32)
    rows = []
    assert fx.compare(m, canvas, a32, O, P, x0, y0, feather=4, reach=2, dist2=d2, rows=rows) == []
    assert {'matte', 'canvas_ramp', 'canvas_alpha1'} <= {r['tensor'] for r in rows}
    hard = fx.composite(O, P, m, x0, y0, (a32 > 0).astype(np.float32), np.float32)
    assert fx.compare(m, hard, a32, O, P, x0, y0, feather=4, reach=2, dist2=d2)


# --------------------------------------------------------------------------------------------- interfaces and refusals
NEW_SYMBOLS = ('him_membrane_basis', 'him_membrane_ws', 'him_membrane_solve', 'him_canvas_seamless_apply')


def test_header_exports_and_ctypes_signatures():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    header = open(os.path.join(ROOT, 'include', 'him.h')).read()
    assert 'Seamless canvas composite' in header and '#define HIM_MEMBRANE_NO_SIDE 1' in header
    lib = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NEW_SYMBOLS:
        decl = re.search(r'^(int|size_t) %s\(([^;]*)\);' % name, header, re.M | re.S)
        assert decl, name
        assert hasattr(lib, name), name
        restype, argtypes = _cabi._SIGS[name]
        assert len(argtypes) == decl.group(2).count(',') + 1, name
        assert restype is (ctypes.c_size_t if decl.group(1) == 'size_t' else ctypes.c_int)
    lib.him_membrane_ws.restype = ctypes.c_size_t
    per = lambda ny, nx: 3 * (4 * (nx + ny) + 2 * ny * nx) * 8          # noqa: E731
    assert lib.him_membrane_ws(10, 12, 15) == per(8, 10) and lib.him_membrane_ws(10, 12, 1) == per(10, 11)
    for H, W, s in ((2, 12, 12), (10, 1, 1), (0, 4, 1), (2051, 8, 12), (2050, 8, 12 + 16), (8, 2049, 4)):
        assert lib.him_membrane_ws(H, W, s) == 0, (H, W, s)
    assert lib.him_membrane_ws(2050, 8, 12) > 0


def test_host_refusals_come_before_any_device_work():
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd.util import data_util
    with pytest.raises(ValueError):
        ops.membrane_sides(20, 20, 3, 3, 2, 8)                # top and bottom counted: ny = 0
    with pytest.raises(ValueError):
        ops.membrane_sides(20, 20, 0, 3, 5, 1)                # right counted: nx = 0
    with pytest.raises(ValueError):
        ops.membrane_sides(4000, 8, 1, 1, 2051, 6)            # ny = 2049
    with pytest.raises(ValueError):
        ops.membrane_sides(20, 20, 3, 3, 18, 5)               # outside the canvas
    assert ops.membrane_sides(4000, 8, 0, 1, 2050, 8) == (0, 0, 1, 1, 2048, 8)
    for bad in (dict(n=0), dict(n=2049), dict(n=True), dict(lo=2), dict(hi=-1)):
        with pytest.raises(ValueError):
            ops.membrane_basis(**dict(dict(n=4, lo=1, hi=1), **bad))
    canvas, patch = torch.zeros(1, 3, 20, 20), torch.zeros(1, 3, 8, 8)   # host tensors: reaching a kernel would raise HimError
    for kw in (dict(H=2), dict(feather=0), dict(feather=4, profile='cubic'), dict(profile='cubic'), dict(reach=1)):
        a = dict(dict(H=6, W=6), **kw)
        with pytest.raises(ValueError):
            ops.canvas_paste_seamless(patch, (0, 0, 8, 8), canvas, 3, 3, a.pop('H'), a.pop('W'), 0, **a)
    info = {'output_bbox_global': torch.tensor([3., 3., 9., 9.]), 'output_bbox': torch.tensor([0., 0., 7., 7.])}
    with pytest.raises(ValueError):
        data_util.paste_canvas_seamless(canvas, patch, info, is_img=False)              # a label paste
    with pytest.raises(ValueError):
        data_util.paste_canvas_seamless(canvas, patch, info, reach=2)                   # reach needs feather
    with pytest.raises(ValueError):
        data_util.paste_canvas_seamless(canvas, patch, info, profile='cubic')
    thin = {'output_bbox_global': torch.tensor([3., 3., 9., 4.]), 'output_bbox': torch.tensor([0., 0., 7., 7.])}
    with pytest.raises(ValueError):
        data_util.paste_canvas_seamless(canvas, patch, thin)                            # two rows between two counted sides


def test_new_signatures():
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd.models.joint_inference_model import JointInference as ji
    from neurips18_hierchical_image_manipulation_amd.util import data_util
    sig = lambda f: inspect.signature(f).parameters                  # noqa: E731
    assert list(sig(data_util.paste_canvas_seamless)) == list(sig(data_util.paste_canvas_feathered))
    assert list(sig(ji.gen_image_seamless)) == list(sig(ji.gen_image_feathered))
    for a, b in ((data_util.paste_canvas_seamless, data_util.paste_canvas_feathered),
                 (ji.gen_image_seamless, ji.gen_image_feathered)):
        assert [(p.kind, p.default) for p in sig(a).values()] == [(p.kind, p.default) for p in sig(b).values()]
    assert list(sig(ops.canvas_paste_seamless)) == ['cropped', 'box', 'canvas', 'x0', 'y0', 'H', 'W', 'pre', 'feather',
                                                    'reach', 'dist2', 'profile', 'want_matte']
    assert sig(ops.canvas_paste_seamless)['feather'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig(ops.membrane_solve)) == ['canvas', 'x0', 'y0', 'P']
    assert list(sig(ops.membrane_basis))[:3] == ['n', 'lo', 'hi']
    for name in ('remove_object', 'move_object', 'rescale_object'):
        p = sig(getattr(ji, name))['seamless']
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, name
    for bad in (1, None, 'yes'):
        with pytest.raises(ValueError):
            ji.remove_object(None, None, None, None, None, None, seamless=bad)
