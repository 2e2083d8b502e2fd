"""CPU: the float64 restatement of the region Poisson clone (tests/region_poisson_fixture.py) against the dense membrane
of tests/seamless_fixture.py and against hand-written answers, the properties of the solution, the iteration counts of
the conjugate-gradient restatement under the cap 6 (H + W), the planted defects ``compare`` must catch, and the new
interfaces with every host-side refusal."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import region_poisson_fixture as fx
import seamless_fixture as sf

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
E_INVALID, E_WORKSPACE = -1, -2


def _exact_scene(seed, Hc, Wc, H, W):
    """Values on multiples of 1/64 below 1/2: sums and differences are exact."""
    g = np.random.default_rng(seed)
    O = (g.integers(0, 32, size=(3, Hc, Wc)) / 64.0).astype(np.float32)
    P = (g.integers(0, 32, size=(3, H, W)) / 64.0).astype(np.float32)
    return O, P


# ------------------------------------------------------------------------------------------------------- the equations
@pytest.mark.parametrize('flags', [(1, 1, 1, 1), (0, 1, 1, 0), (1, 0, 0, 1), (0, 0, 1, 0)], ids=str)
def test_a_rectangle_is_the_dense_membrane(flags):
    Hc, Wc, x0, y0, H, W = sf.window_for(6, 9, flags)
    O, P = fx.scene(3, Hc, Wc, H, W)
    s = fx.system(O, P, x0, y0, np.ones((H, W), np.uint8))
    assert sf.sides(Hc, Wc, x0, y0, H, W) == flags and s['n'] == 6 * 9
    m = sf.dense_membrane(sf.boundary_values(O, P, x0, y0), flags)
    inside = ~sf.ring_mask(H, W, flags)
    assert np.array_equal(s['omega'], inside)
    assert np.abs(fx.dense(s) - np.where(inside, m, 0.0)).max() <= 1e-12
    u, its = fx.cg(s, 1e-12)
    assert np.abs(u - fx.dense(s)).max() <= 1e-9 and max(its) <= fx.default_cap(H, W) // 2


def _blob_scene(x0, y0, Hc=60, Wc=80, seed=5):
    R = fx.blob_region()
    H, W = R.shape
    O, P = fx.scene(seed, Hc, Wc, H, W)
    return O, P, x0, y0, R


def test_discrete_maximum_principle_in_import_mode():
    for x0, y0 in ((0, 0), (9, 7)):
        O, P, x0, y0, R = _blob_scene(x0, y0)
        s = fx.system(O, P, x0, y0, R)
        om, H, W = s['omega'], s['H'], s['W']
        g = sf.boundary_values(O, P, x0, y0)
        rim = np.zeros((H, W), bool)                              # the pixels whose g enters some equation
        for y, x in np.argwhere(om):
            for dy, dx in fx.NEIGHBOURS:
                qy, qx = y + dy, x + dx
                if 0 <= qy < H and 0 <= qx < W and not om[qy, qx]:
                    rim[qy, qx] = True
        u = fx.dense(s)
        for c in range(3):
            assert g[c][rim].min() - 1e-12 <= u[c][om].min() and u[c][om].max() <= g[c][rim].max() + 1e-12


def test_constant_offset_and_equal_patch():
    R = fx.blob_region()
    H, W = R.shape
    for x0, y0 in ((0, 0), (5, 4), (27, 23)):
        O, _ = _exact_scene(1, 60, 80, H, W)
        for c, mixed in ((0.25, False), (0.25, True), (0.0, False), (0.0, True)):
            P = (O[:, y0:y0 + H, x0:x0 + W] - np.float32(c)).astype(np.float32)      # O = P + c, exactly
            s = fx.system(O, P, x0, y0, R, mixed)
            u = fx.dense(s)
            assert np.abs(u[:, s['omega']] - c).max() <= 1e-12 and not u[:, ~s['omega']].any()
            if c == 0.0:
                assert not s['b'].any() and fx.cg(s, 1e-10)[1] == [0, 0, 0]        # b == 0: no iteration, no division


def test_mixed_tie_takes_the_patch():
    H, W = 5, 7
    _, P = _exact_scene(2, 9, 11, H, W)
    O = np.zeros((3, 9, 11), np.float32)
    O[:, 2:2 + H, 2:2 + W] = 0.5 - P                              # O(p) - O(q) = -(P(p) - P(q)): equal magnitudes
    R = np.zeros((H, W), np.uint8)
    R[1:4, 2:5] = 1
    tie, plain = fx.system(O, P, 2, 2, R, True), fx.system(O, P, 2, 2, R, False)
    assert np.array_equal(tie['b'], plain['b'])                  # every pair ties, every pair keeps the patch's gradient
    assert not np.array_equal(fx.system(O, P, 2, 2, R, True, no_abs=True)['b'], plain['b'])
    O[:, 4, 5] += np.float32(1 / 64.0)                           # one photograph gradient now strictly stronger
    assert not np.array_equal(fx.system(O, P, 2, 2, R, True)['b'], fx.system(O, P, 2, 2, R, False)['b'])


@pytest.mark.parametrize('case', fx.hand_cases(), ids=[c[0] for c in fx.hand_cases()])
def test_hand_written_answers(case):
    name, O, P, x0, y0, R, mixed, want = case
    s = fx.system(O, P, x0, y0, R, mixed)
    assert s['n'] == len(want) and s['dropped'] == 0
    for u in (fx.dense(s), fx.cg(s, 1e-10)[0]):
        for (y, x), v in want.items():
            assert np.abs(u[:, y, x] - v).max() <= 2e-10 + fx.HAND_SLACK, (name, y, x)


# (name, window, region, position of the window's corner in a 100 x 300 canvas)
GPU_REGIONS = [('blob', fx.blob_region(), (9, 7)), ('full', np.ones((37, 53), np.uint8), (9, 7)),
               ('band', fx.band_region(), (17, 13))]


@pytest.mark.parametrize('case', GPU_REGIONS, ids=[c[0] for c in GPU_REGIONS])
def test_cg_stays_within_half_the_cap(case):
    """Iterations of the restatement at rtol 1e-10, import mode (this file's figures, printed):
    blob 37 x 53: 568 unknowns, 87 iterations (cap 540); full 37 x 53: 1785, 174 (540); band 67 x 261: 1800, 78 (1968)."""
    name, R, (x0, y0) = case
    H, W = R.shape
    O, P = fx.scene(11, 100, 300, H, W)
    s = fx.system(O, P, x0, y0, R)
    _, its = fx.cg(s, 1e-10)
    print('%s %dx%d: %d unknowns, iterations %s, cap %d' % (name, H, W, s['n'], its, fx.default_cap(H, W)))
    assert 0 < s['n'] <= 2000 and 0 < max(its) <= fx.default_cap(H, W) // 2


# ----------------------------------------------------------------------------------------------------- planted defects
def _result(O, P, x0, y0, R, mixed, rtol=1e-10, clamp=True, **defect):
    """(u, canvas fp32, status) of a restated solve with the given defect."""
    s = fx.system(O, P, x0, y0, R, mixed, **defect)
    u, its = fx.cg(s, rtol)
    canvas = fx.composite(O, P, u, x0, y0, s['omega'], clamp=clamp, dtype=np.float32)
    return u, canvas, [sf.sides_mask(s['flags']), s['n'], s['dropped'], max(its), 0, 0, 0, 0]


def test_compare_accepts_the_contract_and_catches_planted_defects():
    O, P, x0, y0, R = _blob_scene(0, 0, Hc=37 + 6, Wc=53 + 6)        # top and left on the canvas edge: Neumann
    for mixed in (False, True):
        s = fx.system(O, P, x0, y0, R, mixed)
        u64 = fx.dense(s)
        check = lambda got, rtol=1e-10: fx.compare(got[0], got[1], got[2], O, P, x0, y0, R, mixed, rtol, s=s,   # noqa: E731
                                                   u64=u64)
        rows = []
        good = _result(O, P, x0, y0, R, mixed)
        assert fx.compare(good[0], good[1], good[2], O, P, x0, y0, R, mixed, 1e-10, rows=rows) == []
        assert len(rows) == 9 and all(r['ratio'] is not None and r['ratio'] <= 1 for r in rows)
        v = P.astype(np.float64) + u64
        assert (v[:, s['omega']] > 1).any() or (v[:, s['omega']] < 0).any(), 'the scene must reach the clamp'
        hole = np.zeros(R.shape, bool)
        hole[16, 18] = True
        assert R[16, 18] == 0 and R[16, 13] == 1                      # a pixel of the hole, inside the blob
        assert check(_result(O, P, x0, y0, R, mixed, omega_extra=hole))           # 1: a hole pixel solved for
        assert check(_result(O, P, x0, y0, R, mixed, all_dirichlet=True))         # 2: a Neumann side as Dirichlet
        assert check(_result(O, P, x0, y0, R, mixed, deg4=True))                  # 3: deg fixed at 4 on the canvas edge
        if mixed:
            assert check(_result(O, P, x0, y0, R, mixed, no_abs=True))            # 4: the comparison without |.|
        assert check(_result(O, P, x0, y0, R, mixed, rtol=1e-2))                  # 5: stopped at 1e-2, claimed converged
        assert check(_result(O, P, x0, y0, R, mixed, clamp=False))                # 6: no clamp
        assert check(_result(O, P, x0, y0, R, mixed, rtol=1e-2), rtol=1e-2) == [] # ... and honest about it: accepted
        moved = good[1].copy()
        moved[0, 36 + 3, 2] += 1e-3                                                # a pixel outside Omega written
        assert check((good[0], moved, good[2]))


# ----------------------------------------------------------------------------------------------------------- interfaces
NEW_SYMBOLS = ('him_region_poisson_ws', 'him_region_poisson_solve', 'him_region_poisson_apply')


def test_header_exports_and_ctypes_signatures():
    from neurips18_hierchical_image_manipulation_amd import _cabi
    header = open(os.path.join(ROOT, 'include', 'him.h')).read()
    assert 'Region Poisson clone' in header
    for name, v in (('EMPTY', 1), ('SINGULAR', 2), ('MAX_ITER_HIT', 4), ('NONFINITE', 8), ('MAX_N', 2048)):
        assert '#define HIM_REGION_POISSON_%s %d' % (name, v) in header
    lib = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NEW_SYMBOLS:
        decl = re.search(r'^(int|size_t) %s\(([^;]*)\);' % name, header, re.M | re.S)
        assert decl, name
        assert hasattr(lib, name), name
        restype, argtypes = _cabi._SIGS[name]
        assert len(argtypes) == decl.group(2).count(',') + 1, name
        assert restype is (ctypes.c_size_t if decl.group(1) == 'size_t' else ctypes.c_int)
    assert 'him_region_poisson.hip' in open(os.path.join(os.path.dirname(_cabi.__file__), 'csrc', 'Makefile')).read()
    lib.him_region_poisson_ws.restype = ctypes.c_size_t
    for H, W in ((0, 4), (4, 0), (-1, 4), (2049, 8), (8, 2049)):
        assert lib.him_region_poisson_ws(H, W) == 0, (H, W)
    small, big = lib.him_region_poisson_ws(1, 1), lib.him_region_poisson_ws(2048, 2048)
    assert small > 0 and small % 8 == 0 and big >= 12 * 8 * 2048 * 2048
    assert lib.him_region_poisson_ws(37, 53) - lib.him_region_poisson_ws(37, 52) >= 12 * 8 * 37   # r, two p, A p per channel


def test_library_refusals_come_before_any_launch():
    """Every pointer is a small fake address: a call that reached a kernel would fault, a refused one returns first."""
    from neurips18_hierchical_image_manipulation_amd import _cabi
    lib = _cabi.lib._load()
    nws = int(lib.him_region_poisson_ws(5, 7))
    ok = dict(canvas=64, Hc=9, Wc=11, x0=2, y0=2, H=5, W=7, P=64, region=64, mixed=0, rtol=1e-7, max_iter=10, u=64,
              status=64, resid=64, ws=64, ws_bytes=nws, stream=0)
    order = list(ok)

    def solve(**kw):
        return lib.him_region_poisson_solve(*[dict(ok, **kw)[k] for k in order])

    invalid = [dict(canvas=0), dict(P=0), dict(region=0), dict(u=0), dict(status=0), dict(resid=0), dict(x0=-1), dict(y0=-1),
               dict(x0=5), dict(y0=5), dict(Wc=8), dict(Hc=6), dict(H=0), dict(W=0), dict(H=-3), dict(H=2049, Hc=4000),
               dict(W=2049, Wc=4000), dict(rtol=0.0), dict(rtol=1.0), dict(rtol=-1e-3), dict(rtol=float('nan')),
               dict(rtol=float('inf')), dict(max_iter=0), dict(max_iter=-5), dict(max_iter=(1 << 20) + 1), dict(mixed=2),
               dict(mixed=-1), dict(u=68), dict(ws=68), dict(resid=68)]
    for kw in invalid:
        assert solve(**kw) == E_INVALID, kw
        assert lib.him_last_error()
    for kw in (dict(ws=0), dict(ws_bytes=nws - 1), dict(ws_bytes=0)):
        assert solve(**kw) == E_WORKSPACE, kw
    ok_a = dict(P=64, u=64, region=64, canvas=64, Hc=9, Wc=11, x0=2, y0=2, H=5, W=7, stream=0)
    for kw in (dict(P=0), dict(u=0), dict(region=0), dict(canvas=0), dict(x0=-1), dict(y0=5), dict(Wc=8), dict(H=0),
               dict(W=0), dict(H=2049, Hc=4000), dict(W=2049, Wc=4000), dict(u=68)):
        assert lib.him_region_poisson_apply(*[dict(ok_a, **kw)[k] for k in ok_a]) == E_INVALID, kw


def test_wrapper_refusals_come_before_any_device_work():
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd._cabi import HimError
    assert ops.region_poisson_args(401, 397, False, 1e-7, None) == (0, 1e-7, 6 * 798)
    assert ops.region_poisson_args(5, 7, True, 0.5, 3) == (1, 0.5, 3)
    for kw in (dict(mixed=1), dict(mixed=None), dict(rtol=0), dict(rtol=1.0), dict(rtol=float('nan')), dict(rtol='1e-7'),
               dict(rtol=True), dict(max_iter=0), dict(max_iter=2.5), dict(max_iter=True), dict(max_iter=(1 << 20) + 1),
               dict(H=0), dict(W=2049)):
        with pytest.raises(ValueError):
            ops.region_poisson_args(**dict(dict(H=5, W=7, mixed=False, rtol=1e-7, max_iter=None), **kw))
    # host tensors: reaching a kernel would raise HimError, the refusals below are ValueError and come first
    canvas, P, R = torch.zeros(1, 3, 9, 11), torch.zeros(1, 3, 5, 7), torch.zeros(5, 7, dtype=torch.uint8)
    u = torch.zeros(1, 3, 5, 7, dtype=torch.float64)
    for kw in (dict(mixed=1), dict(rtol=2.0), dict(max_iter=0)):
        with pytest.raises(ValueError):
            ops.region_poisson_solve(canvas, 2, 2, P, R, **kw)
    for x0, y0 in ((-1, 2), (2, -1), (5, 2), (2, 5)):
        with pytest.raises(ValueError):
            ops.region_poisson_solve(canvas, x0, y0, P, R)
        with pytest.raises(ValueError):
            ops.region_poisson_apply(P, u, R, canvas, x0, y0)
    with pytest.raises(HimError):
        ops.region_poisson_solve(canvas, 2, 2, P, R)                 # nothing left to refuse but the host tensors
    src, plane = torch.zeros(1, 3, 20, 20), torch.zeros(9, 11, dtype=torch.uint8)
    for kw in (dict(src_box=(0, 0, 21, 5)), dict(src_box=(3, 3, 3, 8)), dict(dst_box=(11, 0, 15, 4)),
               dict(dst_box=(0, -6, 4, 0)), dict(dst_box=(1, 2, 3)), dict(mixed='yes'), dict(rtol=0.0), dict(max_iter=-1),
               dict(src=canvas)):
        a = dict(dict(src=src, src_box=(2, 2, 8, 8), canvas=canvas, dst_box=(1, 1, 6, 5), region=plane), **kw)
        with pytest.raises(ValueError):
            ops.canvas_clone_region(a.pop('src'), a.pop('src_box'), a.pop('canvas'), a.pop('dst_box'), a.pop('region'), **a)


def test_new_signatures_and_defaults():
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd.models.joint_inference_model import JointInference as ji
    sig = lambda f: inspect.signature(f).parameters                  # noqa: E731
    assert list(sig(ops.region_poisson_solve)) == ['canvas', 'x0', 'y0', 'P', 'region', 'mixed', 'rtol', 'max_iter']
    assert list(sig(ops.region_poisson_apply)) == ['P', 'u', 'region', 'canvas', 'x0', 'y0']
    assert list(sig(ops.canvas_clone_region)) == ['src', 'src_box', 'canvas', 'dst_box', 'region', 'mixed', 'rtol',
                                                  'max_iter']
    for f in (ops.region_poisson_solve, ops.canvas_clone_region):
        for name, default in (('mixed', False), ('rtol', 1e-7), ('max_iter', None)):
            p = sig(f)[name]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default and type(p.default) is type(default)
    for name in ('keep_appearance', 'mixed'):
        p = sig(ji.move_object)[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, name
    assert sig(ji.rescale_object)['kw'].kind is inspect.Parameter.VAR_KEYWORD
    for kw in (dict(keep_appearance=1), dict(keep_appearance=None), dict(keep_appearance=True, mixed='yes'),
               dict(mixed=True), dict(keep_appearance=False, mixed=True)):
        with pytest.raises(ValueError):
            ji.move_object(None, None, (1, 1, 5, 5), None, None, None, None, **kw)
