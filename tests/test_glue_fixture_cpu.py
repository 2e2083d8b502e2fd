"""The checks of tests/test_glue_abi_gpu.py must be able to FAIL, and tests/glue_fixture.py must keep its own conditions.
Runs without a GPU: Python stand-ins of the entry points write into a CPU arena through raw addresses (abi_harness.mem),
bands included; each planted defect must be caught by the check that is meant to catch it, and the stand-ins without a
defect are green on every runner and every case of the GPU module."""
import ctypes
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi_harness as ah
import glue_fixture as fx
import test_glue_abi_gpu as G
from glue_fixture import F32, F64
from oracle import ref_cpu

OK, INVALID, WORKSPACE = 0, ah.E_INVALID, ah.E_WORKSPACE


@pytest.fixture(autouse=True)
def _rows_stay_in_memory(monkeypatch):
    monkeypatch.setattr(G, 'flush', lambda: None)
    yield
    del G.ROWS[:]


def _ptrs(addr, n, ctype=ctypes.c_void_p):
    return [v or 0 for v in (ctype * n).from_address(addr)]


def _windows(x, k):
    planes, H, W = x.shape
    OH, OW = H // k, W // k
    return x[:, :OH * k, :OW * k].reshape(planes, OH, k, OW, k).permute(0, 1, 3, 2, 4).reshape(planes, OH, OW, k * k)


class StandIn(object):
    """The entry points in fp32 torch on the CPU, with the library's argument checks; ``defect`` plants one fault."""

    def __init__(self, defect=None):
        self.defect = defect

    def him_last_error(self):
        return b'stand-in'

    def him_reduce_ws(self, n):
        return 1024 * 4

    def him_l1_multi_ws(self, npairs):
        return max(npairs, 0) * 1024 * 4

    def him_sn_ws(self, rows, cols):
        return (2 * rows + 3 * cols + 64) * 4

    # ---- flat elementwise
    def him_add(self, a, b, out, n, stream):
        if not n:
            return OK
        if not (a and b and out):
            return INVALID
        ah.mem(out, n).copy_(ah.mem(a, n) + ah.mem(b, n))
        if self.defect == 'input_modified':
            ah.mem(a, n)[n - 1] += 1.0
        return OK

    def him_fill(self, p, n, value, stream):
        if n and not p:
            return INVALID
        if n:
            ah.mem(p, n).fill_(value)
        return OK

    def him_scale(self, p, n, s, stream):
        if n and not p:
            return INVALID
        if n:
            ah.mem(p, n).mul_(torch.tensor(s, dtype=F32))
        return OK

    def him_u8_to_f32(self, src, dst, n, stream):
        if n and not (src and dst):
            return INVALID
        if n:
            u8 = torch.frombuffer((ctypes.c_uint8 * n).from_address(src), dtype=torch.uint8)
            ah.mem(dst, n).copy_(u8.float())
        return OK

    # ---- losses
    def him_l1_mean_fwd(self, a, b, n, out, ws, ws_bytes, stream):
        if not n:
            return INVALID
        if not ws or ws_bytes < self.him_reduce_ws(n):
            return WORKSPACE
        ah.mem(out, 1).copy_(fx.l1_mean(ah.mem(a, n), ah.mem(b, n), F32))
        return OK

    def him_mse_const_fwd(self, x, n, target, out, ws, ws_bytes, stream):
        if not n:
            return INVALID
        if not ws or ws_bytes < self.him_reduce_ws(n):
            return WORKSPACE
        ah.mem(out, 1).copy_(fx.mse_const(ah.mem(x, n), target, F32))
        return OK

    def him_l1_mean_bwd(self, a, b, n, g, da, accumulate, stream):
        if not n:
            return OK
        A, B = ah.mem(a, n), ah.mem(b, n)
        gs = ah.mem(g, 1)[0] * torch.tensor(1.0 / n, dtype=F32)
        d = A - B
        v = torch.where(d > 0, gs, torch.where(d < 0, -gs, gs if self.defect == 'sign0' else torch.zeros(())))
        if accumulate & 2:
            v = torch.where(A > 0, v, torch.zeros(()))
        out = ah.mem(da, n)
        m = min(n, fx.GRID_CAP) if self.defect == 'stops_at_cap' else n
        out[:m] = (out + v if accumulate & 1 else v)[:m]
        return OK

    def him_mse_const_bwd(self, x, n, target, g, dx, accumulate, stream):
        if not n:
            return OK
        v = (ah.mem(x, n) - target) * (ah.mem(g, 1)[0] * 2.0 * torch.tensor(1.0 / n, dtype=F32))
        out = ah.mem(dx, n)
        out.copy_(out + v if accumulate else v)
        return OK

    def him_l1_multi_fwd(self, a, b, n, npairs, out, ws, ws_bytes, stream):
        if npairs <= 0:
            return OK
        if not (a and b and n and out):
            return INVALID
        if not ws or ws_bytes < self.him_l1_multi_ws(npairs):
            return WORKSPACE
        A, B, N = _ptrs(a, npairs), _ptrs(b, npairs), _ptrs(n, npairs, ctypes.c_size_t)
        for i in range(npairs):
            self.him_l1_mean_fwd(A[i], B[i], N[i], out + 4 * i, ws, ws_bytes, stream)
        return OK

    def him_l1_multi_bwd(self, a, b, n, npairs, g, da, accumulate, stream):
        if npairs <= 0:
            return OK
        if not (a and b and n and g and da):
            return INVALID
        A, B, N, D = _ptrs(a, npairs), _ptrs(b, npairs), _ptrs(n, npairs, ctypes.c_size_t), _ptrs(da, npairs)
        for i in range(npairs):
            if D[i]:
                self.him_l1_mean_bwd(A[i], B[i], N[i], g + 4 * i, D[i], accumulate, stream)
        return OK

    def him_lincomb_fwd(self, terms, weights, n, scale, out, stream):
        if n <= 0 or n > 8 or not (terms and weights and out):
            return INVALID
        t = [float(ah.mem(p, 1)[0]) for p in _ptrs(terms, n)]
        ah.mem(out, 1).copy_(fx.lincomb(t, _ptrs(weights, n, ctypes.c_float), scale))
        return OK

    def him_lincomb_bwd(self, g, weights, n, scale, dterms, stream):
        if n <= 0 or n > 8 or not (g and weights and dterms):
            return INVALID
        d = fx.lincomb_bwd(float(ah.mem(g, 1)[0]), _ptrs(weights, n, ctypes.c_float), scale)
        for i, p in enumerate(_ptrs(dterms, n)):
            if p:
                ah.mem(p, 1)[0] = d[i]
        return OK

    # ---- pools
    def _avg_args(self, p, q, planes, H, W, OH, OW):
        if planes <= 0 or H <= 0 or W <= 0 or OH != fx.pool_out(H) or OW != fx.pool_out(W) or not (p and q):
            return INVALID
        return OK

    def him_avgpool3s2_fwd(self, x, y, planes, H, W, OH, OW, stream):
        rc = self._avg_args(x, y, planes, H, W, OH, OW)
        if rc:
            return rc
        X = ah.mem(x, planes * H * W).view(planes, H, W)
        out = F.avg_pool2d(X.unsqueeze(0), 3, 2, 1, count_include_pad=self.defect == 'avg_div9')[0]
        ah.mem(y, planes * OH * OW).copy_(out.reshape(-1))
        return OK

    def him_avgpool3s2_bwd(self, dy, dx, planes, H, W, OH, OW, stream):
        rc = self._avg_args(dy, dx, planes, H, W, OH, OW)
        if rc:
            return rc
        g = fx.avgpool(torch.zeros(planes, H, W), F32, ah.mem(dy, planes * OH * OW).view(planes, OH, OW))
        ah.mem(dx, planes * H * W).copy_(g.reshape(-1))
        return OK

    def _max_args(self, ptrs, planes, H, W, k):
        if planes <= 0 or H <= 0 or W <= 0 or k <= 0 or H // k <= 0 or W // k <= 0 or not all(ptrs):
            return INVALID
        return OK

    def him_maxpool_fwd(self, x, y, planes, H, W, k, stream):
        rc = self._max_args((x, y), planes, H, W, k)
        if rc:
            return rc
        X = ah.mem(x, planes * H * W).view(planes, H, W)
        ah.mem(y, planes * (H // k) * (W // k)).copy_(_windows(X, k).max(-1).values.reshape(-1))
        return OK

    def _maxpool_bwd(self, x, dy, dx, planes, H, W, k, gate):
        rc = self._max_args((x, dy, dx), planes, H, W, k)
        if rc:
            return rc
        OH, OW = H // k, W // k
        X = ah.mem(x, planes * H * W).view(planes, H, W)
        win = _windows(X, k)
        first = torch.from_numpy(win.numpy().argmax(-1))
        am = (k * k - 1 - torch.from_numpy(win.flip(-1).numpy().argmax(-1))) if self.defect == 'last_max' else first
        g = ah.mem(dy, planes * OH * OW).view(planes, OH, OW).clone()
        if gate and self.defect != 'no_relu_gate':
            g = torch.where(win.max(-1).values > 0, g, torch.zeros(()))
        routed = torch.zeros(planes, OH, OW, k * k).scatter_(-1, am.unsqueeze(-1), g.unsqueeze(-1))
        out = ah.mem(dx, planes * H * W).view(planes, H, W)
        if self.defect != 'tail_unzeroed':
            out.zero_()
        out[:, :OH * k, :OW * k] = routed.view(planes, OH, OW, k, k).permute(0, 1, 3, 2, 4).reshape(planes, OH * k, OW * k)
        return OK

    def him_maxpool_bwd(self, x, dy, dx, planes, H, W, k, stream):
        return self._maxpool_bwd(x, dy, dx, planes, H, W, k, False)

    def him_maxpool_relu_bwd(self, x, dy, dx, planes, H, W, k, stream):
        return self._maxpool_bwd(x, dy, dx, planes, H, W, k, True)

    # ---- encoding
    def him_onehot(self, label, dst, B, nc, Ctot, c0, hw, stream):
        if B <= 0 or nc <= 0 or hw <= 0 or c0 < 0 or c0 + nc > Ctot or not (label and dst):
            return INVALID
        at = c0 + 1 if self.defect == 'slice_plus_one' and c0 + 1 + nc <= Ctot else c0
        ah.mem(dst, B * Ctot * hw).view(B, Ctot, hw)[:, at:at + nc] = fx.onehot(ah.mem(label, B * hw).view(B, hw), nc)
        return OK

    def him_onehot_pool3s2(self, label, dst, B, nc, Ctot, c0, H, W, OH, OW, stream):
        if B <= 0 or nc <= 0 or H <= 0 or W <= 0 or c0 < 0 or c0 + nc > Ctot or not (label and dst):
            return INVALID
        if OH != fx.pool_out(H) or OW != fx.pool_out(W):
            return INVALID
        oh = fx.onehot(ah.mem(label, B * H * W).view(B, H * W), nc).view(B * nc, H, W)
        ah.mem(dst, B * Ctot * OH * OW).view(B, Ctot, OH, OW)[:, c0:c0 + nc] = fx.avgpool(oh, F32).view(B, nc, OH, OW)
        return OK

    def him_edges(self, inst, dst, B, H, W, Ctot, c0, stream):
        if B <= 0 or H <= 0 or W <= 0 or c0 < 0 or c0 + 1 > Ctot or not (inst and dst):
            return INVALID
        e = ref_cpu.get_edges(ah.mem(inst, B * H * W).view(B, 1, H, W))
        ah.mem(dst, B * Ctot * H * W).view(B, Ctot, H, W)[:, c0:c0 + 1] = e
        return OK

    def him_masked_image(self, image, bbox, mask, obj, ctx, B, C, H, W, cls2fill, stream):
        if B <= 0 or C <= 0 or H <= 0 or W <= 0 or not (image and bbox):
            return INVALID
        outs = fx.masked_image(ah.mem(image, B * C * H * W).view(B, C, H, W), ah.mem(bbox, B * 4).view(B, 4), cls2fill)
        for p, t in zip((mask, obj, ctx), outs):
            if p:
                ah.mem(p, t.numel()).copy_(t.reshape(-1))
        return OK

    def him_masked_mean(self, image, mask, noise, emb, B, hw, stream):
        if B <= 0 or hw <= 0 or not (image and mask and emb):
            return INVALID
        e = ref_cpu.color_embedding(ah.mem(mask, B * hw).view(B, 1, hw), ah.mem(image, B * 3 * hw).view(B, 3, hw),
                                    ah.mem(noise, B * 3).view(B, 3) if noise else None)
        ah.mem(emb, B * 3).copy_(e.reshape(-1))
        return OK

    def him_tile_embed(self, emb, mask, dst, B, Ctot, c0, hw, stream):
        if B <= 0 or hw <= 0 or c0 < 0 or c0 + 3 > Ctot or not (emb and mask and dst):
            return INVALID
        ah.mem(dst, B * Ctot * hw).view(B, Ctot, hw)[:, c0:c0 + 3] = fx.tile_embed(ah.mem(emb, B * 3).view(B, 3), ah.mem(mask, B * hw).view(B, hw))
        return OK

    def him_copy_channels(self, src, Csrc, cs0, dst, Cdst, cd0, n, B, hw, mask, mode, accumulate, stream):
        if n < 0 or B <= 0 or hw <= 0 or cs0 < 0 or cs0 + n > Csrc or cd0 < 0 or cd0 + n > Cdst or (mode and not mask):
            return INVALID
        if not n:
            return OK
        if not (src and dst):
            return INVALID
        v = fx.copy_channels(ah.mem(src, B * Csrc * hw).view(B, Csrc, hw), cs0, n, ah.mem(mask, B * hw).view(B, hw) if mask else None, mode)
        out = ah.mem(dst, B * Cdst * hw).view(B, Cdst, hw)[:, cd0:cd0 + n]
        out.copy_(out + v if accumulate else v)
        return OK

    def him_blend(self, a, Ca, ca0, b, Cb, cb0, m, out, B, C, hw, stream):
        if B <= 0 or C <= 0 or hw <= 0 or ca0 < 0 or ca0 + C > Ca or cb0 < 0 or cb0 + C > Cb or not (a and b and m and out):
            return INVALID
        v = fx.blend(ah.mem(a, B * Ca * hw).view(B, Ca, hw), ca0, ah.mem(b, B * Cb * hw).view(B, Cb, hw), cb0, C,
                     ah.mem(m, B * hw).view(B, hw))
        ah.mem(out, B * C * hw).copy_(v.reshape(-1))
        if self.defect == 'past_output':
            ah.mem(out, B * C * hw + 1)[-1] = 0.0
        return OK

    # ---- spectral norm
    def him_sn_power_iter_fwd(self, W, u, rows, cols, v_out, u_out, sigma_out, ws, ws_bytes, stream):
        if rows <= 0 or cols <= 0 or not (W and u and v_out and u_out and sigma_out):
            return INVALID
        if not ws or ws_bytes < self.him_sn_ws(rows, cols):
            return WORKSPACE
        r = fx.sn_chain(ah.mem(W, rows * cols).view(rows, cols), ah.mem(u, rows), F32)
        if self.defect == 'sn_rows1_no_eps' and rows == 1:
            Wm = ah.mem(W, rows * cols).view(rows, cols)
            r['sigma'] = (Wm * r['v'].view(1, -1)).sum(1).abs()
        ah.mem(v_out, cols).copy_(r['v'])
        ah.mem(u_out, rows).copy_(r['u_out'])
        ah.mem(sigma_out, 1).copy_(r['sigma'])
        return OK

    def him_sn_power_iter_bwd(self, W, u, v_out, u_out, sigma, g_sigma, rows, cols, dW, accumulate, ws, ws_bytes, stream):
        if rows <= 0 or cols <= 0 or not (W and u and v_out and g_sigma and dW):
            return INVALID
        if not ws or ws_bytes < self.him_sn_ws(rows, cols):
            return WORKSPACE
        Wm, U, V = ah.mem(W, rows * cols).view(rows, cols), ah.mem(u, rows), ah.mem(v_out, cols)
        eps = torch.tensor(fx.SN_EPS, dtype=F32)
        t = Wm @ V
        d = t.norm() + eps
        a = t / d + t * (eps / (d * d))
        dv, s = a @ Wm, U @ Wm
        nrm = s.norm()
        den = nrm + eps
        k = (s @ dv) / (nrm * den * den) if float(nrm) > 0 else torch.zeros(())
        ds = dv / den - s * k
        val = a.view(-1, 1) * V.view(1, -1)
        if self.defect != 'sn_no_ds':
            val = val + U.view(-1, 1) * ds.view(1, -1)
        val = ah.mem(g_sigma, 1)[0] * val
        out = ah.mem(dW, rows * cols).view(rows, cols)
        out.copy_(out + val if accumulate else val)
        return OK

    def him_div_scalar_fwd(self, W, sigma, out, n, stream):
        if not n:
            return OK
        if not (W and sigma and out):
            return INVALID
        ah.mem(out, n).copy_(ah.mem(W, n) / ah.mem(sigma, 1))
        return OK

    def him_div_scalar_bwd(self, W, sigma, dout, dW, dsigma, n, accumulate, ws, ws_bytes, stream):
        if not n:
            return OK
        if not (W and sigma and dout and dW and dsigma):
            return INVALID
        if not ws or ws_bytes < G.div_scalar_ws(n):
            return WORKSPACE
        out = ah.mem(dW, n)
        r = fx.div_scalar_bwd(ah.mem(W, n), ah.mem(sigma, 1), ah.mem(dout, n), accumulate, out.clone(), F32)
        out.copy_(r[0])
        ah.mem(dsigma, 1).copy_(r[1])
        return OK


# ------------------------------------------------------------------------------------------------- planted defects
def _runs(lib):
    """defect -> the run that must catch it."""
    return {
        'stops_at_cap': lambda: G.run_loss_bwd(lib, 'cpu', fx.BIG, 0),
        'slice_plus_one': lambda: G.run_onehot(lib, 'cpu', 2, 4, 'middle', 3, 3),
        'tail_unzeroed': lambda: G.run_maxpool(lib, 'cpu', 2, 3, 9, 17),
        'last_max': lambda: G.run_maxpool(lib, 'cpu', 2, 3, 8, 16),
        'sign0': lambda: G.run_loss_bwd(lib, 'cpu', 1025, 0),
        'no_relu_gate': lambda: G.run_maxpool(lib, 'cpu', 2, 3, 8, 16),
        'avg_div9': lambda: G.run_avgpool(lib, 'cpu', 2, 5, 4),
        'sn_no_ds': lambda: G.run_sn(lib, 'cpu', 16, 72),
        'sn_rows1_no_eps': lambda: G.run_sn(lib, 'cpu', 1, 8192, scale=1e-10),
        'past_output': lambda: G.run_blend(lib, 'cpu', 2, 3, 7, 'middle', True),
        'input_modified': lambda: G.run_elementwise(lib, 'cpu', 100),
    }


DEFECTS = [('stops_at_cap', r'loss_bwd\|n2097157\|acc0 l1 da: error inf'), ('slice_plus_one', r'onehot\|.* dst: not bit-identical'),
           ('tail_unzeroed', r'maxpool_bwd dx: not bit-identical.*maxpool_bwd dx tail: not bit-identical'),
           ('last_max', r'maxpool_bwd dx: not bit-identical'), ('sign0', r'l1 da: error .* > limit.*l1 da zeros: not bit-identical'),
           ('no_relu_gate', r'maxpool_relu_bwd dx: not bit-identical'), ('avg_div9', r'avgpool\|2x5x4 y: error .* > limit'),
           ('sn_no_ds', r'sn\|16x72\|scale1 dW: error .* > limit'), ('sn_rows1_no_eps', r'sn\|1x8192\|scale1e-10 sigma: error .* > limit'),
           ('past_output', r'guard behind out changed: first byte at \+0'), ('input_modified', r'him_add wrote its input a')]


@pytest.mark.parametrize('defect', [d[0] for d in DEFECTS])
def test_stand_in_without_defect_is_green(defect):
    _runs(StandIn())[defect]()
    assert G.ROWS and all(r['error'] <= r['limit'] for r in G.ROWS)


@pytest.mark.parametrize('defect,message', DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defect_is_caught_by_its_check(defect, message):
    with pytest.raises(AssertionError) as e:
        _runs(StandIn(defect))[defect]()
    assert re.search(message, str(e.value)), str(e.value)
    if defect == 'last_max':
        assert 'maxpool_fwd' not in str(e.value) and ' y:' not in str(e.value)


# ------------------------------------------------------------- every runner, every case of the GPU module, on the CPU
def test_stand_in_is_green_on_the_elementwise_and_loss_cases():
    lib = StandIn()
    for n in (1, 100, 1025, fx.BIG):
        G.run_elementwise(lib, 'cpu', n)
    for n in G.LOSS_N:
        for offset in (0, 1):
            G.run_loss_fwd(lib, 'cpu', n, offset)
    for n in (100, 1025, fx.BIG):
        for accumulate in (0, 1, 2, 3):
            G.run_loss_bwd(lib, 'cpu', n, accumulate)
    for n in range(1, 9):
        G.run_lincomb(lib, 'cpu', n)
    for n in (1, 1025, fx.BIG):
        for accumulate in (0, 1):
            G.run_div_scalar(lib, 'cpu', n, accumulate)


def test_stand_in_is_green_on_l1_multi():
    for accumulate in (0, 1, 2, 3):
        G.run_l1_multi(StandIn(), 'cpu', accumulate, fwd=accumulate == 0)


def test_stand_in_is_green_on_the_pool_cases():
    lib = StandIn()
    for shape in G.AVG_SHAPES:
        G.run_avgpool(lib, 'cpu', *shape)
    for shape in G.MAX_SHAPES:
        G.run_maxpool(lib, 'cpu', *shape)


def test_stand_in_is_green_on_the_encoding_cases():
    lib = StandIn()
    for where in G.SLICES:
        for plane in G.PLANES:
            G.run_onehot(lib, 'cpu', 2, 4, where, *plane)
        for plane in G.PLANES + [(1, 1), (2, 2), (40, 41)]:
            G.run_edges(lib, 'cpu', 2, *plane, where)
        for hw in (7, 9, 117):
            G.run_tile_embed(lib, 'cpu', 2, hw, where)
        for mode in (0, 1, 2):
            for hw in (7, 9, 117):
                G.run_copy_channels(lib, 'cpu', 2, hw, where, mode)
            for fractional, accumulate in ((True, 0), (False, 1), (True, 1)):
                G.run_copy_channels(lib, 'cpu', 2, 117, where, mode, fractional=fractional, accumulate=accumulate)
        for fractional in (False, True):
            for hw in (7, 100, 1025):
                G.run_blend(lib, 'cpu', 2, 3, hw, where, fractional)
    for case in ((1, 3, 'middle', 1, 85), (3, 35, 'last', 31, 33), (1, 3, 'middle', 701, 999)):
        G.run_onehot(lib, 'cpu', *case)
    G.run_edges(lib, 'cpu', 1, 701, 2993, 'first', Ctot=1)
    G.run_tile_embed(lib, 'cpu', 1, 699053, 'first', Ctot=3)
    for mode in (0, 2):
        G.run_copy_channels(lib, 'cpu', 1, 349527, 'last', mode, fractional=mode == 0, n=6, Csrc=6, Cdst=6)
    for fractional in (False, True):
        G.run_blend(lib, 'cpu', 1, 3, 699053, 'first', fractional)
    for null in (None, 'mask', 'obj', 'ctx'):
        G.run_masked_image(lib, 'cpu', 4, 1, 5, 7, null)
        G.run_masked_image(lib, 'cpu', 4, 3, 9, 13, null)
    G.run_masked_image(lib, 'cpu', 1, 3, 700, 999)
    for hw in (1, 100, 256, 5000):
        for kind in fx.MASK_KINDS:
            for with_noise in (0, 1):
                G.run_masked_mean(lib, 'cpu', hw, kind, with_noise)


def test_stand_in_is_green_on_the_spectral_norm_cases():
    lib = StandIn()
    for shape in fx.SN_SHAPES:
        for accumulate in (0, 1):
            G.run_sn(lib, 'cpu', *shape, accumulate=accumulate)
        G.run_sn(lib, 'cpu', *shape, chained=True)
    for shape in ((1, 8192), (16, 72)):
        G.run_sn(lib, 'cpu', *shape, scale=1e-10)
    for shape in ((1, 300), (16, 72), (300, 48)):
        for accumulate in (0, 1):
            G.run_sn_zero(lib, 'cpu', *shape, accumulate)


def test_stand_in_refuses_what_the_library_refuses():
    G.run_refusals(StandIn(), 'cpu')


def test_every_row_has_the_direct_form_limit_or_exact_equality():
    G.run_sn(StandIn(), 'cpu', 16, 72)
    G.run_maxpool(StandIn(), 'cpu', 2, 2, 9, 16)
    for r in G.ROWS:
        assert r['limit'] == (0.0 if r['e32'] == 0.0 and r['ratio'] is None and r['error'] in (0.0, 1.0) and r['limit'] == 0.0
                              else max(8 * r['e32'], 16 * 2.0 ** -24)), r


# ------------------------------------------------------------------------------------------- the fixture's own conditions
def _inside(what, r32, r64):
    for r in (r32 if isinstance(r32, list) else [r32]):
        e32 = ah.max_rel_err(r, r64)
        assert e32 < float('inf') and e32 <= fx.limit(e32), '%s: the float32 restatement is %.3e from float64' % (what, e32)


def test_the_three_summation_orders_are_what_they_say():
    x = fx.rand(3, 1000, seed=1)
    seq = np.float32(0)
    for v in x[1].numpy():
        seq = np.float32(seq + v)
    assert float(fx.fsum(x, 'sequential')[1]) == float(seq)
    lanes = np.zeros(256, np.float32)
    for i, v in enumerate(x[2].numpy()):
        lanes[i % 256] = np.float32(lanes[i % 256] + v)
    m = 256
    while m > 1:
        m //= 2
        lanes = lanes[:m] + lanes[m:]
    assert float(fx.fsum(x, 'lanes')[2]) == float(lanes[0])
    assert torch.equal(fx.fsum(x, 'torch'), x.sum(-1))
    xd = x.double().requires_grad_(True)
    for o in fx.ORDERS:                                  # differentiable, over any axis
        (g,) = torch.autograd.grad(fx.fsum(xd * xd, o, dim=0).sum(), xd)
        assert torch.equal(g, 2 * xd.detach())
        assert ah.max_rel_err(fx.fsum(x.double(), o, dim=0), x.double().sum(0)) < 1e-14


def test_sign_decisions_are_exact_in_both_precisions():
    for n in (100, 1025, fx.BIG):
        for relu in (False, True):
            a, b = fx.l1_pair(n, seed=n % 1000, relu=relu)
            assert fx.sign_margin_ok(a.double() - b.double()) and fx.sign_margin_ok(a - b)
            assert bool((a[::3] == b[::3]).all()) and int((a == b).sum()) >= n // 3
            assert torch.equal(torch.sign(a - b).double(), torch.sign(a.double() - b.double()))
            if relu:
                assert fx.sign_margin_ok(a) and bool((a == 0).any()) and bool((a > 0).any())
    for k, planes, H, W in G.MAX_SHAPES:
        x = fx.maxpool_input(planes, H, W, k)
        assert fx.sign_margin_ok(x)
        win = _windows(x, k)
        mx = win.max(-1).values
        assert bool(((win == mx.unsqueeze(-1)).sum(-1) > 1).any()), 'no tie'
        if W >= 2 * k:
            assert bool((mx == 0).any()) and bool((mx < 0).any())


def test_restatements_follow_torch_and_the_oracle():
    inst = fx.inst_map(2, 9, 13, seed=4)
    for t in (inst, fx.inst_map(2, 1, 7), fx.inst_map(2, 7, 1), fx.inst_map(1, 1, 1)):
        assert torch.equal(fx.edges(t), ref_cpu.get_edges(t.unsqueeze(1))[:, 0])
        assert 0 < float(fx.edges(inst).mean()) < 1
    for kind in fx.MASK_KINDS:
        for noise in (None, torch.tensor([[3.0, 3.0, 1.01], [0.97, -3.0, -3.0]])):
            image, mask = fx.rand(2, 3, 100, seed=1) * 0.3 + torch.tensor([0.6, -0.6, 0.1]).view(1, 3, 1), fx.mean_mask(kind, 2, 100, seed=2)
            want = ref_cpu.color_embedding(mask.double().unsqueeze(1), image.double(), None if noise is None else noise.double())
            got = fx.masked_mean(image, mask, noise, F64)
            assert ah.max_rel_err(got, want) < 1e-14
            if noise is not None and kind != 'empty':
                assert bool((got == 1).any()) and bool((got == -1).any())                     # both clamps
    lab = fx.label_map(2, 21, 4, seed=1)
    oh = fx.onehot(lab, 4)
    assert {4.0, 255.0, -1.0} <= set(lab.view(-1).tolist())
    assert bool((oh[0, :, 0] == 0).all()) and bool((oh[0, :, -1] == 0).all()) and bool((oh[-1, :, 10] == 0).all())
    ok = (lab >= 0) & (lab < 4)
    assert torch.equal(oh.permute(0, 2, 1)[ok], F.one_hot(lab[ok].long(), 4).float())
    a, b = fx.l1_pair(1025, seed=3)
    assert abs(float(fx.l1_mean(a, b, F64)) - float(F.l1_loss(a.double(), b.double()))) < 1e-15
    assert abs(float(fx.mse_const(a, 1.0, F64)) - float(F.mse_loss(a.double(), torch.ones(1025, dtype=F64)))) < 1e-15
    image = fx.rand(1, 2, 5, 7, seed=1)
    m, obj, ctx = fx.masked_image(image, torch.tensor([[4.0, 1.0, 12.0, 9.0]]), -0.25)
    assert float(m.sum()) == 3 * 4 and torch.equal(obj, m * image) and bool((ctx[0, :, 1:, 4:] == -0.25).all())
    assert float(fx.masked_image(image, torch.tensor([[2.0, 3.0, 5.0, 3.0]]), 0.0)[0].sum()) == 0
    t, w = [0.1, 0.7, -1.3], [2.0, 0.5, 10.0]
    assert abs(float(fx.lincomb(t, w, 0.5)) - 0.5 * sum(x * y for x, y in zip(t, w))) < 1e-5


def test_spectral_norm_restatement_agrees_with_the_oracle():
    """On the shapes of tests/test_ops_gpu.py's spectral-norm test, and dW is the oracle's own autograd gradient."""
    for rows, cols in ((8, 48), (64, 1024), (512, 8192 // 16)):
        W, u = fx.sn_case(rows, cols)
        Wd = W.double().requires_grad_(True)
        sigma, un = ref_cpu.max_singular_value(Wd, u.double().view(1, -1))
        r = fx.sn_chain(W, u, F64, g_sigma=0.7)
        assert ah.max_rel_err(r['sigma'], sigma.detach().reshape(1)) < 1e-13
        assert ah.max_rel_err(r['u_out'], un.detach().reshape(-1)) < 1e-13
        (dW,) = torch.autograd.grad(sigma.sum(), Wd, torch.tensor(0.7, dtype=F64))
        assert ah.max_rel_err(r['dW'], dW) < 1e-12


def test_float32_restatements_stay_near_float64():
    for n in G.LOSS_N:
        a, b = fx.l1_pair(n, seed=n % 1000)
        _inside('l1', fx.orders32(lambda dt, o: fx.l1_mean(a, b, dt, o)), fx.l1_mean(a, b, F64))
        _inside('mse', fx.orders32(lambda dt, o: fx.mse_const(a, 1.0, dt, o)), fx.mse_const(a, 1.0, F64))
    a, b = fx.l1_pair(1025, seed=25, relu=True)
    d0 = fx.rand(1025, seed=5)
    for acc in (0, 1, 2, 3):
        _inside('l1 bwd', fx.l1_bwd(a, b, 0.7, acc, d0, F32), fx.l1_bwd(a, b, 0.7, acc, d0, F64))
    _inside('mse bwd', fx.mse_bwd(a, 1.0, 0.7, 1, d0, F32), fx.mse_bwd(a, 1.0, 0.7, 1, d0, F64))
    for planes, H, W in G.AVG_SHAPES[:-1]:
        x, dy = fx.rand(planes, H, W, seed=1), fx.rand(planes, fx.pool_out(H), fx.pool_out(W), seed=2)
        _inside('avgpool', fx.avgpool(x, F32), fx.avgpool(x, F64))
        _inside('avgpool bwd', fx.avgpool(x, F32, dy), fx.avgpool(x, F64, dy))
    for k, planes, H, W in G.MAX_SHAPES[:-1]:
        x, dy = fx.maxpool_input(planes, H, W, k), fx.rand(planes, H // k, W // k, seed=3)
        for gate in (False, True):
            assert torch.equal(fx.maxpool(x, k, F32, dy, gate).double(), fx.maxpool(x, k, F64, dy, gate))
    src, mask = fx.rand(2, 5, 117, seed=1), fx.uniform(2, 117, seed=3)
    for mode in (0, 1, 2):
        _inside('copy', fx.copy_channels(src, 1, 3, mask, mode, F32), fx.copy_channels(src, 1, 3, mask, mode, F64))
    _inside('blend', fx.blend(src, 0, src, 2, 3, mask, F32), fx.blend(src, 0, src, 2, 3, mask, F64))
    for hw in (1, 100, 256, 5000):
        image, m = fx.rand(2, 3, hw, seed=hw), fx.mean_mask('fractional', 2, hw, seed=hw + 1)
        _inside('masked mean', fx.orders32(lambda dt, o: fx.masked_mean(image, m, None, dt, o)), fx.masked_mean(image, m, None, F64))
    for shape, scale in [(s, 1.0) for s in fx.SN_SHAPES[:-1]] + [((1, 8192), 1e-10), ((16, 72), 1e-10)]:
        W, u = fx.sn_case(*shape, scale)
        r64 = fx.sn_chain(W, u, F64, g_sigma=0.7)
        for k in ('v', 'u_out', 'sigma', 'dW'):
            _inside('sn %s %s' % (shape, k), [fx.sn_chain(W, u, F32, o, g_sigma=0.7)[k] for o in fx.ORDERS], r64[k])
    W, sigma, dout = fx.rand(1025, seed=1), torch.tensor([1.7]), fx.rand(1025, seed=2)
    r64 = fx.div_scalar_bwd(W, sigma, dout, 0, W, F64)
    for o in fx.ORDERS:
        r = fx.div_scalar_bwd(W, sigma, dout, 0, W, F32, o)
        _inside('div dW', r[0], r64[0])
        _inside('div dsigma', r[1], r64[1])
