#!/usr/bin/env python
"""The weight-gradient plan (csrc/him_conv.hip plan_wgrad) over the grid of tools/conv_plan_table.py -- its descriptors x
HimAlgo settings -- plus a few descriptors that grid does not need (EXTRA), for the three callers of the plan: the conv, the
transposed conv whose adjoint it is, and the dense slice of a one-hot stem.  No GPU: him_conv2d_bwd_weight_plan /
him_deconv2d_bwd_weight_plan are host functions of the descriptor.

    python tools/wgrad_plan_table.py [--lib libhim_hip.so] [-o tests/golden/wgrad_plan_table.json]

Per caller: family, need_bytes, splits, tile_m, tile_n of the plan, and `slab` = the *_bwd_weight_ws answer minus the dbias
scratch behind the slab region (csrc/him_conv_wgrad.inc bias_ws_bytes).  A refused descriptor answers -1 everywhere.

The one-hot dense slice has no query of its own.  It is planned like a transposed conv -- no Winograd space reserved, and the
padding mode does not enter the plan -- so its columns are the transposed-conv query on the twin whose adjoint is the dense
descriptor (Cin - n_onehot input channels).

tests/test_wgrad_plan_cpu.py compares the built library with the committed table, which was written by the library of the
commit BEFORE the selection became a plan, given a dry-run switch in run_wgrad that reported (family, need, splits, tile)
where each branch would launch.  Regenerate it only with a change that is meant to move a selection.  File form: pack() /
unpack() of tools/conv_plan_table.py."""
import argparse
import ctypes
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('conv_plan_table', os.path.join(HERE, 'conv_plan_table.py'))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)
A = T.A

GOLDEN = os.path.join(T.ROOT, 'tests', 'golden', 'wgrad_plan_table.json')
FIELDS = ['family', 'need', 'splits', 'tile_m', 'tile_n', 'slab']
CALLERS = ['conv', 'deconv', 'onehot_dense']
COLUMNS = ['%s_%s' % (c, f) for c in CALLERS for f in FIELDS]
FAMILIES = ['wino', 'head', 'stem', 'small_win', 'small', 'fast', 'generic']      # the codes of include/him.h
# (B, Cin, H, W, Cout, k, stride, pad, pad_mode, act, n_onehot) that tools/conv_plan_table.py's pinned grid lacks
EXTRA = [
    (1, 131, 8, 8, 128, 3, 1, 1, 'reflect', 'none', 3),      # one-hot stems whose dense slice has the F(2x2) shape under
    (1, 131, 8, 8, 128, 3, 1, 1, 'zero', 'none', 3),         # wino_min_c = 16: planned without Winograd space
    (8, 4, 256, 256, 3, 5, 2, 2, 'zero', 'none', 0),         # tiny-M 5x5 off the "same" geometry: generic, 512 splits
]


def descriptors():
    return T.descriptors() + EXTRA


def load(path=None):
    dll = T.load(path)
    for name in ('him_conv2d_bwd_weight_plan', 'him_deconv2d_bwd_weight_plan'):
        fn = getattr(dll, name)
        fn.restype, fn.argtypes = A._SIGS[name]
    return dll


def bias_ws_bytes(C):
    return C * 32 * 2 * 4 + 256


def _plan(query, ws_query, desc, bias_c):
    fam, spl, tm, tn, need = ctypes.c_int(-1), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    if query(ctypes.byref(desc), ctypes.byref(fam), ctypes.byref(need), ctypes.byref(spl), ctypes.byref(tm), ctypes.byref(tn)):
        return [-1] * len(FIELDS)
    return [fam.value, need.value, spl.value, tm.value, tn.value, ws_query(ctypes.byref(desc)) - bias_ws_bytes(bias_c)]


def answers(lib, d, over):
    B, Cin, H, W, Cout, k, s, p, pm, act, nc = d
    a = A.HimAlgo()
    for key, v in over.items():
        setattr(a, key, v)
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    out_pad = H - ((OH - 1) * s - 2 * p + k)

    def deconv(cin):     # the transposed conv whose adjoint is the conv from `cin` channels
        t = A.HimDeconv2d(B, Cout, OH, OW, cin, k, k, s, p, out_pad, H, W, T.ACTS[act], 0.2, a)
        return _plan(lib.him_deconv2d_bwd_weight_plan, lib.him_deconv2d_bwd_weight_ws, t, cin)

    c = A.HimConv2d(B, Cin, H, W, Cout, k, k, s, p, A.PAD_REFLECT if pm == 'reflect' else A.PAD_ZERO, OH, OW, T.ACTS[act], 0.2, a)
    conv = _plan(lib.him_conv2d_bwd_weight_plan, lib.him_conv2d_bwd_weight_ws, c, Cout)
    dense = deconv(Cin - nc) if 0 < nc < Cin and lib.him_conv2d_onehot_bwd_weight_ws(ctypes.byref(c), nc) else [-1] * len(FIELDS)
    return conv + deconv(Cin) + dense


def table(lib):
    ds, als = descriptors(), T.algos()
    rows = []
    for i, d in enumerate(ds):
        groups = []                                  # [values, [algo indices]] in first-seen order
        for j, over in enumerate(als):
            v = [int(x) for x in answers(lib, d, over)]
            for g in groups:
                if g[0] == v:
                    g[1].append(j)
                    break
            else:
                groups.append([v, [j]])
        rows += [[i, g[1], g[0]] for g in groups]
    return {'columns': COLUMNS, 'descriptors': [list(d) for d in ds], 'algos': als, 'rows': rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--lib', default=None, help='library to query (default: the built in-tree one)')
    ap.add_argument('-o', '--out', default=GOLDEN)
    args = ap.parse_args()
    tab = table(load(args.lib))
    with open(args.out, 'w') as f:
        f.write(T.pack(tab))
    with open(args.out) as f:
        assert T.expand(T.unpack(json.load(f))) == T.expand(tab)
    print('%d descriptors x %d algos -> %d rows, %d bytes: %s' % (len(tab['descriptors']), len(tab['algos']), len(tab['rows']),
                                                                 os.path.getsize(args.out), args.out))


if __name__ == '__main__':
    main()
