#!/usr/bin/env python
"""Every pure query of the convolution dispatch (csrc/him_conv.hip plan_fprop / plan_dgrad and their readers) over a fixed
grid of descriptors x HimAlgo settings, for the conv and for the transposed conv whose adjoint it is.  No GPU: the queries
are host functions of the descriptor.

    python tools/conv_plan_table.py [--lib libhim_hip.so] [-o tests/golden/conv_plan_table.json]

tests/test_conv_plan_cpu.py recomputes the table from the built library and compares it with the committed one, which
was written by the library of the commit BEFORE the dispatch became a plan: a refactor of the selection must not move a
byte of it.  Regenerate it only with a change that is meant to move a selection or a workspace size.

Grid: the op tests' case lists, the layer-shape families of bench.py's c2 and box2mask workloads, and edge descriptors on
each threshold of the selection; each under every HimAlgo override of tests/test_conv_abi_gpu.py.  Overrides that answer
alike are stored once per descriptor, as their difference from the default's answers (pack / unpack)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
from neurips18_hierchical_image_manipulation_amd import _cabi as A      # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_plan_table.json')
COLUMNS = ['fwd_ws', 'bwd_data_ws', 'panel_bytes_fwd', 'panel_bytes_bwd', 'panel_layout_fwd', 'panel_layout_bwd',
           'shares_fwd_panel', 'in_act_fused', 'fwd_keep_bytes', 'bwd_weight_ws', 'onehot_fwd_ws',
           'deconv_fwd_ws', 'deconv_bwd_data_ws', 'deconv_panel_bytes_fwd', 'deconv_panel_bytes_bwd', 'deconv_bwd_weight_ws',
           'resblock_supported', 'resblock_ws', 'resblock_bwd_weight_ws']
ACTS = {'none': A.ACT_NONE, 'relu': A.ACT_RELU, 'lrelu': A.ACT_LRELU, 'tanh': A.ACT_TANH}


def descriptors():
    """(B, Cin, H, W, Cout, k, stride, pad, pad_mode, act, n_onehot), in a fixed order."""
    from test_ops_gpu import CONV_CASES, DECONV_CASES, WINO_CASES, WINO4_CASES, ONEHOT_CASES
    out = []

    def add(B, Cin, H, W, Cout, k, s, p, pm='zero', act='none', nc=0):
        d = (B, Cin, H, W, Cout, k, s, p, pm, act, nc)
        if d not in out:
            out.append(d)

    for c in CONV_CASES:
        add(*c)
    for B, Cin, H, W, Cout, pm in WINO_CASES:
        add(B, Cin, H, W, Cout, 3, 1, 1, pm)
    for B, Cin, H, W, Cout in WINO4_CASES:
        add(B, Cin, H, W, Cout, 3, 1, 1)
    for B, Cin, H, W, Cout in DECONV_CASES:          # ConvTranspose2d 3x3 stride 2 pad 1 out_pad 1 = adjoint of this conv
        add(B, Cout, 2 * H, 2 * W, Cin, 3, 2, 1)
    for B, NC, Cd, H, W, Cout, k, pm in ONEHOT_CASES:
        add(B, NC + Cd, H, W, Cout, k, 1, k // 2, pm, 'none', NC)
    for Cd in (16, 64, 256):                         # one-hot stems whose dense part lands on other families
        add(2, 35 + Cd, 16, 32, 64, 3, 1, 1, 'reflect', 'none', 35)
    add(2, 41, 32, 64, 64, 4, 2, 2, 'zero', 'lrelu', 35)     # first PatchGAN conv on label ids

    # c2: GlobalGenerator ngf 64, 4 down, 9 blocks at 256x512, batch 8; 3-scale PatchGAN; VGG19 perceptual loss
    add(8, 38, 256, 512, 64, 7, 1, 3, 'reflect', 'none', 35)
    for i, c in enumerate((64, 128, 256, 512)):
        add(8, c, 256 >> i, 512 >> i, 2 * c, 3, 2, 1)                     # down convs; their adjoints = the up deconvs
    add(8, 1024, 16, 32, 1024, 3, 1, 1, 'reflect')
    add(8, 64, 256, 512, 3, 7, 1, 3, 'reflect', 'tanh')
    for sc in range(3):
        h, w = 256 >> sc, 512 >> sc
        for cin, cout, s, act in ((41, 64, 2, 'lrelu'), (64, 128, 2, 'none'), (128, 256, 2, 'none'), (256, 512, 1, 'none'),
                                  (512, 1, 1, 'none')):
            add(16, cin, h, w, cout, 4, s, 2, 'zero', act)
            h, w = (h + 4 - 4) // s + 1, (w + 4 - 4) // s + 1
    for cin, cout, div in ((3, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 2), (128, 256, 4), (256, 256, 4), (256, 512, 8),
                           (512, 512, 8), (512, 512, 16)):
        add(16, cin, 256 // div, 512 // div, cout, 3, 1, 1, 'zero', 'relu')
    # box2mask: two-stream mask generator + 2-scale PatchGAN at 256x256, batch 32
    add(32, 70, 256, 256, 64, 7, 2, 3)
    for i, c in enumerate((64, 128, 256)):
        add(32, c, 128 >> i, 128 >> i, 2 * c, 3, 2, 1)
    for pm in ('zero', 'reflect'):
        add(32, 512, 16, 16, 512, 3, 1, 1, pm)
        add(32, 256, 16, 16, 256, 3, 1, 1, pm)
    add(32, 64, 256, 256, 1, 7, 1, 3, 'reflect', 'none')
    h = 256
    for cin, cout, s in ((36, 64, 2), (64, 128, 2), (128, 256, 1), (256, 1, 1)):
        add(32, cin, h, h, cout, 4, s, 2)
        h = h // s + 1

    # ---- edges: channel thresholds (Cin 15..17, wino_fused_min_c 64, wino4_min_c 128, wino_fused_max_c 255, wino_min_c 256,
    # each +-1 and the next multiples of 8 / 16 around them) x planes with H or W of 2, 3, 4, odd and even
    chans = (15, 16, 17, 32, 56, 63, 64, 65, 72, 120, 127, 128, 129, 136, 240, 248, 255, 256, 257, 264, 272, 1024)
    for c in chans:
        for pm in ('zero', 'reflect'):
            add(2, c, 16, 32, c, 3, 1, 1, pm)
    for c in (16, 128, 256):
        for h, w in ((2, 2), (3, 3), (3, 4), (4, 4), (5, 7)):
            for pm in ('zero', 'reflect'):
                add(2, c, h, w, c, 3, 1, 1, pm)
    for cin, cout in ((64, 128), (128, 64), (256, 128), (1024, 512), (200, 136)):
        for pm in ('zero', 'reflect'):
            add(16, cin, 16, 32, cout, 3, 1, 1, pm)
    for cout in (1, 2, 3, 4, 5):                     # tiny heads, and the small-split head from 256 channels
        for cin in (15, 16, 17, 255, 256, 257):
            add(2, cin, 16, 32, cout, 3, 1, 1)
    for cout in (3, 4, 5):
        add(2, 256, 16, 32, cout, 7, 1, 3, 'reflect')
    for w in (127, 128):                             # B*OH*OW on / under 256*512: the small-split boundary ...
        add(8, 256, 128, w, 3, 3, 1, 1)
        add(8, 32, 128, w, 128, 3, 1, 1)             # ... and 1024 / 1016 tiles of 128x128: fast_ksplit's boundary
        add(8, 32, 128, w, 64, 3, 1, 1)
    for act in ('none', 'relu'):                     # few-tile layers: split-K, slabs handed to the norm only without act
        add(2, 64, 17, 33, 128, 4, 2, 2, 'zero', act)
        add(2, 256, 16, 32, 256, 3, 1, 1, 'reflect', act)
    for k, s, p in ((3, 2, 1), (4, 2, 1), (4, 2, 2), (1, 2, 0), (1, 1, 0), (5, 1, 2), (7, 2, 3)):
        add(2, 16, 16, 32, 16, k, s, p)
        add(2, 256, 9, 13, 512, k, s, p)
    add(2, 64, 16, 32, 64, 3, 2, 1, 'reflect')       # refused by check_conv (reflect needs stride 1): every query answers 0
    return out


def algos():
    """The default and every override tests/test_conv_abi_gpu.py runs (ROWS' 'over' and 'base', EXTRA_ROWS)."""
    import test_conv_abi_gpu as T
    out = [{}]
    for r in T.all_rows():
        for over in (r['over'], r.get('base') or {}):
            over = {k: v for k, v in sorted(over.items()) if v != 0}
            if over not in out:
                out.append(over)
    return out


def load(path=None):
    dll = ctypes.CDLL(path or A.LIB_PATH)
    for name, (res, args) in A._SIGS.items():
        if name.endswith(('_ws', '_bytes')) or name in ('him_conv2d_panel_layout', 'him_conv2d_bwd_data_shares_fwd_panel',
                                                        'him_conv2d_in_act_fused', 'him_resblock_supported'):
            fn = getattr(dll, name)
            fn.restype, fn.argtypes = res, args
    return dll


def answers(lib, d, over):
    B, Cin, H, W, Cout, k, s, p, pm, act, nc = d
    a = A.HimAlgo()
    for key, v in over.items():
        setattr(a, key, v)
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    c = A.HimConv2d(B, Cin, H, W, Cout, k, k, s, p, A.PAD_REFLECT if pm == 'reflect' else A.PAD_ZERO, OH, OW, ACTS[act], 0.2, a)
    # the transposed conv whose adjoint `c` is: it maps c's output space onto c's input space
    t = A.HimDeconv2d(B, Cout, OH, OW, Cin, k, k, s, p, H - ((OH - 1) * s - 2 * p + k), H, W, ACTS[act], 0.2, a)
    r = A.HimResBlock(B, Cin, H, W, 1e-5, a)
    block = Cin == Cout and (k, s, p, pm) == (3, 1, 1, 'reflect')
    cp, tp, rp = ctypes.byref(c), ctypes.byref(t), ctypes.byref(r)
    return [lib.him_conv2d_fwd_ws(cp), lib.him_conv2d_bwd_data_ws(cp), lib.him_conv2d_panel_bytes(cp, 0),
            lib.him_conv2d_panel_bytes(cp, 1), lib.him_conv2d_panel_layout(cp, 0), lib.him_conv2d_panel_layout(cp, 1),
            lib.him_conv2d_bwd_data_shares_fwd_panel(cp), lib.him_conv2d_in_act_fused(cp), lib.him_conv2d_fwd_keep_bytes(cp),
            lib.him_conv2d_bwd_weight_ws(cp), lib.him_conv2d_onehot_fwd_ws(cp, nc),
            lib.him_deconv2d_fwd_ws(tp), lib.him_deconv2d_bwd_data_ws(tp), lib.him_deconv2d_panel_bytes(tp, 0),
            lib.him_deconv2d_panel_bytes(tp, 1), lib.him_deconv2d_bwd_weight_ws(tp),
            lib.him_resblock_supported(rp) if block else 0, lib.him_resblock_ws(rp) if block else 0,
            lib.him_resblock_bwd_weight_ws(rp) if block else 0]


def table(lib):
    ds, als = descriptors(), algos()
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


def expand(tab):
    """{(descriptor index, algo index): values}"""
    return {(i, j): v for i, js, v in tab['rows'] for j in js}


def pack(tab):
    """The file form: one line per descriptor -- [descriptor, the default HimAlgo's values, [set, column, value, ...] per
    group of overrides that answer otherwise]; `sets` holds the groups' algo-index lists, each once."""
    sets, lines = [], []
    for i, d in enumerate(tab['descriptors']):
        groups = [(js, v) for k, js, v in tab['rows'] if k == i]
        base = groups[0][1]                          # the group of algo 0; its algo list is the rest
        line = [d, base]
        for js, v in groups[1:]:
            if js not in sets:
                sets.append(js)
            line.append([sets.index(js)] + [x for c, (a, b) in enumerate(zip(base, v)) if a != b for x in (c, b)])
        lines.append(line)
    return '{"columns": %s,\n "algos": %s,\n "sets": %s,\n "table": [\n%s\n]}\n' % (
        json.dumps(tab['columns']), json.dumps(tab['algos']), json.dumps(sets, separators=(',', ':')),
        ',\n'.join(json.dumps(ln, separators=(',', ':')) for ln in lines))


def unpack(f):
    """pack()'s inverse: the dict table() returns."""
    rows = []
    for i, line in enumerate(f['table']):
        base, others = line[1], []
        for g in line[2:]:
            v = list(base)
            v[:] = [dict(zip(g[1::2], g[2::2])).get(c, x) for c, x in enumerate(base)]
            others.append([i, f['sets'][g[0]], v])
        taken = {j for _, js, _ in others for j in js}
        rows += [[i, [j for j in range(len(f['algos'])) if j not in taken], base]] + others
    return {'columns': f['columns'], 'descriptors': [ln[0] for ln in f['table']], 'algos': f['algos'], 'rows': rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--lib', default=None, help='library to query (default: the built in-tree one)')
    ap.add_argument('-o', '--out', default=GOLDEN)
    args = ap.parse_args()
    tab = table(load(args.lib))
    with open(args.out, 'w') as f:
        f.write(pack(tab))
    with open(args.out) as f:
        assert expand(unpack(json.load(f))) == expand(tab)
    print('%d descriptors x %d algos -> %d rows, %d bytes: %s' % (len(tab['descriptors']), len(tab['algos']), len(tab['rows']),
                                                                 os.path.getsize(args.out), args.out))


if __name__ == '__main__':
    main()
