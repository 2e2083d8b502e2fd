"""Seeded inputs of the tensor -> picture cases shared by tests/golden/make_golden_vis.py (which records what the live
reference's util/util.py returns for them in tests/golden/vis_cases.npz) and the tests (which rebuild the inputs from the
same seeds).  numpy's legacy RandomState only: its streams do not change between releases."""
from collections import OrderedDict

import numpy as np


def _uniform(seed, shape, lo, hi):
    rs = np.random.RandomState(seed)
    return (rs.uniform(lo, hi, size=shape)).astype(np.float32)


def rounding_edge_values():
    """(3, 16, 16): x = k / 127.5 - 1 for k = 0..255 and its two fp32 neighbours -- the inputs whose (x + 1) / 2 * 255
    lands on or next to an integer, where rounding x + 1 first and a single fused multiply-add part ways."""
    k = np.arange(256, dtype=np.float64)
    x = (k / 127.5 - 1.0).astype(np.float32)
    lo = np.nextafter(x, np.float32(-np.inf), dtype=np.float32)
    hi = np.nextafter(x, np.float32(np.inf), dtype=np.float32)
    return np.stack([lo, x, hi]).reshape(3, 16, 16)


def id_map(seed, shape, hi):
    rs = np.random.RandomState(seed)
    return rs.randint(0, hi, size=shape).astype(np.float32)


def _ids_frac():
    a = id_map(21, (1, 64, 96), 41)
    a[0, 5, 7] = np.float32(7.5)
    a[0, 63, 95] = np.float32(33.999996)
    return a


def _tie23():
    a = np.zeros((4, 8, 8), np.float32)
    a[2:] = 1.0
    a[1, :4] = 1.0          # upper half: channels 1, 2, 3 tie -> 1; lower half: 2, 3 tie -> 2
    return a


# name -> (function, inputs (arrays or a list of arrays), keyword arguments of the upstream call)
CASES = OrderedDict([
    ('im_norm', ('tensor2im', _uniform(1, (3, 33, 65), -1.2, 1.2), dict(normalize=True))),
    ('im_plain', ('tensor2im', _uniform(2, (3, 64, 96), -0.1, 1.1), dict(normalize=False))),
    ('im_gray', ('tensor2im', _uniform(3, (1, 17, 20), -1.2, 1.2), dict())),
    ('im_list', ('tensor2im', [_uniform(4, (3, 8, 12), -1.0, 1.0), _uniform(5, (1, 5, 7), -1.0, 1.0)], dict())),
    ('im_edge', ('tensor2im', rounding_edge_values(), dict(normalize=True))),
    ('lab_scores35', ('tensor2label', np.random.RandomState(11).randn(35, 33, 65).astype(np.float32), dict(n_label=35))),
    ('lab_scores49', ('tensor2label', np.random.RandomState(12).randn(49, 32, 32).astype(np.float32), dict(n_label=49))),
    ('lab_tie_zeros', ('tensor2label', np.zeros((4, 8, 8), np.float32), dict(n_label=8))),
    ('lab_tie_23', ('tensor2label', _tie23(), dict(n_label=8))),
    ('lab_ids', ('tensor2label', id_map(20, (1, 64, 96), 41), dict(n_label=35))),
    ('lab_ids_frac', ('tensor2label', _ids_frac(), dict(n_label=35))),
    ('lab_n0', ('tensor2label', _uniform(6, (3, 12, 10), -1.0, 1.0), dict(n_label=0))),
    ('seg', ('tensor2seglabel', _uniform(7, (2, 9, 11), 0.0, 255.0), dict())),
    ('colorize', ('Colorize', id_map(22, (1, 16, 16), 41), dict(n=35))),
])

# the errors dictionary whose loss_log.txt line tests/golden/vis_api.json records (one entry is zero and is left out)
LOG_CALL = dict(epoch=3, i=120, t=0.4567,
                errors=[['G_GAN', 1.23456], ['G_GAN_Feat', 0], ['G_VGG', 10.5], ['D_real', 0.25], ['D_fake', 0.0004]])
