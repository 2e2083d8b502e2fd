"""Joint box -> layout -> image edit, host side: load_script_to_opt against the live reference's results
(tests/golden/joint_api.json, tests/golden/make_golden_joint.py), the public signatures, and sample_bbox's draws."""
import inspect
import json
import math
import os
import random

import numpy as np
import pytest

import joint_fixture
from neurips18_hierchical_image_manipulation_amd.models.joint_inference_model import JointInference
from neurips18_hierchical_image_manipulation_amd.options import BoxToMaskTestOptions, MaskToImageTestOptions
from neurips18_hierchical_image_manipulation_amd.util import data_util
from neurips18_hierchical_image_manipulation_amd.util.util import load_script_to_opt

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'joint_api.json')))


def _norm(v):
    return 'inf' if isinstance(v, float) and math.isinf(v) else v


@pytest.mark.parametrize('multiline', [False, True], ids=['one_line', 'multi_line'])
@pytest.mark.parametrize('which', ['box2mask', 'mask2image'])
def test_load_script_to_opt_matches_reference(tmp_path, which, multiline):
    sb, sm = joint_fixture.script_pair(str(tmp_path), multiline)
    path, cls = (sb, BoxToMaskTestOptions) if which == 'box2mask' else (sm, MaskToImageTestOptions)
    got = {k: _norm(v) for k, v in vars(load_script_to_opt(path, cls)).items()}
    want = GOLD['opts']['%s_%s' % (which, 'multi' if multiline else 'one')]
    diff = {k: (got.get(k, '<missing>'), v) for k, v in want.items() if got.get(k, '<missing>') != v}
    assert not diff, diff


def test_multiline_script_reads_only_unindented_flag_lines(tmp_path):
    """Upstream's rule: a line counts when its first word (split on single spaces) is a known flag, quotes dropped, its
    last word (the backslash) dropped -- an indented line is skipped."""
    p = tmp_path / 's.sh'
    p.write_text('python vis_box2mask.py \\\n--fineSize 64 \\\n  --label_nc 7 \\\n--name "q" \\\n\n')
    opt = load_script_to_opt(str(p), BoxToMaskTestOptions)
    default = BoxToMaskTestOptions().parse(save=False, default_args=[])
    assert (opt.fineSize, opt.name, opt.label_nc) == (64, 'q', default.label_nc)


def _params(fn):
    return [[p.name, None if p.default is inspect.Parameter.empty else p.default]
            for p in inspect.signature(fn).parameters.values()]


def test_signatures_match_reference():
    sigs = GOLD['signatures']
    assert _params(data_util.crop_canvas) == sigs['crop_canvas']
    assert _params(data_util.paste_canvas) == sigs['paste_canvas']
    assert _params(load_script_to_opt) == sigs['load_script_to_opt']
    for m in ('__init__', 'sample_bbox', 'sample_window', 'normalize_input', 'gen_layout', 'gen_image'):
        assert _params(getattr(JointInference, m)) == sigs['JointInference.' + m], m


class _Opt(object):
    min_box_size = 128


def test_sample_bbox_draws_once_from_numpy():
    """One np.random.choice over the boxes that reach min_box_size (all boxes if none does, or with random=True); the
    Python RNG is not touched."""
    boxes = [{'cls': 26, 'bbox': [0, 0, 50, 60]}, {'cls': 24, 'bbox': [10, 10, 200, 150]},
             {'cls': 33, 'bbox': [300, 100, 500, 400]}]
    ji = JointInference.__new__(JointInference)
    for rnd, given, pool in ((False, boxes, boxes[1:]), (True, boxes, boxes), (False, boxes[:1], boxes[:1])):
        np.random.seed(5)
        random.seed(5)
        got = ji.sample_bbox(given, _Opt(), random=rnd)
        after = (np.random.uniform(), random.random())
        np.random.seed(5)
        want = np.random.choice(pool)
        assert got == want
        assert after == (np.random.uniform(), random.Random(5).random())
