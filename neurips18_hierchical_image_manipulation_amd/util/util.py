"""The reference's ``util/util.py``: ``load_script_to_opt`` (:46-63, the options a shell script would pass, parsed by an
options class) and the tensor -> picture helpers every driver and both models' ``get_current_visuals`` go through --
``tensor2im``, ``tensor2label``, ``tensor2seglabel``, ``labelcolormap``, ``Colorize``, ``save_image``, ``mkdirs``,
``mkdir`` -- with upstream's names, positional parameters and return values.

The three converters run on the device (``ops.tensor2im_bytes`` / ``label2color_bytes`` / ``seglabel_bytes``: one HIP pass
each) and return host ``numpy`` arrays: the only thing that crosses to the host is the finished ``uint8`` picture, copied
into a pinned buffer behind the current stream.  There is no host evaluation: a CPU tensor is moved to the device first.

Not carried over (Python-2 leftovers nothing in the drivers calls): ``load_image``, the first ``save_image`` (the one that
writes a JPEG through ``StringIO``; the second definition, kept here, shadows it upstream too), ``force_mkdir`` /
``force_rmdir`` / ``force_rmfile``, ``tensor2pil`` / ``pil2tensor`` (the canvas code crops and pastes on the device,
``util/data_util.py``)."""
import os
import re

import numpy as np
import torch


def load_script_to_opt(script_path, opt_class):
    """A one-line script passes everything after ``python <driver>.py``; a multi-line script (one ``--flag value \\`` per
    line) passes the lines whose first word is a flag the options class knows, minus the line's last word (the trailing
    backslash).  Quotes are dropped.  Same rules as upstream, indented lines and a final line without a backslash
    included."""
    dummy_opt = opt_class().parse(save=False, default_args=[])
    with open(script_path, 'r') as f:
        lines = f.readlines()
    if len(lines) == 1:
        options = [option.strip('\n') for option in lines[0].split(' ')[2:]]
    else:
        options = []
        for line in lines:
            option = re.sub('["\']', '', line).split(' ')
            if hasattr(dummy_opt, option[0].strip('--')):
                options += option[:-1]
    return opt_class().parse(save=False, default_args=options)


def _as_imtype(picture, imtype):
    """The device pass produces bytes; any other ``imtype`` is a widening of those bytes."""
    return picture if np.dtype(imtype) == np.uint8 else picture.astype(imtype)


def tensor2im(image_tensor, imtype=np.uint8, normalize=True):
    """(H, W, 3) picture of a (C, H, W) fp32 image tensor, C = 1 (written three times) or 3: ``(x + 1) / 2 * 255`` when
    ``normalize`` else ``x * 255``, clipped to [0, 255] and truncated.  A list gives the list of its pictures."""
    from .. import ops
    if isinstance(image_tensor, list):
        return [tensor2im(t, imtype, normalize) for t in image_tensor]
    return _as_imtype(ops.bytes_to_host(ops.tensor2im_bytes(image_tensor, normalize)), imtype)


def tensor2seglabel(label_tensor, imtype=np.uint8):
    """(H, W, C) array of a (C, H, W) tensor of values in [0, 255], truncated."""
    from .. import ops
    if torch.is_tensor(label_tensor) and label_tensor.dtype != torch.float32:
        label_tensor = label_tensor.float()
    return _as_imtype(ops.bytes_to_host(ops.seglabel_bytes(label_tensor)), imtype)


def tensor2label(label_tensor, n_label, imtype=np.uint8):
    """(H, W, 3) colour picture of a label tensor: (C, H, W) scores with C > 1 (the label is the channel of the maximum),
    a (1, H, W) id map, or an ``ops.LabelCond`` (its id map, batch entry 0).  ``n_label == 0``: an ordinary image."""
    from .. import ops
    if n_label == 0:
        return tensor2im(label_tensor, imtype)
    if torch.is_tensor(label_tensor) and label_tensor.dim() == 3 and label_tensor.shape[0] > 1 \
            and label_tensor.dtype != torch.float32:
        label_tensor = label_tensor.float()
    return _as_imtype(ops.bytes_to_host(ops.label2color_bytes(label_tensor, n_label)), imtype)


def save_image(image_numpy, image_path):
    from PIL import Image
    Image.fromarray(image_numpy).save(image_path)


def mkdirs(paths):
    if isinstance(paths, list):
        for path in paths:
            mkdir(path)
    else:
        mkdir(paths)


def mkdir(path):
    if not os.path.exists(path):
        os.makedirs(path)


# The public Cityscapes label definitions (cityscapesScripts, helpers/labels.py), ids 0..33 in order, then the licence
# plate (id -1 there, 34 in a 35-class map) and one white row for a 36th class.
_CITYSCAPES = (
    ('unlabeled', (0, 0, 0)), ('ego vehicle', (0, 0, 0)), ('rectification border', (0, 0, 0)), ('out of roi', (0, 0, 0)),
    ('static', (0, 0, 0)), ('dynamic', (111, 74, 0)), ('ground', (81, 0, 81)), ('road', (128, 64, 128)),
    ('sidewalk', (244, 35, 232)), ('parking', (250, 170, 160)), ('rail track', (230, 150, 140)),
    ('building', (70, 70, 70)), ('wall', (102, 102, 156)), ('fence', (190, 153, 153)), ('guard rail', (180, 165, 180)),
    ('bridge', (150, 100, 100)), ('tunnel', (150, 120, 90)), ('pole', (153, 153, 153)), ('polegroup', (153, 153, 153)),
    ('traffic light', (250, 170, 30)), ('traffic sign', (220, 220, 0)), ('vegetation', (107, 142, 35)),
    ('terrain', (152, 251, 152)), ('sky', (70, 130, 180)), ('person', (220, 20, 60)), ('rider', (255, 0, 0)),
    ('car', (0, 0, 142)), ('truck', (0, 0, 70)), ('bus', (0, 60, 100)), ('caravan', (0, 0, 90)), ('trailer', (0, 0, 110)),
    ('train', (0, 80, 100)), ('motorcycle', (0, 0, 230)), ('bicycle', (119, 11, 32)), ('license plate', (0, 0, 142)),
    ('extra', (255, 255, 255)))


def labelcolormap(N):
    """(N, 3) uint8 colours of N labels -- (36, 3) for N = 35 or 36, the Cityscapes palette.  Any other N: bit 3j of the
    label goes to red, bit 3j + 1 to green, bit 3j + 2 to blue, each at bit 7 - j of the colour, for j = 0..6 (the PASCAL
    VOC rule, one triple more)."""
    if N == 35 or N == 36:
        return np.array([rgb for _, rgb in _CITYSCAPES], dtype=np.uint8)
    ids = np.arange(N, dtype=np.int64)
    cmap = np.zeros((N, 3), dtype=np.uint8)
    for j in range(7):
        for ch in range(3):
            cmap[:, ch] |= (((ids >> (3 * j + ch)) & 1) << (7 - j)).astype(np.uint8)
    return cmap


class Colorize(object):
    """``Colorize(n)(label_map)``: the (3, H, W) ``ByteTensor`` colour picture of a (1, H, W) label map; labels outside
    [0, n) stay black.  ``cmap`` holds the first ``n`` rows of ``labelcolormap(n)``."""

    def __init__(self, n=35):
        self.cmap = torch.from_numpy(labelcolormap(n)[:n])

    def __call__(self, gray_image):
        from .. import ops
        picture = ops.bytes_to_host(ops.label2color_bytes(gray_image[:1], len(self.cmap)))
        return torch.from_numpy(np.ascontiguousarray(picture.transpose(2, 0, 1)))
