"""``JointInference`` (reference models/joint_inference_model.py): a box with a class -> box2mask draws the object's
layout in the box's context window -> mask2image paints its pixels -> both are pasted back into the full canvases.

Both generators and all the canvas work run on the device (util/data_util.py); the host draws the same random numbers
as upstream, in the same order (``np.random.choice`` in ``sample_bbox``; per ``crop_canvas`` one ``random.random`` and
one ``np.random.uniform``).  Canvases are device tensors: label canvas (1,1,H,W) of class ids, photo canvas (1,3,H,W) in
[0,1] (``normalize_input``)."""
import numpy as np
import torch

from ..data.base_dataset import NEAREST, get_raw_transform_fn
from ..data.device import ImageTransform
from ..util.data_util import _blend_args, _paste_image, crop_canvas, paste_canvas
from ..util.util import load_script_to_opt


class JointInference(object):
    def __init__(self, joint_opt):
        from ..options import BoxToMaskTestOptions, MaskToImageTestOptions
        from .models import create_model
        self.opt_maskgen = load_script_to_opt(joint_opt.maskgen_script, BoxToMaskTestOptions)
        self.opt_imggen = load_script_to_opt(joint_opt.imggen_script, MaskToImageTestOptions)
        self.opt_maskgen.gpu_ids = self.opt_imggen.gpu_ids = joint_opt.gpu_ids
        self.G_box2mask = create_model(self.opt_maskgen)
        self.G_mask2img = create_model(self.opt_imggen)

    def sample_bbox(self, bbox_originals, opt, random=False):
        """A box whose longer side reaches ``opt.min_box_size`` (any box with ``random`` or when there is none)."""
        candidate_list = []
        for bbox in bbox_originals:
            xmin, ymin, xmax, ymax = bbox['bbox'][:4]
            if max(xmax - xmin, ymax - ymin) < opt.min_box_size:
                continue
            candidate_list.append(bbox)
        if not random and len(candidate_list) > 0:
            return np.random.choice(candidate_list)
        return np.random.choice(bbox_originals)

    def sample_window(self, img, label, bbox_sampled):
        pass

    def normalize_input(self, img, label, normalize_image=False):
        """PIL photo / label map -> device tensors as upstream: ToTensor (+ Normalize) of the photo (3,H,W), ToTensor * 255
        of the label map (1,H,W) (a mode 'L' / 'P' map: its ids as fp32).  The caller adds the batch axis, as
        vis_joint_inference.py does."""
        return get_raw_transform_fn(normalize=normalize_image)(img), \
            ImageTransform(None, None, NEAREST, False, True, False)(label) * 255.0

    def gen_layout(self, bbox_sampled, label_original, opt):
        """-> (label canvas with the generated layout pasted in, crop_canvas's dict, the layout at the window's size)."""
        input_dict = crop_canvas(bbox_sampled, label_original, opt)
        label_generated = self.G_box2mask.evaluate({
            'label_map': input_dict['label'], 'mask_ctx_in': input_dict['mask_ctx_in'],
            'mask_out': input_dict['mask_out'], 'mask_in': input_dict['mask_in'], 'cls': input_dict['cls'],
            'label_map_orig': input_dict['label_orig'], 'mask_ctx_in_orig': input_dict['mask_ctx_in_orig'],
            'mask_out_orig': input_dict['mask_out_orig']}, target_size=tuple(input_dict['label_orig'].shape[2:4]))
        label_canvas = paste_canvas(label_original, label_generated, input_dict, resize=False)
        return label_canvas, input_dict, label_generated

    def gen_image(self, bbox_sampled, img_original, label_generated, opt):
        """-> (photo canvas with the generated pixels pasted in, crop_canvas's dict, the generator's (1,3,fs,fs) output)."""
        return self.gen_image_feathered(bbox_sampled, img_original, label_generated, opt)

    def gen_image_feathered(self, bbox_sampled, img_original, label_generated, opt, *, feather=None, reach=0,
                            profile='smooth', label_before=None):
        """``gen_image`` (which keeps the reference's exact parameter list) with the blended paste's options
        (util/data_util.py ``_paste_image``).  ``feather=None`` IS ``gen_image``.  With ``feather`` the
        generated pixels enter the photo canvas through a matte, left in ``input_dict['matte']`` (1,1,H,W) (a picture
        through ``tensor2im(matte[0], normalize=False)``); with ``label_before``, the label canvas ``gen_layout`` was given
        (``label_generated`` being the one it returned), only pixels within ``reach + feather`` of what the layout edit
        changed are touched."""
        # refuse bad options before crop_canvas draws its random numbers
        _blend_args(img_original, feather, reach, profile, label_before, None if label_before is None else label_generated,
                    False)
        input_dict = crop_canvas(bbox_sampled, label_generated, opt, img_original=img_original, transform_img=True)
        with torch.no_grad():
            img_generated = self.G_mask2img.inference(input_dict['label'], torch.zeros_like(input_dict['label']),
                                                      input_dict['image'], input_dict['mask_in'],
                                                      input_dict['mask_out'])
        # paste_canvas(img_original, (img_generated + 1) / 2, input_dict, method=BICUBIC, is_img=True) with the
        # (x + 1) / 2 folded into the paste's quantisation (same fp32 operations)
        if feather is None:
            img_canvas = _paste_image(img_original, img_generated, input_dict, 2)
        else:
            img_canvas, input_dict['matte'] = _paste_image(
                img_original, img_generated, input_dict, 2, feather=feather, reach=reach, profile=profile,
                label_before=label_before, label_after=None if label_before is None else label_generated,
                want_matte=True)
        return img_canvas, input_dict, img_generated

