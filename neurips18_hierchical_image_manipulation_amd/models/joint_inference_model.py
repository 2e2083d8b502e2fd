"""``JointInference`` (reference models/joint_inference_model.py): a box with a class -> box2mask draws the object's
layout in the box's context window -> mask2image paints its pixels -> both are pasted back into the full canvases.

Both generators and all the canvas work run on the device (util/data_util.py); the host draws the same random numbers
as upstream, in the same order (``np.random.choice`` in ``sample_bbox``; per ``crop_canvas`` one ``random.random`` and
one ``np.random.uniform``).  Canvases are device tensors: label canvas (1,1,H,W) of class ids, photo canvas (1,3,H,W) in
[0,1] (``normalize_input``)."""
import numpy as np
import torch

from .. import ops
from .._cabi import HimError
from ..data.base_dataset import NEAREST, get_raw_transform_fn
from ..data.device import ImageTransform
from ..util.data_util import _blend_args, _paste_image, _paste_image_seamless, _seamless_args, crop_canvas, paste_canvas
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

    def gen_image_seamless(self, bbox_sampled, img_original, label_generated, opt, *, feather=None, reach=0,
                           profile='smooth', label_before=None):
        """``gen_image_feathered``'s parameters with the paste done in the gradient domain (util/data_util.py
        ``_paste_image_seamless``): the generated patch is moved onto the photograph's values along the
        window's border before it is written.  Here ``feather=None`` means "membrane, alpha 1": the whole interior of the
        window is replaced; with ``feather`` the matte of ``gen_image_feathered`` decides where and is left in
        ``input_dict['matte']``.  The membrane's status ``[sides mask, ny, nx, flags]`` (device int32) is left in
        ``input_dict['membrane']``."""
        # refuse bad options before crop_canvas draws its random numbers
        _seamless_args(img_original, feather, reach, profile, label_before,
                       None if label_before is None else label_generated, False)
        input_dict = crop_canvas(bbox_sampled, label_generated, opt, img_original=img_original, transform_img=True)
        with torch.no_grad():
            img_generated = self.G_mask2img.inference(input_dict['label'], torch.zeros_like(input_dict['label']),
                                                      input_dict['image'], input_dict['mask_in'],
                                                      input_dict['mask_out'])
        if feather is None:
            img_canvas = _paste_image_seamless(img_original, img_generated, input_dict, 2, profile=profile)
        else:
            img_canvas, input_dict['matte'] = _paste_image_seamless(
                img_original, img_generated, input_dict, 2, feather=feather, reach=reach, profile=profile,
                label_before=label_before, label_after=None if label_before is None else label_generated,
                want_matte=True)
        return img_canvas, input_dict, img_generated

    # -- edits of an object that is already in the scene: the layout edit is ops.layout_erase /
    # ops.layout_place, the photograph is repainted window by window with gen_image_feathered (``seamless``: with
    # gen_image_seamless) -------------------------------------------------------------------------------------------------
    def _edit_classes(self, fill, things):
        n_class = int(self.opt_maskgen.label_nc)
        if fill is None:
            things = ops.CITYSCAPES_THINGS if things is None else things
            things = set(int(c) for c in things)
            fill = tuple(c for c in range(n_class) if c not in things)
        return tuple(fill), n_class

    def _repaint(self, box, cls, img_canvas, label_before, label_after, opt, feather, reach, profile, seamless=False):
        bbox = {'bbox': [int(v) for v in box], 'cls': int(cls)}
        gen = self.gen_image_seamless if seamless else self.gen_image_feathered
        if feather is None:
            canvas, input_dict, _ = gen(bbox, img_canvas, label_after, opt)
        else:
            canvas, input_dict, _ = gen(bbox, img_canvas, label_after, opt, feather=feather, reach=reach, profile=profile,
                                        label_before=label_before)
        return canvas, input_dict

    def _erase(self, obj, label_original, inst_original, img_original, fill, things, feather, reach, profile):
        obj_id, box, cls = edit_object(obj)
        _blend_args(img_original, feather, reach, profile, None if feather is None else label_original,
                    None if feather is None else label_original, False)
        fill, n_class = self._edit_classes(fill, things)
        label_canvas, inst_canvas, _, status = ops.layout_erase(label_original, inst_original, obj_id, fill=fill,
                                                                n_class=n_class)
        erase = [int(v) for v in status.cpu().tolist()]
        if erase[3] & ops.LAYOUT_NO_SEED:
            raise HimError('JointInference: object %d cannot be removed: no pixel outside it has a class of the fill set %s'
                           % (obj_id, list(fill)))
        return obj_id, box, cls, label_canvas, inst_canvas, erase

    def remove_object(self, obj, label_original, inst_original, img_original, opt, *, fill=None, things=None, feather=None,
                      reach=0, profile='smooth', seamless=False):
        """Take the object ``obj`` (an item ``(id, {'bbox', 'cls'})`` of an ``inst_info`` / ``layout_info`` dict's
        ``'objects'``, or a dict with ``id``, ``bbox``, ``cls``) out of the scene: its pixels take label and instance id of
        the nearest pixel whose class is in ``fill`` (None: every class of the layout generator's ``label_nc`` that is not
        in ``things``, by default ``ops.CITYSCAPES_THINGS``), the box table is rebuilt, and the photograph is repainted
        over the object's box with ``gen_image_feathered`` (``feather`` / ``reach`` / ``profile`` as there; with
        ``feather`` only pixels near what the edit changed are touched; ``seamless``: with ``gen_image_seamless``, the
        repaint moved onto the photograph's values along the window's border).  -> ``(label_canvas, inst_canvas, img_canvas,
        info, report)``; ``report``: ``{'erase': [|R|, seeds, changed, flags], 'place': None, 'passes': [input_dict]}``.
        ``HimError`` when there is nothing to fill from: no canvas with the object still in it is returned."""
        from ..preprocess import inst_info
        _seamless_flag(seamless)
        _, box, cls, label_canvas, inst_canvas, erase = self._erase(obj, label_original, inst_original, img_original, fill,
                                                                    things, feather, reach, profile)
        info = inst_info(inst_canvas, label_canvas)
        img_canvas, input_dict = self._repaint(box, cls, img_original, label_original, label_canvas, opt, feather, reach,
                                               profile, seamless)
        return label_canvas, inst_canvas, img_canvas, info, {'erase': erase, 'place': None, 'passes': [input_dict]}

    def move_object(self, obj, dst_box, label_original, inst_original, img_original, opt, *, fill=None, things=None,
                    protect=(), new_id=None, feather=None, reach=0, profile='smooth', seamless=False,
                    keep_appearance=False, mixed=False):
        """Move ``obj`` to ``dst_box`` (``[xmin, ymin, xmax, ymax]`` inclusive, as ``obj``'s own ``bbox``; another size
        rescales the mask as Pillow's NEAREST resize would; the box may hang over the canvas): ``remove_object``'s erase on
        the originals, then the object's original mask is written at ``dst_box`` with its class and ``new_id`` (None: its
        own id), behind the pixels whose class is in ``protect``.  The photograph is repainted over the vacated box and
        then, on that result, over the box of the pixels written.  -> as ``remove_object``; ``report['place']``:
        ``[written, blocked, xmin, ymin, xmax, ymax]``, ``report['passes']`` one ``input_dict`` per repaint.

        ``keep_appearance``: the second pass is not a repaint: the object's own pixels, cut from the untouched original
        photograph at its box and resized to ``dst_box`` as Pillow's BICUBIC resize would, are Poisson-cloned onto the
        pixels ``layout_place`` wrote, the canvas after the first repaint being the boundary data
        (``ops.canvas_clone_region``; ``mixed``: per neighbour pair the stronger of the two gradients).  The
        pass's entry of ``report['passes']`` is then ``{'clone': status as host ints, 'resid': [...]}``."""
        try:
            dx0, dy0, dx1, dy1 = (int(v) for v in dst_box)
        except (TypeError, ValueError):
            raise ValueError('move_object: dst_box must be [xmin, ymin, xmax, ymax], got %r' % (dst_box,))
        if dx1 < dx0 or dy1 < dy0:
            raise ValueError('move_object: dst_box %r is empty' % (dst_box,))
        _seamless_flag(seamless)
        _clone_flags(keep_appearance, mixed)
        dst_excl = (dx0, dy0, dx1 + 1, dy1 + 1)                       # exclusive, as the ops take boxes

        def src_excl(box):
            return box[0], box[1], box[2] + 1, box[3] + 1

        def place(label_e, inst_e, obj_id, box, cls):
            return ops.layout_place(label_e, inst_e, inst_original, obj_id, src_excl(box), dst_excl, cls,
                                    obj_id if new_id is None else new_id, protect=protect)

        def clone(box, img_canvas, placed):
            return ops.canvas_clone_region(img_original, src_excl(box), img_canvas, dst_excl, placed, mixed=mixed)

        return self._replace(obj, label_original, inst_original, img_original, opt, place, clone, fill, things, feather,
                             reach, profile, seamless, keep_appearance)

    def _replace(self, obj, label_original, inst_original, img_original, opt, place_fn, clone_fn, fill, things, feather,
                 reach, profile, seamless, keep_appearance):
        """What ``move_object`` and ``transform_object`` share: the erase, ``place_fn(label_e, inst_e, id, box, cls)`` (a
        ``layout_place``), the box table, the repaint over the vacated box, then ``clone_fn(box, canvas, placed)`` (a
        ``canvas_clone_region``) or the repaint over the box of the pixels written."""
        from ..preprocess import inst_info
        obj_id, box, cls, label_e, inst_e, erase = self._erase(obj, label_original, inst_original, img_original, fill,
                                                               things, feather, reach, profile)
        label_canvas, inst_canvas, placed, status = place_fn(label_e, inst_e, obj_id, box, cls)
        place = [int(v) for v in status.cpu().tolist()]
        info = inst_info(inst_canvas, label_canvas)
        img_canvas, first = self._repaint(box, cls, img_original, label_original, label_canvas, opt, feather, reach, profile,
                                          seamless)
        passes = [first]
        if place[0] > 0 and keep_appearance:
            img_canvas, clone, resid = clone_fn(box, img_canvas, placed)
            passes.append({'clone': [int(v) for v in clone.cpu().tolist()], 'resid': [float(v) for v in resid.cpu().tolist()]})
        elif place[0] > 0:
            img_canvas, second = self._repaint(place[2:6], cls, img_canvas, label_original, label_canvas, opt, feather,
                                               reach, profile, seamless)
            passes.append(second)
        return label_canvas, inst_canvas, img_canvas, info, {'erase': erase, 'place': place, 'passes': passes}

    def rescale_object(self, obj, scale, label_original, inst_original, img_original, opt, *, seamless=False, **kw):
        """``move_object`` to ``scaled_box(obj's bbox, scale)``: the box scaled about its centre."""
        _, box, _ = edit_object(obj)
        return self.move_object(obj, scaled_box(box, scale), label_original, inst_original, img_original, opt,
                                seamless=seamless, **kw)

    def transform_object(self, obj, label_original, inst_original, img_original, opt, *, angle=0.0, scale=1.0, shear=0.0,
                         flip='', shift=(0, 0), fill=None, things=None, protect=(), new_id=None, feather=None, reach=0,
                         profile='smooth', seamless=False, keep_appearance=False, mixed=False):
        """Turn, mirror, shear or scale ``obj`` about the centre of its box and move that centre by ``shift``
        (``ops.affine_map``'s parameters and conventions: ``angle`` in degrees, counter-clockwise on the picture; below
        scale 1 the sampling aliases).  ``move_object``'s sequence with the affine place and the affine clone in the
        place of the separable ones: the erase on the originals, the object's original mask written
        through the map (``ops.layout_place_affine``), the box table, the repaint over the vacated box, then the repaint
        over the box of the pixels written or, with ``keep_appearance``, the object's own pixels warped bicubically
        through the same map and Poisson-cloned onto the pixels written (``ops.canvas_clone_region_affine``).
        -> as ``move_object``; ``report`` gains ``'affine': {'inv': [...], 'dst_box': [...]}``."""
        _seamless_flag(seamless)
        _clone_flags(keep_appearance, mixed)
        _, box, _ = edit_object(obj)
        amap = ops.affine_map((box[0], box[1], box[2] + 1, box[3] + 1), angle=angle, scale=scale, shear=shear, flip=flip,
                              shift=shift)
        def place(label_e, inst_e, obj_id, box, cls):
            return ops.layout_place_affine(label_e, inst_e, inst_original, obj_id, amap, cls,
                                           obj_id if new_id is None else new_id, protect=protect)

        def clone(box, img_canvas, placed):
            return ops.canvas_clone_region_affine(img_original, amap, img_canvas, placed, mixed=mixed)

        result = self._replace(obj, label_original, inst_original, img_original, opt, place, clone, fill, things, feather,
                               reach, profile, seamless, keep_appearance)
        result[4]['affine'] = {'inv': list(amap.inv), 'dst_box': list(amap.dst_box)}
        return result

    def rotate_object(self, obj, angle, label_original, inst_original, img_original, opt, **kw):
        """``transform_object`` with ``angle`` (degrees, counter-clockwise on the picture)."""
        return self.transform_object(obj, label_original, inst_original, img_original, opt, angle=angle, **kw)

    def flip_object(self, obj, axis, label_original, inst_original, img_original, opt, **kw):
        """``transform_object`` with ``flip=axis``: ``'x'`` mirrors left-right, ``'y'`` top-bottom, ``'xy'`` both."""
        return self.transform_object(obj, label_original, inst_original, img_original, opt, flip=axis, **kw)


def _clone_flags(keep_appearance, mixed):
    for name, v in (('keep_appearance', keep_appearance), ('mixed', mixed)):
        if not isinstance(v, bool):
            raise ValueError('%s must be True or False, got %r' % (name, v))
    if mixed and not keep_appearance:
        raise ValueError('mixed=True needs keep_appearance=True')


def _seamless_flag(seamless):
    if not isinstance(seamless, bool):
        raise ValueError('seamless must be True or False, got %r' % (seamless,))


def edit_object(obj):
    """(id, [xmin, ymin, xmax, ymax], cls) of an ``info['objects']`` item ``(id, {'bbox', 'cls'})`` or of a dict with
    ``id``, ``bbox`` and ``cls``."""
    try:
        if isinstance(obj, dict):
            obj_id, entry = obj['id'], obj
        else:
            obj_id, entry = obj
        box = [int(v) for v in entry['bbox'][:4]]
        obj_id, cls = int(obj_id), int(entry['cls'])
    except (TypeError, ValueError, KeyError, IndexError):
        raise ValueError("an object is an item (id, {'bbox': [xmin, ymin, xmax, ymax], 'cls': c}) of info['objects'] or a "
                         "dict with id, bbox and cls, got %r" % (obj,))
    if len(box) != 4 or box[2] < box[0] or box[3] < box[1]:
        raise ValueError('object %d: bbox %r is not [xmin, ymin, xmax, ymax]' % (obj_id, box))
    return obj_id, box, cls


def scaled_box(box, scale):
    """The inclusive box ``[xmin, ymin, xmax, ymax]`` with both sides multiplied by ``scale`` (rounded, at least one
    pixel) about its centre."""
    import math
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale) or scale <= 0:
        raise ValueError('scale must be a positive finite number, got %r' % (scale,))
    x0, y0, x1, y1 = (int(v) for v in box)
    w, h = x1 - x0 + 1, y1 - y0 + 1
    w2, h2 = max(1, int(round(w * scale))), max(1, int(round(h * scale)))
    nx0, ny0 = int(math.floor((x0 + x1 + 1 - w2) / 2.0)), int(math.floor((y0 + y1 + 1 - h2) / 2.0))
    return [nx0, ny0, nx0 + w2 - 1, ny0 + h2 - 1]

