"""``crop_canvas`` / ``paste_canvas`` (reference util/data_util.py:8-120) on device canvases.

The reference round-trips the full-resolution canvas through ``ToPILImage`` / Pillow / ``ToTensor`` on the host.  Here
the canvas never leaves the device: the host decides the windows (the reference's own box arithmetic and random draws,
in its order) and the resampling tables (data/resample.py); the pixel work is csrc/him_data.hip
(``him_canvas_window_bytes`` -> ``him_data_nearest`` / ``him_data_bicubic_h`` -> ``him_data_bicubic_v`` /
``him_canvas_paste_bicubic_v``, ``him_data_region_masks``, ``him_canvas_paste_window``), bit-identical to the Pillow
path.  Departure: the returned dict holds DEVICE tensors where the reference returns host ``FloatTensor``s (the
window / box entries ``crop_pos``, ``cls``, ``output_bbox``, ``output_bbox_global`` stay on the host, as upstream)."""
import numpy as np
import torch

from .. import ops
from ..data import device as _device
from ..data import resample
from ..data.base_dataset import BICUBIC, NEAREST, get_soft_bbox, get_transform_params

CANVAS_XMAX, CANVAS_YMAX = 2047, 1023      # paste_canvas's literal clamps (a 1024 x 2048 Cityscapes canvas)


def _region_masks(label, box_in, box_out, fill):
    """get_masked_image(label, box_in, fill) and get_masked_image(label, box_out) of a (1,1,H,W) device map, one kernel:
    -> (mask_in, mask_ctx_in, mask_out)."""
    m = _device.region_masks(label.contiguous(), None, [[int(v) for v in box_in[:4]]], [[int(v) for v in box_out[:4]]],
                             [float(fill)], [None])
    return m[0], m[2], m[3]


def crop_canvas(bbox_sampled, label_original, opt, img_original=None, patch_to_obj_ratio=1.2, min_ctx_ratio=1.2,
                max_ctx_ratio=1.5, resize=True, transform_img=False):
    """The box's context window of the label canvas (1,1,H,W) -- and of the photo canvas (1,3,H,W) in [0,1] with
    ``transform_img`` -- at ``opt.fineSize`` plus the masks at that size and at the window's own resolution."""
    if opt.resize_or_crop != 'select_region':
        raise NotImplementedError('crop_canvas: --resize_or_crop select_region (got %s)' % opt.resize_or_crop)
    h, w = label_original.shape[2:4]
    config = {'prob_flip': 0.0, 'fineSize': opt.fineSize if resize else None, 'img_to_obj_ratio': opt.contextMargin,
              'patch_to_obj_ratio': patch_to_obj_ratio, 'min_ctx_ratio': min_ctx_ratio, 'max_ctx_ratio': max_ctx_ratio}
    params = get_transform_params((w, h), config=config, bbox=bbox_sampled, random_crop=False)
    box = resample.pil_crop_box(params['crop_pos'])
    out_w, out_h = (opt.fineSize, opt.fineSize) if resize else (box[2] - box[0], box[3] - box[1])

    output_dict = {}
    output_dict['label'] = ops.canvas_crop_nearest(label_original, box, out_h, out_w, pre=1)
    input_bbox = np.array(params['bbox_in_context'])
    crop_pos = np.array(params['crop_pos']).astype(int)
    bbox_cls = params['bbox_cls']
    img_size = out_h                                     # output_dict['label'].size(1) of the (1,H,W) label upstream
    context_ratio = np.random.uniform(low=config['min_ctx_ratio'], high=config['max_ctx_ratio'])
    output_bbox = np.array(get_soft_bbox(input_bbox, img_size, img_size, context_ratio))
    mask_in, mask_ctx_in, mask_out = _region_masks(output_dict['label'], input_bbox, output_bbox, bbox_cls)
    output_dict['mask_ctx_in'] = mask_ctx_in
    output_dict['mask_in'] = mask_in
    output_dict['mask_out'] = mask_out
    output_dict['crop_pos'] = torch.from_numpy(crop_pos)
    output_dict['cls'] = torch.LongTensor([bbox_cls])
    if transform_img:
        image = ops.canvas_crop_bicubic(img_original, box, out_h, out_w, normalize=True)
        output_dict['image'] = ops.cat_channels([image], mask_in, 2)          # image * (1 - mask_in)

    x1, y1, x2, y2 = crop_pos
    x1, y1 = max(0, x1), max(0, y1)
    width, height = x2 - x1 + 1, y2 - y1 + 1
    label_crop = label_original[:, :, y1:y2 + 1, x1:x2 + 1]
    input_bbox_orig = input_bbox.astype(float)
    input_bbox_orig = np.array([input_bbox_orig[0] / opt.fineSize * width, input_bbox_orig[1] / opt.fineSize * height,
                                input_bbox_orig[2] / opt.fineSize * width, input_bbox_orig[3] / opt.fineSize * height])
    output_bbox_orig = output_bbox.astype(float)
    output_bbox_orig = np.array([output_bbox_orig[0] / opt.fineSize * width,
                                 output_bbox_orig[1] / opt.fineSize * height,
                                 output_bbox_orig[2] / opt.fineSize * width,
                                 output_bbox_orig[3] / opt.fineSize * height])
    _, mask_ctx_in_orig, mask_out_orig = _region_masks(label_crop, input_bbox_orig, output_bbox_orig, bbox_cls)
    output_dict['label_orig'] = label_crop
    output_dict['mask_ctx_in_orig'] = mask_ctx_in_orig
    output_dict['mask_out_orig'] = mask_out_orig
    output_dict['output_bbox'] = torch.from_numpy(output_bbox)
    output_dict['output_bbox_global'] = torch.from_numpy(np.array([x1 + output_bbox_orig[0], y1 + output_bbox_orig[1],
                                                                   x1 + output_bbox_orig[2], y1 + output_bbox_orig[3]]))
    return output_dict


def _window(box_tensor):
    """``.int()`` of a host box (truncation toward zero), the lower corner clamped at 0 and the upper at the literal
    2047 / 1023, as upstream."""
    x1, y1, x2, y2 = (int(v) for v in box_tensor.int())
    return max(0, x1), max(0, y1), min(CANVAS_XMAX, x2), min(CANVAS_YMAX, y2)


def _slice_len(start, stop, size):
    """len(range(size)[start:stop]) for non-negative start (Python slice clipping)."""
    return max(0, min(stop, size) - min(start, size))


def _blend_args(original, feather, reach, profile, label_before, label_after, want_matte):
    """The blended paste's options, checked on the host before any device work -> None (``feather`` None: the hard
    paste) or (feather, reach, profile)."""
    if feather is None:
        if label_before is not None or label_after is not None or want_matte or reach != 0:
            raise ValueError('paste_canvas: reach / label_before / label_after / want_matte need feather')
        return None
    ops.matte_args(feather, reach, profile, 'paste_canvas')
    if (label_before is None) != (label_after is None):
        raise ValueError('paste_canvas: label_before and label_after come together')
    for name, lab in (('label_before', label_before), ('label_after', label_after)):
        if lab is not None and (lab.dim() != 4 or tuple(lab.shape[:2]) != (1, 1) or
                                tuple(lab.shape[2:]) != tuple(original.shape[2:])):
            raise ValueError('paste_canvas: %s %s is not a (1,1,%d,%d) label canvas of the photo canvas'
                             % (name, tuple(lab.shape), original.shape[2], original.shape[3]))
    return feather, reach, profile


def _paste_windows(original, cropped, info_dict):
    """``_paste_image``'s window arithmetic -> (x1, y1, width, height) on the canvas and (x3, y3, sw, sh) in the patch."""
    x1, y1, x2, y2 = _window(info_dict['output_bbox_global'])
    width, height = x2 - x1 + 1, y2 - y1 + 1
    x3, y3, x4, y4 = (int(v) for v in info_dict['output_bbox'].int())
    x3, y3 = max(0, x3), max(0, y3)
    ph, pw = cropped.shape[2], cropped.shape[3]
    sh, sw = _slice_len(y3, y4 + 1, ph), _slice_len(x3, x4 + 1, pw)
    Hc, Wc = original.shape[2], original.shape[3]
    if sh <= 0 or sw <= 0 or width <= 0 or height <= 0 or (_slice_len(y1, y2 + 1, Hc), _slice_len(x1, x2 + 1, Wc)) != \
            (height, width):
        raise ValueError('paste_canvas: a %dx%d patch window does not fit the %dx%d canvas window at (%d,%d)'
                         % (sw, sh, width, height, x1, y1))
    return (x1, y1, width, height), (x3, y3, sw, sh)


def _seamless_args(original, feather, reach, profile, label_before, label_after, want_matte):
    """The seamless paste's options, checked on the host before any device work: ``_blend_args``, and without ``feather``
    (membrane, alpha 1) the profile still has to be a known one."""
    if feather is None and profile not in ops.MATTE_PROFILES:
        raise ValueError('paste_canvas: profile %r (one of %s)' % (profile, ', '.join(ops.MATTE_PROFILES)))
    return _blend_args(original, feather, reach, profile, label_before, label_after, want_matte)


def _paste_image(original, cropped, info_dict, pre, *, feather=None, reach=0, profile='smooth', label_before=None,
                 label_after=None, want_matte=False):
    """The is_img branch: the ``output_bbox`` slice of ``cropped`` (1,3,fs,fs), ToPILImage of pre(v), BICUBIC to the
    global window, ToTensor, written into a clone of ``original``.

    ``feather`` (pixels, None: the hard rectangle above, unchanged) writes through a matte instead: it
    fades over ``feather`` pixels towards every side of the window with photograph behind it and, given the label canvas
    before and after the layout edit, from full strength within ``reach`` pixels of the pixels the edit changed to nothing
    at ``reach + feather`` (``canvas_changed`` -> ``distance_transform`` -> the blended paste); ``profile`` 'linear' or
    'smooth'.  ``want_matte``: -> (canvas, matte (1,1,H,W))."""
    blend = _blend_args(original, feather, reach, profile, label_before, label_after, want_matte)
    (x1, y1, width, height), (x3, y3, sw, sh) = _paste_windows(original, cropped, info_dict)
    raw = original.clone()
    if blend is None:
        ops.canvas_paste_bicubic(cropped.contiguous(), (x3, y3, x3 + sw, y3 + sh), raw, x1, y1, height, width, pre)
        return raw
    dist2 = None
    if label_before is not None:
        changed = ops.canvas_changed(label_before.contiguous(), label_after.contiguous(), x1, y1, height, width)
        dist2 = ops.distance_transform(changed, rule='nonzero')[0]
    _, matte = ops.canvas_paste_blend(cropped.contiguous(), (x3, y3, x3 + sw, y3 + sh), raw, x1, y1, height, width, pre,
                                      feather=feather, reach=reach, dist2=dist2, profile=profile, want_matte=want_matte)
    return (raw, matte) if want_matte else raw


def paste_canvas_feathered(original, cropped, info_dict, method=BICUBIC, resize=True, is_img=True, *, feather=None,
                           reach=0, profile='smooth', label_before=None, label_after=None, want_matte=False):
    """``paste_canvas`` with the blended image paste's options (see ``_paste_image``).  ``paste_canvas`` itself keeps the
    reference's exact parameter list, so the options live here; ``feather=None`` IS ``paste_canvas``.  A label paste
    (``is_img`` False) has nothing to blend: with ``feather`` it raises ValueError."""
    if feather is not None and not is_img:
        raise ValueError('paste_canvas: feather blends an image paste; a label map (is_img=False) is copied')
    blend = _blend_args(original, feather, reach, profile, label_before, label_after, want_matte)
    if blend is None:
        return paste_canvas(original, cropped, info_dict, method=method, resize=resize, is_img=is_img)
    if method != BICUBIC:
        raise NotImplementedError('paste_canvas(is_img=True): only Image.BICUBIC is on the HIP path')
    return _paste_image(original, cropped, info_dict, 0, feather=feather, reach=reach, profile=profile,
                        label_before=label_before, label_after=label_after, want_matte=want_matte)


def _paste_image_seamless(original, cropped, info_dict, pre, *, feather=None, reach=0, profile='smooth', label_before=None,
                          label_after=None, want_matte=False):
    """``_paste_image`` in the gradient domain: the patch is moved onto the photograph's values along the
    window's border by the membrane of ``ops.membrane_solve`` before it is written, so no offset in exposure or colour
    between generator and photograph survives.  ``feather=None``: the whole interior of the window is replaced (alpha 1);
    otherwise the matte of ``_paste_image`` decides where.  The membrane's status is left in ``info_dict['membrane']``."""
    _seamless_args(original, feather, reach, profile, label_before, label_after, want_matte)
    (x1, y1, width, height), (x3, y3, sw, sh) = _paste_windows(original, cropped, info_dict)
    ops.membrane_sides(original.shape[2], original.shape[3], x1, y1, height, width, 'paste_canvas_seamless')
    raw = original.clone()
    dist2 = None
    if label_before is not None:
        changed = ops.canvas_changed(label_before.contiguous(), label_after.contiguous(), x1, y1, height, width)
        dist2 = ops.distance_transform(changed, rule='nonzero')[0]
    _, matte, info_dict['membrane'] = ops.canvas_paste_seamless(
        cropped.contiguous(), (x3, y3, x3 + sw, y3 + sh), raw, x1, y1, height, width, pre, feather=feather, reach=reach,
        dist2=dist2, profile=profile, want_matte=want_matte)
    return (raw, matte) if want_matte else raw


def paste_canvas_seamless(original, cropped, info_dict, method=BICUBIC, resize=True, is_img=True, *, feather=None,
                          reach=0, profile='smooth', label_before=None, label_after=None, want_matte=False):
    """``paste_canvas_feathered``'s parameters, the image paste done in the gradient domain (see
    ``_paste_image_seamless``).  Here ``feather=None`` means "membrane, alpha 1".  A label paste (``is_img`` False) has no
    gradient domain: ValueError."""
    if not is_img:
        raise ValueError('paste_canvas_seamless: an image paste; a label map (is_img=False) is copied by paste_canvas')
    _seamless_args(original, feather, reach, profile, label_before, label_after, want_matte)
    if method != BICUBIC:
        raise NotImplementedError('paste_canvas(is_img=True): only Image.BICUBIC is on the HIP path')
    return _paste_image_seamless(original, cropped, info_dict, 0, feather=feather, reach=reach, profile=profile,
                                 label_before=label_before, label_after=label_after, want_matte=want_matte)


def paste_canvas(original, cropped, info_dict, method=NEAREST, resize=True, is_img=False):
    """Label map (``is_img`` False): ``cropped`` (1,C,h,w) copied into a clone of ``original`` at ``crop_pos``.  Image:
    see ``_paste_image`` (Pillow BICUBIC only: ``method`` must be ``Image.BICUBIC``, as the joint inference passes)."""
    if not is_img:
        x1, y1, x2, y2 = _window(info_dict['crop_pos'])
        Hc, Wc = original.shape[2], original.shape[3]
        want = (cropped.shape[1], _slice_len(y1, y2 + 1, Hc), _slice_len(x1, x2 + 1, Wc))
        if tuple(cropped.shape[1:]) != want:
            raise ValueError('paste_canvas: a %s label patch into a %s canvas window' % (tuple(cropped.shape[1:]), want))
        raw = original.clone()
        ops.canvas_paste_window(cropped[0:1], raw, x1, y1)
        return raw
    if method != BICUBIC:
        raise NotImplementedError('paste_canvas(is_img=True): only Image.BICUBIC is on the HIP path')
    return _paste_image(original, cropped, info_dict, 0)
