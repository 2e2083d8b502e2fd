"""ctypes binding of libhim_hip.so (the C ABI declared in include/him.h).

There is deliberately NO fallback: if the shared library is missing or a call fails the product raises.
The oracle (``oracle/``) is never imported from here.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libhim_hip.so')

c_float_p = C.c_void_p  # raw device pointers travel as integers
c_int, c_size_t, c_float, c_void_p, c_double = C.c_int, C.c_size_t, C.c_float, C.c_void_p, C.c_double


class HimAlgo(C.Structure):
    """Kernel-selection overrides carried by every descriptor (include/him.h "Algorithm selection"); zero = defaults."""
    _fields_ = [(n, c_int) for n in ('wino_min_c', 'wino_fused_min_c', 'wino_fused_max_c', 'wino4_min_c', 'ksplit_max',
                                     'tile_wb', 'tile_nb', 'wino_tblock', 'wgrad_splits')] + \
               [('disable', C.c_uint), ('wino_fused_chunk', c_int), ('wgrad_tile', c_int)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != 'reserved'}


# HimAlgo.disable bits / tile codes (include/him.h)
ALGO_NO_SPLITK, ALGO_NO_DFOLD, ALGO_WINO_PADDED_DGRAD, ALGO_NO_SMALL_WIN, ALGO_NO_FEWOUT_TILED, ALGO_NO_FEWIN_TILED, \
    ALGO_NO_FEWCH_MFMA, ALGO_GENERIC_CONV, ALGO_NO_RESBLOCK_FUSED, ALGO_FROZEN_WEIGHTS, ALGO_NO_BGEMM, ALGO_NO_ONEHOT_RLE = (1 << i for i in range(12))
ALGO_NO_FEWIN_FOLD = 1 << 12
ALGO_WINO4_TRAIN_FWD = 1 << 13
ALGO_NO_FEWIN_REFLECT = 1 << 14
ALGO_NO_WINO_FUSED2 = 1 << 15
ALGO_NO_BGEMM_PERSISTENT = 1 << 16
ONEHOT_PART_IDS, ONEHOT_PART_DENSE = 1, 2      # him_conv2d_onehot_bwd_weight_part
TILE_DEFAULT, TILE_128x128, TILE_128x128_8W, TILE_128x256, TILE_64x128, TILE_64x64, TILE_MIXED, TILE_128x64 = range(8)


class HimConv2d(C.Structure):
    _fields_ = [(n, c_int) for n in ('B', 'Cin', 'H', 'W', 'Cout', 'KH', 'KW', 'stride', 'pad', 'pad_mode',
                                     'OH', 'OW', 'act')] + [('slope', c_float), ('algo', HimAlgo)]


class HimDeconv2d(C.Structure):
    _fields_ = [(n, c_int) for n in ('B', 'Cin', 'H', 'W', 'Cout', 'KH', 'KW', 'stride', 'pad', 'out_pad',
                                     'OH', 'OW', 'act')] + [('slope', c_float), ('algo', HimAlgo)]


class HimResBlock(C.Structure):
    _fields_ = [(n, c_int) for n in ('B', 'C', 'H', 'W')] + [('eps', c_float), ('algo', HimAlgo)]


ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4
PAD_ZERO, PAD_REFLECT = 0, 1

P = c_void_p
_CONV, _DECONV, _RESB, _ALGO = C.POINTER(HimConv2d), C.POINTER(HimDeconv2d), C.POINTER(HimResBlock), C.POINTER(HimAlgo)

# name -> (restype, argtypes); int-returning entries are error-checked by the wrapper
_SIGS = {
    'him_version': (C.c_char_p, []),
    'him_arch': (C.c_char_p, []),
    'him_last_error': (C.c_char_p, []),
    'him_conv2d_fwd_ws': (c_size_t, [_CONV]),
    'him_conv2d_fwd': (c_int, [_CONV, P, P, P, P, P, c_size_t, P]),
    'him_conv2d_bwd_data_ws': (c_size_t, [_CONV]),
    'him_conv2d_bwd_data': (c_int, [_CONV, P, P, P, P, c_size_t, P]),
    'him_conv2d_bwd_weight_ws': (c_size_t, [_CONV]),
    'him_conv2d_bwd_weight': (c_int, [_CONV, P, P, P, P, c_int, P, c_size_t, P]),
    'him_deconv2d_fwd_ws': (c_size_t, [_DECONV]),
    'him_deconv2d_fwd': (c_int, [_DECONV, P, P, P, P, P, c_size_t, P]),
    'him_deconv2d_bwd_data_ws': (c_size_t, [_DECONV]),
    'him_deconv2d_bwd_data': (c_int, [_DECONV, P, P, P, P, c_size_t, P]),
    'him_deconv2d_bwd_weight_ws': (c_size_t, [_DECONV]),
    'him_deconv2d_bwd_weight': (c_int, [_DECONV, P, P, P, P, c_int, P, c_size_t, P]),
    # diagnostics: (descriptor, &family, &need_bytes, &splits, &tile_m, &tile_n)
    'him_conv2d_bwd_weight_plan': (c_int, [_CONV, C.POINTER(c_int), C.POINTER(c_size_t)] + [C.POINTER(c_int)] * 3),
    'him_deconv2d_bwd_weight_plan': (c_int, [_DECONV, C.POINTER(c_int), C.POINTER(c_size_t)] + [C.POINTER(c_int)] * 3),
    'him_algo_resolve': (None, [_ALGO, _ALGO]),
    'him_algo_from_env': (None, [_ALGO]),
    'him_conv2d_onehot_fwd_ws': (c_size_t, [_CONV, c_int]),
    'him_conv2d_onehot_fwd': (c_int, [_CONV, P, c_int, P, P, P, P, P, c_size_t, P]),
    'him_conv2d_onehot_bwd_weight_ws': (c_size_t, [_CONV, c_int]),
    'him_conv2d_onehot_bwd_weight': (c_int, [_CONV, P, c_int, P, P, P, P, c_int, P, c_size_t, P]),
    'him_conv2d_onehot_fwd_dense': (c_int, [_CONV, P, c_int, P, P, P, P, P, c_size_t, P]),
    'him_conv2d_onehot_bwd_weight_dense': (c_int, [_CONV, P, c_int, P, P, P, P, c_int, P, c_size_t, P]),
    'him_conv2d_onehot_bwd_weight_part': (c_int, [_CONV, P, c_int, P, c_int, P, P, P, c_int, P, c_size_t, c_int, P]),
    'him_winograd_gemm': (c_int, [P, P, P, c_int, c_int, c_int, _ALGO, P]),
    'him_conv2d_panel_bytes': (c_size_t, [_CONV, c_int]),
    'him_conv2d_bwd_data_shares_fwd_panel': (C.c_uint, [_CONV]),
    'him_conv2d_panel_layout': (C.c_uint, [_CONV, c_int]),
    'him_conv2d_panel_build': (c_int, [_CONV, c_int, P, P, c_size_t, P]),
    'him_conv2d_fwd_panel': (c_int, [_CONV, P, P, P, P, P, c_size_t, P]),
    'him_conv2d_bwd_data_panel': (c_int, [_CONV, P, P, P, P, c_size_t, P]),
    'him_conv2d_bwd_data_gated': (c_int, [_CONV, P, P, P, P, P, P, c_size_t, P]),
    'him_conv2d_fwd_keep_bytes': (c_size_t, [_CONV]),
    'him_conv2d_fwd_panel_keep': (c_int, [_CONV, P, P, P, P, P, P, c_size_t, P]),
    'him_conv2d_bwd_weight_kept': (c_int, [_CONV, P, P, P, P, c_int, P, c_size_t, P]),
    'him_deconv2d_panel_bytes': (c_size_t, [_DECONV, c_int]),
    'him_deconv2d_panel_build': (c_int, [_DECONV, c_int, P, P, c_size_t, P]),
    'him_deconv2d_fwd_panel': (c_int, [_DECONV, P, P, P, P, P, c_size_t, P]),
    'him_deconv2d_bwd_data_panel': (c_int, [_DECONV, P, P, P, P, c_size_t, P]),
    'him_batchnorm_ws': (c_size_t, [c_int]),
    'him_batchnorm_fwd': (c_int, [P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_float, c_float, c_int, c_int, c_float,
                                  P, c_size_t, P]),
    'him_batchnorm_bwd': (c_int, [P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_float, c_int, P,
                                  c_size_t, P]),
    'him_act_fwd': (c_int, [P, P, c_size_t, c_int, c_float, P]),
    'him_upsample2_fwd': (c_int, [P, P, c_int, c_int, c_int, c_int, P]),
    'him_upsample2_bwd': (c_int, [P, P, c_int, c_int, c_int, c_int, P]),
    'him_resize_compose': (c_int, [P, P, c_int, c_int, c_int, P, P, c_int, c_int, P, c_int, c_int, c_int, P]),
    'him_logsoftmax_fwd': (c_int, [P, P, c_int, c_int, c_int, P]),
    'him_logsoftmax_bwd': (c_int, [P, P, P, c_int, c_int, c_int, P]),
    'him_gate_comb_fwd': (c_int, [P, P, P, P, c_int, c_int, c_int, P]),
    'him_gate_comb_bwd': (c_int, [P, P, P, P, P, P, P, c_int, c_int, c_int, P]),
    'him_mask_loss_ws': (c_size_t, []),
    'him_masked_nll_fwd': (c_int, [P, P, P, P, c_int, c_int, c_int, P, c_size_t, P]),
    'him_masked_nll_bwd': (c_int, [P, P, P, P, P, c_int, c_int, c_int, P]),
    'him_bce_mean_fwd': (c_int, [P, P, c_size_t, P, P, c_size_t, P]),
    'him_space_to_batch': (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    'him_lr_control': (c_int, [P, P, c_float, P, P]),
    'him_class_mask': (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    'him_bce_mean_bwd': (c_int, [P, P, c_size_t, P, P, P]),
    'him_instnorm_fwd': (c_int, [P, P, P, P, P, c_int, c_int, c_float, c_int, c_float, P]),
    'him_conv2d_in_act_fused': (C.c_uint, [_CONV]),
    'him_conv2d_in_act_fwd': (c_int, [_CONV, P, P, P, P, P, P, P, P, P, c_float, c_int, c_float, P, c_size_t, P]),
    'him_instnorm_bwd': (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_float, P]),
    'him_act_bwd': (c_int, [P, P, P, c_size_t, c_int, c_float, P]),
    'him_add': (c_int, [P, P, P, c_size_t, P]),
    'him_onehot': (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P]),
    'him_onehot_pool3s2': (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    'him_u8_to_f32': (c_int, [P, P, c_size_t, P]),
    'him_data_nearest': (c_int, [P, P, P, P, P, c_int, P, c_int, c_int, c_int, c_int, P]),
    'him_data_nearest_rle': (c_int, [P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P]),
    'him_data_bicubic_h': (c_int, [P, P, P, P, P, P, P, c_int, P, c_int, c_int, c_int, P]),
    'him_data_bicubic_v': (c_int, [P, c_int, P, P, P, c_int, P, P, c_int, c_int, c_int, c_int, P]),
    'him_data_region_masks': (c_int, [P, P, c_int, P, P, P, P, P, P, P, P, P, c_int, c_int, c_int, P]),
    'him_canvas_window_bytes': (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    'him_canvas_paste_bicubic_v': (c_int, [P, P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    'him_canvas_paste_window': (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, c_int, c_int, P]),
    'him_tensor2im_bytes': (c_int, [P, c_int, c_int, c_int, c_int, P, P]),
    'him_label2color_bytes': (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, P, P]),
    'him_seglabel_bytes': (c_int, [P, c_int, c_int, c_int, P, P]),
    'him_inst_summary_workspace': (c_size_t, [c_int, c_int, c_int]),
    'him_inst_summary': (c_int, [P, c_int, P, c_int, c_int, c_int, c_int, c_int, P, P, P, c_size_t, P]),
    'him_ade_decode_workspace': (c_size_t, []),
    'him_ade_decode': (c_int, [P, c_int, c_int, c_int, P, c_int, P, P, P, P, P, P, c_size_t, P]),
    'him_image_metrics_workspace': (c_size_t, [c_int, c_int, c_int, c_int]),
    'him_image_metrics': (c_int, [P, P, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_float, P, P, P, P, c_size_t, P]),
    'him_confusion_workspace': (c_size_t, [c_int]),
    'him_confusion': (c_int, [P, c_int, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P,
                              c_size_t, P]),
    'him_label_instances_workspace': (c_size_t, [c_int, c_int, c_int]),
    'him_label_instances': (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, c_int, c_int, c_int, P, P, P, c_size_t, P]),
    'him_edt_workspace': (c_size_t, [c_int, c_int, c_int]),
    'him_edt': (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, P, P, P, P, c_size_t, P]),
    'him_boundary_stats_workspace': (c_size_t, [c_int, c_int, c_int]),
    'him_boundary_stats': (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, P, c_int, P, P, P, c_size_t, P]),
    'him_label_ids': (c_int, [P, c_int, c_int, c_int, c_int, c_int, P, P]),
    'him_bw_loss_ws': (c_size_t, []),
    'him_bw_nll_fwd': (c_int, [P, P, P, P, c_int, c_int, c_int, c_float, c_float, P, P, c_size_t, P]),
    'him_bw_nll_bwd': (c_int, [P, P, P, P, P, c_float, c_float, P, c_int, c_int, c_int, P]),
    'him_bw_pair_fwd': (c_int, [P, P, P, c_size_t, c_int, c_float, c_float, P, P, c_size_t, P]),
    'him_bw_pair_bwd': (c_int, [P, P, P, c_size_t, c_int, P, P, c_float, c_float, P, P]),
    'him_surface_fwd': (c_int, [P, P, P, P, c_int, c_int, c_int, P, P, c_size_t, P]),
    'him_surface_bwd': (c_int, [P, P, P, c_int, c_int, c_int, P, P, P]),
    'him_canvas_changed': (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, P]),
    'him_canvas_paste_blend_v': (c_int, [P, P, P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, P, c_int, c_int,
                                         c_int, P, P]),
    'him_membrane_basis': (c_int, [c_int, c_int, c_int, P, P, P, P]),
    'him_membrane_ws': (c_size_t, [c_int, c_int, c_int]),
    'him_membrane_solve': (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, P, P, P, P, P, P]),
    'him_canvas_seamless_apply': (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P, c_int, c_int, c_int, P,
                                          P]),
    'him_region_poisson_ws': (c_size_t, [c_int, c_int]),
    'him_region_poisson_solve': (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int, c_double, c_int, P, P, P,
                                         P, c_size_t, P]),
    'him_region_poisson_apply': (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    'him_layout_erase_workspace': (c_size_t, [c_int, c_int]),
    'him_layout_erase': (c_int, [P, c_int, P, c_int, P, c_int, c_int, c_int, P, c_int, P, P, P, P, P, c_size_t, P]),
    'him_layout_place': (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, c_int, P] +
                                [c_int] * 8 + [P, c_int, P, P, P]),
    'him_layout_place_affine': (c_int, [P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P] +
                                       [c_int] * 8 + [P, c_int, P, P, P]),
    'him_canvas_warp_affine': (c_int, [P, c_int, c_int, P, c_int, c_int, c_int, c_int, P, P]),
    'him_lap_levels': (C.c_uint, [c_int, c_int, c_int]),
    'him_lap_level_offset': (C.c_longlong, [c_int] * 5),
    'him_lap_pyramid_ws': (c_size_t, [c_int] * 5),
    'him_lap_pyramid': (c_int, [P] + [c_int] * 5 + [P, P, P, c_size_t, P]),
    'him_swd_gather_ws': (c_size_t, [c_int, c_int]),
    'him_swd_gather': (c_int, [P, c_int, c_int, c_int, c_int, P, c_int, P, C.c_longlong, C.c_longlong, P, P, P, c_size_t, P]),
    'him_swd_project': (c_int, [P, C.c_longlong, c_int, P, P, c_int, P, P, P]),
    'him_sort_segments_ws': (c_size_t, [C.c_longlong, C.c_longlong]),
    'him_sort_segments': (c_int, [P, C.c_longlong, C.c_longlong, P, P, c_size_t, P]),
    'him_swd_distance': (c_int, [P, C.c_longlong, P, C.c_longlong, c_int, P, P, P]),
    'him_feat_pool': (c_int, [P, c_int, c_int, c_int, c_int, P, C.c_longlong, C.c_longlong, c_int, c_int, P]),
    'him_feat_moments_ws': (c_size_t, [C.c_longlong, c_int]),
    'him_feat_moments': (c_int, [P, C.c_longlong, C.c_longlong, c_int, P, P, P, c_size_t, P]),
    'him_kid_sums_ws': (c_size_t, [c_int, c_int]),
    'him_kid_sums': (c_int, [P, C.c_longlong, P, C.c_longlong, c_int, P, P, c_int, c_int, C.c_double, C.c_double, P, P, P,
                             c_size_t, P]),
    'him_knn_radii_ws': (c_size_t, [C.c_longlong, c_int, c_int]),
    'him_knn_radii': (c_int, [P, C.c_longlong, c_int, c_int, P, P, P, c_size_t, P]),
    'him_knn_membership_ws': (c_size_t, [C.c_longlong, C.c_longlong, c_int]),
    'him_knn_membership': (c_int, [P, C.c_longlong, P, C.c_longlong, c_int, P, P, P, P, P, c_size_t, P]),
    'him_panoptic_match_workspace': (c_size_t, [c_int, c_int]),
    'him_panoptic_match': (c_int, [P, c_int, P, c_int, P, c_int, P, c_int, P] + [c_int] * 7 + [P, P, P, P, P, c_size_t, P]),
    'him_masked_image': (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, c_float, P]),
    'him_edges': (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P]),
    'him_masked_mean': (c_int, [P, P, P, P, c_int, c_int, P]),
    'him_tile_embed': (c_int, [P, P, P, c_int, c_int, c_int, c_int, P]),
    'him_copy_channels': (c_int, [P, c_int, c_int, P, c_int, c_int, c_int, c_int, c_int, P, c_int, c_int, P]),
    'him_blend': (c_int, [P, c_int, c_int, P, c_int, c_int, P, P, c_int, c_int, c_int, P]),
    'him_avgpool3s2_fwd': (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P]),
    'him_avgpool3s2_bwd': (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, P]),
    'him_maxpool_fwd': (c_int, [P, P, c_int, c_int, c_int, c_int, P]),
    'him_maxpool_bwd': (c_int, [P, P, P, c_int, c_int, c_int, c_int, P]),
    'him_maxpool_relu_bwd': (c_int, [P, P, P, c_int, c_int, c_int, c_int, P]),
    'him_reduce_ws': (c_size_t, [c_size_t]),
    'him_l1_mean_fwd': (c_int, [P, P, c_size_t, P, P, c_size_t, P]),
    'him_l1_mean_bwd': (c_int, [P, P, c_size_t, P, P, c_int, P]),
    'him_l1_multi_ws': (c_size_t, [c_int]),
    'him_l1_multi_fwd': (c_int, [P, P, P, c_int, P, P, c_size_t, P]),
    'him_l1_multi_bwd': (c_int, [P, P, P, c_int, P, P, c_int, P]),
    'him_lincomb_fwd': (c_int, [P, P, c_int, c_float, P, P]),
    'him_lincomb_bwd': (c_int, [P, P, c_int, c_float, P, P]),
    'him_mse_const_fwd': (c_int, [P, c_size_t, c_float, P, P, c_size_t, P]),
    'him_mse_const_bwd': (c_int, [P, c_size_t, c_float, P, P, c_int, P]),
    'him_resblock_supported': (C.c_uint, [_RESB]),
    'him_resblock_ws': (c_size_t, [_RESB]),
    'him_resblock_bwd_weight_ws': (c_size_t, [_RESB]),
    'him_resblock_fwd': (c_int, [_RESB, P, P, P, P, P, P, P, P, P, P, P, c_size_t, P]),
    'him_resblock_bwd_data': (c_int, [_RESB, P, P, P, P, P, P, P, P, P, P, P, c_size_t, P]),
    'him_resblock_bwd_weight': (c_int, [_RESB, c_int, P, P, P, P, c_int, P, c_size_t, P]),
    'him_adam_step': (c_int, [P, P, P, P, c_size_t, c_double, c_double, c_double, c_double, c_int, P]),
    'him_adam_ema_step': (c_int, [P, P, P, P, P, c_size_t, c_double, c_double, c_double, c_double, c_int, c_double, P]),
    'him_ema_update': (c_int, [P, P, c_size_t, c_double, P]),
    'him_swap': (c_int, [P, P, c_size_t, P]),
    'him_grad_stats_ws': (c_size_t, [c_size_t, c_int]),
    'him_grad_stats': (c_int, [P, c_size_t, P, c_int, P, P, c_double, P, c_size_t, P]),
    'him_adam_guarded_step': (c_int, [P, P, P, P, P, c_size_t, c_double, c_double, c_double, c_double, c_int, c_double, P,
                                      P]),
    'him_diffaug_ws': (c_size_t, [c_int, c_int, c_int]),
    'him_diffaug_fwd': (c_int, [P, P, P] + [c_int] * 8 + [P, c_size_t, P]),
    'him_diffaug_bwd': (c_int, [P, P, P] + [c_int] * 10 + [P, c_size_t, P]),
    'him_diffaug_draw': (c_int, [P, c_int, c_int, c_int, C.c_longlong, C.c_longlong, C.c_longlong, c_int, c_double,
                                 c_double, C.POINTER(c_int), C.POINTER(c_int), P]),
    'him_fill': (c_int, [P, c_size_t, c_float, P]),
    'him_scale': (c_int, [P, c_size_t, c_float, P]),
    'him_sn_ws': (c_size_t, [c_int, c_int]),
    'him_sn_power_iter_fwd': (c_int, [P, P, c_int, c_int, P, P, P, P, c_size_t, P]),
    'him_sn_power_iter_bwd': (c_int, [P, P, P, P, P, P, c_int, c_int, P, c_int, P, c_size_t, P]),
    'him_div_scalar_fwd': (c_int, [P, P, P, c_size_t, P]),
    'him_div_scalar_bwd': (c_int, [P, P, P, P, P, c_size_t, c_int, P, c_size_t, P]),
}

EXPORTS = sorted(_SIGS)


class HimError(RuntimeError):
    pass


class _Lib(object):
    def __init__(self):
        self._dll = None

    def _load(self):
        if self._dll is not None:
            return self._dll
        if not os.path.isfile(LIB_PATH):
            raise HimError('libhim_hip.so not built (%s): run `python -c "import __graft_entry__ as g; g.build()"` '
                           'or `make -C neurips18_hierchical_image_manipulation_amd/csrc` -- there is no CPU '
                           'fallback' % LIB_PATH)
        # torch FIRST: it ships its own libamdhip64 and the library must bind to THAT runtime (the device pointers and
        # streams it is handed live there).  Loaded before torch, libhim_hip.so pulls in /opt/rocm's copy instead: two HIP
        # runtimes in one process, and every launch on a torch stream fails with "no ROCm-capable device is detected"
        # (round 5: `python __graft_entry__.py smoke` = build() -- which loads the library -- and smoke() in ONE process).
        import torch  # noqa: F401
        dll = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(dll, name)          # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        self._dll = dll
        return dll

    def __getattr__(self, name):
        if name.startswith('_') or name not in _SIGS:
            raise AttributeError(name)
        dll = self._load()
        fn = getattr(dll, name)
        if _SIGS[name][0] is not c_int:
            return fn

        def checked(*a):
            rc = fn(*a)
            if rc != 0:
                raise HimError('%s failed (%d): %s' % (name, rc, dll.him_last_error().decode()))
            return rc
        checked.__name__ = name
        self.__dict__[name] = checked
        return checked


lib = _Lib()


def loaded_path():
    lib._load()
    return LIB_PATH
