/*
 * him.h -- C ABI of libhim_hip.so: the MI355X (gfx950 / CDNA4) kernels under the mask2image
 * (layout-to-image GAN) training hot path of xcyan/neurips18_hierchical_image_manipulation.
 *
 * The reference has NO native/FFI boundary (it is 100 % Python on stock torch.nn modules); the
 * boundary this header defines sits directly beneath the reference's Python operator surface.  Each
 * entry point names the reference call sites it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain C, `extern "C"`; raw DEVICE pointers + sizes; no torch / hip types in signatures
 *     (`stream` is a hipStream_t passed as void*; NULL = the null stream).
 *   - every call is asynchronous on `stream`, never synchronises, never allocates: the caller owns
 *     all memory, including the scratch `ws` whose size the matching *_ws() query returns.
 *   - all tensors are fp32, NCHW, contiguous unless a (ptr, total-channels, first-channel) "channel
 *     slice" triple says otherwise.
 *   - return 0 on success, a negative HIM_E_* code on failure; him_last_error() (thread local) says why.
 */
#ifndef HIM_H_
#define HIM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIM_OK 0
#define HIM_E_INVALID (-1)   /* bad descriptor / argument */
#define HIM_E_WORKSPACE (-2) /* ws too small */
#define HIM_E_LAUNCH (-3)    /* HIP launch / runtime error */
#define HIM_E_UNSUPPORTED (-4)

/* activations fused into epilogues / norm kernels */
#define HIM_ACT_NONE 0
#define HIM_ACT_RELU 1  /* nn.ReLU        (models/Pix2Pix_NET.py:70) */
#define HIM_ACT_LRELU 2 /* nn.LeakyReLU(0.2) (models/Discriminator_NET.py:73) */
#define HIM_ACT_TANH 3  /* nn.Tanh        (models/Pix2Pix_NET.py:91) */
#define HIM_ACT_SIGMOID 4 /* nn.Sigmoid    (models/MaskTwoStreamConvSwitch_NET.py:22,206: object-mask head) */

#define HIM_PAD_ZERO 0    /* Conv2d(padding=p) */
#define HIM_PAD_REFLECT 1 /* nn.ReflectionPad2d(p) followed by Conv2d(padding=0) */

const char* him_version(void);
const char* him_arch(void); /* "gfx950" */
const char* him_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Conv2d family: fp32-MFMA (v_mfma_f32_32x32x2_f32) implicit GEMM, LDS-staged tiles.
 * Replaces nn.Conv2d (+ the nn.ReflectionPad2d in front of it, + bias, + the activation behind it)
 * at models/Pix2Pix_NET.py:74,78-79,91; models/layer_util.py:333-378 (ResnetBlock);
 * models/Discriminator_NET.py:69-93; models/layer_util.py:380-411 (Vgg19 conv3+ReLU).
 * ------------------------------------------------------------------------------------------- */
/* ---------------------------------------------------------------------------------------------
 * Algorithm selection.  The library holds NO mutable global state and reads NO environment variable on any compute or
 * size-query path: which kernel family a descriptor runs on -- and therefore its workspace size, its panel layout and
 * its fp32 summation order -- is a pure function of the descriptor, whose `algo` member carries the caller's overrides.
 * A zero-filled HimAlgo selects the defaults (what `him_algo_resolve` writes back); every entry point is re-entrant
 * across host threads, also with different HimAlgo values (tests/test_ops_gpu.py::test_library_is_reentrant).
 * Use ONE HimAlgo for the size query, the panel build and the launches of a layer.
 * (torch has no counterpart: cuDNN / MIOpen pick algorithms behind `torch.backends.cudnn.benchmark`; reference call
 * sites = every nn.Conv2d / nn.ConvTranspose2d of the path, see "Conv2d family" below.)
 * ------------------------------------------------------------------------------------------- */
#define HIM_TILE_DEFAULT 0   /* 64x128 (MxN) tiles: best inside the multi-stream training step */
#define HIM_TILE_128x128 1
#define HIM_TILE_128x128_8W 2
#define HIM_TILE_128x256 3   /* batched Winograd GEMM only */
#define HIM_TILE_64x128 4
#define HIM_TILE_64x64 5
#define HIM_TILE_MIXED 6     /* 128x128 when the launch has >= 512 (or 200..256) such tiles, else 128x64 */
#define HIM_TILE_128x64 7

#define HIM_ALGO_NO_SPLITK (1u << 0)        /* no split-K of few-tile conv / data-gradient launches */
#define HIM_ALGO_NO_DFOLD (1u << 1)         /* reflect-pad-1 3x3 data gradient through the padded gradient + fold pass */
#define HIM_ALGO_WINO_PADDED_DGRAD (1u << 2)/* Winograd reflect data gradient on the padded grid instead of folded border tiles */
#define HIM_ALGO_NO_SMALL_WIN (1u << 3)     /* tiny-M "same"-window weight gradient kernel off */
#define HIM_ALGO_NO_FEWOUT_TILED (1u << 4)  /* LDS-tiled VALU kernel for 2..4 output channels off */
#define HIM_ALGO_NO_FEWIN_TILED (1u << 5)   /* LDS-tiled VALU kernel for <= 4 reduction channels off */
#define HIM_ALGO_NO_FEWCH_MFMA (1u << 6)    /* MFMA weight gradient of the few-channel 5x5 / 7x7 layers off */
#define HIM_ALGO_GENERIC_CONV (1u << 7)     /* generic implicit-GEMM kernels instead of the buffer-load fast path */
#define HIM_ALGO_NO_RESBLOCK_FUSED (1u << 8)/* him_resblock_supported() answers 0 */
#define HIM_ALGO_NO_BGEMM (1u << 10)        /* batched Winograd GEMMs on the conv kernel instead of the LDS-DMA GEMM kernel */
#define HIM_ALGO_NO_ONEHOT_RLE (1u << 11)   /* one-hot stem weight gradient per pixel (round-1 kernel) instead of per run of equal class */
#define HIM_ALGO_NO_FEWIN_FOLD (1u << 12)    /* reflection-padded few-channel data gradient (generator head) through the padded
                                               gradient + reflect_fold pass instead of the fold inside the tiled kernel */
#define HIM_ALGO_NO_FEWIN_REFLECT (1u << 14) /* forward of a reflection-padded conv with <= 4 input channels (the dense channels of a
                                               generator stem: 3 -> 64, 7x7) on the generic implicit-GEMM kernel (K = 147 is too
                                               ragged for it: 0.55 ms at C2) instead of the tiled few-channel kernel (0.3 ms) */
#define HIM_ALGO_NO_WINO_FUSED2 (1u << 15)   /* fused Winograd launches on the round-2 kernel (one workgroup per spatial block, all
                                               waves producer + consumer) instead of the persistent wave-specialised kernel
                                               (csrc/him_wino_fused2.inc, round 6) */
#define HIM_ALGO_NO_BGEMM_PERSISTENT (1u << 16) /* F(4x4) GEMMs with K <= 256 on one workgroup per tile instead of the persistent
                                               form of the batched GEMM (csrc/him_bgemm.inc: bgemm_p_kernel, round 6) */
#define HIM_ALGO_WINO4_TRAIN_FWD (1u << 13)  /* OPT-IN, reduced-work variant: the FORWARD of trainable 3x3 s1 p1
                                               layers with >= wino4_min_c channels (the ResnetBlock stack) as Winograd
                                               F(4x4,3x3) -- 1.78x fewer multiplies than F(2x2), ~3e-6 instead of 5e-7 relative
                                               rounding per convolution; data / weight gradients stay F(2x2).  Never the
                                               default: reported as its own bench line (bench.py --variant) */
#define HIM_ALGO_FROZEN_WEIGHTS (1u << 9)   /* the layer's weights never change (VGG19 of the perceptual loss,
                                               models/layer_util.py:380-411): forward / data gradient may use Winograd
                                               F(4x4,3x3), whose 36-position panel is built once per run */

typedef struct HimAlgo {
  int wino_min_c;       /* 3x3 s1 p1 layers with Cin and Cout >= this run as separate-transform Winograd F(2x2,3x3);
                           0 = default (256); < 0: EVERY Winograd form off (all convolutions in the direct form) */
  int wino_fused_min_c; /* lower end of the fused single-launch Winograd kernel's channel range; 0 = default (64); < 0: off */
  int wino_fused_max_c; /* upper end; 0 = default (255) */
  int wino4_min_c;      /* FROZEN_WEIGHTS layers with Cin and Cout >= this AND at least 64 output tiles of 4x4 in the batch
                           (B*H*W >= 1024) run as F(4x4,3x3); 0 = default (128: VGG conv2_2 upwards; 256 until
                           the last session of round 5 -- in the step -0.34 ms, profiles/r05_ab_log.txt); < 0: off */
  int ksplit_max;       /* cap of the split-K factor; 0 = default (4; 8 until the last session of round 5: -0.24 ms in the step) */
  int tile_wb, tile_nb; /* HIM_TILE_*: batched Winograd GEMMs / direct-form convolutions */
  int wino_tblock;      /* threads per workgroup of the Winograd transform kernels: 64 (default), 128, 256 */
  int wgrad_splits;     /* fast weight-gradient kernel: split count; 0 = automatic */
  unsigned disable;     /* HIM_ALGO_* bits */
  int wino_fused_chunk; /* reduction channels per K-chunk of the fused Winograd kernel: 0 = default, 8 = the whole 160 KB of a CU's
                           LDS per workgroup (fastest alone: 0.54 ms at VGG conv1_2), 4 = 80 KB (0.69 ms alone, but the
                           workgroup shares its CU with the other streams' kernels inside the training step) */
  int wgrad_tile;       /* fast weight-gradient kernel: 0 = default (128x128 where M > 64 and C % 128 == 0: 74 KB of LDS, two
                           workgroups per CU), 1 = 64-row tiles (64x128: 55 KB), 2 = 64x64 tiles (37 KB: four per CU) */
} HimAlgo;
/* out = in with every 0 replaced by the default it selects (in == NULL: all defaults). */
void him_algo_resolve(const HimAlgo* in, HimAlgo* out);
/* Development aid for tools/: zero-fills *a, then applies the HIM_* environment overrides (HIM_NO_WINOGRAD,
 * HIM_WINO_MIN_C, HIM_NO_WINO_FUSED, HIM_WINO_FUSED_MIN_C / _MAX_C, HIM_WINO4_MIN_C, HIM_KSPLIT_MAX, HIM_NO_SPLITK,
 * HIM_GCONV_TILE[_WB|_NB], HIM_WINO_TBLOCK, HIM_WGRAD_SPLITS, HIM_NO_DFOLD, HIM_WINO_PADDED_DGRAD, HIM_NO_SMALL_WIN,
 * HIM_NO_FEWOUT_TILED, HIM_NO_FEWIN_TILED, HIM_NO_FEWCH_MFMA, HIM_GENERIC_CONV, HIM_NO_RESBLOCK_FUSED, HIM_NO_BGEMM, HIM_NO_ONEHOT_RLE,
 * HIM_NO_WINO_FUSED2, HIM_NO_BGEMM_PERSISTENT).  The ONLY place
 * the library reads the environment; nothing else calls it. */
void him_algo_from_env(HimAlgo* a);

typedef struct HimConv2d {
  int B, Cin, H, W;   /* input  (B,Cin,H,W) */
  int Cout, KH, KW;   /* weight (Cout,Cin,KH,KW) */
  int stride, pad;    /* symmetric stride / padding */
  int pad_mode;       /* HIM_PAD_ZERO | HIM_PAD_REFLECT */
  int OH, OW;         /* output (B,Cout,OH,OW); must equal (H+2p-K)/s+1 */
  int act;            /* epilogue activation applied by *_fwd */
  float slope;        /* LeakyReLU negative slope */
  HimAlgo algo;       /* kernel selection overrides; zero-filled = defaults */
} HimConv2d;

/* y = act(conv(x, w) + bias); bias may be NULL.  ws holds the tap-major regrouped weight tile stream. */
size_t him_conv2d_fwd_ws(const HimConv2d* d);
int him_conv2d_fwd(const HimConv2d* d, const float* x, const float* w, const float* bias, float* y, void* ws,
                   size_t ws_bytes, void* stream);
/* dx = conv^T(dy, w); dy is the gradient w.r.t. the PRE-activation output (see him_act_bwd). */
size_t him_conv2d_bwd_data_ws(const HimConv2d* d);
int him_conv2d_bwd_data(const HimConv2d* d, const float* dy, const float* w, float* dx, void* ws,
                        size_t ws_bytes, void* stream);
/* dw (+)= x (*) dy, dbias (+)= sum dy (dbias may be NULL).  accumulate!=0 adds into dw/dbias
 * (this is how the flat gradient arena receives several contributions per step). */
size_t him_conv2d_bwd_weight_ws(const HimConv2d* d);
int him_conv2d_bwd_weight(const HimConv2d* d, const float* x, const float* dy, float* dw, float* dbias,
                          int accumulate, void* ws, size_t ws_bytes, void* stream);

/* nn.ConvTranspose2d(k3,s2,p1,op1)+bias(+act): models/Pix2Pix_NET.py:89-90,185-188.
 * Computed as stride-phase sub-convolutions (no zero insertion). weight is (Cin,Cout,KH,KW). */
typedef struct HimDeconv2d {
  int B, Cin, H, W;
  int Cout, KH, KW;
  int stride, pad, out_pad;
  int OH, OW; /* (H-1)*s - 2p + K + out_pad */
  int act;
  float slope;
  HimAlgo algo;
} HimDeconv2d;
size_t him_deconv2d_fwd_ws(const HimDeconv2d* d);
int him_deconv2d_fwd(const HimDeconv2d* d, const float* x, const float* w, const float* bias, float* y,
                     void* ws, size_t ws_bytes, void* stream);
size_t him_deconv2d_bwd_data_ws(const HimDeconv2d* d);
int him_deconv2d_bwd_data(const HimDeconv2d* d, const float* dy, const float* w, float* dx, void* ws,
                          size_t ws_bytes, void* stream);
size_t him_deconv2d_bwd_weight_ws(const HimDeconv2d* d);
int him_deconv2d_bwd_weight(const HimDeconv2d* d, const float* x, const float* dy, float* dw, float* dbias,
                            int accumulate, void* ws, size_t ws_bytes, void* stream);
/* Diagnostics (pure host functions, no GPU): the plan him_conv2d_bwd_weight / him_deconv2d_bwd_weight run for a descriptor.
 * family: 0 Winograd F(2x2), 1 few-channel MFMA head (Cout <= 4), 2 few-channel MFMA stem (Cin <= 4), 3 small-window,
 * 4 small, 5 fast split-K GEMM, 6 generic split-K GEMM.  need_bytes: the workspace bytes that family touches, never more
 * than the slab region (*_bwd_weight_ws minus the dbias scratch behind it).  splits: partial results summed in fixed
 * order (split-K slabs / slices / slots / workgroups; 1: none).  tile_m x tile_n: the GEMM tile of families 5 and 6, else 0.
 * Any out pointer may be NULL.  Returns the descriptor's error code, like the call itself. */
int him_conv2d_bwd_weight_plan(const HimConv2d* d, int* family, size_t* need_bytes, int* splits, int* tile_m, int* tile_n);
int him_deconv2d_bwd_weight_plan(const HimDeconv2d* d, int* family, size_t* need_bytes, int* splits, int* tile_m, int* tile_n);

/* ---------------------------------------------------------------------------------------------
 * box2mask building blocks (second hot path, SURVEY 8 row a18: models/MaskTwoStreamConvSwitch_NET.py,
 * models/layer_util.py:128-250 ConvResnetBlock / DeconvResnetBlock, models/mask_losses.py).
 *   batchnorm: nn.BatchNorm2d(affine=True) of get_norm_layer('batch') (layer_util.py:19-21), training mode = batch
 *     statistics + running-statistics update (momentum, unbiased variance), eval mode = running statistics; fused with
 *     the activation behind it and an optional residual add.  gamma/beta may be NULL (affine=False).
 *     bwd: dgamma/dbeta (+)= when accumulate != 0; dx may be NULL.
 *   act_fwd: stand-alone nn.ReLU / LeakyReLU / Tanh / Sigmoid (the blocks start with an activation).
 *   upsample2: nn.Upsample(scale_factor=2, mode='bilinear') (layer_util.py:189,206); align_corners selects the
 *     torch >= 0.4 default (0) or the torch 0.3.1 behaviour (1).
 *   logsoftmax: nn.LogSoftmax(dim=1) over the channel axis (MaskTwoStreamConvSwitch_NET.py:21,196).
 *   masked_nll: MaskReconLoss = NLLLoss2d(ignore_index) with the positions where mask < 0.5 ignored
 *     (mask_losses.py:12-27); out2 = {loss, #valid positions}.   bce_mean: nn.BCELoss() (TwoStreamAE_mask.py:53).
 * -------------------------------------------------------------------------------------------*/
size_t him_batchnorm_ws(int C);
int him_batchnorm_fwd(const float* x, const float* residual, const float* gamma, const float* beta, float* run_mean,
                      float* run_var, float* y, float* save_mean, float* save_rstd, int B, int C, int hw, float eps,
                      float momentum, int training, int act, float slope, void* ws, size_t ws_bytes, void* stream);
int him_batchnorm_bwd(const float* x, const float* gamma, const float* beta, const float* save_mean,
                      const float* save_rstd, const float* dy, float* dx, float* dgamma, float* dbeta, int B, int C,
                      int hw, int training, int act, float slope, int accumulate, void* ws, size_t ws_bytes,
                      void* stream);
int him_act_fwd(const float* x, float* y, size_t n, int act, float slope, void* stream);
int him_upsample2_fwd(const float* x, float* y, int planes, int H, int W, int align_corners, void* stream);
int him_upsample2_bwd(const float* dy, float* dx, int planes, int H, int W, int align_corners, void* stream);
/* TwoStreamAE_mask.evaluate(target_size) (reference models/TwoStreamAE_mask.py:318-335): the generator's low-resolution
 * probabilities comb_prob (1,C,h,w) and obj_prob (1,1,h,w) (already gated by the low-resolution mask_out under
 * --use_output_gate) sampled bilinearly at the (H,W) of the original crop (align_corners as upsample_align_corners,
 * same source positions as him_upsample2_fwd) and composed with label (1,1,H,W) in one pass; the upsampled C-channel
 * tensor and the one-hot of the label are never written.
 *   background 0 (cls != label_nc-1): dst f32 = obj > .5 ? cls : label;           comb_prob / mask_out may be NULL.
 *   background 1 (cls == label_nc-1): dst i64 = argmax_c (p_c * m + (1 - m) * [label == c]), m = mask_out (1,1,H,W),
 *                                     the first index wins ties (torch.max(dim)); obj_prob may be NULL. */
int him_resize_compose(const float* comb_prob, const float* obj_prob, int C, int h, int w, const float* label,
                       const float* mask_out, int cls, int background, void* dst, int H, int W, int align_corners,
                       void* stream);
int him_logsoftmax_fwd(const float* x, float* y, int B, int C, int hw, void* stream);
int him_logsoftmax_bwd(const float* y, const float* dy, float* dx, int B, int C, int hw, void* stream);
/* MaskTwoStreamConv_NET.py:213-221 (the generator the parser builds without --no_comb): the context stream's logits gated
 * by the object stream's probability, comb = (1 - p) * ctx + p * obj with p, obj (B,1,hw) broadcast over ctx's C channels
 * (products and sum rounded one by one: torch's values).  bwd: dctx (B,C,hw), dp and dobj (B,1,hw). */
int him_gate_comb_fwd(const float* ctx, const float* p, const float* obj, float* out, int B, int C, int hw, void* stream);
int him_gate_comb_bwd(const float* ctx, const float* p, const float* obj, const float* dout, float* dctx, float* dp,
                      float* dobj, int B, int C, int hw, void* stream);
size_t him_mask_loss_ws(void);
int him_masked_nll_fwd(const float* logp, const float* label, const float* mask, float* out2, int B, int C, int hw,
                       void* ws, size_t ws_bytes, void* stream);
int him_masked_nll_bwd(const float* label, const float* mask, const float* g, const float* count, float* dlogp, int B,
                       int C, int hw, void* stream);
int him_bce_mean_fwd(const float* p, const float* t, size_t n, float* out, void* ws, size_t ws_bytes, void* stream);
int him_bce_mean_bwd(const float* p, const float* t, size_t n, const float* g, float* dp, void* stream);
/* The ADE recipe of box2mask (scripts/train_box2mask_ade.sh: --add_dilated_layers --lr_control):
 *   space_to_batch: y[(b*d+py)*d+px][c][i][j] = x[b][c][i*d+py][j*d+px] (inverse != 0: the reverse copy).  The dilated
 *     bias-free conv3x3 of DilatedResnetBlock (models/layer_util.py:254-293, dilation = padding = d) is the plain pad-1
 *     conv on the d*d phase images, so it runs on the same MFMA / Winograd kernels as every other 3x3 layer.
 *   lr_control: models/Discriminator_NET.py:190-211 on device scalars, out2 = {g_lr, d_lr} (no host read-back). */
int him_space_to_batch(const float* x, float* y, int B, int C, int H, int W, int d, int inverse, void* stream);
int him_lr_control(const float* loss_d_real, const float* loss_d_fake, float margin, float* out2, void* stream);
/* box2mask condition, object half (models/TwoStreamAE_mask.py:127-152): dst[b][c0+c][px] = (c == cls[b]) ? mask[b][px] : 0
 * for c in [0, NC); cls = one class id per sample as a float on the device. */
int him_class_mask(const float* mask, const float* cls, float* dst, int B, int NC, int Ctot, int c0, int hw, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One-hot stems: conv over [one-hot(label) | dense channels] evaluated from the label ids.  `label` is the
 * (B,1,H,W) float id map (data/segmentation_dataset.py:82), channels [0, n_onehot) of x are its one-hot encoding
 * (him_onehot; reference encode_input models/pix2pixHD_condImg_model.py:150-155) and are never read; channels
 * [n_onehot, Cin) are ordinary dense inputs.  Replaces nn.Conv2d(input_nc, ngf, 7) of models/Pix2Pix_NET.py:74-76
 * (GlobalGenerator stem) and :137-140 (two-stream label encoder stem).  stride 1, odd square kernel, pad = K/2
 * (zero or reflect) -- or, round 5, 4x4 stride 2 zero-padded (see below) --, Cout % 16 == 0; *_ws returns 0 when the
 * descriptor is not eligible (use him_conv2d_*).
 * No data gradient: the stem input is data.
 * -------------------------------------------------------------------------------------------*/
size_t him_conv2d_onehot_fwd_ws(const HimConv2d* d, int n_onehot);
int him_conv2d_onehot_fwd(const HimConv2d* d, const float* label, int n_onehot, const float* x, const float* w,
                          const float* bias, float* y, void* ws, size_t ws_bytes, void* stream);
size_t him_conv2d_onehot_bwd_weight_ws(const HimConv2d* d, int n_onehot);
int him_conv2d_onehot_bwd_weight(const HimConv2d* d, const float* label, int n_onehot, const float* x,
                                 const float* dy, float* dw, float* dbias, int accumulate, void* ws, size_t ws_bytes,
                                 void* stream);
/* Round 5.  (1) The same pair for the first PatchGAN convolution of scale 0 -- nn.Conv2d(input_nc, ndf, 4, stride 2,
 * padding 2) of models/Discriminator_NET.py:71-74 applied to cat(one-hot | cond image | real-or-fake image)
 * (pix2pixHD_condImg_model.py:149-152,176-186): 4x4, stride 2, zero padding is eligible too (*_ws != 0); forward = 16
 * table lookups per output pixel, weight gradient in the run-length form (one difference of two prefix sums of a dy row per
 * (run of equal class, tap), output columns ceil((x0 - tw) / 2) .. ceil((x1 - tw) / 2)).  (2) *_dense: the dense channels
 * arrive as their OWN tensor xdense (B, Cin - n_onehot, H, W) (NULL when Cin == n_onehot): the (B, Cin, H, W) concatenation
 * -- 147 MB of one-hot at 512x256 bs 8, written and re-read by three discriminator passes per step -- never exists.
 * Workspace sizes are those of the plain pair. */
int him_conv2d_onehot_fwd_dense(const HimConv2d* d, const float* label, int n_onehot, const float* xdense, const float* w,
                                const float* bias, float* y, void* ws, size_t ws_bytes, void* stream);
int him_conv2d_onehot_bwd_weight_dense(const HimConv2d* d, const float* label, int n_onehot, const float* xdense,
                                       const float* dy, float* dw, float* dbias, int accumulate, void* ws,
                                       size_t ws_bytes, void* stream);
/* (3) The weight gradient in two independently launchable parts, for callers that own two streams: HIM_ONEHOT_PART_IDS = the
 * label-id channels' slice of dw (run-length kernel: LDS-bound, one workgroup per CU, 1.1 ms at the generator stem of
 * 512x256 bs 8), HIM_ONEHOT_PART_DENSE = the dense channels' slice of dw (an MFMA weight gradient) + dbias.  The parts write
 * disjoint elements of dw and use disjoint regions of ws; on two streams they run next to each other (the stem's weight
 * gradient is the LAST kernel chain of the generator's backward, netG.model[1] of models/Pix2Pix_NET.py:74, and what the
 * next step's generator forward waits for).  x: the (B, Cin, H, W) concatenation, or the dense channels alone when
 * x_is_dense != 0.  parts == IDS | DENSE is the one-call form above. */
#define HIM_ONEHOT_PART_IDS 1
#define HIM_ONEHOT_PART_DENSE 2
int him_conv2d_onehot_bwd_weight_part(const HimConv2d* d, const float* label, int n_onehot, const float* x, int x_is_dense,
                                      const float* dy, float* dw, float* dbias, int accumulate, void* ws, size_t ws_bytes,
                                      int parts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weight panels.  The MFMA kernels read the weights regrouped (forward: [Cout][Cin/16][KH][KW][16]; data
 * gradient: the transpose, per stride phase).  The plain entry points above rebuild that panel inside the
 * workspace on EVERY launch (75 MB of HBM traffic for a 1024x1024x3x3 ResnetBlock conv); weights only change
 * once per optimizer step, so a trainer builds each panel once after the Adam update (on a side stream, under
 * the other network's backward) and calls the *_panel variants.  torch.nn has no counterpart: cuDNN/MIOpen
 * hide the same transform inside their "find"/workspace logic (reference call sites: every nn.Conv2d /
 * nn.ConvTranspose2d of models/Pix2Pix_NET.py:63-135, models/Discriminator_NET.py:62-125,
 * models/layer_util.py:340-378,400-440).
 *   kind HIM_PANEL_FWD      -> consumed by him_conv2d_fwd_panel      / him_deconv2d_fwd_panel
 *   kind HIM_PANEL_BWD_DATA -> consumed by him_conv2d_bwd_data_panel / him_deconv2d_bwd_data_panel
 * *_panel_bytes returns 0 when that kernel reads the raw weights (Cout <= 4 heads, Cin < 16 stems):
 * use the plain entry point.  Workspace sizes are those of the plain entry points.
 * -------------------------------------------------------------------------------------------*/
/* 3x3 stride-1 pad-1 convs with Cin and Cout >= HimAlgo.wino_min_c channels (default 256) run as Winograd F(2x2,3x3):
 * transforms + ONE batched fp32-MFMA GEMM over the 16 transform positions (2.25x fewer multiplies; fp32 rounding differs
 * from the direct form at the 1e-6 level).  The data and weight gradients of those layers use the same scheme.  Workspace
 * / panel sizes follow the descriptor's HimAlgo: a cached panel belongs to the HimAlgo it was built with. */

/* Stage 2 of the Winograd convolution on its own: c[z][m][n] = sum_k a[z][m][k] * b[z][k][n] for the 16 transform
 * positions z (a: [16][M][K] weight/gradient panels, b: [16][K][N], c: [16][M][N]; K % 16 == 0, N % 128 == 0).
 * This is the launch the roofline in bench.py is measured on (fp32 MFMA, 2*16*M*K*N executed FLOP).  algo: tile_wb is
 * read (NULL = defaults). */
int him_winograd_gemm(const float* a, const float* b, float* c, int M, int K, int N, const HimAlgo* algo, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ResnetBlock  out = x + IN(conv3x3(refpad(relu(IN(conv3x3(refpad(x)))))))  with both InstanceNorms fused into the
 * Winograd transforms of the two convolutions: reference models/layer_util.py:333-378 (ResnetBlock.build_conv_block /
 * forward) with norm_layer = InstanceNorm2d(affine=False) (:19-26), as built by GlobalGenerator
 * (models/Pix2Pix_NET.py:82-84).  Statistics are reduced in the output transform, the normalisation + ReLU is applied on
 * load by the next input transform (the normalised tensor is never written), the tail norm + residual in the second
 * output transform; backward applies the ReLU gate + InstanceNorm backward in the data gradient's output transform.
 * Supported: the separate-transform Winograd range (C above the fused kernel's, C % 128 == 0), even planes >= 4x4 with
 * H*W <= 4096; him_resblock_supported() tells.  panel*: HIM_PANEL_FWD / HIM_PANEL_BWD_DATA panels of the 3x3 reflect-pad
 * conv descriptor (him_conv2d_panel_build).  stat*: [mean(B*C) | rstd(B*C)].  y1 / y2: raw conv outputs (+bias).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int B, C, H, W;
  float eps;
  HimAlgo algo;
} HimResBlock;
int him_resblock_supported(const HimResBlock* d);
size_t him_resblock_ws(const HimResBlock* d);
size_t him_resblock_bwd_weight_ws(const HimResBlock* d);
int him_resblock_fwd(const HimResBlock* d, const float* x, const void* panel1, const float* bias1, const void* panel2,
                     const float* bias2, float* y1, float* stat1, float* y2, float* stat2, float* out, void* ws,
                     size_t ws_bytes, void* stream);
int him_resblock_bwd_data(const HimResBlock* d, const float* g_out, const float* y1, const float* stat1, const float* y2,
                          const float* stat2, const void* panel1_bwd, const void* panel2_bwd, float* dy2, float* dy1,
                          float* dx, void* ws, size_t ws_bytes, void* stream);
int him_resblock_bwd_weight(const HimResBlock* d, int which, const float* src, const float* stat, const float* dy, float* dw,
                            int accumulate, void* ws, size_t ws_bytes, void* stream);

#define HIM_PANEL_FWD 0
#define HIM_PANEL_BWD_DATA 1
size_t him_conv2d_panel_bytes(const HimConv2d* d, int kind);
/* 1 when the data gradient of `d` reads the SAME panel as its forward (the separate-transform Winograd layers: the batched
 * GEMM reads the forward panel transposed with mirrored transform positions) -- a trainer then keeps one panel per weight:
 * HIM_PANEL_FWD serves him_conv2d_bwd_data_panel / him_resblock_bwd_data as well (a HIM_PANEL_BWD_DATA panel built for
 * such a layer has the same content). */
int him_conv2d_bwd_data_shares_fwd_panel(const HimConv2d* d);
/* Which regrouping the panel of (d, kind) holds: 0 none (raw weights), 1 implicit-GEMM panel, 2 Winograd F(2x2,3x3) for the
 * separate-transform pipeline, 3 the fused Winograd kernel's chunked panel, 4 Winograd F(4x4,3x3) (frozen weights).  A pure
 * function of the descriptor, NOT of the weight alone: one nn.Conv2d weight called with another batch / plane size may need
 * another layout (e.g. VGG conv5_1 of models/layer_util.py:380-411 on the last, smaller batch of an epoch leaves F(4x4)),
 * so a cache of built panels keys on (kind, layout, him_conv2d_panel_bytes, HimAlgo). */
int him_conv2d_panel_layout(const HimConv2d* d, int kind);
int him_conv2d_panel_build(const HimConv2d* d, int kind, const float* w, void* panel, size_t panel_bytes,
                           void* stream);
int him_conv2d_fwd_panel(const HimConv2d* d, const float* x, const void* panel, const float* bias, float* y,
                         void* ws, size_t ws_bytes, void* stream);
int him_conv2d_bwd_data_panel(const HimConv2d* d, const float* dy, const void* panel, float* dx, void* ws,
                              size_t ws_bytes, void* stream);
/* Separate-transform Winograd layers (the 1024-channel ResnetBlock convolutions, models/layer_util.py:333-378): the
 * transformed input V = B^T x B of the forward, [16][Cin][tiles] floats, is also the column operand of the layer's weight
 * gradient dU = dM V^T.  A trainer that keeps it between forward and backward (67 MB per conv at config C2; this build is
 * sized for 288 GB) saves the weight gradient's own transposed input transform, and the weight-gradient GEMM reads both
 * operands K-contiguous.  *_keep_bytes: 0 when the descriptor has no such tensor (use the plain entry points).
 * him_conv2d_fwd_panel_keep == him_conv2d_fwd_panel that leaves V in `keep` (NULL: not kept);
 * him_conv2d_bwd_weight_kept == him_conv2d_bwd_weight with `keep` in place of x (same workspace size). */
size_t him_conv2d_fwd_keep_bytes(const HimConv2d* d);
int him_conv2d_fwd_panel_keep(const HimConv2d* d, const float* x, const void* panel, const float* bias, float* y, float* keep,
                              void* ws, size_t ws_bytes, void* stream);
int him_conv2d_bwd_weight_kept(const HimConv2d* d, const float* keep, const float* dy, float* dw, float* dbias, int accumulate,
                               void* ws, size_t ws_bytes, void* stream);
/* Data gradient GATED by the ReLU that produced this layer's input x: dx[i] = x[i] > 0 ? dgrad(dy)[i] : 0  -- the
 * activation backward of the PREVIOUS layer (models/layer_util.py:380-411 Vgg19: conv -> ReLU -> conv chains) done in
 * this launch's epilogue instead of a separate pass over dx.  `panel` (him_conv2d_panel_build, kind BWD_DATA) or `w`. */
int him_conv2d_bwd_data_gated(const HimConv2d* d, const float* dy, const float* w, const void* panel, const float* x,
                              float* dx, void* ws, size_t ws_bytes, void* stream);
size_t him_deconv2d_panel_bytes(const HimDeconv2d* d, int kind);
int him_deconv2d_panel_build(const HimDeconv2d* d, int kind, const float* w, void* panel, size_t panel_bytes,
                             void* stream);
int him_deconv2d_fwd_panel(const HimDeconv2d* d, const float* x, const void* panel, const float* bias, float* y,
                           void* ws, size_t ws_bytes, void* stream);
int him_deconv2d_bwd_data_panel(const HimDeconv2d* d, const float* dy, const void* panel, float* dx, void* ws,
                                size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * InstanceNorm2d(affine=False, eps) fused with the activation behind it and, for the second half of a
 * ResnetBlock, the residual add.  Replaces get_norm_layer('instance') models/layer_util.py:19-26 and
 * the `x + conv_block(x)` of models/layer_util.py:376-378.  Per-(n,c) reductions are wave64 shuffles.
 *   fwd: mean/rstd[planes] written; y = act((x-mean)*rstd) (+ residual when residual!=NULL)
 *   bwd: dz = dy*act'(xhat); dx = rstd*(dz - mean(dz) - xhat*mean(dz*xhat))
 * ------------------------------------------------------------------------------------------- */
int him_instnorm_fwd(const float* x, const float* residual, float* y, float* mean, float* rstd,
                     int planes, int hw, float eps, int act, float slope, void* stream);
int him_instnorm_bwd(const float* x, const float* mean, const float* rstd, const float* dy, float* dx,
                     int planes, int hw, int act, float slope, void* stream);

/* Conv2d -> InstanceNorm2d(affine=False) [-> ReLU / LeakyReLU] [+ residual] as ONE call: the encoder / PatchGAN block of
 * models/Pix2Pix_NET.py:74-92 and models/Discriminator_NET.py:64-96 (`nn.Conv2d`, `norm_layer`, activation in sequence).
 *   y_raw (B,Cout,OH,OW) = conv(x) + bias (kept: the InstanceNorm backward reads it), z = act((y_raw - mean) * rstd)
 *   [+ residual], mean / rstd [B*Cout].  `d->act` must be HIM_ACT_NONE (the activation follows the norm).
 * Few-tile layers that the forward launches with split-K (him_conv2d_in_act_fused(d) == 1: the PatchGAN blocks, the
 * generator's last down-convolutions) hand the raw split-K slabs to the InstanceNorm kernel, which sums them in the finish
 * pass's order, adds the bias, writes y_raw, reduces the statistics and writes z in one pass: the split-K finish launch
 * and one read of y_raw disappear, every output is bit-identical to him_conv2d_fwd + him_instnorm_fwd.  All other
 * descriptors run exactly those two launches behind this entry.  `panel` (HIM_PANEL_FWD) or `w`; workspace =
 * him_conv2d_fwd_ws(d).  Backward: him_instnorm_bwd(y_raw, ...) then the conv's him_conv2d_bwd_*. */
int him_conv2d_in_act_fused(const HimConv2d* d);
int him_conv2d_in_act_fwd(const HimConv2d* d, const float* x, const float* w, const void* panel, const float* bias,
                          float* y_raw, const float* residual, float* z, float* mean, float* rstd, float eps, int act,
                          float slope, void* ws, size_t ws_bytes, void* stream);

/* Return codes of the elementwise, encoding, pooling and spectral-norm entries below (him_act_bwd ... him_maxpool_relu_bwd,
 * him_fill, him_scale, him_sn_*, him_div_scalar_*), all decided on the host before any launch; a refused call writes nothing:
 *   flat entries taking `size_t n` (him_act_bwd, him_add, him_fill, him_scale, him_u8_to_f32, him_div_scalar_*): n == 0 is
 *     HIM_OK and launches nothing, whatever the pointers; a null pointer with n > 0 is HIM_E_INVALID.
 *   shaped entries: HIM_E_INVALID for a non-positive B / planes / C / label_nc / hw / H / W / rows / cols, for a channel
 *     slice outside [0, Ctot) (c0 < 0 or c0 + n > Ctot; likewise cs0 / cd0 / ca0 / cb0), for OH / OW other than
 *     (H - 1) / 2 + 1, (W - 1) / 2 + 1, for k <= 0 or k larger than H or W, and for a null pointer other than the ones named
 *     optional below (him_masked_image's three outputs, him_masked_mean's noise, him_copy_channels' mask at mask_mode 0,
 *     him_sn_power_iter_bwd's u_out and sigma, which it does not read).  him_copy_channels: n < 0 is HIM_E_INVALID, n == 0
 *     with a valid slice is HIM_OK without a launch.
 *   HIM_E_WORKSPACE: ws null or ws_bytes below the size the entry names. */
/* dz = dy * act'(.) expressed through the activation OUTPUT y (ReLU/LeakyReLU/Tanh epilogues). */
int him_act_bwd(const float* y, const float* dy, float* dz, size_t n, int act, float slope, void* stream);
/* out = a + b  (gradient fan-in, residual adds) */
int him_add(const float* a, const float* b, float* out, size_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Input encoding: models/pix2pixHD_condImg_model.py:144-174 (+ :285-291 get_edges,
 * models/pix2pixHD_condImgColor_model.py:147-186).  All write into a channel slice
 * [c0, c0+n) of a (B,Ctot,H,W) destination so torch.cat never materialises.
 * ------------------------------------------------------------------------------------------- */
int him_onehot(const float* label, float* dst, int B, int label_nc, int Ctot, int c0, int hw, void* stream);
/* nn.AvgPool2d(3, 2, 1, count_include_pad=False) applied to one-hot(label) (models/Discriminator_NET.py:31-32,47-58 on the
 * label channels of pix2pixHD_condImg_model.py:176-186's discriminator input) evaluated from the ids: class counts of the
 * 3x3 window / valid pixels, written to channels [c0, c0 + label_nc) of a (B, Ctot, OH, OW) destination.  Bit-identical to
 * him_avgpool3s2_fwd(him_onehot(label)); the full-resolution one-hot tensor is never written. */
int him_onehot_pool3s2(const float* label, float* dst, int B, int label_nc, int Ctot, int c0, int H, int W, int OH, int OW,
                       void* stream);
/* Compact inputs: label / instance maps travel as uint8 ids (1 byte per pixel over PCIe instead of the
 * float maps of data/segmentation_dataset.py:82) and are widened on the device; get_masked_image of
 * data/base_dataset.py:342-357 for a whole batch: bbox[b] = (wmin, hmin, wmax, hmax) floats on the device;
 * mask (B,1,H,W), masked_object = mask*image, masked_context = (1-mask)*image + mask*cls2fill (any output may be NULL). */
int him_u8_to_f32(const unsigned char* src, float* dst, size_t n, void* stream);
int him_masked_image(const float* image, const float* bbox, float* mask, float* masked_object, float* masked_context,
                     int B, int C, int H, int W, float cls2fill, void* stream);
int him_edges(const float* inst, float* dst, int B, int H, int W, int Ctot, int c0, void* stream);
/* per-image masked mean colour, times noise (B,3) (NULL = 1), clamped to [-1,1]  -> emb (B,3) */
int him_masked_mean(const float* image, const float* obj_mask, const float* noise, float* emb, int B,
                    int hw, void* stream);
/* dst[:, c0:c0+3] = emb[b,c] * mask[b]   (encode_global_embedding) */
int him_tile_embed(const float* emb, const float* mask, float* dst, int B, int Ctot, int c0, int hw,
                   void* stream);

/* dst[:, cd0:cd0+n] = f(mask) * src[:, cs0:cs0+n]; mask (B,1,HW) or NULL;
 * mask_mode 0: f=1, 1: f=mask, 2: f=1-mask.  Implements torch.cat / slicing / `x*mask.repeat(...)`
 * (pix2pixHD_condImg_model.py:165-166,176-186,229-233) and their backward passes. */
int him_copy_channels(const float* src, int Csrc, int cs0, float* dst, int Cdst, int cd0, int n, int B,
                      int hw, const float* mask, int mask_mode, int accumulate, void* stream);
/* out = (1-m)*a + m*b with a, b channel slices: output gate models/Pix2Pix_NET.py:96-99,242-245 and the
 * two-stream fusion :215-217.  m is (B,1,HW).  The sum is contracted (one fused multiply-add): with a 0/1 mask the result
 * is a or b exactly; with a fractional mask it is within one rounding of the exact value, not torch's two roundings.  The
 * same holds for him_copy_channels with accumulate and a mask. */
int him_blend(const float* a, int Ca, int ca0, const float* b, int Cb, int cb0, const float* m, float* out,
              int B, int C, int hw, void* stream);

/* nn.AvgPool2d(3, stride=2, padding=1, count_include_pad=False): models/Discriminator_NET.py:31-32. */
int him_avgpool3s2_fwd(const float* x, float* y, int planes, int H, int W, int OH, int OW, void* stream);
int him_avgpool3s2_bwd(const float* dy, float* dx, int planes, int H, int W, int OH, int OW, void* stream);
/* nn.MaxPool2d(k, k): VGG19 2x2 pools (models/layer_util.py:383) and the 2^n mask pool
 * (models/Pix2Pix_NET.py:134). bwd routes to the first maximum in row-major window order and writes every element of dx:
 * rows and columns that no window covers (H or W not a multiple of k) get 0. */
int him_maxpool_fwd(const float* x, float* y, int planes, int H, int W, int k, void* stream);
int him_maxpool_bwd(const float* x, const float* dy, float* dx, int planes, int H, int W, int k, void* stream);
/* the same for a pool that follows a ReLU whose backward is folded in: windows with a non-positive maximum pass nothing */
int him_maxpool_relu_bwd(const float* x, const float* dy, float* dx, int planes, int H, int W, int k, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Losses: models/losses.py:40-50 (LSGAN MSE vs a constant), nn.L1Loss pairs of
 * pix2pixHD_condImg_model.py:235-251 and models/losses.py:75-82.  Deterministic two-stage reductions.
 *   *_fwd : out[0] = mean(...)     (device scalar)
 *   *_bwd : d(in) (+)= g[0] * d mean / d in     (g = device scalar upstream gradient)
 *   HIM_E_INVALID: n == 0 in a *_fwd (the mean of nothing), him_lincomb_* with n outside 1..8 or a null table;
 *   HIM_E_WORKSPACE: ws null or ws_bytes < him_reduce_ws(n) / him_l1_multi_ws(npairs).  *_bwd with n == 0, and
 *   him_l1_multi_* with npairs <= 0, are HIM_OK and launch nothing.  All of these return before any launch, except an
 *   empty pair (n[i] == 0) inside him_l1_multi_fwd, which is found after the preceding table of 16 pairs was launched.
 * ------------------------------------------------------------------------------------------- */
size_t him_reduce_ws(size_t n);
int him_l1_mean_fwd(const float* a, const float* b, size_t n, float* out, void* ws, size_t ws_bytes,
                    void* stream);
/* him_l1_mean_bwd: `accumulate` bit 0 = add into da, bit 1 = gate by a > 0 (a is a ReLU output whose activation
 * backward is folded into this pass) */
int him_l1_mean_bwd(const float* a, const float* b, size_t n, const float* g, float* da, int accumulate,
                    void* stream);
/* Several L1 terms at once (feature matching: 12 pairs, VGG: 5): out[i] = mean|a[i] - b[i]|, da[i] = g[i] * d/da[i]
 * (NULL da[i]: skipped).  a / b / n / da are HOST arrays of npairs entries; out and g are device vectors.  Work split and
 * summation order per pair are those of him_l1_mean_fwd / _bwd (bit-identical results), three launches per 16 pairs. */
size_t him_l1_multi_ws(int npairs);
int him_l1_multi_fwd(const float* const* a, const float* const* b, const size_t* n, int npairs, float* out, void* ws,
                     size_t ws_bytes, void* stream);
int him_l1_multi_bwd(const float* const* a, const float* const* b, const size_t* n, int npairs, const float* g,
                     float* const* da, int accumulate, void* stream);
/* Scalar loss arithmetic on device scalars (pix2pixHD_condImg_model.py:218-251: the per-scale GAN-loss sums, `* lambda_feat`;
 * train_mask2image.py:68-76: (D_fake + D_real) * 0.5, G_GAN + G_GAN_Feat + G_VGG):  out[0] = scale * sum_i weights[i] * terms[i][0],
 * summed left to right, every product and sum rounded to fp32 (the reference's chain of one-element tensor ops, in ONE
 * launch).  terms / dterms / weights are HOST arrays of n <= 8 entries; bwd: dterms[i][0] = g[0] * scale * weights[i]. */
int him_lincomb_fwd(const float* const* terms, const float* weights, int n, float scale, float* out, void* stream);
int him_lincomb_bwd(const float* g, const float* weights, int n, float scale, float* const* dterms, void* stream);
int him_mse_const_fwd(const float* x, size_t n, float target, float* out, void* ws, size_t ws_bytes,
                      void* stream);
int him_mse_const_bwd(const float* x, size_t n, float target, const float* g, float* dx, int accumulate,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * torch.optim.Adam (betas=(beta1,0.999), eps 1e-8, no weight decay) over a flat parameter arena:
 * pix2pixHD_condImg_model.py:135-139 + the .step() calls of train_mask2image.py:80,86.
 * `step` is the 1-based step count.  lr / betas / eps are DOUBLES: 1 - beta2, the bias corrections and lr / bc1 are
 * derived in double and rounded to fp32 once, as torch.optim.Adam does with its python-float hyper-parameters.
 * ------------------------------------------------------------------------------------------- */
int him_adam_step(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1,
                  double beta2, double eps, int step, void* stream);
int him_fill(float* p, size_t n, float value, void* stream);
int him_scale(float* p, size_t n, float s, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Exponential moving average of the weights (the generator a GAN is served from), in the pass Adam already makes
 * over the arena.  No counterpart in the reference: off unless the trainer asks for it (--ema_decay).
 *   him_adam_ema_step: him_adam_step -- the SAME kernel body, p / m / v come out bit-identical -- followed, per element
 *     and in fp32, by  ema' = fma(w, p' - ema, ema)  with w = (float)(1.0 - ema_decay) derived in double and rounded
 *     once (the lerp form: d * ema + (1 - d) * p' loses the whole update at d = 0.999).  ema_decay == 0 stores p' itself.
 *     One more read and one more write per parameter: 36 B instead of 28 B.
 *   him_ema_update: the same EMA arithmetic on its own, for tensors that change outside an Adam run.
 *   him_swap: exchanges two fp32 buffers in place (the averaged weights go under the live parameter views and come
 *     out again without a third buffer).
 * Any n, pointers need only be 4-byte aligned.  HIM_E_INVALID: step < 1, ema_decay outside [0, 1), a null pointer with
 * n > 0.  n == 0 is HIM_OK and launches nothing.
 * ------------------------------------------------------------------------------------------- */
int him_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, double lr, double beta1,
                      double beta2, double eps, int step, double ema_decay, void* stream);
int him_ema_update(float* ema, const float* p, size_t n, double ema_decay, void* stream);
int him_swap(float* a, float* b, size_t n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient guard: the global norm of a flat gradient arena, a clip coefficient and a non-finite flag, all left in
 * DEVICE memory where the Adam kernel reads them -- no host synchronisation inside an optimizer step.  No counterpart
 * in the reference: off unless the trainer asks for it (--clip_grad_norm / --skip_nonfinite).
 *
 * him_grad_stats: one pass over g[0, n) (4 B per element).
 *   seg      device array of nseg (begin, length) pairs: sorted, non-overlapping sub-ranges of [0, n) (the arena's
 *            parameter tensors; padding belongs to no segment).  nseg == 0: seg and seg_out may be null.
 *   seg_out  device, 2 * nseg doubles: [2i] = sum of squares of the FINITE elements of segment i, [2i+1] = its number
 *            of non-finite elements (Inf or NaN).
 *   st       device, 8 doubles:  [0] sum of squares of the finite elements of [0, n)   [1] non-finite count of [0, n)
 *            [2] sqrt(st[0])   [3] clip coefficient c   [4] calls seen   [5] calls with st[1] > 0   [6], [7] = 0.
 *            [4] and [5] are cumulative: the caller zeroes the buffer once, every accepted call adds to them.
 *   c        1 when max_norm <= 0 or +inf (clipping off), else min(1, max_norm / (st[2] + 1e-6)) -- the rule of
 *            torch.nn.utils.clip_grad_norm_ -- evaluated in double and rounded to fp32 ONCE; st[3] is that fp32 value
 *            widened back.
 *   Every square is formed in double (exact for fp32 inputs) and every sum is a double sum.  The result is a pure
 *   function of (g, n, seg, max_norm): no floating-point atomics, and the order of the additions is fixed by a
 *   decomposition into chunks counted from each range's start, independent of grid size and of the device's CU count.
 *   Loads are 16 bytes wide where the chunk is 16-byte aligned (256-byte aligned arena slots always are); any 4-byte
 *   aligned g is correct and gives the same bits.  A seg table that breaks its contract is clamped into [0, n): wrong
 *   sums, never an access outside g or ws.
 *   ws: him_grad_stats_ws(n, nseg) bytes, rewritten by every call.
 *   HIM_E_INVALID: nseg < 0, max_norm negative or NaN, null st, null seg / seg_out with nseg > 0, null g / ws with
 *   n > 0.  HIM_E_WORKSPACE: ws_bytes too small.  A refused call writes nothing.  n == 0 reads nothing (g, ws may be
 *   null), writes zeros and still counts as a call.
 *
 * him_adam_guarded_step: him_adam_step (ema == NULL; ema_decay ignored) or him_adam_ema_step (ema != NULL) -- the SAME
 *   kernel body -- behind st[1] and st[3], read by the kernel from device memory.  st[1] > 0: nothing is stored, p / m /
 *   v / ema keep their bits.  Otherwise the body runs on g' = fl32(g * c) with c = (float)st[3]; at c == 1 the multiply
 *   is skipped and the results are bit-identical to the unguarded entries.  UNLIKE torch.nn.utils.clip_grad_norm_ the
 *   gradient buffer is never modified: clipping happens in registers, g is read-only.  A caller that wants clipping
 *   without the skip hands over an st whose slot [1] is zero.  Return codes as him_adam_ema_step, plus null st.
 * ------------------------------------------------------------------------------------------- */
size_t him_grad_stats_ws(size_t n, int nseg);
int him_grad_stats(const float* g, size_t n, const long long* seg, int nseg, double* seg_out, double* st,
                   double max_norm, void* ws, size_t ws_bytes, void* stream);
int him_adam_guarded_step(float* p, const float* g, float* m, float* v, float* ema, size_t n, double lr,
                          double beta1, double beta2, double eps, int step, double ema_decay, const double* st,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spectral norm power iteration, Ip = 1: models/sn_utils.py:8-25,62-67.
 *   v = l2n(u W), u' = l2n(W v^T), sigma = u' W v^T, with NOTHING detached: the backward
 *   differentiates through both normalisations.
 *   fwd: v_out[cols], u_out[rows], sigma_out[1]; scratch t[rows], s[cols] live in ws.
 *   bwd: dW (+)= g_sigma * d sigma / dW   given the saved u (input), v_out, u_out.
 *   ws: him_sn_ws(rows, cols) bytes for either pass.  W == 0 gives v = u' = sigma = 0 and dW (+)= 0 exactly.
 * ------------------------------------------------------------------------------------------- */
size_t him_sn_ws(int rows, int cols);
int him_sn_power_iter_fwd(const float* W, const float* u, int rows, int cols, float* v_out, float* u_out,
                          float* sigma_out, void* ws, size_t ws_bytes, void* stream);
int him_sn_power_iter_bwd(const float* W, const float* u, const float* v_out, const float* u_out,
                          const float* sigma, const float* g_sigma, int rows, int cols, float* dW,
                          int accumulate, void* ws, size_t ws_bytes, void* stream);
/* out = W / sigma[0] ; and the W-side of its backward: dW (+)= dWbar/sigma, dsigma = -sum(dWbar*W)/sigma^2.
 * him_div_scalar_bwd's ws holds one partial sum per block: min(ceil(n / 1024), 1024) floats; him_reduce_ws(n) bytes
 * (what ops.py passes) are always enough.  HIM_E_WORKSPACE below that, or with ws null. */
int him_div_scalar_fwd(const float* W, const float* sigma, float* out, size_t n, void* stream);
int him_div_scalar_bwd(const float* W, const float* sigma, const float* dout, float* dW, float* dsigma,
                       size_t n, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Loader-side pixel work: what the reference's Dataset does per sample with PIL / torchvision on the
 * host -- data/base_dataset.py:243-268 get_transform_fn (select_region crop -> Image.resize NEAREST | BICUBIC ->
 * FLIP_LEFT_RIGHT -> ToTensor -> Normalize), data/segmentation_dataset.py:86-131 (get_masked_image x2, the instance
 * mask) -- for a whole batch on the device.  The crop windows are raw bytes inside ONE staging buffer `base`
 * (sample b at byte offset off[b], pitch[b] pixels per row); the per-row / per-column tables come from the host
 * (neurips18_hierchical_image_manipulation_amd/data/resample.py) and live in the same buffer.  Results are bit-identical to Pillow 12.2's.
 *   him_data_nearest:   dst[b][y][x] = src_b[ytab[b][y]][xtab[b][x]]; src_kind 0 u8 / 1 u16 / 2 i32;
 *                       dst_kind 0 f32 value / 1 f32 value/255 / 2 u8 / 3 i32.  A flip is folded into xtab.
 *   him_data_bicubic_h: tmp[b][r][i][c] = clip8((2^21 + sum_k weights[b][i][k] * src_b[r][first[b][i]+k][c]) >> 22),
 *                       interleaved RGB bytes, rows[b] source rows, tmp (B, maxrows, W, 3) bytes.
 *   him_data_bicubic_v: the same down the columns of tmp, then flip[b], /255 and (t-.5)/.5 -> dst (B,3,H,W) f32.
 *   him_data_region_masks: boxes (B,8) = input window, output window as (wmin,hmin,wmax,hmax) ints; fill (B) = the
 *                       class written into the input window; inst_id (B,2) = (selected?, id); inst_kind 0 f32 / 1 i32.
 *                       Writes mask_in, mask_object_in, mask_context_in, mask_out, mask_object_out and (if not NULL)
 *                       mask_object_inst, all (B,1,H,W) f32.
 * ------------------------------------------------------------------------------------------- */
int him_data_nearest(const void* base, const long long* off, const int* pitch, const int* xtab, const int* ytab,
                     int src_kind, void* dst, int dst_kind, int B, int H, int W, void* stream);
/* him_data_nearest over a map kept as per-row run lists in a resident pack (preprocess_pack.py, INTEGRATION.md "Packed
 * dataset"): sample b's image has int32 arrays row_start[h+1] / run_x[n] / run_v[n] at byte offsets row_off[b] /
 * runx_off[b] / runv_off[b] from `base` (4-byte aligned); the runs of row r are [row_start[r], row_start[r+1]), run_x
 * ascends inside a row from 0.  dst[b][y][x] = run_v of the last run of row y0[b] + ytab[b][y] whose run_x is
 * <= x0[b] + xtab[b][x]  ((x0, y0) = the window's origin inside the image), converted by dst_kind as above.  The
 * search stays inside the row's range (an empty range gives 0).  HIM_E_INVALID before any launch for a null pointer,
 * B / H / W <= 0 or an unknown dst_kind. */
int him_data_nearest_rle(const void* base, const long long* row_off, const long long* runx_off,
                         const long long* runv_off, const int* x0, const int* y0, const int* xtab, const int* ytab,
                         void* dst, int dst_kind, int B, int H, int W, void* stream);
int him_data_bicubic_h(const void* base, const long long* off, const int* pitch, const int* rows, const int* first,
                       const int* count, const int* weights, int ksize, unsigned char* tmp, int maxrows, int B, int W,
                       void* stream);
int him_data_bicubic_v(const unsigned char* tmp, int maxrows, const int* first, const int* count, const int* weights,
                       int ksize, const int* flip, float* dst, int normalize, int B, int H, int W, void* stream);
int him_data_region_masks(const float* label, const void* inst, int inst_kind, const int* boxes, const float* fill,
                          const int* inst_id, float* mask_in, float* obj_in, float* ctx_in, float* mask_out,
                          float* obj_out, float* inst_mask, int B, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Canvas crop / paste of the joint box -> layout -> image edit (reference util/data_util.py crop_canvas / paste_canvas,
 * models/joint_inference_model.py): the full-resolution canvas stays on the device; the host only supplies windows and
 * the resampling tables of data/resample.py.  Byte results are bit-identical to ToPILImage -> Pillow 12.2 -> ToTensor.
 *   him_canvas_window_bytes: dst (h,w,C) interleaved bytes = trunc(pre(src[c][y0+y][x0+x]) * 255) for a window of C
 *                       fp32 planes (Hs,Ws) that may extend past them (0 there, Image.crop's fill); pre 0: v, 1: v/255,
 *                       2: (v+1)/2.  C = 1 is the plain 2-D byte map him_data_nearest reads (src_kind 0), C = 3 the
 *                       interleaved RGB rows him_data_bicubic_h reads.
 *   him_canvas_paste_bicubic_v: him_data_bicubic_v's column pass of tmp (rows,W,3) without flip / Normalize, written as
 *                       v/255 into canvas (3,Hc,Wc) at [y0,y0+H) x [x0,x0+W) (the window must lie inside the canvas).
 *   him_canvas_paste_window: canvas[c][y0+y][x0+x] = src[c][y][x] for C planes (h,w); src_kind 0 f32 / 1 i64.
 * ------------------------------------------------------------------------------------------- */
int him_canvas_window_bytes(const float* src, int C, int Hs, int Ws, int x0, int y0, int h, int w, int pre,
                            unsigned char* dst, void* stream);
int him_canvas_paste_bicubic_v(const unsigned char* tmp, const int* first, const int* count, const int* weights,
                               int ksize, float* canvas, int Hc, int Wc, int x0, int y0, int H, int W, void* stream);
int him_canvas_paste_window(const void* src, int src_kind, int C, int h, int w, float* canvas, int Hc, int Wc, int x0,
                            int y0, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Tensors to pictures (reference util/util.py tensor2im / tensor2label + Colorize / tensor2seglabel): one pass over a
 * (C,H,W) device tensor, interleaved bytes out, so that only bytes cross to the host.  No global state; any H, W.
 *   tensor2im:   src fp32, C = 1 or 3; byte = trunc(clip(normalize ? (x + 1) / 2 * 255 : x * 255, 0, 255)), each
 *                operation rounded to fp32 on its own (numpy's order); C = 1 writes the value three times.  dst (H,W,3).
 *   label2color: C > 1: src fp32 scores, label = channel of the maximum, the lowest channel on a tie; C = 1: src holds
 *                the ids, dtype 0 fp32 / 1 uint8 / 2 int64.  dst (H,W,3) = table[label], table = n rows of 3 bytes on
 *                the device (n <= 8192).  A label outside [0, n) or a non-integer fp32 id writes (0,0,0).
 *   seglabel:    src fp32 with values in [0, 255]; dst (H,W,C) = trunc(src).
 * ------------------------------------------------------------------------------------------- */
int him_tensor2im_bytes(const float* src, int C, int H, int W, int normalize, unsigned char* dst, void* stream);
int him_label2color_bytes(const void* src, int dtype, int C, int H, int W, const unsigned char* table, int n,
                          unsigned char* dst, void* stream);
int him_seglabel_bytes(const float* src, int C, int H, int W, unsigned char* dst, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Instance-box summary (reference preprocess_city.py:16-41 construct_box): for every instance id >= min_id of an (H,W)
 * instance plane its inclusive bounding box, its pixel count and int(np.median(classes under it)), in ONE call on the
 * device.  Integer atomics only (min / max / add commute): results are bit-identical from run to run.
 *   inst:   (H,W) ids, inst_kind 0 uint8 / 1 16-bit read as unsigned / 2 int32 / 3 int64; accepted ids 0..65535.
 *   cls:    (H,W) classes, cls_kind 0 uint8 / 1 int32 / 2 int64 / 3 fp32 holding integral values; accepted 0..255.
 *   status: 2 ints, written by the device: [0] = number of objects found (also when it exceeds max_objects),
 *           [1] = HIM_INST_OVERFLOW | HIM_INST_ID_RANGE | HIM_INST_CLS_RANGE bits.
 *   table:  max_objects rows of 7 ints (id, xmin, ymin, xmax, ymax, count, cls), ascending id (np.unique's order),
 *           rows [0, min(status[0], max_objects)) are written; zero-based inclusive pixel indices; for an even count
 *           cls is the mean of the two middle order statistics truncated toward zero.  With any status bit set the
 *           table's contents are unspecified; nothing outside status, table and ws is ever written.
 *   ws:     him_inst_summary_workspace(H, W, max_objects) bytes, 16-byte aligned; cleared by the call itself, so
 *           one workspace serves any sequence of calls on one stream.  1 <= max_objects <= 65536.
 * Planes whose width is not a multiple of 8 or whose base is not 16-byte aligned are read element by element.
 * ------------------------------------------------------------------------------------------- */
#define HIM_INST_OVERFLOW 1
#define HIM_INST_ID_RANGE 2
#define HIM_INST_CLS_RANGE 4
size_t him_inst_summary_workspace(int H, int W, int max_objects);
int him_inst_summary(const void* inst, int inst_kind, const void* cls, int cls_kind, int H, int W, int min_id,
                     int max_objects, int* status, int* table, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ADE20K segmentation decode (reference preprocess_ade.py: loadAde20K, and the relabel and box loops of its main): the
 * colour planes of one `_seg.png` to a class plane, a label plane, an instance-rank plane and a box per instance, in ONE
 * call on the device.  Integer atomics only (min / max / add): results are bit-identical from run to run.
 *   seg:       (H,W,pixel_bytes) interleaved bytes R,G,B[,A] as the PNG decodes; pixel_bytes 3 or 4, a fourth byte is
 *              ignored.  Never written.
 *   keep:      n_keep (0..255) class ids on the device; may be NULL when n_keep is 0.
 *   cls_out:   (H,W) uint16 raw class (R / 10) * 256 + G, the division flooring; may be NULL.
 *   label_out: (H,W) bytes: the 1-based position of the class in keep (of its first occurrence), 0 when it is not there.
 *   inst_out:  (H,W) bytes: the rank of the pixel's B value among the distinct B values of the image
 *              (np.unique(B, return_inverse=True)); rank 0 is the lowest value present, zero or not.
 *   status:    2 ints: [0] = number of distinct B values (1..256), [1] = flags, 0 (reserved).
 *   table:     256 rows of 7 ints (rank, b, xmin, ymin, xmax, ymax, count), ascending rank, zero-based inclusive pixel
 *              indices; rows [0, status[0]) are written and nothing behind them.
 *   ws:        him_ade_decode_workspace() bytes, 16-byte aligned; cleared by the call itself, so one workspace serves
 *              any sequence of calls on one stream.
 * Three launches on `stream`, no host synchronisation.  Nothing outside the five outputs and ws is written.  With every
 * plane's base on a 16-byte boundary whole 16-pixel groups move as 16-byte words; any other base, and the last partial
 * group of a plane, is read and written byte by byte.  H * W <= 2^31 - 1.
 * ------------------------------------------------------------------------------------------- */
size_t him_ade_decode_workspace(void);
int him_ade_decode(const unsigned char* seg, int H, int W, int pixel_bytes, const unsigned short* keep, int n_keep,
                   unsigned short* cls_out, unsigned char* label_out, unsigned char* inst_out, int* status, int* table,
                   void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Evaluation metrics (the reference ships none; these are the measures this line of work reports): SSIM / PSNR / L1
 * sums of a generated batch against the real one inside the edited box, and the confusion matrix behind pixel
 * accuracy, class IoU and object-mask IoU.  One call each on `stream`, no host synchronisation, results bit-identical
 * from run to run.
 *
 * him_image_metrics: a, b (B,C,H,W) planar fp32, C = 1 or 3, never written.
 *   Mapping on load: x' = x * scale + offset, the product and the sum each rounded to fp32; with quantize != 0 then
 *   x' = trunc(clip(x', 0, 255)).  ONE preset takes another operation order: scale = 127.5, offset = 127.5 and
 *   quantize != 0 evaluates (x + 1) / 2 * 255 as him_tensor2im_bytes(normalize = 1) does, so that the values are the
 *   bytes of the saved pictures and the SSIM is theirs.
 *   SSIM (Wang et al. 2004): separable 11 x 11 window, g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), i = 0..10, normalised to
 *   sum 1 in double and then rounded to fp32; only windows wholly inside the image (or the box) are used, so the map is
 *   (H - 10) x (W - 10); weighted moments mu_a, mu_b, E[a^2], E[b^2], E[ab]; s_a^2 = E[a^2] - mu_a^2, s_b^2 likewise,
 *   s_ab = E[ab] - mu_a mu_b, no sample correction; C1 = (0.01 L)^2, C2 = (0.03 L)^2 with L = data_range (computed in
 *   double, rounded to fp32);
 *     ssim = (2 mu_a mu_b + C1) (2 s_ab + C2) / ((mu_a^2 + mu_b^2 + C1) (s_a^2 + s_b^2 + C2)).
 *   The moments are accumulated in fp32 on x' - p with a per-tile pivot p (the tile's first pixel; variance and covariance
 *   are shift-invariant, the means get p back), which avoids the cancellation of E[x^2] - mu^2 on bright flat regions.
 *   box:  NULL = the whole image; else (B,4) int32 on the device, (xmin, ymin, xmax, ymax) inclusive, clipped to the
 *         image.  Everything is evaluated as if both images had been cropped to the box.  A box thinner than 11 in
 *         either direction has 0 windows (its error sums are still produced); an empty box gives five zeros.
 *   sums: (B,C,5) doubles per plane: [sum of ssim over the windows, number of windows, sum of (a' - b')^2, sum of
 *         |a' - b'|, number of pixels].  The error sums are accumulated in double.
 *   map_out: NULL, or (B,C,H-10,W-10) fp32, the SSIM of every window; whole-image calls only (box must be NULL, H and
 *         W >= 11).  `sums` does not depend on whether the map is written.
 *   ws:   him_image_metrics_workspace(B, C, H, W) bytes, 8-byte aligned, fully overwritten by the call.
 *   Limits: H * W <= 2^31 - 1, B * C <= 65535 planes, H <= 65535 * 16 rows; beyond them the call is refused.
 *   Kernel layout: one 256-thread workgroup per tile of 16 x 64 window origins stages (16+10) x (64+10) pixels of both
 *   images in LDS once, runs the row pass into LDS and the column pass from it, and writes three doubles to its own
 *   workspace slot; a second launch adds a plane's slots in a fixed order in double.  No floating-point atomics.
 *
 * him_confusion: counts[gt id][predicted id] over the pixels of a batch of label planes, in integers.
 *   pred: pred_kind 0 uint8 ids / 1 int32 ids / 2 int64 ids / 3 fp32 holding integral ids, all (B,1,H,W) with C = 1;
 *         4 fp32 scores (B,C,H,W), the label is the channel of the maximum, the lowest channel on a tie (strict >
 *         walking upwards, him_label2color_bytes' rule); 5 fp32 probabilities (B,1,H,W), C = 1, label = p > 0.5 ? 1 : 0
 *         (the reference's object-mask threshold, models/TwoStreamAE_mask.py:333).
 *   gt:   gt_kind 0..3 as pred_kind 0..3, (B,1,H,W).
 *   mask: NULL, or fp32 (B,1,H,W): a pixel counts where mask != 0.
 *   ignore: a ground-truth id whose pixels are left out (compared before the range check, so it may be >= n); -1: none.
 *   n:    classes, 1 <= n <= 256.  A pixel that passes mask and ignore and whose gt or predicted id is negative, >= n or
 *         a non-integral fp32 is SKIPPED: it is counted in status[0] and never in counts.
 *   counts: int64, (B,n,n) with per_sample != 0, else (1,n,n); row = ground truth, column = prediction.
 *   accumulate != 0 adds into counts and into status (status[0] += skipped, flags are or-ed): an evaluation loop needs
 *         neither a host add nor a synchronisation.  Otherwise both are overwritten.
 *   status: 2 ints: [0] = skipped pixels (saturating at 2^31 - 1), [1] = HIM_CONF_SKIPPED | HIM_CONF_SATURATED bits.
 *   ws:   him_confusion_workspace(n) bytes, 8-byte aligned, cleared by the call itself.
 *   Each workgroup keeps a private 32-bit histogram in LDS while n <= 160 (n * n * 4 bytes <= 100 KiB of the CU's 160
 *   KiB; a workgroup's share of pixels stays below 2^32) and flushes its non-zero cells with 64-bit integer atomics;
 *   above that it adds to counts directly.  Integer adds commute: exact, and identical from run to run.  Planes whose
 *   base is not 16-byte aligned or whose width is not a multiple of 4 are read element by element.  H * W <= 2^31 - 1.
 *   Nothing outside counts, status and ws is written.
 * Both return HIM_E_INVALID / HIM_E_WORKSPACE before any launch for a NULL required pointer, C outside {1, 3} (image
 * metrics), H or W < 1, n out of range, an unknown kind, or a workspace smaller than the query's size.
 * ------------------------------------------------------------------------------------------- */
#define HIM_CONF_SKIPPED 1
#define HIM_CONF_SATURATED 2
size_t him_image_metrics_workspace(int B, int C, int H, int W);
int him_image_metrics(const float* a, const float* b, int B, int C, int H, int W, float scale, float offset, int quantize,
                      float data_range, const int* box, double* sums, float* map_out, void* ws, size_t ws_bytes,
                      void* stream);
size_t him_confusion_workspace(int n);
int him_confusion(const void* pred, int pred_kind, const void* gt, int gt_kind, const float* mask, int B, int C, int H,
                  int W, int n, int ignore, int per_sample, int accumulate, long long* counts, int* status, void* ws,
                  size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Instance labelling of layouts (the reference ships none; its loaders expect instance maps from the dataset):
 * connected-component labelling of a batch of class planes into instance planes in the Cityscapes convention, so that
 * him_inst_summary, him_edges and the loader work on a layout that has no instance annotation.  Exact integer work.
 * Per plane b of cls (B,H,W), independently of the other planes:
 *   - a component is a maximal 4- or 8-connected set of pixels of ONE class c with thing[c] != 0;
 *   - components of fewer than min_area pixels are no objects (min_area <= 1 keeps all);
 *   - kept components are numbered r = 0, 1, ... in raster order of their first pixel (the smallest y * W + x);
 *   - inst_out = base_id + r on their pixels, and the pixel's class on every other pixel (classes without instances
 *     and dropped components).
 *   cls:     cls_kind 0 uint8 / 1 int32 / 2 int64 / 3 fp32 holding integral values; accepted 0..255.  Never written.
 *   thing:   256 bytes on the device, non-zero = the class has instances.
 *   connectivity: 4 or 8.   base_id: >= 256 (1000 is the Cityscapes convention).   max_objects: 1..65536.
 *   inst_out: (B,H,W) int32.
 *   status:  B x 2 ints written by the device: [b][0] = number of kept components of plane b (also when it exceeds
 *            max_objects), [b][1] = flag bits: HIM_CCL_OVERFLOW (count > max_objects, or base_id + count - 1 > 65535,
 *            the id domain him_inst_summary accepts) | HIM_CCL_CLS_RANGE (a class is negative, > 255 or a non-integral
 *            fp32).  With a bit set that plane's inst_out is unspecified; nothing outside inst_out, status and ws is
 *            ever written.
 *   ws:      him_label_instances_workspace(B, H, W) bytes (two ints per pixel and a few per tile), 16-byte aligned;
 *            every cell that is read is written by the call first, so one workspace serves any sequence of calls on one
 *            stream.
 * Asynchronous, no allocation.  Seven launches on `stream`: tile pass (a 256-thread workgroup labels a tile of 32 x 64
 * pixels by union-find on int32 parents in LDS), border pass (atomicMin on the global parents across tile borders),
 * flatten (+ integer area counts), count / scan / rank (an exclusive prefix sum of the kept roots in raster order) and
 * the write.  No cooperative launch, no grid-wide barrier, no workgroup waits for another.  The root of a component is
 * its smallest pixel index whatever the order of the atomics, and ranks come from the prefix sum: inst_out and status
 * are bit-identical from run to run.  Planes are read element by element (a lane per column), any base and any width.
 * HIM_E_INVALID before any launch for a NULL pointer, connectivity outside {4, 8}, B, H or W < 1, H * W > 2^31 - 1,
 * B * H * W > 2^40, base_id < 256, max_objects outside 1..65536, an unknown kind or a misaligned workspace;
 * HIM_E_WORKSPACE for a workspace smaller than the query's size (the query returns 0 for a shape that is refused).
 * ------------------------------------------------------------------------------------------- */
#define HIM_CCL_OVERFLOW 1
#define HIM_CCL_CLS_RANGE 2
size_t him_label_instances_workspace(int B, int H, int W);
int him_label_instances(const void* cls, int cls_kind, int B, int H, int W, const unsigned char* thing, int connectivity,
                        int min_area, int base_id, int max_objects, int* inst_out, int* status, void* ws,
                        size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Differentiable discriminator augmentation (Zhao et al., "Differentiable Augmentation for Data-Efficient GAN
 * Training", NeurIPS 2020; the reference ships none): brightness -> saturation -> contrast -> translation with zero
 * fill -> cutout, applied with ONE parameter row per sample to a dense (B,C,H,W) tensor, the concatenated discriminator
 * input.  Channels [c0, c0+3) are the image; every other channel is condition and takes part in the geometric steps only.
 *   table: int32 (B,8) on the device: [bits(b), bits(a), bits(k), ty, tx, cut_y0, cut_x0, policy_bits]; b, a, k are fp32
 *          values stored as their bits.  policy_bits: HIM_AUG_COLOR | HIM_AUG_TRANSLATION | HIM_AUG_CUTOUT; a cleared
 *          bit SKIPS that step (it is not run with neutral values), so a row with only geometric bits copies and zeroes.
 *   policy: the steps this CALL may run; a row's effective bits are policy_bits & policy.  Without HIM_AUG_COLOR in
 *          `policy` no channel is treated as image, c0 is not constrained and ws may be NULL.
 *   ch, cw: the cutout's size, scalars of the call.
 * Forward, output element (b,c,y,x): 0 if (y+ty, x+tx) lies outside the plane; 0 if (y,x) lies in
 *   [cut_y0, cut_y0+ch) x [cut_x0, cut_x0+cw); else in[b,c,y+ty,x+tx], for the image channels of a colour row after the
 *   colour map  v_c = in_c + b,  p = (v_0+v_1+v_2)/3,  s_c = (v_c - p) a + p,  m = mean_b + b,  o_c = (s_c - m) k + m,
 *   with mean_b the mean of the sample's three image channels over the whole, untranslated plane (brightness and
 *   saturation leave the per-sample mean at mean(x) + b, so one reduction of the INPUT serves the contrast step).
 * Backward, the exact adjoint: g[b,c,y',x'] = dout[b,c,y'-ty,x'-tx] if that output position is in the plane and not
 *   cut, else 0; condition channels dx = g; image channels of a colour row, with S_b = sum over c,y',x' of g and
 *   N = 3 H W:  ds_c = k g_c + (1-k) S_b/N,  dx_c = a ds_c + (1-a)(ds_0+ds_1+ds_2)/3.
 *   Only channels [g0, g0+gn) are computed: dx is (B,gn,H,W), channel c of the input at channel c - g0.
 * Any table content is legal: shifts of +-H / +-W and beyond give zeros, a rectangle may be empty, hang over an edge or
 *   cover the plane; the kernels clamp both, no content moves an address outside the buffers.
 * ws: him_diffaug_ws(B,H,W) bytes, needed with HIM_AUG_COLOR.  After the call the first B doubles at ws rounded up to 8
 *   bytes hold the per-sample sums (forward: of the image channels of x; backward: S_b; 0 for a row without the colour
 *   bit).  Both sums are accumulated in double without atomics in a fixed tree over chunks of 16384 floats counted from
 *   the sample's first image element: a pure function of the inputs, independent of the grid (him_grad_stats' rule).
 * Each pass is one read and one write of the tensor (16 bytes per lane at any 4-byte alignment of base, row and shift)
 *   plus, with HIM_AUG_COLOR, one more read of the image channels and two small launches.
 * HIM_E_INVALID before any launch: a NULL x / table / y (or ws with HIM_AUG_COLOR), a negative size, unknown policy
 *   bits, c0 + 3 > C with HIM_AUG_COLOR in `policy`, [g0, g0+gn) outside [0, C), H * W > 2^29, or a workspace below the
 *   query.  Asynchronous, no allocation.
 *
 * him_diffaug_draw fills the table on the device; nothing is staged on the host, nothing synchronises.
 *   mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31  (the splitmix64
 *           finaliser), all arithmetic modulo 2^64, G = 0x9E3779B97F4A7C15.
 *   key = mix(mix(mix(seed + G) + step + G) + (sample0 + b) + G);   z_i = mix(key + (i + 1) G), i = 0..6.
 *   uniform u_i = (z_i >> 40) 2^-24;   integer in [lo, hi]: lo + (((z_i >> 32) (hi - lo + 1)) >> 32).
 *   b = u_0 - 0.5,  a = 2 u_1,  k = u_2 + 0.5  (each rounded to fp32 once);
 *   ty in [-sy, sy] from z_3 with sy = floor(H rt + 0.5), tx in [-sx, sx] from z_4 with sx = floor(W rt + 0.5);
 *   ch = floor(H rc + 0.5), oy in [0, H - (ch mod 2)] from z_5, cut_y0 = oy - floor(ch / 2); cw, z_6, cut_x0 likewise
 *   (the products in double).  DiffAugment's defaults are rt = 0.125, rc = 0.5.
 *   A step missing from `policy` leaves its neutral values (b 0, a 1, k 1; ty tx 0; cut_y0 cut_x0 0) and its bit clear;
 *   *ch and *cw (host) receive the cutout size, 0 without HIM_AUG_CUTOUT.
 *   HIM_E_INVALID: NULL pointer, B < 0, H or W outside 1..2^20, unknown policy bits, a ratio negative, NaN or > 1024.
 * ------------------------------------------------------------------------------------------- */
#define HIM_AUG_COLOR 1
#define HIM_AUG_TRANSLATION 2
#define HIM_AUG_CUTOUT 4
size_t him_diffaug_ws(int B, int H, int W);
int him_diffaug_fwd(const float* x, const int* table, float* y, int B, int C, int c0, int H, int W, int ch, int cw,
                    int policy, void* ws, size_t ws_bytes, void* stream);
int him_diffaug_bwd(const float* dout, const int* table, float* dx, int B, int C, int c0, int H, int W, int ch, int cw,
                    int policy, int g0, int gn, void* ws, size_t ws_bytes, void* stream);
int him_diffaug_draw(int* table, int B, int H, int W, long long seed, long long step, long long sample0, int policy,
                     double ratio_translation, double ratio_cutout, int* ch, int* cw, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Distance transform and boundary metrics (the reference ships none): the exact Euclidean distance transform of label
 * planes, and on it the contour measures of a predicted layout or object mask against the ground truth.  Integer work,
 * everything on `stream`, no host synchronisation, results bit-identical from run to run.
 *
 * him_edt: K independent jobs over the B planes of src; per job the squared distance from every pixel to the nearest
 * SEED pixel of the job's plane and, optionally, that seed's index (the feature transform).
 *   src:    (B,H,W), kind 0 uint8 / 1 int32 / 2 int64 / 3 fp32 holding integral ids (him_confusion's kinds); any base
 *           aligned to the element, any width; never written.
 *   jobs:   int32 (K,3) on the device, row k = [plane b, value v, rule]:
 *             HIM_EDT_NONZERO       seeds = pixels with src != 0;
 *             HIM_EDT_EQUALS        seeds = pixels with src == v;
 *             HIM_EDT_BOUNDARY_OF   seeds = pixels with src == v that have a 4-neighbour INSIDE the plane with
 *                                   src != v: the inner boundary of class v (the image border alone makes none);
 *             HIM_EDT_ANY_BOUNDARY  seeds = pixels with a 4-neighbour inside the plane holding another value.
 *   dist2:  int32 (K,H,W): min over seeds of (x - x')^2 + (y - y')^2, exact; HIM_EDT_NONE on every pixel of a job
 *           without a seed.
 *   nearest: NULL, or int32 (K,H,W): y' * W + x' of a nearest seed; among equidistant seeds the smallest index (the
 *           smallest y', then the smallest x'); -1 where there is no seed.
 *   status: int32 (K,2) written by the device: [k][0] = the job's seed count, [k][1] = flag bits; HIM_EDT_BAD_JOB marks
 *           a job whose plane is outside 0..B-1 or whose rule is unknown: it writes HIM_EDT_NONE / -1, counts 0 seeds
 *           and reads no plane.
 *   ws:     him_edt_workspace(K, H, W) bytes (an int16 per pixel and job, rounded up to 16), 2-byte aligned; every
 *           cell that is read is written by the call first.
 *   Limits, refused with HIM_E_INVALID before any launch: B < 1, H or W outside 1..16384 (so dx^2 + dy^2 < 2^30 fits
 *   an int32), K < 1, K * H * W > 2^40, a NULL src / jobs / dist2 / status / ws, an unknown kind, a pointer not aligned
 *   to its element; HIM_E_WORKSPACE for a workspace below the query (which returns 0 for a refused shape).
 *   Kernel layout, three launches.  Status: zero counts, job flags.  Row pass, a 256-thread workgroup per (row, job):
 *   a prefix maximum of "x if seed else -1" walking right and a suffix minimum walking left (wave shuffles, a carry
 *   between steps of 256 columns) give the nearest seed column of the row, the LEFT one on a tie, stored as int16;
 *   seeds are counted with integer atomics.  Column pass, a workgroup per (64 columns x 32 rows, job), lane = column,
 *   8 rows per thread: the row-pass columns are staged in LDS 64 rows at a time as (x - x')^2 and each thread minimises
 *   (x - x')^2 + (y - y')^2, first over the chunk of its tile and upwards in decreasing y' with <=, then downwards in
 *   increasing y' with <, so the smallest y' keeps a tie; a sweep stops once the chunk's row gap squared exceeds every
 *   thread's current distance (a workgroup vote), so the work follows the distances, bounded by H.  A job without a seed
 *   is answered from its count.  Integer arithmetic only, no cooperative launch, no workgroup waits for another.
 *
 * him_boundary_stats: one direction of a boundary comparison.  Job k has the seeds P_k of src under jobs[k] (as above);
 * dist2 (K,H,W) holds the distances to the OTHER map's boundary (a him_edt result over the other map, same job table).
 *   counts: int64 (K,4): [n_seed = |P_k|, n_matched = |{p : dist2 <= tol2}|, max_d2 over the reachable seeds (-1: none),
 *           n_unreachable = |{p : dist2 == HIM_EDT_NONE}|]; unreachable seeds enter neither max_d2 nor the sum.
 *   sumd:   double (K): sum over the reachable seeds of sqrt((double)dist2).  Each workgroup (16 rows of a job) writes its
 *           partial to its own workspace slot, a second launch adds a job's slots in a fixed order: no floating-point
 *           atomics, identical bits from run to run.
 *   tol2 >= 0.  ws: him_boundary_stats_workspace(K, H, W) bytes, 8-byte aligned, written before it is read.  A
 *   HIM_EDT_BAD_JOB row gives [0, 0, -1, 0] and 0.0.  Limits and refusals as him_edt.
 * The measures util/metrics.py builds from the two directions, per sample and class c with dP / dG the
 * HIM_EDT_BOUNDARY_OF c sets of prediction and ground truth and tol2 = floor(tolerance^2):
 *   precision = |{p in dP : d2(p, dG) <= tol2}| / |dP|, recall its mirror image, f1 = 2 P R / (P + R) (0 when P + R = 0);
 *   assd = (sum over dP of d(p, dG) + sum over dG of d(g, dP)) / (|dP| + |dG|);  hausdorff = sqrt(max of both max_d2);
 *   both boundaries empty: all five nan; exactly one empty: precision = recall = f1 = 0, assd and hausdorff nan.
 *   The band of radius r around the class boundaries of a map: dist2 <= floor(r^2) under HIM_EDT_ANY_BOUNDARY; a
 *   confusion matrix restricted to it (him_confusion's mask) gives the "trimap" IoU.
 *
 * him_label_ids: fp32 scores (pred_kind 4, (B,C,H,W): the channel of the maximum, the lowest on a tie) or probabilities
 * (pred_kind 5, C = 1: p > 0.5) to int32 ids (B,H,W), him_confusion's rules, so that predictions enter the two calls above.
 * ------------------------------------------------------------------------------------------- */
#define HIM_EDT_NONZERO 0
#define HIM_EDT_EQUALS 1
#define HIM_EDT_BOUNDARY_OF 2
#define HIM_EDT_ANY_BOUNDARY 3
#define HIM_EDT_NONE 2147483647
#define HIM_EDT_BAD_JOB 1
size_t him_edt_workspace(int K, int H, int W);
int him_edt(const void* src, int kind, int B, int H, int W, const int* jobs, int K, int* dist2, int* nearest, int* status,
            void* ws, size_t ws_bytes, void* stream);
size_t him_boundary_stats_workspace(int K, int H, int W);
int him_boundary_stats(const void* src, int kind, int B, int H, int W, const int* jobs, int K, const int* dist2, int tol2,
                       long long* counts, double* sumd, void* ws, size_t ws_bytes, void* stream);
int him_label_ids(const float* src, int pred_kind, int B, int C, int H, int W, int* ids, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Boundary-weighted and surface losses (the reference ships none): the box2mask trainer's reconstruction terms with a
 * weight that peaks on the outlines of the ground truth, and a signed-distance term on the object probability.  The
 * training-side counterpart of the boundary metrics above: every call reads int32 squared-distance planes as him_edt
 * writes them.  Everything on `stream`, no host synchronisation, no atomics, results bit-identical from run to run.
 *
 * Weight of a position with squared distance d2:  w = 1 + amp * exp(-d2 / (2 sigma^2)), and w = 1 exactly where
 * d2 == HIM_EDT_NONE (tested, not left to underflow); a boundary pixel (d2 == 0) weighs exactly 1 + amp.  fp32.
 *
 * him_bw_nll: him_masked_nll with that weight.  logp (B,C,hw), label / mask (B,hw) as there, dist2 (B,hw): one
 *   HIM_EDT_ANY_BOUNDARY job per sample over the ground-truth label plane.  Valid positions: mask >= 0.5 and
 *   0 <= (int)label < C.  out2 = {sum_valid w * -logp[label] / sum_valid w, sum_valid w}; nothing valid gives 0/0 = nan,
 *   as the unweighted loss.  bwd: dlogp[b][c][i] = -g * w_i / sum_w at c = label_i on valid positions, 0 elsewhere;
 *   sum_w is out2 + 1 of the forward.
 * him_bw_pair: the mean of him_bce_mean_fwd, kind 0: -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)), or of
 *   him_l1_mean_fwd, kind 1: |p - t|, with that weight, over n positions: out2 = {sum w l / sum w, sum w}.  dist2 (n): one
 *   HIM_EDT_ANY_BOUNDARY job per sample over t.  bwd: the derivative of him_bce_mean_bwd ((p - t) / max(p (1 - p), 1e-12))
 *   or of him_l1_mean_bwd (the sign of p - t, 0 at p == t) times g * w_i / sum_w.
 * him_surface, after Kervadec et al., "Boundary loss for highly unbalanced segmentation", MIDL 2019: with
 *   d2_fg / d2_bg (B,H,W) the HIM_EDT_EQUALS 1 / HIM_EDT_EQUALS 0 distances over t, phi = +sqrt(d2_fg) where t < 0.5,
 *   -sqrt(d2_bg) where t >= 0.5, 0 where the distance it needs is HIM_EDT_NONE (an empty or a full mask).
 *   out[0] = sum phi * p / (B*H*W * sqrt(H^2 + W^2));  bwd: dp = g * phi / (B*H*W * sqrt(H^2 + W^2)).
 *
 * The backward calls recompute w / phi from the distance planes: no weight plane is ever stored.  amp and sigma of a
 * backward call are those of its forward.
 * Kernel layout.  Forward: 256-thread workgroups on a fixed grid of at most 64, a grid-stride loop with fp32 sums per
 *   thread, the workgroup's two sums added in double (block_sum_f64) and written to the workgroup's own workspace slot; a
 *   second launch of one workgroup adds the slots in slot order in double and writes fp32.  Backward: one element per
 *   thread and trip of a grid-stride loop, coalesced.
 * ws: him_bw_loss_ws() bytes, 8-byte aligned; every slot that is read is written by the call first.
 * HIM_E_INVALID before any launch, outputs untouched: a NULL pointer, B, C, hw, H, W or n < 1, kind outside {0, 1},
 *   amp < 0, sigma <= 0, a non-finite amp or sigma, a workspace not aligned to 8 bytes; HIM_E_WORKSPACE for a short one.
 * ------------------------------------------------------------------------------------------- */
size_t him_bw_loss_ws(void);
int him_bw_nll_fwd(const float* logp, const float* label, const float* mask, const int* dist2, int B, int C, int hw,
                   float amp, float sigma, float* out2, void* ws, size_t ws_bytes, void* stream);
int him_bw_nll_bwd(const float* label, const float* mask, const int* dist2, const float* g, const float* sum_w, float amp,
                   float sigma, float* dlogp, int B, int C, int hw, void* stream);
int him_bw_pair_fwd(const float* p, const float* t, const int* dist2, size_t n, int kind, float amp, float sigma,
                    float* out2, void* ws, size_t ws_bytes, void* stream);
int him_bw_pair_bwd(const float* p, const float* t, const int* dist2, size_t n, int kind, const float* g,
                    const float* sum_w, float amp, float sigma, float* dp, void* stream);
int him_surface_fwd(const float* p, const float* t, const int* d2_fg, const int* d2_bg, int B, int H, int W, float* out,
                    void* ws, size_t ws_bytes, void* stream);
int him_surface_bwd(const float* t, const int* d2_fg, const int* d2_bg, int B, int H, int W, const float* g, float* dp,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * Feathered canvas composite (the reference ships none: its paste_canvas replaces the whole output window as a hard
 * rectangle).  The image paste of a joint edit with a matte: full strength on and near the pixels the layout edit
 * changed, fading with the exact Euclidean distance to them, and fading towards every side of the paste window that has
 * photograph behind it.  Everything on `stream`, no host synchronisation, no workspace, no atomics, results bit-identical
 * from run to run.
 *
 * him_canvas_changed: changed[y][x] = before[y0+y][x0+x] != after[y0+y][x0+x], stored as 0 / 1; before / after are
 *   one-channel fp32 id canvases (Hc,Wc), never written; changed is an (H,W) uint8 plane: what him_edt reads as kind 0
 *   under HIM_EDT_NONZERO.  HIM_E_INVALID before any launch for a NULL pointer, H or W < 1 or a window
 *   [y0,y0+H) x [x0,x0+W) not inside the canvas.
 *
 * him_canvas_paste_blend_v: him_canvas_paste_bicubic_v's column pass (same tmp (rows,W,3), tables and byte arithmetic)
 *   with a matte.  P = byte / 255 (what that call would write), O = the canvas value already there.  For window pixel
 *   (x, y) every decision is an integer comparison:
 *     border term  d_b = min over the window sides NOT on the canvas edge of: left (x0 > 0) x + 1; right (x0 + W < Wc)
 *                  W - x; top (y0 > 0) y + 1; bottom (y0 + H < Hc) H - y.  No side counts: t_b = 1.  Otherwise
 *                  t_b = 1 if d_b >= feather, else (float)d_b / (float)feather.
 *     object term  dist2 NULL: t_o = 1.  Otherwise d2 = dist2[y][x] (int32 (H,W), a him_edt result over `changed`):
 *                  d2 == HIM_EDT_NONE: 0;  d2 <= reach^2: 1;  d2 >= (reach + feather)^2: 0 (64-bit comparisons);
 *                  otherwise t_o = 1 - (sqrtf((float)d2) - reach) / feather.
 *     matte        t = min(t_b, t_o); alpha = t (HIM_MATTE_LINEAR) or t * t * (3 - 2 t) (HIM_MATTE_SMOOTH); t = 0 and
 *                  t = 1 give exactly 0 and 1.  fp32, every operation rounded on its own (no contraction).
 *     canvas       alpha == 1: canvas = P, bit for bit;  alpha == 0: untouched (not even read);  otherwise
 *                  canvas = O + alpha * (P - O) in fp32.  One alpha for the three channels of canvas (3,Hc,Wc).
 *   matte: NULL, or fp32 (H,W) receiving alpha.  Nothing outside the window is read or written; each canvas element is
 *   read and written by one thread.  HIM_E_INVALID before any launch, outputs untouched, for a NULL tmp / first / count /
 *   weights / canvas, H, W or ksize < 1, a window not inside the canvas, feather outside 1..16384, reach outside
 *   0..16384, an unknown profile.
 *   Kernel layout: a 256-thread workgroup per tile of 64 columns x 4 rows of the window, lane = column, a wave per row,
 *   a pixel per thread; canvas, dist2 and matte rows move as 256 contiguous bytes per wave.
 * ------------------------------------------------------------------------------------------- */
#define HIM_MATTE_LINEAR 0
#define HIM_MATTE_SMOOTH 1
int him_canvas_changed(const float* before, const float* after, int Hc, int Wc, int x0, int y0, int H, int W,
                       unsigned char* changed, void* stream);
int him_canvas_paste_blend_v(const unsigned char* tmp, const int* first, const int* count, const int* weights, int ksize,
                             float* canvas, int Hc, int Wc, int x0, int y0, int H, int W, const int* dist2, int feather,
                             int reach, int profile, float* matte, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Seamless canvas composite (the reference ships none): gradient-domain (Poisson) cloning of a patch into the
 * photograph.  For the 5-point Laplacian on a rectangle the clone of P into O is exactly P + m, m being the discrete
 * harmonic function ("membrane") whose boundary values are O - P on the window's border.  Everything on `stream`, no host
 * synchronisation, no atomics, fp64 up to the stored fp32 membrane, results bit-identical from run to run.
 *
 * Window and sides: the window is H x W at (x0, y0) of an Hc x Wc canvas; a side is counted as in the feathered
 *   composite: left iff x0 > 0, right iff x0 + W < Wc, top iff y0 > 0, bottom iff y0 + H < Hc; l, r, t, b in {0,1}.
 *   The sides mask is l | r << 1 | t << 2 | b << 3.  Ring: the window's first / last row / column on each counted side.
 *   Interior: rows [t, H - b), columns [l, W - r); ny = H - t - b, nx = W - l - r.  ny < 1 or nx < 1: HIM_E_INVALID.
 *
 * Membrane, per channel: P (3,H,W) fp32 is the byte / 255 value the hard paste writes.  g = (double)O - (double)P on ring
 *   pixels.  For every interior pixel p:   deg(p) m(p) - sum_{q in N(p), q interior} m(q) = sum_{q in N(p), q in ring} g(q)
 *   N(p): the 4-neighbours of p inside the window, deg(p) = |N(p)|; a neighbour beyond an uncounted side does not exist
 *   (Neumann); a corner ring pixel is nobody's neighbour.  On the ring m := g.  No side counted: m := 0 and
 *   HIM_MEMBRANE_NO_SIDE is set in the status.  The dense float64 solve of these equations is the authority.
 *
 * Solver: per axis of length n with flags (lo, hi) the orthonormal basis V (n x n, V[j][k], j the pixel, k the mode) is
 *   the normalised columns of, with eigenvalue lam[k] of the 1-D second difference (j, k = 0..n-1):
 *     (1,1)  sin(pi (k+1)(j+1) / (n+1))          2 - 2 cos(pi (k+1) / (n+1))
 *     (0,0)  cos(pi k (2j+1) / (2n))             2 - 2 cos(pi k / n)
 *     (1,0)  sin(pi (2k+1)(j+1) / (2n+1))        2 - 2 cos(pi (2k+1) / (2n+1))
 *     (0,1)  sin(pi (2k+1)(n-j) / (2n+1))        as (1,0)
 *   m = Vy (Bh / (lamy_i + lamx_j)) Vx^T on the interior, Bh = Vy^T B Vx with B the right-hand side above:
 *     Bh[i][j] = Vy[0][i] (gT . Vx[:,j]) + Vy[ny-1][i] (gB . Vx[:,j]) + (Vy[:,i] . gL) Vx[0][j] + (Vy[:,i] . gR) Vx[nx-1][j]
 *   (terms of uncounted sides dropped; gT / gB: the ring rows above / below the interior's columns, gL / gR: the ring
 *   columns beside its rows).  lamy_0 + lamx_0 = 0 only when no side is counted, which never reaches the division.
 *
 * him_membrane_basis: V, its transpose Vt and lam (n doubles) of the pair (lo, hi) on the device.  The integer product in
 *   the sine / cosine argument is reduced modulo the period and folded into the first quarter in integers, then sinpi /
 *   cospi of the reduced rational: accuracy does not fall with n.  Columns are normalised by the square root of their
 *   fp64 sum of squares, added in a fixed order.  lam is evaluated as 4 sin^2 of the half angle.  HIM_E_INVALID: a NULL or
 *   misaligned pointer, V == Vt, n outside 1..2048, a flag outside {0,1}.
 * him_membrane_ws: bytes of workspace for an H x W window with the given sides mask; 0 for a refused shape.
 * him_membrane_solve: m (3,H,W) fp32: (float)g on the ring, the membrane on the interior.  Vy / Vyt / lamy: the basis of
 *   (ny, t, b); Vx / Vxt / lamx: of (nx, l, r); all may be NULL when no side is counted (ws too).
 *   status: 4 ints written by the device: [sides mask, ny, nx, flags].
 *   ws: him_membrane_ws bytes, 8-byte aligned; every slot that is read is written by the call first.
 *   HIM_E_INVALID before any launch, outputs untouched: a NULL canvas / P / m / status or a NULL basis with a side
 *   counted, a window not inside the canvas, ny or nx < 1 or > 2048, a workspace not aligned to 8 bytes;
 *   HIM_E_WORKSPACE: ws NULL with a side counted.
 *   Kernel layout: ring gather (a thread per ring pixel and channel) -> four matrix-vector products (a wave per output,
 *   fixed-order sums) -> the rank-4 update fused with the division -> a row-major fp64 GEMM run twice, grid z = channel:
 *   256 threads, a 64 x 64 tile as four waves of 2 x 2 v_mfma_f64_16x16x4_f64 accumulators, K step 16 staged through
 *   LDS at conflict-free pitches, edge tiles masked, plain vector stores; the second pass narrows to fp32 into m.
 *
 * him_canvas_seamless_apply: v = min(max(P + m, 0), 1) (one fp32 add, no contraction).  On the ring the canvas is left
 *   untouched (P + g is O).  On the interior the canvas becomes O + alpha (v - O) with alpha exactly the matte of
 *   him_canvas_paste_blend_v (same feather, reach, profile, dist2, same arithmetic); feather == 0: alpha = 1 (dist2 must
 *   be NULL and reach 0).  alpha == 1 writes v without reading the canvas; alpha == 0 touches nothing.  One alpha for the
 *   three channels.  matte: NULL, or fp32 (H,W) receiving alpha over the whole window, ring included.
 *   HIM_E_INVALID before any launch, outputs untouched: a NULL P / m / canvas, H or W < 1, a window not inside the
 *   canvas or without interior, feather outside 0..16384, reach outside 0..16384, dist2 or reach without feather, an
 *   unknown profile.  Kernel layout: the 64 x 4 tile of him_canvas_paste_blend_v, lane = column.
 * ------------------------------------------------------------------------------------------- */
#define HIM_MEMBRANE_NO_SIDE 1
#define HIM_MEMBRANE_MAX_N 2048
int him_membrane_basis(int n, int lo, int hi, double* V, double* Vt, double* lam, void* stream);
size_t him_membrane_ws(int H, int W, int sides);
int him_membrane_solve(const float* canvas, int Hc, int Wc, int x0, int y0, int H, int W, const float* P,
                       const double* Vy, const double* Vyt, const double* lamy, const double* Vx, const double* Vxt,
                       const double* lamx, float* m, void* ws, int* status, void* stream);
int him_canvas_seamless_apply(const float* P, const float* m, float* canvas, int Hc, int Wc, int x0, int y0, int H, int W,
                              const int* dist2, int feather, int reach, int profile, float* matte, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Region Poisson clone (the reference ships none): Poisson image editing of a patch into the photograph on an
 * ARBITRARY pixel set of the paste window, the photograph being Dirichlet data all around the set -- what keeps a moved
 * object's own pixels.  Everything on `stream`, no host synchronisation, no host read between launches, no atomics on
 * floating-point data, all vectors and scalars fp64, results bit-identical from run to run.
 *
 * Inputs: the photo canvas O (3,Hc,Wc) fp32, a window H x W at (x0, y0) inside it, the patch P (3,H,W) fp32 (what a hard
 *   paste would write on the window), a region plane (H,W) uint8 (nonzero: clone this pixel), mixed in {0,1}.
 * Sides and ring: as in "Seamless canvas composite" (left counted iff x0 > 0, ...; sides mask l | r << 1 | t << 2 |
 *   b << 3; ring = the window's first / last row / column on each counted side).
 * Unknown set Omega = {region != 0} minus the ring.  N(p): the 4-neighbours of p inside the window (none beyond an
 *   uncounted side: Neumann), deg(p) = |N(p)| in 2..4.  Per channel, for p in Omega, with f~(q) = f(q) for q in Omega and
 *   O(q) otherwise:
 *       deg(p) f(p) - sum_{q in N(p)} f~(q) = sum_{q in N(p)} v_pq
 *   mixed 0: v_pq = P(p) - P(q).   mixed 1: v_pq = O(p) - O(q) when |O(p) - O(q)| > |P(p) - P(q)| (strictly: ties take
 *   the patch), else P(p) - P(q).  All differences in fp64 from the fp32 values.
 *   The solver works on the correction u = f - P (0 outside Omega):
 *       deg(p) u(p) - sum_{q in N(p) in Omega} u(q) = sum_{q in N(p) not in Omega} (O(q) - P(q))
 *                                                     [+ sum_{q in N(p)} (v_pq - (P(p) - P(q))) when mixed]
 *   The system is symmetric positive definite unless Omega is the whole window and no side is counted
 *   (HIM_REGION_POISSON_SINGULAR: u := 0).  The dense float64 solve of these equations is the authority.
 *
 * him_region_poisson_ws: bytes of workspace for an H x W window; 0 for H or W outside 1..2048.
 * him_region_poisson_solve: conjugate gradients, no preconditioner, the three channels in lockstep with their own
 *   scalars.  A channel stops when r.r <= rtol^2 b.b and is frozen: none of its vectors is touched again.  b.b == 0: u = 0,
 *   0 iterations, resid 0, no division is reached; p.Ap <= 0 stops the channel the same way.  At most max_iter
 *   iterations (the callers' default is 6 (H + W): CG on the full L x L window, the worst region a window admits, has
 *   sqrt(kappa) ~ 0.64 L and reaches 1e-10 in about 7.6 L iterations, the cap there is 12 L; a cap, not a measurement).
 *   u      (3,H,W) fp64: the correction, exactly 0 outside Omega.
 *   resid  fp64[3]: the recursive ||r||_2 / ||b||_2 of each channel at its stop (0 where b.b == 0 or a flag of bits 0, 1, 3
 *          is set).
 *   status int32[8]: [sides mask, |Omega|, region pixels dropped on the ring, iterations run (maximum over channels),
 *          flags, 0, 0, 0].  Flags: HIM_REGION_POISSON_EMPTY (Omega is empty, nothing solved), _SINGULAR (above),
 *          _MAX_ITER_HIT (a channel ended above rtol), _NONFINITE (a non-finite value of P or O was read on Omega or on
 *          its neighbours: u := 0).
 *   ws     him_region_poisson_ws bytes, 8-byte aligned; every slot that is read is written by the call first.
 *   HIM_E_INVALID before any launch, outputs untouched: a NULL canvas / P / region / u / status / resid, a window not
 *   inside the canvas, H or W < 1 or > 2048, rtol outside (0, 1) or NaN, max_iter < 1 or > 2^20 (the call enqueues
 *   2 max_iter + 2 launches), mixed outside {0,1}, u, resid or ws not aligned to 8 bytes.  HIM_E_WORKSPACE: ws NULL or
 *   ws_bytes too small.
 *   Kernel layout: 256-thread workgroups own 64 x 4 tiles (lane = column, the three channels in one thread), at most
 *   1024 workgroups taking the tiles in strides.  init (deg plane, b, u := 0, partial b.b and counts) -> per iteration
 *   dir (the sum of the r.r partials, the stop decision and beta in every workgroup, p = r + beta p_old evaluated at the
 *   pixel and its neighbours from the other of two direction buffers, A p, partial p.Ap) and upd (the sum of the p.Ap
 *   partials, alpha, u += alpha p, r -= alpha A p, partial r.r) -> finish (status, resid).  Iteration boundaries are
 *   kernel boundaries; once every channel has stopped a launch returns after loading three ints.
 * him_region_poisson_apply: canvas[p] = min(max((float)(P(p) + u(p)), 0), 1) for p in Omega: the sum of the fp32 patch
 *   value and the fp64 correction is narrowed to fp32 once, its only fp32 rounding; every other canvas element is neither
 *   read nor written.  HIM_E_INVALID: a NULL pointer, a window not inside the canvas, H or W
 *   outside 1..2048, u not aligned to 8 bytes.
 * ------------------------------------------------------------------------------------------- */
#define HIM_REGION_POISSON_EMPTY 1
#define HIM_REGION_POISSON_SINGULAR 2
#define HIM_REGION_POISSON_MAX_ITER_HIT 4
#define HIM_REGION_POISSON_NONFINITE 8
#define HIM_REGION_POISSON_MAX_N 2048
#define HIM_REGION_POISSON_MAX_ITER 1048576
size_t him_region_poisson_ws(int H, int W);
int him_region_poisson_solve(const float* canvas, int Hc, int Wc, int x0, int y0, int H, int W, const float* P,
                             const unsigned char* region, int mixed, double rtol, int max_iter, double* u, int* status,
                             double* resid, void* ws, size_t ws_bytes, void* stream);
int him_region_poisson_apply(const float* P, const double* u, const unsigned char* region, float* canvas, int Hc, int Wc,
                             int x0, int y0, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Layout edits (the reference ships none: its public path only adds an object): take an instance out of a (label,
 * instance) canvas pair and fill the hole, and write an instance of one pair into another at another place and size.
 * Everything on `stream`, no host synchronisation, integer work, integer atomics only (add / or / min / max): results
 * bit-identical from run to run.  Planes are (H,W) of kind 0 uint8 / 1 int32 / 2 int64 / 3 fp32 holding integral ids
 * (him_edt's kinds), label and instance plane each of its own kind; outputs have the kind of their input.  A class bit
 * table is uint32 words on the device, class c being bit (c & 31) of word c >> 5, (n_class + 31) / 32 words.
 *
 * him_layout_erase: R = {p : region[p] != 0} when region (uint8 (H,W)) is given, else {p : inst[p] == id}.  Seeds
 *   S = {p not in R : 0 <= label[p] < n_class and label[p] in fill}.  s(p) = the seed nearest to p in squared Euclidean
 *   distance, among equidistant seeds the smallest y * W + x: him_edt's feature transform, run by this call on a seed
 *   plane it writes into the workspace (the transform is not restated).  For p in R with 0 <= label[p] < n_class:
 *   label_out[p] = label[s(p)], inst_out[p] = inst[s(p)]; every other pixel is copied.  changed[p] (uint8 (H,W)) =
 *   label_out[p] != label[p].
 *   status: 4 ints written by the device: [|R|, |S|, pixels whose label changed, flags].  HIM_LAYOUT_NO_SEED: S is empty,
 *           both planes come out as copies, changed is zero.  HIM_LAYOUT_CLASS_RANGE: a label outside [0, n_class) (or
 *           not integral) was seen; such pixels are never seeds and are never rewritten.
 *   ws:     him_layout_erase_workspace(H, W) bytes (0 for a refused shape), 16-byte aligned; written before it is read.
 *   HIM_E_INVALID before any launch: H or W outside 1..16384, an unknown kind, n_class outside 1..65536, a NULL label /
 *   inst / fill / label_out / inst_out / changed / status, a pointer not aligned to its element, an output that overlaps
 *   an input or another output.  HIM_E_WORKSPACE: ws NULL or short.
 *   Kernel layout: init (one thread), the seed pass (grid-stride, a pixel per thread and trip: region test, table
 *   lookup, the seed byte, the copies, |R| and the range flag with one atomic per wave), him_edt's three launches, the
 *   gather pass (grid-stride; reads both planes at nearest[p], counts the changed pixels, copies the seed count).
 *
 * him_layout_place: the mask Rs = {p in the source box [sx0, sy0, sx1, sy1) : inst_src[p] == id} of an (Hs,Ws) plane,
 *   resampled to the destination box [dx0, dy0, dx1, dy1) of an (Hd,Wd) pair: destination pixel (x, y) of the box reads
 *   source pixel (sx0 + xs[x - dx0], sy0 + ys[y - dy0]); xs (dx1 - dx0 ints) and ys (dy1 - dy0 ints) are index tables on
 *   the device, Pillow's NEAREST tables for a bit-identical Image.resize of the cropped mask (an entry outside the source
 *   box reads as unset).  Where the resampled mask is set and the pixel lies inside the canvas (the box may hang over any
 *   edge): if protect is given and the pixel's current class is in it, the pixel is counted as blocked and left alone;
 *   otherwise label_dst = cls, inst_dst = new_id and, with changed (uint8 (Hd,Wd), may be NULL) given, changed = 1.
 *   Nothing else is written; label_dst / inst_dst are edited in place.  inst_src and inst_dst share inst_kind.
 *   status: 6 ints written by the device: [pixels written, pixels blocked, xmin, ymin, xmax, ymax of the written
 *           pixels], zero-based inclusive as him_inst_summary's rows; [2147483647, 2147483647, -1, -1] when none.
 *   HIM_E_INVALID before any launch: a plane side outside 1..16384, an unknown kind, a source box that is empty or not
 *   inside its plane, an empty destination box or one beyond +-2^20, n_class outside 1..65536 with protect given, cls /
 *   new_id that the planes' kinds cannot hold (uint8: 0..255, fp32: |v| <= 2^24), a NULL inst_src / xs / ys / label_dst /
 *   inst_dst / status, a misaligned pointer, inst_src overlapping a destination plane (a move reads the mask from the
 *   original canvas and writes onto the erased copy), destination planes overlapping each other.
 *   Kernel layout: status init; a 256-thread workgroup per tile of 64 columns x 4 rows of the clipped box, lane =
 *   column, a pixel per thread; wave reductions in front of the atomics.
 * ------------------------------------------------------------------------------------------- */
#define HIM_LAYOUT_NO_SEED 1
#define HIM_LAYOUT_CLASS_RANGE 2
size_t him_layout_erase_workspace(int H, int W);
int him_layout_erase(const void* label, int label_kind, const void* inst, int inst_kind, const unsigned char* region,
                     int id, int H, int W, const unsigned int* fill, int n_class, void* label_out, void* inst_out,
                     unsigned char* changed, int* status, void* ws, size_t ws_bytes, void* stream);
int him_layout_place(const void* inst_src, int inst_kind, int Hs, int Ws, int id, int sx0, int sy0, int sx1, int sy1,
                     const int* xs, const int* ys, void* label_dst, int label_kind, void* inst_dst, int Hd, int Wd, int dx0,
                     int dy0, int dx1, int dy1, int cls, int new_id, const unsigned int* protect, int n_class,
                     unsigned char* changed, int* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Affine layout edits (the reference ships none): rotate, mirror, shear or scale an instance and the pixels that go with
 * it.  One geometric primitive, an inverse-mapped affine resampling -- NEAREST for ids, BICUBIC for pixels -- in front of
 * the unchanged machinery of "Layout edits" and "Region Poisson clone".  Everything on `stream`, no host
 * synchronisation, no workspace, results bit-identical from run to run.
 *
 * The map.  Pixel index i has its centre at coordinate i.  `inv` points to six int64 coefficients on the HOST (copied
 * into the kernel arguments by the call; no device table, no upload), [a00, a01, a02, a10, a11, a12], the INVERSE map in
 * units of 2^-24 source pixel: for the destination canvas indices (x, y)
 *       U = a00 x + a01 y + a02        V = a10 x + a11 y + a12
 *   nearest source pixel: xs = (U + 2^23) >> 24, ys = (V + 2^23) >> 24, arithmetic shifts (floor): the only tie rule.
 *   bicubic: ix = U >> 24, tx = (U & (2^24 - 1)) 2^-24 (exact), iy / ty from V alike; taps ix - 1 .. ix + 2 by
 *     iy - 1 .. iy + 2, indices clamped to the source plane (edge replicate); weights: Keys' kernel, a = -0.5, at the
 *     distances 1 + t, t, 1 - t, 2 - t.  Point sampling, no prefilter: below scale 1 it aliases (the callers bound the
 *     minification).  A zero fraction gives the weights (0, 1, 0, 0) exactly.
 *   Limits: |a00|, |a01|, |a10|, |a11| <= 2^30 (a coefficient of 64), |a02|, |a12| <= 2^52.  Destination coordinates lie
 *     inside +-(2^20 + 2^14), so each product stays below 2^51 and no sum leaves int64 (|U|, |V| < 2^53).  All
 *     geometry is integer arithmetic: a 64-bit integer restatement gives the device's bits.
 *
 * him_layout_place_affine: him_layout_place with the tables xs / ys replaced by `inv`.  For every pixel (x, y) of the
 *   destination box [dx0, dy0, dx1, dy1) inside the canvas the resampled mask is set iff sx0 <= xs < sx1 and
 *   sy0 <= ys < sy1 and inst_src[ys, xs] == id (anything outside the source box reads as unset).  Everything else is
 *   him_layout_place's contract: protect and the blocked count, label_dst = cls, inst_dst = new_id, changed = 1, the
 *   six-int status, the four plane kinds, the refusals (with a NULL or 8-byte-misaligned inv and a coefficient beyond
 *   the limits in the place of the tables'), the kernel layout, integer atomics behind wave reductions only.
 *
 * him_canvas_warp_affine: P[c, y, x] (3,H,W) fp32 = the bicubic sample above of src (3,Hs,Ws) fp32 at the destination
 *   pixel (x0 + x, y0 + y).  Values are used as they are: no 8-bit round trip, no clamp to [0,1] (the overshoot of the
 *   cubic stays; him_region_poisson_apply clamps at the end).  Non-finite source values are not special-cased: they
 *   propagate through the taps that read them, a tap of weight 0 included.  Weights and sums in fp64 (48 multiply-adds
 *   per pixel), narrowed to fp32 once per output.  On a map with zero fractions the result is the source value bit for
 *   bit, with one exception: the sum starts from +0, so a source -0.0 comes out as +0.0.
 *   HIM_E_INVALID before any launch: source sides outside 1..16384, H or W outside 1..2048 (the window
 *   him_region_poisson_solve accepts), |x0| or |y0| > 2^20, a NULL or misaligned src / inv / P, P overlapping src, a
 *   coefficient beyond the limits.
 *   Kernel layout: a 256-thread workgroup per tile of 64 columns x 4 rows of the window, lane = column, the three
 *   channels in one thread, taps gathered straight from global memory, plain stores; no atomics.
 * ------------------------------------------------------------------------------------------- */
#define HIM_AFFINE_FRAC_BITS 24
#define HIM_AFFINE_MAX_WINDOW 2048
int him_layout_place_affine(const void* inst_src, int inst_kind, int Hs, int Ws, int id, int sx0, int sy0, int sx1, int sy1,
                            const long long* inv, void* label_dst, int label_kind, void* inst_dst, int Hd, int Wd, int dx0,
                            int dy0, int dx1, int dy1, int cls, int new_id, const unsigned int* protect, int n_class,
                            unsigned char* changed, int* status, void* stream);
int him_canvas_warp_affine(const float* src, int Hs, int Ws, const long long* inv, int x0, int y0, int H, int W, float* P,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * Set-level metrics (the reference ships none): the sliced Wasserstein distance between the Laplacian-pyramid patches of
 * two SETS of images (Karras et al., "Progressive Growing of GANs", ICLR 2018, section 5 and its sliced_wasserstein.py).
 * No network, no weights; everything on `stream`, no host synchronisation, no allocation, results bit-identical from
 * run to run.  Every entry checks its arguments and returns HIM_E_INVALID / HIM_E_WORKSPACE before any launch.
 *
 * Pyramid of a planar fp32 batch x (B,C,H,W), C = 1 or 3.  k = [1, 4, 6, 4, 1] / 16, borders mirrored WITHOUT repeating
 * the edge pixel (d c b | a b c d | c b a; SciPy's mode='mirror').  G_0 = x; G_{i+1} = down(G_i): filter with k in both
 * directions and keep the even rows and columns; up(g): write g to the even positions of a zero plane of twice the size
 * and filter with 2 k in both directions, same border rule.  L_i = G_i - up(G_{i+1}), and the last level is G_last.
 *   him_lap_levels(H, W, want): the largest count such that the smallest level keeps min(H, W) >= 16 (0 when there is
 *     none), or `want` when that is positive and smaller.
 *   him_lap_level_offset(B, C, H, W, l): the element offset of level l in the packed output, the sum over i < l of
 *     B C (H >> i) (W >> i); level l there is a dense (B, C, H >> l, W >> l) tensor.  l = levels gives the total size.
 *   him_lap_pyramid: lap receives the `levels` Laplacian levels, packed.  gauss: NULL, or the Gaussian levels
 *     1 .. levels - 1 packed from him_lap_level_offset(l) - him_lap_level_offset(1) (what separates down from up in a
 *     test).  ws: him_lap_pyramid_ws bytes (the same Gaussian levels; written before it is read), 4-byte aligned.
 *     Refused: C outside {1, 3}; levels < 1 or above him_lap_levels(H, W, 0); H or W not divisible by 2^(levels - 1);
 *     B C H W > 2^40; a NULL x / lap / ws; a short workspace (the query returns 0 for a refused shape).
 *     2 levels - 1 launches: down stages the 19 x 131 inputs of a tile of 8 x 64 outputs in LDS, mirror indices resolved
 *     while staging, so a pass reads each input pixel from memory once but for the tile halo; up-and-subtract stages the
 *     6 x 34 coarse cells of an 8 x 64 tile and evaluates the zero-insertion filter literally.
 *
 * Descriptors.  him_swd_gather copies, for every image b and patch p, the HIM_SWD_PATCH x HIM_SWD_PATCH x C patch of
 * `level` (B,C,h,w) whose top-left corner is pos[b][p] = (y, x) (int32 (B,n_patches,2) on the device) into row
 * row0 + b n_patches + p of desc (capacity, 49 C), channel-major: column c 49 + r 7 + q = level[b][c][y + r][x + q].
 * A corner outside [0, h - 7] x [0, w - 7] is clamped into it and counted: status[0] += the number of clamped corners
 * (an integer atomic; the caller zeroes the word).  The same pass folds the copied values into stats, 4 C doubles
 * [sum, sum of squares, minimum, maximum] per channel, which the caller starts at [0, 0, +inf, -inf]: each image's
 * partial is a fixed tree over the thread slots of its workgroup and a second launch adds the partials to stats in
 * image order, so a set streamed in any batch sizes ends with the same bits.  ws: him_swd_gather_ws(B, C) bytes, 8-byte
 * aligned.  Refused: C outside {1, 3}, h or w < 7, n_patches outside 1..65536, rows outside [0, capacity).
 *
 * Normalisation and projection.  him_swd_project derives per channel, in double, mean = sum / (49 N) and the POPULATION
 * deviation sqrt(sum2 / (49 N) - mean^2) from stats and writes
 *   out[d][n] = sum_k dirs[k][d] * (desc[n][k] - mean[c(k)]) / deviation[c(k)],  c(k) = k / 49,
 * for the first N rows of desc: dirs is fp32 (49 C, n_dirs), out fp32 (n_dirs, N), direction-major so that every
 * direction is one contiguous segment for the sort.  A channel with minimum == maximum (or a deviation that is not
 * positive) sets HIM_SWD_ZERO_DEVIATION in status[0] (atomic or; the caller zeroes the word) and makes every output
 * NaN.  Plain FMA in double, k ascending: K = 49 C <= 147 is too short for a matrix-core pipeline to repay its operand
 * shuffles, and double keeps the result within one rounding of the exact sum.  N * n_dirs <= 2^31 - 1.
 *
 * him_sort_segments sorts S contiguous segments of N fp32 keys each, in place, ascending in the order of the sign-fixed
 * bit pattern  key(b) = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000)  compared as unsigned: NaNs with the sign bit, -inf,
 * negative values, -0, +0, positive values, +inf, NaNs without the sign bit.  Bits are moved, never changed.  status[0] =
 * the number of NaNs among the keys (written by the call).  Not stable (there is no payload to tell).  Two regimes:
 * N <= HIM_SORT_LDS_MAX: one workgroup per segment, a bitonic network in LDS; longer segments: chunks of HIM_SORT_LDS_MAX
 * keys sorted the same way, then ceil(log2(chunks)) merge passes through global memory between keys and ws, every key
 * finding its slot by a binary search of the partner run.  ws: him_sort_segments_ws(S, N) bytes (16 in the LDS regime,
 * S N floats beyond), 4-byte aligned.  Refused: S or N < 1, S * N > 2^31 - 1, a short workspace.
 *
 * him_swd_distance: a, b fp32 (n_dirs, N), each direction sorted.  dir_sums[d] = sum_n |a[d][n] - b[d][n]| in double
 * (thread t of the direction's workgroup adds n = t, t + 256, ..., then a fixed tree); mean[0] = sum_d dir_sums[d] /
 * (n_dirs N), the level's distance.  Na != Nb is refused.
 * ------------------------------------------------------------------------------------------- */
#define HIM_SWD_PATCH 7
#define HIM_LAP_MAX_LEVELS 12
#define HIM_SORT_LDS_MAX 8192
#define HIM_SWD_ZERO_DEVIATION 1
unsigned him_lap_levels(int H, int W, int want);
long long him_lap_level_offset(int B, int C, int H, int W, int level);
size_t him_lap_pyramid_ws(int B, int C, int H, int W, int levels);
int him_lap_pyramid(const float* x, int B, int C, int H, int W, int levels, float* lap, float* gauss, void* ws,
                    size_t ws_bytes, void* stream);
size_t him_swd_gather_ws(int B, int C);
int him_swd_gather(const float* level, int B, int C, int h, int w, const int* pos, int n_patches, float* desc,
                   long long capacity, long long row0, double* stats, int* status, void* ws, size_t ws_bytes, void* stream);
int him_swd_project(const float* desc, long long N, int C, const double* stats, const float* dirs, int n_dirs, float* out,
                    int* status, void* stream);
size_t him_sort_segments_ws(long long S, long long N);
int him_sort_segments(float* keys, long long S, long long N, int* status, void* ws, size_t ws_bytes, void* stream);
int him_swd_distance(const float* a, long long Na, const float* b, long long Nb, int n_dirs, double* dir_sums, double* mean,
                     void* stream);

/* ----------------------------------------------------------------------------------------------
 * Feature-space set metrics (the reference ships none): the distance between a generated and a real SET in the feature
 * space of a frozen network -- KID (Binkowski et al., "Demystifying MMD GANs", ICLR 2018: the unbiased MMD^2 estimate
 * with the kernel k(x, y) = (gamma x.y + coef0)^3) and the Frechet distance between the Gaussians fitted to the two sets
 * (Heusel et al. 2017; FID's formula on whatever features are supplied).  Everything on `stream`, no host
 * synchronisation, no allocation, no floating-point atomics, results bit-identical from run to run.  Every entry checks
 * its arguments and returns HIM_E_INVALID / HIM_E_WORKSPACE, with a him_last_error() text that names it, before any
 * launch: a refused call writes nothing.
 *
 * him_feat_pool: feat[(row0 + b) D + c0 + c] = the mean over the h w plane of x[b][c], x planar fp32 (B,C,h,w), summed
 * in double (thread t of the plane's workgroup adds elements t, t + 256, ..., then a fixed tree) and rounded to fp32
 * once.  feat is a (capacity, D) fp32 matrix; several feature maps are concatenated into one row by one call each with
 * its own c0.  Nothing else of feat is written.  Refused: a size < 1, h w > 2^31 - 1, B C h w > 2^40,
 * row0 < 0 or row0 + B > capacity, c0 < 0 or c0 + C > D.
 *
 * him_feat_moments ADDS to the float64 accumulators sum[D] and second[D D] the column sums and X^T X of the rows
 * row0 .. row0 + n - 1 of the fp32 matrix feat with row length D, so that a set can be streamed batch by batch (the
 * caller starts both at zero).  second is the full matrix; its two triangles receive the same bits (a wave computes a
 * 16 x 16 tile of the upper triangle and writes it and its mirror image).  The products run on v_mfma_f64_16x16x4_f64
 * with the operands widened fp32 -> fp64 on load: every product is exact, only the summation (rows ascending, four per
 * instruction) rounds.  1 <= D <= HIM_FEAT_MAX_DIM; neither D nor n need be a multiple of the tile: the padding lives
 * in registers and nothing is read past a row or past the last row.  ws: him_feat_moments_ws(n, D) bytes, 8-byte
 * aligned (16 bytes today: one wave owns a tile for all n rows, so there are no partials to park; 0 for a refused
 * shape).
 *
 * him_kid_sums: x (nx, D) and y (ny, D) fp32; ix, iy int32 (n_subsets, m) row indices into x and y.  For subset s
 *   out[3 s + 0] = sum_{i != j} k(x_ix[s][i], x_ix[s][j]),   out[3 s + 1] = the same over y and iy,
 *   out[3 s + 2] = sum_{i, j} k(x_ix[s][i], y_iy[s][j]),     k(a, b) = (gamma a.b + coef0)^3,
 * float64, i and j POSITIONS in the subset (the diagonal is excluded by position, not by row index), every sum over
 * ordered pairs.  gamma == 0 means 1 / D.  The dot products run on v_mfma_f64_16x16x4_f64 (exact products, k
 * ascending in groups of sixteen columns), the cube and both masks on the accumulators; a workgroup owns a 64 x 64 tile
 * of pairs and leaves one partial in ws (tiles below the diagonal of the two symmetric blocks are skipped, those above
 * count twice, which is exact), and a second launch adds a subset's partials in tile order.  An index outside [0, nx)
 * (or [0, ny)) is never dereferenced: it sets HIM_KID_BAD_INDEX in the int32 status[0] (atomic or; the caller zeroes
 * the word) and makes the three sums of its subset NaN; other subsets are unaffected.  ws: him_kid_sums_ws(n_subsets, m)
 * bytes, 8-byte aligned.  Refused: m outside 2..65536, n_subsets outside 1..65535, D outside 1..2^20, nx or ny outside
 * 1..2^31 - 1, a negative or non-finite gamma, a non-finite coef0, a short workspace.
 *
 * k-nearest-neighbour manifold estimates (improved precision / recall, Kynkaanniemi et al. 2019; density / coverage,
 * Naeem et al. 2020).  d2(a, b) is the squared Euclidean distance of two fp32 rows in the Gram form
 * |a|^2 + |b|^2 - 2 a.b: operands widened to fp64 on load (every product exact), the dot products on
 * v_mfma_f64_16x16x4_f64 (k ascending in groups of sixteen columns), the norms once per row in fp64, the result clamped
 * at 0.  Both entries use the same arithmetic; neither stores the matrix of pairs.  Neither the row counts nor D need be
 * a multiple of a tile; nothing is read past a row or past the last row.
 *
 * him_knn_radii: x (n, D) fp32; radii2[i], float64, = the k-th smallest d2(x_i, x_j) over j != i.  Self is excluded by
 * position, not by value: a duplicate row is a neighbour at distance 0.  A workgroup owns 64 rows and a chunk of the
 * columns and keeps, per row, the smallest values in a sorted register list; its first k go to ws, and a second launch
 * merges a row's partial lists in chunk order.  The k smallest values of a set do not depend on the order they are met
 * in, and there are no floating-point atomics: two runs give identical bits.  1 <= k <= HIM_KNN_MAX_K, k < n <=
 * 2^31 - 1, 1 <= D <= HIM_FEAT_MAX_DIM.  ws: him_knn_radii_ws(n, D, k) bytes, 8-byte aligned (the norms and at most
 * sixteen partial lists per row; 0 for a refused shape).
 *
 * him_knn_membership: q (nq, D) and r (nr, D) fp32, radii2 (nr) float64 -- the radii of the REFERENCE rows r.  With
 *   I[j][i] = [ d2(q_j, r_i) <= radii2[i] ]      row_count[j] = sum_i I[j][i]      col_count[i] = sum_j I[j][i],
 * int32; the call itself clears both (integer atomics add the non-zero tile sums: exact and order-free).  Either count
 * pointer may be NULL to skip it, not both.  ws: him_knn_membership_ws(nq, nr, D) bytes, 8-byte aligned.
 *
 * A row with a non-finite feature sets HIM_KNN_NONFINITE in the int32 status[0] (atomic or; the caller zeroes the word).
 * Every distance to or from it is NaN, which passes no comparison: it is nobody's neighbour, it lies within no radius
 * and nothing lies within its own, which is NaN.  The other rows are unaffected; one with fewer than k finite
 * neighbours has the radius +inf.  Refused: k, n, nq, nr or D outside the limits above, a NULL or misaligned x, q, r,
 * radii2, status or ws, a short ws_bytes.
 * ------------------------------------------------------------------------------------------- */
#define HIM_FEAT_MAX_DIM 4096
#define HIM_KID_BAD_INDEX 1
#define HIM_KNN_MAX_K 16
#define HIM_KNN_NONFINITE 1
int him_feat_pool(const float* x, int B, int C, int h, int w, float* feat, long long capacity, long long row0, int D, int c0,
                  void* stream);
size_t him_feat_moments_ws(long long n, int D);
int him_feat_moments(const float* feat, long long row0, long long n, int D, double* sum, double* second, void* ws,
                     size_t ws_bytes, void* stream);
size_t him_kid_sums_ws(int n_subsets, int m);
int him_kid_sums(const float* x, long long nx, const float* y, long long ny, int D, const int* ix, const int* iy, int n_subsets,
                 int m, double gamma, double coef0, double* out, int* status, void* ws, size_t ws_bytes, void* stream);
size_t him_knn_radii_ws(long long n, int D, int k);
int him_knn_radii(const float* x, long long n, int D, int k, double* radii2, int* status, void* ws, size_t ws_bytes,
                  void* stream);
size_t him_knn_membership_ws(long long nq, long long nr, int D);
int him_knn_membership(const float* q, long long nq, const float* r, long long nr, int D, const double* radii2, int* row_count,
                       int* col_count, int* status, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Panoptic matching (the reference ships no metric code; panoptic quality PQ = SQ x RQ of Kirillov et al., "Panoptic
 * Segmentation", CVPR 2019): the instance-aware comparison of a predicted layout with the ground truth.  One call on
 * `stream`, no host synchronisation, no allocation; integer counting throughout, results bit-identical from run to run.
 * Each plane b of the batch is handled independently.
 *   pred_seg, gt_seg: (B,H,W) segment ids, kind 0 uint8 / 1 int32 / 2 int64; accepted ids 0..65535 (the id domain of
 *            him_inst_summary and of what him_label_instances writes).  Never written.
 *   pred_cls, gt_cls: (B,H,W) classes, kind 0 uint8 / 1 int32 / 2 int64 / 3 fp32 holding integral values; accepted
 *            0..n_class-1, 1 <= n_class <= 256.  Never written.
 *   mask:    NULL, or fp32 (B,H,W).
 *   Void:    a pixel is void where mask == 0, or where its ground-truth class equals `ignore` (-1: none; compared before
 *            the range check, so it may be >= n_class).  A void pixel belongs to no ground-truth segment -- its
 *            ground-truth id and class are not examined -- but it still belongs to its predicted segment.
 *   Segment: the set of a plane's pixels with one id (ground truth: non-void pixels only); its class is the smallest
 *            class value under it; classes that are not all equal set HIM_PQ_MIXED (informational, the plane is still
 *            counted).  Segments are ranked per side in ascending id (np.unique's order).
 *   Matching, in integers, of ground-truth segment g and predicted segment p: inter = |g n p|, void_p = |p n void|,
 *            union = |g| + |p| - inter - void_p; they match iff their classes are equal and 2 * inter > union.  Such a
 *            match is unique on both sides (csrc/him_panoptic.hip has the proof).
 *   Counts per class: a matched pair adds 1 to tp of its class and (double)inter / (double)union to iou_sum; an
 *            unmatched ground-truth segment adds 1 to fn; an unmatched predicted segment adds 1 to fp unless
 *            2 * void_p > |p|.  No crowd regions.
 *   counts:  int64 (n_class,3) = tp, fp, fn.   iou_sum: double (n_class).  accumulate != 0 adds into both (and into
 *            status: the two counts are added, the flags or-ed); otherwise they are overwritten.  Each class has one
 *            writer, which adds its IoU terms in a fixed order; no floating-point atomics.
 *   matches: NULL, or int32 (B,max_segments,6): one row per ground-truth segment in rank order: id, class, area,
 *            matched predicted id or -1, inter, union (0, 0 when unmatched).  Rows behind the plane's segment count are
 *            not written.
 *   status:  int32 (B,4): [ground-truth segments, predicted segments, flags, 0]; the counts are the true ones (of the
 *            ids inside 0..65535), also past max_segments.  Flags: HIM_PQ_OVERFLOW (either side has more than
 *            max_segments), HIM_PQ_ID_RANGE (an id outside 0..65535), HIM_PQ_CLS_RANGE (a class outside 0..n_class-1 or
 *            a non-integral fp32), HIM_PQ_MIXED.  A plane with any of the first three adds nothing to counts or iou_sum,
 *            its matches rows are unspecified and its HIM_PQ_MIXED bit is clear; the other planes are unaffected.
 *            HIM_PQ_CCL is never set by the library: the caller's spare bit (util/metrics.py marks a plane whose
 *            instance labelling reported a flag of its own).
 *   ws:      him_panoptic_match_workspace(B, max_segments) bytes, 16-byte aligned, cleared by the call itself;
 *            1 <= max_segments <= 4096 (a dense (max_segments + 1) x max_segments int32 pair table per plane, of which
 *            a call touches (ground-truth segments + 1) x predicted segments).
 * Nothing outside counts, iou_sum, matches, status and ws is ever written.  Seven launches: clear, segment pass (one
 * integer atomic per run of equal ids into a table of 65536 ids per plane and side), rank pass (prefix sum of the present
 * ids), clear of the pair table, pair pass (one atomic per run of equal pairs), match pass (a wave per ground-truth
 * segment), reduce pass (a wave per class).  A lane reads 4 pixels of every plane per step, as one vector load where every
 * base is 16-byte aligned and W % 4 == 0, element by element otherwise.  No cooperative launch, no workgroup waits for
 * another.
 * HIM_E_INVALID before any launch: a NULL required pointer, an unknown kind, B, H or W < 1, B > 65535,
 * H * W > 2^31 - 1, n_class or max_segments out of range, ignore < -1, a plane not aligned to its element, a misaligned
 * output or workspace; HIM_E_WORKSPACE for a short workspace (the query returns 0 for a refused shape).
 * ------------------------------------------------------------------------------------------- */
#define HIM_PQ_OVERFLOW 1
#define HIM_PQ_ID_RANGE 2
#define HIM_PQ_CLS_RANGE 4
#define HIM_PQ_MIXED 8
#define HIM_PQ_CCL 16
size_t him_panoptic_match_workspace(int B, int max_segments);
int him_panoptic_match(const void* pred_seg, int pred_seg_kind, const void* pred_cls, int pred_cls_kind,
                       const void* gt_seg, int gt_seg_kind, const void* gt_cls, int gt_cls_kind, const float* mask, int B,
                       int H, int W, int n_class, int ignore, int max_segments, int accumulate, long long* counts,
                       double* iou_sum, int* matches, int* status, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIM_H_ */
