/*
 * innfer_amd.h -- flat C ABI of the MI355X (gfx950) hot path for victorca25/iNNfer.
 *
 * Scope (SURVEY.md section 8): generator forward (ESRGAN RRDBNet / SRResNet) +
 * chop_forward tile extraction and overlap blend + uint8<->float pre/post.
 * The reference has no FFI; each entry point below names the reference
 * interface (file:line in victorca25/iNNfer) it replaces.  INTEGRATION.md shows
 * the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 (INNFER_OK) or a negative innfer_status; no C++
 *     exception crosses the boundary; innfer_last_error() gives the thread's
 *     last message.
 *   - pointers named d_* are device (HBM) pointers owned by the caller (e.g.
 *     torch storages); h_* are host pointers.  `stream` is a hipStream_t passed
 *     as void* (NULL = default stream).  Nothing synchronises the stream.
 *   - activations inside the library are fp16 blocked-NHWC channel slabs, accumulated
 *     in fp32 on MFMA; tensors at the boundary are NCHW like the reference's
 *     torch tensors.
 *   - handles are immutable after the last innfer_net_set_conv(); forward is
 *     re-entrant across streams given distinct workspaces.
 */
#ifndef INNFER_AMD_H
#define INNFER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    INNFER_OK = 0,
    INNFER_ERR_INVALID = -1,     /* bad argument (the reference raises ValueError/AssertionError) */
    INNFER_ERR_HIP = -2,         /* HIP runtime error */
    INNFER_ERR_UNSUPPORTED = -3, /* valid for the reference, not built here (NotImplementedError) */
    INNFER_ERR_NOMEM = -4,
    INNFER_ERR_WORKSPACE = -5    /* workspace too small */
} innfer_status;

typedef enum { INNFER_F16 = 0, INNFER_F32 = 1, INNFER_U8 = 2 /* uint8 HWC image: innfer_net_forward only */ } innfer_dtype;

typedef struct innfer_net* innfer_net_t;

/* ABI revision of this header (major*100 + minor).  101/102: innfer_conv_args grew reflect_pad / dilation / dilation_groups (zero-initialise the struct),
 * innfer_wbc_create takes tf_mode, innfer_net_set_final_act.  103: innfer_net_forward_timed reports algorithmic bytes, innfer_conv_args.pixel_shuffle2, innfer_unet_set_eval,
 * innfer_comm_* / innfer_gather_tiles / innfer_shard_tiles.  104: innfer_rrdbnet_create_ex, innfer_pan_create_ex, innfer_srresnet_create_ex, innfer_resnet_create_ex, innfer_unet_create_ex, innfer_net_set_outm, innfer_guided_filter_ex, innfer_filter2d, innfer_net_set_pair_convs, innfer_inthwc_to_nchw / innfer_nchw_to_inthwc, innfer_linear_resize, INNFER_U8 at the network boundary (innfer_net_set_u8_io), innfer_extract_tiles_u8 / innfer_recompose_u8, innfer_conv_args.stride2_k4 / transposed2x / column7 with innfer_pack_conv4x4s2 / innfer_pack_convt2x / innfer_pack_conv7x1.  105: innfer_net_set_conv_input_map, SRResNet scale 3, PixelShuffle(3) stages (nf 64) and PixelShuffle(2) on nf 32.  106: the fp32-accurate mode -- innfer_net_set_precision, innfer_conv_args.split / *_lo, innfer_pack_conv3x3_split, innfer_nchw_to_slab_split / innfer_slab_split_to_nchw.  107: innfer_net_set_fused_tail, innfer_net_set_upconv_phases.  108: innfer_net_set_residual_lds, innfer_conv_args.res1_from_input, innfer_pan_set_fused_scpa, innfer_unet_set_precision, innfer_pan_set_precision, innfer_ppon_set_precision, innfer_resnet_set_precision, innfer_wbc_set_precision.  109: innfer_conv_args.plane_rows, innfer_pack_conv3x3_rows, innfer_pack_convt2x_rows; innfer_net_set_upconv_phases takes 0 / 1 / 2.  110: innfer_net_set_conv on a network in the fp32 mode builds that conv's split panels (either call order of set_precision / set_conv works); innfer_pack_conv3x3_shuffle2 + innfer_conv_args.plane_rows = 2.  111: innfer_net_set_hr_chain.  112: REMOVED -- innfer_net_set_pair_convs (csrc/conv_pair.hip: the fused conv pairs of a dense block, measured 3 % slower per frame in round 2 and off ever since), innfer_pack_conv3x3_wino / innfer_conv3x3_wino_packed_bytes and the meaning of innfer_conv_args.winograd (now reserved0, must be 0): the row-Winograd experiment of round 3.  113: no new symbol -- innfer_pan_set_precision(p, 1) now selects the split-operand forms for PAN's SCPA trunk / up-stages / attention (innfer_pan_set_fused_scpa(p, 0) keeps the 112 form; 5: A/B of the PA epilogue).  114: innfer_f32conv_args, innfer_f32conv_packed_floats, innfer_pack_f32conv, innfer_f32conv, innfer_f32conv_plan, innfer_f32_norm (the fp32-mode building blocks as single launches, for tests).  115: fit_channels -- innfer_channel_minmax, innfer_extract_tiles_u8_fit, innfer_recompose_u8_fit, innfer_inthwc_to_nchw_fit, innfer_nchw_to_inthwc_fit (gray, gray + alpha and BGRA images through an RGB network).  116: innfer_rrdbnet_create_ex2 (pixel_unshuffle(2 | 4) folded into the first conv: BasicSR / Real-ESRGAN RRDBNet scale 2 and 1), innfer_first_conv_unshuffle (that conv as a single launch, for tests).  117: seamless modes -- innfer_border_index, innfer_pad_inthwc, innfer_extract_tiles_u8_seamless, innfer_extract_tiles_u8_fit_seamless, innfer_recompose_u8_seamless, innfer_recompose_u8_fit_seamless (tileable textures: the chop path reads the image through a border index map and blends only the crop window).  118: -outscale -- innfer_resample_taps, innfer_resample_plan, innfer_resample_workspace_bytes, innfer_resample_inthwc (the result resampled to any final size on the device: an antialiased separable resampler in the Pillow / ATen antialias=True convention).  119: -tta -- innfer_dihedral_index, innfer_extract_tiles_u8_tta, innfer_recompose_u8_tta (the 8-way flip / rotate self-ensemble fused into the uint8 chop path: one gather of the eight orientations' tiles, one blend that averages the eight results before quantisation).  120: the fp16 engine's norm statistics as single launches, for tests -- innfer_conv_args.d_stats_part / stats_part_floats, innfer_conv_stats_records, innfer_norm_combine_parts, innfer_norm_stats, innfer_resnet_post_slab_parts, innfer_unet_post_slab_parts.  121: every remaining form of the conv kernel as a single launch, for tests -- innfer_conv_args.conv1x1 / prefix_lrelu / d_gate_packed / d_gate_bias / in_relu / conv7x7 / out_planar / out_denorm / out_round16 / planar_phases / outm and act 3 / 6, innfer_conv1x1_packed_bytes, innfer_pack_conv1x1, innfer_pack_conv1x1_split, innfer_pack_selfgate, innfer_conv7x7_packed_bytes, innfer_pack_conv7x7, innfer_pack_up2x_phases.  Added under 121 without a new revision (new entry points only, no struct or signature changed): BasicSR's SRVGGNetCompact -- innfer_compact_create, innfer_net_set_conv_slope, innfer_conv3x3_f16_slope (act 8: per-channel slopes), innfer_shuffle_add.  122: the gather GEMM (csrc/gather_gemm.h) as a single launch, for tests -- innfer_gather_gemm_args, innfer_gather_gemm_packed_bytes, innfer_pack_gather_gemm, innfer_gather_gemm, innfer_gather_gemm_plan.  Added under 122 without a new revision (122, additive: new entry points only, no struct or signature changed): the stitched tile path, `-tile N -tile_pad P` -- innfer_tile_plan, innfer_tile_owner, innfer_extract_tiles_rect, innfer_extract_tiles_u8_rect, innfer_stitch_tiles, innfer_stitch_tiles_u8 (csrc/tiles_stitch.hip).  Also added under 122 (additive: new entry points only, no struct or signature changed): innfer_net_set_consumer_grid, innfer_conv3x3_f16_grid (the 64-output trunk convs on a 2 x 4 consumer-wave grid with the residual prefetched; bit-identical results).  Also added under 122 (additive): the launches of PAN's self-attention block one at a time, for tests -- innfer_pan_attention, innfer_pan_attention_workspace_bytes, innfer_pan_maxpool, innfer_pan_fsa_combine.  Also added under 122 (additive): one SCPA block of PAN as a single launch, for tests -- innfer_pan_scpa_blob_bytes, innfer_pack_pan_scpa, innfer_pan_scpa_block, innfer_pan_split_from_nchw, innfer_pan_split_to_nchw.  123: the pass kernels of the pix2pix UNet and the CycleGAN ResNet one launch at a time, for tests (additive) -- innfer_unet_pre / _post / _post_slab / _deep_post / _final, innfer_unet_first_packed_bytes, innfer_pack_unet_first, innfer_unet_first_conv, innfer_resnet_pre / _post / _post_slab / _post_slab_pad / _sum9_tanh / _final.  Added under 123 without a new revision (additive: new entry points only, no struct or signature changed): many images as one tile stream, `-batch B` -- innfer_chop_multi_plan, innfer_extract_tiles_u8_multi, innfer_recompose_u8_multi (csrc/tiles_u8_multi.hip).  Also added under 123 (additive): the colour-fix modes, `-cf_mode wavelet | adain` -- innfer_color_fix_mode_workspace_bytes, innfer_color_fix_mode (csrc/colorfix.hip).  Also added under 123 (additive: new entry points only, no struct or signature changed): the launches every RRDBNet / SRResNet / SRVGGNetCompact forward starts with and the slab passes between its convs one at a time, for tests -- innfer_first_conv, innfer_slab_upsample_nearest, innfer_slab_pixel_shuffle, innfer_slab_input_map.  Also added under 123 (additive: new entry points and new values of existing fields only, no struct or signature changed): SPAN -- innfer_span_create, innfer_first_conv_map (a per-input-channel affine map in front of the first conv), innfer_conv_args.act 9 (SiLU) / 10 (SPAN's gate), innfer_shuffle_add with a NULL base (PixelShuffle alone).  Also added under 123 (additive: new entry points and a new value of an existing field only, no struct or signature changed): RealPLKSR -- innfer_plksr_create, innfer_net_set_group_norm, innfer_conv_args.act 11 (Mish), innfer_plk_conv (the partial large-kernel conv as a single launch), innfer_group_norm_skip / innfer_group_norm_skip_work_bytes (per-sample GroupNorm + skip over a 64-channel slab).  Also added under 123 (additive: new entry points and a new value of an existing field only, no struct or signature changed): SwinIR -- innfer_swinir_create, innfer_net_set_layer_norm, innfer_net_set_attn_bias, innfer_conv_args.act 12 (exact GELU on the 1x1 form), innfer_window_attention (the 8 x 8 window attention as a single launch), innfer_layer_norm (per-pixel LayerNorm over a padded slab).  Also added under 123 (additive: new entry points and a new value of an existing field only, no struct or signature changed; innfer_net_set_layer_norm / innfer_net_set_attn_bias also accept a HAT): HAT -- innfer_hat_create, innfer_net_set_chan_attn, innfer_net_set_conv_scale, innfer_conv_args.act 13 (exact GELU on the plain 3x3 form), innfer_window_attention16 (the 16 x 16 window attention over a 16 x 16 or an overlapping 24 x 24 key window as a single launch), innfer_chan_attn_work_bytes / innfer_chan_attn_excite / innfer_chan_attn_scale_add (the channel attention's launches).  Also added under 123 (additive: new entry points only, no struct or signature changed): the kernels of DAT's blocks as single launches -- innfer_window_attention_rect (rectangular windows in two transposed head branches), innfer_channel_attention_work_bytes / innfer_channel_attention_scores / innfer_channel_attention_apply (attention across channels over a whole sample), innfer_dwconv3x3 (depthwise 3 x 3 with its three epilogues), innfer_chan_attn_excite_gelu, innfer_aim_mix (the two gates that blend the attention and conv branches), innfer_layer_norm_wide (LayerNorm over up to 512 channels) -- and the network on them: innfer_dat_create, innfer_dat_block_floats, innfer_net_set_dat_block (innfer_net_set_layer_norm / innfer_net_set_attn_bias also accept a DAT).  124: the remaining pass kernels of PAN, PPON and the WBC UNet and two passes of the fp32 mode one launch at a time, for tests (additive) -- innfer_pan_pre, innfer_pan_upsample, innfer_pan_final, innfer_pan_slab_pair, innfer_ppon_upsample3, innfer_ppon_axpy, innfer_wbc_pre, innfer_wbc_upadd, innfer_f32_prefix_lrelu, innfer_f32_act_copy.  Added under 124 without a new revision (additive: new entry points only, no struct or signature changed; innfer_net_set_layer_norm / innfer_net_set_attn_bias also accept a DRCT): DRCT -- innfer_drct_create, innfer_window_attention16_wide (the 16 x 16 window attention for heads of 33 .. 128 channels as a single launch), innfer_layer_norm_holed (LayerNorm over a dense slab whose real channels have a hole).  innfer_version() returns the library's; a binding should compare. */
#define INNFER_ABI_VERSION 124
int innfer_version(void);
const char* innfer_last_error(void);

/* ------------------------------------------------------------------ networks
 * Replaces architectures.get_network(opt_net) + nn.Module.forward
 * (architectures/__init__.py:5-40, RRDBNet_arch.py:16-62, SRResNet_arch.py:15-91).
 */

/* RRDBNet (old-arch ESRGAN).  gc is the dense growth (32 in the reference,
 * RRDBNet_arch.py:27); scale in {1,2,3,4,8,16} (3: one nearest-3x stage).  plus != 0 adds the ESRGAN+ paths
 * (x2 += conv1x1(x), x4 += x2: RRDBNet_arch.py:155-160; GaussianNoise is the identity in eval). */
int innfer_rrdbnet_create(innfer_net_t* out, int in_nc, int out_nc, int nf, int nb,
                          int gc, int scale, int plus);

/* The same with the graph-changing constructor arguments of RRDBNet_arch.py:16-48: nr = dense blocks per RRDB (3: parameters
 * `RDB1..RDB3`, else `RDBs.<i>`, RRDBNet_arch.py:73-88); act = `act_type` of every conv block (1 LeakyReLU(0.2), 2 ReLU);
 * pixelshuffle_up != 0 = upsample_mode 'pixelshuffle' (conv nf -> 4 nf, PixelShuffle(2), act: block.py:333-346; scale 3: conv nf -> 9 nf,
 * PixelShuffle(3), nf 64 only) instead of 'upconv'.  innfer_rrdbnet_create(...) = innfer_rrdbnet_create_ex(..., 3, 1, 0).  (104) */
int innfer_rrdbnet_create_ex(innfer_net_t* out, int in_nc, int out_nc, int nf, int nb,
                             int gc, int scale, int plus, int nr, int act, int pixelshuffle_up);

/* The same with BasicSR's RRDBNet input stage (Real-ESRGAN x2plus and every BasicSR model of scale 2 or 1): unshuffle = r in {1, 2, 4} puts pixel_unshuffle(x, r) in
 * front of the first conv, which then has in_nc r^2 input channels (torch order c r^2 + i r + j; `model.0` reports C = in_nc r^2 and takes [nf, in_nc r^2, 3, 3]).  The
 * unshuffled tensor is never written: the conv reads a 3r x 3r window of the image at stride r.  With r > 1 (built for in_nc 3) H x W of innfer_net_workspace_bytes /
 * innfer_net_flops / innfer_net_forward[_timed] is the IMAGE: every layer runs on the LR grid h x w = ceil(H / r) x ceil(W / r), an image whose size is not a multiple
 * of r is reflect-padded bottom / right (pad <= 3, needs H, W >= 4) and the result is [N, out_nc, scale h, scale w] -- the caller crops it to (scale / r) H x (scale / r) W.
 * innfer_net_scale still answers `scale`.  r = 1 is innfer_rrdbnet_create_ex.  (116) */
int innfer_rrdbnet_create_ex2(innfer_net_t* out, int in_nc, int out_nc, int nf, int nb,
                              int gc, int scale, int plus, int nr, int act, int pixelshuffle_up, int unshuffle);
/* The first conv of such a network alone (for tests): conv3x3(pixel_unshuffle(x, unshuffle)) + bias + act (0 none, 1 LeakyReLU(0.2), 2 ReLU) of N images [in_nc 3, H, W]
 * (planar fp16 / fp32, or uint8 HWC BGR with np2tensor's `normalize` and fp16 rounding as in innfer_net_set_u8_io) into a blocked slab of K (32 | 64) channels on the
 * LR grid (group stride in elements; lo != 0: the (hi, lo) pair of the fp32-accurate mode, lo elements apart).  Host fp32 weights [K, 3 r^2, 3, 3]; packs, uploads,
 * launches and waits.  (116) */
int innfer_first_conv_unshuffle(const void* d_in, int in_dtype, int normalize, int fp16_mode, int N, int in_nc, int H, int W, int unshuffle,
                                const float* h_weight_oihw, const float* h_bias, int K, int act, void* d_slab, int64_t group_stride, int64_t lo, void* stream);
/* (123, additive) The plain first conv alone (for tests): conv3x3(x) + bias + act of N images [in_nc 1..8, H, W] -- planar fp16 / fp32, or the uint8 HWC BGR(A) image with
 * np2tensor as the prologue (channel flip as np2tensor's: reversed for in_nc % 3 == 0, channels 0 and 2 swapped for in_nc 4, none otherwise; `normalize`; fp16_mode != 0
 * rounds the converted value to fp16) -- into a blocked slab of K (32 | 64) channels through the launcher the networks call.  act: 0 none, 1 LeakyReLU(0.2), 2 ReLU,
 * 8 f >= 0 ? f : h_slope[c] * f (K host floats; fp16 outputs only).  d_slab2 (may be NULL) receives the same values (the copy the dense blocks concatenate onto).
 * lo / lo2 != 0: the (hi, lo) pair of the fp32-accurate mode, the lo part that many elements behind its hi part -- for both slabs or neither.  Host fp32 weights
 * [K, in_nc, 3, 3], brought to the kernel's [in_nc * 9][K] layout by the code innfer_net_set_conv uses; uploads, launches and waits.
 * Refused, with nothing launched: a NULL pointer, a bad dtype or shape, a group stride below N * H * W * 32, a lo distance that does not clear its hi slab, lo for one
 * slab only, act 8 without slopes (INNFER_ERR_INVALID); K outside {32, 64}, in_nc outside 1 .. 8, another act, act 8 with a split output (INNFER_ERR_UNSUPPORTED). */
int innfer_first_conv(const void* d_in, int in_dtype, int normalize, int fp16_mode, int N, int in_nc, int H, int W,
                      const float* h_weight_oihw, const float* h_bias, int K, int act, const float* h_slope,
                      void* d_slab, int64_t group_stride, int64_t lo, void* d_slab2, int64_t group_stride2, int64_t lo2, void* stream);
/* The same launch with a per-input-channel affine map on the loaded value (SPAN's `(x - mean) * img_range` as the prologue of conv_1): the conv's operand is
 * fp16(h_alpha[c] * v + h_shift[c]) -- one fp32 fma, one rounding -- of the value v innfer_first_conv would multiply (the fp16 tensor value; np2tensor of the uint8 image:
 * with fp16_mode 0 and h_alpha = 255 that is code - 255 mean in one rounding).  The zero padding stays zero AFTER the map (a mean folded into the bias would be wrong on
 * the border ring).  h_alpha / h_shift: in_nc host floats, NULL = 1 / 0; both NULL: no map, innfer_first_conv's launch and bits.  fp16 or uint8 input, act 0 .. 2, one
 * fp16 slab; a float32 input with a map is INNFER_ERR_UNSUPPORTED. */
int innfer_first_conv_map(const void* d_in, int in_dtype, int normalize, int fp16_mode, int N, int in_nc, int H, int W,
                          const float* h_weight_oihw, const float* h_bias, int K, int act, const float* h_alpha, const float* h_shift,
                          void* d_slab, int64_t group_stride, void* stream);
/* (123, additive) The slab passes innfer_net_forward runs between its convs, as single launches (for tests); each checks its arguments and calls the launcher the network
 * calls.  Slabs are blocked-NHWC fp16, 32-channel groups `*_gs` elements apart; lo != 0 repeats the launch on the lo twins `lo` elements behind source and destination
 * (the fp32-accurate mode).  The first two do not wait for the stream.
 * innfer_slab_upsample_nearest: `groups` groups on the H x W grid -> nearest-neighbour `factor` x (source pixel = destination / factor) on factor H x factor W.
 * innfer_slab_pixel_shuffle: nn.PixelShuffle(r): nf r^2 channels on H x W -> nf channels on r H x r W, out[n, y r + i, x r + j, c] = in[n, y, x, c r^2 + i r + j].
 * innfer_slab_input_map: the 'NAC' input map dst = act(h_alpha[c] * src + h_shift[c]) (NULL: 1 / 0; act 0 none, 1 LeakyReLU(0.2), 2 ReLU) over every element of the
 *   ceil(C / 32) groups of gs elements each (gs % 32 == 0; gs is group size AND stride, as in the network); channels beyond C are written as zeros.  lo != 0: the pair
 *   form -- x = hi + lo 2^-11 mapped in fp32 and split again.  Uploads the map, launches and waits.
 * Refused, with nothing launched (INNFER_ERR_INVALID): a NULL pointer, a shape or factor below 1, a group stride below the tensor (N H W 32 / N H W factor^2 32),
 * nf not a positive multiple of 8, groups < 1, C < 1, act outside 0 .. 2, gs not a multiple of 32, a lo distance that does not clear the hi slabs. */
int innfer_slab_upsample_nearest(const void* d_src, int64_t src_gs, void* d_dst, int64_t dst_gs, int groups, int N, int H, int W, int factor, int64_t lo, void* stream);
int innfer_slab_pixel_shuffle(const void* d_src, int64_t src_gs, void* d_dst, int64_t dst_gs, int nf, int N, int H, int W, int r, int64_t lo, void* stream);
int innfer_slab_input_map(const void* d_src, void* d_dst, int64_t gs, int64_t lo, int C, const float* h_alpha, const float* h_shift, int act, void* stream);

/* SRResNet / SRGAN with the reference defaults (norm none, ReLU, CNA,
 * pixelshuffle, res_scale 1: utils/defaults.py:53-67). */
int innfer_srresnet_create(innfer_net_t* out, int in_nc, int out_nc, int nf, int nb, int scale);
/* The same with the constructor arguments that keep the graph on the built kernels (SRResNet_arch.py:16-46,69-91): act = `act_type` (1 LeakyReLU(0.2),
 * 2 ReLU), res_scale (x + res * res_scale), upconv_up != 0 = upsample_mode 'upconv' (Upsample, conv, act) instead of 'pixelshuffle';
 * scale in {1,2,3,4,8} (3: one factor-3 stage; PixelShuffle(3) needs nf 64).  (104, 105) */
int innfer_srresnet_create_ex(innfer_net_t* out, int in_nc, int out_nc, int nf, int nb, int scale, int act, float res_scale, int upconv_up);
/* mode 'NAC' conv blocks (block.py:246-254: norm -> act -> conv; SRResNet's own default, SRResNet_arch.py:16-27): conv `idx` reads
 * act(alpha[c] * x + shift[c]) instead of x -- the eval-mode BatchNorm2d of its input channels as a per-channel map (NULL alpha / shift: 1 / 0) and
 * act (0 none, 1 LeakyReLU(0.2), 2 ReLU), one elementwise launch in front of the conv.  Built for the first conv of an SRResNet block and LR_conv
 * (the norm in front of a block's second conv follows the first conv and is folded into its weights by the host).  All of NULL, NULL, 0 removes the map.  (105) */
int innfer_net_set_conv_input_map(innfer_net_t net, int idx, const float* h_alpha, const float* h_shift, int act);

/* BasicSR's SRVGGNetCompact (realesr-animevideov3, realesr-general-x4v3 and the community "compact" checkpoints; the reference has no such architecture):
 *   body.0 = Conv2d(in_nc, nf, 3, 1, 1) + activation; body.2i = Conv2d(nf, nf, 3, 1, 1) + activation for i = 1 .. num_conv; body.<2 num_conv + 2> =
 *   Conv2d(nf, out_nc scale^2, 3, 1, 1); out = PixelShuffle(scale)(body(x)) + nearest_upsample(x, scale)
 * on the engine of innfer_net_*: innfer_net_conv_info reports the convs under the keys `body.<i>` (the last one with K = out_nc scale^2), innfer_net_set_conv loads
 * them, innfer_net_set_conv_slope the activation behind each conv but the last, innfer_net_forward[_timed] / innfer_net_workspace_bytes / innfer_net_flops /
 * innfer_net_set_u8_io work as for the other networks (uint8 images at either end included; band rows and the RRDBNet scheduling knobs do not apply).
 * nf in {32, 64} (fewer features: zero-pad weights, bias and slopes), in_nc == out_nc in 1 .. 4, num_conv >= 0, scale in 1 .. 4; anything else is
 * INNFER_ERR_UNSUPPORTED.  fp16 mode only: fp16 or uint8 input, fp16 / fp32 / uint8 output; innfer_net_set_precision(net, 1) and fp32 input are INNFER_ERR_UNSUPPORTED.
 * Every layer is ONE launch (the activation is the conv's epilogue, act 8); the workspace holds two nf-channel slabs and the last conv's 32- / 64-channel slab.
 * Arithmetic of the tail, per output value: fp16(float(fp16 conv value) + float(fp16 input value)) -- torch's half `out += base` -- then float() or tensor2np. */
int innfer_compact_create(innfer_net_t* out, int in_nc, int out_nc, int nf, int num_conv, int scale);

/* SPAN, the Swift Parameter-free Attention Network (the community's "fast" 2x / 4x models; the reference has no such architecture).  With Conv3XC collapsed to ONE
 * 3x3 zero-pad-1 conv (its eval form; the caller folds sk + conv.2 . conv.1 . conv.0 into one weight and bias):
 *   SPAB(x): out1 = c1_r(x); out2 = c2_r(SiLU(out1)); out3 = c3_r(SiLU(out2)); out = (out3 + x) * (sigmoid(out3) - 0.5); returns (out, out1)
 *   x = (x - mean) * img_range when norm (per channel; the mean is NOT added back); f0 = conv_1(x); b1 .. b5 = block_1 .. block_5; (b6, b5_2) = block_6(b5);
 *   out = PixelShuffle(scale)(upsampler.0(conv_cat(cat[f0, conv_2(b6), b1, b5_2])))
 * on the engine of innfer_net_*: innfer_net_conv_info reports the convs under the keys conv_1, block_<i>.c<j>_r (i = 1 .. 6, j = 1 .. 3), conv_2, conv_cat ([nf, 4 nf, 1, 1])
 * and upsampler.0 (K = out_nc scale^2); innfer_net_set_conv loads them; innfer_net_forward[_timed] / innfer_net_workspace_bytes / innfer_net_flops / innfer_net_set_u8_io
 * work as for SRVGGNetCompact.  nf in {32, 64} (fewer features: zero-pad the weights -- exact: SiLU(0) = 0 and the gate of (0, 0) is 0), in_nc == out_nc in 1 .. 4,
 * scale 1 .. 4; anything else is INNFER_ERR_UNSUPPORTED.  fp16 mode only, as SRVGGNetCompact.  mean: in_nc host floats (read only when norm).
 * A forward is 24 launches: conv_1 (the input map is its prologue: operand fp16(img_range * v - mean[c] * img_range), zero padding AFTER the map), three per SPAB
 * (act 9, act 9, act 10 with res1 = the block's input), one SiLU pass (block_6's out1 goes to the concat raw), conv_2, conv_cat (1x1 over the concat slab: f0, b1, b5_2 and
 * conv_2's result were written into it at their channel offsets), upsampler.0, and the PixelShuffle store (innfer_shuffle_add without a base). */
int innfer_span_create(innfer_net_t* out, int in_nc, int out_nc, int nf, int scale, int norm, float img_range, const float* h_mean);

/* RealPLKSR (the community's large-kernel models; the reference has no such architecture):
 *   DCCM(dim):       Sequential(Conv2d(dim, 2 dim, 3, 1, 1), Mish(), Conv2d(2 dim, dim, 3, 1, 1))
 *   PLKConv2d(p, k): conv = Conv2d(p, p, k, 1, k // 2);  forward: x[:, :p] = conv(x[:, :p])  (the other channels pass through)
 *   EA(dim):         f = Sequential(Conv2d(dim, dim, 3, 1, 1), Sigmoid());  forward: x * f(x)
 *   PLKBlock:        channel_mixer = DCCM(dim); lk = PLKConv2d(int(dim * split_ratio), k); attn = EA(dim) or Identity (use_ea False);
 *                    refine = Conv2d(dim, dim, 1); norm = GroupNorm(norm_groups, dim)       (eps 1e-5, biased variance, per sample over (dim / groups) x H x W)
 *                    forward: norm(refine(attn(lk(channel_mixer(x))))) + x
 *   RealPLKSR(in_ch 3, out_ch 3, dim 64, n_blocks 28, upscaling_factor 4, kernel_size 17, split_ratio 0.25, use_ea True, norm_groups 4):
 *                    feats = Sequential(Conv2d(in_ch, dim, 3, 1, 1), n_blocks x PLKBlock, Dropout2d (no parameters), Conv2d(dim, out_ch s^2, 3, 1, 1))
 *                    forward: PixelShuffle(s)(feats(x) + repeat_interleave(x, s^2, dim=1))
 *   Mish(f) = f * tanh(softplus(f)) = f * (n^2 + 2 n) / (n^2 + 2 n + 2),  n = exp(f)
 * on the engine of innfer_net_*: innfer_net_conv_info reports the convs under the keys feats.0, then per block i = 1 .. n_blocks feats.<i>.channel_mixer.0a and
 * .channel_mixer.0b ([64, 64, 3, 3] each: output channels 0 .. 63 and 64 .. 127 of channel_mixer.0, one launch each), .channel_mixer.2 ([64, 128, 3, 3]), .lk.conv
 * ([16, 16, k, k]), .attn.f.0 (use_ea only), .refine ([64, 64, 1, 1]), and feats.<n_blocks + 2> (K = out_ch s^2); innfer_net_set_conv loads them,
 * innfer_net_set_group_norm the GroupNorm behind every refine; innfer_net_forward[_timed] / innfer_net_workspace_bytes / innfer_net_flops / innfer_net_set_u8_io work as
 * for SRVGGNetCompact.  dim 64 (split_ratio 0.25: the large kernel on 16 channels), kernel_size odd 3 .. 17, in_ch == out_ch in 1 .. 4, scale 1 .. 4, norm_groups in
 * {1, 2, 4, 8}; anything else is INNFER_ERR_UNSUPPORTED.  fp16 mode only.
 * A forward is 9 n_blocks + 3 launches (8 per block without EA): feats.0; per block two Mish launches (act 11), channel_mixer.2, the large-kernel conv, the EA gate (act 5
 * with res1 = its own input), refine, the GroupNorm statistics, their merge, and t = fp16(alpha[n, c] u + shift[n, c] + x); the last conv; innfer_shuffle_add with the
 * input as base (PixelShuffle(s)(y + repeat_interleave(x, s^2)) = PixelShuffle(s)(y) + nearest_upsample(x, s)).
 * GroupNorm statistics are PER SAMPLE and those of whatever the network is given: a tiling front end (the 200-px chop) normalises per tile. */
int innfer_plksr_create(innfer_net_t* out, int in_nc, int out_nc, int dim, int n_blocks, int scale, int kernel_size, int use_ea, int norm_groups);
/* gamma / beta (64 host floats each, NULL = 1 / 0) of the GroupNorm behind conv `idx` (a RealPLKSR's refine convs; other convs refuse).  Load time, synchronous. */
int innfer_net_set_group_norm(innfer_net_t net, int idx, const float* h_gamma, const float* h_beta);
/* (123, additive) SwinIR (Liang et al. 2021, the super-resolution forms; the reference has no such architecture), KAIR / BasicSR swinir_arch.py with window_size 8,
 * patch_size 1, qkv_bias, patch_norm, no absolute position embedding, img_range 1:
 *   forward(x):   reflect-pad right / bottom to multiples of 8; f = conv_first(x - mean); f = conv_after_body(norm(RSTBs(patch_embed.norm(f)))) + f; tail; + mean; crop
 *   RSTB:         t = conv(blocks(t)) + t       (conv: '1conv' Conv2d(C, C, 3, 1, 1); '3conv' Conv2d(C, C/4, 3), LeakyReLU(0.2), Conv2d(C/4, C/4, 1), LeakyReLU(0.2), Conv2d(C/4, C, 3))
 *   block j:      t = t + proj(attn(norm1(t))); t = t + fc2(GELU(fc1(norm2(t))))    (exact GELU; LayerNorm(C) per token, eps 1e-5; shift 4 for odd j)
 *   attn:         8 x 8 windows of roll(u, (-shift, -shift)); per head softmax((q d^-0.5) k^T + B_h + M) v; M = -100 between tokens of different regions (shift only)
 *   tails:        pixelshuffle (conv_before_upsample + LeakyReLU(0.01), conv + PixelShuffle stages, conv_last), pixelshuffledirect (upsample.0 + PixelShuffle(s)),
 *                 nearest+conv (conv_before_upsample + LeakyReLU(0.01), lrelu(conv_up1(nearest 2x)), [conv_up2,] conv_last(lrelu(conv_hr)))
 * on the engine of innfer_net_*.  The token slab holds C_pad = 64 ceil(C / 64) channels (pad channels zero), the MLP's hidden slab hidden_pad likewise; q, k and v of head h
 * each own one 32-channel group (d = C / nH real channels, then zeros).  Every Linear and every conv from or to C_pad channels is a chain of 64-output launches:
 * innfer_net_conv_info reports them under `<state-dict key>#<p>` ([64, C_in_pad, k, k]: rows 64 p .. 64 p + 63 of the weight re-laid-out by the caller -- input channels
 * padded with zeros; attn.qkv rows in the order (q | k | v) x head x 32 with d^-0.5 inside the q rows and their bias; attn.proj columns head x 32), the tail's convs under
 * their own keys (conv_last / pixelshuffledirect's upsample.0 with + mean inside their bias).  innfer_net_set_conv loads them, innfer_net_set_layer_norm the LayerNorms,
 * innfer_net_set_attn_bias every block's dense bias table.  upsampler: 0 pixelshuffle (scale 2, 3, 4), 1 pixelshuffledirect (2, 3, 4), 2 nearest+conv (2, 4).
 * embed_dim <= 256, num_heads <= 8, head_dim <= 32, mlp_hidden <= 1024, in_nc == out_nc in 1 .. 4; anything else is INNFER_ERR_UNSUPPORTED.  fp16 mode only.
 * innfer_net_forward takes H x W (each side larger than its pad 8 ceil(n / 8) - n) and writes scale H x scale W: pad and crop are launches of the engine.
 * Launches of a forward, with Hp x Wp the padded size, B the number of blocks, R the residual groups, S1 = C_pad / 64, SQ = ceil(3 nH / 2), SH = hidden_pad / 64,
 * SR = S1 ('1conv') or 2 ceil(C / 256) + S1 ('3conv'), T = 2 (pixelshuffledirect), 2 + log2(scale) (pixelshuffle 2 / 4), 4 (pixelshuffle 3), 3 + log2(scale) (nearest+conv):
 *   S1 + 2 + B (3 + SQ + 2 S1 + SH) + (R + 1) SR + T + 2 [H x W is not Hp x Wp]. */
int innfer_swinir_create(innfer_net_t* out, int in_nc, int out_nc, int embed_dim, const int* depths, int n_layers, int num_heads, int mlp_hidden, int upsampler,
                         int scale, int conv3, const float* h_mean);
/* (123, additive) gamma / beta (C host floats each) of LayerNorm `idx` of a SwinIR: 0 patch_embed.norm; 1 + 2 b and 2 + 2 b norm1 and norm2 of block b (counted through
 * the residual groups); 2 + 2 B norm.  Load time, synchronous. */
int innfer_net_set_layer_norm(innfer_net_t net, int idx, const float* h_gamma, const float* h_beta);
/* (123, additive) The relative position bias of block `blk` of a SwinIR as the dense table the attention reads: [num_heads][64 query][64 key] host floats,
 * B[h][i][j] = relative_position_bias_table[(ri - rj + 7) * 15 + (ci - cj + 7)][h] for tokens i = 8 ri + ci, j = 8 rj + cj.  Load time, synchronous. */
int innfer_net_set_attn_bias(innfer_net_t net, int blk, const float* h_bias);
/* (123, additive) The window attention as a single launch (for tests; csrc/win_attn.hip).  d_qkv: fp16 slab of 3 num_heads 32-channel groups of N x Hp x Wp pixels
 * (q | k | v, head h of each in its own group: head_dim real channels, then zeros; q already scaled), d_out: num_heads groups (channels >= head_dim written as zeros);
 * *_gs: group strides in elements; h_bias as innfer_net_set_attn_bias; Hp, Wp multiples of 8; shift 0 or 4 (the windows of the rolled frame, -100 between regions).
 * fp32 scores, maximum, exponentials and sums; P rounded to fp16 in front of P v; fp32 accumulation; one rounding of o / sum.  Uploads the table, launches, waits. */
int innfer_window_attention(const void* d_qkv, int64_t qkv_gs, void* d_out, int64_t out_gs, const float* h_bias, int N, int Hp, int Wp, int num_heads, int head_dim,
                            int shift, void* stream);
/* (123, additive) nn.LayerNorm(C) per pixel over slabs of c_pad channels (for tests; csrc/layer_norm.hip): d_out = fp16(fma((x - mean) rstd, gamma[c], beta[c])), mean and
 * biased variance in fp32 over the C real channels; channels C .. c_pad - 1 are ignored on input and written as zeros.  d_out may be d_in.  c_pad % 64 == 0, <= 256.
 * Uploads gamma / beta (C host floats each), launches, waits. */
int innfer_layer_norm(const void* d_in, int64_t in_gs, void* d_out, int64_t out_gs, int64_t npix, int C, int c_pad, const float* h_gamma, const float* h_beta, float eps,
                      void* stream);
/* (123, additive) Swin2SR (Conde et al. 2022, "Swin2SR: SwinV2 Transformer for Compressed Image Super-Resolution and Restoration"; the reference has no such
 * architecture), the published network_swin2sr.py with window_size 8, patch_size 1, qkv_bias, patch_norm, no absolute position embedding, img_range 1.  SwinIR's skeleton
 * (innfer_swinir_create: pad, x - mean, conv_first, patch_embed.norm, RSTB = conv(blocks(t)) + t, norm, conv_after_body + f, the tails, + mean, crop, shift 4 for odd j,
 * the -100 mask between the region labels of the rolled frame) around another block:
 *   block j:   t = t + norm1(proj(attn(t)));  t = t + norm2(fc2(GELU(fc1(t))))      (the LayerNorm BEHIND each branch; attn reads t itself; exact GELU; eps 1e-5)
 *   attn(t):   8 x 8 windows of roll(t, (-shift, -shift)); qkv = Linear(C, 3 C, no bias)(t') + cat(q_bias, zeros(C), v_bias) -- k has no bias; per head h
 *              S = (q^ k^^T) tau_h + B_h + M,  q^ = q / max(||q||_2, 1e-12) over the d channels of the head, k^ likewise;  tau_h = exp(min(logit_scale[h], ln 100));
 *              P = softmax(S); o = P v; heads concatenated, proj, windows back, roll back.  There is no d^-0.5.
 *   B_h:       T[225][nH] = cpb_mlp(coords), cpb_mlp = Linear(2, hidden, bias) -> ReLU -> Linear(hidden, nH, no bias);
 *              coords[15 a + b] = (g(a - 7), g(b - 7)), g(c) = sign(c) log2(|8 c / 7| + 1) / 3  (a checkpoint's relative_coords_table [1, 15, 15, 2], when stored, is used
 *              in its place);  B_h[i][j] = 16 sigmoid(T[(ri - rj + 7) 15 + (ci - cj + 7)][h]) for tokens i = 8 ri + ci, j = 8 rj + cj
 * on the engine of innfer_net_*, laid out as innfer_swinir_create's (same arguments, limits, conv slots `<state-dict key>#<p>`, LayerNorm numbering, workspace, fp16 mode
 * only).  The caller re-lays-out as for SwinIR EXCEPT that attn.qkv's q rows carry no scale and its bias is cat(q_bias, 0, v_bias) under the same permutation; it builds
 * B_h (innfer_net_set_attn_bias) and tau (innfer_net_set_attn_scale) at load.  Per block: qkv from t (SQ launches), the cosine attention (1), proj -> u (S1),
 * t = t + LN(u) (1), fc1 with GELU from t (SH), fc2 -> u (S1), t = t + LN(u) (1): 3 + SQ + 2 S1 + SH, so a forward has SwinIR's launch count:
 *   S1 + 2 + B (3 + SQ + 2 S1 + SH) + (R + 1) SR + T + 2 [H x W is not Hp x Wp]. */
int innfer_swin2sr_create(innfer_net_t* out, int in_nc, int out_nc, int embed_dim, const int* depths, int n_layers, int num_heads, int mlp_hidden, int upsampler,
                          int scale, int conv3, const float* h_mean);
/* (123, additive) tau of block `blk` of a Swin2SR: exp(min(logit_scale, ln 100)) per head, num_heads host floats (finite, > 0).  Load time, synchronous. */
int innfer_net_set_attn_scale(innfer_net_t net, int blk, const float* h_tau);
/* (123, additive) The cosine window attention as a single launch (for tests; csrc/win_attn.hip, the COS form).  Slabs, sizes and shift as innfer_window_attention's, q and k
 * unscaled; h_tau: num_heads host floats.  The raw product runs on the fp16 operands as stored; then in fp32 S = raw (rq_i tau_h) rk_j + B_h[i][j] with
 * r = 1 / max(sqrtf(sum of squares), 1e-12) (an all-zero row: scores = the bias); mask, softmax, P v as innfer_window_attention.  Uploads, launches, waits. */
int innfer_window_attention_cos(const void* d_qkv, int64_t qkv_gs, void* d_out, int64_t out_gs, const float* h_bias, const float* h_tau, int N, int Hp, int Wp,
                                int num_heads, int head_dim, int shift, void* stream);
/* (123, additive) LayerNorm + residual per pixel (for tests; csrc/layer_norm.hip, the ADD form): d_out = fp16(res + fma((x - mean) rstd, gamma[c], beta[c])), statistics as
 * innfer_layer_norm's, ONE fp16 rounding; channels C .. c_pad - 1 written as zeros.  d_out may be d_res or d_in.  Uploads gamma / beta, launches, waits. */
int innfer_layer_norm_add(const void* d_in, int64_t in_gs, const void* d_res, int64_t res_gs, void* d_out, int64_t out_gs, int64_t npix, int C, int c_pad,
                          const float* h_gamma, const float* h_beta, float eps, void* stream);
/* (123, additive) HAT (Chen et al. 2023, "Activating More Pixels in Image Super-Resolution Transformer"; the reference has no such architecture) on SwinIR's skeleton, with
 * C = embed_dim, nH heads of d = C / nH, window ws = 16, overlapping window ows = 24, patch_size 1, qkv_bias, patch_norm, no absolute position embedding, img_range 1, '1conv':
 *   forward(x):  reflect-pad right / bottom to multiples of 16; f = conv_first(x - mean); f = conv_after_body(norm(RHAGs(patch_embed.norm(f)))) + f;
 *                conv_before_upsample + LeakyReLU(0.01); upsample (pixelshuffle); conv_last; + mean; crop
 *   RHAG i:      t = conv(OCAB(HAB_{n-1}(... HAB_0(t)))) + t
 *   HAB j:       u = norm1(t);  t = t + proj(attn(u)) + conv_scale * CAB(u);  t = t + fc2(GELU(fc1(norm2(t))))
 *                attn: SwinIR's window attention with ws 16, shift 8 for odd j; -100 between region labels of the rolled frame (rows / columns split at Hp - 16 and Hp - 8)
 *   CAB(u):      z = conv3x3(C -> C / compress_ratio) -> exact GELU -> conv3x3(C / compress_ratio -> C);  y = sigmoid(W2 relu(W1 mean_pixels(z) + b1) + b2);  CAB = z * y[channel]
 *                -- the mean runs over the whole padded Hp x Wp grid of ONE sample
 *   OCAB:        u = norm1(t); q, k, v = qkv(u); queries: the 16 x 16 windows; keys / values of window (wy, wx): the 24 x 24 pixels from (16 wy - 4, 16 wx - 4), a position
 *                outside the padded grid has k = v = 0 (its score is the bias alone and it takes part in the softmax); softmax(q d^-0.5 k^T + B) v; no shift, no mask;
 *                t = t + proj(.);  t = t + fc2(GELU(fc1(norm2(t))))
 * on the engine of innfer_net_*, laid out as innfer_swinir_create's: conv slots `<state-dict key>#<p>` in forward order -- conv_first; per HAB conv_block.cab.0 (ONE slice:
 * [64, C_pad, 3, 3], C / compress_ratio real rows), conv_block.cab.2 ([64, 64, 3, 3] slices), attn.qkv, attn.proj, mlp.fc1, mlp.fc2; per group overlap_attn.qkv, .proj,
 * .mlp.fc1, .mlp.fc2 and the group's conv; conv_after_body; the pixelshuffle tail.  LayerNorms (innfer_net_set_layer_norm) and bias tables (innfer_net_set_attn_bias) are
 * numbered in forward order: 0 patch_embed.norm; per group (norm1, norm2) of every HAB, then (norm1, norm2) of the OCAB; the last one norm -- tables: per group every HAB's
 * [nH][256][256], then the OCAB's [nH][256][576].  compress_ch = C / compress_ratio and squeeze_ch = C / squeeze_factor, 1 .. 64 each; scale 2, 3, 4; the other limits as SwinIR's.
 * innfer_net_forward takes H x W (each side larger than its pad to 16) and writes scale H x scale W.  Launches of a forward, with B HABs, R groups, S1 = C_pad / 64,
 * SQ = ceil(3 nH / 2), SH = hidden_pad / 64, T = 2 + log2(scale) (4 for scale 3):
 *   S1 + 2 + B (7 + SQ + 3 S1 + SH) + R (3 + SQ + 2 S1 + SH) + (R + 1) S1 + T + 2 [H x W is not Hp x Wp]. */
int innfer_hat_create(innfer_net_t* out, int in_nc, int out_nc, int embed_dim, const int* depths, int n_layers, int num_heads, int mlp_hidden, int compress_ch, int squeeze_ch,
                      int scale, const float* h_mean);
/* (123, additive) The channel attention of HAB `blk` of a HAT (counted through the groups): conv_block.cab.3.attention.1 as W1 [squeeze_ch][C], b1 [squeeze_ch] and
 * conv_block.cab.3.attention.3 as W2 [C][squeeze_ch], b2 [C], host floats, kept and applied in fp32.  Load time, synchronous. */
int innfer_net_set_chan_attn(innfer_net_t net, int blk, const float* h_w1, const float* h_b1, const float* h_w2, const float* h_b2);
/* (123, additive) conv_scale of a HAT: a constructor argument of the published code that no state dict carries; 0.01 until set. */
int innfer_net_set_conv_scale(innfer_net_t net, float conv_scale);
/* (123, additive) The 16 x 16 window attention as a single launch (for tests; csrc/win_attn16.hip).  Slabs as innfer_window_attention's; Hp, Wp multiples of 16.
 * key_window 16: the window's own 256 tokens, shift 0 or 8 (the windows of the rolled frame, -100 between regions), h_bias [num_heads][256][256].  key_window 24: the
 * 24 x 24 pixels from (16 wy - 4, 16 wx - 4), zeros in k and v outside the grid (such a key still takes part in the softmax), shift 0, h_bias [num_heads][256][576].
 * fp32 scores, running maximum and sum over blocks of 64 keys; P rounded to fp16 in front of P v; fp32 accumulation; one rounding of o / sum.  Uploads the table, launches, waits. */
int innfer_window_attention16(const void* d_qkv, int64_t qkv_gs, void* d_out, int64_t out_gs, const float* h_bias, int N, int Hp, int Wp, int num_heads, int head_dim,
                              int shift, int key_window, void* stream);
/* (123, additive) HAT's channel attention as single launches (for tests; csrc/chan_attn.hip), per sample over slabs of c_pad channels (64, 128, 192, 256) of N x HW pixels.
 * innfer_chan_attn_excite: the per-(sample, channel) sums of d_z (fp32, a fixed merge order: bit-identical on a repeat) and d_y[n][c] = sigmoid(W2 relu(W1 sums / HW + b1) + b2)
 * in fp32 (N x c_pad floats; 0 for c >= C); d_sums (may be NULL) receives the sums, N x c_pad floats; d_work: innfer_chan_attn_work_bytes(N, HW, c_pad) bytes.
 * innfer_chan_attn_scale_add: d_t = fp16(float(d_t) + conv_scale * d_y[n][c] * float(d_z)), one fp16 rounding, in place.  Nothing crosses samples.  Launch, wait. */
size_t innfer_chan_attn_work_bytes(int N, int64_t HW, int c_pad);
int innfer_chan_attn_excite(const void* d_z, int64_t z_gs, int N, int64_t HW, int C, int c_pad, int hidden, const float* h_w1, const float* h_b1, const float* h_w2,
                            const float* h_b2, void* d_y, void* d_sums, void* d_work, size_t work_bytes, void* stream);
int innfer_chan_attn_scale_add(void* d_t, int64_t t_gs, const void* d_z, int64_t z_gs, const void* d_y, float conv_scale, int N, int64_t HW, int c_pad, void* stream);
/* (123, additive) The kernels of a DAT block (Chen et al. 2023, "Dual Aggregation Transformer for Image Super-Resolution"; the reference has no such architecture) as single
 * launches, for tests.  All slabs hold N x H x W (or N x HW) pixels WITHOUT padding; *_gs are group strides in elements; every entry uploads its host parameters, launches, waits.
 *
 * innfer_window_attention_rect (csrc/win_attn_rect.hip): attention over rectangular windows in two head branches of transposed shape.  d_qkv / d_out as
 * innfer_window_attention's (3 num_heads / num_heads groups of 32 channels; q already scaled).  split [s0, s1] is [8, 32] or [8, 16], T = s0 s1; heads 0 .. nH / 2 - 1 use
 * windows of s0 rows x s1 columns and shift (s0 / 2, s1 / 2), heads nH / 2 .. nH - 1 windows of s1 x s0 and shift (s1 / 2, s0 / 2) (num_heads even).  The windows tile the
 * frame Hp x Wp = H, W rounded up to multiples of s1 -- rolled by minus the shift when shifted != 0; a token whose stored pixel lies outside H x W has q = k = v = 0: it is
 * never read and never stored, as a key its score is bias + mask and it takes part in the softmax.  Shifted: -100 between tokens whose labels 3 a(r) + b(c) in the rolled
 * frame differ (a = 0 below Hp - wh, 1 below Hp - shy, else 2; b likewise with Wp, ww, shx, for the head's own window wh x ww and shift).  h_bias: [num_heads][T][T] host
 * floats, query-major, tokens row-major inside the head's own window shape.  Arithmetic as innfer_window_attention16's: fp32 scores, running maximum and sum over blocks of 64
 * keys; P rounded to fp16 in front of P v; fp32 accumulation; one rounding of o / sum; channels >= head_dim written as zeros. */
int innfer_window_attention_rect(const void* d_qkv, int64_t qkv_gs, void* d_out, int64_t out_gs, const float* h_bias, int N, int H, int W, int num_heads, int head_dim,
                                 int s0, int s1, int shifted, void* stream);
/* innfer_channel_attention_scores / _apply (csrc/chan_self_attn.hip): attention across the head_dim channels of a head over all HW pixels of one sample, on the same qkv slab
 * (q and k unscaled; whatever their channels >= head_dim hold is ignored).  scores: G[x][y] = sum_n q[n][x] k[n][y], sq[x] = sum_n q[n][x]^2, sk[y] likewise -- fp32 fma
 * chains over segments of 1024 pixels in order, the segments merged in index order (bit-identical on a repeat) -- then
 * A[x][y] = softmax_y((G[x][y] (rq[x] rk[y])) temperature[h]), r = 1 / max(sqrtf(s), 1e-12), in fp32.  d_A: [N][num_heads][32][32] floats, rows and columns >= head_dim zeros;
 * d_gram (may be NULL): [N][num_heads][1088] floats, the merged G [32][32], sq [32], sk [32]; d_work: innfer_channel_attention_work_bytes bytes; d_A and d_work 16-byte
 * aligned; h_temperature: num_heads host floats.  apply: d_out[n][x] = fp16(sum_{y < head_dim} A[x][y] v[n][y]), an fp32 fma chain over y in order, one rounding, into
 * num_heads groups whose channels >= head_dim are written as zeros.  Nothing crosses samples. */
size_t innfer_channel_attention_work_bytes(int N, int64_t HW, int num_heads);
int innfer_channel_attention_scores(const void* d_qkv, int64_t qkv_gs, int N, int64_t HW, int num_heads, int head_dim, const float* h_temperature, void* d_A, void* d_gram,
                                    void* d_work, size_t work_bytes, void* stream);
int innfer_channel_attention_apply(const void* d_qkv, int64_t qkv_gs, void* d_out, int64_t out_gs, const void* d_A, int N, int64_t HW, int num_heads, int head_dim, void* stream);
/* innfer_dwconv3x3 (csrc/dwconv.hip): depthwise 3 x 3 conv, zero padding, over slabs of c_pad channels (a multiple of 32, <= 512).  h_taps [C][3][3], h_bias [C] host floats
 * (a BatchNorm behind the conv is folded into both by the caller).  Per value f = bias, then f = fma(tap, x, f) over the nine taps row-major in fp32; epilogue 0: f; 1: the
 * exact GELU of the conv kernels' act 12; 2: f * d_mul (a second slab of the same shape; NULL otherwise); ONE fp16 rounding.  Channels C .. c_pad - 1 are written as zeros.
 * d_out must not be d_in. */
int innfer_dwconv3x3(const void* d_in, int64_t in_gs, const void* d_mul, int64_t mul_gs, void* d_out, int64_t out_gs, int N, int H, int W, int C, int c_pad,
                     const float* h_taps, const float* h_bias, int epilogue, void* stream);
/* innfer_chan_attn_excite_gelu: innfer_chan_attn_excite with the exact GELU, f (1 + erff(f / sqrt 2)) / 2, on the hidden units in place of the ReLU (DAT's
 * channel_interaction with its BatchNorm folded into W1 / b1).  Arguments, sums, merge order and limits as innfer_chan_attn_excite's. */
int innfer_chan_attn_excite_gelu(const void* d_z, int64_t z_gs, int N, int64_t HW, int C, int c_pad, int hidden, const float* h_w1, const float* h_b1, const float* h_w2,
                                 const float* h_b2, void* d_y, void* d_sums, void* d_work, size_t work_bytes, void* stream);
/* innfer_aim_mix (csrc/aim_mix.hip): d_out = fp16(fma(X, gate[n][c], Y * s[pixel])), s = sigmoid(w2 . GELU(W1 X[pixel] + b1) + b2) -- DAT's spatial_interaction (1x1 conv
 * C -> hidden with its BatchNorm folded in, exact GELU, 1x1 conv hidden -> 1) and the blend of the two branches in ONE launch.  d_x, d_y, d_out: slabs of c_pad channels (64,
 * 128, 192, 256); d_gate: N x c_pad device floats (innfer_chan_attn_excite_gelu's d_y); h_w1 [hidden][C], h_b1 [hidden], h_w2 [hidden] host floats; hidden <= 16.  fp32: per
 * hidden unit an fma chain over a lane's 8-channel pieces and a 4-lane butterfly, erff, expf, the division; one fma and one fp16 rounding per output.  X's channels >= C are
 * ignored; out's are written as zeros.  d_out may be d_x or d_y. */
int innfer_aim_mix(const void* d_x, int64_t x_gs, const void* d_y, int64_t y_gs, void* d_out, int64_t out_gs, const void* d_gate, int N, int64_t HW, int C, int c_pad,
                   int hidden, const float* h_w1, const float* h_b1, const float* h_w2, float b2, void* stream);
/* innfer_layer_norm_wide: innfer_layer_norm over slabs of up to 512 channels (c_pad % 64 == 0; DAT's ffn.sg.norm on half the hidden channels).  Same arithmetic and order. */
int innfer_layer_norm_wide(const void* d_in, int64_t in_gs, void* d_out, int64_t out_gs, int64_t npix, int C, int c_pad, const float* h_gamma, const float* h_beta, float eps,
                           void* stream);
/* (124, additive) The 16 x 16 window self-attention for heads WIDER than one 32-channel group, as a single launch (for tests; csrc/win_attn16_wide.hip).  32 < head_dim <= 128;
 * a head owns G = ceil(head_dim / 32) consecutive groups: d_qkv holds 3 num_heads G groups (q of head h in groups h G .. h G + G - 1 -- head_dim real channels, then zeros,
 * q already scaled -- then the num_heads G groups of k, then those of v), d_out num_heads G groups whose channels >= head_dim of every head are written as zeros.  Hp, Wp
 * multiples of 16; shift 0 or 8 (the windows of the rolled frame, -100 between regions); h_bias [num_heads][256][256].  Arithmetic as innfer_window_attention16's: fp32 scores
 * (the G channel steps chained in one accumulator), running maximum and sum over blocks of 64 keys; P rounded to fp16 in front of P v; fp32 accumulation; one rounding of
 * o / sum.  Refused with a status, before anything is uploaded or written: head_dim <= 32 (innfer_window_attention16 takes those) or > 128, sizes that are no multiples of 16,
 * a shift other than 0 or 8.  Uploads the table, launches, waits. */
int innfer_window_attention16_wide(const void* d_qkv, int64_t qkv_gs, void* d_out, int64_t out_gs, const float* h_bias, int N, int Hp, int Wp, int num_heads, int head_dim,
                                   int shift, void* stream);
/* (124, additive) innfer_layer_norm over a slab whose real channels are [0, C) and [32 ceil(C / 32), c_end) (csrc/layer_norm.hip; DRCT's dense slab: x in its own groups,
 * every 32-channel x_k in one group behind them).  The hole [C, 32 ceil(C / 32)) and the channels from c_end on stay out of the statistics whatever they hold -- NaN
 * included -- and are written as zeros.  c_pad % 64 == 0, <= 512; h_gamma / h_beta: c_pad host floats in SLAB order.  Same arithmetic and order; d_in == d_out allowed. */
int innfer_layer_norm_holed(const void* d_in, int64_t in_gs, void* d_out, int64_t out_gs, int64_t npix, int C, int c_end, int c_pad, const float* h_gamma,
                            const float* h_beta, float eps, void* stream);
/* (124, additive) DRCT (Hsu et al. 2024, "DRCT: Saving Image Super-Resolution away from Information Bottleneck"; the reference has no such architecture).  Written down
 * without the published drct_arch.py at hand: that file is the definition, and a checkpoint's shapes are authoritative over the formulas here.  C = embed_dim, gc = 32,
 * 16 x 16 windows, tokens = pixels:
 *   forward(x):  reflect-pad right / bottom to multiples of 16; f = conv_first(x - mean); f = conv_after_body(norm(RDG_{R-1}(.. RDG_0(patch_embed.norm(f))))) + f;
 *                conv_before_upsample + LeakyReLU(0.01); upsample (pixelshuffle); conv_last; + mean; crop
 *   RDG(x):      x_k = lrelu_0.2(adjust_k(swin_k(cat(x, x_1 .. x_{k-1})))) for k = 1 .. 4 (dim_k = C + 32 (k - 1) -> 32);  x_5 = adjust_5(swin_5(cat(x, x_1 .. x_4))) (-> C);
 *                return 0.2 x_5 + x          (adjust_k: a 1x1 conv with bias)
 *   swin_k(t):   t = t + proj(attn(norm1(t)));  t = t + fc2(GELU(fc1(norm2(t))));  attn: shift 8 for k = 2, 4; softmax(q d^-0.5 k^T + B_h + M) v, nH_k heads of d = dim_k / nH_k
 * on the engine of innfer_net_*.  h_heads / h_hidden: 5 n_groups ints, block k of group g at 5 g + k -- read off the checkpoint (relative_position_bias_table.shape[1],
 * fc1.weight.shape[0]).  torch.cat is never materialised: one dense slab holds x in its own ceil(C / 32) groups (pad channels zero) and every x_k in one group behind them;
 * the caller permutes the input columns of every norm, qkv, fc1 and adjust to that order, zero columns at the hole and the pads; qkv rows and proj columns are head-padded as
 * innfer_window_attention16_wide's slab (G = 1: innfer_window_attention16's).  Conv slots `<state-dict key>#<p>` in forward order: conv_first; per block attn.qkv, attn.proj,
 * mlp.fc1, mlp.fc2, then layers.<g>.adjust<k> (ONE slice for k < 5: 32 real rows and 32 zero rows, which clear the next group of the dense slab; C_pad / 64 slices for k = 5);
 * conv_after_body; the pixelshuffle tail.  LayerNorms in forward order: 0 patch_embed.norm (C_pad floats), per block norm1, norm2 (lp_k floats each, slab order), the last one
 * norm.  Bias tables: block b's [nH_b][256][256].  Limits (INNFER_ERR_UNSUPPORTED): embed_dim <= 256; <= 8 heads of <= 128 channels, dim_k % nH_k == 0; hidden <= 1024;
 * in_nc == out_nc in 1 .. 4; scale 2, 3, 4; the fp16 mode only.  Launches of a forward, with S1 = C_pad / 64, per block lp_k = 32 (ceil(C / 32) + k - 1) rounded up to 64,
 * S = lp_k / 64, SQ = ceil(3 nH G / 2), SH = hidden_pad / 64, A = 1 (k < 5) | S1 (k = 5), T = 2 + log2(scale) (4 for scale 3):
 *   2 S1 + 2 + sum over blocks (3 + SQ + 2 S + SH + A) + T + 2 [H x W is not Hp x Wp]. */
int innfer_drct_create(innfer_net_t* out, int in_nc, int out_nc, int embed_dim, int n_groups, const int* h_heads, const int* h_hidden, int scale, const float* h_mean);
/* (123, additive) DAT (Chen et al. 2023, "Dual Aggregation Transformer for Image Super-Resolution"; the reference has no such architecture), the published dat_arch.py, on
 * SwinIR's skeleton WITHOUT padding (the engine works on H x W).  C = embed_dim, nH heads of d = C / nH, split = [s0, s1], hid = hidden, tokens = pixels:
 *   forward(x):  f = conv_first(x - mean); f = conv_after_body(norm(RGs(before_RG.1(f)))) + f; tail (pixelshuffle | pixelshuffledirect); + mean
 *   RG i:        t = conv(blocks(t)) + t                      ('1conv' | '3conv' as SwinIR's)
 *   block b:     t = t + attn(norm1(t));  t = t + ffn(norm2(t));   attn: even b (inside its group) the windows (ASA), odd b the channels (ACA)
 *   ASA:         the attention of innfer_window_attention_rect over qkv = Linear(C, 3 C)(u); shifted when (i even and b > 0 and (b - 2) % 4 == 0) or (i odd and b % 4 == 0),
 *                or where h_shift (one int per block, counted through the groups; may be NULL) says so
 *   ACA:         the attention of innfer_channel_attention_scores / _apply with temperature[h]
 *   both:        c = GELU(BN(dwconv3x3(v)));  out = proj(X sigmoid(cm(mean_pixels(Y))) + Y sigmoid(sm(X))), (X, Y) = (a, c) for ASA, (c, a) for ACA (innfer_aim_mix);
 *                the mean runs over the H x W grid of ONE sample of whatever the forward is given
 *   ffn:         h = GELU(fc1(u)); x1, x2 = halves; fc2(x1 * dwconv3x3(LayerNorm(hid / 2)(x2)))
 * on the engine of innfer_net_*, laid out as innfer_swinir_create's.  Conv slots `<state-dict key>#<p>` in forward order: conv_first; per block attn.qkv (rows as SwinIR's
 * re-layout, the q rows of an ODD block WITHOUT d^-0.5), attn.proj (columns head x 32), ffn.fc1 (rows: x1's hid / 2 padded to h1p = 64 ceil(hid / 128) with zero rows,
 * then x2's likewise), ffn.fc2 (h1p input columns); per group its conv; conv_after_body; the tail.  LayerNorms (innfer_net_set_layer_norm): 0 before_RG.1; 1 + 2 k and
 * 2 + 2 k norm1 / norm2 of block k (counted through the groups); the last one norm.  innfer_net_set_attn_bias(net, k, .) takes the dense [nH][T][T] table of an EVEN block
 * (T = s0 s1; heads nH / 2 .. nH - 1 in their own s1 x s0 token order); innfer_net_set_dat_block everything else of block k, in the head-padded channel order
 * (channel 32 h + e = channel d h + e of the model for e < d, zeros for e >= d; Chp = 32 nH), as ONE array of innfer_dat_block_floats(net) host floats:
 *   dwconv taps [Chp][9], bias [Chp] (BatchNorm folded) | channel_interaction W1 [C / 8][Chp], b1 [C / 8] (BatchNorm folded), W2 [Chp][C / 8], b2 [Chp] |
 *   spatial_interaction W1 [C / 16][Chp], b1 [C / 16] (BatchNorm folded), w2 [C / 16], b2 [1] | ffn.sg.norm gamma [hid / 2], beta [hid / 2] |
 *   ffn.sg.conv taps [hid / 2][9], bias [hid / 2] | temperature [nH] (zeros for an even block)
 * Limits: C in 16 .. 256, nH 2, 4, 6 or 8, d <= 32, hid even and <= 1024, split [8, 32] or [8, 16], in_nc == out_nc in 1 .. 4, upsampler 0 pixelshuffle | 1
 * pixelshuffledirect, scale 2, 3, 4; fp16 mode only.  Launches of a forward, with B0 / B1 the blocks of even / odd index in their group, R the groups, S1 = C_pad / 64,
 * SQ = 3 nH / 2, SF = 2 h1p / 64, SR = S1 ('1conv') or 2 ceil(C / 256) + S1 ('3conv'), T = 2 (pixelshuffledirect), 2 + log2(scale) (pixelshuffle 2 / 4), 4 (pixelshuffle 3):
 *   S1 + 2 + B0 (9 + SQ + 2 S1 + SF) + B1 (11 + SQ + 2 S1 + SF) + (R + 1) SR + T. */
int innfer_dat_create(innfer_net_t* out, int in_nc, int out_nc, int embed_dim, const int* depths, int n_layers, int num_heads, int hidden, int s0, int s1, int upsampler,
                      int scale, int conv3, const float* h_mean, const int* h_shift);
size_t innfer_dat_block_floats(innfer_net_t net);
int innfer_net_set_dat_block(innfer_net_t net, int blk, const float* h_params, size_t n_floats);
/* The activation behind conv `idx` as K host floats: y = x >= 0 ? x : h_slope[c] * x -- nn.PReLU(num_parameters = K).weight, or the constant 0 (ReLU) / 0.1
 * (LeakyReLU(0.1)).  Load time, synchronous.  Every conv of an SRVGGNetCompact except the last needs one before the first forward; other convs refuse it. */
int innfer_net_set_conv_slope(innfer_net_t net, int idx, const float* h_slope);

/* Arithmetic precision of innfer_net_forward, the reference's fp16 switch (`fp16 = not args.no_fp16 and gpu`, then `model.half()` / `t_img.half()`:
 * run.py:345,383,421-422).  fp32 = 0 (default): fp16 activations and weights, fp32 accumulation.  fp32 = 1: the fp32-accurate forward -- every activation
 * is kept as a PAIR of fp16 slabs (hi = fp16(x), lo = fp16((x - hi) * 2^11): 22 significant bits), every weight as a pair of panels, and a product is
 * xh wh + 2^-11 (xh wl + xl wh) on the fp16 matrix cores with fp32 accumulation; input fp32 or uint8, twice the workspace (ask innfer_net_workspace_bytes
 * after this call), three times the MFMA work.  Against the fp32 reference: <= 1e-4 on [0,1]-scaled outputs (SURVEY 8c; measured ~1e-6).  Built for
 * RRDBNet / SRResNet (every constructor variant of innfer_*_create_ex); the other generators have their own fp32 mode (innfer_<api>_set_precision, 108).  (106)
 * A LOAD-TIME call: with fp32 = 1 it builds the split weight panels of every conv set so far (hipMalloc + synchronous copies; INNFER_ERR_NOMEM when they
 * do not fit -- the panels this call had built are released again) -- outside stream capture; innfer_net_forward itself never allocates.  Either call
 * order works: an innfer_net_set_conv on a network that is already in the fp32 mode builds that conv's panels itself (110). */
int innfer_net_set_precision(innfer_net_t net, int fp32);

void innfer_net_destroy(innfer_net_t net);

/* Convolutions in forward order.  key is the state-dict prefix in the
 * reference's naming ("model.1.sub.0.RDB1.conv1.0"); weights are
 * key+".weight" [K,C,3,3] and key+".bias" [K]. */
int innfer_net_num_convs(innfer_net_t net);
int innfer_net_conv_info(innfer_net_t net, int idx, char* key, size_t key_cap, int* K, int* C);

/* Replaces net.load_state_dict for one conv (run.py:93): host fp32 OIHW
 * weights + bias are packed into the MFMA panel layout and uploaded.
 * Synchronous (load time, not forward time). */
int innfer_net_set_conv(innfer_net_t net, int idx, const float* h_weight_oihw, const float* h_bias);

int innfer_net_scale(innfer_net_t net);
size_t innfer_net_workspace_bytes(innfer_net_t net, int N, int H, int W);

/* nn.Module.forward(x): d_in [N,in_nc,H,W] -> d_out [N,out_nc,s*H,s*W], NCHW,
 * dtypes per innfer_dtype.  Replaces `self.model(data)` (run.py:187-189,217-219). */
int innfer_net_forward(innfer_net_t net, const void* d_in, int in_dtype, void* d_out, int out_dtype,
                       int N, int H, int W, void* d_workspace, size_t workspace_bytes, void* stream);

/* Same forward with a HIP-event pair around every kernel launch (on `stream`), then a
 * stream synchronise.  Fills up to `cap` entries: elapsed ms, algorithmic FLOPs, algorithmic HBM
 * bytes (every operand read once, every result written once: (C + K) * 2 B per output pixel,
 * + K * 2 B per residual, + the weight panel) and kernel kind (0 = first conv; 16*NT +
 * out_mode = the conv instantiation with NT 16-channel output tiles; + 1000 its fp32-accurate form,
 * + 2000 the fused HR_conv0 + conv_last launch, + 3000 an up-conv as four 2x2-tap phases, whose FLOPs
 * are the algorithmic ones of the nine-tap layer it replaces: it executes 4/9 of them).  Used by
 * bench.py for the roofline object (both roofs per kernel). */
int innfer_net_forward_timed(innfer_net_t net, const void* d_in, int in_dtype, void* d_out, int out_dtype,
                             int N, int H, int W, void* d_workspace, size_t workspace_bytes, void* stream,
                             int cap, float* h_ms, double* h_flops, double* h_bytes, int* h_kind, int* n_launches);

/* Scheduling knob: 0 = one launch per layer over the whole frame; R>0 = skewed
 * row bands of R rows through the RRDB trunk (working set kept Infinity-Cache
 * resident; identical results). */
/* uint8 images at the network boundary (104): innfer_net_forward accepts INNFER_U8 as in_dtype and / or out_dtype.  The input then is N
 * uint8 HWC BGR(A) images back to back and np2tensor (utils/utils.py:164-194: /255, BGR->RGB, optional [-1,1] normalisation, `.half()` in fp16
 * mode) runs as the first conv's prologue; the output is N uint8 HWC BGR(A) images and tensor2np (utils/utils.py:197-248: optional
 * denormalisation, clip(255 x).round() half to even, RGB->BGR) runs as the last conv's epilogue.  Bit-identical to the separate passes
 * innfer_u8hwc_to_nchw / innfer_nchw_to_u8hwc around a float forward.  normalize: the `normalize` / `denormalize` flag of both; fp16_mode != 0:
 * values are rounded to fp16 where the reference's fp16 mode holds an fp16 tensor (default 1). */
int innfer_net_set_u8_io(innfer_net_t net, int normalize, int fp16_mode);

int innfer_net_set_band_rows(innfer_net_t net, int rows);

/* The residual of a dense block's last conv (`x5 * 0.2 + x`, RRDBNet_arch.py:161-165) is that conv's own input channels 0..63.  With the LDS form the
 * kernel stages those two channel groups LAST and adds x / 0.2 to the fp32 accumulators from the staged LDS tile; the epilogue scales by 0.2 -- x is not
 * read a second time (265 MB of a 1327 MB launch at 1080p).  on = 1 (default): the last dense block of every RRDB, whose epilogue also adds the RRDB's own
 * residual (RRDBNet_arch.py:98) -- the measured gain (-3.7 % on those launches; the one-residual launches lose 0.9 % with it); on = 2: every dense block;
 * on = 0: epilogue loads everywhere.  The sum is formed in another order than fma(acc, 0.2, x) (fp32 either way): results agree across the settings to the
 * last rounding of the fp16 output, not bit for bit.  fp16 engine, nf = 64; everything else ignores the switch.  (108) */
int innfer_net_set_residual_lds(innfer_net_t net, int on);

/* Scheduling knob: the 64-output 3x3 slab convs of RRDBNet's trunk (every dense block's conv5 and the trunk conv; fp16 engine, 64 features) run their eight consumer
 * waves as a 2 x 4 grid -- 2 halves of 32 output channels x 4 groups of 4 rows over the same 16 x 32 tile -- instead of 8 groups of 2 rows x 64 channels: half the
 * weight-fragment registers per wave, and in the freed registers the tile's memory residual, loaded a whole chunk of MFMAs ahead of the epilogue that adds it.
 * 1 (default) = that form wherever it exists; 0 = the 8 x 1 form.  Every accumulator sees the same products in the same order: results are bit-identical. */
int innfer_net_set_consumer_grid(innfer_net_t net, int mode);

/* Scheduling knob: the last two convs of RRDBNet / SRResNet (HR_conv0 -> LeakyReLU -> conv_last, RRDBNet_arch.py:36-42) as ONE kernel -- the last conv
 * runs in the epilogue of HR_conv0 on the tile that kernel has just produced (csrc/conv3x3.hip, FUSE: no halo recompute; the pixels within one pixel
 * of a tile edge are finished by a small second pass), and the HR feature slab (4.25 GB for a 1080p -> 4K frame) is neither written nor read.
 * 1 (default) = fused wherever the shapes allow it: fp16 engine, 64 features, <= 3 output channels (planar fp16 / fp32 or the uint8 image), no final activation / outm, HR frame of whole
 * 16 x 32 tiles, no row bands; every other case runs the two launches.  0 = always two launches.  The fused form adds the last conv's 576 products of
 * an output in a different order (fp32 either way): results agree to the last rounding of the fp16 output, not bit for bit.  (107) */
int innfer_net_set_fused_tail(innfer_net_t net, int on);
/* on (default): the LAST upconv_block -> HR_conv0 -> conv_last (RRDBNet_arch.py:31-42, block.py:348-361) run as ONE kernel chained through LDS where the fused tail and the
 * one-visit up-conv both apply (fp16 engine, 64 features, whole 16 x 32 output tiles): the 64-channel HR tensor between them is neither written nor read.  Bit-identical to
 * the two launches it replaces (off).  ABI 111. */
int innfer_net_set_hr_chain(innfer_net_t net, int on);

/* Scheduling knob: the conv of an upconv_block (nn.Upsample(nearest 2x) -> conv 3x3 -> act, block.py:348-361) as the four 2x2-tap output phases of the
 * equivalent ConvTranspose2d(4, 2, 1) on the LR grid -- 2.25 x fewer multiply-adds than nine taps on the HR grid.  The taps that meet the same LR pixel are
 * summed in fp32 and rounded to fp16 ONCE (the nine-tap form rounds each of them): the same linear map with a rounding of the same size, not the same bits.
 * 1 (default) = phases for the fp16 engine where the conv has 64 n output channels -- 64 -> 64 convs on grids wider than 16 pixels compute all four phases in ONE visit of
 * a tile (the input tile staged once); 2 = one phase per visit of a tile everywhere (the same bits as 1: A/B and parity tests) (109); 0 = the nine-tap form through
 * the upsampling loader.  (107) */
int innfer_net_set_upconv_phases(innfer_net_t net, int mode);

/* `finalact` of the reference constructors (RRDBNet_arch.py:45-48: an activation module after the last conv):
 * 0 none (default), 1 LeakyReLU(0.2), 2 ReLU, 3 tanh, 6 sigmoid. */
int innfer_net_set_final_act(innfer_net_t net, int act);

/* `outm` of RRDBNet.forward / SRResNet.forward (RRDBNet_arch.py:50-62): a range limiter applied to the network's output, after `finalact`:
 * 0 none (default), 1 'scaltanh' (tanh(x) + 1) / 2, 2 'tanh', 3 'sigmoid', 4 'clamp' to [0, 1] -- in the last conv's epilogue.  (104) */
int innfer_net_set_outm(innfer_net_t net, int outm);

/* Algorithmic FLOPs of one forward (2*MAC of every conv; SURVEY.md 8d). */
double innfer_net_flops(innfer_net_t net, int N, int H, int W);

/* ------------------------------------------------------------- pix2pix UNet
 * Replaces UnetGenerator(norm=batch, upsample_mode=deconv).forward (architectures/UNet_arch.py:11-161)
 * as run.py runs it for `-a p2p_256 / unet_256` (meval=False: BatchNorm uses the statistics of the
 * current image, run.py:299-303).  A batch is N independent batch-1 forwards (per-image statistics).
 * Parameters are addressed by their state-dict key ("model.model.1.model.2.weight" ...): conv /
 * conv-transpose weights in PyTorch layout, BatchNorm weight and bias, and the running statistics, which only
 * innfer_unet_set_eval(u, 1) forwards read.
 */
typedef struct innfer_unet* innfer_unet_t;
int innfer_unet_create(innfer_unet_t* out, int in_nc, int out_nc, int num_downs, int ngf);
/* The same with norm_type 'instance' (UNet_arch.py:38-41,101-104): nn.InstanceNorm2d layers (no parameters, no running statistics: always the
 * statistics of the image, train() and eval() alike) and a bias on every conv (it only matters where no norm follows: the outermost and the
 * innermost down conv, the outermost up conv).  upconv: upsample_mode 'upconv' (UNet_arch.py:119-122,131-134,143-146; block.py:348-361) -- every
 * ConvTranspose2d(4, 2, 1) is Upsample(nearest 2x) + Conv2d(3x3, zero padding), keys `<i>.1.weight`.
 * innfer_unet_create(...) = innfer_unet_create_ex(..., 0, 0).  (104) */
int innfer_unet_create_ex(innfer_unet_t* out, int in_nc, int out_nc, int num_downs, int ngf, int instance_norm, int upconv);
void innfer_unet_destroy(innfer_unet_t u);
int innfer_unet_num_params(innfer_unet_t u);
int innfer_unet_param_info(innfer_unet_t u, int idx, char* key, size_t key_cap, int* ndim, int* shape4);
int innfer_unet_set_param(innfer_unet_t u, int idx, const float* h_data);
/* nn.Module.eval() / .train() (run.py:96-99): eval_mode != 0 normalises with the running statistics ("...running_mean" / "...running_var",
 * set like any other parameter; unset = a fresh BatchNorm's 0 / 1) as ATen's eval-mode batch_norm does: alpha = weight / sqrt(running_var + eps),
 * y = x * alpha + (bias - running_mean * alpha).  Default 0: statistics of the current image (how run.py runs pix2pix, meval=False). */
int innfer_unet_set_eval(innfer_unet_t u, int eval_mode);
/* The reference's fp16 switch for this generator (`fp16 = not args.no_fp16 and gpu`, run.py:345,421-422).  fp32 = 0 (default): the fp16 engine.  fp32 = 1: every
 * conv, norm and activation in fp32 on NCHW fp32 tensors (csrc/f32ops.hip: v_mfma_f32_16x16x4_f32, fp32 statistics) -- <= 1e-4 of the fp32 reference (SURVEY 8c);
 * innfer_unet_forward then takes and returns INNFER_F32 only, and innfer_unet_workspace_bytes answers for this mode.  A load-time call (packs fp32 panels:
 * hipMalloc + synchronous copies); call it after the last innfer_unet_set_param.  (108) */
int innfer_unet_set_precision(innfer_unet_t u, int fp32);
size_t innfer_unet_workspace_bytes(innfer_unet_t u, int N, int H, int W);
double innfer_unet_flops(innfer_unet_t u, int N, int H, int W);
/* d_in [N,in_nc,H,W] -> d_out [N,out_nc,H,W] (tanh range), NCHW f16/f32; H, W multiples of 2^num_downs. */
int innfer_unet_forward(innfer_unet_t u, const void* d_in, int in_dtype, void* d_out, int out_dtype,
                        int N, int H, int W, void* d_workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------- PAN
 * Replaces PAN.forward (architectures/PAN_arch.py:163-222) with its SCPA blocks (PAN_arch.py:47-106),
 * PAConv (PAN_arch.py:24-45), the FSA SelfAttentionBlock on a 4x max-pooled map (block.py:398-473,
 * bicubic re-expansion) and the nearest pixel-attention up-blocks (block.py pa_upconv_block), as
 * utils/defaults.py:78-89 configures them: nf 40, unf 24, nb 16, scale 1/2/3/4, self_attention=True,
 * double_scpa=False, ups_inter_mode='nearest'.  Parameters are addressed by state-dict key
 * ("SCPA_trunk.3.PACnv.k2.weight" ...), PyTorch layout, fp32 host data.
 */
typedef struct innfer_pan* innfer_pan_t;
int innfer_pan_create(innfer_pan_t* out, int in_nc, int out_nc, int nf, int unf, int nb, int scale);
/* The same with PAN's graph-changing constructor arguments (PAN_arch.py:115-141): self_attention = 0 drops the FSA block (fea + trunk goes
 * straight to the upsampler), double_scpa != 0 runs a second SCPA trunk + `trunk_conv2` behind the first, bilinear_up != 0 =
 * ups_inter_mode 'bilinear' (the up-blocks' B.Upsample(2, mode), align_corners False: PAN_arch.py:11-19, block.py:286-323) instead of 'nearest'.
 * innfer_pan_create(...) = innfer_pan_create_ex(..., 1, 0, 0).  (104) */
int innfer_pan_create_ex(innfer_pan_t* out, int in_nc, int out_nc, int nf, int unf, int nb, int scale, int self_attention, int double_scpa, int bilinear_up);
void innfer_pan_destroy(innfer_pan_t p);
int innfer_pan_num_params(innfer_pan_t p);
int innfer_pan_param_info(innfer_pan_t p, int idx, char* key, size_t key_cap, int* ndim, int* shape4);
int innfer_pan_set_param(innfer_pan_t p, int idx, const float* h_data);
size_t innfer_pan_workspace_bytes(innfer_pan_t p, int N, int H, int W);
/* Schedule of the SCPA trunk (PAN_arch.py:58-105).  on = 1 (default): a block is ONE launch -- conv1_a | conv1_b, k1, k3 * sigmoid(k2), k4, conv3 and the
 * residual on a 16 x 32 pixel tile with a 2-pixel halo, intermediates in LDS / registers, the block's weights resident in LDS (csrc/pan_scpa.hip); on = 0:
 * five launches of the halo-tile conv kernel per block (rounds 1-3).  Same fp16 roundings of every intermediate tensor; the fp32 sums of conv1 and conv3 are
 * formed per 32-channel k-step in both, so results agree to the last rounding of the fp16 tensors.  on != 0 also moves the FSA block's attention
 * (softmax(f^T g) h over the pooled pixels, block.py:398-473) from the VALU kernel to the matrix cores: scores from fp16 (hi, lo) pairs -- fp32-accurate --,
 * exact row maxima, exp and sums in fp32, p and h as fp16 operands of the P V product; on = 2 keeps the VALU attention behind the fused blocks; on = 3 (110) keeps the
 * trunk tensors on two-group slabs between the fused blocks (default since 110: channels 32..39 travel as a compact 16-byte plane there; same bits); on = 4 (110) runs the
 * last stage's HRconv and conv_last as two launches (default since 110 where the full-resolution grid is whole 16 x 32 tiles: conv_last in HRconv's epilogue, the 24-channel
 * full-resolution tensor neither written nor read; same values to the summation order of conv_last).  (108)
 * In the fp32 mode (innfer_pan_set_precision(p, 1); since 113): on != 0 runs the SCPA blocks (csrc/pan_scpa_split.hip), the up-stages and the attention on
 * (hi, lo) fp16 operand pairs of the matrix cores, on = 0 every conv on the generic fp32 kernel and the attention on the VALU kernel (the form of 108 - 112);
 * on = 5 keeps the PA block of an up-stage as its own 1x1 launch instead of the up-conv's epilogue (A/B).
 * fp16 (113): the block kernel has two forms with the same bits -- one 8-wave workgroup per CU on 16 x 32 tiles, two 4-wave workgroups per CU on 8 x 32 tiles (x loaded straight into
 * MFMA fragments; the default) -- on = 6 / 7 force the second / the first (A/B). */
int innfer_pan_set_fused_scpa(innfer_pan_t p, int on);
/* The reference's fp16 switch for this generator (run.py:345,421-422), as innfer_unet_set_precision: fp32 = 1 runs PAN.forward with fp32-accurate arithmetic
 * -- <= 1e-4 of the fp32 reference; fp32 tensors in and out; a load-time call.  (108: every conv on the generic fp32 kernel of csrc/f32ops.hip, the FSA
 * attention on the fp32 VALU kernel.  113: the SCPA trunk, nearest-2x up-stages and the attention as three-MFMA products of (hi, lo = (x - hi) * 2^11) fp16
 * pairs with fp32 accumulation -- the SR engine's SPLIT convention; conv_first, the trunk conv, the f | g | h projections, bilinear / 3x stages stay on f32ops.) */
int innfer_pan_set_precision(innfer_pan_t p, int fp32);
/* d_in [N,in_nc,H,W] -> d_out [N,out_nc,scale*H,scale*W], NCHW f16/f32; H, W >= 4. */
int innfer_pan_forward(innfer_pan_t p, const void* d_in, int in_dtype, void* d_out, int out_dtype,
                       int N, int H, int W, void* d_workspace, size_t workspace_bytes, void* stream);
/* (122, additive) The launches of the FSA block (block.py:398-473) one at a time, for tests: the launch functions both forwards call (csrc/pan.hip att_launch /
 * maxpool_launch / fsa_combine_launch, csrc/f32ops.hip f32_maxpool4_launch / f32_fsa_combine_launch).  All pointers are device pointers; no network object is needed.
 * innfer_pan_attention: out[n][i][c] = sum_j softmax_j((f_i + bf) . (g_j + bg)) (h_j[c] + bh[c]).  d_fgh: fp32 [N][Np][64] rows [f(5) | g(5) | h(40) | 14 unused], as the
 *   projection GEMM writes them; d_bf / d_bg / d_bh: 5 / 5 / 40 floats; d_out: fp32 [N][Np][40].  form 0: pan_attention (the VALU kernel, no workspace); 1: pan_attn_prep +
 *   pan_attention_mfma<false> (the fp16 engine's); 2: the same pair with <true>, p and h as (hi, lo) fp16 pairs too (the fp32 mode's).  d_ws: at least
 *   innfer_pan_attention_workspace_bytes(N, Np, form) bytes (0 for form 0) -- the function the forwards' workspace carve uses; it need not be cleared.
 *   Refused, with nothing launched: Np < 1, N outside 1 .. 65535, an unknown form (INNFER_ERR_INVALID), a short or missing workspace (INNFER_ERR_WORKSPACE).
 * innfer_pan_maxpool: nn.MaxPool2d(4).  dtype INNFER_F16: d_in / d_out are blocked fp16 slabs [ceil(C / 32)][N * H * W][32] / [ceil(C / 32)][N * (H/4) * (W/4)][32]
 *   (pan_maxpool; C % 8 == 0, the output's channels C .. 32 ceil(C / 32) are written as zeros); INNFER_F32: NCHW fp32 (f32_maxpool4_launch).  H < 4 or W < 4 is refused.
 * innfer_pan_fsa_combine: out = gamma[0] * bicubic(att, size = (H, W), align_corners = False) + inp; d_att fp32 [N][hp * wp][C].  INNFER_F16: d_inp / d_out slabs as
 *   above (C % 8 == 0); pan_fsa_combine_x4 when W == 4 wp and form == 0, else pan_fsa_combine -- the forward's choice.  INNFER_F32: NCHW fp32 through
 *   f32_fsa_combine_launch; d_scratch (N * C * hp * wp floats, the transposed att) lets it take the strip kernel when W == 4 wp; form == 1 or a NULL scratch forces
 *   the one-pixel kernel.  The strip and the one-pixel kernels give the same bits. */
size_t innfer_pan_attention_workspace_bytes(int N, int Np, int form);
int innfer_pan_attention(const float* d_fgh, const float* d_bf, const float* d_bg, const float* d_bh, int N, int Np, int form, float* d_out,
                         void* d_workspace, size_t workspace_bytes, void* stream);
int innfer_pan_maxpool(const void* d_in, int dtype, int N, int C, int H, int W, void* d_out, void* stream);
int innfer_pan_fsa_combine(const float* d_att, int hp, int wp, int C, const void* d_inp, int dtype, int N, int H, int W, const float* d_gamma, int form,
                           void* d_out, float* d_scratch, void* stream);
/* (122, additive) One SCPA block (PAN_arch.py:58-105) as a single launch, for tests: x -> x + conv3(cat[lrelu(k1(lrelu(conv1_a x))), lrelu(k4(k3(b) * sigmoid(k2(b) + bias)))]),
 * b = lrelu(conv1_b x), 40 channels, through the launch functions both forwards call (csrc/pan_scpa.hip pan_scpa_launch, csrc/pan_scpa_split.hip pan_scpa_split_launch);
 * the grid and the tiles are theirs.  No network object is needed.
 * innfer_pack_pan_scpa: host fp32 weights in torch layouts -- conv1_a / conv1_b [20][40], k1 / k3 / k4 [20][20][3][3], k2 [20][20] + bias [20], conv3 [40][40] -- into the
 *   kernel's blob of innfer_pan_scpa_blob_bytes(split) bytes (split != 0: the (hi, lo) blob pair of the fp32 mode); the caller uploads it.
 * innfer_pan_scpa_block, form 0 (pan_scpa_fused<16>: one 8-wave workgroup per CU, 16 x 32 tiles), 1 (pan_scpa_duo: two 4-wave workgroups per CU, 8 x 32 tiles), -1 (the forward's
 *   choice): d_in / d_out are fp16 slabs of TWO 32-channel groups, npx = N * H * W pixels, group_stride >= npx * 32 elements between the groups:
 *     channel c < 32 of pixel p at element p * 32 + c; channel 32 + c (c < 8) at group_stride + p * 32 + c.
 *   Channels 40 .. 63 are pad channels: the kernels never read them and write them as zeros.  in_c8 / out_c8 != 0: channels 32 .. 39 of the input / output travel as a COMPACT
 *   plane of 16 bytes per pixel instead -- channel 32 + c at element group_stride + p * 8 + c; nothing else of group 1 is read / written (a compact output leaves the other
 *   48 bytes per pixel of a two-group slab untouched).  The same values bit for bit whatever the form and the flags.
 *   form 2 (pan_scpa_split, 8 x 32 tiles): d_in / d_out are SPLIT PLANES of 160 npx bytes -- every value x as hi = fp16(x), lo = fp16((x - hi) * 2^11) --
 *     [hi, channels 0 .. 31: 64 B per pixel][hi, 32 .. 39: 16 B per pixel][lo, 0 .. 31: 64 B per pixel][lo, 32 .. 39: 16 B per pixel]
 *   at byte offsets 0, 64 npx, 80 npx, 144 npx; group_stride, in_c8 and out_c8 must be 0.
 *   Refused with nothing launched: a null pointer, N, H or W < 1, an unknown form, group_stride < npx * 32, a split form with a stride or a compact flag (INNFER_ERR_INVALID);
 *   a tensor beyond 32-bit byte offsets -- npx * 64 + 2 group_stride >= 2^31 - 1 for the fp16 forms, npx * 160 >= 2^31 - 1 for the split form (INNFER_ERR_UNSUPPORTED).
 * innfer_pan_split_from_nchw / _to_nchw: NCHW fp32 [N][40][H][W] <-> split planes (to_nchw gives hi + 2^-11 lo in fp32). */
size_t innfer_pan_scpa_blob_bytes(int split);
int innfer_pack_pan_scpa(const float* h_conv1_a, const float* h_conv1_b, const float* h_k1, const float* h_k2, const float* h_k2_bias, const float* h_k3, const float* h_k4,
                         const float* h_conv3, int split, void* h_blob);
int innfer_pan_scpa_block(const void* d_in, void* d_out, int64_t group_stride, const void* d_blob, int N, int H, int W, int form, int in_c8, int out_c8, void* stream);
int innfer_pan_split_from_nchw(const float* d_x, void* d_planes, int N, int H, int W, void* stream);
int innfer_pan_split_to_nchw(const void* d_planes, float* d_x, int N, int H, int W, void* stream);
/* (124, additive) The kernels at the two ends of the forwards one launch at a time, for tests: the launch functions both forwards call (csrc/pan.hip pan_pre_launch /
 * pan_upsample_launch / pan_final_launch / pan_slab_pair_launch, csrc/f32ops.hip f32_upsample_launch).  Device pointers; no network object is needed.
 * innfer_pan_pre: NCHW [N][C][H][W] (fp16 | fp32, rounded to nearest even) -> one fp16 group [N * H * W][32], channels C .. 31 written as zeros.  C > 32: INNFER_ERR_UNSUPPORTED.
 * innfer_pan_upsample: F.interpolate(scale_factor = f, f = 2 | 3; bilinear 0: 'nearest', 1: 'bilinear' with align_corners=False).  INNFER_F16: blocked slabs of C / 32 groups
 *   (C = 32 | 64; [N * h * w][32] -> [N * f h * f w][32], the groups in_group_stride / out_group_stride elements apart; pan_upsample); INNFER_F32: NCHW fp32, any C
 *   (f32_upsample_launch; the strides are ignored).  Refused: another f, a slab C other than 32 | 64, a group stride below N H W 32 of its side.
 * innfer_pan_final: out = raw + bilinear(x, size = (scale H, scale W), align_corners=True) (scale 1: raw + x); d_raw fp32 NCHW [N][C][scale H][scale W], 16-byte aligned;
 *   d_x [N][C][H][W] and d_out fp16 | fp32 NCHW.  form 0: pan_final (one pixel per thread); 1: pan_final_x4 (four pixels of a row per thread), refused unless
 *   (W * scale) % 4 == 0; -1: the fp16 forward's choice -- form 1 where it is accepted.  The two forms give the same bits.  scale outside 1 .. 4 is refused.
 * innfer_pan_slab_pair: fp32 NCHW [N][C][H][W] -> a (hi, lo) pair of fp16 slabs of ceil(C / 32) groups [N * H * W][32]: hi = fp16(x), lo = fp16((x - hi) * 2^11), lo_offset
 *   elements behind hi; the pad channels up to the next multiple of 32 are written as zeros in both.  Refused: lo_offset below ceil(C / 32) N H W 32 or no multiple of 8.
 * All four refuse, with nothing launched, a null pointer, a size below 1 and an unknown dtype or form (INNFER_ERR_INVALID). */
int innfer_pan_pre(const void* d_in, int in_dtype, int N, int C, int H, int W, void* d_slab, void* stream);
int innfer_pan_upsample(const void* d_in, int dtype, int N, int C, int h, int w, int f, int bilinear, int64_t in_group_stride, void* d_out, int64_t out_group_stride,
                        void* stream);
int innfer_pan_final(const float* d_raw, int C, const void* d_x, int x_dtype, int N, int H, int W, int scale, void* d_out, int out_dtype, int form, void* stream);
int innfer_pan_slab_pair(const float* d_x, int N, int C, int H, int W, void* d_slab, int64_t lo_offset, void* stream);

/* -------------------------------------------------------------------- PPON
 * Replaces PPON.forward with RRBlock_32 / _ResBlock_32 (architectures/PPON_arch.py:12-129): first conv,
 * nb residual-in-residual blocks of eight dilated 3x3 convs (rates 1..8) each, the structure / perception
 * branches and the three reconstruction heads, as utils/defaults.py:68-77 configures them (nf 64, nb 24,
 * alpha 1).  Returns the three outputs of the reference (content, structure, perceptual); run.py keeps the
 * last one (run.py:191-192).  Parameters are addressed by state-dict key ("CFEM.1.sub.3.RB2.d5.weight" ...).
 */
typedef struct innfer_ppon* innfer_ppon_t;
int innfer_ppon_create(innfer_ppon_t* out, int in_nc, int out_nc, int nf, int nb, int scale, float alpha);
void innfer_ppon_destroy(innfer_ppon_t p);
int innfer_ppon_num_params(innfer_ppon_t p);
int innfer_ppon_param_info(innfer_ppon_t p, int idx, char* key, size_t key_cap, int* ndim, int* shape4);
int innfer_ppon_set_param(innfer_ppon_t p, int idx, const float* h_data);
size_t innfer_ppon_workspace_bytes(innfer_ppon_t p, int N, int H, int W);
/* The reference's fp16 switch for this generator (run.py:345,421-422), as innfer_unet_set_precision: fp32 = 1 runs PPON.forward in fp32 on NCHW fp32 tensors
 * (csrc/f32ops.hip: the dilated convs are entries of the generic conv's tap table) -- <= 1e-4 of the fp32 reference; fp32 tensors in and out.  (108) */
int innfer_ppon_set_precision(innfer_ppon_t p, int fp32);
/* d_in [N,in_nc,H,W] -> d_out_{c,s,p} [N,out_nc,scale*H,scale*W], NCHW f16/f32; d_out_c / d_out_s may be NULL. */
int innfer_ppon_forward(innfer_ppon_t p, const void* d_in, int in_dtype, void* d_out_c, void* d_out_s, void* d_out_p,
                        int out_dtype, int N, int H, int W, void* d_workspace, size_t workspace_bytes, void* stream);
/* (124, additive) The forwards' two pass kernels one launch at a time, for tests: the launch functions they call (csrc/ppon.hip ppon_upsample3_launch / ppon_axpy_launch,
 * csrc/f32ops.hip f32_axpy_launch).  Device pointers; no network object is needed.
 * innfer_ppon_upsample3: nearest 3x of a 64-channel fp16 slab: d_in two groups [N * H * W][32] in_group_stride elements apart -> d_out two groups [N * 3H * 3W][32]
 *   out_group_stride apart.  Refused: a group stride below N H W 32 (9 N H W 32 for the output).
 * innfer_ppon_axpy: out[i] = a * x[i] + y[i], i < n; d_x may alias d_out, as the forwards call it.  form 0: ppon_axpy (the fp16 engine's kernel; dtype INNFER_F16, or
 *   INNFER_F32 as with fp32 outputs); form 1: f32_axpy_launch (the fp32 mode's; INNFER_F32 only).
 * Refused with nothing launched (INNFER_ERR_INVALID): a null pointer, a size below 1, an unknown dtype or form, form 1 on fp16 values. */
int innfer_ppon_upsample3(const void* d_in, int64_t in_group_stride, void* d_out, int64_t out_group_stride, int N, int H, int W, void* stream);
int innfer_ppon_axpy(const void* d_x, const void* d_y, void* d_out, float a, int64_t n, int dtype, int form, void* stream);

/* -------------------------------------------------------- CycleGAN ResNet
 * Replaces ResnetGenerator(norm=instance, padding=reflect, upsample=deconv).forward with ResnetBlock
 * (architectures/ResNet_arch.py:19-151; `-a resnet_9blocks / cg_6 ...`, utils/defaults.py:124-140): reflection-padded
 * 7x7 and 3x3 convs, two stride-2 convs, n_blocks residual blocks, two ConvTranspose2d(3,2,1,1), tanh; InstanceNorm2d
 * without affine parameters, statistics of the instance.  H, W multiples of 4, >= 16; ngf 32 / 64 / 96 / 128 (the presets use 64).
 */
typedef struct innfer_resnet* innfer_resnet_t;
int innfer_resnet_create(innfer_resnet_t* out, int in_nc, int out_nc, int ngf, int n_blocks);
/* The same with ResnetBlock's constructor arguments (ResNet_arch.py:104-146): padding 0 reflect / 1 replicate / 2 zero (the pad layer in front of
 * the two 3x3 convs of every block; the parameter indices inside `conv_block` follow), use_dropout != 0 = an nn.Dropout(0.5) behind the first
 * conv + norm + ReLU (identity in eval mode -- how run.py runs these generators -- but it shifts the second conv's index); upconv != 0 =
 * upsample_mode 'upconv': the two ConvTranspose2d stages become Upsample(nearest 2x) + Conv2d(3x3) (block.py:348-361; parameters `model.<i>.1`);
 * batch_norm != 0 = norm_type 'batch' (the constructor's default, ResNet_arch.py:19,39-49): nn.BatchNorm2d behind every conv but the last (parameters
 * and buffers `model.<i+1>.{weight,bias,running_mean,running_var,num_batches_tracked}`) and no bias on those convs.  (104) */
int innfer_resnet_create_ex(innfer_resnet_t* out, int in_nc, int out_nc, int ngf, int n_blocks, int padding, int use_dropout, int upconv, int batch_norm);
/* BatchNorm mode of a batch_norm generator, as innfer_unet_set_eval: 0 (nn.Module.train()) the statistics of the image, != 0 (eval(), Model's default)
 * the running statistics.  No effect on instance-norm generators.  (104) */
int innfer_resnet_set_eval(innfer_resnet_t r, int eval_mode);
void innfer_resnet_destroy(innfer_resnet_t r);
int innfer_resnet_num_params(innfer_resnet_t r);
int innfer_resnet_param_info(innfer_resnet_t r, int idx, char* key, size_t key_cap, int* ndim, int* shape4);
int innfer_resnet_set_param(innfer_resnet_t r, int idx, const float* h_data);
size_t innfer_resnet_workspace_bytes(innfer_resnet_t r, int N, int H, int W);
/* The reference's fp16 switch for this generator (run.py:345,421-422), as innfer_unet_set_precision: fp32 = 1 runs the forward in fp32 on NCHW fp32 tensors
 * (csrc/f32ops.hip) -- <= 1e-4 of the fp32 reference; fp32 tensors in and out; a load-time call.  (108) */
int innfer_resnet_set_precision(innfer_resnet_t r, int fp32);
int innfer_resnet_forward(innfer_resnet_t r, const void* d_in, int in_dtype, void* d_out, int out_dtype,
                          int N, int H, int W, void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------- WBC UNet + guided filter
 * Replaces UnetGeneratorWBC(mode='pt' or 'tf').forward with ResBlock (architectures/WBCNet_arch.py:8-99; `-a wbcunet`) and
 * guided_filter(x, y, r=1, eps) in 'regular' mode (utils/utils.py:548-626; run.py:427-429 applies it with eps 5e-3 to
 * (input image, network output)).  H, W multiples of 4 (run.py modcrops to 4).
 */
typedef struct innfer_wbc* innfer_wbc_t;
int innfer_wbc_create(innfer_wbc_t* out, int nf, int tf_mode);   /* tf_mode: tf_same_padding + tf_2xupsample_bilinear (WBCNet_arch.py:126-142) */
void innfer_wbc_destroy(innfer_wbc_t u);
int innfer_wbc_num_params(innfer_wbc_t u);
int innfer_wbc_param_info(innfer_wbc_t u, int idx, char* key, size_t key_cap, int* ndim, int* shape4);
int innfer_wbc_set_param(innfer_wbc_t u, int idx, const float* h_data);
size_t innfer_wbc_workspace_bytes(innfer_wbc_t u, int N, int H, int W);
/* The reference's fp16 switch for this generator (run.py:345,421-422), as innfer_unet_set_precision: fp32 = 1 runs the forward in fp32 on NCHW fp32 tensors
 * (csrc/f32ops.hip) -- <= 1e-4 of the fp32 reference; fp32 tensors in and out; a load-time call.  (108) */
int innfer_wbc_set_precision(innfer_wbc_t w, int fp32);
int innfer_wbc_forward(innfer_wbc_t u, const void* d_in, int in_dtype, void* d_out, int out_dtype,
                       int N, int H, int W, void* d_workspace, size_t workspace_bytes, void* stream);
/* (124, additive) The forward's two pass kernels one launch at a time, for tests: the launch functions it calls (csrc/wbcunet.hip wb_pre_launch / wb_upadd_launch,
 * csrc/f32ops.hip f32_upadd_launch).  Device pointers; no network object is needed.
 * innfer_wbc_pre: NCHW [N][C][H][W] (fp16 | fp32, rounded to nearest even) -> the row-patch slab [N * H * W][32] of the first 7x7 conv: channel kx * C + c of pixel (y, x)
 *   holds in[c][y][x + kx - 3], zero outside the row and in channels 7 C .. 31.  Refused: 7 C > 32 (INNFER_ERR_UNSUPPORTED).
 * innfer_wbc_upadd: out[2h x 2w] = up2x(in[h x w]) + skip.  tf_mode 0: F.interpolate(scale_factor=2, 'bilinear', align_corners=False); 1: tf_2xupsample_bilinear
 *   (WBCNet_arch.py:126-137).  INNFER_F16: blocked slabs [C / 32][N * pixels][32], C = 32 | 64 (wb_upadd; the upsampled value is rounded to fp16 before the add);
 *   INNFER_F32: NCHW fp32 (f32_upadd_launch, any C).
 * Refused with nothing launched (INNFER_ERR_INVALID): a null pointer, a size below 1, a dtype or tf_mode outside the above, a slab C other than 32 | 64. */
int innfer_wbc_pre(const void* d_in, int in_dtype, int N, int C, int H, int W, void* d_slab, void* stream);
int innfer_wbc_upadd(const void* d_in, const void* d_skip, int dtype, int N, int C, int h, int w, int tf_mode, void* d_out, void* stream);
/* d_x (guidance), d_y (input), d_out: [N,C,H,W] tensors of one dtype (f16/f32); means over 3x3 windows, reflect padding. */
size_t innfer_guided_filter_workspace_bytes(int N, int C, int H, int W);
int innfer_guided_filter(const void* d_x, const void* d_y, int dtype, int N, int C, int H, int W, float eps, void* d_out,
                         void* d_workspace, size_t workspace_bytes, void* stream);
/* guided_filter with a ks x ks window (ks = 2 r + 1, odd) and, when d_x_hr is not null, its 'fast' mode (utils/utils.py:548-626): A and b of
 * the [N,C,H,W] pair are enlarged to [N,C,Hh,Wh] (bilinear, align_corners=True) and applied to the high-resolution guidance d_x_hr; d_out then is
 * [N,C,Hh,Wh].  Same workspace as innfer_guided_filter.  (104) */
int innfer_guided_filter_ex(const void* d_x, const void* d_y, int dtype, int N, int C, int H, int W, int ks, float eps,
                            const void* d_x_hr, int Hh, int Wh, void* d_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* filter2D (utils/utils.py:484-535): every [H,W] plane of d_x (planes = B*C, f16 / f32) cross-correlated with one kH x kW fp32 kernel in device memory
 * behind F.pad(x, (pad_left, kW-1-pad_left, pad_top, kH-1-pad_top), mode); border 0 constant / 1 reflect / 2 replicate / 3 circular.  (104) */
int innfer_filter2d(const void* d_x, int dtype, long planes, int H, int W, const float* d_kernel, int kH, int kW, int pad_left, int pad_top,
                    int border, void* d_out, void* stream);

/* -------------------------------------------------- single fused convolution
 * The building block, exposed for tests: 3x3 stride-1 zero-pad-1 convolution
 * over an fp16 "blocked NHWC" channel slab (conv_block, block.py:213-254).
 * Slab layout: channels in groups of 32; element (n,y,x,c) lives at
 *   base + (c/32)*group_stride + ((n*H + y)*W + x)*32 + c%32   (elements; group_stride >= N*H*W*32)
 * so a 32-channel chunk of consecutive pixels is a contiguous run of full 128-byte lines and the
 * reference's torch.cat is a group offset.
 *   out[.., out_ch_off + k] = epilogue(conv(in[.., 0:C]))
 *   epilogue: +bias -> act -> (*res1_scale + res1) -> (*res2_scale + res2)
 * act: 0 none, 1 LeakyReLU(0.2) (block.py:89-90), 2 ReLU; 4 / 5: the pixel-attention gate of PAN (PAN_arch.py PA, PAConv):
 *   out = d_res1 * sigmoid(conv + bias), followed by LeakyReLU(0.2) for 4 (d_res1 required, no d_res2, scales unused);
 *   7: the pair gate of PAN's PAConv (PAN_arch.py:36-55: k3(x) * sigmoid(k2(x))) as ONE conv of K = 64 g rows that writes 32 g channels:
 *   row 16 q + r (r < 8) is value channel 8 q + r, row 16 q + 8 + r its gate -- out[8 q + r] = (conv + bias)[16 q + r] * sigmoid((conv + bias)[16 q + 8 + r])
 *   (no residuals; d_out holds K / 2 channels).
 * upsample2x: input is read through nearest-2x upsampling (block.py:321-322,358),
 *   i.e. d_in is [N,H/2,W/2,*] while H,W are the conv's (output) size.
 * d_packed comes from innfer_pack_conv3x3().  C % 32 == 0, K % 16 == 0, K <= 64 (pixel_shuffle2: K % 64 == 0, any K).
 */
typedef struct {
    const void* d_in;  int64_t in_group_stride;  /* elements between 32-channel groups of the input slab */
    int C;
    const void* d_packed; const float* d_bias;
    void* d_out; int64_t out_group_stride; int out_ch_off; int K;
    int N, H, W;
    int act; int upsample2x;
    const void* d_res1; int64_t res1_group_stride; float res1_scale;
    const void* d_res2; int64_t res2_group_stride; float res2_scale;
    int row_begin, row_end;             /* rows of the output to compute; 0,0 = all */
    int reflect_pad;                    /* != 0: nn.ReflectionPad2d(1) in front of the conv instead of zero padding (CycleGAN ResnetBlock,
                                           ResNet_arch.py:103-140); not together with upsample2x */
    int dilation;                       /* > 1: dilated 3x3 conv with zero padding = dilation (PPON's _ResBlock_32, PPON_arch.py:83-91); K == 32,
                                           no residuals / upsampling / row range */
    int dilation_groups;                /* G > 0 (<= 8): K = 32*G output channels, channel group g is the conv of dilation g+1 -- PPON's eight dilated
                                           convs as ONE launch; d_packed = the G panels of innfer_pack_conv3x3(K = 32) back to back, d_bias[32*G] */
    int pixel_shuffle2;                 /* != 0: nn.PixelShuffle(2) folded into the store (pixelshuffle_block, block.py:333-346): K % 64 == 0 conv channels,
                                           d_out is the [N,2H,2W,K/4] slab, out[n, c, 2y+i, 2x+j] = act(conv)[n, 4c+2i+j, y, x] -- a pure index map,
                                           bit-exact; act 0 / 1 / 2, residuals allowed, out_ch_off 0, no row range */
    int stride2_k4;                     /* != 0: nn.Conv2d(C, K, kernel_size=4, stride=2, padding=1) (the down convs of UnetSkipConnectionBlock, UNet_arch.py:105-106):
                                           d_in is the [N,2H,2W,C] slab, H x W the OUTPUT grid; d_packed from innfer_pack_conv4x4s2(); K % 64 == 0 (any K), act 0 / 1 / 2,
                                           no residuals / row range / out_ch_off (104) */
    int transposed2x;                   /* 3 | 4: nn.ConvTranspose2d(C, K, kernel_size=k, stride=2, padding=1, output_padding = 1 for k 3 / 0 for k 4) (UNet_arch.py:116-142,
                                           ResNet_arch.py:66-72): d_in is the [N,H,W,C] slab, d_out the [N,2H,2W,K] slab; d_packed from innfer_pack_convt2x(); d_bias holds
                                           the K biases FOUR times (one run per output phase); K % 64 == 0 (any K), act 0 / 1 / 2, no residuals / row range / out_ch_off (104) */
    int column7;                        /* != 0: nn.Conv2d(C, K, kernel_size=(7, 1), padding=(3, 0)) -- rows zero-padded, or reflected with reflect_pad (ReflectionPad2d rows):
                                           the 7x7 first convs of ResnetGenerator / UnetGeneratorWBC (ResNet_arch.py:57-60, WBCNet_arch.py:31) over their row-patch slab
                                           (channel kx * in_nc + c holds the horizontally displaced input); d_packed from innfer_pack_conv7x1(); K % 32 == 0, K <= 64,
                                           act 0 / 1 / 2, no residuals / row range / out_ch_off (104) */
    int split;                          /* != 0: the fp32-accurate form (innfer_net_set_precision): d_in / d_out / d_res1 / d_res2 are the HI slabs of (hi, lo) pairs whose
                                           lo slab = fp16((x - hi) * 2^11) lies in_lo / out_lo / res1_lo / res2_lo ELEMENTS behind; d_packed from innfer_pack_conv3x3_split();
                                           K in {32, 64} for slab outputs; act 0 / 1 / 2, residuals, upsample2x, row range and batches as for the fp16 form (106) */
    int64_t in_lo, out_lo, res1_lo, res2_lo;
    int reserved0;                      /* must be 0 (until ABI 111: `winograd`, the row-Winograd experiment of profiles/r3/winograd.txt -- measured slower, removed in 112; the
                                           field keeps the struct layout) */
    int res1_from_input;                /* != 0: d_res1 == d_in (same group stride), act 0, K = 64, C >= 96 -- the dense block's `x5 * 0.2 + x`: the residual is taken from the
                                           conv's own staged input tiles (see innfer_net_set_residual_lds); ignored when the shape does not qualify (108) */
    int plane_rows;                     /* 2 with pixel_shuffle2 (K % 256 == 0): d_packed / d_bias from innfer_pack_conv3x3_shuffle2() (110).
                                           != 0 (plain 3x3 slab convs and transposed2x with K % 64 == 0): d_packed comes from innfer_pack_conv3x3_rows(.., 1) /
                                           innfer_pack_convt2x_rows(.., 1) -- the row order in which a lane's sixteen output channels are 16 bytes in each of the group's two
                                           32-channel slab planes (what the networks use for their 64-output layers: one plane per store instruction); results are the same (109) */
    float* d_stats_part;                /* != NULL: the launch also writes the partial norm statistics of its fp32 result (bias included, before the fp16 rounding) that the
                                           pix2pix UNet and the CycleGAN ResNet take out of their convs: innfer_conv_stats_records(H, W, phases) records of (count, mean, M2)
                                           per image and channel, d_stats_part[((n * records + r) * channels + c) * 3], r = ((tile row * tile columns + tile column) [* 4 +
                                           phase]) * 8 + consumer wave -- tiles of 16 x 32 pixels of the kernel's grid (transposed2x: the input grid, 4 phases), a wave owns
                                           2 rows.  The 64-channel slab kernels without activation / residual: plain 3x3 (K % 64 == 0, any K), stride2_k4, transposed2x
                                           (lane-contiguous panels), column7 with K = 64; anything else is INNFER_ERR_UNSUPPORTED.  Merged by innfer_norm_combine_parts. (120) */
    int64_t stats_part_floats;          /* floats behind d_stats_part: at least N * records * K * 3, else INNFER_ERR_WORKSPACE (nothing is launched) (120) */
    /* (121) The remaining forms of the kernel as single launches, for tests.  Zero keeps the behaviour of 120.  None of them combines with column7 / stride2_k4 /
     * transposed2x / pixel_shuffle2 / dilation / dilation_groups / d_stats_part (INNFER_ERR_UNSUPPORTED); which other combinations exist is the launcher's decision
     * and its message (csrc/conv3x3.hip conv_launch). */
    int conv1x1;                        /* != 0: 1x1 conv; d_packed from innfer_pack_conv1x1() (with split: innfer_pack_conv1x1_split()); slab outputs, K in {32, 64};
                                           act 0 / 1 / 2 / 4 / 5, residuals, out_ch_off */
    int prefix_lrelu;                   /* != 0 (with conv1x1, K = 64): the operand of input group g is fp16(LeakyReLU(0.2)(group 0 + .. + group g)), the sums running
                                           in fp32 over the stored fp16 values (PPON's c2) */
    const void* d_gate_packed;          /* != NULL: the self gate (PAN's pixel attention behind an up-conv) -- out = act(v * sigmoid(Wg v + bg)), v = fp16(conv + bias):
                                           d_gate_packed from innfer_pack_selfgate() (Wg [32][32]), d_gate_bias 32 floats; K = 32, slab output, act 0 / 1 / 2 applied
                                           AFTER the gate, upsample2x allowed, no residuals */
    const float* d_gate_bias;
    int in_relu;                        /* != 0: the operand is max(stored input, 0) -- the planar kernel of <= 16 channels only (the UNet's outermost transposed conv) */
    int conv7x7;                        /* != 0: nn.Conv2d(C, K, 7, padding=3), zero padding or reflect_pad; d_packed from innfer_pack_conv7x7(); out_planar, K <= 16 */
    int out_planar;                     /* 1 / 2: d_out is the planar [N][K][H][W] tensor in fp16 / fp32 instead of a slab (the networks' last convs): any K <= 64
                                           (d_bias padded with zeros to a multiple of 64 floats), act 0 / 1 / 2 / 3 tanh / 6 sigmoid, out_ch_off 0, no residuals.
                                           3: d_out is the uint8 [N][H][W][K] image tensor2np makes of that result (K <= 4; BGR / BGRA byte order for K = 3 / 4) */
    int out_denorm, out_round16;        /* out_planar 3: (v + 1) / 2 before the quantisation; v rounded to fp16 first */
    int planar_phases;                  /* != 0 (out_planar 1 / 2): K = the channels of a ConvTranspose2d(C, K, 4, 2, 1) written as ONE 3x3 conv of 4 K channels over the
                                           H x W INPUT grid, channel (2 a + b) K + c = output pixel (2 y + a, 2 x + b) of channel c; d_out is [N][K][2H][2W]; d_packed from
                                           innfer_pack_conv3x3(4 K, C) over those 3x3 weights, d_bias the K biases four times; act 0 / 3 (the networks: 4 K <= 16) */
    int outm;                           /* out_planar with K <= 16: 1 (tanh + 1) / 2, 2 tanh, 3 sigmoid, 4 clamp(0, 1), applied after act */
} innfer_conv_args;

size_t innfer_conv3x3_packed_bytes(int K, int C);
int innfer_pack_conv3x3(const float* h_weight_oihw, int K, int C, void* h_packed);
int innfer_pack_conv3x3_rows(const float* h_weight_oihw, int K, int C, int plane_rows, void* h_packed);      /* (109) same size; plane_rows: see innfer_conv_args */
int innfer_pack_convt2x_rows(const float* h_weight_iohw, int K, int C, int k, int plane_rows, void* h_packed); /* (109) */
/* (110) Panels for pixel_shuffle2 with plane_rows = 2: the conv channels PHASE-MAJOR (packed channel ph * K / 4 + oc = reference channel 4 oc + ph, ph = 2a + b the position
 * in nn.PixelShuffle's 2 x 2 block) in the plane row order, so that the shuffle is the store of the producer / consumer kernel (what the networks use for their PixelShuffle(2)
 * stages on 64 features).  K % 256 == 0; same size as innfer_pack_conv3x3; h_bias_out receives the K biases in the same order (zeros when h_bias is NULL): pass it as d_bias. */
int innfer_pack_conv3x3_shuffle2(const float* h_weight_oihw, const float* h_bias, int K, int C, void* h_packed, float* h_bias_out);
/* Panels of the two stride-2 forms above: h_weight is torch's layout, [K][C][4][4] for the conv and [C][K][k][k] for the transposed conv (k = 3 | 4). (104) */
size_t innfer_conv7x1_packed_bytes(int K, int C);
int innfer_pack_conv7x1(const float* h_weight_oc7, int K, int C, void* h_packed);     /* h_weight [K][C][7] */
size_t innfer_conv4x4s2_packed_bytes(int K, int C);
int innfer_pack_conv4x4s2(const float* h_weight_oihw, int K, int C, void* h_packed);
size_t innfer_convt2x_packed_bytes(int K, int C);
int innfer_pack_convt2x(const float* h_weight_iohw, int K, int C, int k, void* h_packed);
/* (121) Panels of the forms above.  1x1: h_weight [K][C]; innfer_conv1x1_packed_bytes(K, C) bytes, the split form three times that.  Self gate: h_weight [32][32]
 * (out, in), 2048 bytes.  7x7: h_weight [K][C][7][7].  innfer_pack_up2x_phases: nearest-2x + 3x3 conv (h_weight [K][C][3][3], K % 64 == 0) as the four 2x2-tap phases of a
 * transposed conv, the taps that meet the same source pixel summed in fp32 and rounded to fp16 ONCE -- innfer_convt2x_packed_bytes(K, C) bytes that run through
 * transposed2x = 4 with the same plane_rows (d_in the [N,H,W,C] slab, d_out the [N,2H,2W,K] slab, d_bias the K biases four times). */
size_t innfer_conv1x1_packed_bytes(int K, int C);
int innfer_pack_conv1x1(const float* h_weight_oi, int K, int C, void* h_packed);
int innfer_pack_conv1x1_split(const float* h_weight_oi, int K, int C, void* h_packed);
int innfer_pack_selfgate(const float* h_weight_32x32, void* h_packed_2k);
size_t innfer_conv7x7_packed_bytes(int K, int C);
int innfer_pack_conv7x7(const float* h_weight_oihw, int K, int C, void* h_packed);
int innfer_pack_up2x_phases(const float* h_weight_oihw, int K, int C, int plane_rows, void* h_packed);
int innfer_conv3x3_f16(const innfer_conv_args* a, void* stream);
/* a->act = 9 (SiLU): f * sigmoid(f); a->act = 10 (the gate that ends a SPAB block of SPAN): (f + res1) * (sigmoid(f) - 0.5) with d_res1 the block's input in the
 * output's slab layout (res1_scale unused; no d_res2) -- fp32 on the accumulator + bias with the hardware exponential / reciprocal, one fp16 rounding at the store.
 * Built like act 8: epilogues of the plain 3x3 slab convs with K = 64 (plane_rows 0 / 1) and K = 32, batches, row ranges and out_ch_off included; every other form (split,
 * d_stats_part, the self gate, conv1x1, out_planar, the stride-2 / phase / column / dilated forms, upsample2x, reflect_pad, d_res2, act 9 with d_res1) answers
 * INNFER_ERR_UNSUPPORTED and act 10 without d_res1 INNFER_ERR_INVALID; nothing is launched. */
/* a->act = 11 (Mish): f * tanh(softplus(f)) as f * w / (w + 2), w = n (n + 2), n = e^min(f, 20) -- fp32 on the accumulator + bias, one hardware exponential and one
 * reciprocal per value, f itself for large f, one fp16 rounding at the store.  An epilogue of the plain 3x3 slab conv with K = 64 (plane_rows 0 / 1), batches, row ranges
 * and out_ch_off included; every other form (K = 32, split, d_stats_part, the self gate, conv1x1, out_planar, the stride-2 / phase / column / dilated forms, residuals,
 * upsample2x, reflect_pad) answers INNFER_ERR_UNSUPPORTED; nothing is launched. */
/* (123, additive) a->act = 12 (GELU, the exact form): f (1 + erf(f / sqrt 2)) / 2 with erfc from Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7), as f - h above zero and
 * -h below, h = |f| erfc(|f| / sqrt 2) / 2 -- fp32 on the accumulator + bias, one hardware exponential and one reciprocal per value, f itself (or -0) for large |f|, one
 * fp16 rounding at the store.  An epilogue of the conv1x1 slab conv with K = 64, batches, row ranges and whole-group out_ch_off included; every other form (3x3, K = 32,
 * split, d_stats_part, prefix_lrelu, out_planar, the stride-2 / phase / column / dilated forms, residuals, upsample2x, reflect_pad) answers INNFER_ERR_UNSUPPORTED;
 * nothing is launched. */
/* (123, additive) a->act = 13: the same GELU as the epilogue of the plain 3x3 slab conv with K = 64 (plane_rows 0), batches, row ranges and whole-group out_ch_off included
 * (HAT's conv block); every other form (conv1x1 -- that is act 12 --, K = 32, plane_rows, split, d_stats_part, the self gate, out_planar, the stride-2 / phase / column /
 * dilated forms, residuals, upsample2x, reflect_pad) answers INNFER_ERR_UNSUPPORTED; nothing is launched. */
/* (123, additive) RealPLKSR's partial large-kernel conv as a single launch (for tests; csrc/plk_conv.hip): d_in / d_out point at channel 0 of two DIFFERENT 32-channel
 * slab groups of N * H * W pixels; out channels 0 .. 15 = the k x k zero-padded conv (h_weight_oihw [16][16][k][k], h_bias 16 floats or NULL; k odd, 3 .. 17) of in channels
 * 0 .. 15 -- fp16 operands, fp32 accumulation, one rounding --, out channels 16 .. 31 = in channels 16 .. 31 bit for bit.  Overlapping groups are INNFER_ERR_INVALID
 * (other workgroups still read the halo); nothing is launched then.  Uploads, launches, waits. */
int innfer_plk_conv(const void* d_in, void* d_out, int N, int H, int W, int k, const float* h_weight_oihw, const float* h_bias, void* stream);
/* (123, additive) GroupNorm(groups, 64) per sample + skip over 64-channel slabs as the network runs it (for tests; csrc/group_norm.hip: statistics, merge, apply):
 * d_out = fp16(alpha[n][c] * u + shift[n][c] + skip), alpha = h_gamma[c] / sqrt(var + eps), shift = h_beta[c] - mean alpha, mean / biased variance over the
 * (64 / groups) x HW values of image n's group.  *_gs: group strides in elements; d_out may be d_skip.  groups in {1, 2, 4, 8}.  d_work: at least
 * innfer_group_norm_skip_work_bytes(N, HW) bytes.  Uploads gamma / beta, launches, waits. */
size_t innfer_group_norm_skip_work_bytes(int N, int64_t HW);
int innfer_group_norm_skip(const void* d_u, int64_t u_gs, const void* d_skip, int64_t skip_gs, void* d_out, int64_t out_gs, int N, int64_t HW, int groups,
                           const float* h_gamma, const float* h_beta, float eps, void* d_work, size_t work_bytes, void* stream);
/* The same launch with the per-channel slope activation: a->act = 8 computes f >= 0 ? f : d_slope[c] * f (nn.PReLU; d_slope: device floats padded like d_bias and
 * indexed by the same channel, whatever plane_rows / out_ch_off).  Built as the epilogue of the plain 3x3 slab convs with K = 64 (plane_rows 0 / 1) and K = 32, row
 * ranges and batches included; every other form (split, d_stats_part, the self gate, conv1x1, out_planar, the stride-2 / phase / column / dilated forms, residuals,
 * upsample2x, reflect_pad) answers INNFER_ERR_UNSUPPORTED and act 8 without d_slope -- innfer_conv3x3_f16 included -- INNFER_ERR_INVALID; nothing is launched. */
int innfer_conv3x3_f16_slope(const innfer_conv_args* a, const float* d_slope, void* stream);
/* The same launch with the consumer-wave grid chosen (for tests and A/B runs; see innfer_net_set_consumer_grid): consumer_grid 1 = what innfer_conv3x3_f16 does -- the plain
 * and the res1_from_input 3x3 slab conv with K = 64 and plane_rows = 1 runs on the 2 x 4 grid with its memory residual prefetched (single images, and batches that are
 * not laid out as an image canvas); 0 = the 8 x 1 form everywhere.  Every other launch ignores it.  Results are bit-identical. */
int innfer_conv3x3_f16_grid(const innfer_conv_args* a, int consumer_grid, void* stream);
/* SRVGGNetCompact's tail as a single launch (for tests): d_out = PixelShuffle(scale)(slab) + nearest_upsample(base, scale).  d_slab: fp16 blocked slab of N x H x W
 * pixels whose first C scale^2 channels are the conv result (channel c s^2 + a s + b -> output channel c at (s y + a, s x + b)); d_base: planar fp16 [N][C][H][W]
 * (INNFER_F16) or N uint8 HWC BGR(A) images (INNFER_U8: np2tensor with `normalize`, rounded to fp16); d_out: planar fp16 / fp32 [N][C][sH][sW], or N uint8 HWC BGR(A)
 * images (tensor2np of the fp16 result, denormalize = `normalize`).  r = fp16(float(slab) + float(base)): one fp32 add, one rounding.  C 1 .. 4, scale 1 .. 4. */
/* d_base == NULL: no base -- d_out = PixelShuffle(scale)(slab) alone, the same three stores (SPAN's tail); base_dtype is then ignored. */
int innfer_shuffle_add(const void* d_slab, int64_t group_stride, const void* d_base, int base_dtype, int normalize, void* d_out, int out_dtype,
                       int N, int C, int H, int W, int scale, void* stream);
/* Panels of the split form: 3 * innfer_conv3x3_packed_bytes(K, C) bytes ((w - wh) * 2^11 | wh | wh, in the order the kernel's virtual chunks meet them).  (106) */
int innfer_pack_conv3x3_split(const float* h_weight_oihw, int K, int C, void* h_packed);

/* (114) The generic fp32 convolution and normalisation of the fp32 mode (csrc/f32ops.hip: the -no_fp16 forwards of pix2pix UNet, CycleGAN ResNet, WBC UNet, PPON
 * and PAN's fp32 convs) as single launches, for tests.  The fields are csrc/common.h F32Conv's (see there), device pointers, NCHW fp32 views:
 *   out[n][k][Y][X] = epilogue(bias[k] + sum_{tap, c} w[k][c][tap] * in_act(in[n][c][oy * isy + dy[tap]][ox * isx + dx[tap]])),  (Y, X) = (oy * osy + ooy, ox * osx + oox)
 * form: 0 the kernel the networks get for this view (the planner's choice), 1 the direct (large-view) kernel whatever the plan.
 * d_packed from innfer_pack_f32conv (h_w [K][C][ntap]; innfer_f32conv_packed_floats(K, C, ntap) floats). */
typedef struct {
    const float* d_in; int64_t in_nstride, in_cstride; int C, Hin, Win;
    const float* d_packed; const float* d_bias; int K;
    float* d_out; int64_t out_nstride, out_cstride, out_pstride; int Wout;
    int Ho, Wo;
    int osy, osx, ooy, oox;
    int isy, isx;
    int ntap, dy[49], dx[49];
    int pad_mode;                       /* 0 zero, 1 reflect, 2 replicate */
    int up;                             /* taps walk the nearest-2x upsampled input */
    int in_act;                         /* 0 / 1 LeakyReLU(0.2) / 2 ReLU on the input */
    int act;                            /* 0 none, 1 LeakyReLU(0.2), 2 ReLU, 3 tanh, 4 sigmoid */
    float oscale;
    const float* d_res; int64_t res_nstride, res_cstride;
    const float* d_mul; int64_t mul_nstride, mul_cstride;
    int N;
    int phase_k;
    int form;
} innfer_f32conv_args;

size_t innfer_f32conv_packed_floats(int K, int C, int ntap);
int innfer_pack_f32conv(const float* h_w, int K, int C, int ntap, float* h_packed);
int innfer_f32conv(const innfer_f32conv_args* a, void* stream);
/* Host only (no device call): what innfer_f32conv would launch.  plan[8] = {direct, NKT, NPT, IMG, CC, vec4, workgroups, LDS bytes}; the direct kernel reports
 * NKT = NPT = IMG = CC = vec4 = 0 and LDS 0. */
int innfer_f32conv_plan(const innfer_f32conv_args* a, int* plan);
/* Per-(image, channel) plane normalisation (f32_norm_launch): mode 0 batch statistics + affine, 1 running statistics + affine, 2 instance norm, 3 y = x * weight + bias;
 * then act (as above), then + res.  form: 0 the kernel the networks get for this plane size, 1 the three-pass kernel. */
int innfer_f32_norm(const float* d_in, int64_t in_ns, int64_t in_cs, float* d_out, int64_t out_ns, int64_t out_cs, int N, int C, int64_t HW, int mode, float eps,
                    const float* d_weight, const float* d_bias, const float* d_rmean, const float* d_rvar, int act,
                    const float* d_res, int64_t res_ns, int64_t res_cs, int form, void* stream);
/* (124, additive) Two more passes of the fp32 mode as single launches, for tests (csrc/f32ops.hip f32_prefix_lrelu_launch / f32_act_copy_launch, as PPON's and the UNet's
 * fp32 forwards call them).  Device pointers; no network object is needed.
 * innfer_f32_prefix_lrelu: d_t fp32 [N][groups * gc][hw], IN PLACE: channel c of group k becomes LeakyReLU(0.2)(group 0 + .. + group k), the sums formed in group order.
 * innfer_f32_act_copy: d_out[n * out_ns + r] = act(d_in[n * in_ns + r]), r < per_image, n < N; act 0 none, 1 LeakyReLU(0.2), 2 ReLU, 3 tanh, 4 sigmoid.
 * Refused with nothing launched (INNFER_ERR_INVALID): a null pointer, a size below 1, an image stride below per_image, an act outside 0 .. 4. */
int innfer_f32_prefix_lrelu(float* d_t, int N, int groups, int gc, int64_t hw, void* stream);
int innfer_f32_act_copy(const float* d_in, int64_t in_ns, float* d_out, int64_t out_ns, int64_t per_image, int N, int act, void* stream);

/* (120) The norm statistics of the fp16 engine (csrc/norm_stats.h; train-mode BatchNorm2d of the pix2pix UNet, InstanceNorm2d of the CycleGAN ResNet) as single
 * launches, for tests.  alpha / shift: [N][C] floats with  norm(x) = x * alpha + shift,  alpha = gamma / sqrt(var + eps), shift = beta - mean * alpha  (biased variance
 * per image and channel; d_gamma / d_beta [C] or NULL for 1 / 0).  All pointers are device pointers.
 * innfer_conv_stats_records: host only -- the records per image (and channel) a conv with d_stats_part writes for an H x W grid with `phases` (1 | 4) phases.
 * innfer_norm_combine_parts: merges the records d_part[N][nper][C][3] of such a conv (Chan's update, fixed order).
 * innfer_norm_stats: the re-read forms -- slab 0: d_src is fp32 [N][HW][cpad] (norm::launch_stats), slab != 0: d_src is an fp16 slab of group stride `gs` elements
 * (norm::launch_stats_slab; cpad unused).  d_part: scratch of part_floats >= N * C * ceil(HW / 1024) * 2 floats when HW > 1024 (else INNFER_ERR_WORKSPACE).
 * innfer_resnet_post_slab_parts / innfer_unet_post_slab_parts: merge + normalisation + activation in one launch, as the two networks run them behind such a conv
 *   (rn_post_slab_parts / unet_post_slab_parts), on the grid the networks choose; eps is the networks' 1e-5.  C % 32 == 0.
 *   resnet: d_dst = [relu](x * alpha + shift) [+ d_res]; d_src, d_res, d_dst are slabs of one group stride gs.
 *   unet: d_dst0 (group stride dst0_gs, channel offset dst0_coff % 8 == 0, act0 1 LeakyReLU(0.2) | 2 ReLU) and, when d_dst1 is not NULL, the same for d_dst1. */
int innfer_conv_stats_records(int H, int W, int phases);
int innfer_norm_combine_parts(const float* d_part, int nper, int64_t HW, float eps, const float* d_gamma, const float* d_beta, float* d_alpha, float* d_shift,
                              int C, int N, void* stream);
int innfer_norm_stats(const void* d_src, int slab, int64_t gs, int cpad, int64_t HW, float eps, const float* d_gamma, const float* d_beta, float* d_alpha, float* d_shift,
                      int C, int N, float* d_part, int64_t part_floats, void* stream);
int innfer_resnet_post_slab_parts(const void* d_src, int64_t gs, int C, int64_t HW, int N, const float* d_part, int nper, const float* d_gamma, const float* d_beta,
                                  int relu, const void* d_res, void* d_dst, void* stream);
int innfer_unet_post_slab_parts(const void* d_src, int64_t src_gs, int C, int64_t HW, int N, const float* d_part, int nper, const float* d_gamma, const float* d_beta,
                                void* d_dst0, int64_t dst0_gs, int dst0_coff, int act0, void* d_dst1, int64_t dst1_gs, int dst1_coff, int act1, void* stream);

/* (123) The pass kernels that carry the pix2pix UNet (csrc/unet.hip) and the CycleGAN ResNet (csrc/resnet.hip) from one conv to the next, as single launches, for tests.
 * Every entry checks its arguments and then calls the launcher the network calls (grid, block and instantiation are the network's); on a refusal (INNFER_ERR_INVALID /
 * INNFER_ERR_UNSUPPORTED, innfer_last_error says why) nothing is launched.  All pointers are device pointers but h_w / h_packed.  Slabs are blocked-NHWC fp16 with
 * 32-channel groups `gs` elements apart (gs >= pixels * 32); a destination view is (pointer, group stride, channel offset % 8 == 0, act 1 LeakyReLU(0.2) | 2 ReLU).
 * innfer_unet_pre: NCHW (in_dtype INNFER_F16 | INNFER_F32) -> one zero-padded group (patch 0; C <= 32), or -> the 64-channel patch slab of the 4x4 stride-2 window at
 *   half resolution, channel (ky * 4 + kx) * C + c, zero outside the image (patch 1; 16 * C <= 64, H and W even, gs = group stride of the two groups).
 * innfer_unet_post / innfer_unet_post_slab: fp32 rows [N * HW][cpad] / an fp16 slab -> act(x * alpha + shift) into one or two views (d_dst1 may be NULL); alpha / shift
 *   [N][C] (nstride = C) or [C] (nstride = 0); innfer_unet_post takes d_alpha = d_shift = NULL for act(x).  C % 8 == 0, cpad % 4 == 0.
 * innfer_unet_deep_post: d_part = ks segments, split_elems floats apart, of fp32 rows [N * HW][cpad]; their sum in segment order -> train-mode BatchNorm of each image
 *   (d_gamma, d_beta; eps 1e-5) | y = x * ev_alpha + ev_shift | x -> one or two views.  HW <= 256 (INNFER_ERR_UNSUPPORTED beyond); the kernel instantiation follows HW.
 * innfer_unet_final / innfer_resnet_final: tanh(raw[.., c] + bias[c]) -> NCHW (out_dtype INNFER_F16 | INNFER_F32); rows of cpad / rs >= C floats.
 * innfer_pack_unet_first: h_w [64][C][4][4] -> the 8192-byte panel (innfer_unet_first_packed_bytes) of innfer_unet_first_conv: Conv2d(C, 64, 4, 2, 1) [+ bias] straight
 *   from the NCHW input; d_dst0 = LeakyReLU(0.2), d_dst1 (may be NULL) = ReLU, two-group slabs at half resolution.  16 * C <= 64, H and W even, (W / 2) % 16 == 0
 *   (INNFER_ERR_UNSUPPORTED otherwise: the kernel walks 16-pixel segments), C * H * W < 2^31 - 1.
 * innfer_resnet_pre: NCHW -> one zero-padded group (patch 0) or the row-patch slab, channel kx * C + c = in[c][y][reflect(x + kx - 3)] (patch 1; 7 * C <= 32, H, W >= 4).
 * innfer_resnet_post / innfer_resnet_post_slab: [relu](x * alpha + shift) [+ d_res]; alpha / shift [N][C]; source fp32 rows / a slab of the destination's group stride
 *   (d_dst may be d_src for the slab form).  C % 8 == 0.
 * innfer_resnet_post_slab_pad: the same (no residual) into the (H + 8) x (W + 8) slab of ReflectionPad2d(3) plus one ring of zeros, image at (4, 4): the zero-ring
 *   launch and the pass, as the network issues them.  C % 32 == 0, H, W >= 4.
 * innfer_resnet_sum9_tanh: Q planar fp32 [N][9 K][H + 8][W + 8] -> out[n][k][y][x] = tanh(bias[k] + sum over (sr, sc) of Q[n][9 k + 3 sr + sc][y + 3 sr + 1][x + 3 sc + 1]). */
int innfer_unet_pre(const void* d_in, int in_dtype, int C, int H, int W, int N, void* d_slab, int64_t gs, int patch, void* stream);
int innfer_unet_post(const float* d_raw, int cpad, int C, int64_t HW, int N, const float* d_alpha, const float* d_shift, int nstride,
                     void* d_dst0, int64_t dst0_gs, int dst0_coff, int act0, void* d_dst1, int64_t dst1_gs, int dst1_coff, int act1, void* stream);
int innfer_unet_post_slab(const void* d_src, int64_t src_gs, int C, int64_t HW, int N, const float* d_alpha, const float* d_shift, int nstride,
                          void* d_dst0, int64_t dst0_gs, int dst0_coff, int act0, void* d_dst1, int64_t dst1_gs, int dst1_coff, int act1, void* stream);
int innfer_unet_deep_post(const float* d_part, int64_t split_elems, int ks, int cpad, int C, int HW, int N, const float* d_gamma, const float* d_beta,
                          const float* d_ev_alpha, const float* d_ev_shift, void* d_dst0, int64_t dst0_gs, int dst0_coff, int act0,
                          void* d_dst1, int64_t dst1_gs, int dst1_coff, int act1, void* stream);
int innfer_unet_final(const float* d_raw, int cpad, int C, int64_t HW, int N, const float* d_bias, void* d_out, int out_dtype, void* stream);
size_t innfer_unet_first_packed_bytes(void);
int innfer_pack_unet_first(const float* h_w, int C, void* h_packed);
int innfer_unet_first_conv(const void* d_in, int in_dtype, int C, int H, int W, int N, const void* d_packed, const float* d_bias, void* d_dst0, void* d_dst1, int64_t gs,
                           void* stream);
int innfer_resnet_pre(const void* d_in, int in_dtype, int C, int H, int W, int N, void* d_slab, int patch, void* stream);
int innfer_resnet_post(const float* d_raw, int cpad, int C, int64_t HW, int N, const float* d_alpha, const float* d_shift, int relu, const void* d_res, void* d_dst,
                       int64_t gs, void* stream);
int innfer_resnet_post_slab(const void* d_src, int C, int64_t HW, int N, const float* d_alpha, const float* d_shift, int relu, const void* d_res, void* d_dst, int64_t gs,
                            void* stream);
int innfer_resnet_post_slab_pad(const void* d_src, int64_t src_gs, int C, int H, int W, int N, const float* d_alpha, const float* d_shift, int relu, void* d_dst,
                                int64_t dst_gs, void* stream);
int innfer_resnet_sum9_tanh(const float* d_q, const float* d_bias, void* d_out, int out_dtype, int K, int H, int W, int N, void* stream);
int innfer_resnet_final(const float* d_raw, int rs, int C, int64_t HW, int N, const float* d_bias, void* d_out, int out_dtype, void* stream);

/* (122) The gather GEMM (csrc/gather_gemm.h gg::gemm_gather: the second conv engine -- the pix2pix UNet's deep levels, every conv of the CycleGAN ResNet, the WBC UNet,
 * PPON's fallback dilated convs and c2, PAN's attention projections) as a single launch, for tests.  The struct carries what gg::launch takes, and the entry runs the
 * decision code of the five families (gg::decide) before it fires (gg::fire):
 *   raw[n, oy * os + ooy, ox * os + oox, co] = sum over taps t and input channels ci of in[n, oy * stride + dy[t] * m, ox * stride + dx[t] * m, ci] * w[co, ci, t]
 * in fp32 over fp16 operands; m = 1 + g * g_tapmul is group g's tap multiplier; out-of-image taps read zero, or the mirrored pixel with reflect; with up the input is
 * read through nearest 2x (Hin, Win = the source size).  d_in: blocked-NHWC fp16 slab, 32-channel chunks in_group_stride elements apart; d_raw: fp32 rows of raw_stride
 * floats per pixel of the N x Hfull x Wfull grid (0 = cout_pad; a positive multiple of 4), of which channels [0, cout_store) are written (0 = min(raw_stride, cout_pad)).
 * ngroup > 1: several convs of the same input as one launch -- weights d_packed + g * g_wbytes BYTES, output d_raw + g * g_outoff FLOATS.  g_phase (ngroup == 4, os == 2,
 * ntaps <= 12): group g uses taps [g * ntaps, (g + 1) * ntaps) of dy / dx and writes output pixel (2 oy + (g >> 1), 2 ox + (g & 1)); ooy / oox unused.
 * d_scratch / scratch_bytes (optional): where the layer's geometry asks for a split over K and the partial results fit, the launch writes ksplit partial results of
 * N * Hfull * Wfull * raw_stride floats each into d_scratch and reduces them into d_raw in split order; with keep_partials they stay in d_scratch unreduced (d_raw is
 * not written), as the UNet's deep levels use the launch.  The in-call reduction covers channels [0, cout_store) only, so a raw row wider than cout_store (several
 * GEMMs filling one row) keeps its other columns when the launch is split (until 121 it ran over the whole row: unwritten scratch stored over the neighbours' columns;
 * no network formed that launch).
 * Refused, with nothing launched: raw_stride not a positive multiple of 4, ntaps outside 1 .. 49, g_phase without 4 groups of <= 12 taps (INNFER_ERR_INVALID), an input
 * of N * Hin * Win * 64 >= 2^31 - 1 bytes per chunk (INNFER_ERR_UNSUPPORTED) -- as gg::launch refuses them -- and, by this entry only: cout_store not a multiple of 4 or
 * beyond raw_stride (INNFER_ERR_INVALID); reflect with a tap that one reflection does not bring back into the image (|dy| * m >= Hin for a stride-1 same-size conv),
 * reflect together with up or g_phase (INNFER_ERR_UNSUPPORTED).
 * info[5] (may be NULL for innfer_gather_gemm) = {tile shape (0: 128 px x 64 co, 1: 256 x 128, 2: 256 x 256 on eight waves), ksplit, seg (k-steps per segment), taps kept
 * per group after the dead-tap drop, scratch bytes a split of this layer needs (0: never split)}.  innfer_gather_gemm_plan: host only, no device call, pointers unread
 * (d_scratch only compared with NULL).
 * Panels: h_w [cout][cin][ntaps] float32 -> innfer_gather_gemm_packed_bytes(cout, cin_pad, ntaps) bytes through gg::pack_panels, the packer of every family: cout_pad =
 * ceil(cout / 64) * 64 rows, cin_pad % 32 == 0, padding zero; [channel tile][tap][chunk][64 rows][4 slots of 8], slot s of row R = channels 8 * (s ^ 2 * bit2(R)) .. + 7. */
typedef struct {
    const void* d_in; int64_t in_group_stride; int cin_pad;
    const void* d_packed; int cout_pad;
    float* d_raw; int raw_stride, cout_store;
    int N, Hin, Win, Ho, Wo, stride;
    int ntaps, dy[49], dx[49];
    int Hfull, Wfull, os, ooy, oox, up, reflect;
    int ngroup; int64_t g_wbytes, g_outoff; int g_tapmul, g_phase;
    float* d_scratch; int64_t scratch_bytes;
    int keep_partials;
} innfer_gather_gemm_args;
size_t innfer_gather_gemm_packed_bytes(int cout, int cin_pad, int ntaps);
int innfer_pack_gather_gemm(const float* h_w, int cout, int cin, int cin_pad, int ntaps, void* h_packed);
int innfer_gather_gemm(const innfer_gather_gemm_args* a, int* info, void* stream);
int innfer_gather_gemm_plan(const innfer_gather_gemm_args* a, int* info);

/* NCHW (f16/f32) <-> blocked-NHWC f16 slab helpers used by tests of the single conv. */
int innfer_nchw_to_slab(const void* d_src, int src_dtype, void* d_slab, int64_t group_stride, int ch_off,
                        int N, int C, int H, int W, void* stream);
int innfer_slab_to_nchw(const void* d_slab, int64_t group_stride, int ch_off, void* d_dst, int dst_dtype,
                        int N, int C, int H, int W, void* stream);
/* The same for the (hi, lo) slab pairs of the fp32-accurate mode: fp32 NCHW -> hi slab at d_slab, lo slab `lo` elements behind it, and back
 * (hi + lo * 2^-11, exact in fp32).  (106) */
int innfer_nchw_to_slab_split(const float* d_src, void* d_slab, int64_t group_stride, int64_t lo, int ch_off, int N, int C, int H, int W, void* stream);
int innfer_slab_split_to_nchw(const void* d_slab, int64_t group_stride, int64_t lo, int ch_off, float* d_dst, int N, int C, int H, int W, void* stream);

/* ------------------------------------------------------------ launch timer (measurement only)
 * Between innfer_timer_start() and innfer_timer_stop() every kernel launch the calling thread makes through the library's conv / gather-GEMM / UNet
 * entry points is bracketed by a HIP-event pair on its stream.  innfer_timer_stop synchronises `stream` and returns, per launch in issue order, a
 * kernel-family name (names[i * name_cap ..], NUL-terminated), the elapsed ms, and the launch's ALGORITHMIC flops and HBM bytes (operands read once,
 * results written once; 0 where a family has none).  n receives the number of launches recorded (entries beyond cap are dropped).  bench.py builds
 * the per-kernel two-roof entries of its `unet64` object from it.  (106) */
int innfer_timer_start(void);
int innfer_timer_stop(void* stream, int cap, char* names, int name_cap, float* h_ms, double* h_flops, double* h_bytes, int* n);

/* ------------------------------------------------------------ chop / blend
 * Replaces extract_patches_2d / recompose_tensor (utils/utils.py:318-369,
 * 372-445) as used by Model.chop_forward (run.py:167-202).
 */

/* Geometry only (host).  ps = min(H,W,patch); origins are the row-major tile
 * lattice of stride int(ps*step) plus one ragged row/column anchored at H-ps /
 * W-ps.  ys/xs may be NULL to query counts.  Capacity: nh<=H, nw<=W. */
int innfer_chop_plan(int H, int W, int patch, double step, int* ps, int* nh, int* nw,
                     int* ys, int* xs);

/* d_img [B,C,H,W] -> d_tiles [nh*nw*?..]: tiles[(b? see below)]
 * Output order matches extract_patches_2d(batch_first=True).squeeze(0) for B=1:
 * d_tiles [n, C, ps, ps], n = nh*nw row-major.  tile_begin/tile_count select a
 * contiguous sub-range (multi-GPU sharding). */
int innfer_extract_tiles(const void* d_img, int dtype, int C, int H, int W, int patch, double step,
                         int tile_begin, int tile_count, void* d_tiles, void* stream);

/* 1-D blending profile (utils.py:396,413-416), host, fp32, length P. */
int innfer_blend_profile(int P, double step, int scale, float* h_profile);

/* recompose_tensor: d_tiles [n,C,P,P] (HR tiles, row-major over the tile
 * lattice) -> d_out [1,C,scale*height,scale*width].  Accumulates in fp32 in
 * the reference's (h,w) order: with fp32 tiles the result is bit-identical to
 * the reference's fp32 path. */
int innfer_recompose(const void* d_tiles, int dtype, int n, int C, int P, int height, int width,
                     double step, int scale, void* d_out, int out_dtype, void* stream);

/* ------------------------------------------------------------ multi-GPU chop (RCCL over xGMI)
 * The reference is single-process; what shards is chop_forward's tile list (run.py:186-197: every tile's forward is independent) and the
 * one exchange is "raw HR tiles -> rank 0" in front of recompose_tensor (utils/utils.py:372-445), plus the broadcast of the blended
 * intermediate between the models of a chain (run.py:424-426).  One process per GPU; the calls below are collective over the ranks of a
 * communicator.  RCCL (librccl.so.1) is bound at run time, on the first of these calls: single-GPU users never load it.
 */
#define INNFER_COMM_ID_BYTES 128
typedef struct innfer_comm* innfer_comm_t;

/* Host geometry: rank's contiguous share [first, first+count) of the row-major tile list, split as evenly as possible (earlier ranks take
 * the remainder: 798 tiles over 8 ranks -> 100 x 6, 99 x 2).  Use it with innfer_extract_tiles(tile_begin, tile_count). */
int innfer_shard_tiles(int n_tiles, int nranks, int rank, int* first, int* count);

/* ncclGetUniqueId on ONE rank; the caller ships the INNFER_COMM_ID_BYTES to the other ranks by its own means (file, socket, MPI, torch store). */
int innfer_comm_unique_id(void* h_id);
/* ncclCommInitRank on the calling thread's current HIP device. */
int innfer_comm_init(innfer_comm_t* out, const void* h_id, int rank, int nranks);
void innfer_comm_destroy(innfer_comm_t c);
int innfer_comm_rank(innfer_comm_t c);
int innfer_comm_size(innfer_comm_t c);

/* Collect every rank's tiles on rank 0, real tiles only.  Rank 0: d_tiles is the whole [n_tiles][tile_bytes] buffer the blend reads, with
 * its own share already in place; rank r > 0: d_tiles is its own share [count][tile_bytes] (innfer_shard_tiles).  One group of ncclSend /
 * ncclRecv enqueued on `stream`; the buffer may be read by work enqueued on `stream` after the call. */
int innfer_gather_tiles(innfer_comm_t c, void* d_tiles, size_t tile_bytes, int n_tiles, void* stream);
/* ncclBroadcast of `bytes` bytes from `root` (the blended intermediate of a model chain), in place. */
int innfer_comm_broadcast(innfer_comm_t c, void* d_buf, size_t bytes, int root, void* stream);

/* --------------------------------------------------------------- pre / post
 * np2tensor / tensor2np (utils/utils.py:164-194,197-248, colors.py:5-26):
 * uint8 HWC BGR(A) <-> float NCHW RGB(A), /255, optional [-1,1] (de)normalise,
 * clip*255 and round-half-to-even on the way back.
 */
int innfer_u8hwc_to_nchw(const uint8_t* d_img, int H, int W, int C, int normalize,
                         void* d_out, int out_dtype, void* stream);
int innfer_nchw_to_u8hwc(const void* d_in, int in_dtype, int H, int W, int C, int denormalize,
                         uint8_t* d_img, void* stream);
/* The same with the remaining arguments of np2tensor / tensor2np (104).  bits: 8 or 16 (uint8 / uint16 image, MAX_VALUES_BY_DTYPE
 * utils.py:22-33); maxval: what the image is divided by (255, 65535; 1 = change_range False); bgr2rgb / rgb2bgr = 0 keeps the channel order.
 * innfer_nchw_to_inthwc scales by the data_range that goes with the type (255 / 65535), clips and rounds half to even. */
/* The chop path with uint8 images at both ends (104): extract_patches_2d(np2tensor(img)) and tensor2np(recompose_tensor(tiles)) without the
 * float image in between -- the tile gather converts (same /255, flip, normalisation, cast to the tile dtype), the blend stores uint8 HWC
 * BGR(A) (the blended value is first rounded to via_dtype, the dtype recompose_tensor would have returned).  One image; same geometry and
 * arithmetic as innfer_extract_tiles / innfer_recompose, bit-identical to the separate passes.  They are innfer_extract_tiles_u8_seamless at
 * pad = 0 and innfer_recompose_u8_seamless at crop = 0 (117, below): one gather and one blend kernel serve every uint8 chop entry point.  The
 * gather takes any C >= 1 (3 n channels are fully flipped, 4 is [2, 1, 0, 3]), the blend C 1 .. 4. */
int innfer_extract_tiles_u8(const uint8_t* d_img, int C, int H, int W, int normalize, int patch, double step,
                            int tile_begin, int tile_count, void* d_tiles, int tile_dtype, void* stream);
int innfer_recompose_u8(const void* d_tiles, int dtype, int n_tiles, int C, int P, int height, int width, double step, int scale,
                        int via_dtype, int denormalize, uint8_t* d_img, void* stream);
int innfer_inthwc_to_nchw(const void* d_img, int bits, int H, int W, int C, int bgr2rgb, int normalize, float maxval,
                          void* d_out, int out_dtype, void* stream);
int innfer_nchw_to_inthwc(const void* d_in, int in_dtype, int H, int W, int C, int rgb2bgr, int denormalize, int bits,
                          void* d_img, void* stream);

/* fit_channels (115): gray, gray + alpha and BGRA images through an RGB network (in_nc == out_nc == 3).  Extends np2tensor / tensor2np
 * (utils/utils.py:164-248) and the image loop (run.py:404-442), which hand such images to the network as they are.  Layouts, HWC in OpenCV
 * order, C = 1 gray, 2 gray + alpha, 4 BGRA; the last channel of C 2 / 4 is the alpha plane.
 *   colour input [3, H, W]: (g, g, g), or R, G, B from BGRA -- np2tensor of a 3-channel image (same /maxval, normalisation, cast);
 *   alpha input  [3, H, W]: (a, a, a);
 *   output: B, G, R of the colour result exactly as tensor2np (C 4), or gray = mean3(colour result) (C 1 / 2); alpha = mean3(alpha result), or
 *   alpha_const when the network did not run on a constant alpha plane (it is copied as is).
 * mean3(y) = ((y0 + y1) + y2) / 3 in fp32, round to nearest, of the result's three channels already rounded to the result dtype (via_dtype on the
 * chop path); rounded to that dtype again, then quantised as tensor2np (denormalise, clip, * 255 or 65535, round half to even).
 *
 * innfer_channel_minmax: d_minmax[0] = min, d_minmax[1] = max of channel `ch` of a uint8 / uint16 (bits 8 / 16) HWC image; two device ints.
 * innfer_extract_tiles_u8_fit: innfer_extract_tiles_u8 of the colour input into tiles [0, tile_count) of a [*, 3, P, P] buffer and, alpha != 0,
 *   of the alpha input into tiles [tile_count, 2 tile_count): one pixel's C bytes in one load, four pixels per thread where the geometry allows.
 *   It is innfer_extract_tiles_u8_fit_seamless at pad = 0, as innfer_recompose_u8_fit is innfer_recompose_u8_fit_seamless at crop = 0.
 * innfer_recompose_u8_fit: innfer_recompose_u8 of the n colour tiles [0, n) and, alpha != 0, of the alpha tiles [n, 2 n) in one pass: each
 *   pixel's weights once, every channel summed in innfer_recompose_u8's order (so B, G, R are its bytes), then the output above; alpha == 0 with
 *   C 2 / 4 needs alpha_const in [0, 255].  Stores C bytes per pixel into d_img [scale H, scale W, C].
 * innfer_inthwc_to_nchw_fit / innfer_nchw_to_inthwc_fit: the same split and merge on whole images (uint8 / uint16), for the tensor path: d_alpha
 *   may be null (no alpha plane, or a constant one: then alpha_const in [0, 2^bits - 1] is stored).  Channel order is always flipped (bgr2rgb). */
int innfer_channel_minmax(const void* d_img, int bits, int H, int W, int C, int ch, int* d_minmax, void* stream);
int innfer_extract_tiles_u8_fit(const uint8_t* d_img, int C, int H, int W, int normalize, int patch, double step,
                                int tile_begin, int tile_count, int alpha, void* d_tiles, int tile_dtype, void* stream);
int innfer_recompose_u8_fit(const void* d_tiles, int dtype, int n_tiles, int P, int height, int width, double step, int scale,
                            int via_dtype, int denormalize, int C, int alpha, int alpha_const, uint8_t* d_img, void* stream);
int innfer_inthwc_to_nchw_fit(const void* d_img, int bits, int H, int W, int C, int normalize, float maxval,
                              void* d_colour, void* d_alpha, int out_dtype, void* stream);
int innfer_nchw_to_inthwc_fit(const void* d_colour, const void* d_alpha, int in_dtype, int H, int W, int C, int denormalize, int bits,
                              int alpha_const, void* d_img, void* stream);

/* Seamless modes (117): upscale a tileable texture without a seam at its border.  The image is treated as if it had been padded by `pad` pixels on
 * every side and the padding (scale * pad pixels) cut off the result; not in the reference, whose users pad and crop on the host.  The virtual padded
 * image is P[y, x, c] = img[m(y - pad, H), m(x - pad, W), c], all channels (alpha included), size (H + 2 pad) x (W + 2 pad), with the index map
 *   INNFER_BORDER_TILE       m(i, n) = i mod n, a true modulo, any n >= 1                                     (np.pad mode 'wrap')
 *   INNFER_BORDER_MIRROR     j = i mod 2 (n - 1); m = j < n ? j : 2 (n - 1) - j; n >= 2, else INNFER_ERR_INVALID  (np.pad 'reflect', OpenCV REFLECT_101)
 *   INNFER_BORDER_REPLICATE  m = clamp(i, 0, n - 1)                                                            (np.pad 'edge')
 *   INNFER_BORDER_ALPHA_PAD  every channel is 0 outside the image (transparent black)
 *
 * innfer_border_index (host only): m(i, n) as the kernels compute it -- the source index, INNFER_BORDER_OUTSIDE for alpha_pad outside [0, n),
 *   INNFER_BORDER_ERROR (and innfer_last_error) for mirror with n < 2, n < 1 or an unknown mode.
 * innfer_pad_inthwc: the padded image itself, uint8 / uint16 (bits 8 / 16) HWC, any C, into d_out [H + 2 pad, W + 2 pad, C]: the front end of every
 *   path that is not fused (whole-image forwards, model chains, 16-bit images, the guided filter); the result is then cropped by the caller.
 * innfer_extract_tiles_u8_seamless / innfer_extract_tiles_u8_fit_seamless: innfer_extract_tiles_u8 / innfer_extract_tiles_u8_fit of the padded image
 *   without the padded image: the tile lattice is innfer_chop_plan(H + 2 pad, W + 2 pad, patch, step), every tile element is read from d_img [H, W, C]
 *   through the index map (alpha_pad outside: the value of a 0 byte, i.e. 0, or -1 under `normalize`).  Arithmetic, channel flip, tile range, tile
 *   dtype and tile order (fit: colour tiles, then alpha tiles) are those of the entry points they extend; C 1 .. 4 (fit: 1, 2, 4; C > 4 only at
 *   pad = 0, INNFER_ERR_UNSUPPORTED otherwise).  Four pixels per thread where patch % 4 == 0, as one load where the run does not cross a fold of the
 *   map and its bytes are aligned.  pad = 0 is the plain gather, whatever the mode: the map is the identity.
 * innfer_recompose_u8_seamless / innfer_recompose_u8_fit_seamless: innfer_recompose_u8 / innfer_recompose_u8_fit restricted to a crop window.  height
 *   and width are those of the PADDED low-resolution image, crop (low-resolution pixels, 2 crop < height, width) is what is cut off each side: d_img
 *   is [scale (height - 2 crop), scale (width - 2 crop), C] and its pixel (Y, X) is pixel (Y + scale crop, X + scale crop) of the full blend -- the
 *   same tiles in the same order with the same weights, so the same bytes.  Pixels outside the window are neither computed nor stored.  crop = 0 is
 *   the plain blend. */
#define INNFER_BORDER_TILE 0
#define INNFER_BORDER_MIRROR 1
#define INNFER_BORDER_REPLICATE 2
#define INNFER_BORDER_ALPHA_PAD 3
#define INNFER_BORDER_OUTSIDE (-1)
#define INNFER_BORDER_ERROR (-2)
int innfer_border_index(int i, int n, int mode);
int innfer_pad_inthwc(const void* d_img, int bits, int H, int W, int C, int pad, int mode, void* d_out, void* stream);
int innfer_extract_tiles_u8_seamless(const uint8_t* d_img, int C, int H, int W, int normalize, int patch, double step,
                                     int tile_begin, int tile_count, int pad, int mode, void* d_tiles, int tile_dtype, void* stream);
int innfer_extract_tiles_u8_fit_seamless(const uint8_t* d_img, int C, int H, int W, int normalize, int patch, double step,
                                         int tile_begin, int tile_count, int alpha, int pad, int mode, void* d_tiles, int tile_dtype, void* stream);
int innfer_recompose_u8_seamless(const void* d_tiles, int dtype, int n_tiles, int C, int P, int height, int width, double step, int scale,
                                 int via_dtype, int denormalize, int crop, uint8_t* d_img, void* stream);
int innfer_recompose_u8_fit_seamless(const void* d_tiles, int dtype, int n_tiles, int P, int height, int width, double step, int scale,
                                     int via_dtype, int denormalize, int C, int alpha, int alpha_const, int crop, uint8_t* d_img, void* stream);

/* Many images as one tile stream (123, additive; `-batch B`, Model.run_u8_batch; csrc/tiles_u8_multi.hip).  Not in the reference, which runs one image at
 * a time.  n_images uint8 HWC BGR(A) images of any sizes that share the channel count C (1 .. 4) and the tile size
 * ps = min(H_i + 2 pad, W_i + 2 pad, patch) lie packed in ONE device buffer, image i at byte offset in_off[i].  Their tiles -- image 0's in its own
 * innfer_chop_plan(H_0 + 2 pad, W_0 + 2 pad, patch, step) order, then image 1's, ... -- are one [first[n_images], C, ps, ps] buffer, image i's at
 * [first[i], first[i] + counts[i]); the results lie packed in one output buffer, image i's [scale H_i, scale W_i, C] at byte offset out_off[i].
 * sizes: 2 n_images host ints H_0, W_0, H_1, W_1, ...
 *
 * innfer_chop_multi_plan (host only): the geometry into caller memory; every output pointer may be NULL.  *ps; counts [n_images]; first [n_images + 1]
 *   (running tile count; the last entry is the total); in_off / out_off [n_images + 1] (every image starts on a 16-byte boundary; the last entry is the size
 *   of the packed buffer; out_off is for `scale` and C result channels); tiles [first[n_images]]: per tile its image's byte offset and size and the tile's
 *   origin in the padded image; images [n_images]: per image what the blend reads.  The caller uploads `tiles` for the gather and `images` for the blend:
 *   the library copies nothing.  INNFER_ERR_INVALID: images whose tile sizes differ, C outside 1 .. 4, a non-positive size, a negative pad, scale < 1.
 * innfer_extract_tiles_u8_multi: one launch (per 65535 tiles) for all images.  Tile first[i] + k is bit for bit tile k of
 *   innfer_extract_tiles_u8_seamless(image i, C, H_i, W_i, normalize, patch, step, .., pad, mode, .., tile_dtype): four pixels per thread where
 *   ps % 4 == 0, one otherwise.  d_table: the plan's `tiles` on the device.
 * innfer_recompose_u8_multi: one launch (per 65535 images or output rows) for all images.  Image i's bytes are bit for bit
 *   innfer_recompose_u8_seamless(tiles [first[i], first[i] + counts[i]), dtype, counts[i], C, P, H_i + 2 pad, W_i + 2 pad, step, scale, via_dtype,
 *   denormalize, crop = pad).  patch: the gather's, so that ps is; P = scale * ps.  d_images: the plan's `images` (made with this C and scale) on the device.
 * Both check the host `sizes` as the plan does, and per image what the single-image entry points check (the border mode and mirror's two rows and columns;
 * the blend geometry), before anything is launched.  The device tables are read as they are: they must be the plan's for the same arguments. */
typedef struct innfer_multi_tile { int64_t img_off; int H, W, oy, ox; } innfer_multi_tile;           /* the tile's image: in_off[i], H_i, W_i; its origin in the padded image */
typedef struct innfer_multi_image { int64_t out_off, first; int FH, FW, nh, nw; } innfer_multi_image;  /* out_off[i], first[i]; the blend's frame scale (H_i + 2 pad) x scale (W_i + 2 pad); its lattice */
int innfer_chop_multi_plan(int n_images, const int* sizes, int C, int pad, int patch, double step, int scale, int* ps, int* counts, int* first,
                           int64_t* in_off, int64_t* out_off, innfer_multi_tile* tiles, innfer_multi_image* images);
int innfer_extract_tiles_u8_multi(const uint8_t* d_imgs, int n_images, const int* sizes, int C, int normalize, int patch, double step, int pad, int mode,
                                  const innfer_multi_tile* d_table, void* d_tiles, int tile_dtype, void* stream);
int innfer_recompose_u8_multi(const void* d_tiles, int dtype, int n_images, const int* sizes, int C, int P, int patch, double step, int scale,
                              int via_dtype, int denormalize, int pad, const innfer_multi_image* d_images, uint8_t* d_out, void* stream);

/* Self-ensemble (119, `-tta`; ESRGAN's / EDSR's --self_ensemble, "x8"): the image runs through the network in its eight dihedral orientations and the
 * eight results, turned back, are averaged BEFORE quantisation.  Not in the reference.  t_k(x), k = 0 .. 7: transpose (H, W) if k & 4, then flip the
 * columns if k & 1, then flip the rows if k & 2; t_0 is the identity and t_k^-1 undoes the steps in reverse order.  For k >= 4 the oriented image is
 * W x H and has the chop lattice of a W x H image: nh and nw swap, the tile count n stays.  Every orientation has its OWN lattice (the lattice clamps its
 * last row and column, so the tiles of t_k(x) are not the turned tiles of x).  The result is, in tensor terms,
 *   acc = t_0^-1(f(t_0(x))) as float32;  acc += t_k^-1(f(t_k(x))) as float32 for k = 1 .. 7 in this order;  (acc * 0.125) rounded to the tensor dtype
 * with f = chop, run, blend (Model.forward_tta), then quantised as innfer_recompose_u8 / _fit does.
 *
 * innfer_dihedral_index (host only): *sy, *sx = the pixel of the H x W image that pixel (y, x) of t_k(image) shows.  INNFER_ERR_INVALID for k outside
 *   0 .. 7 or a pixel outside the oriented image.
 * innfer_extract_tiles_u8_tta: all tiles of the eight orientations of d_img [H, W, C] into d_tiles [8 n (16 n with alpha), C | 3, ps, ps], n the tile count
 *   of innfer_chop_plan(H + 2 pad, W + 2 pad, patch, step).  Orientation k occupies slots [k n, (k + 1) n), with alpha its alpha tiles [8 n + k n, ..).
 *   Slot k n + i holds what innfer_extract_tiles_u8[_fit][_seamless] returns as tile i of the image t_k(d_img): arithmetic, channel flip and the border
 *   map (pad, mode; the padding is pad on every side, so t_k(pad(x)) == pad(t_k(x))) are theirs.  fit = 0, pad = 0 is the plain form; fit != 0 the
 *   fit_channels form (C 1, 2, 4; alpha only then).  C 1 .. 4, else INNFER_ERR_UNSUPPORTED.
 * innfer_recompose_u8_tta: d_tiles [8 n (16 n), C | 3, P, P] in that slot order -> d_img [scale (height - 2 crop), scale (width - 2 crop), C].  height,
 *   width, crop, n, fit, alpha, alpha_const as for innfer_recompose_u8[_fit]_seamless (n = tiles of ONE orientation; crop = 0: the whole blend).  Per
 *   output pixel and orientation the blend of innfer_recompose_u8 at the pixel's place in that orientation's frame, rounded to via_dtype; the eight are
 *   added as float32 in the order k = 0 .. 7, multiplied by 0.125f and rounded to via_dtype; then mean3 / the constant alpha (fit) and the quantisation.
 *   C 1 .. 4, else INNFER_ERR_UNSUPPORTED. */
int innfer_dihedral_index(int k, int H, int W, int y, int x, int* sy, int* sx);
int innfer_extract_tiles_u8_tta(const uint8_t* d_img, int C, int H, int W, int normalize, int patch, double step, int fit, int alpha,
                                int pad, int mode, void* d_tiles, int tile_dtype, void* stream);
int innfer_recompose_u8_tta(const void* d_tiles, int dtype, int n, int C, int P, int height, int width, double step, int scale,
                            int via_dtype, int denormalize, int fit, int alpha, int alpha_const, int crop, uint8_t* d_img, void* stream);

/* The stitched tile path (122, additive; `-tile N -tile_pad P`, Real-ESRGAN's --tile / --tile_pad; csrc/tiles_stitch.hip).  Large rectangular tiles that
 * carry a halo of context pixels; the halo is thrown away, every output pixel comes from exactly one tile (its owner) and nothing is averaged.  Not in the
 * reference, whose chop blends 200 x 200 tiles at step 0.5 (3.7 .. 3.9x the image's pixels through the network; this lattice: 1.05 .. 1.12x).
 * Per axis of A pixels, tile core `tile` = T >= 1 and `halo` = h >= 0, in low-resolution pixels:
 *   A <= T + 2h :  n = 1, P = A, origin 0
 *   otherwise   :  n = ceil((A - 2h) / T);  P = ceil((A + 2h (n - 1)) / n);  S = P - 2h;  o_i = min(i S, A - P), i = 0 .. n - 1
 *   owner(y)    =  the largest i with i == 0 or o_i + h <= y
 * Tiles are P_h x P_w, all equal (balanced: 1080 rows at T = 1024 are two tiles of 556 rows), row-major, wholly inside the image.  Pixel (Y, X) of the
 * scale H x scale W result is pixel (Y - scale o_ky, X - scale o_kx) of tile (ky, kx)'s result, ky = owner(Y / scale), kx = owner(X / scale): an owned
 * pixel is at least h away from every tile edge that is not an image edge.
 *
 * innfer_tile_plan (host only): P_h, P_w, the tile counts and the origins (ys [nh] / xs [nw], either may be NULL, as may every other output).
 *   INNFER_ERR_INVALID for a non-positive H, W or tile, or a negative halo.
 * innfer_tile_owner (host only): the owner as the kernels compute it -- *index = owner(X / scale) and *origin = scale o_index for position X of the
 *   scale * A output axis.
 * innfer_extract_tiles_rect: d_img [1, C, H, W] (INNFER_F16 / INNFER_F32, any C) -> d_tiles [tile_count, C, P_h, P_w], tiles tile_begin .. of the lattice.
 * innfer_extract_tiles_u8_rect: the same of np2tensor(image) for a uint8 HWC BGR(A) image, C 1 .. 4, without the float image: /255, BGR(A) -> RGB(A),
 *   `normalize`, cast to tile_dtype -- innfer_extract_tiles_u8's arithmetic.  The lattice is that of the virtual (H + 2 pad) x (W + 2 pad) image and every
 *   element is read through the border map `mode`, exactly as innfer_extract_tiles_u8_seamless reads it; pad = 0 is the plain form.
 * innfer_stitch_tiles: d_tiles [n, C, scale P_h, scale P_w] -> d_out [1, C, scale height, scale width] of the same dtype, a copy from the owner tile;
 *   n must be the lattice's tile count.
 * innfer_stitch_tiles_u8: the same with tensor2np as the store (denormalise, RGB(A) -> BGR(A), clip, * 255, round half to even: innfer_recompose_u8's
 *   quantisation without a blend in front), C 1 .. 4.  height and width are those of the PADDED image, crop (2 crop < height, width) is cut off every side:
 *   d_img is [scale (height - 2 crop), scale (width - 2 crop), C]; pixels outside that window are neither read nor stored.  crop = 0: the whole frame.
 * One read and one write per element; all offsets are 64-bit (an 8K frame's tiles at scale 4 pass 2^31 elements).  More than 65535 tile rows (gathers) or
 * output rows (stitches): INNFER_ERR_UNSUPPORTED.  The 200 / 0.5 chop, its kernels and entry points are unchanged. */
int innfer_tile_plan(int H, int W, int tile, int halo, int* ph, int* pw, int* nh, int* nw, int* ys, int* xs);
int innfer_tile_owner(int A, int tile, int halo, int scale, int X, int* index, int* origin);
int innfer_extract_tiles_rect(const void* d_img, int dtype, int C, int H, int W, int tile, int halo, int tile_begin, int tile_count,
                              void* d_tiles, void* stream);
int innfer_extract_tiles_u8_rect(const uint8_t* d_img, int C, int H, int W, int normalize, int tile, int halo, int tile_begin, int tile_count,
                                 int pad, int mode, void* d_tiles, int tile_dtype, void* stream);
int innfer_stitch_tiles(const void* d_tiles, int dtype, int n, int C, int height, int width, int tile, int halo, int scale, void* d_out, void* stream);
int innfer_stitch_tiles_u8(const void* d_tiles, int dtype, int n, int C, int height, int width, int tile, int halo, int scale, int denormalize,
                           int crop, uint8_t* d_img, void* stream);

/* srgb2linear / linear2srgb (utils/colors.py:29-46, 49-60), the pointwise halves of the `-cf` colour
 * fix: uint8 sRGB -> float32 linear, and float32 linear -> uint8 sRGB (clip, gamma, *255, TRUNCATING
 * cast like astype(np.uint8)).  n = number of elements (any layout). */
int innfer_srgb_to_linear(const uint8_t* d_in, float* d_out, size_t n, void* stream);
int innfer_linear_to_srgb(const float* d_in, uint8_t* d_out, size_t n, void* stream);

/* Colour fix (`-cf`): replaces color_fix (utils/utils.py:278-315).  d_lr / d_sr / d_out are uint8 HWC images
 * on the device (any channel order, C <= 4); out = linear2srgb(resize(gauss3(lin(lr) - resize(lin(sr)))) + lin(sr)).
 * The reference's cv2.resize(INTER_CUBIC) and cv2.GaussianBlur(3x3, sigma 0) are restated from OpenCV's
 * published float32 algorithms (parity with OpenCV itself is unpinned: it is absent from the image). */
size_t innfer_color_fix_workspace_bytes(int h_lr, int w_lr, int h_sr, int w_sr, int channels);
int innfer_color_fix(const uint8_t* d_lr, int h_lr, int w_lr, const uint8_t* d_sr, int h_sr, int w_sr, int channels,
                     uint8_t* d_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* Colour-fix modes (123, additive; `-cf_mode`; not in the reference, whose only fix is mode 0).  mode: INNFER_COLOR_FIX_LOWFREQ forwards to innfer_color_fix
 * above.  INNFER_COLOR_FIX_WAVELET: StableSR's wavelet reconstruction in code units -- out = quantise(sr + B5(up(lr) - sr)), up = the cubic enlargement
 * innfer_color_fix uses, B5 = five a-trous levels (dilation 1, 2, 4, 8, 16) of the [0.25, 0.5, 0.25] filter along x, then y, replicate border; one fused
 * kernel, every intermediate in LDS, no workspace.  INNFER_COLOR_FIX_ADAIN: every channel of sr moved to lr's mean and (unbiased) standard deviation --
 * exact integer sums, gain and offset in float64, out = quantise(sr * g + o); the workspace holds the counters and the per-channel gain / offset, is
 * zeroed on the stream by the call and must be 8-byte aligned.  quantise(v) = clamp(floor(v + 0.5), 0, 255); utils.color_fix_np is the contract.
 * Shapes as for innfer_color_fix; bad modes, bad shapes and short workspaces are refused before anything is launched.  The workspace of modes 1 and 2
 * does not depend on the image sizes (0 and a few hundred bytes). */
enum { INNFER_COLOR_FIX_LOWFREQ = 0, INNFER_COLOR_FIX_WAVELET = 1, INNFER_COLOR_FIX_ADAIN = 2 };
size_t innfer_color_fix_mode_workspace_bytes(int mode, int h_lr, int w_lr, int h_sr, int w_sr, int channels);
int innfer_color_fix_mode(int mode, const uint8_t* d_lr, int h_lr, int w_lr, const uint8_t* d_sr, int h_sr, int w_sr, int channels,
                          uint8_t* d_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* linear_resize (utils/utils.py:267-276, the pix2pix pre-step of run.py:413-414): uint8 HWC image -> srgb2linear -> bicubic resize to
 * (oh, ow) (OpenCV INTER_CUBIC, a = -0.75, as in innfer_color_fix: parity with OpenCV itself unpinned) -> linear2srgb, uint8 HWC.
 * Workspace: h * w * C floats.  (104) */
int innfer_linear_resize(const uint8_t* d_img, int h, int w, int C, uint8_t* d_out, int oh, int ow,
                         void* d_workspace, size_t workspace_bytes, void* stream);

/* Resampling to any final size (118, `-outscale`): an antialiased separable resampler in the Pillow / ATen `antialias=True` convention, uint8 / uint16 HWC
 * images of 1 .. 4 channels, enlarging and reducing.  Not in the reference, whose users download the full result and resize on the host.  innfer_linear_resize
 * above (OpenCV's 4-tap cubic, enlarging only, no antialiasing) is another function and is unchanged.
 *
 * The tables of one axis of n_in samples and n_out outputs, filter f of support S
 *   INNFER_RESAMPLE_BOX       1 on (-0.5, 0.5], S = 0.5          INNFER_RESAMPLE_BILINEAR  triangle, S = 1
 *   INNFER_RESAMPLE_BICUBIC   Keys a = -0.5, S = 2               INNFER_RESAMPLE_LANCZOS   sinc(x) sinc(x / 3) on [-3, 3), S = 3
 * for output i: scale = n_in / n_out, fs = max(scale, 1), support = S fs, c = (i + 0.5) scale, lo = floor(c - support + 0.5), hi = floor(c + support + 0.5);
 * wrap = 0: lo is clamped to >= 0 and hi to <= n_in (the window is truncated at the border and renormalised); wrap != 0: lo and hi stay and tap j reads
 * sample j mod n_in (a tileable texture stays tileable).  w_j = f((j - c + 0.5) / fs) for j in [lo, hi), computed in float64, divided by their sum,
 * rounded once to float32.
 *
 * innfer_resample_taps (host only): T, the largest hi - lo of any output, wrapped or not; < 0 on a bad argument.
 * innfer_resample_plan (host only, no HIP call): start[i] = lo (may be negative when wrapping), count[i] = hi - lo, weights [n_out][T] zero-padded
 *   behind count[i]; T >= innfer_resample_taps.  n_in, n_out 1 .. 2^28.
 * innfer_resample_inthwc: d_src [h, w, C] -> d_dst [oh, ow, C], bits 8 / 16, C 1 .. 4, with DEVICE copies of the horizontal plan (w -> ow, width Th)
 *   and the vertical one (h -> oh, width Tv).  Channels are filtered independently (alpha is straight, not premultiplied).  The horizontal pass runs
 *   first, on every source row the vertical pass needs; its float32 result is the input of the vertical pass.  In each pass the float32 accumulator
 *   starts at 0 and takes acc = acc + w x per tap in ascending j, the multiply and the add each rounded to float32 (no FMA); the stored code is
 *   clamp(floor(acc + 0.5f), 0, 255 | 65535).  An axis with n_out == n_in goes through its table like any other.  One launch with the intermediate
 *   in LDS wherever a block of output pixels fits (innfer_resample_workspace_bytes returns 0); otherwise (reductions by hundreds) two launches
 *   through the float32 intermediate [h, ow, C] in d_workspace -- the same arithmetic in the same order, so the same bytes; too small a workspace:
 *   INNFER_ERR_WORKSPACE.  Offsets are size_t.  Arguments are checked before any device call (INNFER_ERR_INVALID). */
#define INNFER_RESAMPLE_BOX 0
#define INNFER_RESAMPLE_BILINEAR 1
#define INNFER_RESAMPLE_BICUBIC 2
#define INNFER_RESAMPLE_LANCZOS 3
int innfer_resample_taps(int n_in, int n_out, int filter);
int innfer_resample_plan(int n_in, int n_out, int filter, int wrap, int* start, int* count, float* weights, int T);
size_t innfer_resample_workspace_bytes(int h, int w, int C, int oh, int ow, int Th, int Tv);
int innfer_resample_inthwc(const void* d_src, int bits, int h, int w, int C, void* d_dst, int oh, int ow,
                           const int* d_hstart, const int* d_hcount, const float* d_hweights, int Th,
                           const int* d_vstart, const int* d_vcount, const float* d_vweights, int Tv,
                           int wrap, void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INNFER_AMD_H */
