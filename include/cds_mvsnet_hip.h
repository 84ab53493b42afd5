/*
 * cds_mvsnet_hip.h — C ABI of libcdsmvs_hip.so, the MI355X (gfx950) implementation of the
 * CDS-MVSNet plane-sweep hot path.
 *
 * The reference (TruongKhang/cds-mvsnet) is pure Python/PyTorch and has no FFI of its own; its
 * boundary for this path is models.model.CDSMVSNet.forward (models/model.py:140).  Beneath that
 * boundary this library replaces the PyTorch op sequences listed below.  Each entry point cites
 * the reference lines it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless the name ends in _host.  Since round 6 that includes the
 *     per-call GEOMETRY: homographies (`mats`), epipoles and the depth-range scalars are device data - slices of one small
 *     "geometry block" the host writes with a single host -> device copy per forward (cds_mvsnet_amd/geometry.py) - and no
 *     longer by-value arguments, so that a captured hipGraph of the forward / training step is replayed for new cameras by
 *     rewriting that block;
 *   - the caller owns all memory; nothing is allocated, freed or synchronised inside;
 *   - `stream` is a hipStream_t (NULL = default stream); calls are re-entrant across streams;
 *   - return value: 0 on success, a negative hipError_t on a launch failure,
 *     CDS_EINVAL (-1000) for invalid arguments;
 *   - batch: one call handles one batch item (the Python host loops over B).
 *
 * Layouts: feature maps NCHW without the N ([C][h][w]); channels-last copies [h][w][C] where
 * stated; cost volumes [C][D][h][w]; per-pixel hypotheses [D][h][w].
 */
#ifndef CDS_MVSNET_HIP_H
#define CDS_MVSNET_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define CDS_EINVAL (-1000)
#define CDS_MAX_VIEWS 8 /* source views per launch; more are handled by chunked calls */
#define CDS_MAX_IMAGES 16 /* images per batched FeatureNet launch */
#define CDS_STAGE_STATE_WORDS 2080 /* workspace of cds_stage_inputs_f32: 1 + 2 x (<= 1024 + CDS_MAX_VIEWS workgroups), rounded up */

/* activation codes for the conv entry points */
#define CDS_ACT_NONE 0
#define CDS_ACT_RELU 1
#define CDS_ACT_LEAKY01 2 /* LeakyReLU(0.1) */
#define CDS_ACT_SIGMOID 3
#define CDS_ACT_ACCUM 16 /* OR-ed onto an activation code of cds_conv2d_*_f32: out += act(conv) (gradient accumulation) */
#define CDS_ACT_TANH 4

/* flags of cds_warp_aggregate_f32 */
#define CDS_AGG_ACCUMULATE 1 /* add onto the existing volume / vis_sum instead of overwriting */
#define CDS_AGG_NORMALIZE 2  /* divide by (vis_sum + 1e-6) before the store (model.py:74) */
#define CDS_AGG_CHANNELS_LAST 4 /* volume laid out [D][h][w][C] (a voxel's channels contiguous: one 32-byte store per 8 channels) */
/*
 * Sample-position arithmetic of the LDS-staged K1 / K3 kernels (flag of cds_warp_aggregate_f32 and cds_warp_entropy_flags_f32).
 * Absent (what the product path passes by default): the reference's fp32 operation order (correctly rounded divisions, ATen's
 * normalise / de-normalise round trip): sample positions bit-identical to F.grid_sample's.  Set (opt-in): (u, v) = p.xy *
 * rcp(p.z + 1e-6) directly, 5-11 % faster; the positions then differ by up to ~1e-4 px at w = 640 and the volume of sharp
 * feature maps moves by up to 8.4e-5 against the reference - OUTSIDE the 1e-5 parity tolerance (exact mode: 1.2e-7); the depth
 * mean-L1 is unaffected (tests/test_hip_parity.py::test_fast_positions_leave_the_parity_tolerance_at_full_width).  The direct
 * (non-LDS) fallback kernels always use the reference order.
 */
#define CDS_AGG_FAST_POSITIONS 8
#define CDS_WARP_FAST_POSITIONS CDS_AGG_FAST_POSITIONS

/* Library version (major*10000 + minor*100 + patch). */
int cds_version(void);

/* [C][h][w] -> [h][w][C] re-layout of one feature map (source maps are gathered channels-last). */
int cds_chw_to_hwc_f32(const float* src_chw, float* dst_hwc, int C, int h, int w, void* stream);

/*
 * The reference-signature boundary of one stage in one launch.  models/model.py:16-40 hands StageNet.forward a list over the
 * source views of {'ref': (fea, nc_sum, nc), 'src': (fea, nc_sum, _)}; this gathers it into the layouts K1 / K3 read:
 *   ref_feas, src_feas      HOST arrays of V DEVICE pointers, each one [C][h][w] feature map (contiguous fp32)
 *   ref_nc, ref_ncsum, src_ncsum   HOST arrays of V DEVICE pointers to [h][w] maps (model.py:51,59), or NULL with their outputs
 *   ref_chw_out [V][C][h][w]   the stacked reference copies
 *   src_hwc_out [V][h][w][C]   the source maps channels-last (cds_chw_to_hwc_f32 per view)
 *   ref_nc_out  [V][h][w] | NULL;  nc_mean_out [h][w] | NULL = sum_v ((ref_ncsum[v] + src_ncsum[v]) / 2) / V in view order
 *                              (= cds_pair_mean_f32 then cds_view_mean_f32, model.py:59-60)
 *   state [CDS_STAGE_STATE_WORDS] | NULL   device workspace (no initialisation needed); on completion state[0] = max |ref| *
 *                              max |src|: the bound of the normalised volume, the in_bound of cds_conv3d_sf16_f32's first layer
 *                              (NaN if a feature is NaN); the rest holds the per-workgroup maxima a second tiny launch merges
 * V <= CDS_MAX_VIEWS, C in {8, 16, 32}.
 */
int cds_stage_inputs_f32(const float* const* ref_feas, const float* const* src_feas, const float* const* ref_nc,
                         const float* const* ref_ncsum, const float* const* src_ncsum, float* ref_chw_out, float* src_hwc_out,
                         float* ref_nc_out, float* nc_mean_out, float* state, int V, int C, int h, int w, void* stream);

/*
 * homo_warping_3D (models/utils/warping.py:69-104): bilinear, zero padding, align_corners=True.
 *   src_hwc   [h][w][C]   source feature map, channels-last
 *   mat       12 floats   rows of (P_src * P_ref^-1)[:3,:3] then its [:3,3] (warping.py:80-82); DEVICE memory
 *   hyp       [D][h][w] if hyp_per_pixel else [D]
 *   out       [C][D][h][w]
 */
int cds_homo_warp_f32(const float* src_hwc, const float* mat, const float* hyp, float* out,
                      int C, int D, int h, int w, int hyp_per_pixel, void* stream);

/*
 * K1 "warp-correlate-entropy" (warping.py:79-102 + model.py:46-50): for every source view v and
 * pixel, the entropy over D of softmax_D( sum_C ref_v * warp(src_v) ).  Never materialises the
 * warped volume.
 *   ref_chw   [V][C][h][w]  per-pair reference features
 *   src_hwc   [V][h][w][C]  source features, channels-last
 *   mats      [V][12]       homographies as above, DEVICE memory (geometry block)
 *   entropy   [V][h][w]
 */
int cds_warp_entropy_f32(const float* ref_chw, const float* src_hwc, const float* mats,
                         const float* hyp, float* entropy, int V, int C, int D, int h, int w,
                         int hyp_per_pixel, void* stream);
/* the same with flags: CDS_WARP_FAST_POSITIONS (cds_warp_entropy_f32 == flags 0) */
int cds_warp_entropy_flags_f32(const float* ref_chw, const float* src_hwc, const float* mats,
                               const float* hyp, float* entropy, int V, int C, int D, int h, int w,
                               int hyp_per_pixel, int flags, void* stream);

/*
 * K3 "warp-aggregate" (model.py:44-47,57-60,74): volume = sum_v vis_v * (ref_v (x) warp(src_v)),
 * vis_sum = sum_v vis_v, optionally normalised by (vis_sum + 1e-6).  The volume is written once.
 *   vis_w     [V][h][w]
 *   volume    [C][D][h][w], or [D][h][w][C] with CDS_AGG_CHANNELS_LAST (what the split-bf16 CostRegNet kernels read)
 *   vis_sum   [h][w]
 *   flags     CDS_AGG_*
 * V <= CDS_MAX_VIEWS per call.
 */
int cds_warp_aggregate_f32(const float* ref_chw, const float* src_hwc, const float* vis_w,
                           const float* mats, const float* hyp, float* volume, float* vis_sum,
                           int V, int C, int D, int h, int w, int hyp_per_pixel, int flags,
                           void* stream);

/*
 * Row-window forms of K1 / K3 (pixel-slab sharding across GPUs): the reference-side tensors cover rows [y_off, y_off + h) of the
 * hs x w image grid -- ref_chw [V][C][h][w], hyp [D][h][w] (per pixel), vis_w / entropy [V][h][w], volume [C][D][h][w] or
 * [D][h][w][C], vis_sum [h][w] -- while src_hwc [V][hs][w][C] covers the whole grid.  Positions are computed from the global row
 * y_off + y: a window's result equals the same rows of the full-grid call bit for bit.  flags as in the full-grid calls.
 * Returns CDS_EINVAL for shapes outside the LDS-staged kernels (C not in {8, 16, 32}, w < 2).
 */
int cds_warp_entropy_window_f32(const float* ref_chw, const float* src_hwc, const float* mats, const float* hyp,
                                float* entropy, int V, int C, int D, int h, int w, int hs, int y_off, int flags, void* stream);
int cds_warp_aggregate_window_f32(const float* ref_chw, const float* src_hwc, const float* vis_w, const float* mats,
                                  const float* hyp, float* volume, float* vis_sum, int V, int C, int D, int h, int w, int hs,
                                  int y_off, int flags, void* stream);

/*
 * Backward of the un-normalised K3 (training step).  With volume = sum_v vis_v * ref_v (x) warp(src_v):
 *   grad_volume  [C][D][h][w]   incoming gradient
 *   grad_ref     [V][C][h][w]   ACCUMULATED with atomics (partial sums per depth segment): the caller zeroes it first
 *   grad_src_hwc [V][h][w][C]   ACCUMULATED with atomics (bilinear scatter; runs of planes in one texel cell are merged first)
 *   grad_vis     [V][h][w]      ACCUMULATED with atomics (partial sums per channel group and depth segment)
 * The sampling grid has no gradient (built under no_grad, warping.py:79): nothing flows to hypotheses / cameras.
 */
int cds_warp_aggregate_bwd_f32(const float* ref_chw, const float* src_hwc, const float* vis_w,
                               const float* mats, const float* hyp, const float* grad_volume,
                               float* grad_ref, float* grad_src_hwc, float* grad_vis, int V, int C, int D,
                               int h, int w, int hyp_per_pixel, void* stream);
/* The training step's epilogue of K3 (models/model.py:56-78) in one launch, and its backward in two: volume = volume_sum /
 * (sum_v vis + 1e-6), feat_distance[d] = sum_c volume_sum[c][d] / (sum_v vis + 1e-6), plane D from gt_sum [C][hw] (K3 at the
 * ground-truth depth) when given.  Backward: g_volume / g_feat_distance may be NULL (no gradient); scratch D x hw floats. */
int cds_volume_finish_f32(const float* volume_sum, const float* gt_sum, const float* vis, int V, int C, int D, int hw, float* volume,
                          float* feat_distance, void* stream);
int cds_volume_finish_bwd_f32(const float* g_volume, const float* g_feat_distance, const float* volume_sum, const float* gt_sum,
                              const float* vis, int V, int C, int D, int hw, float* g_volume_sum, float* g_gt_sum, float* g_vis,
                              float* scratch, void* stream);

/* volume[c][d][p] /= (vis_sum[p] + 1e-6)  (model.py:74) — the finalisation after a view-shard
 * all-reduce of partial sums. */
int cds_volume_normalize_f32(float* volume, const float* vis_sum, int C, int D, int hw, void* stream);

/* The same division for a channels-last partial volume [D][h][w][C] (C % 4 == 0): every channel of voxel (d, p) is divided
 * by (vis_sum[p] + 1e-6).  Used after the view-shard all-reduce (model.py:74). */
int cds_volume_normalize_cl_f32(float* volume, const float* vis_sum, int C, int D, int hw, void* stream);

/*
 * K5 (model.py:90-92, module.py:373-391): softmax over D, depth = sum p*hyp, confidence =
 * sum of p over [i-1,i+2] at i = clamp(trunc(sum p*index),0,D-1).  prob (may be NULL) receives
 * the softmax volume [D][h][w].
 */
int cds_softargmin_conf_f32(const float* prob_pre, const float* hyp, float* depth, float* conf,
                            float* prob, int D, int h, int w, int hyp_per_pixel, void* stream);

/*
 * K6 (module.py:394-439 + model.py:176-193): per-pixel hypotheses of a cascade stage.
 *   prev_depth [hp][wp]  previous stage depth map; it is bilinearly (align_corners=False)
 *                        upsampled to H x W, sampled at  up - ((D-1)/2)*interval + k*interval,
 *                        clamped to [dmin,dmax] and resized trilinearly to [D][H/scale][W/scale].
 *   out        [D][H/scale][W/scale]
 *   interval   1 float, DEVICE: the stage's hypothesis spacing (ratio x depth interval)
 *   depth_range 2 floats, DEVICE: (dmin, dmax)
 */
int cds_depth_hypotheses_f32(const float* prev_depth, float* out, int D, int hp, int wp, int H, int W,
                             int scale, const float* interval, const float* depth_range, void* stream);

/* First-stage planes: out[k][y][x] = lo + k*((hi-lo)/(D-1))  (module.py:425-433); depth_range = (lo, hi), DEVICE. */
int cds_depth_planes_f32(float* out, int D, int h, int w, const float* depth_range, void* stream);

/*
 * K4 (module.py:80-116,270-315): 3x3x3 convolution, padding 1, stride 1 or 2, with fused
 * per-channel bias (folded BatchNorm3d), optional ReLU and optional residual added AFTER the
 * activation (module.py:311-313).
 *   x [Cin][D][H][W]; bias [Cout] or NULL; skip like out or NULL
 *   weight PACKED [Cin][27][Cout] (tap = (kz*3+ky)*3+kx, cout fastest) — i.e. PyTorch's
 *          [Cout][Cin][3][3][3] permuted (1,2,3,4,0); Cout must be 1 or a multiple of 8
 *   out [Cout][Do][Ho][Wo], Xo = (X-1)/stride+1
 */
int cds_conv3d_k3_f32(const float* x, const float* weight, const float* bias, const float* skip,
                      float* out, int Cin, int Cout, int D, int H, int W, int stride, int act,
                      void* stream);

/*
 * Same convolution at stride 1 for Cin % 16 == 0, Cout % 16 == 0, W % 4 == 0 on the matrix cores with a
 * channels-last LDS tile (one 16-byte LDS read feeds four MFMAs).
 *   weight_cl PACKED [27][Cout][Cin] (cin fastest) = PyTorch's [Cout][Cin][3][3][3] permuted (2,3,4,0,1)
 * Returns CDS_EINVAL for shapes it does not cover (callers fall back to cds_conv3d_k3_f32).
 */
int cds_conv3d_k3_cl_f32(const float* x, const float* weight_cl, const float* bias, const float* skip,
                         float* out, int Cin, int Cout, int D, int H, int W, int act, void* stream);

/* K4, split-bf16 arithmetic on channels-last volumes (csrc/conv3d_sbf.hip): 3x3x3 convolution, pad 1, stride 1 | 2
 * (+bias +ReLU +residual).  Every fp32 operand is split exactly into three bf16 terms and multiplied as six error-compensated
 * partial products on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: fp32-class error (dropped terms <= 2^-23 |a b| per
 * product) at the bf16 matrix rate.  Replaces models/module.py:80-116 (Conv3d + BatchNorm3d(eval, folded) + ReLU) like
 * cds_conv3d_k3_f32, on x [D][H][W][Cin] -> out [Do][Ho][Wo][Cout] (a voxel's channels contiguous).
 * weight_split: int16 [Cin/8][7][ceil(Cout/16)][3][64][8] packed by the host (ops.split_pack_conv3d).
 * stride == CDS_SBF_PAIR: stride 1 with Cout == 8 and pair-packed weights [Cin/8][9][1][3][64][8] (ops.split_pack_conv3d_pair):
 * an MFMA column is a pair of x-adjacent voxels, its rows (x parity, cout), so no matrix row multiplies padding.
 * Needs Cin % 8 == 0, Cout % 4 == 0, Cout <= 64; CDS_EINVAL otherwise. */
#define CDS_SBF_PAIR 101
int cds_conv3d_sbf_f32(const float* x, const void* weight_split, const float* bias, const float* skip, float* out,
                       int Cin, int Cout, int D, int H, int W, int stride, int act, void* stream);
/* The same convolution in SPLIT-F16 arithmetic: every fp32 operand as TWO fp16 terms of (operand x a power-of-two tensor scale), three
 * partial products per K-step on v_mfma_f32_16x16x32_f16, fp32 accumulate, exact rescaling in the epilogue - fp32-class error (the
 * representation error is ~0.3x the rounding error of an fp32 convolution) at half the matrix-pipe work of split-bf16.  Shapes: those
 * of the z-marching kernels (Cin, Cout, stride) in {(8 | 16 | 32, 8, PAIR), (16, 16, 1), (8, 16, 2), (16, 32, 2)}; CDS_EINVAL otherwise.
 *   weight_split  the split-bf16 layout with fp16 terms (hi, lo, unused) of weight * w_scale (ops.split_pack_conv3d / _pair (f16=True))
 *   w_inv_scale   1 / w_scale, a power of two
 *   in_bound      DEVICE scalar >= max |x| (the producing kernel's out_bound, or any upper bound: it fixes the input's scale)
 *   out_bound     DEVICE scalar that receives max |out| by an atomic maximum (zero it before the call), or NULL */
int cds_conv3d_sf16_f32(const float* x, const void* weight_split, const float* bias, float* out, int Cin, int Cout, int D, int H, int W,
                        int stride, int act, const float* in_bound, float w_inv_scale, float* out_bound, void* stream);


/* ConvTranspose3d k3 s2 p1 op1 (+bias +ReLU +residual) in the same split-bf16 arithmetic, channels-last: x [D][H][W][Cin]
 * -> out [2D][2H][2W][Cout].  Replaces models/module.py:125-160 (Deconv3d + BatchNorm3d(eval, folded) + ReLU + the U-Net
 * skip addition of :310-312).  weight_split from ops.split_pack_deconv3d.  Cout in {8, 16, 32}, Cin % 8 == 0.
 * out_planar != 0: the output is written [Cout][2D][2H][2W] (for a planar consumer: conv11 -> prob); skip stays channels-last. */
int cds_deconv3d_sbf_f32(const float* x, const void* weight_split, const float* bias, const float* skip, float* out,
                         int Cin, int Cout, int D, int H, int W, int act, int out_planar, void* stream);

/* ConvTranspose3d(32 -> 16, k3 s2 p1 op1) + folded BN shift + ReLU + residual (conv9 of CostRegNet: models/module.py:125-160, :496)
 * as a z-marching kernel with one consumer wave per output parity class and that class's weights resident in registers
 * (csrc/deconv3d_zm.hip).  Same arithmetic (split-bf16) and tensors as cds_deconv3d_sbf_f32: x [D][H][W][32] channels-last ->
 * out [2D][2H][2W][16], skip like out or NULL; weight_cls from ops.split_pack_deconv_cls (int16 [8][4][2][3][64][8]).
 * Cin == 32 and Cout == 16 only (CDS_EINVAL otherwise). */
int cds_deconv3d_zm_f32(const float* x, const void* weight_cls, const float* bias, const float* skip, float* out,
                        int Cin, int Cout, int D, int H, int W, int act, void* stream);
/* conv7 (Cout = 32) and conv9 (32 -> 16, z-marching) in SPLIT-F16 arithmetic (see cds_conv3d_sf16_f32 for the operands: weights from the
 * packers with f16=True, w_inv_scale, in_bound / out_bound device scalars). */
int cds_deconv3d_sf16_f32(const float* x, const void* weight_split, const float* bias, const float* skip, float* out, int Cin, int Cout,
                          int D, int H, int W, int act, const float* in_bound, float w_inv_scale, float* out_bound, void* stream);
int cds_deconv3d_zm_sf16_f32(const float* x, const void* weight_cls, const float* bias, const float* skip, float* out, int Cin, int Cout,
                             int D, int H, int W, int act, const float* in_bound, float w_inv_scale, float* out_bound, void* stream);


/* The tail of CostRegNet in one launch: conv11 = ConvTranspose3d(16 -> 8, k3 s2 p1 op1) + BatchNorm3d(eval, folded) + ReLU
 * (models/module.py:125-160, :495), the residual `conv0 + conv11(x)` (:498) and prob = Conv3d(8 -> 1, k3, p1, bias=False)
 * (:499).  x [D][H][W][16] channels-last input cells, skip [2D][2H][2W][8] channels-last, out [2D][2H][2W] fp32.  The 8-channel
 * full-resolution volume between the two layers stays in LDS (z-marching workgroups, csrc/deconv_prob_zm.hip); the transposed
 * convolution runs in split-bf16 arithmetic on the matrix cores, prob in plain fp32 on the VALU.
 * weight_split from ops.split_pack_deconv_prob (int16 [2][5][3][64][8]), bias [8], prob_table from ops.pack_prob_table
 * (float [3 kx][2][3 ky][3 kz][4]). */
int cds_deconv_prob_zm_f32(const float* x, const void* weight_split, const float* bias, const float* skip,
                           const float* prob_table, float* out, int D, int H, int W, void* stream);
/* The fused tail with its transposed convolution in SPLIT-F16 arithmetic (weights from ops.split_pack_deconv_prob(..., f16=True);
 * in_bound: DEVICE scalar >= max |x|, conv9's out_bound). */
int cds_deconv_prob_zm_sf16_f32(const float* x, const void* weight_split, const float* bias, const float* skip, const float* prob_table,
                                float* out, int D, int H, int W, const float* in_bound, float w_inv_scale, void* stream);
/* The split-f16 tail with prob on the matrix cores too: the consumers keep the volume between the layers as two fp16 terms, the prob
 * waves run a tap-expanded GEMM on it (csrc/deconv_prob_zm.hip).  prob_mfma / p_inv_scale from ops.split_pack_prob (int16 [3][3][64][8]
 * and 1 / scale); skip_bound: DEVICE scalar >= max |skip| (conv0's out_bound); y_gain >= max over cout of sum |folded conv11 weight| (ops.deconv_prob_gain).
 * CDS_DPZ_PROB_MFMA=0 (read per launch) runs prob on the VALU from prob_table: the kernel of cds_deconv_prob_zm_sf16_f32. */
int cds_deconv_prob_zm_sf16_mfma_f32(const float* x, const void* weight_split, const float* bias, const float* skip,
                                     const float* prob_table, const void* prob_mfma, float* out, int D, int H, int W,
                                     const float* in_bound, float w_inv_scale, const float* skip_bound, float y_gain, float p_inv_scale,
                                     void* stream);

/* How the z-marching CostRegNet kernels (conv3d_zmg, deconv3d_zm, deconv_prob_zm) cut a layer into workgroups, on the host (no GPU
 * call; for tests).  Uniform cutting: columns x z segments equal units.  Balanced cutting (csrc/zm_common.hpp): workgroup wg of nwg
 * owns one contiguous range of the column-major (column, stage) sequence, cut at the column boundaries into pieces; a piece shorter
 * than min_len stages goes to the neighbour that holds the rest of its column.  CDS_ZM_BALANCE (read per launch): 0 = uniform only,
 * 1 (default) = balanced where the cost model says it is cheaper, 2 = balanced wherever a workgroup has at most 8 pieces and the
 * kernel has the registers; CDS_ZM_NCU overrides the number of workgroups (default: the device's CU count).  Results do not depend
 * on either.
 * cds_zm_partition: the pieces of workgroup wg for `cols` columns of `planes` planes, `unit` planes per stage, as (column, first
 * plane, one past the last plane) triples in out[24]; returns their number - more than 8 (of which the first 8 are stored) where
 * the layer keeps the uniform cutting.
 * cds_zm_plan: what a launch would choose for such a layer with ys cout splits on ncu workgroups under CDS_ZM_BALANCE = balance;
 * family 0 = conv3d_zmg, 1 = deconv3d_zm (ys = 2: conv7), 2 = the fused tail; out[4] = {balanced?, z segments of the uniform form,
 * its model cost, the balanced cutting's model cost}, the costs in 1/1000 stage. */
int cds_zm_partition(int cols, int planes, int unit, int nwg, int wg, int min_len, int* out);
/* cds_zm_partition for all nwg workgroups at once, up to cap pieces each: out[nwg][1 + 3 cap] = {number of pieces, triples}. */
int cds_zm_partition_all(int cols, int planes, int unit, int nwg, int min_len, int cap, int* out);
int cds_zm_plan(int family, int cols, int planes, int unit, int ys, int ncu, int balance, int* out);


/*
 * K4 (module.py:125-160): ConvTranspose3d k=3, stride 2, padding 1, output_padding 1 (doubles
 * D,H,W) + bias + activation + residual.
 *   weight PACKED [Cin][27][Cout] — PyTorch's transposed-conv layout [Cin][Cout][3][3][3]
 *          permuted (0,2,3,4,1) (no flip: out[2*zi-1+kz] += x[zi]*w[kz]); Cout multiple of 8
 *   x [Cin][D][H][W] -> out [Cout][2D][2H][2W]
 */
int cds_deconv3d_k3s2_f32(const float* x, const float* weight, const float* bias, const float* skip,
                          float* out, int Cin, int Cout, int D, int H, int W, int act, void* stream);

/*
 * Direct 2D convolution (vis CNN model.py:14; FeatureNet branches dynamic_conv.py:112,116;
 * module.py:28-71).  Square kernel k in {1,3,5,7,11} at stride 1, k = 3 at stride 2, zero padding.
 *   x [N][Cin][H][W]; bias [Cout] or NULL; out [N][Cout][Ho][Wo]
 *   weight PACKED [Cin][k*k][CoutP], CoutP = Cout rounded up to a multiple of 8 (zero padded),
 *          cout fastest — PyTorch's [Cout][Cin][k][k] permuted (1,2,3,0)
 */
int cds_conv2d_f32(const float* x, const float* weight, const float* bias, float* out, int N, int Cin,
                   int Cout, int H, int W, int k, int stride, int pad, int act, void* stream);
/*
 * Same convolution with the producing layer's InstanceNorm + LeakyReLU applied on load:
 *   in_affine [N][Cin][3] = (alpha, beta, slope) per image and input channel (device) or NULL; every in-bounds input
 *   value v is replaced by t = v * alpha + beta, t > 0 ? t : t * slope before it is multiplied (zero padding stays zero).
 *   (alpha, beta, slope) = (1, 0, 1) leaves a channel untouched.  Built by cds_instnorm_affine_f32.
 */
int cds_conv2d_affine_f32(const float* x, const float* in_affine, const float* weight, const float* bias, float* out,
                          int N, int Cin, int Cout, int H, int W, int k, int stride, int pad, int act, void* stream);

/*
 * 3x3 convolution, padding 1, 16 -> 16 channels, on the matrix cores: the inner ConvBn2d layers of the visibility CNN
 * (model.py:14, BN folded by the caller).  x [N][16][H][W], W % 4 == 0;
 *   weight_cl [9][16][16] = (tap ky*3+kx, cout, cin)  — PyTorch's [Cout][Cin][3][3] permuted (2,3,0,1);  bias [16] or NULL;
 *   act = CDS_ACT_NONE | CDS_ACT_RELU.
 * head_w / head_b NULL: out [N][16][H][W].  Otherwise (head_w [16], head_b [1], device) the CNN's 1x1 head follows in the
 * same kernel: out [N][H][W] = sigmoid(head_b + sum_c head_w[c] * act(conv + bias)[c])   (nn.Conv2d(16,1,1) + Sigmoid).
 * fp32 inputs and accumulation (v_mfma_f32_16x16x4_f32); the summation order differs from cds_conv2d_f32 (~1e-6).
 */
int cds_conv2d_k3_c16_f32(const float* x, const float* weight_cl, const float* bias, const float* head_w,
                          const float* head_b, float* out, int N, int H, int W, int act, void* stream);

/*
 * K7 on the matrix cores (csrc/conv2d_sbf.hip): ALL branch convolutions of one DynamicConv (models/dynamic_conv.py:112,116:
 * convs[k] and the 3-channel att_convs[k] of every kernel size k, concatenated to Co3 = Cout + 3 output channels per branch)
 * from one staged input tile, stride 1, "same" padding, in split-bf16 arithmetic (every fp32 operand split exactly into three
 * bf16 terms, six error-compensated partial products on v_mfma_f32_16x16x32_bf16, fp32 accumulation: fp32-class error).
 *   x [N][Cin][H][W]; in_affine [N][Cin][3] or NULL (normalise-on-load like cds_conv2d_affine_f32); bias [nb][Co3] or NULL
 *   weight_split: int16 [Cin/8][sum_b ceil(k_b^2/4)][ceil(Co3/16)][3][64][8] (ops.split_pack_dynconv)
 *   out [nb][N][Co3][H][W] (the `branches` tensor of cds_dynconv_blend_*_f32); ksizes: HOST array of nb kernel sizes in {1,3,5,7}
 * Covers Cin % 8 == 0, Co3 <= 48, W % 4 == 0, (nb, ceil(Co3/16)) in {(3,1), (3,2), (2,1), (2,2), (2,3)}; CDS_EINVAL otherwise.
 */
int cds_dynconv_branches_sbf_f32(const float* x, const float* in_affine, const void* weight_split, const float* bias,
                                 float* out, int N, int Cin, int Co3, int H, int W, const int* ksizes, int nb, void* stream);

/* One DynamicConv (models/dynamic_conv.py:97-122) in ONE kernel: the branch convolutions of cds_dynconv_branches_sbf_f32 with
 * the epilogue of cds_dynconv_blend_stats_f32 (epipolar projection of the curvature responses, 1x1 MLP, softmax(./T), blend,
 * InstanceNorm records of the result) applied to the accumulators: the [K][N][Cout + 3] branch tensor never reaches HBM.
 *   out [N][Cout][H][W] (before its InstanceNorm), norm_curv [N][H][W]
 *   partial: 8-byte aligned scratch of 2 * N * parts * Cout doubles, parts = cds_dynconv_fused_parts(H, W); reduce with
 *            cds_instnorm_reduce_f32
 *   w1 [4][K], b1 [4], w2 [K][4]: the attention MLP with its BatchNorm folded in; epipoles [N][2] (DEVICE) (pixels, this resolution)
 * K in {2, 3}, kernel sizes in {1, 3, 5, 7}, Cin % 8 == 0, Cout + 3 <= 48, Cout % 16 <= 13, W % 4 == 0, N <= CDS_MAX_IMAGES. */
int cds_dynconv_fused_sbf_f32(const float* x, const float* in_affine, const void* weight_split, const float* bias,
                              const float* w1, const float* b1, const float* w2, const float* epipoles,
                              float temperature, float* out, float* norm_curv, double* partial, int N, int Cin, int Cout,
                              int H, int W, const int* ksizes, int nb, void* stream);
int cds_dynconv_fused_parts(int H, int W);

/* Visibility-CNN layers 2 and 3 (models/model.py:14: Conv2d 16 -> 16 k3 p1 + BatchNorm(folded) + ReLU; the last one followed by
 * the 1x1 head 16 -> 1 + sigmoid) in split-bf16 arithmetic on the bf16 matrix cores (the same kernel as the DynamicConv
 * branches, one branch).  x [N][Cin][H][W], weight_split = ops.split_pack_dynconv([w]) with w [16][Cin][3][3], bias [16];
 * head_w [16] / head_b [1] or both NULL; out [N][16][H][W], or [N][H][W] with the head.  Cin % 8 == 0, W % 4 == 0. */
int cds_conv2d_k3_relu_sbf_f32(const float* x, const void* weight_split, const float* bias, const float* head_w,
                               const float* head_b, float* out, int N, int Cin, int H, int W, void* stream);

/*
 * FPN lateral connection (module.py:253-254, 260-261): the 1x1 convolution of
 *   cat(interpolate(coarse, scale_factor=2, mode="nearest"), skip)
 * without materialising the up-sampled tensor or the concatenation.
 *   coarse [N][Ca][H/2][W/2], skip [N][Cb][H][W] (H, W even), out [N][Cout][H][W]
 *   weight PACKED [Ca + Cb][CoutP] (coarse channels first, as in the concatenation)
 *   coarse_affine [N][Ca][3] / skip_affine [N][Cb][3]: normalise-on-load tables like cds_conv2d_affine_f32, or NULL.
 * Results are bit-identical to cds_conv2d_affine_f32 (k = 1) on the materialised concatenation.
 *   partial: NULL, or a scratch of 4 * N * cds_fpn_stats_parts(H, W) * Cout floats that receives the per-wave
 *   InstanceNorm records of `out` (as in cds_dynconv_blend_stats_f32; reduce with cds_instnorm_reduce_f32).
 */
int cds_fpn_stats_parts(int H, int W);
int cds_conv2d_fpn_f32(const float* coarse, const float* coarse_affine, const float* skip, const float* skip_affine,
                       const float* weight, float* out, float* partial, int N, int Ca, int Cb, int Cout, int H, int W,
                       void* stream);

/*
 * K7 epilogue of DynamicConv (dynamic_conv.py:97-122) for a batch of N images (each with its own epipole):
 * epipolar projection of the K 3-channel curvature responses, 1x1 MLP (K->4, folded BN, ReLU, 4->K),
 * softmax(./temperature), blend.
 *   branches [K][N][Cout+3][H][W]  per kernel size: the Cout responses of convs[k] followed by the 3 responses of
 *                                  att_convs[k] (one batched cds_conv2d_f32 per size)
 *   w1 [4][K], b1 [4] (BN folded), w2 [K][4]   (device pointers); K in {2,3}
 *   epipoles [N][2] (DEVICE)           (x, y) in pixels of this resolution; N <= CDS_MAX_IMAGES
 *   out [N][Cout][H][W]; norm_curv [N][H][W]
 */
int cds_dynconv_blend_f32(const float* branches, const float* w1, const float* b1, const float* w2,
                          const float* epipoles, float temperature, float* out, float* norm_curv,
                          int N, int K, int Cout, int H, int W, void* stream);
/*
 * Same, when the first n_shared images of the batch are copies of ONE image (the reference image of every pair,
 * model.py:154-161) that only differ in their epipole: the responses of convs[k] / att_convs[k] do not depend on the
 * epipole (dynamic_conv.py:112,116), so they are computed once.
 *   branches [K][N - n_shared + 1][Cout+3][H][W]: slot 0 = the shared image, slot n - n_shared + 1 = image n >= n_shared
 */
int cds_dynconv_blend_shared_f32(const float* branches, const float* w1, const float* b1, const float* w2,
                                 const float* epipoles, float temperature, float* out, float* norm_curv, int N,
                                 int K, int Cout, int H, int W, int n_shared, void* stream);

/*
 * cds_dynconv_blend_shared_f32 that also leaves the InstanceNorm statistics of `out`, so that the normalisation that
 * follows every DynamicConv (module.py:53,66-69) needs no second pass over the tensor.  Every wave writes one
 * (sum, sum of squares) fp64 record per channel of the rounded fp32 outputs:
 *   partial: caller-provided, 8-byte aligned scratch of 4 * N * parts * Cout floats, parts = cds_blend_stats_parts(H, W)
 * cds_instnorm_reduce_f32 adds the records in a fixed order (no atomics: bit-reproducible) into
 *   stats  [N][C][2] doubles (sum, sum of squares) — stored in a float* scratch of 4*N*C floats like cds_instnorm_act_f32's
 *   affine [N][C][3] (alpha, beta, slope) as cds_instnorm_affine_f32 would produce, or NULL
 * cds_instnorm_apply_f32 is the second half of cds_instnorm_act_f32 for given statistics.
 */
int cds_blend_stats_parts(int H, int W);
int cds_dynconv_blend_stats_f32(const float* branches, const float* w1, const float* b1, const float* w2,
                                const float* epipoles, float temperature, float* out, float* norm_curv,
                                float* partial, int N, int K, int Cout, int H, int W, int n_shared, void* stream);
int cds_instnorm_reduce_f32(const float* partial, int parts, float* stats, float* affine, int N, int C, int H, int W,
                            float slope, void* stream);
int cds_instnorm_apply_f32(const float* x, const float* stats, float* out, int N, int C, int H, int W, int act,
                           int out_hwc, void* stream);

/*
 * K8 (module.py:53,66-69,223,230,232): InstanceNorm2d (no affine, eps 1e-5, biased variance) followed by
 * LeakyReLU(0.1) or tanh, for N images.  x [N][C][H][W]; `stats` is a caller-provided, 8-byte aligned scratch of
 * 4*N*C floats (per-(image,channel) fp64 sum and sum of squares).  If out_hwc is non-zero the result is written
 * channels-last [N][H][W][C].
 */
int cds_instnorm_act_f32(const float* x, float* out, float* stats, int N, int C, int H, int W, int act,
                         int out_hwc, void* stream);
/*
 * InstanceNorm statistics only (module.py:53,66-69): affine [N][C][3] = (1/sqrt(var + 1e-5), -mean/sqrt(var + 1e-5), slope)
 * for consumers that normalise on load (cds_conv2d_affine_f32); stats = scratch of 4*N*C floats like cds_instnorm_act_f32.
 */
int cds_instnorm_affine_f32(const float* x, float* affine, float* stats, int N, int C, int H, int W, float slope,
                            void* stream);

/*
 * FeatureNet on CHANNELS-LAST activations (csrc/feat_cl.hip, round 5; models/module.py:234-267, models/dynamic_conv.py:97-122).
 * Every activation is [N][H][W][C] fp32 (a pixel's channels contiguous); normalise-on-load tables [N][C][3] as above; InstanceNorm
 * records [N][parts][C][2] doubles (sum, sum of squares per record) reduced by cds_instnorm_reduce_f32.  The inference runner
 * (cds_mvsnet_amd.model._FeatureRunner) uses these; the planar entry points above remain for the training path and the
 * visibility CNN.
 *
 * cds_dynconv_cl_f32: one DynamicConv (dynamic_conv.py:97-122) in ONE kernel - all branch convolutions on the bf16 matrix cores in
 *   split-bf16 arithmetic as a transposed implicit GEMM (rows = output channels, columns = pixels) + the blend epilogue on the
 *   accumulators + the InstanceNorm records of the result.
 *     x [N][H][W][C], in_affine [N][C][3] or NULL, weight_split = ops.split_pack_dynconv (as cds_dynconv_branches_sbf_f32),
 *     bias [nb][C + 3] or NULL, w1 [4][nb], b1 [4], w2 [nb][4], epipoles [N][2] (DEVICE) (pixels at this resolution)
 *     out [N][H][W][C] (before its InstanceNorm), norm_curv [N][H][W], partial [N][cds_dynconv_cl_parts(H, W)][C][2]
 *   (C, ksizes) in {(8, 3-5-7), (8, 1-3), (16, 3-5), (16, 1-3), (32, 1-3)}, Cin == Cout == C, N <= CDS_MAX_IMAGES.
 * cds_dynconv_blend_cl_f32: the epilogue alone over a PLANAR branch tensor [3][N - n_shared + 1][8 + 3][H][W] (conv00: 3 input
 *   channels, the VALU branch kernels; the first n_shared images share slot 0) -> out [N][H][W][8], norm_curv, partial
 *   [N][cds_blend_cl_parts(H, W)][8][2].
 * cds_conv2d_k3s2_cl_f32: 3x3, stride 2, pad 1, no bias (downsample1 / downsample2): x [N][H][W][Cin] -> out [N][Ho][Wo][Cout],
 *   weight [9][Cin][Cout] (tap = ky * 3 + kx, cout fastest); (Cin, Cout) in {(8, 16), (16, 32)}.
 * cds_conv2d_fpn_cl_f32: FPN lateral, 1x1 convolution of cat(nearest2x(coarse [N][H/2][W/2][Ca]), skip [N][H][W][Cb]) ->
 *   out [N][H][W][Cout]; weight [Ca + Cb][Cout]; partial NULL or [N][cds_fpn_cl_parts(H, W)][Cout][2];
 *   (Ca, Cb, Cout) in {(32, 16, 16), (16, 8, 8)}.
 * cds_instnorm_stats_cl_f32: records of x [N][H][W][C] -> partial [N][cds_instnorm_stats_cl_parts(H, W)][C][2]; C in {8, 16, 32}.
 * cds_instnorm_apply_cl_f32: InstanceNorm + activation for given statistics [N][C][2] doubles: the images n >= cl_from channels-last
 *   into out_cl [N - cl_from][H][W][C] (or NULL), the first n_chw images planar into out_chw [n_chw][C][H][W] (the reference-view
 *   feature maps K1 / K3 read).
 */
/* Debug aid: synchronise the device and fill the LDS of every CU with `pattern` (see csrc/lib.hip; CDS_DEBUG_POISON_LDS=<hex> makes
 * every entry point do this after its launch). */
int cds_debug_poison_lds(unsigned pattern);

int cds_dynconv_cl_parts(int H, int W);
int cds_dynconv_cl_f32(const float* x, const float* in_affine, const void* weight_split, const float* bias, const float* w1,
                       const float* b1, const float* w2, const float* epipoles, float temperature, float* out,
                       float* norm_curv, double* partial, int N, int C, int H, int W, const int* ksizes, int nb, void* stream);
/* The same DynamicConv in SPLIT-F16 arithmetic (two fp16 terms of value x power-of-two scale, three products per K-step; see
 * cds_conv3d_sf16_f32): weight_split from ops.split_pack_dynconv(..., f16=True), w_inv_scale = 1 / its weight scale; x_bound = a HOST
 * number >= max |input after its affine + LeakyReLU| (sqrt(H W) bounds any InstanceNorm-ed map: Samuelson's inequality). */
int cds_dynconv_cl_sf16_f32(const float* x, const float* in_affine, const void* weight_split, const float* bias, const float* w1,
                            const float* b1, const float* w2, const float* epipoles, float temperature, float* out, float* norm_curv,
                            double* partial, int N, int C, int H, int W, const int* ksizes, int nb, float x_bound, float w_inv_scale,
                            void* stream);

/* conv00 of FeatureNet (module.py:209: DynamicConv 3 -> 8, kernel sizes 3 / 7 / 11) in ONE kernel on the matrix cores: x [S][3][H][W]
 * planar images in S = N - n_shared + 1 slots (slot 0 is shown by the first n_shared output images, each with its own epipole),
 * weight_split = ops.split_pack_conv00, bias [3][11] or NULL -> out [N][H][W][8], norm_curv [N][H][W],
 * partial [N][cds_dynconv_cl_parts(H, W)][8][2] doubles. */
int cds_conv00_cl_f32(const float* x, const void* weight_split, const float* bias, const float* w1, const float* b1, const float* w2,
                      const float* epipoles, float temperature, float* out, float* norm_curv, double* partial, int N, int n_shared,
                      int H, int W, void* stream);
/* conv00 in SPLIT-F16 arithmetic (see cds_conv3d_sf16_f32): weight_split from ops.split_pack_conv00(..., f16=True), w_inv_scale = 1 / its
 * weight scale, in_bound a DEVICE scalar >= max |x| (e.g. the images' amax). */
int cds_conv00_cl_sf16_f32(const float* x, const void* weight_split, const float* bias, const float* w1, const float* b1, const float* w2,
                           const float* epipoles, float temperature, float* out, float* norm_curv, double* partial, int N, int n_shared,
                           int H, int W, const float* in_bound, float w_inv_scale, void* stream);

int cds_blend_cl_parts(int H, int W);
int cds_dynconv_blend_cl_f32(const float* branches, const float* w1, const float* b1, const float* w2, const float* epipoles,
                             float temperature, float* out, float* norm_curv, double* partial, int N, int K, int Cout, int H, int W,
                             int n_shared, void* stream);
int cds_conv2d_k3s2_cl_f32(const float* x, const float* in_affine, const float* weight, float* out, int N, int Cin, int Cout, int H,
                           int W, void* stream);
/* The stride-2 units on the matrix cores in SPLIT-F16 arithmetic (round 6): weight_split from ops.split_pack_dynconv([w [Cout,Cin,3,3]],
 * f16=True), w_inv_scale = 1 / its weight scale, x_bound a HOST number >= max |input after its affine + LeakyReLU|. */
int cds_conv2d_k3s2_cl_sf16_f32(const float* x, const float* in_affine, const void* weight_split, float* out, int N, int Cin, int Cout,
                                int H, int W, float x_bound, float w_inv_scale, void* stream);

int cds_fpn_cl_parts(int H, int W);
int cds_conv2d_fpn_cl_f32(const float* coarse, const float* coarse_affine, const float* skip, const float* skip_affine,
                          const float* weight, float* out, double* partial, int N, int Ca, int Cb, int Cout, int H, int W,
                          void* stream);
/* Visibility CNN on channels-last activations (models/model.py:14,51; csrc/feat_cl.hip): layer 1 from the two maps
 * (entropy, ref_nc [V][h][w]; weight packed [2][9][16], bias [16], BatchNorm folded) to [V][h][w][16]; layers 2 / 3 (3x3, 16 -> 16,
 * bias + ReLU, split-bf16 on the matrix cores; weight_split = ops.split_pack_dynconv([w]); with head_w [16] / head_b [1] the 1x1 head
 * + sigmoid follows and out is [N][H][W], else [N][H][W][16]). */
int cds_vis_layer1_cl_f32(const float* entropy, const float* ref_nc, const float* weight, const float* bias, float* out, int V, int H,
                          int W, void* stream);
int cds_conv2d_k3_relu_cl_f32(const float* x, const void* weight_split, const float* bias, const float* head_w, const float* head_b,
                              float* out, int N, int Cin, int H, int W, void* stream);
/* The whole visibility CNN in ONE launch (csrc/vis_rm.hip): a workgroup marches down the rows of a 60-pixel column strip, the two
 * 16-channel activations stay in LDS rings.  Same operands as the three calls above (w0 [2][9][16] / b0 [16]; ws1, ws2 =
 * ops.split_pack_dynconv([w]) with b1, b2 [16]; head_w [16], head_b [1]); out [V][H][W] is bit-equal to theirs.  CDS_VIS_NSEG:
 * number of row segments per strip (A/B and test knob). */
int cds_vis_cnn_rm_f32(const float* entropy, const float* ref_nc, const float* w0, const float* b0, const void* ws1, const float* b1,
                       const void* ws2, const float* b2, const float* head_w, const float* head_b, float* out, int V, int H, int W,
                       void* stream);
int cds_instnorm_stats_cl_parts(int H, int W);
int cds_instnorm_stats_cl_f32(const float* x, double* partial, int N, int C, int H, int W, void* stream);
int cds_instnorm_apply_cl_f32(const float* x, const double* stats, float* out_cl, float* out_chw, int N, int C, int H, int W, int act,
                              int n_chw, int cl_from, void* stream);

/*
 * Depth-map filtering + fusion (fusion.py:7-114, test.py:334-351).  Per reference pixel and source
 * view: re-projection through the source depth map, pixel-distance / relative-depth / in-range tests, average fusion.
 *   ref_depth [h][w]; ref_conf [3][h][w]; src_depths [V][h][w]; src_confs [V][3][h][w] (probability filter
 *   conf_k > prob_thresh_host[k] applied to the source depths and to the final mask)
 *   cams [V][100]: per view Kinv_ref(9) Einv_ref(16) E_src(16) K_src(9) Kinv_src(9) Einv_src(16) E_ref(16) K_ref(9)
 *   fused [h][w], mask [h][w] (0/1), points [3][h][w] (world), view_masks [V][h][w] or NULL
 */
int cds_depth_fusion_f32(const float* ref_depth, const float* ref_conf, const float* src_depths,
                         const float* src_confs, const float* cams, float* fused, float* mask, float* points,
                         float* view_masks, int V, int h, int w, const float* prob_thresh_host,
                         float dist_thresh, float depth_thresh, float view_thresh, void* stream);

/*
 * Depth-map fusion with a dynamic consistency check: the thresholds grow with the number of agreeing views, so
 * tight agreement needs few views and loose agreement needs many.  Inputs, cams layout and probability filter as
 * cds_depth_fusion_f32.  The rule, per reference pixel (px, py) = (x + 0.5, y + 0.5) with reference depth rd:
 *   1. Re-projection, exactly that of cds_depth_fusion_f32, arithmetic included: source depths zeroed where any of the three
 *      confidences is not above its threshold; chain image -> camera -> world -> other camera -> image with +1e-9
 *      normalisations; grid coordinates clamped to +-1.1; in_range_v taken before the sample; the source -> reference
 *      (x, y, depth) map sampled bilinearly (zero padding, align_corners=True), evaluated at the four taps.  Per view v:
 *      (rx, ry, rz)_v and in_range_v.
 *   2. e_v = sqrt((rx - px)^2 + (ry - py)^2);  r_v = |rd - rz_v| / rd  (denominator rd, not max(rd, rz); rd = 0 gives NaN or
 *      inf and every comparison is false).
 *   3. Level l_v = the smallest integer n in [1, n_max] with in_range_v, e_v < (float)n * dist_base and
 *      r_v < (float)n * rel_base (products and comparisons in fp32); n_max + 1 if there is none (inconsistent).
 *   4. c_n = #{v : l_v <= n}.  admit = the smallest n with n_min <= n <= min(n_max, V) and c_n >= n, or 0.  V < n_min admits
 *      nothing; that is not an error.
 *   5. fused = (rd + sum_v rz_v [l_v <= n_max]) / (1 + sum_v [l_v <= n_max]), in view order.
 *   6. mask = (admit > 0) and the reference pixel's three confidences are above their thresholds.
 *   7. points = the world point of the fused depth, as in cds_depth_fusion_f32.
 *   fused [h][w], mask [h][w] (0/1), points [3][h][w] (world); admit [h][w] uint8 or NULL; levels [V][h][w] uint8 or NULL
 *   CDS_EINVAL: a null required pointer; V, h or w < 1; n_min < 1, n_max < n_min or n_max > 16; dist_base or rel_base not > 0.
 */
int cds_depth_fusion_dynamic_f32(const float* ref_depth, const float* ref_conf, const float* src_depths,
                                 const float* src_confs, const float* cams, float* fused, float* mask, float* points,
                                 unsigned char* admit, unsigned char* levels, int V, int h, int w,
                                 const float* prob_thresh_host, float dist_base, float rel_base, int n_min, int n_max,
                                 void* stream);

/*
 * Oriented normals of a depth map (csrc/cloud.hip): an inverse-depth plane fit.  For a plane n.X = rho and
 * X = z Kinv p, 1/z is an affine function g.p of the pixel p = (px, py, 1) and n is proportional to K^T g, so the fit is exact on
 * planes, closed form, and needs no eigen-solver.
 *   depth [h][w] fp32 (z-depth); valid [h][w] uint8 or NULL (every pixel valid); cam_host: 25 floats on the HOST, K 3x3 then
 *   E 4x4 (world -> camera), row-major; normals [3][h][w] fp32 (world frame); ok [h][w] uint8 (0 / 1)
 * The rule, per pixel (x, y):
 *   1. A pixel is valid when valid is non-zero there and its depth is finite and > 0.  A centre that is not valid gets ok = 0 and
 *      the normal (0, 0, 0).
 *   2. Window: the centre has depth dc.  Visit dy = -r..r (outer), dx = -r..r (inner).  A neighbour q enters the fit when it is
 *      inside the image, valid, and |dq - dc| <= jump * dc, evaluated in fp64 from the fp32 values (the difference and the
 *      product of two floats are exact in fp64: the decision is reproducible bit for bit).
 *   3. Over the entering pixels, v = (dx, dy, 1): S = sum v v^T (integers), b = sum v * (1.0 / (double)dq) in fp64 in visiting
 *      order (b0 += (double)dx * inv, b1 += (double)dy * inv, b2 += inv), n = their number.
 *   4. det S and A = adj(S) exactly, in integers; t = A b in fp64, row i as (A[i][0] b0 + A[i][1] b1) + A[i][2] b2.  No
 *      division.  The fitted inverse depth of the centre has the sign of t[2].  The pixel has a normal iff n >= min_pts,
 *      det S != 0 and t[2] > 0.
 *   5. g = (t0, t1, (t2 - t0 px) - t1 py) with (px, py) = (x + 0.5, y + 0.5), the pixel coordinates of the fused point
 *      (store_world_point), so normal and point describe the same ray.  nc = -K^T g: nc[j] = -((K[0][j] g0 + K[1][j] g1) +
 *      K[2][j] g2).  Then nc . (Kinv p) = -t[2] < 0: the normal faces the camera.
 *   6. nw = R^T nc with R = E[:3,:3], nw[j] = (R[0][j] nc0 + R[1][j] nc1) + R[2][j] nc2; norm = sqrt((nw0^2 + nw1^2) + nw2^2);
 *      normal = fp32(nw / norm), one rounding.  A norm that is zero or not finite gives ok = 0 and (0, 0, 0).
 *   ok depends only on integer counts and fp64-exact or fixed-order fp64 expressions: it is the same on every machine.
 *   CDS_EINVAL: a null depth, cam_host, normals or ok; h or w < 1, h * w >= 2^31 or h > 524280; radius outside 1..4;
 *   jump not > 0; min_pts outside 3..(2 radius + 1)^2.
 */
int cds_depth_normals_f32(const float* depth, const unsigned char* valid, const float* cam_host, int h, int w, int radius,
                          float jump, int min_pts, float* normals, unsigned char* ok, void* stream);

/*
 * One attributed point per occupied voxel (csrc/cloud.hip).  Voxels as in cds_voxel_mean_f32: voxel v of n_voxels
 * holds the points perm[start[v] .. start[v + 1]); keys, stable sort and offsets are the caller's.
 *   points [n][3] fp32; colors [n] uint32 packed r | g << 8 | b << 16; normals [n][3] fp32 or NULL (then out_normals is not
 *   written and may be NULL)
 *   out_points [v][3]  the fp64 mean in perm order, rounded once: bit for bit cds_voxel_mean_f32
 *   out_colors [v]     per channel (2 sum + k) / (2 k) in integers (round half up), k the voxel's point count; packed as colors
 *   out_normals [v][3] the fp64 sum of the voxel's normals in perm order, divided by its norm sqrt((sx^2 + sy^2) + sz^2) and
 *                      rounded once; (0, 0, 0) when the norm is zero or not finite.  Opposing faces inside one voxel are not
 *                      separated.
 *   out_counts [v]     k, int32
 *   CDS_EINVAL: n or n_voxels < 0, n_voxels > n, n >= 2^31, a null required pointer (n_voxels == 0 returns 0 first).
 */
int cds_voxel_merge_f32(const float* points, const unsigned* colors, const float* normals, long long n, const long long* perm,
                        const int* start, long long n_voxels, float* out_points, unsigned* out_colors, float* out_normals,
                        int* out_counts, void* stream);

/*
 * Sparse TSDF fusion and tetrahedra extraction: a triangle mesh from the fused depth maps (csrc/tsdf.hip).
 *
 * Frame.  voxel s > 0, truncation T with s <= T <= 8 s, both doubles.  Lattice point (i, j, k) lies at
 *   X[a] = origin[a] + (double)idx[a] * s  (fp64).  Blocks are 8 x 8 x 8 lattice points; B = 8.0 * s.
 *   From the kept points of the scan (fp32, lo / hi their per-axis minimum / maximum):
 *     origin[a] = (floor((double)lo[a] / B) - 1.0) * B,   nb[a] = (int)floor(((double)hi[a] - origin[a]) / B) + 2.
 *   The block of a point is floor(((double)p[a] - origin[a]) / B) per axis; it lies in 0 .. nb[a] - 2.
 *   nb[0] nb[1] nb[2] <= CDS_TSDF_MAX_CELLS, else the voxel is too small for the scan.
 *   Block key = (bz nb[1] + by) nb[0] + bx; local index of a point in its block = (lz 8 + ly) 8 + lx.
 * Allocation.  A block exists iff it holds a kept point or is one of the 26 neighbours of such a block and lies inside the
 *   grid.  Blocks are stored in ascending key order: keys [n_blocks] int32; table [nb[2]][nb[1]][nb[0]] int32 gives a block's
 *   position in keys, or -1.  Since T <= 8 s, the band of +-T along every kept ray lies in existing blocks.
 * Storage, [n_blocks][512] each: sum fp32, n int32, nc int32; rgb int32 [3][n_blocks][512].
 *
 * Integration of one lattice point X over the views in the order given, in fp64 from the fp32 camera entries
 *   (cams [n_views][24] doubles: R 0..8 and t 9..11 the rows of E = [R | t] world -> camera, K 12..20 row-major, 21 the largest
 *   depth of the view that passes step 4, -inf if none; 22, 23 unused):
 *   1. Xc[r] = ((R[r][0] X0 + R[r][1] X1) + R[r][2] X2) + t[r];  z = Xc[2];  skip the view unless z > 0.
 *   2. p[r] = (K[r][0] Xc0 + K[r][1] Xc1) + K[r][2] Xc2;  u = p0 / p2,  v = p1 / p2.
 *   3. x = floor(u), y = floor(v): pixel x covers [x, x + 1), its centre is x + 0.5 (the convention of the fused points).
 *      Skip the view unless 0 <= u < w and 0 <= v < h (false for NaN).
 *   4. d = depths[view][y][x].  Skip if masks[view][y][x] == 0, or d is not finite, or d <= 0.
 *   5. sdf = (double)d - z.  Skip if sdf < -T.  tv = (float)min(1.0, sdf / T).
 *   6. sum = sum + tv, one fp32 add per view, in view order;  n += 1.
 *   7. If sdf <= T: rgb += images[view][y][x][0..2] (uint8) and nc += 1.
 *   Every observation weighs 1.  A view is skipped for a whole block only when no point of the block could pass steps 1, 3 and 5
 *   (bounding sphere against the frustum planes and entry 21); that never changes a result.
 *
 * Extraction, with min_weight >= 1.
 *   A point is valid iff it exists and n >= min_weight; it is inside iff sum < 0 (no division enters a decision).
 *   A cube (lower corner L, corners L + {0,1}^3) is processed iff its 8 corners are valid.  It is split into the six tetrahedra
 *   000 -> e_a -> e_a + e_b -> 111 over the axis orders (a, b, c) in lexicographic order: (x,y,z) (x,z,y) (y,x,z) (y,z,x) (z,x,y)
 *   (z,y,x); tetrahedron corners v0..v3 along the path.  Every tetrahedron edge joins nested corners, so it is a lattice edge
 *   with a lower point A and an offset of one of seven kinds, in this order: x, y, z, xy, xz, yz, xyz.
 *   Vertices.  Edge (A, kind) carries a vertex iff exactly one of its ends is inside and some processed cube has it as an edge
 *   (the cubes with lower corner A - o, o a corner offset that shares no axis with the kind).  Da = (double)sum_A / (double)n_A,
 *   Db likewise for the upper end B;  tt = Da / (Da - Db);  P[a] = (float)(XA[a] + tt * (XB[a] - XA[a])).
 *   Colour per channel: c_A = (2 rgb_A + nc_A) / (2 nc_A) in integers when nc_A > 0, else c_B; c_B likewise;
 *   colour = clamp(floor(((double)c_A + tt * (double)(c_B - c_A)) + 0.5), 0, 255); 128 when nc_A = nc_B = 0.
 *   Triangles of a tetrahedron, case = the set of inside corners:
 *     one corner i inside or one corner i outside, the others j < k < l: (ij, ik, il);
 *     i < j inside and k < l outside: the quadrilateral q = (ik, il, jl, jk) as (q0, q1, q2), (q0, q2, q3), in this order.
 *   Each triangle is wound so that its normal points to the outside (the positive, camera-facing side); the other winding
 *   swaps the second and third vertex.  The winding is a function of the case and of the parity of the axis order alone.
 *   A point with sum == 0 is outside; its edges' vertices coincide with it and give zero-area triangles, which are kept.
 *   Order.  Vertices by (block key, local index of A, kind); faces by (block key, local index of L, tetrahedron, triangle).
 *
 * cds_tsdf_integrate_f32: depths [n_views][h][w] fp32, masks uint8, images [n_views][h][w][3] uint8; frame_host: 4 doubles on the
 *   HOST (origin, s); dims_host: 3 ints on the HOST (nb).  Adds n_views views to the accumulators.
 *   CDS_EINVAL: a null frame_host / dims_host, a frame that is not finite, s <= 0, nb < 1 or more than CDS_TSDF_MAX_CELLS cells;
 *   n_blocks < 0 or > CDS_TSDF_MAX_CELLS; n_views outside 1..CDS_TSDF_MAX_CHUNK; h or w < 1; n_views h w >= 2^31; T outside [s, 8 s];
 *   a null device pointer (n_blocks == 0 returns 0 first).
 * cds_tsdf_classify: vmask [n_blocks][512] uint8 (bit k: the point's edge of kind k carries a vertex), tcount [n_blocks][512]
 *   uint8 (triangles of the point's cube), block_vertices / block_faces [n_blocks] int32 (their sums per block).
 *   CDS_EINVAL: the frame cases above; min_weight < 1; a null pointer.
 * cds_tsdf_emit: block_vstart / block_tstart [n_blocks] int32: the exclusive prefix sums of block_vertices / block_faces;
 *   n_vertices / n_faces their totals; vstart [n_blocks][512] int32 scratch (the first vertex of every point);
 *   vertices [n_vertices][3] fp32, colors [n_vertices][3] uint8, faces [n_faces][3] int32.
 *   CDS_EINVAL: the frame cases above; a total < 0 or >= 2^31; a null pointer (outputs may be null when their total is 0).
 */
#define CDS_TSDF_MAX_CHUNK 32
#define CDS_TSDF_MAX_CELLS (1 << 26)
int cds_tsdf_integrate_f32(const int* keys, long long n_blocks, const double* frame_host, const int* dims_host, double trunc,
                           const float* depths, const unsigned char* masks, const unsigned char* images, const double* cams,
                           int n_views, int h, int w, float* sum, int* n, int* nc, int* rgb, void* stream);
int cds_tsdf_classify(const int* keys, const int* table, long long n_blocks, const double* frame_host, const int* dims_host,
                      const float* sum, const int* n, int min_weight, unsigned char* vmask, unsigned char* tcount,
                      int* block_vertices, int* block_faces, void* stream);
int cds_tsdf_emit(const int* keys, const int* table, long long n_blocks, const double* frame_host, const int* dims_host,
                  const float* sum, const int* n, const int* nc, const int* rgb, const unsigned char* vmask,
                  const unsigned char* tcount, const int* block_vstart, const int* block_tstart, long long n_vertices,
                  long long n_faces, int* vstart, float* vertices, unsigned char* colors, int* faces, void* stream);

/*
 * Weighted TSDF fusion: a weight per pixel and a depth interpolated between pixels (csrc/tsdf.hip).
 *
 * cds_tsdf_view_weights: the weight map of one view.
 *   depth [h][w] fp32; mask [h][w] uint8; normals [3][h][w] fp32 (world frame) with ok [h][w] uint8, as cds_depth_normals_f32
 *   writes them when called with valid = mask, both NULL or both set; conf [h][w] fp32 or NULL; cam_host: the 25 HOST floats
 *   of cds_depth_normals_f32 (K 3x3, then E 4x4); weights [h][w] uint8.
 *   The rule, per pixel (x, y), in fp64 from the fp32 values, bracketed as written:
 *   1. K has the rows (fx, s, cx), (0, fy, cy), (0, 0, 1); R = E[:3,:3].
 *   2. weights = 0 where mask is 0 or the depth is not finite or is <= 0.
 *   3. Angle term a: 1 when normals is NULL; 0 where ok is 0; else, with the camera-frame ray through the pixel centre
 *        c1 = ((y + 0.5) - cy) / fy,  c0 = (((x + 0.5) - cx) - s c1) / fx,  c2 = 1,
 *      and the camera-frame normal nc[r] = (R[r][0] n0 + R[r][1] n1) + R[r][2] n2,
 *        a = -((nc0 c0 + nc1 c1) + nc2) / sqrt((c0 c0 + c1 c1) + 1.0),
 *      the cosine between the normal and the direction to the camera.  A value that is not finite or is below 0 gives 0, a
 *      value above 1 gives 1.
 *   4. Confidence term c: 1 when conf is NULL, else conf clamped to [0, 1]; NaN gives 0.
 *   5. weights = min(255, max(1, (int)floor(255.0 * (a * c) + 0.5))): a kept pixel weighs at least 1, so it still counts
 *      towards min_weight; grazing pixels and pixels without a normal get that minimum.
 *   Division and sqrt are the correctly rounded fp64 operations.
 *   CDS_EINVAL: a null depth, mask, cam_host or weights; normals without ok or ok without normals; h or w < 1, h w >= 2^31;
 *   a K whose last row is not (0, 0, 1) or whose K[1][0] is not 0.
 *
 * cds_tsdf_integrate_w_f32: cds_tsdf_integrate_f32 with weights [n_views][h][w] uint8 or NULL (every kept pixel weighs 1),
 *   interp (0 / non-zero), jump, and wn [n_blocks][512] int32, the sum of the weights, set iff weights is.
 *   Per lattice point and view, steps 1-4 of the integration above give u, v, the nearest pixel q = (x, y) and its depth d. Then
 *   4a. wq = weights ? weights[view][y][x] : 1.  Skip the view if wq == 0.
 *   4b. dd = (double)d, unless interp is set and all of this holds, then dd = 1.0 / i:
 *       a = u - 0.5, b = v - 0.5, x0 = floor(a), y0 = floor(b), fx = a - x0, fy = b - y0 (pixel centres lie at x + 0.5);
 *       x0 >= 0, x0 + 1 < w, y0 >= 0, y0 + 1 < h;
 *       the pixels (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), depths d00 d10 d01 d11, all have a non-zero mask and
 *       a finite depth > 0 (their weights are not looked at);
 *       with lo / hi the smallest / largest of the four, (double)hi - (double)lo <= (double)jump * (double)lo;
 *       i00 = 1.0 / (double)d00 and so on;  i0 = i00 + fx (i10 - i00),  i1 = i01 + fx (i11 - i01),  i = i0 + fy (i1 - i0).
 *       1 / z is affine in the pixel for a plane (the fact cds_depth_normals_f32 uses), so dd is exact on planes up to the
 *       rounding of the fp32 depths.  q is always one of the four; the mask test, the weight and the colour stay its own.
 *   5.  sdf = dd - z.  Skip if sdf < -T.
 *   6.  sum = sum + (float)((double)wq * min(1.0, sdf / T)), one fp32 add per view, in view order;  n += 1;  wn += wq.
 *   7.  As above: colours are not weighted and come from q.
 *   With weights NULL and interp 0 the accumulators get the bits of cds_tsdf_integrate_f32.
 *   Extraction of a weighted volume: cds_tsdf_classify reads n (valid iff n >= min_weight views), cds_tsdf_emit takes wn in the
 *   place of n, so that Da = sum / wn.  inside iff sum < 0 stands, because the weights are positive.
 *   CDS_EINVAL: the cases of cds_tsdf_integrate_f32; weights without wn or wn without weights; interp != 0 with a jump that is
 *   not finite or not > 0.
 */
int cds_tsdf_view_weights(const float* depth, const unsigned char* mask, const float* normals, const unsigned char* ok,
                          const float* conf, const float* cam_host, int h, int w, unsigned char* weights, void* stream);
int cds_tsdf_integrate_w_f32(const int* keys, long long n_blocks, const double* frame_host, const int* dims_host, double trunc,
                             const float* depths, const unsigned char* masks, const unsigned char* images, const double* cams,
                             int n_views, int h, int w, float* sum, int* n, int* nc, int* rgb, const unsigned char* weights,
                             int interp, float jump, int* wn, void* stream);

/*
 * Rendering a triangle mesh into the views of a scan: depth, face, facing and colour per pixel (csrc/raster.hip).
 *
 * Inputs.  vertices fp32 [n_vertices][3], faces int32 [n_faces][3], optional colours uint8 [n_vertices][3]; per view
 *   cams [CDS_RASTER_CAM] doubles: R 0..8 and t 9..11 the rows of E = [R | t] world -> camera, then fx 12, s 13, cx 14, fy 15,
 *   cy 16 of K = [[fx, s, cx], [0, fy, cy], [0, 0, 1]] (the host refuses another K); 17.. unused.  A map of h x w pixels.
 *   All arithmetic is fp64 from the fp32 entries, bracketed as written; decisions on snapped coordinates are exact in int64.
 * 1. Vertex.  Xc[r] = ((R[r][0] X0 + R[r][1] X1) + R[r][2] X2) + t[r];  z = Xc[2].
 *      u = ((fx Xc0 + s Xc1) + cx z) / z,  v = (fy Xc1 + cy z) / z.  Pixel x covers [x, x + 1), its centre is x + 0.5.
 *      X = floor(u * 256 + 0.5), Y = floor(v * 256 + 0.5) as int64.
 *      The vertex is usable iff z > 0, u and v are finite, |X| < 2^28 and |Y| < 2^28.
 * 2. Face (a, b, c) with snapped corners 0, 1, 2.  Drawn iff its three vertices are usable and
 *      A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) != 0.  No clipping: a face with an unusable vertex is dropped whole.
 * 3. Coverage.  Q = (256 px + 128, 256 py + 128), g = sign(A).  For every edge i -> j, j = (i + 1) mod 3:
 *      dx = g (Xj - Xi), dy = g (Yj - Yi), E = dx (Qy - Yi) - dy (Qx - Xi).
 *      The pixel is covered iff for all three edges E > 0, or E == 0 and (dy < 0 or (dy == 0 and dx > 0)) (top-left).
 *      Candidates: the pixels of the map with min X <= Qx <= max X and min Y <= Qy <= max Y.
 * 4. Depth, from the face's plane in camera space.  n = (Xc_b - Xc_a) x (Xc_c - Xc_a), each component as p q - r s
 *      (n0 = e1[1] e2[2] - e1[2] e2[1], cyclic);  d = (n0 Xa0 + n1 Xa1) + n2 Xa2.
 *      ry = ((py + 0.5) - cy) / fy,  rx = (((px + 0.5) - cx) - s ry) / fx,  den = (n0 rx + n1 ry) + n2,  zf = d / den.
 *      The fragment exists iff zf is finite and zf > 0.  front = d < 0: the face's own winding looks at the camera.
 * 5. Visibility.  key = ((uint64)bits((float)zf) << 32) | face index; the pixel takes the minimum key over its fragments: the
 *      nearest depth, the lowest face index on a tie.  The minimum does not depend on any order.
 * 6. Outputs per view: depth fp32 (the key's upper word; 0 without a hit), face int32 (-1 without a hit), front uint8,
 *      valid uint8 = hit and front, and, with colours, image uint8 [h][w][3] (0 without a hit):  P = zf (rx, ry, 1) with the zf
 *      of rule 4 for the winning face,  w_a = n . ((Xc_b - P) x (Xc_c - P)) / (n . n), w_b from (c, a), w_c from (a, b), the
 *      cross products as in 4 and every dot product as (x0 y0 + x1 y1) + x2 y2;
 *      channel = floor(clamp((w_a c_a + w_b c_b) + w_c c_c, 0, 255) + 0.5), with clamp(NaN) = 0.
 *
 * cds_raster_project: xy [n_views][n_vertices][2] int32 (X, Y; both INT_MIN for an unusable vertex), xc [n_views][n_vertices][3]
 *   doubles (Xc).
 * cds_raster_faces: keys [n_views][h][w] uint64, filled with all ones by the caller before the first launch; rules 2-5 for every
 *   face with at most large_px candidates; large [n_views][n_faces] uint8 is written for EVERY (view, face): 1 for a drawn face
 *   with more candidates, which is NOT drawn here, else 0.
 * cds_raster_large: list [n_list] int64 of entries view * n_faces + face; one wave draws one entry, whatever its size.
 *   The result of faces + large over the marked entries does not depend on large_px.
 * cds_raster_resolve: rule 6; colors and image may both be null.
 *   CDS_EINVAL: n_vertices or n_faces < 0 or >= 2^31; n_views outside 1..CDS_RASTER_MAX_CHUNK; h or w < 1; h w >= 2^31;
 *   large_px < 1; n_list < 0 or > CDS_RASTER_MAX_LIST; a null required pointer (an empty mesh or list returns 0 first, except in
 *   resolve, which then writes the all-miss outputs).  A face index outside the vertices drops the face; nothing is read there.
 */
#define CDS_RASTER_CAM 24
#define CDS_RASTER_MAX_CHUNK 32
#define CDS_RASTER_MAX_LIST (1ll << 30)
int cds_raster_project(const float* vertices, long long n_vertices, const double* cams, int n_views, int* xy, double* xc,
                       void* stream);
int cds_raster_faces(const int* faces, long long n_faces, long long n_vertices, const double* cams, int n_views, const int* xy,
                     const double* xc, int h, int w, long long large_px, unsigned long long* keys, unsigned char* large,
                     void* stream);
int cds_raster_large(const long long* list, long long n_list, const int* faces, long long n_faces, long long n_vertices,
                     const double* cams, int n_views, const int* xy, const double* xc, int h, int w, unsigned long long* keys,
                     void* stream);
int cds_raster_resolve(const unsigned long long* keys, const int* faces, long long n_faces, long long n_vertices,
                       const double* cams, int n_views, const double* xc, const unsigned char* colors, int h, int w, float* depth,
                       int* face, unsigned char* front, unsigned char* valid, unsigned char* image, void* stream);

/*
 * Connected components of a triangle mesh and the removal of the small ones (csrc/mesh_clean.hip).
 *
 * Inputs.  faces int32 [n_faces][3] over n_vertices vertices, every index in [0, n_vertices) (the host refuses another mesh; a
 *   kernel skips such a face and reads nothing there).  Everything below is integer arithmetic; nothing depends on any order.
 * 1. Connectivity.  Two vertices are connected when some face holds both; a component is a class of the transitive closure.
 *      Two sheets that share a single vertex are one component (vertex, not edge, adjacency).  A face with a repeated index
 *      (a, a, b) still connects a and b.  A duplicate face is a face like any other.
 * 2. Label.  label[v] = the smallest vertex index of v's component.  A vertex in no face is a component of its own, with 0 faces.
 * 3. Size.  A face belongs to the component of its first vertex; count[c] = the number of faces of the component with label c.
 *      Nothing else measures a component (no area: no floating-point sum enters a decision).
 * 4. Selection, with min_faces >= 0 and keep_largest >= 0.  A component is kept iff count >= min_faces and, when
 *      K = keep_largest > 0, it is among the first K components in the order (count descending, label ascending) of ALL
 *      components.  keep_largest = 0 sets no limit.
 * 5. Output.  The kept faces (those of kept components) in their order; the vertices that some kept face holds, in their order,
 *      numbered 0, 1, ...; the rows of vertices and colors copied bit for bit; the faces rewritten to the new numbers.  A vertex in
 *      no kept face is dropped.  With min_faces <= 1 and keep_largest = 0 a mesh whose every vertex lies in a face comes back as
 *      it was.
 *
 * The labels come from a union-find over parent int32 [n_vertices] with parent[x] <= x at all times:
 * cds_mesh_cc_init: parent[v] = v.
 * cds_mesh_cc_hook: one pass over the faces: the roots of a face's vertices, the larger ones lowered to the smallest by atomicMin;
 *   *changed (a device word the caller zeroed) is set to 1 when the pass lowered any word.
 * cds_mesh_cc_jump: parent[v] = the root above v.  The caller repeats hook and jump until a hook leaves *changed at 0, at most
 *   CDS_MESH_CC_MAX_ROUNDS times; then parent is the label of rule 2.  A caller that reaches the limit must report an error and
 *   must not use parent.
 * cds_mesh_cc_count: count [n_vertices] int32, zeroed by the caller: rule 3 (count[c] for c a label, 0 elsewhere).
 * cds_mesh_cc_mark: keep [n_vertices] uint8 indexed by label (rule 4, made by the caller); face_keep [n_faces] uint8 is written
 *   for every face; vertex_keep [n_vertices] uint8, zeroed by the caller, is set to 1 for the vertices of kept faces.
 * cds_mesh_cc_gather: rule 5.  vertex_new / face_new: the exclusive prefix sums of vertex_keep / face_keep, int32; out_vertices /
 *   out_faces their totals; colors and colors_out may both be null.
 *   CDS_EINVAL: n_vertices or n_faces < 0 or >= 2^31; a total larger than its input; a null required pointer (an empty input or
 *   output returns 0 first).
 */
#define CDS_MESH_CC_MAX_ROUNDS 64
int cds_mesh_cc_init(int* parent, long long n_vertices, void* stream);
int cds_mesh_cc_hook(const int* faces, long long n_faces, long long n_vertices, int* parent, int* changed, void* stream);
int cds_mesh_cc_jump(int* parent, long long n_vertices, void* stream);
int cds_mesh_cc_count(const int* faces, long long n_faces, long long n_vertices, const int* label, int* count, void* stream);
int cds_mesh_cc_mark(const int* faces, long long n_faces, long long n_vertices, const int* label, const unsigned char* keep,
                     unsigned char* face_keep, unsigned char* vertex_keep, void* stream);
int cds_mesh_cc_gather(const float* vertices, const unsigned char* colors, const int* faces, long long n_vertices,
                       long long n_faces, const unsigned char* vertex_keep, const int* vertex_new, const unsigned char* face_keep,
                       const int* face_new, long long out_vertices, long long out_faces, float* vertices_out,
                       unsigned char* colors_out, int* faces_out, void* stream);

/*
 * Simplification of a triangle mesh: vertex clustering with quadric placement (csrc/mesh_simplify.hip).
 *
 * Inputs.  vertices float32 [V][3], all finite; colors uint8 [V][3]; faces int32 [F][3], every index in [0, V) (the host refuses
 *   another mesh; a kernel skips such a face and reads nothing there); cell > 0, finite; placement "quadric" or "mean".
 * 1. Cells.  The cells of cds_voxel_merge_f32 as pointcloud.voxel_groups(vertices, cell) lays them out: origin
 *      float32(min - cell / 2), index floorf((p - o) / cell) in fp32, the grid's key packing.  Cluster c is the c-th occupied cell
 *      in ascending key order; its members perm[start[c] .. start[c + 1]) are ascending vertex indices; k_c is their number.
 * 2. Mean and colour.  S_c: the fp64 sum of the members' positions in member order; m_c = S_c / k_c in fp64.  The colour is
 *      (2 sum + k) / (2 k) per channel in integers.  fp32(m_c) and the colour are what cds_voxel_merge_f32 returns; with
 *      placement "mean" the position is fp32(m_c), that kernel's bits.
 * 3. Quadric.  The incidences of cluster c are the pairs (f, j) with cluster(faces[f][j]) == c in ascending (f, j); a face with
 *      two corners in c appears twice.  Per face, with p_i = (double)vertices[faces[f][i]]: e1 = p1 - p0, e2 = p2 - p0,
 *      n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), w2 = (nx nx + ny ny) + nz nz; a face whose w2 is zero or
 *      not finite contributes nothing.  Per incidence: q = p0 - m_c, d = (nx qx + ny qy) + nz qz; A00 += nx nx, A01 += nx ny,
 *      A02 += nx nz, A11 += ny ny, A12 += ny nz, A22 += nz nz, b += n d per component; nine sequential fp64 sums in incidence
 *      order.  The weight is the squared area: no square root and no division enters a sum.
 * 4. Solve, regularised towards the mean.  tr = (A00 + A11) + A22; lam = tr 2^-10; M = A + lam I.  Cofactors, each one
 *      difference of two products: c00 = M11 M22 - A12 A12, c01 = A02 A12 - A01 M22, c02 = A01 A12 - A02 M11,
 *      c11 = M00 M22 - A02 A02, c12 = A01 A02 - M00 A12, c22 = M00 M11 - A01 A01.  det = (M00 c00 + A01 c01) + A02 c02.
 *      y_i = ((C_i0 b0 + C_i1 b1) + C_i2 b2) / det.  The position is fp32(m_c + y), per component.  The cluster FALLS BACK to
 *      fp32(m_c) unless tr is finite and > 0, det is finite and > 0, y is finite and max |y_i| <= (double)cell, with cell the
 *      fp32 value the cells were made with.  All fp64, no contraction (-ffp-contract=off).
 * 5. Faces.  A face is mapped corner by corner to clusters.  It is COLLAPSED, and dropped, when two corners share a cluster.
 *      The identity of another face is its triple rotated so that the smallest cluster comes first (unique: the clusters are
 *      distinct; the winding is kept).  A face is a DUPLICATE, and dropped, when a face with a lower index has the same identity.
 *      Two faces over the same clusters with opposite winding both stay.
 * 6. Output.  The surviving faces in their order, corners in their original order; the clusters some surviving face holds in
 *      ascending key order, numbered densely, with positions and colours.  A cluster in no surviving face is dropped.
 *
 * cds_mesh_simplify_faces: rule 5 per face.  cluster int32 [n_vertices]: the cluster of every vertex.  Writes face_clusters
 *   int32 [n_faces][3], collapsed uint8 [n_faces] and identity int32 [n_faces][3].  A face with an index outside the vertices, or
 *   a cluster outside [0, n_clusters), is written as collapsed with the clusters -1.  The caller finds the duplicates (a stable
 *   sort of the identities on the device: the first of a run is the lowest index).
 * cds_mesh_simplify_quadric_f32: rules 2-4.  perm int64 [n_vertices] and start int32 [n_clusters + 1] as voxel_groups returns
 *   them; inc int64 [3 n_faces]: the corners 3 f + j sorted by their cluster, stable; inc_start int32 [n_clusters + 1].  Writes
 *   out_positions float32 [n_clusters][3] and out_fallback uint8 [n_clusters].  An offset or index outside its array is skipped.
 * cds_mesh_simplify_mark: cluster_keep uint8 [n_clusters], zeroed by the caller, is set to 1 for the clusters of the faces with
 *   face_keep != 0.
 * cds_mesh_simplify_gather: rule 6.  positions float32 [n_clusters][3]; colors: the packed words of cds_voxel_merge_f32, or null
 *   (then colors_out is not written); cluster_new / face_new: the exclusive prefix sums of cluster_keep / face_keep, int32;
 *   out_vertices / out_faces their totals.  It is cds_mesh_cc_gather's rule 5 with positions as vertices, face_clusters as
 *   faces and n_clusters as n_vertices: one kernel serves both, and only the colour source differs.
 *   CDS_EINVAL: a count < 0 or >= 2^31; 3 n_faces >= 2^31 (quadric); n_clusters > n_vertices; cell not finite or <= 0; a total
 *   larger than its input; a null required pointer (an empty input or output returns 0 first).
 */
int cds_mesh_simplify_faces(const int* faces, long long n_faces, long long n_vertices, const int* cluster, long long n_clusters,
                            int* face_clusters, unsigned char* collapsed, int* identity, void* stream);
int cds_mesh_simplify_quadric_f32(const float* vertices, long long n_vertices, const int* faces, long long n_faces,
                                  const long long* perm, const int* start, const long long* inc, const int* inc_start,
                                  long long n_clusters, float cell, float* out_positions, unsigned char* out_fallback,
                                  void* stream);
int cds_mesh_simplify_mark(const int* face_clusters, const unsigned char* face_keep, long long n_faces, long long n_clusters,
                           unsigned char* cluster_keep, void* stream);
int cds_mesh_simplify_gather(const float* positions, const unsigned* colors, long long n_clusters,
                             const unsigned char* cluster_keep, const int* cluster_new, const int* face_clusters, long long n_faces,
                             const unsigned char* face_keep, const int* face_new, long long out_vertices, long long out_faces,
                             float* vertices_out, unsigned char* colors_out, int* faces_out, void* stream);

/*
 * Smoothing of a triangle mesh: the Taubin lambda|mu filter with uniform weights (csrc/mesh_smooth.hip).  Only the
 * vertex positions change; faces, colours, counts and order stay bit for bit.
 *
 * Inputs.  vertices float32 [V][3], all finite; faces int32 [F][3]; iterations in 1..1000; lam in (0, 1]; mu in [-1, 0];
 *   max_move >= 0, finite.
 * 1. Valid faces and edges.  A face is valid when its three indices are in [0, V); another is skipped.  A valid face has three
 *      edge slots (0,1), (1,2), (2,0); a slot whose two corners are equal is dropped.  The multiplicity of the undirected edge
 *      {i,j} is the number of slots over all valid faces that hold it.
 * 2. Boundary.  An edge of multiplicity 1 is a boundary edge; a vertex with at least one boundary edge is a boundary vertex.
 * 3. Neighbours.  N(i) of an interior vertex: the distinct j with an edge {i,j}.  N(i) of a boundary vertex: only the j whose
 *      edge {i,j} is a boundary edge, so an open border relaxes along itself and is never pulled inward.  A vertex with an empty
 *      N(i) (in no face, or only in slots that were dropped) is ISOLATED and keeps its bits.
 * 4. One step with the factor s (Jacobi: every vertex reads the positions from before the step).  Per coordinate,
 *      m_i = (sum over j in N(i), ascending j, of (double)p_j) / (double)|N(i)|, the sum sequential in fp64 from +0.0;
 *      p_i' = (float)((double)p_i + s * (m_i - (double)p_i)), in that operation order: one round-to-nearest-even cast per step,
 *      no contraction (-ffp-contract=off).  Positions are fp32 between steps.
 * 5. One iteration: a step with lam, then, unless mu == 0, a step with mu.  mu == 0 is the plain Laplacian filter.
 * 6. max_move = D > 0, once after the last iteration, against the input positions p0: d = (double)p - (double)p0,
 *      n2 = (dx dx + dy dy) + dz dz; where n2 > D D: p = (float)(p0 + d * (D / sqrt(n2))) per coordinate.  D == 0: no limit.
 * 7. Statistics.  n2 of rule 6, taken before the clamp, per vertex; the caller takes its maximum (a maximum does not depend
 *      on the order) and counts the clamped, boundary and isolated vertices.
 *
 * The adjacency is a CSR with slack: start int32 [V + 1], the exclusive prefix sum of the entries each vertex receives (two per
 * kept slot, one at either end); vertex v owns nbr[start[v] .. start[v + 1]) and, after cds_mesh_adj_finish, its first deg[v]
 * entries are N(v), ascending.  n_entries = start[V] <= 6 F.
 * cds_mesh_adj_small: CDS_MESH_ADJ_SMALL.
 * cds_mesh_adj_count: count int32 [V], zeroed by the caller: the entries of each vertex (integer atomics).
 * cds_mesh_adj_fill: cursor int32 [V], zeroed by the caller; writes the other end of every kept slot into the segment of each end.
 *   The order inside a segment is the hardware's; cds_mesh_adj_finish removes it.  An entry past its segment is not written.
 * cds_mesh_adj_finish: one thread per vertex sorts its segment when it has at most CDS_MESH_ADJ_SMALL entries (the caller has
 *   sorted every longer segment ascending: there are few, and one sort of just their entries serves them all), reads the
 *   multiplicity of {v,j} off the run of j, applies rules 2 and 3 in place and writes deg int32 [V] and flags uint8 [V]
 *   (CDS_MESH_ADJ_BOUNDARY | CDS_MESH_ADJ_ISOLATED).  A vertex whose offsets lie outside [0, n_entries] is written as isolated.
 * cds_mesh_smooth_step_f32: rule 4 from `in` to `out`, float32 [V][3] each, in != out.  A vertex with deg 0, with a segment outside
 *   [start[v], start[v + 1]] or with a neighbour outside [0, V) copies its bits.
 * cds_mesh_smooth_limit_f32: rules 6 and 7.  original: p0; vertices: p, clamped in place; move2_out fp64 [V]; clamped_out uint8 [V].
 *   CDS_EINVAL: a count < 0 or >= 2^31; 3 n_faces 2 >= 2^31 entries; n_entries > 6 n_faces; in == out or original == vertices; a
 *   factor that is not finite; max_move negative or not finite; a null required pointer (an empty input returns 0 first).
 */
#define CDS_MESH_ADJ_SMALL 64
#define CDS_MESH_ADJ_BOUNDARY 1
#define CDS_MESH_ADJ_ISOLATED 2
int cds_mesh_adj_small(void);
int cds_mesh_adj_count(const int* faces, long long n_faces, long long n_vertices, int* count, void* stream);
int cds_mesh_adj_fill(const int* faces, long long n_faces, long long n_vertices, const int* start, int* cursor, int* nbr,
                      long long n_entries, void* stream);
int cds_mesh_adj_finish(long long n_vertices, const int* start, int* nbr, long long n_entries, int* deg, unsigned char* flags,
                        void* stream);
int cds_mesh_smooth_step_f32(const float* in, float* out, long long n_vertices, const int* start, const int* deg, const int* nbr,
                             double factor, void* stream);
int cds_mesh_smooth_limit_f32(const float* original, float* vertices, long long n_vertices, double max_move, double* move2_out,
                              unsigned char* clamped_out, void* stream);

/*
 * Filling the small holes of a triangle mesh with centroid fans (csrc/mesh_fill.hip).  The result is a function of
 * the input mesh alone.  The input's vertex, colour and face rows stay bit for bit; rows are only added.
 *
 * Inputs.  vertices float32 [V][3]; colors uint8 [V][3]; faces int32 [F][3]; max_edges in 3..CDS_MESH_FILL_MAX_EDGES.
 * 1. Valid faces.  A face is valid when its three indices are in [0, V) and pairwise distinct.  A valid face (a, b, c) holds the
 *      directed half-edges a->b, b->c, c->a.  An invalid face holds none, is never touched and is copied through.
 * 2. Border half-edges.  a->b is a border half-edge iff the undirected edge {a,b} is held by exactly one face slot over all valid
 *      faces.  An edge held by three or more slots is no border, nor is one held twice in the same direction.
 * 3. Regular vertices.  A vertex is regular iff exactly one border half-edge leaves it and exactly one enters it; next[a] = b for
 *      the border half-edge a->b of a regular a.
 * 4. Loops.  A loop is a cycle v0, v1 = next[v0], ..., v(n-1) with next[v(n-1)] = v0, every vertex on it regular; v0 is its
 *      smallest vertex and its label, n its edge count.  A walk that meets a vertex that is not regular belongs to no loop (two
 *      holes that touch in a vertex, the end of a non-manifold fin).  A loop is filled iff 3 <= n <= max_edges.  The outer rim of
 *      an open scan is a loop too: max_edges is what leaves it alone.
 * 5. The fill.  n == 3: the one face (v0, v2, v1), no new vertex.  n >= 4: one new vertex c and the n faces (v(k+1), v(k), c),
 *      k = 0..n-1 with v(n) = v0: every new face runs its border edge backwards, which is the orientation of the surface around
 *      the hole.  Position of c, per coordinate: the sum of (double)p over v0, v1, ..., v(n-1) in that order, sequential in fp64
 *      from +0.0, divided by (double)n, rounded once to fp32; a mean that is a NaN is written as 0x7fc00000, whatever the NaNs
 *      that went in.  Colour of c, per channel, in integers: (2 sum + n) / (2 n), floored.
 * 6. Order.  The V input vertices first, then the new vertices in ascending label order.  The F input faces first, invalid ones
 *      included, then the new faces loop by loop in ascending label order, within a loop in the order of rule 5.  V + new
 *      vertices and F + new faces stay below 2^31 (the host refuses before anything is written).
 *
 * A key is ((min(a,b) << 31 | max(a,b)) << 1) | direction, direction 0 for a < b: 63 bits, so that a signed sort orders it; the
 * key of an invalid face's slots is 2^63 - 1.  The caller sorts the 3 F keys ascending.
 * cds_mesh_fill_max_edges: CDS_MESH_FILL_MAX_EDGES.  The walk of a loop is one thread's serial chain: that is the limit's reason.
 * cds_mesh_fill_keys: keys int64 [3 F].
 * cds_mesh_fill_borders: over the sorted keys; out, in int32 [V] zeroed by the caller (integer atomics): the border half-edges
 *   that leave and enter each vertex; next, prev int32 [V]: next[a] = b, meaningful where out[a] == 1 only, and prev[b] = a,
 *   meaningful where in[b] == 1 only.  A key that decodes to an index outside [0, V) is skipped.
 * cds_mesh_fill_init: regular uint8 [V] (rule 3); next = prev = -1 where the vertex is not regular; the start of the pointer
 *   doubling in both pairs of arrays, int32 [2][V] each, row 0 the chain along next and row 1 the chain along prev: label = v and
 *   jump = next[v] (prev[v]) for a regular v, label = -1 and jump = v for another.
 * cds_mesh_fill_double: one round over list int32 [n_list], the regular vertices, in both rows: label_out[v] = min(label_in[v],
 *   label_in[jump_in[v]]), jump_out[v] = jump_in[jump_in[v]].  After r rounds label[0][v] is the minimum over v and its 2^r - 1
 *   successors and label[1][v] that over v and its 2^r - 1 predecessors, -1 if one of them is not regular.  With 2^r >= max_edges
 *   only a v with label[0][v] == label[1][v] == v can be the v0 of a loop that is filled, and a rim of any length and any
 *   numbering has at most one such v per 2^r vertices: the pruning saves walks and decides nothing.
 * cds_mesh_fill_walk: per entry i of list: edges[i] = n of the filled loop whose v0 is list[i], else 0; centre float32
 *   [n_list][3] and centre_color uint8 [n_list][3]: rule 5's vertex where n >= 4.
 * cds_mesh_fill_emit: vertex_at, face_at int64 [n_list]: the exclusive prefix sums of (edges >= 4) and of (edges == 3 ? 1 :
 *   edges); writes the new vertex of entry i at row V + vertex_at[i] of vertices_out / colors_out and its faces from row
 *   F + face_at[i] of faces_out.  An offset outside [0, new_vertices) / [0, new_faces] writes nothing.
 *   CDS_EINVAL: a count < 0 or >= 2^31; 3 n_faces >= 2^31; n_list > n_vertices; max_edges outside 3..CDS_MESH_FILL_MAX_EDGES; the
 *   same array for both sides of a round; a null required pointer (an empty input returns 0 first).
 */
#define CDS_MESH_FILL_MAX_EDGES 4096
int cds_mesh_fill_max_edges(void);
int cds_mesh_fill_keys(const int* faces, long long n_faces, long long n_vertices, long long* keys, void* stream);
int cds_mesh_fill_borders(const long long* keys, long long n_keys, long long n_vertices, int* out, int* in, int* next, int* prev,
                          void* stream);
int cds_mesh_fill_init(long long n_vertices, const int* out, const int* in, int* next, int* prev, unsigned char* regular,
                       int* label_a, int* jump_a, int* label_b, int* jump_b, void* stream);
int cds_mesh_fill_double(const int* list, long long n_list, long long n_vertices, const int* label_in, const int* jump_in,
                         int* label_out, int* jump_out, void* stream);
int cds_mesh_fill_walk(const float* vertices, const unsigned char* colors, long long n_vertices, const int* next,
                       const unsigned char* regular, const int* label, const int* list, long long n_list, int max_edges, int* edges,
                       float* centre, unsigned char* centre_color, void* stream);
int cds_mesh_fill_emit(const int* next, const unsigned char* regular, long long n_vertices, long long n_faces, const int* list,
                       long long n_list, int max_edges, const int* edges, const long long* vertex_at, const long long* face_at,
                       const float* centre, const unsigned char* centre_color, long long new_vertices, long long new_faces,
                       float* vertices_out, unsigned char* colors_out, int* faces_out, void* stream);

/*
 * Surface samples of a triangle mesh: a dense, deterministic point set from the faces (csrc/mesh_sample.hip).
 *
 * Inputs.  vertices float32 [V][3]; colors uint8 [V][3]; faces int32 [F][3], every index in [0, V) (the host refuses another
 *   mesh; a kernel skips such a face and reads nothing there); spacing > 0, finite, a double.
 * 1. Subdivision count per face.  A, B, C: the corners as doubles.  L2: the largest of the three squared edge lengths, each
 *      ((dx dx + dy dy) + dz dz) in fp64.  n is the smallest integer >= 1 with ((double)n spacing) ((double)n spacing) >= L2,
 *      evaluated in fp64.  The kernel starts from ceil(sqrt(L2) / spacing) and corrects downwards and upwards with that test, so
 *      n does not depend on how sqrt or the division round.  A face with a corner coordinate that is not finite has n = 0 and
 *      emits nothing; a face with L2 == 0 has n = 1.  n > CDS_MESH_SAMPLE_MAX_N = 2^15 is refused by the host.
 * 2. Samples.  The barycentric lattice cuts the face into n^2 congruent sub-triangles; sample k in [0, n^2) is the centroid of
 *      sub-triangle k.  r = isqrt(k) exactly (an integer correction after any floating-point guess), c = k - r r, j = c >> 1.
 *      Even c (upright): p = 3 r + 2, q = 3 j + 1; odd c: p = 3 r + 1, q = 3 j + 2.  Integer weights wa = 3 n - p, wb = p - q,
 *      wc = q: all > 0, their sum 3 n.  Position per component: ((wa A + wb B) + wc C) / (double)(3 n) in fp64, no contraction
 *      (-ffp-contract=off), rounded once to fp32.  Colour per channel, in integers: (2 (wa ca + wb cb + wc cc) + 3 n) / (6 n),
 *      which rounds half up.
 * 3. Order.  Face order, then k ascending.  Outputs: points float32 [N][3], colors uint8 [N][3], face int32 [N], N = sum n^2.
 *
 * cds_mesh_sample_max_n: CDS_MESH_SAMPLE_MAX_N.
 * cds_mesh_sample_count: rule 1, one thread per face.  Writes out_n int32 [n_faces], clamped to CDS_MESH_SAMPLE_MAX_N + 1 so that
 *   the host sees an overflow, and out_n2 int64 [n_faces] = n n.  A face with an index outside the vertices gets 0.
 * cds_mesh_sample_emit: rules 2 and 3, by sample: a workgroup owns a run of consecutive output indices, finds the run's faces by
 *   a binary search in offsets and its threads resolve their face inside that range.  n int32 [n_faces] as the count kernel wrote
 *   it; offsets int64 [n_faces]: the exclusive prefix sum of n n (faces without samples repeat the next offset; the sample
 *   belongs to the last face whose offset is <= its index); n_points the total.  out_points, out_colors and out_face 16-byte
 *   aligned.  A sample whose face has an index outside the vertices, an n outside 1 .. CDS_MESH_SAMPLE_MAX_N
 *   or offsets that do not fit n n is not written.
 *   CDS_EINVAL: a count < 0 or >= 2^31; spacing not finite or <= 0; a null required pointer or a misaligned output (an empty
 *   input or output returns 0 first).
 */
#define CDS_MESH_SAMPLE_MAX_N 32768
int cds_mesh_sample_max_n(void);
int cds_mesh_sample_count(const float* vertices, long long n_vertices, const int* faces, long long n_faces, double spacing,
                          int* out_n, long long* out_n2, void* stream);
int cds_mesh_sample_emit(const float* vertices, const unsigned char* colors, long long n_vertices, const int* faces,
                         long long n_faces, const int* n, const long long* offsets, long long n_points, float* out_points,
                         unsigned char* out_colors, int* out_face, void* stream);

/*
 * A texture atlas for a mesh from the images of a scan: one view and one square cell per face (csrc/mesh_texture.hip;
 * DESIGN 1.17).
 *
 * Inputs.  vertices fp32 [n_vertices][3], colours uint8 [n_vertices][3], faces int32 [n_faces][3]; V views: per view an image
 *   uint8 [h][w][3] (h and w the view's own) and cams [CDS_RASTER_CAM] doubles as the rasteriser above takes them; scale > 0 (texels per pixel), max_cell
 *   a power of two in 4 .. CDS_TEXTURE_MAX_CELL, min_px >= 1.  All arithmetic is fp64 from the fp32 or uint8 entries, bracketed
 *   as written; every decision is made on integers or on one fp64 comparison.
 * 1. Visibility.  The mesh is rendered into every view by the rasteriser above, unchanged.  votes[v][f] is the number of pixels
 *      of view v with valid != 0 and face == f: an integer, whatever the order of the additions.
 * 2. View of a face.  key[f] = max over v of (votes[v][f] << 32) | (0xffffffff - v), a uint64, 0 before the first view: the most
 *      votes, the lowest view on a tie.  The face is seen iff key >> 32 >= min_px; then view[f] = 0xffffffff - (key & 0xffffffff),
 *      else view[f] = -1.
 * 3. Cell size.  For a seen face whose three vertices are usable by rule 1 of the rasteriser in the face's view, (X_i, Y_i) their
 *      snapped coordinates: L2 = the largest of the three (Xj - Xi)^2 + (Yj - Yi)^2, exact in int64;  t = (scale scale) (double)L2.
 *      n is the smallest integer >= 1 with (256 n)^2 >= t; c is the smallest power of two >= n + 2, at least 4 and at most
 *      max_cell.  Evaluated without a square root: c is the smallest power of two p in 4 .. max_cell / 2 with
 *      (256 (p - 2)) (256 (p - 2)) >= t, both sides doubles, and max_cell when there is none.  Every other face has c = 4.
 * 4. Packing.  A cell of side c takes (c / 4)^2 units of 4 x 4 texels.  The faces sorted by c descending, stable in the face index:
 *      start[k] is the sum of the units of the sorted positions before k, total the sum of all.  The cell takes the units
 *      start .. start + (c / 4)^2 - 1 of the Z-order curve: its origin is x0 = 4 (the even bits of start, packed), y0 = 4 (the odd
 *      bits).  Every start is a multiple of the cell's own unit count, so cells are aligned to their size and disjoint.
 *      W is the smallest power of two >= 4 with (W / 4)^2 >= total;  H = W / 2 when 2 total <= (W / 4)^2 and W >= 8, else W.
 * 5. UV, in texels of the atlas (the texel (x, y) covers [x, x + 1)^2, row y = 0 the first of the image):  corner a at
 *      (x0 + 1, y0 + 1), b at (x0 + c - 1, y0 + 1), c at (x0 + 1, y0 + c - 1).
 * 6. Texel (x0 + i, y0 + j) of a cell, 0 <= i, j < c, inside the triangle or not:
 *      wb = ((i + 0.5) - 1) / (c - 2),  wc = ((j + 0.5) - 1) / (c - 2),  wa = (1 - wb) - wc.
 *      For a seen face: P = (wa A + wb B) + wc C per coordinate; u, v, z of P by rule 1 of the rasteriser in view[f].  If z > 0
 *      and u, v are finite:  uc = min(max(u, 0.5), w - 0.5), x = uc - 0.5, xl = floor(x), xh = min(xl + 1, w - 1), fx = x - xl,
 *      gx = 1 - fx, and likewise vc, y, yl, yh, fy, gy from v and h;  per channel
 *        value = (((gx gy) I[yl][xl] + (fx gy) I[yl][xh]) + (gx fy) I[yh][xl]) + (fx fy) I[yh][xh],  texel = floor(value + 0.5).
 *      Otherwise, and for every texel of a face that is not seen:  value = (wa ca + wb cb) + wc cc from the vertex colours,
 *      texel = floor(clamp(value, 0, 255) + 0.5) with clamp(NaN) = 0.
 *      A texel that belongs to no cell is 0.
 *
 * cds_texture_votes: rule 1 for a chunk of views.  face int32 and valid uint8 [n_views][h][w] as cds_raster_resolve wrote them;
 *   votes int32 [n_views][n_faces], zeroed by the caller, receives integer atomic adds.  runs 1: the first lane of a run of equal
 *   faces inside a wave adds the run's length; runs 0: one add per pixel.  The counts are the same.
 * cds_texture_best: rule 2 for that chunk, whose first view has the index view0: key uint64 [n_faces], zeroed by the caller
 *   before the first chunk.
 * cds_texture_cells: the end of rule 2 and rule 3.  cams [n_views] of ALL views.  Writes view int32 [n_faces] and
 *   cell int32 [n_faces][3] = (0, 0, c).
 * cds_texture_place: rules 4 and 5 after the caller's sort.  order int64 [n_faces]: the face of every sorted position;
 *   starts int64 [n_faces].  Writes the origin into cell and uv int32 [n_faces][3][2].  A position whose face, size or start cannot
 *   come from rule 4 is skipped.
 * cds_texture_fill: rule 6.  images: image_bytes bytes that hold every view's [h][w][3] image; views int64 [n_views][3]: the byte
 *   offset of the view's image in images, its h and its w (the views of a scan may differ in size; a face whose view's entry
 *   does not lie inside images is coloured as an unseen one).  cams [n_views] of all views.
 *   atlas uint8 [atlas_h][atlas_w][3], 4-byte aligned; every texel is written.  The unit of a texel
 *   finds its sorted position by a binary search of its Morton index in starts.  per_unit 0: one thread per texel;
 *   per_unit 1: one thread per 4 x 4 unit.  The texels are the same.  A unit whose tables do not fit together is written 0.
 *   CDS_EINVAL: a count < 0 or >= 2^31; n_views < 1 (votes, best: outside 1..CDS_RASTER_MAX_CHUNK); view0 < 0; h or w < 1;
 *   h w >= 2^31; image_bytes < 0; min_px < 1; scale not finite or <= 0; max_cell not a power of two in 4..CDS_TEXTURE_MAX_CELL; total < 0 or
 *   > CDS_TEXTURE_MAX_UNITS; atlas_w not a power of two in 4..CDS_TEXTURE_MAX_SIZE; atlas_h neither atlas_w nor atlas_w / 2;
 *   total beyond the atlas; runs or per_unit not 0 or 1; a null required pointer or a misaligned atlas (an empty mesh returns 0
 *   first, except in fill, which then writes zeros).
 */
#define CDS_TEXTURE_MAX_CELL 4096
#define CDS_TEXTURE_MAX_SIZE 32768
#define CDS_TEXTURE_MAX_UNITS (1ll << 26)
int cds_texture_votes(const int* face, const unsigned char* valid, int n_views, int h, int w, long long n_faces, int* votes,
                      int runs, void* stream);
int cds_texture_best(const int* votes, long long n_faces, int n_views, int view0, unsigned long long* key, void* stream);
int cds_texture_cells(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const double* cams,
                      int n_views, const unsigned long long* key, long long min_px, double scale, int max_cell, int* view,
                      int* cell, void* stream);
int cds_texture_place(const long long* order, const long long* starts, long long n_faces, long long total, int max_cell, int* cell,
                      int* uv, void* stream);
int cds_texture_fill(const float* vertices, const unsigned char* colors, long long n_vertices, const int* faces, long long n_faces,
                     const double* cams, const unsigned char* images, long long image_bytes, const long long* views, int n_views,
                     const int* view, const int* cell, const long long* order, const long long* starts, long long total,
                     int max_cell, int atlas_h, int atlas_w, unsigned char* atlas, int per_unit, void* stream);

/*
 * Seam levelling of that atlas: an additive correction per (vertex, view), found by least squares and interpolated over each
 * face, so that faces which take their colour from different exposures meet without a step (csrc/mesh_texture.hip).
 * Rules 1-5 above are unchanged; only the texel colours of seen faces change.  All arithmetic is fp64 from the fp32 or uint8
 * entries, bracketed as written; every decision is made on integers.  V is the number of views, at most
 * CDS_TEXTURE_LEVEL_MAX_VIEWS: rule L3 keeps a dense V x V table.
 *
 * L1. Nodes.  Every corner k of every face f with view[f] = l >= 0 and valid vertex indices has the key vertex V + l (int64).
 *      The nodes are the distinct keys, ascending; a node's id is its rank.  corner_node int32 [n_faces][3] holds the node of
 *      every corner, -1 for the corners of unseen faces.  A node's corners are the corner indices 3 f + k that map to it,
 *      ascending.  The nodes of one vertex are consecutive and ordered by label.  (The caller sorts: these are tables, not a
 *      kernel.)
 * L2. Sample.  s_n[ch] is the unrounded value of rule 6 (the same clamps, the same brackets) at the projection of the node's
 *      vertex, as a double, into the node's view.  ok_n iff z > 0, u and v are finite and the view's image entry lies inside
 *      the bytes; a node that is not ok samples 0.
 * L3. Per-view offsets.  q_n[ch] = (int64)floor(s_n[ch] 256 + 0.5).  For every pair of ok nodes i < j of one vertex, with the
 *      labels a < b:  cnt[a][b] += 1, dsum[a][b][ch] += q_i - q_j, int64 sums, whatever the order of the additions.
 *      The host reads the table once and solves per channel, in fp64, the normal equations of
 *        sum cnt[a][b] ((o_a - o_b) + dsum[a][b] / (256 cnt[a][b]))^2 + RIDGE sum max(n_a, 1) o_a^2,   RIDGE = 2^-10,
 *      n_a the number of nodes with label a:  o fp64 [V][3].
 * L4. Start.  g_n = o[label_n].
 * L5. One iteration, a damped Jacobi step of
 *        sum over seam pairs ((s + g) - (s' + g'))^2 + lambda sum over faces, over the face's three edges (g - g')^2.
 *      For node n, per channel, every read from the previous iteration's g:
 *        S = the sum of ((s_m + g_m) - s_n) over the other ok nodes m of n's vertex, ascending in m, from 0, c their number,
 *            when n is ok; else S = 0, c = 0;
 *        T = the sum of g over the two other corner nodes of each corner of n, the corners ascending and the partners in the
 *            order (k + 1) % 3, (k + 2) % 3, from 0, d their number;
 *        den = c + lambda d;   g'_n = g_n + OMEGA (((S + lambda T) / den) - g_n),   OMEGA = CDS_TEXTURE_LEVEL_OMEGA.
 * L6. Texel.  Where rule 6 takes its image branch for face f, with the face's three corner nodes A, B, C:
 *        corr = (wa g_A + wb g_B) + wc g_C,   texel = floor(clamp(value + corr, 0, 255) + 0.5) with clamp(NaN) = 0.
 *      The vertex-colour branch and unseen faces are unchanged.  A face with a corner node outside [0, N) is unlevelled: the
 *      node is never followed.
 *
 * cds_texture_level_samples: rule L2.  node_key int64 [n_nodes]; images, image_bytes, views, cams as cds_texture_fill takes them.
 *   Writes sample fp64 [n_nodes][3] and ok uint8 [n_nodes].  A key < 0 or with a vertex outside the vertices is not ok.
 * cds_texture_level_pairs: the table of rule L3.  span int32 [n_nodes][2]: the first node of the node's vertex and the number
 *   of its nodes.  table int64 [n_views][n_views][4] = cnt, dsum[3], zeroed by the caller, receives integer atomic adds (a
 *   workgroup sums its pairs in LDS first and adds every entry it used once; the sums are the same).  A span
 *   that does not hold its node, leaves the nodes or is longer than n_views is skipped, as is a partner of another vertex.
 * cds_texture_level_step: rule L5, one thread per node, gathers only.  corner_start int64 [n_nodes + 1] and corner_list int64
 *   [n_list]: the corners of node n are corner_list[corner_start[n] .. corner_start[n + 1]).  g_in and g_out fp64 [n_nodes][3],
 *   two buffers.  A range outside the list, a corner outside 0 .. 3 n_faces and a partner outside [0, n_nodes) are skipped.
 * cds_texture_fill_level: cds_texture_fill with rule L6 from corner_node int32 [n_faces][3] and g fp64 [n_nodes][3].
 *   CDS_EINVAL: what cds_texture_fill refuses; a count < 0 or >= 2^31; n_views outside 1..CDS_TEXTURE_LEVEL_MAX_VIEWS; lambda not
 *   finite or <= 0; n_list < 0 or > 3 n_faces; g_in == g_out; a null required pointer (zero nodes return 0 first, except in the fill).
 */
#define CDS_TEXTURE_LEVEL_MAX_VIEWS 512
#define CDS_TEXTURE_LEVEL_OMEGA 0.75
int cds_texture_level_samples(const float* vertices, long long n_vertices, const double* cams, const unsigned char* images,
                              long long image_bytes, const long long* views, int n_views, const long long* node_key,
                              long long n_nodes, double* sample, unsigned char* ok, void* stream);
int cds_texture_level_pairs(const double* sample, const unsigned char* ok, const long long* node_key, const int* span,
                            long long n_nodes, int n_views, long long* table, void* stream);
int cds_texture_level_step(const double* sample, const unsigned char* ok, const int* span, const long long* corner_start,
                           const long long* corner_list, long long n_list, const int* corner_node, long long n_nodes,
                           long long n_faces, int n_views, double lambda, const double* g_in, double* g_out, void* stream);
int cds_texture_fill_level(const float* vertices, const unsigned char* colors, long long n_vertices, const int* faces,
                           long long n_faces, const double* cams, const unsigned char* images, long long image_bytes,
                           const long long* views, int n_views, const int* view, const int* cell, const long long* order,
                           const long long* starts, long long total, int max_cell, int atlas_h, int atlas_w, unsigned char* atlas,
                           int per_unit, const int* corner_node, const double* g, long long n_nodes, void* stream);

/*
 * A mesh scored against the photographs of its scan: the textured render, and PSNR / SSIM sums of two images under a mask
 * (csrc/photo.hip).  All arithmetic is fp64 from the uint8, fp32 or int32 entries, bracketed as written; every
 * decision is made on integers.
 *
 * S. Shade.  vertices, faces and cams [n_views][CDS_RASTER_CAM] as the rasteriser takes them; uv int32 [n_faces][3][2] and atlas
 *      uint8 [H][W][3] as rule 5 and rule 6 of the texture stage give them; face int32 [n_views][h][w] as cds_raster_resolve wrote
 *      it.  For a pixel (px, py) with face = f in [0, n_faces) whose three indices are inside the vertices:
 *      Surface point: Xc of the three corners by rule 1 of the rasteriser; n, d, rx, ry, zf by its rule 4; P and w_a, w_b, w_c
 *        by its rule 6, with the same brackets: the bits the rasteriser computed.
 *      Texel coordinate: T = (w_a U_a + w_b U_b) + w_c U_c per coordinate, U the face's three uv corners as doubles.
 *      Cell, from the corners (so a model read back from an OBJ is shaded too): x0 = U_a.x - 1, y0 = U_a.y - 1,
 *        c = U_b.x - U_a.x + 2, in int64.  The fall-back: when c < 4 or the cell does not lie inside the atlas
 *        (x0 < 0, y0 < 0, x0 + c > W or y0 + c > H) the pixel is black (0, 0, 0) and nothing is read.
 *      Clamp into the cell: tx = T.x if T.x > x0 + 0.5 else x0 + 0.5 (a NaN takes the lower bound); tx = min(tx, x0 + c - 0.5);
 *        x = tx - 0.5, xl = floor(x), xh = min(xl + 1, x0 + c - 1), fx = x - xl, gx = 1 - fx; likewise ty, y, yl, yh, fy, gy.
 *      Value, per channel:  value = (((gx gy) A[yl][xl] + (fx gy) A[yl][xh]) + (gx fy) A[yh][xl]) + (fx fy) A[yh][xh],
 *        pixel = floor(value + 0.5).
 *      Every other pixel is 0.
 * C. Compare.  a, b uint8 [n_views][h][w][3], mask uint8 [n_views][h][w]; g: 11 doubles of the HOST, the window's weights (the
 *      kernels evaluate no exp).  Per view:
 *      Masked pixels: n_px = the number of pixels with mask != 0; sse[ch] = the sum of (a - b)^2 over them, exact in int64.
 *      Windows: one for every top-left (x', y') with 0 <= x' <= w - 11 and 0 <= y' <= h - 11; it counts iff all 121 mask bytes are
 *        non-zero (an integer sum).
 *      Moments of a counting window, per channel: for m in {a, b, a a, b b, a b} (the products as doubles)
 *        r[y][x'] = ((g0 m[y][x'] + g1 m[y][x' + 1]) + ...) + g10 m[y][x' + 10], ascending, left to right;
 *        E[m] = ((g0 r[y'][x'] + g1 r[y' + 1][x']) + ...) + g10 r[y' + 10][x'].
 *      SSIM: mua = E[a], mub = E[b], va = E[aa] - mua mua, vb = E[bb] - mub mub, vab = E[ab] - mua mub;
 *        ssim = ((2 mua mub + C1) (2 vab + C2)) / (((mua mua + mub mub) + C1) ((va + vb) + C2)),  C1 = 6.5025, C2 = 58.5225.
 *      Outputs: counts int64 [n_views][5] = n_px, sse[3], n_win (the counting windows); ssim_sum fp64 [n_views][3], the sum of
 *        ssim over the counting windows: per tile of CDS_PHOTO_TILE x CDS_PHOTO_TILE windows a fixed tree over the tile's
 *        windows, then per view a fixed walk and tree over the tiles: the same bits run to run, no atomics.
 *        ssim_map, when not null: fp64 [n_views][3][h - 10][w - 10], NaN for a window that does not count; with h < 11 or w < 11
 *        there is no window, n_win = 0 and the map is not touched.
 *
 * cds_photo_shade: rule S.  image uint8 [n_views][h][w][3]; every pixel is written.  An empty mesh or an atlas of 0 x 0 writes
 *   zeros.  CDS_EINVAL: a count < 0 or >= 2^31; n_views outside 1..CDS_RASTER_MAX_CHUNK; h or w < 1; h w >= 2^31; an atlas that
 *   is neither 0 x 0 nor of a size cds_texture_fill accepts; a null required pointer.
 * cds_photo_scores: rule C.  ws: CDS_PHOTO_SCORES_WS_WORDS(n_views, h, w) int64 words of workspace, ws_words the words it has.
 *   CDS_EINVAL: n_views, h, w as above; ws_words too small; a null pointer other than ssim_map.
 */
#define CDS_PHOTO_TILE 16
#define CDS_PHOTO_RECORD 8
#define CDS_PHOTO_SCORES_WS_WORDS(n_views, h, w) \
  ((long long)(n_views) * (((h) + CDS_PHOTO_TILE - 1) / CDS_PHOTO_TILE) * (((w) + CDS_PHOTO_TILE - 1) / CDS_PHOTO_TILE) * CDS_PHOTO_RECORD)
int cds_photo_shade(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const int* uv,
                    const unsigned char* atlas, int atlas_h, int atlas_w, const double* cams, int n_views, const int* face, int h,
                    int w, unsigned char* image, void* stream);
int cds_photo_scores(const unsigned char* a, const unsigned char* b, const unsigned char* mask, const double* g, int n_views, int h,
                     int w, long long* ws, long long ws_words, long long* counts, double* ssim_sum, double* ssim_map, void* stream);

/*
 * Norm-curvature bookkeeping of one FeatureNet level (module.py:250-251,257-258,264-265) in one launch:
 *   nc_sum[i] = (a[i]^2 + b[i]^2 + c[i]^2) / 3,  nc_abs[i] = |c[i]|   for the three DynamicConv curvature maps of the level
 */
int cds_curvature_stats_f32(const float* a, const float* b, const float* c, float* nc_sum, float* nc_abs, int n,
                            void* stream);
/* Its backward (training): ga = (g_sum / 3) 2 a, gb likewise, gc = (g_sum / 3) 2 c + g_abs sgn(c); g_sum / g_abs may be NULL. */
int cds_curvature_stats_bwd_f32(const float* a, const float* b, const float* c, const float* g_sum, const float* g_abs, float* ga,
                                float* gb, float* gc, int n, void* stream);
/* out[v][i] = (x[v][i] + x[V+v][i]) / 2 for v < V (model.py:59); x [2V][n] */
int cds_pair_mean_f32(const float* x, float* out, int V, int n, void* stream);
/* out[i] = (sum over v of x[v][i]) / V (model.py:60,79); x [V][n] */
int cds_view_mean_f32(const float* x, float* out, int V, int n, void* stream);

/*
 * Refinement network (module.py:318-370) pieces besides its 3x3 Conv+BN+ReLU units (those run on cds_conv2d_f32):
 *   depth_range            3 floats, DEVICE (geometry block): (depth_min, depth_max, ival).  models/model.py:213-216 divides the depth
 *                          and both limits by the depth interval before the network and multiplies the result by it (:218): that is
 *                          folded into the two kernels - lo = depth_min / ival, hi = depth_max / ival (true divisions, as the
 *                          reference's tensor ops); ival = 1 gives module.py's network on its own
 *   cds_depth_affine_f32   out[i] = (depth[i] / ival - lo) / (hi - lo) * 10               (module.py:353-355)
 *   cds_deconv2d_k3s2_f32  ConvTranspose2d k=3, stride 2, padding 1, output_padding 1 (+ bias + activation);
 *                          x [Cin][H][W] -> out [Cout][2H][2W]; weight PACKED [Cin][9][Cout] = PyTorch's
 *                          [Cin][Cout][3][3] permuted (0,2,3,1) (BatchNorm folded in by the caller); Cout = 8
 *   cds_refine_finish_f32  out = (((bilinear x2, align_corners=True)(d_norm [h][w]) + res [2h][2w]) / 10 * (hi - lo) + lo) * ival
 */
int cds_depth_affine_f32(const float* depth, float* out, int n, const float* depth_range, void* stream);
int cds_deconv2d_k3s2_f32(const float* x, const float* weight, const float* bias, float* out, int Cin, int Cout,
                          int H, int W, int act, void* stream);
int cds_refine_finish_f32(const float* d_norm, const float* res, float* out, int h, int w, const float* depth_range,
                          void* stream);

/*
 * Training kernels of the CostRegNet stack (models/module.py:80-160 with BatchNorm3d in training mode).
 * Activations [B][C][D][H][W] fp32 (V = D*H*W), statistics fp64.  Forward convolutions and data gradients use
 * cds_conv3d_k3_f32 / cds_deconv3d_k3s2_f32 (a convolution's data gradient is the transposed convolution and vice versa).
 *   cds_bn3d_stats_f32:       sums[c] = (sum x, sum x^2) over batch and voxels, ADDED onto sums [C][2] (zero it first)
 *   cds_bn3d_norm_f32:        the per-channel step of nn.BatchNorm3d in training mode from those sums (fp64: mean, biased variance,
 *                             scale = gamma / sqrt(var + eps), shift = beta - mean scale; n = elements per channel) done by every
 *                             workgroup, then out = relu?(y * scale[c] + shift[c]) (+ skip): BatchNorm(train) + ReLU + U-Net skip in
 *                             one launch.  Writes scale / shift [C] floats and mean / invstd [C] doubles for the backward and updates
 *                             running_mean / running_var in place with `momentum` (unbiased variance; both may be NULL)
 *   cds_bn3d_bwd_reduce_f32:  sums[c] += (sum g, sum g*y), g = dout * [relu ? y*scale+shift > 0 : 1]
 *   cds_bn3d_bwd_norm_f32:    dgamma, dbeta [C] and dy = g * scale[c] + y * k1[c] + k0[c] (the BatchNorm backward in closed form; k1,
 *                             k0 derived from the sums of cds_bn3d_bwd_reduce_f32 by every workgroup) in one launch
 *   cds_conv3d_wgrad_f32:     dw[a][b][tap] += sum_{batch, o} g[a][o] * xin[b][stride * o - 1 + tap]   (k3, pad 1)
 *                             Conv3d: g = dy, xin = x -> dw [Cout][Cin][27]; ConvTranspose3d: g = x, xin = dy, stride 2 ->
 *                             dw [Cin][Cout][27] (PyTorch's layouts).  dw is accumulated onto: zero it first.
 */
int cds_bn3d_stats_f32(const float* x, double* sums, int B, int C, long long V, void* stream);
int cds_bn3d_norm_f32(const float* y, const double* sums, const float* gamma, const float* beta, double n, double eps, float momentum,
                      float* running_mean, float* running_var, const float* skip, float* out, float* scale, float* shift, double* mean,
                      double* invstd, int B, int C, long long V, int relu, void* stream);
int cds_bn3d_bwd_reduce_f32(const float* dout, const float* y, const float* scale, const float* shift, double* sums, int B,
                            int C, long long V, int relu, void* stream);
int cds_bn3d_bwd_norm_f32(const float* dout, const float* y, const float* scale, const float* shift, const double* sums,
                          const double* mean, const double* invstd, double n, float* dy, float* dgamma, float* dbeta, int B, int C,
                          long long V, int relu, void* stream);
int cds_conv3d_wgrad_f32(const float* g, const float* xin, float* dw, int B, int Ca, int Cb, int Do, int Ho, int Wo, int Di,
                         int Hi, int Wi, int stride, void* stream);

/* ---- CostRegNet training convolutions in split-f16 (train_ops.conv_arithmetic("split_f16"); csrc/train3d_sf16.hip) -------------
 * Every fp32 operand is two fp16 terms of (value x s), s the power of two of sf16_scale(bound) for a DEVICE-resident upper bound of
 * max |x|; three v_mfma_f32_16x16x32_f16 products per K-step, fp32 accumulation, exact rescale.  No host reads: graph-capturable.
 *   cds_bn3d_norm_bound_f32 / cds_bn3d_bwd_norm_bound_f32: cds_bn3d_norm_f32 / cds_bn3d_bwd_norm_f32 that also raise *out_bound /
 *                             *dy_bound (zeroed by the caller) to the max |value| they store
 *   cds_absmax_bound_f32:     *bound = max(*bound, max |x[0..n)|)
 *   cds_sf16_pack_conv3d_f32: w [A][B][27] (mode 0 / 1: Conv3d stride 1 / 2, A = Cout; mode 2: ConvTranspose3d, A = Cin), A, B
 *                             multiples of 8, <= 64: *w_inv = 1 / s_w from max |w| on the device, fwd / dgrad (either may be NULL) the
 *                             hi / lo operands [C/8][28][2][Mpad][8] fp16 of the forward and of the data gradient (the stride-1
 *                             convolution's flipped and transposed; the stride-2 convolution's for mode 2, the transposed one's for mode 1)
 *   cds_conv3d_k3_sf16_f32:   y [B][M][..] from x [B][C][Di][Hi][Wi] and a pack; mode 0: stride-1 convolution, 1: stride 2 (pad 1),
 *                             2: transposed k3 s2 (pad 1, output padding 1: [2Di][2Hi][2Wi]).  C a multiple of 8, M <= 64
 *   cds_conv3d_wgrad_sf16_f32: cds_conv3d_wgrad_f32 (dw accumulated onto) with bounds of g and xin on the device */
int cds_bn3d_norm_bound_f32(const float* y, const double* sums, const float* gamma, const float* beta, double n, double eps,
                            float momentum, float* running_mean, float* running_var, const float* skip, float* out, float* scale,
                            float* shift, double* mean, double* invstd, int B, int C, long long V, int relu, float* out_bound,
                            void* stream);
int cds_bn3d_bwd_norm_bound_f32(const float* dout, const float* y, const float* scale, const float* shift, const double* sums,
                                const double* mean, const double* invstd, double n, float* dy, float* dgamma, float* dbeta, int B, int C,
                                long long V, int relu, float* dy_bound, void* stream);
int cds_absmax_bound_f32(const float* x, long long n, float* bound, void* stream);
int cds_sf16_pack_conv3d_f32(const float* w, void* fwd, void* dgrad, float* w_inv, int A, int B, int mode, void* stream);
int cds_conv3d_k3_sf16_f32(const float* x, const void* wpk, const float* w_inv, const float* x_bound, float* y, int B, int C, int M,
                           int Di, int Hi, int Wi, int mode, void* stream);
int cds_conv3d_wgrad_sf16_f32(const float* g, const float* xin, const float* g_bound, const float* x_bound, float* dw, int B, int Ca,
                              int Cb, int Do, int Ho, int Wo, int Di, int Hi, int Wi, int stride, void* stream);

/* ---- training step, 2D stacks (csrc/train2d.hip) ---------------------------------------------------------------
 * Backward kernels of FeatureNet / DynamicConv (models/dynamic_conv.py:97-122, models/module.py:28-71,234-267), the visibility CNN
 * (models/model.py:14,51), Refinement (models/module.py:318-370) and depth_regression (models/module.py:373-379); they replace what
 * torch.autograd + cuDNN derive from those forwards in trainer/trainer.py:69-82.
 *   cds_conv2d_wgrad_f32:     dw[co][ci][ky][kx] += sum_{n,o} g[n][co][o] x[n][ci][stride * o - pad + k]; Conv2d: g = dy; a transposed
 *                             convolution swaps the roles (g = x, x = dy, stride 2) and receives [Cin][Cout][k][k].  dw is accumulated
 *                             onto (zero it first).  k in {1,3,5,7,11} at stride 1, k = 3 at stride 2.
 *   cds_conv2d_dgrad_s2_f32:  data gradient of Conv2d(k 3, stride 2, pad 1), weight [Co][Cin][3][3].  (Stride-1 data gradients are
 *                             cds_conv2d_f32 on flipped / transposed weights, CDS_ACT_ACCUM to sum the branches of a DynamicConv.)
 *   cds_instnorm_bwd_f32:     backward of InstanceNorm2d(eps 1e-5) + LeakyReLU(0.1) | tanh | nothing; stats = the forward's fp64
 *                             (sum, sum of squares) per (image, channel), sums = fp64 scratch of the same size.
 *   cds_dynconv_bn_stats_f32: (mean, rstd) [G][4] of the attention MLP's BatchNorm2d for G groups of N / G images - batch statistics
 *                             from the fp64 moments of the K curvature maps (use_batch), else the running ones; updates the running
 *                             statistics group after group.  mom: fp64 scratch [G][K + K (K + 1) / 2].  epipoles: DEVICE [N][2].
 *   cds_dynconv_blend_train_f32: the DynamicConv epilogue with those statistics: out [N][Cout][H][W], norm_curv [N][H][W].
 *   cds_dynconv_blend_bwd_f32:   its backward.  gbr [K][N][Cout+3][H][W] = gradient of the branch tensor; fp64: sums [G][8] =
 *                             per group (sum g_bn_j, sum g_bn_j xhat_j) (dbeta_j / dgamma_j summed over groups) followed by dw2 [K][4];
 *                             dw1 [4][K].  gnc may be NULL.
 *   cds_softargmin_bwd_f32:   gpre[d] = softmax(prob_pre)_d (hyp_d - depth) gdepth.
 * scratch_zeroed != 0: the fp64 accumulation buffers (sums / mom / dw1) arrive zero-filled (the training step zeroes ONE arena per step
 * instead of ~40 small memsets); 0: the function zeroes them itself. */
int cds_conv2d_wgrad_f32(const float* g, const float* x, float* dw, int N, int Co, int Cin, int Ho, int Wo, int H, int W, int k,
                         int stride, int pad, void* stream);
int cds_conv2d_dgrad_s2_f32(const float* g, const float* w, float* gx, int N, int Co, int Cin, int Ho, int Wo, int H, int W,
                            void* stream);
int cds_instnorm_bwd_f32(const float* gz, const float* y, const double* stats, double* sums, float* gy, int N, int C, int H, int W,
                         int act, int scratch_zeroed, void* stream);
int cds_dynconv_bn_stats_f32(const float* branches, const float* epipoles, const float* w1, double* mom, float* mean, float* rstd,
                             float* running_mean, float* running_var, int N, int G, int K, int Cout, int H, int W, float eps,
                             float momentum, int use_batch, int scratch_zeroed, void* stream);
int cds_dynconv_blend_train_f32(const float* branches, const float* epipoles, const float* w1, const float* w2, const float* gamma,
                                const float* beta, const float* mean, const float* rstd, float temperature, float* out,
                                float* norm_curv, int N, int G, int K, int Cout, int H, int W, void* stream);
int cds_dynconv_blend_bwd_f32(const float* branches, const float* epipoles, const float* w1, const float* w2, const float* gamma,
                              const float* beta, const float* mean, const float* rstd, float temperature, const float* gy,
                              const float* gnc, float* gbr, double* sums, double* dw1, int N, int G, int K, int Cout, int H, int W,
                              int use_batch, int scratch_zeroed, void* stream);
/* bf16 STORAGE of the 2D activations with fp32 accumulation (BASELINE config 5 is labelled bf16; the reference itself trains in fp32,
 * trainer/trainer.py:69-82, so this is an opt-in policy of the training step, train2d_ops.activation_storage("bf16")).  Tensors that
 * live from the forward to the backward pass - layer inputs, DynamicConv branch responses, pre-normalisation maps - are raw bfloat16
 * (unsigned short, round to nearest even); every kernel widens on load and accumulates as its fp32 twin does.
 *   cds_f32_to_bf16:             dst = bfloat16(src), n elements.
 *   cds_instnorm_act_b16_f32:    InstanceNorm2d + activation of cds_instnorm_act_f32 that also STORES: y16 = bfloat16(y) (kept for the
 *                                backward), z = act((y - mean) rstd) as out32 (the transient the next layer's forward kernel reads)
 *                                and out16 = bfloat16(z) (kept); out16 == NULL: no stored output.  strict != 0: the forward continues on
 *                                the stored values too (statistics of y16, out32 = widened out16).
 *   *_xb16 / *_yb16 / *_b16:     the fp32 entry of the same name with that operand read from its bf16-stored form.
 *                                cds_instnorm_bwd_yb16_f32 also takes the stored LeakyReLU output z16 (or NULL): its sign bit is the
 *                                gate the forward took. */
int cds_f32_to_bf16(const float* src, unsigned short* dst, long long n, void* stream);
int cds_instnorm_act_b16_f32(const float* y, unsigned short* y16, float* out32, unsigned short* out16, double* stats, int N, int C,
                             int H, int W, int act, int strict, void* stream);
int cds_conv2d_wgrad_xb16_f32(const float* g, const unsigned short* x, float* dw, int N, int Co, int Cin, int Ho, int Wo, int H, int W,
                              int k, int stride, int pad, void* stream);
int cds_instnorm_bwd_yb16_f32(const float* gz, const unsigned short* y, const unsigned short* z16, const double* stats, double* sums,
                              float* gy, int N, int C, int H, int W, int act, int scratch_zeroed, void* stream);
int cds_dynconv_bn_stats_b16_f32(const unsigned short* branches, const float* epipoles, const float* w1, double* mom, float* mean,
                                 float* rstd, float* running_mean, float* running_var, int N, int G, int K, int Cout, int H, int W,
                                 float eps, float momentum, int use_batch, int scratch_zeroed, void* stream);
int cds_dynconv_blend_train_b16_f32(const unsigned short* branches, const float* epipoles, const float* w1, const float* w2,
                                    const float* gamma, const float* beta, const float* mean, const float* rstd, float temperature,
                                    float* out, float* norm_curv, int N, int G, int K, int Cout, int H, int W, void* stream);
int cds_dynconv_blend_bwd_b16_f32(const unsigned short* branches, const float* epipoles, const float* w1, const float* w2,
                                  const float* gamma, const float* beta, const float* mean, const float* rstd, float temperature,
                                  const float* gy, const float* gnc, float* gbr, double* sums, double* dw1, int N, int G, int K,
                                  int Cout, int H, int W, int use_batch, int scratch_zeroed, void* stream);
/* The weight layouts of cds_conv2d_f32 in one launch: fwd [Cin][k k][CoP] (forward) and / or dgrad [Ca+Cb][k k][CiP] (stride-1 data
 * gradient: taps flipped, channels swapped) from wa [Ca][Cin][k][k] and, optionally, wb [Cb][Cin][k][k] stacked behind it. */
int cds_pack_conv2d_f32(const float* wa, const float* wb, float* fwd, float* dgrad, int Ca, int Cb, int Cin, int k, void* stream);
/* The forward and data-gradient weight layouts of a 3x3x3 CostRegNet layer in one launch.  w [A][B][27]; mode 0: Conv3d stride 1
 * (A = Cout, B = Cin): fwd [Cin][27][Cout], dgrad [Cout][27][Cin] with flipped taps; mode 1: Conv3d stride 2: dgrad [Cout][27][Cin]
 * unflipped (cds_deconv3d_k3s2_f32's layout); mode 2: ConvTranspose3d (A = Cin, B = Cout): fwd [Cin][27][Cout], dgrad [Cout][27][Cin]. */
int cds_pack_conv3d_f32(const float* w, float* fwd, float* dgrad, int A, int B, int mode, void* stream);
int cds_softargmin_bwd_f32(const float* prob_pre, const float* hyp, const float* gdepth, float* gpre, int D, int h, int w,
                           int hyp_per_pixel, void* stream);
/* The attention-MLP gradients of a DynamicConv from cds_dynconv_blend_bwd_f32's fp64 accumulators, one launch:
 * out = [dbeta (4) | dgamma (4) | dw2 [K][4] | dw1 [4][K]] floats (the groups summed in a fixed order). */
int cds_dynconv_bwd_finish_f32(const double* sums, const double* dw1, int G, int K, float* out, void* stream);

/* final_loss on the device (reference: models/losses.py:6-48; replaces ~90 ATen launches forward and ~150 backward per step) and the
 * feature-distance targets (models/model.py:202-207).  Sums in fp64 through per-workgroup records reduced in a fixed order.
 *   cds_loss_records(n):       records a pass over n elements writes (recA: x 4 doubles over B h w pixels; recB: x 1 over B Dp h w).
 *   cds_loss_stage_f32:        passes over one stage: depth, gt, mask [B][hw] (mask > 0.5 selects), norm_curv [B][hw] or NULL, dist / target
 *                              [B][Dp][hw] or both NULL (no feature term: the refined-depth stage), interval [B] on the DEVICE.
 *   cds_loss_final_f32:        total = sum_s weight_s (depth_s + 5 feature_s + 0.1 curvature_s), depth_loss of the last stage (device
 *                              scalars) and scalars [n_stages][4] doubles for the backward; host arrays of n_stages <= 4 entries.
 *   cds_loss_stage_bwd_f32:    gdepth [B][hw], gnc [B][hw] or NULL, gdist [B][Dp][hw] or NULL from the device scalar gtotal.
 *   cds_feat_target_f32:       target [B][D+1][hw] = |hyp - gt| / (di[b] scale) < thresh (planes < D), 1 (plane D); di [B] on the DEVICE. */
int cds_loss_records(long long elements);
int cds_loss_stage_f32(const float* depth, const float* gt, const float* mask, const float* norm_curv, const float* dist,
                       const float* target, const float* interval, int B, int hw, int Dp, double* recA, double* recB, void* stream);
int cds_loss_final_f32(const double* const* recA, const double* const* recB, const long long* pixels, const int* Dp, const float* weight,
                       const int* has_curv, int n_stages, float* total, float* depth_loss, double* scalars, void* stream);
int cds_loss_stage_bwd_f32(const float* depth, const float* gt, const float* mask, const float* dist, const float* target,
                           const float* interval, const float* gtotal, const double* scalars, float weight, int B, int hw, int Dp,
                           float* gdepth, float* gnc, float* gdist, void* stream);
int cds_feat_target_f32(const float* hyp, const float* gt, const float* di, float scale, float thresh, int B, int D, int hw,
                        float* target, void* stream);

/* Running statistics of a BatchNorm call that stacked G groups: r = keep r + sum_g group_weights[g] stat[g][c] for the mean and the
 * variance in one launch; batch_mean / batch_var [G][C], group_weights [G] on the device. */
int cds_bn_running_update_f32(const float* batch_mean, const float* batch_var, const float* group_weights, float keep, int G, int C,
                              float* running_mean, float* running_var, void* stream);

/*
 * Point-cloud evaluation (the DTU Acc / Comp protocol, the .m files of evaluations/dtu; cds_mvsnet_amd/pointcloud.py, dtu_eval.py).
 * A sparse uniform grid over a point set: fine cells of side h addressed by 63-bit keys, coarse cell (8 x 8 x 8 fine cells) in
 * the high bits, so that points sorted by key lie cell by cell and the fine cells of a coarse cell are contiguous too.
 *   frame_host  8 floats, HOST: origin x y z, cell side h, slop (bound on how far fp32 binning puts a point outside its nominal
 *               cell; every pruning test is widened by it), fine cells per axis nx ny nz (integers, each <= 2^21)
 *   points      [n][3] fp32; pts [n][4] = the grid's points sorted by key (w: the rank as int bits for thinning, unused by
 *               the queries); cell_start [F+1] int32 point offsets of the F unique fine keys cell_keys [F] (int64, ascending);
 *               coarse_start [C+1] int32 offsets into the fine cells of the C unique coarse keys (cell_keys >> 9)
 *   table_keys [2^log2_slots] int64 / table_vals [2^log2_slots] int32: hash table of the fine keys (value = fine index) and the
 *               coarse keys with bit 63 set (value = coarse index); indices are int32, so point counts up to 2^31 - 1
 * cds_grid_hash_log2_slots  size query: log2 of the table size for n_keys keys (load <= 1/2), or CDS_EINVAL
 * cds_grid_keys_f32         keys[i] = the fine key of point i, cell coordinates floor((p - o) / h) clamped to the grid
 * cds_grid_hash_build       clear the table and insert keys[0..n_keys) (unique; the first n_fine are fine keys)
 * cds_nn_query_f32          dist[order[i]] = min(distance from query[order[i]] to its nearest grid point, max_dist), in fp32 with
 *                           d2 = dx*dx + dy*dy + dz*dz: MaxDistCP.m with the block grid dropped (capped exact nearest neighbour;
 *                           PointCompareMain.m:20-26).  order: a permutation of the m queries (cell order keeps a wave's
 *                           lanes in the same cells) or NULL
 * cds_thin_round_f32        one round of the greedy thinning of reducePts_haa.m:19-31 (PointCompareMain.m:7): state [n] in
 *                           sorted order, 0 undecided / 1 kept / 2 removed.  An undecided point is removed once a lower-rank
 *                           point within min_dist (d2 <= min_dist^2, fp32) is kept and kept once none is undecided; the rounds
 *                           converge to the greedy maximal independent set in rank order bit for bit.  undecided (device int,
 *                           or NULL) is incremented for every point left undecided.  Requires h >= min_dist (27 cells cover it).
 */
int cds_grid_hash_log2_slots(long long n_keys);
int cds_grid_keys_f32(const float* points, long long n, const float* frame_host, long long* keys, void* stream);
int cds_grid_hash_build(const long long* keys, long long n_keys, long long n_fine, long long* table_keys, int* table_vals,
                        int log2_slots, void* stream);
int cds_nn_query_f32(const float* query, const long long* order, long long m, const float* pts, const int* cell_start,
                     const long long* cell_keys, const int* coarse_start, const long long* table_keys, const int* table_vals,
                     int log2_slots, const float* frame_host, float max_dist, float* dist, void* stream);
int cds_thin_round_f32(const float* pts, const int* cell_start, long long n, const long long* table_keys, const int* table_vals,
                       int log2_slots, const float* frame_host, float min_dist, unsigned char* state, int* undecided,
                       void* stream);

/*
 * Registration and preparation of point clouds for the Tanks and Temples F-score (csrc/registration.hip; cds_mvsnet_amd/tt_eval.py,
 * DESIGN.md 1.6).  The grid arguments (pts .. frame_host) are those of cds_nn_query_f32, of a grid whose w lane holds each
 * point's input index as int bits (PointGrid with rank = arange(N)).
 * cds_transform_points_f32  out[i] = fp32(T points[i]): T 12 doubles on the DEVICE (row-major 3x4), row r computed in float64 as
 *                           ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3], every product and sum rounded separately, then
 *                           rounded once to fp32.  out may not alias points.
 * cds_nn_index_f32          the walk of cds_nn_query_f32 with the nearest point's input index: the smallest d2 = dx*dx + dy*dy +
 *                           dz*dz (fp32) wins, among equal d2 the lowest input index; accepted only if d2 < max_dist^2.
 *                           dist[i] as cds_nn_query_f32 (max_dist when nothing is accepted), index[i] int32, -1 in that case.
 * cds_icp_sums_f64          one point-to-point registration step.  Per source point s (source [m][3] fp32, m >= 1):
 *                           p = fp32(T s) as cds_transform_points_f32, q = the nearest target of p as cds_nn_index_f32.  Over
 *                           the accepted pairs, out [CDS_ICP_SUMS] doubles on the DEVICE:
 *                             [0] count   [1..3] sum p   [4..6] sum q   [7 + 3r + c] sum q[r] p[c]   [16] sum |p - q|^2
 *                             [17] sum |p|^2 (the scale of the similarity update divides by the variance of p)
 *                           in fp64 from the fp32 values, |p - q|^2 = (dx dx + dy dy) + dz dz, |p|^2 likewise.  Summed in a fixed order
 *                           (per-workgroup records in ws, ws_doubles >= CDS_ICP_WS_DOUBLES; a second pass whose shape depends
 *                           on m only; no atomics): bit-reproducible for the same inputs.  order: a permutation of the m source
 *                           points that the lanes follow (it fixes the order of the sums as well) or NULL.  index [m] int32 /
 *                           dist [m] fp32: the per-point results as cds_nn_index_f32, or NULL.
 * cds_voxel_mean_f32        voxel v of n_voxels holds the points perm[start[v] .. start[v + 1]) (perm [n] int64 input indices,
 *                           start [n_voxels + 1] int32); out[v] = their mean, accumulated in fp64 in that order, divided by the
 *                           count and rounded once to fp32.  The keys, the stable sort and the offsets are the caller's
 *                           (cds_grid_keys_f32 + torch), so the output order is the caller's voxel order.
 * cds_polygon_crop_f32      keep[i] (uint8 0 / 1) for points [n][3] fp32, all arithmetic in fp64.  axis w = 0 / 1 / 2 (X / Y / Z) with
 *                           (u, v) = (Y, Z) / (X, Z) / (X, Y); polygon [P][3] doubles on the DEVICE, 3 <= P <= CDS_CROP_MAX_VERTICES.
 *                           Kept iff axis_min <= p[w] <= axis_max and an odd number of edges (a = polygon[i], b = polygon[(i+1) % P])
 *                           have (p[v] < a[v]) != (p[v] < b[v]) and a[u] + (p[v] - a[v]) / (b[v] - a[v]) * (b[u] - a[u]) < p[u],
 *                           evaluated in that order with IEEE divide.
 */
#define CDS_ICP_SUMS 18
#define CDS_ICP_MAX_GROUPS 1024 /* workgroups of the first pass of cds_icp_sums_f64 */
#define CDS_ICP_WS_DOUBLES (CDS_ICP_MAX_GROUPS * CDS_ICP_SUMS)
#define CDS_CROP_MAX_VERTICES 256
int cds_transform_points_f32(const float* points, long long n, const double* T, float* out, void* stream);
int cds_nn_index_f32(const float* query, const long long* order, long long m, const float* pts, const int* cell_start,
                     const long long* cell_keys, const int* coarse_start, const long long* table_keys, const int* table_vals,
                     int log2_slots, const float* frame_host, float max_dist, float* dist, int* index, void* stream);
int cds_icp_sums_f64(const float* source, const long long* order, long long m, const double* T, const float* pts,
                     const int* cell_start, const long long* cell_keys, const int* coarse_start, const long long* table_keys,
                     const int* table_vals, int log2_slots, const float* frame_host, float max_dist, double* ws,
                     long long ws_doubles, double* out, int* index, float* dist, void* stream);
int cds_voxel_mean_f32(const float* points, long long n, const long long* perm, const int* start, long long n_voxels, float* out,
                       void* stream);
int cds_polygon_crop_f32(const float* points, long long n, const double* polygon, int P, int axis, double axis_min,
                         double axis_max, unsigned char* keep, void* stream);

/*
 * Outlier removal for fused clouds (csrc/cloud_outlier.hip; cds_mvsnet_amd/pointcloud.py remove_outliers).  The
 * grid arguments (pts .. frame_host) are those of cds_nn_query_f32; query [m][3] fp32, order as there.  The kernels read only
 * their inputs and use no atomics, so every result is a function of the inputs.
 * cds_knn_mean_f64       per query q: d2 = (dx dx + dy dy) + dz dz in fp32 to every grid point (a query that is a grid point finds
 *                        itself at 0); the accepted candidates are the k smallest d2 among those with d2 < max_dist^2 (fp32
 *                        product; with max_dist = +inf every point), a multiset, so ties need no rule.  terms = k, or with
 *                        max_dist = +inf the number accepted, min(k, n).  t_j = sqrt in fp64 of the fp32 d2 for the accepted in
 *                        ascending d2 order, then (double)max_dist for each missing term;
 *                        mean[q] = (((0 + t_0) + t_1) + ...) / terms, one IEEE divide.  kth[q] (or NULL) = sqrtf of the largest
 *                        accepted d2 when no term is missing, else max_dist.  1 <= k <= CDS_KNN_MAX_K, max_dist >= 0.  A query
 *                        with fewer than k points within max_dist walks the grid until the pruning bounds pass max_dist; with
 *                        max_dist = +inf and fewer than k grid points, the whole grid.
 * cds_knn_mean_wg_f64    cds_knn_mean_f64 with the workgroup size as an argument, for measurements: threads = 64, 128 or 256
 *                        (cds_knn_mean_f64 is threads = 64, one wave).  The candidate lists take k * threads * 4 bytes of LDS;
 *                        results do not depend on it.
 * cds_radius_count_f32   count[q] = min(number of grid points with d2 <= radius^2 (fp32), cap), cap >= 1; the scan may stop at
 *                        cap.  Requires cell side h >= radius (CDS_EINVAL otherwise), as cds_thin_round_f32.
 * cds_outlier_stats_f64  out[0] = mu = S(x) / n and out[1] = sigma = sqrt(S((x - mu)^2) / (n - 1)), 0 for n = 1; x [n] doubles,
 *                        out [2] doubles on the DEVICE, n >= 1.  S sums its terms in this order: consecutive chunks of
 *                        CDS_STAT_CHUNK = 4096 terms, the tail padded with +0.0; in a chunk lane l of 256 starts from +0.0 and
 *                        adds terms l, l + 256, ..., l + 15 * 256 in that order; the lanes fold by lane[l] += lane[l + s] for
 *                        s = 128, 64, ..., 1; the chunk sums are added to +0.0 in ascending chunk order.  Two passes (mu, then
 *                        the squared deviations d * d with d = x - mu).  ws: ws_doubles >= ceil(n / CDS_STAT_CHUNK).
 */
#define CDS_KNN_MAX_K 64
#define CDS_STAT_CHUNK 4096
int cds_knn_mean_f64(const float* query, const long long* order, long long m, const float* pts, const int* cell_start,
                     const long long* cell_keys, const int* coarse_start, const long long* table_keys, const int* table_vals,
                     int log2_slots, const float* frame_host, int k, float max_dist, double* mean, float* kth, void* stream);
int cds_knn_mean_wg_f64(const float* query, const long long* order, long long m, const float* pts, const int* cell_start,
                        const long long* cell_keys, const int* coarse_start, const long long* table_keys, const int* table_vals,
                        int log2_slots, const float* frame_host, int k, float max_dist, double* mean, float* kth, int threads,
                        void* stream);
int cds_radius_count_f32(const float* query, const long long* order, long long m, const float* pts, const int* cell_start,
                         const long long* cell_keys, const int* coarse_start, const long long* table_keys, const int* table_vals,
                         int log2_slots, const float* frame_host, float radius, int cap, int* count, void* stream);
int cds_outlier_stats_f64(const double* x, long long n, double* ws, long long ws_doubles, double* out, void* stream);

/*
 * Trajectory alignment of the Tanks and Temples protocol (csrc/ransac.hip, csrc/ransac_common.hpp): RANSAC for
 * the similarity that maps src onto dst, correspondence i <-> i (src, dst [n][3] doubles on the DEVICE), all in float64.
 * cds_ransac_similarity_f64  hypothesis h of `hypotheses` (one per lane) draws k distinct indices (CDS_RANSAC_MIN_SAMPLE <= k <=
 *                            CDS_RANSAC_MAX_SAMPLE) from (seed, h) alone: draw j takes z = splitmix64(seed, 8 h + j),
 *                            r = floor(z (n - j) / 2^64), then r += 1 for every earlier pick <= r, walking them in ascending
 *                            order.  T = Umeyama with scaling on the k pairs (sums in draw order, covariance
 *                            sum q p^T / k - mean_q mean_p^T, 3x3 SVD in the lane, E = diag(1, 1, +-1) from det(U) det(V)).
 *                            Rejected (count 0, err2 +inf): variance of p zero, second singular value <= 1e-9 of the first,
 *                            an entry of T not finite, n < k.  Score: d2_i = |T src_i - dst_i|^2, inlier iff d2_i < threshold^2;
 *                            count = inliers, err2 = sum of their d2 in index order.  The winner is the first in the total
 *                            order (larger count, smaller err2, smaller h): identical bytes run to run.
 *                            out [CDS_RANSAC_RECORD] doubles on the DEVICE: [0] h  [1] count  [2] err2  [3..14] T (rows of
 *                            the 3x4); with no hypothesis, or every one rejected: h = -1, count 0, err2 +inf, the identity.
 *                            count [hypotheses] int32 / err2 [hypotheses] doubles: every hypothesis's score, or NULL.
 *                            ws: ws_doubles >= CDS_RANSAC_RECORD * ceil(hypotheses / 256).  n, hypotheses < 2^31.
 */
#define CDS_RANSAC_RECORD 15
#define CDS_RANSAC_MIN_SAMPLE 3
#define CDS_RANSAC_MAX_SAMPLE 8
int cds_ransac_similarity_f64(const double* src, const double* dst, long long n, long long hypotheses, int k, double threshold,
                              unsigned long long seed, double* ws, long long ws_doubles, double* out, int* count, double* err2,
                              void* stream);

/*
 * Gipuma-style depth-map fusion (the reference's --filter_method gipuma, gipuma.py:153-195, which runs the external fusibile;
 * cds_mvsnet_amd/gipuma.py).  The rule, its fp32 operation order and the points where it fixes behaviour fusibile leaves open
 * are in the header comment of csrc/gipuma.hip.  Views share one h x w; V h w < 2^31.
 *   depths [V][h][w], confs [V][3][h][w] fp32, rgb8 [V][h][w][3] uint8 (device); prob_thresh_host 3 floats (HOST)
 *   views [V][24]: per view P (3x4 row-major, float32 of K E[:3] in float64), Minv = inverse(P[:, :3]) (3x3), 3 unused
 *   fb [V][V]: fb[r][j] = K_r[0][0] |c_r - c_j|, c_v = -Minv_v P_v[:, 3]
 *   used [V][h][w] uint8 (0 on entry to the first view); emit [tiles * 4096] uint8, zeroed, 16-byte aligned;
 *   records [V][h][w][4] words (16-byte aligned): x y z bits and packed colour of every emitted pixel
 * cds_gipuma_tiles            size query: compaction tiles (4096 flags each) for n = V h w flags, or CDS_EINVAL
 * cds_gipuma_prob_filter_f32  depth_out = the probability-filtered depths D'; rgb_out [V][h][w] = r | g << 8 | b << 16
 * cds_gipuma_fuse_view_f32    reference view r: emit / records of its pixels, used marks of the other views.  Call for
 *                             r = 0 .. V-1 in order on one stream (the views depend on each other through `used`)
 * cds_gipuma_scan             tile_count [tiles], tile_off [tiles] (exclusive offsets of the emitted points), *total (device)
 * cds_gipuma_compact_f32      the emitted points in order r, y, x: points [total][3], colors [total] packed, ref_view [total]
 */
int cds_gipuma_tiles(long long n);
int cds_gipuma_prob_filter_f32(const float* depths, const float* confs, const unsigned char* rgb8, int V, int h, int w,
                               const float* prob_thresh_host, float* depth_out, unsigned* rgb_out, void* stream);
int cds_gipuma_fuse_view_f32(const float* depths, const unsigned* rgb, const float* views, const float* fb, int r, int V, int h,
                             int w, float depth_min, float depth_max, float disp_thresh, int num_consistent, unsigned char* used,
                             unsigned char* emit, unsigned* records, void* stream);
int cds_gipuma_scan(const unsigned char* emit, int tiles, int* tile_count, int* tile_off, int* total, void* stream);
int cds_gipuma_compact_f32(const unsigned char* emit, const unsigned* records, const int* tile_off, int tiles, int hw,
                           float* points, unsigned* colors, int* ref_view, void* stream);

/*
 * COLMAP sparse model -> MVSNet scene (the reference's colmap2mvsnet.py; cds_mvsnet_amd/colmap.py).  float64 throughout;
 * the rule and the operation order are in the header comment of csrc/colmap.hip.  All pointers are device memory.
 *   Images are numbered 0 .. N-1 and points 0 .. P-1 by the caller.
 *   ptr [P+1], img [ptr[P]], cnt [ptr[P]]: CSR over points of the (point, image) observations, sorted and unique, the images
 *   of a point ascending, cnt = how often that image observes that point;  pair_off [P+1]: exclusive prefix sum of
 *   L_p (L_p - 1) / 2 with L_p = ptr[p+1] - ptr[p], T = pair_off[P];  xyz [P][3];  centres [N][3] = -R^T t
 *   acc [limbs][N][N] int64, 2 <= limbs <= CDS_COLMAP_SCORE_MAX_LIMBS, zeroed by the caller: only entries i < j are written; limb k is in units of
 *   2^-40(k+1), and S[i][j] = sum_k acc[k][i][j] 2^-40(k+1).  The caller guarantees that no pair can reach 2^23 cnt-weighted terms.
 * cds_colmap_score_limbs        the limbs that keep the two leading limbs of the smallest weight the rule can produce for
 *                                these parameters (7 at theta0 5, sigma 1 / 10; at most 28, which covers every nonzero double)
 * cds_colmap_score_quantum_log2  80: every term enters with an absolute error below q = 2^-80 per occurrence
 * cds_colmap_pair_scores_f64     for every point that images i < j share: the first nonzero 40-bit limb of w and the next
 *                                one, times cnt_i, are added to their acc[k][i][j]
 * cds_colmap_obs_depth_f64       z[e] = ((r0 x + r1 y) + r2 z) + r3 with r = zrow[obs_img[e]] (row 2 of [R | t]) and
 *                                (x, y, z) = xyz[obs_pt[e]], for the n valid observations
 * cds_colmap_depth_ranges_f64    z_sorted: per image (obs_ptr [N+1]) its z values ascending; out [N][2] = the mean of the
 *                                lowest min(num_min[i], n_i) and of the highest min(num_max[i], n_i), summed ascending;
 *                                every image needs n_i >= 1 and num_min, num_max >= 1
 */
#define CDS_COLMAP_SCORE_QUANTUM_LOG2 80
#define CDS_COLMAP_SCORE_MAX_LIMBS 28
int cds_colmap_score_quantum_log2(void);
int cds_colmap_score_limbs(double theta0, double sigma1, double sigma2);
int cds_colmap_pair_scores_f64(const long long* pair_off, const long long* ptr, const int* img, const int* cnt,
                               const double* xyz, const double* centres, long long P, long long T, int N, double theta0,
                               double sigma1, double sigma2, int limbs, long long* acc, void* stream);
int cds_colmap_obs_depth_f64(const int* obs_img, const long long* obs_pt, const double* xyz, const double* zrow, long long n,
                             double* z, void* stream);
int cds_colmap_depth_ranges_f64(const double* z_sorted, const long long* obs_ptr, const int* num_min, const int* num_max,
                                int N, double* out, void* stream);

/* Depth maps scored against ground truth, and the multi-scale ground truth itself (csrc/depth_metrics.hip; reference: utils.py:134-167
 * as trainer/trainer.py:140-164 calls them, evaluations/precision.py:8-13,87-91, datasets/dtu_yao.py:79-128,
 * datasets/blended_dataset.py:79-120).
 *
 * cds_depth_metrics_f32   est, gt, mask [B][hw]; thr [B][T] on the DEVICE, ascending per image, 0 <= T <= CDS_DEPTH_METRICS_MAX_T (NULL
 *                         at T = 0).  Per image b, over the pixels with mask > 0.5, e = fabsf(est - gt) in fp32, out [b][3T + 5]:
 *                           [0] n   [1] sum e   [2] sum e^2 (the fp32 e squared in fp64)   [3 + t] #{e > thr[b][t]}
 *                           [3 + T + 2k], [3 + T + 2k + 1]: count and sum of e over lo_k <= e <= hi_k for the T + 1 bands
 *                           [0, thr0], [thr0, thr1], ..., [thr_{T-1}, cap] - inclusive at BOTH ends (utils.py:164): an error exactly on
 *                           a threshold lies in two bands.
 *                         Every comparison is fp32 against the fp32 threshold; sums are fp64 in a fixed order (per-workgroup records in
 *                         ws, reduced by a second pass; no atomics): bit-reproducible.  A NaN error counts in n and makes the two sums
 *                         NaN; it exceeds no threshold and lies in no band.  One call handles all B images; any hw >= 1.
 *                         ws: ws_doubles >= CDS_DEPTH_METRICS_WS_DOUBLES(B) doubles of workspace.
 * cds_gt_pyramid_f32      src [Hs][Ws]: a depth map.  Level 0 pixel (y, x) = src(rows[y], cols[x]) (rows [h], cols [w]: int32 tables on
 *                         the DEVICE - the resize / crop rule is the host's), level k < levels <= 4 pixel (y, x) = level 0 pixel
 *                         (y 2^k, x 2^k): cv2.resize(INTER_NEAREST) to (w / 2^k, h / 2^k) when h and w are multiples of 2^(levels-1),
 *                         which is required.  mask = mask_src(rows[y], cols[x]) > mask_thresh ? 1 : 0 (mask_src [Hs][Ws] uint8; DTU: 10,
 *                         dtu_yao.py:99), or with mask_src NULL depth > 0 ? 1 : 0 (blended_dataset.py:110).  depth_out, mask_out: the
 *                         levels packed one after the other, level k = (h >> k) x (w >> k) floats.  One launch writes everything.  A
 *                         table entry outside the source yields depth 0, mask 0. */
#define CDS_DEPTH_METRICS_MAX_T 8
#define CDS_DEPTH_METRICS_MAX_GROUPS 1024 /* workgroups of the first pass over all images (at least one per image) */
#define CDS_DEPTH_METRICS_WS_DOUBLES(B) \
  ((long long)(B) * (CDS_DEPTH_METRICS_MAX_GROUPS / (B) < 1 ? 1 : CDS_DEPTH_METRICS_MAX_GROUPS / (B)) * (3 * CDS_DEPTH_METRICS_MAX_T + 5))
int cds_depth_metrics_f32(const float* est, const float* gt, const float* mask, const float* thr, float cap, int B, long long hw, int T,
                          double* ws, long long ws_doubles, double* out, void* stream);
int cds_gt_pyramid_f32(const float* src, const unsigned char* mask_src, int mask_thresh, int Hs, int Ws, const int* rows, const int* cols,
                       int h, int w, int levels, float* depth_out, float* mask_out, void* stream);

/* Training images from decoded bytes (csrc/train_data.hip; reference: datasets/dtu_yao.py:73-77,176, datasets/blended_dataset.py:79-92,165:
 * np.array(img, float32) / 255., centre crop, stack, transpose(0, 3, 1, 2) on the host).
 *
 * cds_image_batch_u8      src [n][Hs][Ws][3] uint8, the decoded images; rows [h], cols [w]: int32 tables on the DEVICE, the format of
 *                         cds_gt_pyramid_f32 (a centre crop is two ranges).  out [n][3][h][w] fp32:
 *                           out[i][c][y][x] = (float)src[i][rows[y]][cols[x]][c] / 255.0f
 *                         - a true fp32 division, bit-equal to numpy's float32 / 255.; a multiplication by 1 / 255.f is not.  A table
 *                         entry outside the source yields 0.  One launch: a thread owns four consecutive x of one row, reads their
 *                         12 bytes once and writes the three planes with 16-byte stores when w % 4 == 0 and out is 16-byte aligned,
 *                         with scalar stores otherwise.  out, rows, cols must be 4-byte aligned. */
int cds_image_batch_u8(const unsigned char* src, int n, int Hs, int Ws, const int* rows, const int* cols, int h, int w, float* out,
                       void* stream);

/* Evaluation views from decoded bytes and the side outputs of a depth map (csrc/eval_data.hip; reference: datasets/general_eval.py:88-118
 * - float32 / 255., the Tanks & Temples edge padding, cv2.resize(INTER_LINEAR) of the float32 image - and test.py:216-248).
 *
 * cds_eval_views_u8       src [V][Hs][Ws][3] uint8, the decoded views; row0, row1 [h] and col0, col1 [w]: int32 tap tables, fy [h] and
 *                         fx [w]: fp32 weights of the second tap, all on the DEVICE (the host builds them by OpenCV's rule; the edge
 *                         padding is a clamp inside the row tables).  out [V][3][h][w] fp32, with S = (float)src / 255.0f (a true
 *                         division):
 *                           R_k = S[row_k][col0] * (1.f - fx) + S[row_k][col1] * fx        k = 0, 1
 *                           out = R_0 * (1.f - fy) + R_1 * fy
 *                         every operation rounded to fp32 on its own (no FMA): numpy float32 arithmetic reproduces it bit for bit,
 *                         and fx = fy = 0 gives u8 / 255 exactly.  Tap indices are clamped to the source.  One launch; a thread owns
 *                         four consecutive x of one row and writes 16-byte stores when w % 4 == 0 and out is 16-byte aligned.
 *                         Tables and out must be 4-byte aligned.
 * cds_eval_outputs_f32    c1 [H1][W1], c2 [H2][W2], c3 [H3][W3]: the stage confidences; img [3][Hi][Wi]: the reference image.
 *                         tab: int32 on the DEVICE, source rows of c1, c2, c3, img for each output row ([h] each), then source columns
 *                         ([w] each) - nearest-neighbour tables built on the host, clamped to the sources here.
 *                         conf3 [h][w][3] = the three confidences; img_u8 [h][w][3] = (uint8)clip(img * 255.0f, 0, 255): one rounded
 *                         fp32 multiply, then truncation.  One launch. */
int cds_eval_views_u8(const unsigned char* src, int V, int Hs, int Ws, const int* row0, const int* row1, const float* fy, const int* col0,
                      const int* col1, const float* fx, int h, int w, float* out, void* stream);
int cds_eval_outputs_f32(const float* c1, int H1, int W1, const float* c2, int H2, int W2, const float* c3, int H3, int W3,
                         const float* img, int Hi, int Wi, const int* tab, int h, int w, float* conf3, unsigned char* img_u8,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CDS_MVSNET_HIP_H */
