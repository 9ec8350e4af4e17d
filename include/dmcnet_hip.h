/*
 * dmcnet_hip.h -- C ABI of libdmcnet_hip.so: the MI355X (gfx950) kernels behind the DMC-Net
 * training hot path.
 *
 * The reference (facebookresearch/dmc-net) has NO FFI seam on this path: its hot path is stock
 * torch.nn modules driven from Python.  Each entry point below therefore
 * names the reference Python it replaces (paths relative to the reference root); the binding a
 * maintainer adds on the reference side is the ctypes stub in INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes, no torch types; every pointer is a DEVICE pointer unless it
 *     says "host";
 *   - the caller owns every buffer, workspaces included; nothing here allocates, frees or
 *     synchronises; every launch is asynchronous on `stream` (a hipStream_t; NULL = the
 *     null stream);
 *   - tensors are contiguous NCHW fp32; weights are in PyTorch's native [Cout][Cin][3][3]
 *     layout with the reference's prepend-concat input-channel order
 *     (code/dmcnet/model.py:187-194: layer k sees [y_{k-1}, ..., y_0, mv(2), residual(3)]);
 *   - return value: DMC_OK (0) or a negative DMC_E_* code; dmc_last_error() gives the text
 *     (thread-local);
 *   - the ONLY process-wide state is the table of kernel-selection options behind dmc_set_option() (A/B
 *     measurement knobs, relaxed atomics, defaults = fastest path; an operator reads them at each of its
 *     entry points, so do not change them while another thread is between two calls of one operator); the
 *     library never reads the environment; otherwise safe from several host threads on distinct streams.
 */
#ifndef DMCNET_HIP_H
#define DMCNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMC_OK 0
#define DMC_E_INVALID (-1) /* bad argument (null pointer, non-positive size, ...) */
#define DMC_E_LAUNCH (-2)  /* hipLaunch / hipGetLastError failure                */

typedef void* dmc_stream_t; /* hipStream_t */

/* Library version: major*10000 + minor*100 + patch. */
int dmc_version(void);
/* Text of the last error on this host thread ("" if none). */
const char* dmc_last_error(void);
/* Kernel-selection options for A/B measurements (tools/, bench.py); every default is the fastest measured path.
 *   "gen_fused"       1 (default): the generator forward as ONE launch (gen_fused.hip: strips of <= 118 columns walked row by row,
 *                     features line-buffered in LDS, the six layers pipelined across the waves of a workgroup; any H, W <= 224);
 *                     0: the layer-by-layer kernels, which also serve wider images.  Bit 0 only: values 0 and 1.
 *   "gen_layer_path"  1 (default) / 0: matrix-core / VALU layer kernels of the layer-by-layer forward and the data gradient.
 *                     Values 0 and 1.
 *   "gen_gather"      0: push form for the Cout-8 layers.        "gen_fuse45"  0: layers 4 and 5 as two launches.
 *   "gen_wgrad_path"  5 (default): the row-sliding weight gradient of gen_wgrad.hip (W % 4 == 0, else path 4's rules); 4: the bf16x3
 *                     tile kernel.  Values 4 and 5.
 *   "gen_fuse_fwd" / "gen_fuse_bwd"  0: the layer-by-layer forward / data-gradient launches instead of the fused groups.
 *   "gen_x3"          bit K: hidden layer K (0 .. 2) of the layer-by-layer forward in bf16x3 arithmetic (gen_x3.hip); default 2.
 *   "gen_wino"        bit K: hidden layer K (0 .. 3) of the layer-by-layer forward, bit 8 + K: data-gradient group K (0 .. 4), on the
 *                     Winograd F(2x2, 3x3) ring kernel (fp32, results within rounding of the direct kernels'; W % 4 == 0,
 *                     64 <= W <= 224); default 768 = gradient groups 0 and 1.
 *   "conv_path" / "conv_arith" / "conv_cfg"  classifier / discriminator / I3D convolutions: second-generation kernels (1), bf16x3
 *                     arithmetic (1) or fp32 MFMA (0), and a forced tile configuration (0 = automatic; 1 .. 5 tiles of the
 *                     tap-stepping 3-D kernel, 6 = never the patch-resident 3x3x3 kernel, 7 / 8 = its 128- / 64-position tiles,
 *                     9 = the scan form of the 3-D max pool, 11 / 12 = the first forms of the I3D stem's weight / data gradient (LDS scatter; one or four rows per wave),
 *                     101 .. 305 = 2-D tile choices named in the kernels).
 *   "conv3d_wgrad"    2 (default): row-ring weight gradient for 3x3x3 and 1x1x1; 1: 3x3x3 only; 0: tap-stepping kernels.
 *   "grid_reserve_cus" 0 (default) .. 128: CUs every PERSISTENT grid (gen_fused, the generator's ring / gather / Winograd kernels,
 *                     gen_wgrad_rs, conv3d_p3) leaves idle -- room for RCCL's channel kernels while gradients are exchanged
 *                     during the backward pass; buffer-size queries do not depend on it; no result changes.
 *   "gen_ablate" / "conv_ablate" (parts of a kernel switched off, results wrong), "gen_stagger": MEASUREMENT BUILD ONLY
 *                     (-DDMC_MEASURE, dmc-net_amd/build.py --measure -> libdmcnet_hip_measure.so): the product library refuses
 *                     them, they read 0 and the ablated paths are not compiled into its kernels.
 * "gen_fused", "gen_layer_path" and "gen_wgrad_path" accept the values named above and no others, in both builds (the kernel
 * variants that further values once selected lost their A/B measurement and are removed); the error text names the option and its
 * accepted values, and the option keeps the value it had.  dmc_get_option("measure_build") reads 1 in the measurement build, 0 in
 * the product library.
 * dmc_set_option returns DMC_E_INVALID for an unknown name or a refused value; dmc_get_option returns -1 for an unknown name. */
int dmc_set_option(const char* name, int value);
int dmc_get_option(const char* name);
/* Launches an empty kernel named dmc_profile_mark_kernel on `stream`: a marker that brackets
 * a region of interest in a rocprofv3 kernel trace (no reference counterpart; tooling only). */
int dmc_profile_mark(dmc_stream_t stream);

/* ---- EstimatorDenseNetTiny (the DMC generator every shipped recipe uses) ----------------
 * Replaces: EstimatorDenseNetTiny.forward            code/dmcnet/model.py:187-194
 *           + torch.cat((mv, residual), 1)            code/dmcnet/model.py:341
 *           + torch.add(gen_flow, input_mv)           code/dmcnet/model.py:345-346
 * Layer widths 5->8, 13->8, 21->6, 27->4, 31->2, 33->2 (last one without LeakyReLU(0.1)).
 *
 * w[6], b[6] (host arrays of device pointers): conv_0..conv_4 `.0.weight/.0.bias`, then
 * predict_flow.weight/.bias.
 */

/* Bytes of `workspace` the generator entry points need (repacked weights, zero words, bf16x3 weight fragments). */
size_t dmc_gen_tiny_workspace_bytes(void);
/* Bytes of the saved-activation buffer for N frames of H x W (28 channels fp32). */
size_t dmc_gen_tiny_saved_bytes(int N, int H, int W);

/*
 * Forward.  mv [N,2,H,W], res [N,3,H,W] -> out [N,2,H,W].
 * saved: buffer of dmc_gen_tiny_saved_bytes(); it receives y0..y4 (the post-LeakyReLU features, physical channel order) for
 * the backward pass.  NULL = inference (nothing is kept: the forward then writes 8 instead of 120 bytes per pixel): accepted
 * when the one-launch forward serves the shape (option "gen_fused" bit 0, W <= 224), DMC_E_INVALID otherwise -- the
 * layer-by-layer kernels pass the features from launch to launch through this buffer.
 * workspace: dmc_gen_tiny_workspace_bytes() (repacked weights + 256 zero words + the bf16x3 weight fragments of gen_x3.hip).
 * add_mv_delta != 0 adds input_mv to the result (gen_flow_or_delta == 1).
 * Any H, W >= 1; W % 4 == 0 takes the vectorised path.
 */
int dmc_gen_tiny_fwd(const float* mv, const float* res, const float* const* w,
                     const float* const* b, float* out, float* saved, float* workspace, int N,
                     int H, int W, int add_mv_delta, dmc_stream_t stream);

/*
 * Forward + flow-reconstruction loss in one go: as dmc_gen_tiny_fwd, and additionally
 * *loss_out = mean((out - flow)^2) = nn.MSELoss()(gen_flow, input_flow), code/dmcnet/train.py:167,245,
 * reduced in the epilogue of the kernel that produces `out` (the separate loss kernel would read `out`
 * back from HBM).  flow [N,2,H,W]; loss_out: one float on the device; mse_partials: workspace of
 * dmc_gen_tiny_mse_partials_bytes().  Shapes that do not reach a kernel with the loss epilogue (W > 224; with option
 * "gen_fused" 0 also W % 4 != 0) fall back to dmc_flow_mse_fwd internally.  The gradient is dmc_flow_mse_bwd's, unchanged.
 */
size_t dmc_gen_tiny_mse_partials_bytes(void);
int dmc_gen_tiny_fwd_mse(const float* mv, const float* res, const float* const* w, const float* const* b,
                         const float* flow, float* out, float* saved, float* workspace, float* loss_out,
                         void* mse_partials, int N, int H, int W, int add_mv_delta, dmc_stream_t stream);

/*
 * The same with the loss kind chosen (--loss-mse MSELoss | SmoothL1Loss | L1, code/dmcnet/train.py:166-172, applied as
 * criterion_mse(gen_flow, input_flow), code/dmcnet/train.py:245): kind 0 = MSE, 1 = SmoothL1 (beta 1), 2 = L1, the terms
 * of dmc_flow_loss_fwd below.  The layer-5 epilogue of the one-launch forward accumulates l(out - flow) in the same double
 * accumulators and partial layout (mse_partials: dmc_gen_tiny_mse_partials_bytes()); the kind is a compile-time argument
 * of that kernel, and kind 0 IS dmc_gen_tiny_fwd_mse (same kernels, same bits).  Shapes the one-launch forward does not
 * serve (W > 224, option "gen_fused" 0) fall back to dmc_flow_loss_fwd internally.  No attention form: the attention
 * estimator is not this generator.  The gradient is dmc_flow_loss_bwd's.  kind outside 0 .. 2, a NULL pointer (saved
 * excepted, as for dmc_gen_tiny_fwd) or a non-positive size: DMC_E_INVALID before any launch.
 */
int dmc_gen_tiny_fwd_loss(int kind, const float* mv, const float* res, const float* const* w, const float* const* b,
                          const float* flow, float* out, float* saved, float* workspace, float* loss_out,
                          void* mse_partials, int N, int H, int W, int add_mv_delta, dmc_stream_t stream);

/* Bytes of the gradient-feature buffer (`gbuf`) and of the per-workgroup weight-gradient
 * partials (`partials`) that the backward needs. */
size_t dmc_gen_tiny_gbuf_bytes(int N, int H, int W);
size_t dmc_gen_tiny_partials_bytes(int N, int H, int W);

/*
 * Backward (autograd of the stack above; replaces loss.backward() through
 * code/dmcnet/model.py:187-194).  grad_out [N,2,H,W] is dL/d(out).
 * Writes dw[6], db[6] (host arrays of device pointers, same shapes as w, b; overwritten, not
 * accumulated).  Gradients w.r.t. mv/res through the convolutions are not produced (the
 * reference never asks for them); in delta mode dL/d(mv) through the skip is grad_out itself.
 */
int dmc_gen_tiny_bwd(const float* mv, const float* res, const float* const* w,
                     const float* saved, const float* grad_out, float* const* dw,
                     float* const* db, float* gbuf, float* partials, float* workspace, int N,
                     int H, int W, dmc_stream_t stream);

/* ---- flow reconstruction loss --------------------------------------------------------------
 * Replaces: nn.MSELoss()(gen_flow, input_flow)        code/dmcnet/train.py:167,245
 * (mean over all `numel` elements).  partials: workspace of dmc_flow_mse_partials_bytes().
 * loss_out: one float on the device.
 */
size_t dmc_flow_mse_partials_bytes(void);
int dmc_flow_mse_fwd(const float* gen_flow, const float* flow, float* loss_out, float* partials,
                     size_t numel, dmc_stream_t stream);
/* grad_gen = 2 (gen - flow) / numel * (*grad_loss) ; grad_loss is a device scalar. */
int dmc_flow_mse_bwd(const float* gen_flow, const float* flow, const float* grad_loss,
                     float* grad_gen, size_t numel, dmc_stream_t stream);

/* ---- flow reconstruction loss, every criterion of the reference ------------------------------
 * Replaces: criterion_mse = nn.MSELoss() | nn.SmoothL1Loss() | nn.L1Loss()   (--loss-mse, code/dmcnet/train.py:166-172)
 *           criterion_mse(gen_flow, input_flow)                               code/dmcnet/train.py:245
 *           criterion_mse(att_flow * gen_flow, att_flow * input_flow)         code/dmcnet/train.py:335,
 *                                                                             code/dmcnet_GAN/train.py:352
 * kind: 0 = MSE, 1 = SmoothL1 (beta 1), 2 = L1.  att: NULL (plain form) or [numel] weights.  In fp32:
 *   x = att ? att * gen : gen,  y = att ? att * flow : flow  (each product rounded before the subtraction),  d = x - y,
 *   l(d)  = d^2            | (|d| < 1 ? 0.5 d^2 : |d| - 0.5) | |d|,
 *   l'(d) = 2 d            | (|d| < 1 ? d : sign(d))         | sign(d), sign(0) = 0,
 *   *loss_out = mean of l(d) over all `numel` elements.
 * One streaming pass (16-byte loads: every array 16-byte aligned), per-lane partials promoted to double, every sum in a
 * fixed order: no atomics, repeated runs are bit-identical.  partials: workspace of dmc_flow_loss_partials_bytes().
 * kind 0 without att runs dmc_flow_mse_fwd / _bwd's kernels and gives their bits.
 * DMC_E_INVALID before any launch (nothing written): kind outside 0 .. 2, a NULL pointer (att / grad_att excepted),
 * numel == 0, grad_att given without att.
 */
size_t dmc_flow_loss_partials_bytes(void);
int dmc_flow_loss_fwd(int kind, const float* gen_flow, const float* flow, const float* att, float* loss_out,
                      float* partials, size_t numel, dmc_stream_t stream);
/* The gradient of the above for the upstream gradient *grad_loss (a device scalar), one pass: with s = *grad_loss / numel,
 *   grad_gen = l'(d) s (att or 1),   grad_att = gen (l'(d) s) - flow (l'(d) s)   (the reference's gradient reaches att
 * through both products, code/dmcnet/train.py:335); grad_att may be NULL (not wanted) and must be NULL when att is NULL.
 * There is no gradient to flow. */
int dmc_flow_loss_bwd(int kind, const float* gen_flow, const float* flow, const float* att, const float* grad_loss,
                      float* grad_gen, float* grad_att, size_t numel, dmc_stream_t stream);

/* ---- TSN segment consensus + cross entropy ---------------------------------------------------
 * Replaces: output.view(-1, S, C).mean(dim=1); CrossEntropyLoss()(output, target)
 *           code/dmcnet/train.py:239-241   (also the adversarial CE with S = 1,
 *           code/dmcnet_GAN/train.py:274,346)
 * logits [B*S, C] fp32, target [B] int64 ->
 *   consensus [B, C] (the averaged logits, what accuracy() consumes),
 *   loss_out  one float: mean over B of -log softmax(consensus)[target],
 *   grad_logits [B*S, C] = (softmax - onehot) / (B*S), i.e. dloss/dlogits for upstream grad 1
 *   (may be NULL to skip).
 * A label outside [0, C) is never used as an index: the loss and that clip's gradient rows become
 * NaN (torch's CrossEntropyLoss asserts on the device instead).
 */
int dmc_consensus_ce_fwd_bwd(const float* logits, const int64_t* target, float* consensus,
                             float* loss_out, float* grad_logits, int B, int S, int C,
                             dmc_stream_t stream);

/* ---- discriminator block tail ----------------------------------------------------------------
 * Replaces the three modules that follow the Conv2d of discriminator_block /
 * discriminator_block2:  LeakyReLU(0.2) -> Dropout2d(0.25) -> BatchNorm2d(C, eps=0.8)
 *           code/dmcnet_GAN/model.py:254-279
 * x [N,C,H,W] is the conv output.  keep [N,C] holds the Dropout2d keep-mask ALREADY divided by
 * (1-p) (0 or 1/0.75) -- the caller draws it, so CPU and GPU runs can share one.
 * Training-mode BatchNorm: batch statistics (biased variance for normalisation), running stats
 * updated with momentum (unbiased variance), as torch.nn.BatchNorm2d does.
 * use_bn == 0 (first block): y = keep * lrelu(x) only; gamma..running_var ignored.
 * stats: workspace of dmc_disc_tail_stats_bytes(C) bytes; its first 2*C floats receive
 * (mean, invstd) for the backward pass, the rest is reduction scratch.
 */
size_t dmc_disc_tail_stats_bytes(int C);
int dmc_disc_tail_fwd(const float* x, const float* keep, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float* y, float* stats, int N,
                      int C, int H, int W, int use_bn, int training, float eps, float momentum,
                      dmc_stream_t stream);
/* Backward of the above in training mode: given dy -> dx, dgamma, dbeta (overwritten).
 * `stats` is the buffer the forward filled (its scratch part is reused). */
int dmc_disc_tail_bwd(const float* x, const float* keep, const float* gamma, float* stats,
                      const float* dy, float* dx, float* dgamma, float* dbeta, int N, int C, int H,
                      int W, int use_bn, dmc_stream_t stream);

/* ---- classifier BatchNorm [+ residual] [+ ReLU], NHWC -------------------------------------------
 * Replaces, inside the torchvision ResNet the reference builds at code/dmcnet/model.py:305 and
 * runs at :352 (GAN: code/dmcnet_GAN/model.py:560): nn.BatchNorm2d followed by the residual
 * addition and the in-place nn.ReLU of the stem and of every BasicBlock / Bottleneck:
 *     y = act( BN(x) [+ residual] ),  act = ReLU if relu != 0 else identity.
 * x, residual, y, dy, dx, dresidual: [M][C] row-major, M = N*H*W (the memory of a channels_last
 * tensor).  Training mode uses batch statistics and updates running_mean / running_var exactly
 * as nn.BatchNorm2d does.  dmc_bn_act_supported() tells whether (M, C) is handled
 * (C % 4 == 0, C/4 <= 256, 256 % (C/4) == 0); callers use the stock op otherwise.
 * stats: dmc_bn_act_stats_bytes(C) bytes (2*C floats): the forward leaves (mean, invstd) there for
 * the backward -- the only thing a caller keeps between the two.  scratch: dmc_bn_act_scratch_bytes(C)
 * bytes of reduction workspace, transient (dead when the call's kernels have run; NULL allowed for
 * an eval-mode forward, which reduces nothing).  relu_mask (nullable, M*C/4 bytes): the forward stores the four ReLU
 * sign bits of every float4; a backward given the same buffer reads them instead of re-reading the
 * residual (`residual` may then be NULL).  Without it the backward recomputes the signs from x
 * (and residual).
 */
int dmc_bn_act_supported(int M, int C);
size_t dmc_bn_act_stats_bytes(int C);
size_t dmc_bn_act_scratch_bytes(int C);
int dmc_bn_act_fwd(const float* x, const float* residual, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float* y, float* stats, void* scratch,
                   unsigned char* relu_mask, int M, int C, int relu, int training, float eps,
                   float momentum, dmc_stream_t stream);
int dmc_bn_act_bwd(const float* x, const float* residual, const float* gamma, const float* beta,
                   const float* stats, void* scratch, const float* dy, float* dx, float* dresidual,
                   float* dgamma, float* dbeta, const unsigned char* relu_mask, int M, int C, int relu,
                   dmc_stream_t stream);

/* Pieces of the same kernels for a producer that has already reduced the statistics (the
 * discriminator blocks, whose convolution epilogue does it): the apply pass alone; the backward
 * of  y = BN(z), z = keep[n][c] * LeakyReLU_slope(pre)  (code/dmcnet_GAN/model.py:254-279: Conv ->
 * LeakyReLU(0.2) -> Dropout2d -> BatchNorm2d) down to d(pre) = the gradient of the convolution's
 * output, gamma == NULL meaning "no BatchNorm" (first block); and a per-channel row sum (the
 * convolution's bias gradient).  scratch: dmc_bn_act_scratch_bytes(C).
 */
int dmc_bn_apply_nhwc(const float* x, const float* gamma, const float* beta, const float* stats, float* y,
                      int M, int C, dmc_stream_t stream);
/* the same apply pass with the residual add / ReLU / ReLU sign mask of dmc_bn_act_fwd: the second half of
 * torchvision's `relu(bn(conv(x)) [+ identity])` when the convolution's epilogue reduced the statistics */
int dmc_bn_apply_act_nhwc(const float* x, const float* residual, const float* gamma, const float* beta,
                          const float* stats, float* y, unsigned char* relu_mask, int M, int C, int relu,
                          dmc_stream_t stream);
int dmc_bn_bwd_act_nhwc(const float* z, const float* gamma, const float* beta, const float* stats, void* scratch,
                        const float* dy, float* dpre, float* dgamma, float* dbeta, const float* keep, int hw,
                        float slope, int M, int C, dmc_stream_t stream);
int dmc_channel_sum_nhwc(const float* g, void* scratch, float* out, int M, int C, dmc_stream_t stream);

/* ---- GPU-side input preparation -----------------------------------------------------------------
 * Replaces the tensor side of CoviarDataSet.__getitem__, code/dmcnet/dataset.py:215-263 (channel
 * split, flow block_reduce(mean)+repeat when flow_ds_factor != 0, /255, (x-0.5)/std) and the
 * horizontal flip of code/dmcnet/transforms.py:47-58, bit-identically.
 * frames_u8 [N,H,W,7] uint8 HWC = [flow_x flow_y mv_x mv_y r g b] (already cropped/resized);
 * flip [N] bytes or NULL (non-zero: mirror the frame, x components of flow and MV -> 256 - v);
 * outputs input_flow [N,2,H,W], input_mv [N,2,H,W], input_residual [N,3,H,W] fp32.
 * std4_host: HOST array {mean(std), std_r, std_g, std_b} as fp32 (what torch computes from
 * [0.229, 0.224, 0.225]).  workspace: dmc_prepare_inputs_workspace_bytes() bytes.
 */
size_t dmc_prepare_inputs_workspace_bytes(int N, int H, int W, int flow_ds_factor);
int dmc_prepare_inputs(const unsigned char* frames_u8, const unsigned char* flip, float* out_flow,
                       float* out_mv, float* out_res, float* workspace, int N, int H, int W,
                       int flow_ds_factor, const float* std4_host, dmc_stream_t stream);

/* Crop + bilinear resize + flip + blockify + normalise on the device: the whole of
 * GroupMultiScaleCrop / GroupCenterCrop / GroupScale (code/dmcnet/transforms.py:36-46,62-78,
 * 117-139), GroupRandomHorizontalFlip (:47-58) and dataset.py:215-263 except the random draws,
 * which stay on the host (crop box, flip bit).
 * frames_u8 [N,H0,W0,7] uint8 as decoded, allocated with >= 16 spare bytes behind the last frame
 * (the 4-pixel path reads whole aligned dwords); boxes [N,8] int32 DEVICE array
 * (y0, x0, h, w, rh, rw, cy, cx): the box (y0, x0, h, w) of each frame is resized to rh x rw with the
 * half-pixel-centre bilinear rule (bit-identical to this package's transforms.resize_bilinear;
 * rh x rw == h x w copies) and the OH x OW window at (cy, cx) of that image is produced
 * (crop -> resize: cy = cx = 0, rh x rw = OH x OW; scale -> centre crop: the window); NULL = the
 * whole frame, which must then measure OH x OW; flip as above (applied last); outputs
 * [N,2,OH,OW], [N,2,OH,OW], [N,3,OH,OW] fp32.  workspace: dmc_prepare_crop_workspace_bytes().
 */
size_t dmc_prepare_crop_workspace_bytes(int N, int OH, int OW, int flow_ds_factor);
int dmc_prepare_inputs_crop(const unsigned char* frames_u8, const int* boxes, const unsigned char* flip,
                            float* out_flow, float* out_mv, float* out_res, float* workspace, int N,
                            int H0, int W0, int OH, int OW, int flow_ds_factor, const float* std4_host,
                            dmc_stream_t stream);

/* Views and interpolated flow upsampling: dmc_prepare_inputs_crop with two additions.
 * src_index [N_out] int32 DEVICE array or NULL: the source frame (0 .. N_src-1) output n reads, so that several
 * outputs -- the ten crops of GroupOverSample, code/dmcnet/transforms.py:77-114 -- are plans over ONE uploaded
 * frame; boxes [N_out,8] and flip [N_out] stay per OUTPUT.  NULL = identity, N_out must equal N_src.
 * upsample_interp != 0 (needs flow_ds_factor > 0 and at least two blocks on each axis; scipy refuses a single
 * block too): the block means are brought back to OH x OW by the reference's linear interpolation
 * (code/dmcnet/dataset.py:236-246: interp1d between linspace(0, 1, n_blocks) and linspace(0, 1, n_blocks * factor),
 * along H and then along W, fp64, first OH x OW kept) instead of by repetition, bit-identically to
 * CoviarDataSet(..., upsample_interp=True).__getitem__.  upsample_interp == 0 computes what
 * dmc_prepare_inputs_crop computes.  workspace: dmc_prepare_views_workspace_bytes() bytes.
 * Everything else (frames_u8 with its 16 spare bytes, outputs, std4_host, asynchronous on the stream, no
 * allocation, bad arguments refused before a launch) as dmc_prepare_inputs_crop.
 *
 * dmc_prepare_interp_taps runs on the HOST only (no GPU needed): for one axis of n_blocks >= 2 blocks it fills
 * lo / dx / t [n_blocks * factor] with the interval index, its width x[lo+1] - x[lo] and the offset xn - x[lo]
 * of every upsampled position, from the same function the kernel uses; the interpolated value is
 * ((y[lo+1] - y[lo]) / dx) * t + y[lo] in fp64 with every operation rounded on its own.  Positions that
 * coincide with a knot use the interval to their LEFT (scipy's searchsorted side).
 */
size_t dmc_prepare_views_workspace_bytes(int N_out, int OH, int OW, int flow_ds_factor, int upsample_interp);
int dmc_prepare_inputs_views(const unsigned char* frames_u8, const int* src_index, const int* boxes,
                             const unsigned char* flip, float* out_flow, float* out_mv, float* out_res,
                             void* workspace, int N_src, int N_out, int H0, int W0, int OH, int OW,
                             int flow_ds_factor, int upsample_interp, const float* std4_host, dmc_stream_t stream);
int dmc_prepare_interp_taps(int n_blocks, int factor, int* lo, double* dx, double* t);

/* I3D clip preparation (modality 'flow+mp4'): the tensor side of the reference's I3D loader on the device --
 * code/dmcnet_I3D/data/iterator_factory.py:49-56,72-77 (the chains), image_transforms.py:14-35,47-59,138-200 (Compose,
 * Normalize, CenterCrop, RandomCrop, RandomHorizontalFlip), video_transforms.py:23-70 (ToTensor) and
 * video_iterator.py:150-178,428-433 (how a clip is packed) -- bit for bit.  Only the random draws stay on the host.
 * clips_u8 [B,H0,W0,T*7] uint8 as decoded, frame t in channels 7t .. 7t+6 = [flow_x flow_y mv_x mv_y res0 res1 res2],
 * with >= 16 spare bytes behind the last clip (the records are read as aligned dwords); plans [B,3] int32 DEVICE array
 * (y1, x1, flip): the OH x OW window at (y1, x1), mirrored along W when flip != 0; out [B,7,T,OH,OW] fp32, contiguous.
 * The reference's quirks, kept as written:
 *   - flip: flow_x and mv_x of every frame (channels 0::7 and 2::7) become (256 - v) cast to uint8, so 0 stays 0;
 *   - flow_ds_factor f >= 2: the two flow channels of every frame are replaced by their f x f block means (after the flip),
 *     ragged edge blocks zero-padded and still divided by f^2 (skimage.measure.block_reduce), the mean TRUNCATED to an
 *     integer (it is assigned into the uint8 array): floor(sum / f^2).  video_transforms.py:46 (`is not 0 or 1`) is always
 *     true, so f = 1 is the identity; 0 and 1 both mean "no blockify" here;
 *   - then float / 255 (fp32, true division);
 *   - Normalize zips over the FIRST dimension and stops at len(mean): only channels 0 .. n_norm-1 (flow_x, flow_y and
 *     mv_x for the recipe's three means) get (v - mean[c]) / std[c]; the others stay in [0, 1].  Every operation is rounded
 *     to fp32 on its own, no reciprocal.
 * mean_host / std_host: HOST fp32 arrays of n_norm entries, 0 <= n_norm <= 7 (may be NULL when n_norm == 0).
 * workspace: dmc_prepare_clip_workspace_bytes() bytes -- 0, the block sums live in LDS; NULL is accepted.
 * Asynchronous on the stream, no allocation, no synchronisation; refused before any launch: null pointers, non-positive
 * sizes, OH > H0, OW > W0, n_norm outside 0 .. 7, a negative factor, pointers that are not 4-byte aligned, and a factor
 * whose single block column (lcm(4, f) pixels, or the row) does not fit the LDS.  Any T >= 1 runs: frames are chunked.
 * Plans are not range-checked on the device (ops.check_clip_plans checks host plans).
 */
size_t dmc_prepare_clip_workspace_bytes(int B, int T, int OH, int OW, int flow_ds_factor);
int dmc_prepare_clip(const unsigned char* clips_u8, const int* plans, float* out, void* workspace,
                     int B, int T, int H0, int W0, int OH, int OW, int flow_ds_factor,
                     int n_norm, const float* mean_host, const float* std_host, dmc_stream_t stream);

/* ---- classifier stem: BatchNorm + ReLU + MaxPool2d(3, stride 2, padding 1) fused -----------------
 * Replaces `self.maxpool(self.relu(self.bn1(x)))` of the torchvision ResNet the reference builds at
 * code/dmcnet/model.py:305 (run at :352) and its autograd.  x [N,H,W,C] fp32 NHWC (conv1 output),
 * y_pool / d_pool [N,PH,PW,C] with PH = (H-1)/2+1, PW = (W-1)/2+1; the rectified full-resolution
 * tensor is never materialised.  Arg-max ties follow PyTorch (first element in row-major window
 * order).  stats: dmc_bn_act_stats_bytes(C) bytes, written by fwd (mean, invstd) and read by bwd;
 * scratch: dmc_bn_act_scratch_bytes(C) bytes, transient (NULL allowed when training == 0).
 * training = 0 normalises with the running statistics (forward only).
 * codes: dmc_bn_relu_pool_codes_bytes() bytes of scratch (the windows' arg-max positions, written by the
 * backward's first pass and read by its second), or NULL to recompute them in the second pass.
 */
int dmc_bn_relu_pool_supported(int N, int H, int W, int C);
int dmc_bn_relu_pool_fwd(const float* x, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float* y_pool, float* stats, void* scratch, int N, int H,
                         int W, int C, int training, float eps, float momentum, dmc_stream_t stream);
size_t dmc_bn_relu_pool_codes_bytes(int N, int H, int W, int C);
int dmc_bn_relu_pool_bwd(const float* x, const float* gamma, const float* beta, const float* stats,
                         void* scratch, const float* d_pool, float* dx, float* dgamma, float* dbeta,
                         void* codes, int N, int H, int W, int C, dmc_stream_t stream);

/* ---- NHWC convolutions on the fp32 matrix cores ---------------------------------------------------
 * Replace nn.Conv2d (3x3 padding 1, or 1x1 padding 0; stride 1 or 2; Cin, Cout multiples of 16) and
 * its autograd wherever the hot path runs them:
 *   - the PatchGAN discriminator blocks, code/dmcnet_GAN/model.py:254-279 (Conv2d(in, out, 3, stride,
 *     1) with bias, followed by LeakyReLU(0.2), Dropout2d(0.25), BatchNorm2d(out, eps=0.8)) as chained
 *     in Discriminator..Discriminator5, :282-438;
 *   - the torchvision ResNet the reference builds at code/dmcnet/model.py:305 and runs at :352
 *     (BasicBlock 3x3 convolutions and the 1x1 stride-2 shortcut convolutions, bias-free).
 * Layouts: activations NHWC fp32 ([N][H][W][C], the memory of a channels_last tensor), weights
 * OHWI ([Cout][KH][KW][Cin], the memory of a channels_last weight); OH = (H + 2 pad - KH) / stride + 1.
 * dmc_conv_nhwc_supported() says whether a shape is handled (callers use the stock op otherwise).
 *
 * fwd: y = conv(x, w) [+ bias] [LeakyReLU(0.2) if act == 1] [* keep[n][co]] -- the Dropout2d keep mask
 * [N][Cout], already divided by 1 - p -- and, if stat_partials != NULL, per-channel (sum, sum of squares)
 * of y per workgroup row, [stat_blocks = dmc_conv_nhwc_stat_blocks()][Cout][2] doubles (the launch FAILS if its grid has
 * another number of rows -- e.g. the tile-configuration option changed between the two calls -- instead of overrunning), which
 * dmc_conv_nhwc_stats_final() turns into the (mean, invstd) pair [2*C] and the running-statistics
 * update of the nn.BatchNorm2d that follows (count = N*OH*OW).
 * wpack: workspace of dmc_conv_nhwc_wt_bytes() bytes for the weights as the kernel wants them (needed when the
 * option "conv_arith" is 1; may be NULL otherwise).
 * dgrad: dx = conv_transpose(dy, w); wt = workspace of dmc_conv_nhwc_wt_bytes().
 * bf16x3 shapes (dmc_conv_nhwc_presplit_supported): dmc_conv_nhwc_split() fills the forward's and the data gradient's workspaces
 * in one launch, and fwd / dgrad called with w == NULL use theirs as it is (one split launch per layer and step instead of two).
 * Arithmetic (option "conv_arith"): 0 = v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulate); 1 = "bf16x3" for
 * Cin % 32 == 0, Cout % 64 == 0: every fp32 operand is the exact sum of three bf16 slices, each product is formed
 * from six slice products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (the omitted three are below 2^-23 of
 * |a||b|) -- the error against an fp64 evaluation is that of the fp32 instruction or below
 * (tools/conv_x3_check.py, tests), at 2.67x its rate.
 * wgrad: dw (OHWI) = sum over pixels, deterministic (fixed-order split-K reduction, no atomics);
 * workspace of dmc_conv_nhwc_wgrad_bytes().
 */
int dmc_conv_nhwc_supported(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int dmc_conv_nhwc_stat_blocks(int N, int H, int W, int Cin, int Cout, int KH, int stride, int pad);
int dmc_conv_nhwc_fwd(const float* x, const float* w, void* wpack, const float* bias, const float* keep, float* y,
                      double* stat_partials, int stat_blocks, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                      int pad, int act, dmc_stream_t stream);
int dmc_conv_nhwc_stats_final(const double* partials, int nblk, int C, long count, float* stats,
                              float* running_mean, float* running_var, float eps, float momentum,
                              dmc_stream_t stream);
size_t dmc_conv_nhwc_wt_bytes(int Cin, int Cout, int KH, int KW);
int dmc_conv_nhwc_presplit_supported(int Cin, int Cout);
int dmc_conv_nhwc_split(const float* w, void* wpack_f, void* wpack_t, int Cin, int Cout, int KH, int KW, dmc_stream_t stream);
int dmc_conv_nhwc_dgrad(const float* dy, const float* w, float* wt, float* dx, int N, int H, int W, int Cin,
                        int Cout, int KH, int KW, int stride, int pad, dmc_stream_t stream);
/* dx = data gradient + addend (the residual branch's gradient of a torchvision BasicBlock, resnet.py BasicBlock.forward:
 * `out += identity`), added in the convolution's epilogue; stride 1 and dmc_conv_nhwc_presplit_supported shapes only. */
int dmc_conv_nhwc_dgrad_add(const float* dy, const float* w, float* wt, const float* addend, float* dx, int N, int H, int W,
                            int Cin, int Cout, int KH, int KW, int stride, int pad, dmc_stream_t stream);
size_t dmc_conv_nhwc_wgrad_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int dmc_conv_nhwc_wgrad(const float* x, const float* dy, float* dw, float* workspace, int N, int H, int W,
                        int Cin, int Cout, int KH, int KW, int stride, int pad, dmc_stream_t stream);

/* ---- 3x3 / stride-1 convolutions on PRE-SPLIT bf16x3 operands (conv_x3s.hip) ---------------------------------
 * Replaces: the stride-1 3x3 convolutions of the ResNet-18 classifier (torchvision BasicBlock behind
 *           code/dmcnet/model.py:305, run at :352) and their autograd, in the same bf16x3 arithmetic as
 *           dmc_conv_nhwc_* (fp32 products from three bf16 slices per operand), with the split moved to the PRODUCER of
 *           each activation: every operand arrives as a "slice tensor"
 *               bf16 [3 slices][C / 16][M pixels][16 channels]        (dmc_x3s_slices_bytes(M, C) = 6 M C bytes)
 *           whose three slices sum to the fp32 value exactly.  dmc_x3s_split / dmc_x3s_merge convert from / to the
 *           fp32 [M][C] (channels_last) tensor; the BatchNorm kernels below write slice tensors directly.
 * Weights: dmc_x3s_pack_weights() packs w [Cout][3][3][Cin] (channels_last memory of the PyTorch weight) once per step
 *           into the forward's and / or the data gradient's image (dmc_x3s_wpack_bytes() each; either may be NULL).
 * fwd:     y [M][Cout] fp32 = conv3x3(x, w), padding 1, stride 1; stat_partials (nullable) receives the per-channel
 *           (sum, sum of squares) of y per workgroup row, [stat_blocks = dmc_x3s_conv_stat_blocks()][Cout][2] doubles, for
 *           dmc_conv_nhwc_stats_final(); a launch whose grid has another number of rows is refused (no overrun).
 * dgrad:   dx [M][Cin] fp32 = conv_transpose(dy, w) [+ addend, nullable: the residual branch's gradient].
 * Cin % 64 == 0, Cout % 64 == 0; dmc_x3s_conv_supported() says whether a shape is handled.  Deterministic. */
size_t dmc_x3s_slices_bytes(long M, int C);
int dmc_x3s_split(const float* x, void* xs, long M, int C, dmc_stream_t stream);
int dmc_x3s_merge(const void* xs, float* x, long M, int C, dmc_stream_t stream);
size_t dmc_x3s_wpack_bytes(int Cin, int Cout);
int dmc_x3s_pack_weights(const float* w, void* wpack_f, void* wpack_t, int Cin, int Cout, dmc_stream_t stream);
int dmc_x3s_conv_supported(int N, int H, int W, int Cin, int Cout);
int dmc_x3s_conv_stat_blocks(int N, int H, int W, int Cout);
int dmc_x3s_conv_fwd(const void* xs, const void* wpack_f, float* y, double* stat_partials, int stat_blocks, int N, int H, int W,
                     int Cin, int Cout, dmc_stream_t stream);
int dmc_x3s_conv_dgrad(const void* dys, const void* wpack_t, const float* addend, float* dx, int N, int H, int W, int Cin,
                       int Cout, dmc_stream_t stream);
/* The forward convolution with the eval-mode BatchNorm [+ shortcut] [+ ReLU] in its epilogue, ONE launch:
 * Replaces: the stride-1 3x3 convolution + BatchNorm2d (running statistics) [+ `out += identity`] [+ ReLU] of torchvision's
 *           BasicBlock (behind code/dmcnet/model.py:305,352) as the evaluator runs them under model.eval() + no_grad
 *           (code/dmcnet/test.py:139-198, validate() of code/dmcnet/train.py) -- what dmc_x3s_conv_fwd followed by
 *           dmc_bn_apply_act_x3s / dmc_bn_apply_act_x3q computes, bit for bit, without the fp32 convolution result in memory.
 * stats = mean[Cout], 1 / sqrt(var + eps)[Cout] (as dmc_bn_apply_act_x3s takes them); residual: fp32 [M][Cout] or NULL.
 * Outputs (at least one): y fp32 [M][Cout] (nullable); ys (nullable) the result's slice tensor, [3][Cout/16][M][16] when
 * s2d == 0, the space-to-depth tensor of dmc_bn_apply_act_x3q over the [N][H][W] grid (H, W even) when s2d != 0.
 * Shapes of dmc_x3s_conv_supported(); obeys option conv_cfg as dmc_x3s_conv_fwd does; writes no statistics partials.
 * DMC_E_INVALID before any launch: a null input, no output, s2d without ys or with odd H / W, Cin or Cout % 64 != 0. */
int dmc_x3s_conv_bn_eval(const void* xs, const void* wpack_f, const float* stats, const float* gamma, const float* beta,
                         const float* residual, float* y, void* ys, int s2d, int relu, int N, int H, int W, int Cin, int Cout,
                         dmc_stream_t stream);
/* wgrad: dw [Cout][3][3][Cin] fp32 (channels_last memory of the PyTorch gradient) from the slice tensors of x and dy;
 * workspace of dmc_x3s_conv_wgrad_bytes() (per-workgroup-row partials, summed in fixed order).  W in {56, 28, 14, 7}. */
int dmc_x3s_conv_wgrad_supported(int N, int H, int W, int Cin, int Cout);
size_t dmc_x3s_conv_wgrad_bytes(int N, int H, int W, int Cin, int Cout);
int dmc_x3s_conv_wgrad(const void* xs, const void* dys, float* dw, float* workspace, int N, int H, int W, int Cin, int Cout,
                       dmc_stream_t stream);
/* Stride-2 3x3 data gradient on pre-split operands in ONE launch (four input-parity classes, nine (tap, class) pairs):
 * dys = slice tensor of dy [N][OH][OW][Cout]; dx [N][2 OH][2 OW][Cin] fp32; weights from dmc_x3s_pack_weights_s2
 * (dmc_x3s_wpack_bytes()).  Replaces the stride-2 convolutions' backward of torchvision's BasicBlock (layerN.0.conv1). */
int dmc_x3s_conv_dgrad_s2_supported(int N, int OH, int OW, int Cin, int Cout);
int dmc_x3s_pack_weights_s2(const float* w, void* wpack_t2, int Cin, int Cout, dmc_stream_t stream);
int dmc_x3s_conv_dgrad_s2(const void* dys, const void* wpack_t2, float* dx, int N, int OH, int OW, int Cin, int Cout,
                          dmc_stream_t stream);


/* Producers of slice tensors (bn_act.hip): the BatchNorm kernels above with the result written as fp32 (nullable) and / or
 * as a bf16x3 slice tensor (nullable), C % 16 == 0 -- the forward's activation for the next convolution
 * (dmc_bn_apply_act_nhwc / dmc_bn_relu_pool_fwd semantics), the backward's convolution-output gradient (dmc_bn_act_bwd
 * semantics) for that convolution's dmc_x3s_conv_dgrad / dmc_x3s_conv_wgrad. */
int dmc_bn_apply_act_x3s(const float* x, const float* residual, const float* gamma, const float* beta, const float* stats,
                         float* y, void* ys, unsigned char* relu_mask, int M, int C, int relu, dmc_stream_t stream);
int dmc_bn_act_bwd_x3s(const float* x, const float* residual, const float* gamma, const float* beta, const float* stats,
                       void* scratch, const float* dy, float* dx, void* dxs, float* dresidual, float* dgamma, float* dbeta,
                       const unsigned char* relu_mask, int M, int C, int relu, dmc_stream_t stream);
int dmc_bn_relu_pool_fwd_x3s(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                             float* y_pool, void* ys, float* stats, void* scratch, int N, int H, int W, int C, int training,
                             float eps, float momentum, dmc_stream_t stream);
/* The stem tail with an arg-max record (replaces torchvision's bn1 / relu / maxpool behind
 * /root/reference/code/dmcnet/model.py:305, as dmc_bn_relu_pool_fwd does): dmc_bn_relu_pool_fwd_arg =
 * dmc_bn_relu_pool_fwd_x3s that also writes, when `codes` / `xmax` are given (both or neither), each window's arg-max
 * position per channel (codes: dmc_bn_relu_pool_codes_bytes) and the raw input there (xmax: fp32 [N][PH][PW][C]);
 * dmc_bn_relu_pool_bwd_arg = dmc_bn_relu_pool_bwd from that record: its BatchNorm-backward sums stream over the
 * pooled-size (d_pool, xmax) pair instead of gathering over the 4x larger input.  Same dx / dgamma / dbeta semantics.
 * stat_split: 0 = reduce the batch statistics of x here; > 0 = `scratch` already holds that many partial sums per channel
 * (written by x's producer, dmc_stem_fwd_x3_stats). */
int dmc_bn_relu_pool_fwd_arg(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                             float* y_pool, void* ys, void* codes, float* xmax, float* stats, void* scratch, int stat_split,
                             int N, int H, int W, int C, int training, float eps, float momentum, dmc_stream_t stream);
int dmc_bn_relu_pool_bwd_arg(const float* x, const float* gamma, const float* beta, const float* stats, void* scratch,
                             const float* d_pool, const void* codes, const float* xmax, float* dx, float* dgamma, float* dbeta,
                             int N, int H, int W, int C, dmc_stream_t stream);
/* ---- the stride-2 residual blocks on PRE-SPLIT operands (conv_x3q.hip) ------------------------------------------------
 * Replaces: torchvision BasicBlock `conv1` (3x3, stride 2, padding 1) together with `downsample[0]` (1x1, stride 2) of
 *           layer2.0 / layer3.0 / layer4.0 -- the two convolutions that read the block input, built at
 *           code/dmcnet/model.py:305 and run at :352 -- and their autograd, in the bf16x3 arithmetic of dmc_x3s_*, ONE
 *           launch per direction for the pair (the shortcut reads x[2a][2b] = the centre tap's operand).
 * Input:    the block input as a SPACE-TO-DEPTH slice tensor ("s2d"; H, W even, OH = H / 2, OW = W / 2, Mq = N OH OW):
 *               bf16 [3 slices][4 parity classes 2 py + px][Cin / 16][Mq pixels][16 channels]       (6 N H W Cin bytes)
 *           class (py, px) holds the pixels (2a + py, 2b + px); written by the input's producer (dmc_bn_apply_act_x3q) or
 *           by dmc_x3q_split; dmc_x3q_merge is the exact inverse.
 * Weights:  dmc_x3q_pack_weights(w3 [Cout][3][3][Cin], w1 [Cout][Cin] -- channels_last memory of the two PyTorch weights)
 *           fills the forward's and / or the data gradient's image (dmc_x3q_wpack_bytes() each; either may be NULL).
 * fwd:      y3 [Mq][Cout] = conv3x3 stride 2 (x, w3), y1 [Mq][Cout] = conv1x1 stride 2 (x, w1), fp32; stat_partials3 / 1
 *           (nullable) receive the per-channel (sum, sum of squares) per workgroup row, [stat_blocks =
 *           dmc_x3q_stat_blocks()][Cout][2] doubles each, for dmc_conv_nhwc_stats_final().
 * dgrad:    dx [N][H][W][Cin] fp32 = conv_transpose(dy3, w3) + conv_transpose(dy1, w1) from the ORDINARY slice tensors of
 *           the two output gradients ([3][Cout / 16][Mq][16], e.g. from dmc_bn_act_bwd_x3s); every element of dx is written.
 * wgrad:    dw3 [Cout][3][3][Cin], dw1 [Cout][Cin] from the s2d input and the two output-gradient slice tensors;
 *           workspace of dmc_x3q_conv_wgrad_bytes(); deterministic (fixed-order reduction of per-workgroup partials).
 * Cin, Cout multiples of 64; dmc_x3q_supported() says whether a shape is handled (OW in {28, 14, 7} for the weight
 * gradient, as the classifier has them). */
size_t dmc_x3q_wpack_bytes(int Cin, int Cout);
int dmc_x3q_supported(int N, int OH, int OW, int Cin, int Cout);
int dmc_x3q_stat_blocks(int N, int OH, int OW, int Cout);
int dmc_x3q_split(const float* x, void* xq, int N, int H, int W, int C, dmc_stream_t stream);
int dmc_x3q_merge(const void* xq, float* x, int N, int H, int W, int C, dmc_stream_t stream);
int dmc_x3q_pack_weights(const float* w3, const float* w1, void* wpack_f, void* wpack_t, int Cin, int Cout, dmc_stream_t stream);
int dmc_x3q_conv_fwd(const void* xq, const void* wpack_f, float* y3, float* y1, double* stat_partials3, double* stat_partials1,
                     int stat_blocks, int N, int OH, int OW, int Cin, int Cout, dmc_stream_t stream);
int dmc_x3q_conv_dgrad(const void* dys3, const void* dys1, const void* wpack_t, float* dx, int N, int OH, int OW, int Cin, int Cout,
                       dmc_stream_t stream);
/* The forward pair with both eval-mode BatchNorms in its epilogue, ONE launch:
 * Replaces: `conv1` + `bn1` + ReLU and `downsample` (1x1 convolution + BatchNorm2d) of torchvision's stride-2 BasicBlock
 *           (layer2.0 / layer3.0 / layer4.0 behind code/dmcnet/model.py:305,352) with running statistics, as the evaluator
 *           runs them (code/dmcnet/test.py:139-198, validate() of code/dmcnet/train.py) -- what dmc_x3q_conv_fwd followed by
 *           dmc_bn_apply_act_x3s (main branch) and dmc_bn_apply_act_nhwc (shortcut branch) computes, bit for bit.
 * stats3 / stats1 = mean[Cout], 1 / sqrt(var + eps)[Cout] of bn1 / the downsample BatchNorm.
 * Main branch relu(bn3(conv3x3/s2)): y3 fp32 [Mq][Cout] (nullable) and / or ys3 its ordinary slice tensor
 * [3][Cout/16][Mq][16] (nullable), at least one; shortcut branch bn1(conv1x1/s2): y1 fp32 [Mq][Cout], no ReLU.
 * Shapes of dmc_x3q_supported(); obeys option conv_cfg as dmc_x3q_conv_fwd does; writes no statistics partials.
 * DMC_E_INVALID before any launch: a null input or y1, neither y3 nor ys3, Cin or Cout % 64 != 0. */
int dmc_x3q_conv_bn_eval(const void* xq, const void* wpack_f, const float* stats3, const float* gamma3, const float* beta3,
                         const float* stats1, const float* gamma1, const float* beta1, float* y3, void* ys3, float* y1, int N, int OH,
                         int OW, int Cin, int Cout, dmc_stream_t stream);
/* dmc_bn_apply_act_x3s (BatchNorm apply [+ residual] [+ ReLU] with given statistics) whose slice output yq is the s2d
 * tensor over the [N][H][W] grid; y (fp32 NHWC, nullable) as usual. */
int dmc_bn_apply_act_x3q(const float* x, const float* residual, const float* gamma, const float* beta, const float* stats,
                         float* y, void* yq, unsigned char* relu_mask, int N, int H, int W, int C, int relu, dmc_stream_t stream);
int dmc_x3q_conv_wgrad_supported(int N, int OH, int OW, int Cin, int Cout);
size_t dmc_x3q_conv_wgrad_bytes(int N, int OH, int OW, int Cin, int Cout);
int dmc_x3q_conv_wgrad(const void* xq, const void* dys3, const void* dys1, float* dw3, float* dw1, float* workspace, int N, int OH,
                       int OW, int Cin, int Cout, dmc_stream_t stream);

/* BatchNorm-backward sums from the data gradient's epilogue: dmc_x3s_conv_dgrad_bnb = dmc_x3s_conv_dgrad that also
 * reduces, for the unit whose output gradient it writes (dx), dbeta = sum(d) and dgamma = sum(d * xhat) (d = dx, zeroed
 * where that unit's ReLU was off; partials: dmc_x3s_conv_stat_blocks(N, H, W, Cin) x Cin x 2 doubles);
 * dmc_bn_act_bwd_x3s_apply = the second half of dmc_bn_act_bwd_x3s with those sums as inputs (no reduction pass). */
int dmc_x3s_conv_dgrad_bnb(const void* dys, const void* wpack_t, const float* addend, float* dx, const float* bn_y,
                           const float* bn_stats, const float* bn_gamma, const float* bn_beta, const unsigned char* bn_relu_mask,
                           int bn_relu, double* partials, int stat_blocks, float* dgamma, float* dbeta, int N, int H, int W, int Cin,
                           int Cout, dmc_stream_t stream);
int dmc_bn_act_bwd_x3s_apply(const float* x, const float* residual, const float* gamma, const float* beta, const float* stats,
                             const float* dy, float* dx, void* dxs, float* dresidual, const float* dgamma, const float* dbeta,
                             const unsigned char* relu_mask, int M, int C, int relu, dmc_stream_t stream);




/* ---- first discriminator block: Conv2d(2, Cout, 3, stride 2, padding 1) on the NCHW cue ------------
 * Replaces the convolution (+ LeakyReLU(0.2) + Dropout2d keep mask) of `discriminator_block(ch_in, 16,
 * bn=False)`, code/dmcnet_GAN/model.py:254-265 as used at :287,:308,:334,:371,:400, and its autograd.
 * x [M,2,H,W] NCHW fp32 (the generated / TV-L1 flow), w [Cout,2,3,3] (PyTorch's layout), Cout 16 (8 for
 * Discriminator4); z, g: [M,OH,OW,Cout] NHWC, OH = (H-1)/2+1.  keep: [M,Cout] or NULL; act != 0
 * applies LeakyReLU(0.2).  wgrad writes dw [Cout,2,3,3] and db [Cout] (NULL to skip) deterministically;
 * workspace: dmc_disc_first_wgrad_bytes(Cout).
 */
int dmc_disc_first_supported(int Cout);
int dmc_disc_first_fwd(const float* x, const float* w, const float* bias, const float* keep, float* z, int M,
                       int H, int W, int Cout, int act, dmc_stream_t stream);
int dmc_disc_first_dgrad(const float* g, const float* w, float* dx, int M, int H, int W, int Cout,
                         dmc_stream_t stream);
size_t dmc_disc_first_wgrad_bytes(int Cout);
int dmc_disc_first_wgrad(const float* x, const float* g, float* dw, float* db, void* workspace, int M, int H,
                         int W, int Cout, dmc_stream_t stream);

/* ---- classifier stem: weight gradient of conv1 (2 -> 64 channels, 7x7, stride 2, pad 3) ----------
 * Replaces what autograd computes for the conv1 the reference installs for the 2-channel flow
 * input, code/dmcnet/model.py:285-294 (nn.Conv2d(2, 64, 7, stride=2, padding=3, bias=False)),
 * inside loss.backward(), code/dmcnet/train.py:258.  (The forward convolution and, when the input
 * needs a gradient, the data gradient stay on MIOpen.)
 * x [N,2,H,W] fp32 NCHW; dy [N,OH,OW,64] fp32 NHWC (channels_last storage of the [N,64,OH,OW]
 * gradient), OH = (H+1)/2, OW = (W+1)/2; dw [64,2,7,7] fp32 contiguous.  Requires W % 4 == 0
 * (dmc_stem_wgrad_supported).  partials: dmc_stem_wgrad_partials_bytes(N,H,W) bytes.
 * Deterministic (fixed summation order).
 */
int dmc_stem_wgrad_supported(int H, int W);
size_t dmc_stem_wgrad_partials_bytes(int N, int H, int W);
int dmc_stem_wgrad(const float* x, const float* dy, float* dw, float* partials, int N, int H, int W,
                   dmc_stream_t stream);
/* forward of the same convolution (replaces F.conv2d(x, conv1.weight, None, 2, 3) behind base_model(input),
 * code/dmcnet/model.py:352): y [N,OH,OW,64] NHWC fp32; w [64,2,7,7] by element strides (contiguous: 98, 49, 7, 1;
 * channels_last: 98, 1, 14, 2).  Exact fp32 (v_mfma_f32_32x32x2_f32), any H, W. */
int dmc_stem_fwd(const float* x, const float* w, long ws_co, long ws_ci, long ws_ky, long ws_kx, float* y, int N, int H, int W,
                 dmc_stream_t stream);
/* the same forward in bf16x3 arithmetic (fp32 operands as three bf16 slices, six bf16 MFMAs per product block, fp32
 * accumulate: fp32-level error); workspace: dmc_stem_fwd_x3_workspace_bytes(N, H, W) (padded slice volumes + split weights) */
size_t dmc_stem_fwd_x3_workspace_bytes(int N, int H, int W);
int dmc_stem_fwd_x3(const float* x, const float* w, long ws_co, long ws_ci, long ws_ky, long ws_kx, void* workspace, float* y, int N,
                    int H, int W, dmc_stream_t stream);
/* dmc_stem_fwd_x3 that also reduces the BatchNorm batch statistics of its output in the epilogue (the stem's bn1,
 * /root/reference/code/dmcnet/model.py:305): stat_scratch (dmc_bn_act_scratch_bytes(64), nullable = plain forward)
 * receives dmc_stem_fwd_x3_stat_blocks(N, H, W) partial (sum, sum of squares) pairs per channel in the layout the
 * BatchNorm kernels reduce; pass that count as `stat_split` to dmc_bn_relu_pool_fwd_arg, which then skips its own
 * statistics pass over the (4x pooled-size) convolution output. */
int dmc_stem_fwd_x3_stat_blocks(int N, int H, int W);
int dmc_stem_fwd_x3_stats(const float* x, const float* w, long ws_co, long ws_ci, long ws_ky, long ws_kx, void* workspace, float* y,
                          void* stat_scratch, int N, int H, int W, dmc_stream_t stream);
/* Data gradient of the stem convolution (the gradient of the 2-channel cue: only the GAN variant needs it, where the
 * classifier's loss reaches the generator -- /root/reference/code/dmcnet_GAN/model.py:557-561; replaces the library
 * GEMM + col2im of autograd's conv2d backward): dx [N][2][H][W] fp32 contiguous from dy [N][OH][OW][64] fp32 (the memory
 * of a channels_last [N,64,OH,OW] tensor, OH = (H + 1) / 2, OW = (W + 1) / 2) and w [64,2,7,7] addressed by its element
 * strides; stride 2, padding 3; bf16x3 arithmetic (fp32-level error), deterministic; W <= 256.  workspace:
 * dmc_stem_dgrad_workspace_bytes() (the pre-split weights). */
size_t dmc_stem_dgrad_workspace_bytes(void);
int dmc_stem_dgrad_supported(int H, int W);
int dmc_stem_dgrad(const float* dy, const float* w, long ws_co, long ws_ci, long ws_ky, long ws_kx, void* workspace, float* dx, int N,
                   int H, int W, dmc_stream_t stream);

/* ---- I3D trunk: bf16 3-D convolutions on the matrix cores (BASELINE config 5) -------------------------
 * Replace nn.Conv3d and its autograd inside the reference's Unit3Dpy, code/dmcnet_I3D/network/i3d.py:328-403
 * (self.conv3d at :372-388, run at :393), for the trunk's stride-1 TF-"SAME" units: conv3d_2b_1x1, conv3d_2c_3x3
 * (:484-486) and the 1x1x1 / 3x3x3 branches of the nine Mixed blocks (:421-455, built at :491-513), as the
 * reference runs them in bf16/fp16-style mixed precision (fp32 master weights, 16-bit activations).
 * Layouts: activations bf16 NDHWC ([N][D][H][W][C], the memory of a channels_last_3d tensor); weights fp32
 * [Cout][Cin][KD][KH][KW] addressed by element strides (w_s_co, w_s_ci, w_s_tap: 1 for a contiguous parameter),
 * rounded to bf16 (nearest even) on the way into the packed workspace; fp32 accumulation; bf16 results rounded to
 * nearest even.  Kernel extents 1 or 3 per dimension, stride 1, zero padding k/2; Cin, Cout multiples of 8.
 * fwd: y = conv3d(x, w); if stat_partials != NULL also per-channel (sum, sum of squares) of the rounded y per
 * workgroup row, [dmc_conv3d_bf16_stat_blocks()][Cout][2] floats (for the BatchNorm3d that follows).
 * dgrad: dx = conv_transpose3d(dy, w).  wgrad: dw fp32 [Cout][Cin][KD][KH][KW] contiguous = sum over pixels
 * (1x1x1 and 3x3x3 only), deterministic split-K reduction; workspace of dmc_conv3d_bf16_wgrad_bytes().
 * wpack: workspace of dmc_conv3d_bf16_wpack_bytes() bytes; dmc_conv3d_bf16_pack() fills the forward's and the data
 * gradient's workspaces in one launch, and fwd / dgrad called with w == NULL use theirs as it is.
 */
int dmc_conv3d_bf16_supported(int N, int D, int H, int W, int Cin, int Cout, int KD, int KH, int KW);
size_t dmc_conv3d_bf16_wpack_bytes(int Cin, int Cout, int KD, int KH, int KW);
int dmc_conv3d_bf16_pack(const float* w, long w_s_co, long w_s_ci, long w_s_tap, void* wpack_f, void* wpack_b, int Cin, int Cout,
                         int KD, int KH, int KW, dmc_stream_t stream);
int dmc_conv3d_bf16_stat_blocks(int N, int D, int H, int W, int Cout);
/* rows of stat_partials dmc_conv3d_bf16_fwd writes for THIS layer (the 3x3x3 layers run a patch-resident kernel whose
 * workgroups are position tiles of one (n, d) plane; everything else: dmc_conv3d_bf16_stat_blocks) */
int dmc_conv3d_bf16_stat_blocks_k(int N, int D, int H, int W, int Cin, int Cout, int KD, int KH, int KW);
int dmc_conv3d_bf16_fwd(const void* x, const float* w, long w_s_co, long w_s_ci, long w_s_tap, void* wpack, void* y,
                        float* stat_partials, int N, int D, int H, int W, int Cin, int Cout, int KD, int KH, int KW,
                        dmc_stream_t stream);
int dmc_conv3d_bf16_dgrad(const void* dy, const float* w, long w_s_co, long w_s_ci, long w_s_tap, void* wpack, void* dx,
                          int N, int D, int H, int W, int Cin, int Cout, int KD, int KH, int KW, dmc_stream_t stream);
size_t dmc_conv3d_bf16_wgrad_bytes(int N, int D, int H, int W, int Cin, int Cout, int KD, int KH, int KW);
int dmc_conv3d_bf16_wgrad(const void* x, const void* dy, float* dw, float* workspace, int N, int D, int H, int W, int Cin,
                          int Cout, int KD, int KH, int KW, dmc_stream_t stream);

/* ---- I3D trunk: MaxPool3dTFPadding on bf16 NDHWC tensors -------------------------------------------
 * Replaces the reference's MaxPool3dTFPadding, code/dmcnet_I3D/network/i3d.py:406-418 (ConstantPad3d with zeros
 * to the TF-"SAME" extent, then nn.MaxPool3d(kernel, stride, ceil_mode=True)), and its autograd, as used at
 * :482,:488,:494,:505 and in every Mixed block (:441-443).  x [N,D,H,W,C] bf16 (channels_last_3d memory), C % 8 == 0;
 * front padding = max(k - s, 0) / 2 per dimension; the scan order and tie rule are nn.MaxPool3d's.  fwd also writes
 * one byte per output value (the winning tap; 255 = a padding zero) which bwd gathers from: no atomics,
 * deterministic, fp32 sums rounded once.  dmc_maxpool3d_tf_out_shape() returns 0 for unsupported arguments.
 */
int dmc_maxpool3d_tf_out_shape(int D, int H, int W, int C, int kd, int kh, int kw, int sd, int sh, int sw, int* od, int* oh,
                               int* ow);
int dmc_maxpool3d_tf_bf16_fwd(const void* x, void* y, void* code, int N, int D, int H, int W, int C, int kd, int kh, int kw,
                              int sd, int sh, int sw, dmc_stream_t stream);
int dmc_maxpool3d_tf_bf16_bwd(const void* dy, const void* code, void* dx, int N, int D, int H, int W, int C, int kd, int kh,
                              int kw, int sd, int sh, int sw, dmc_stream_t stream);

/* ---- I3D trunk: BatchNorm3d (+ ReLU) on bf16 NDHWC tensors, training mode ------------------------------
 * Replaces `self.batch3d(out)` and `F.relu` of the reference's Unit3Dpy.forward, code/dmcnet_I3D/network/i3d.py:394-398
 * (torch.nn.BatchNorm3d, batch statistics, running-statistics update), and their autograd, behind a convolution
 * that ran dmc_conv3d_bf16_fwd with stat_partials: y [M,C] bf16 (M = N*D*H*W), partials [nblk][C][2] floats.
 * fwd: stats [2*C] = (mean, invstd) (biased variance + eps), running_mean / running_var updated with `momentum`
 * (unbiased variance; NULL to skip), out = relu?(gamma * (y - mean) * invstd + beta) in bf16.
 * bwd: dy = gradient of y, dgamma, dbeta (fp32) from dout (pixel stride dout_ld elements: C, or the width of the
 * concatenated Inception output when dout is a channel slice of its gradient); scratch of dmc_bn3d_bf16_scratch_bytes(C).  fp32 per
 * element, fp64 per-channel sums in fixed order (deterministic).  C % 8 == 0, C <= 2048.
 */
int dmc_bn3d_bf16_supported(long M, int C);
size_t dmc_bn3d_bf16_scratch_bytes(int C);
int dmc_bn3d_bf16_fwd(const void* y, const float* partials, int nblk, const float* gamma, const float* beta, float* stats,
                      float* running_mean, float* running_var, void* out, long M, int C, int relu, float eps, float momentum,
                      dmc_stream_t stream);
/* the same with `out` a channel slice of a wider NDHWC tensor: out_ld = elements between consecutive pixels of `out` (a multiple
 * of 8, >= C; `out` 16-byte aligned) -- an Inception branch writes its part of the block's output in place (no concatenation) */
int dmc_bn3d_bf16_fwd_ld(const void* y, const float* partials, int nblk, const float* gamma, const float* beta, float* stats,
                         float* running_mean, float* running_var, void* out, long out_ld, long M, int C, int relu, float eps,
                         float momentum, dmc_stream_t stream);
/* out = ((a + b) + c) + d on bf16 arrays of n elements (n % 8 == 0, pointers 16-byte aligned), every sum rounded to bf16 (nearest
 * even) -- bit for bit what three additions of bf16 tensors give: the gradient of an Inception block's input
 * (network/i3d.py:449-454: four branches read x) in one pass instead of three. */
int dmc_add4_bf16(const void* a, const void* b, const void* c, const void* d, void* out, long n, dmc_stream_t stream);
int dmc_bn3d_bf16_bwd(const void* dout, long dout_ld, const void* y, const float* stats, const float* gamma, const float* beta,
                      float* scratch, void* dy, float* dgamma, float* dbeta, long M, int C, int relu, dmc_stream_t stream);

/* A whole Unit3Dpy (/root/reference/code/dmcnet_I3D/network/i3d.py:328-403: Conv3d -> BatchNorm3d(training) [-> ReLU]) per
 * call: dmc_unit3d_bf16_fwd = dmc_conv3d_bf16_pack + dmc_conv3d_bf16_fwd (statistics in its epilogue) + dmc_bn3d_bf16_fwd,
 * dmc_unit3d_bf16_bwd = dmc_bn3d_bf16_bwd + dmc_conv3d_bf16_dgrad (dx nullable) + dmc_conv3d_bf16_wgrad (dw nullable),
 * with every intermediate carved out of one workspace per direction (dmc_unit3d_bf16_{fwd,bwd}_workspace_bytes; the
 * backward reads the forward's workspace: statistics and the data-gradient weight layout).  w: fp32 [Cout][Cin][KD][KH][KW]
 * contiguous; x, y (convolution output), out, dout (pixel stride dout_ld elements), dy, dx: bf16 NDHWC; dw fp32 in w's
 * layout.  Same kernels in the same order as the separate calls: identical results; the trunk's ~940 launches per
 * micro-step are bound by the host that issues them, and this is a third of the foreign calls and allocations. */
size_t dmc_unit3d_bf16_fwd_workspace_bytes(int N, int D, int H, int W, int Cin, int Cout, int KD, int KH, int KW);
size_t dmc_unit3d_bf16_bwd_workspace_bytes(int N, int D, int H, int W, int Cin, int Cout, int KD, int KH, int KW);
int dmc_unit3d_bf16_fwd(const void* x, const float* w, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, void* workspace, void* y, void* out, int N, int D, int H, int W, int Cin, int Cout,
                        int KD, int KH, int KW, int relu, float eps, float momentum, dmc_stream_t stream);
/* dmc_unit3d_bf16_fwd with `out` a channel slice of a wider NDHWC tensor (see dmc_bn3d_bf16_fwd_ld) */
int dmc_unit3d_bf16_fwd_into(const void* x, const float* w, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, void* workspace, void* y, void* out, long out_ld, int N, int D, int H, int W, int Cin,
                             int Cout, int KD, int KH, int KW, int relu, float eps, float momentum, dmc_stream_t stream);
int dmc_unit3d_bf16_bwd(const void* dout, long dout_ld, const void* x, const void* y, const void* fwd_workspace, const float* gamma,
                        const float* beta, void* bwd_workspace, void* dy, void* dx, float* dw, float* dgamma, float* dbeta, int N,
                        int D, int H, int W, int Cin, int Cout, int KD, int KH, int KW, int relu, dmc_stream_t stream);
/* A whole Unit3Dpy in EVAL mode, forward only: code/dmcnet_I3D/network/i3d.py:390-398 with BatchNorm3d in eval mode (running
 * statistics) under no_grad.  One convolution launch (the kernels of dmc_conv3d_bf16_fwd: the same bf16-rounded master weights,
 * NOT folded with the BatchNorm) whose epilogue applies the BatchNorm as a per-channel affine map,
 *     out[m][co] = bf16(relu?(fma(acc, scale[co], shift[co]))),  scale = gamma / sqrt(running_var + eps),
 *     shift = beta - running_mean * scale  (fp32; fma = one rounding; bf16 round to nearest even, once),
 * scale / shift computed on the device by the weight-pack launch (no host synchronisation; capturable); no statistics, the
 * running buffers are read only.  out: pixel stride out_ld elements (>= Cout, a multiple of 8, `out` 16-byte aligned: a channel
 * slice of an Inception block's output); workspace: dmc_unit3d_bf16_eval_workspace_bytes(). */
size_t dmc_unit3d_bf16_eval_workspace_bytes(int N, int D, int H, int W, int Cin, int Cout, int KD, int KH, int KW);
int dmc_unit3d_bf16_fwd_eval(const void* x, const float* w, const float* gamma, const float* beta, const float* running_mean,
                             const float* running_var, float eps, void* workspace, void* out, long out_ld, int N, int D, int H, int W,
                             int Cin, int Cout, int KD, int KH, int KW, int relu, dmc_stream_t stream);

/* ---- I3D stem: forward of conv3d_1a_7x7 on the bf16 matrix cores -----------------------------------------
 * Replaces ConstantPad3d(TF-"SAME": front 2, back 3) + nn.Conv3d(2, 64, 7, stride 2) of the stem Unit3Dpy,
 * code/dmcnet_I3D/network/i3d.py:480-481 via :390-393, as run in 16-bit mixed precision: x [N,2,T,H,W] fp32 (the DMC
 * cue) and w [64,2,7,7,7] fp32 contiguous are rounded to bf16, fp32 accumulation, y [N,OD,OH,OW,64] bf16 NDHWC with
 * OD = (T + 5 - 7) / 2 + 1 (likewise OH, OW); stat_partials (NULL to skip): [dmc_stem3d_bf16_stat_blocks()][64][2]
 * floats = per-channel (sum, sum of squares) of the rounded outputs, for dmc_bn3d_bf16_fwd.  workspace:
 * dmc_stem3d_bf16_workspace_bytes().
 */
size_t dmc_stem3d_bf16_workspace_bytes(int N, int T, int H, int W);
int dmc_stem3d_bf16_stat_blocks(int N, int T, int H, int W);
int dmc_stem3d_bf16_fwd(const float* x, const float* w, void* workspace, void* y, float* stat_partials, int N, int T, int H, int W,
                        dmc_stream_t stream);
/* the stem unit in EVAL mode, forward only (code/dmcnet_I3D/network/i3d.py:480-481 through :390-398, BatchNorm3d with running
 * statistics, under no_grad): dmc_stem3d_bf16_fwd with the epilogue of dmc_unit3d_bf16_fwd_eval, y dense NDHWC;
 * workspace: dmc_stem3d_bf16_eval_workspace_bytes(). */
size_t dmc_stem3d_bf16_eval_workspace_bytes(int N, int T, int H, int W);
int dmc_stem3d_bf16_fwd_eval(const float* x, const float* w, const float* gamma, const float* beta, const float* running_mean,
                             const float* running_var, float eps, void* workspace, void* y, int N, int T, int H, int W, int relu,
                             dmc_stream_t stream);
/* weight gradient of the same convolution: dw [64,2,7,7,7] fp32 contiguous from x (rounded to bf16 as in the forward) and
 * dy [N,OD,OH,OW,64] bf16 NDHWC; GEMM over pixels on the bf16 matrix cores (plane form for rows of up to 125 output pixels:
 * csrc/stem3d_bf16.hip, stem3d_w2_kernel), deterministic split-K reduction; workspace: dmc_stem3d_bf16_wgrad_workspace_bytes(). */
size_t dmc_stem3d_bf16_wgrad_workspace_bytes(int N, int T, int H, int W);
int dmc_stem3d_bf16_wgrad(const float* x, const void* dy, float* dw, void* workspace, int N, int T, int H, int W, dmc_stream_t stream);
/* data gradient of the same convolution (the gradient of the cue): dx [N,2,T,H,W] fp32 from dy [N,OD,OH,OW,64] bf16 NDHWC and
 * w (rounded to bf16); per input row a GEMM Q[ow][(kx,c)] over (window rows, channels) on the bf16 matrix cores and a 1-D fold
 * along x; W <= 256; deterministic; workspace: dmc_stem3d_bf16_dgrad_workspace_bytes(). */
size_t dmc_stem3d_bf16_dgrad_workspace_bytes(void);
int dmc_stem3d_bf16_dgrad(const void* dy, const float* w, float* dx, void* workspace, int N, int T, int H, int W, dmc_stream_t stream);

/* ---- Post-decode motion-vector / residual extraction ---------------------------------------
 * Replaces the integer loops of create_and_load_mv_residual(), code/dmcnet/data_loader/coviar_data_loader.c:71-175, and
 * the accumulator set-up of decode_video(), :306-319, on arrays the decoder hands over (the bitstream decode itself is
 * FFmpeg's and stays on the host).  `mvs`: DEVICE copy of the frame's AV_FRAME_DATA_MOTION_VECTORS side data, an array
 * of AVMotionVector (libavutil/motion_vector.h, public ABI: int32 source @0, uint8 w @4, h @5, int16 src_x @6, src_y @8,
 * dst_x @10, dst_y @12), `mv_stride` = the caller's sizeof(AVMotionVector) (24 before libavutil 55.63, 40 since).
 * Accumulators use the reference's TRANSPOSED layout, accu[x * H * 2 + y * 2 + c] (:107-108); MV planes are int32
 * [H][W][2] and residuals int32 [H][W][3] as its numpy arrays (:292-309); BGR frames uint8 [H][W][3].
 * Overlapping blocks: the LATER vector of the list wins, as in the sequential loop (realised as the per-pixel maximum of
 * the covering vectors' indices, resolved tile by tile in LDS; owner_ws, int32 [H][W], receives the winner's displacement
 * (src - dst) as two int16: order-independent, bit-exact).  Vectors with zero displacement are skipped (:88); a (block pixel) is written only when destination AND source are inside the frame (:100-103).
 * bad_source (nullable): device int32 incremented once per vector whose `source` is not -1 (the reference asserts, :86).
 *
 *   dmc_mv_accu_init   :311-318  accu = identity (x, y)
 *   dmc_mv_rasterise   :88-121, `accumulate == 0` branch: covered pixels of mv_out get (dst - src); the others keep
 *                      their value (the reference's array is zero-initialised once, :292-298)
 *   dmc_mv_accumulate  :88-127, `accumulate != 0` branch, ONE frame: accu_new[dst] = accu_old[src] where covered,
 *                      accu_old[dst] elsewhere (the reference's two buffers + memcpy; here the caller swaps the pointers)
 *   dmc_mv_from_accu   :130-139  mv_out[y][x] = (x, y) - accu[x][y]
 *   dmc_residual       :141-175  res[y][x][c] = bgr_cur[y][x][c] - bgr_ref[src_y][src_x][c], src from `accu`
 *                      (accumulate) or (x, y) - `mv` (not): pass exactly one of the two.  The source position is NOT
 *                      range-checked (neither is the reference's loop): every `accu` entry / every (x, y) - mv must lie
 *                      inside the frame, which holds for what dmc_mv_accu_init / dmc_mv_accumulate produce and for an mv
 *                      plane rasterised over ZEROS (or from dmc_mv_from_accu) -- not for a plane with other values left
 *                      in its uncovered pixels
 *   dmc_mv_gop_batch   a BATCH of accumulated chains in two launches: chain c owns the frames chain_off[c] ..
 *                      chain_off[c + 1] - 1 (in decode order), frame f the vectors frame_off[f] .. frame_off[f + 1] - 1
 *                      (device int32 arrays of n_chains + 1 / n_frames + 1 entries; owner_ws of dmc_mv_owner_bytes(n_frames,
 *                      H, W)).  Every pixel is walked back through its chain's owner maps -- the same values as n calls of
 *                      dmc_mv_accumulate from the identity -- and whichever of accu_out [n_chains][W][H][2], mv_out
 *                      [n_chains][H][W][2], res_out [n_chains][H][W][3] (bgr_ref / bgr_cur [n_chains][H][W][3]) is non-NULL
 *                      is written.  emit (nullable, device int32 [n_chains]): 0 = leave that chain's outputs untouched (the
 *                      reference's `cur_pos > 0` and `if (sd)` gates, :128, :363).  A one-frame chain is also the
 *                      non-accumulating case (mv = dst - src of the owner, 0 elsewhere).
 */
size_t dmc_mv_owner_bytes(int n_frames, int H, int W);
int dmc_mv_accu_init(int32_t* accu, int H, int W, dmc_stream_t stream);
int dmc_mv_rasterise(const void* mvs, int mv_stride, int n_mv, int32_t* owner_ws, int32_t* mv_out, int32_t* bad_source, int H,
                     int W, dmc_stream_t stream);
int dmc_mv_accumulate(const void* mvs, int mv_stride, int n_mv, int32_t* owner_ws, const int32_t* accu_old, int32_t* accu_new,
                      int32_t* bad_source, int H, int W, dmc_stream_t stream);
int dmc_mv_from_accu(const int32_t* accu, int32_t* mv_out, int H, int W, dmc_stream_t stream);
int dmc_residual(const uint8_t* bgr_ref, const uint8_t* bgr_cur, const int32_t* accu, const int32_t* mv, int32_t* res, int H, int W,
                 dmc_stream_t stream);
int dmc_mv_gop_batch(const void* mvs, int mv_stride, int n_mv, const int32_t* frame_off, int n_frames, const int32_t* chain_off,
                     int n_chains, const int32_t* emit, int32_t* owner_ws, const uint8_t* bgr_ref, const uint8_t* bgr_cur,
                     int32_t* accu_out, int32_t* mv_out, int32_t* res_out, int32_t* bad_source, int H, int W, dmc_stream_t stream);

/* ---- ContextNetwork / ContextNetworkAtt in eval mode (csrc/ctx_eval.hip) ----
 * Replaces: the units Conv2d(3x3, dilation d, padding d, bias=False) -> BatchNorm2d (running statistics) -> LeakyReLU(0.1) of
 *           code/dmcnet/model.py:45-104 as the evaluator runs them under model.eval() + no_grad; one launch per unit, the
 *           normalisation and the activation in the convolution's epilogue.  Activations between units are NHWC fp32.
 * BatchNorm: stats = mean[C], 1 / sqrt(var + eps)[C]; gamma[C], beta[C].  Result = leaky((conv - mean) * invstd * gamma + beta).
 * dmc_ctx_unit_supported: 1 for the first unit (Cin 5, Cout 32, dilation 1), the heads (Cin 32, Cout 2, dilation 1) and the
 *   middle units (Cin, Cout in {32, 64, 96, 128}, dilation in {1, 2, 4, 8, 16}) when N, H, W > 0 and N * H * W * 128 < 2^31
 *   (what one launch indexes; the caller splits larger batches into frame ranges), else 0.
 * dmc_ctx_pack_weights: w OHWI [Cout][3][3][Cin] fp32 -> wpack, dmc_ctx_wpack_bytes() bytes (three bf16 slices,
 *   [tap][Cin / 16][slice][Cout][16]; 0 for an unsupported channel pair).
 * dmc_ctx_unit_eval: a middle unit, x NHWC [N][H][W][Cin] -> y NHWC [N][H][W][Cout]; bf16x3 arithmetic on the matrix cores.
 * dmc_ctx_first_eval: the first unit, x NCHW [N][5][H][W], w OIHW [32][5][3][3] (the module's weight as stored) -> y NHWC
 *   [N][H][W][32]; fp32 FMAs in a fixed order.
 * dmc_ctx_heads_eval: x NHWC [N][H][W][32], w_flow / w_att OHWI [2][3][3][32] -> flow NCHW [N][2][H][W] and, when w_att is
 *   given, att NCHW [N][2][H][W] = max(unit(x), 0), both heads in one launch.  w_att == NULL: one head, att must be NULL.
 * Deterministic, no atomics, independent of the batch a frame is in; inputs are read only.
 * DMC_E_INVALID before any launch (nothing written): a NULL pointer (the attention group excepted, all or none), a shape
 * outside dmc_ctx_unit_supported(). */
int dmc_ctx_unit_supported(int N, int H, int W, int Cin, int Cout, int dilation);
size_t dmc_ctx_wpack_bytes(int Cin, int Cout);
int dmc_ctx_pack_weights(const float* w, void* wpack, int Cin, int Cout, dmc_stream_t stream);
int dmc_ctx_unit_eval(const float* x, const void* wpack, const float* stats, const float* gamma, const float* beta, float* y,
                      int N, int H, int W, int Cin, int Cout, int dilation, dmc_stream_t stream);
int dmc_ctx_first_eval(const float* x, const float* w, const float* stats, const float* gamma, const float* beta, float* y,
                       int N, int H, int W, dmc_stream_t stream);
int dmc_ctx_heads_eval(const float* x, const float* w_flow, const float* stats_flow, const float* gamma_flow, const float* beta_flow,
                       const float* w_att, const float* stats_att, const float* gamma_att, const float* beta_att, float* flow,
                       float* att, int N, int H, int W, dmc_stream_t stream);

/* ---- ContextNetwork / ContextNetworkAtt in training: the dilated convolutions (csrc/dconv.hip) ----
 * Replaces: Conv2d(Cin, Cout, 3, stride 1, padding d, dilation d, bias=False) of the middle units of
 *           code/dmcnet/model.py:45-104 -- its forward, its data gradient and its weight gradient -- over NHWC fp32 tensors
 *           (channels_last memory).  BatchNorm2d and LeakyReLU are not part of it.  bf16x3 arithmetic on the matrix cores.
 * dmc_dconv_supported (code/dmcnet/model.py:45-104): 1 when Cin, Cout in {32, 64, 96, 128}, dilation in {1, 2, 4, 8, 16},
 *   N, H, W > 0 and N * H * W * 128 < 2^31 (what one launch indexes), else 0.
 * dmc_dconv_wpack_bytes (code/dmcnet/model.py:45-104): Cin * Cout * 9 * 3 * 2, the bytes of a weight pack; 0 for an
 *   unsupported channel pair.
 * dmc_dconv_wgrad_workspace_bytes (code/dmcnet/model.py:45-104): the bytes dmc_dconv_wgrad uses of `workspace` (per-range
 *   partial sums, every byte written before it is read); 0 for an unsupported shape.
 * dmc_dconv_pack_weights (code/dmcnet/model.py:45-104): w OHWI [Cout][3][3][Cin] fp32 -> wpack (three bf16 slices).
 *   transposed == 0: the forward's pack [tap][Cin / 16][slice][Cout][16].  transposed != 0: the data gradient's,
 *   W'[ci][t'][co] = W[co][8 - t'][ci] in the same layout with Cin and Cout exchanged, [tap'][Cout / 16][slice][Cin][16].
 * dmc_dconv_fwd (code/dmcnet/model.py:45-104): y NHWC [N][H][W][Cout] = conv(x NHWC [N][H][W][Cin]) with the forward's pack.
 *   The data gradient is the same call: dx = dmc_dconv_fwd(dy, transposed pack, dx, N, H, W, Cout, Cin, d) (Cin and Cout
 *   exchanged), because with stride 1 and padding = dilation the taps mirror.
 * dmc_dconv_wgrad (code/dmcnet/model.py:45-104): dw OHWI [Cout][3][3][Cin] = sum over pixels of dy[p][co] x[p + tap][ci],
 *   x NHWC [N][H][W][Cin], dy NHWC [N][H][W][Cout]; every element of dw is written (a tap no pixel reaches: 0).
 * Deterministic, no atomics; the forward / data gradient of a frame is independent of its batch.  Inputs are read only.
 * DMC_E_INVALID before any launch (nothing written): a NULL pointer, a shape outside dmc_dconv_supported(). */
int dmc_dconv_supported(int N, int H, int W, int Cin, int Cout, int dilation);
size_t dmc_dconv_wpack_bytes(int Cin, int Cout);
size_t dmc_dconv_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int dmc_dconv_pack_weights(const float* w_ohwi, void* wpack, int Cin, int Cout, int transposed, dmc_stream_t stream);
int dmc_dconv_fwd(const float* x, const void* wpack, float* y, int N, int H, int W, int Cin, int Cout, int dilation,
                  dmc_stream_t stream);
int dmc_dconv_wgrad(const float* x, const float* dy, float* dw_ohwi, void* workspace, int N, int H, int W, int Cin, int Cout,
                    int dilation, dmc_stream_t stream);

/* ---- ContextNetwork / ContextNetworkAtt in training: BatchNorm2d + LeakyReLU (csrc/ctx_bn.hip) ----
 * Replaces: nn.BatchNorm2d in train() (batch statistics) followed by the in-place nn.LeakyReLU of the units of
 *           code/dmcnet/model.py:45-104, and their backward passes, over [M][C] fp32 row-major views of channels_last memory
 *           (M = N * H * W).  The convolution in front is not part of it.
 * dmc_bnlrelu_supported (code/dmcnet/model.py:45-104): 1 when C in {32, 64, 96, 128}, M >= 2 and M * C < 2^31, else 0.
 * dmc_bnlrelu_scratch_bytes (code/dmcnet/model.py:45-104): the exact bytes both launching entry points use of `scratch` (fp64
 *   per-workgroup partial sums, then 2 C floats of the backward; every byte is written before it is read); 0 when unsupported.
 * dmc_bnlrelu_fwd (code/dmcnet/model.py:45-104): stats = (mean[C], invstd[C]) of z with invstd = (biased var + eps)^-1/2, sums
 *   and statistics in fp64; y = t > 0 ? t : slope * t with t = fmaf((z - mean) * invstd, gamma, beta), the expression of
 *   dmc_ctx_unit_eval.  running_mean / running_var (both or neither; may be NULL) are updated as nn.BatchNorm2d does:
 *   r = (1 - momentum) r + momentum * (mean | var * M / (M - 1)).
 * dmc_bnlrelu_bwd (code/dmcnet/model.py:45-104): from z, dy and the forward's stats (y is not read): t is recomputed with the
 *   forward's expression, g = dy * (t > 0 ? 1 : slope) (t == 0 takes slope), xhat = (z - mean) * invstd;
 *   dbeta = sum g, dgamma = sum g xhat (fp64 sums), dz = gamma invstd (g - dbeta / M - xhat dgamma / M).
 * Deterministic, no atomics: bit-identical from run to run.  Inputs are read only.
 * DMC_E_INVALID before any launch (nothing written): a NULL required pointer, exactly one running pointer, a shape outside
 * dmc_bnlrelu_supported(), eps <= 0, slope outside (0, 1), momentum outside [0, 1]. */
int dmc_bnlrelu_supported(int M, int C);
size_t dmc_bnlrelu_scratch_bytes(int M, int C);
int dmc_bnlrelu_fwd(const float* z, const float* gamma, const float* beta, float* running_mean, float* running_var, float* y,
                    float* stats, void* scratch, int M, int C, float slope, float eps, float momentum, dmc_stream_t stream);
int dmc_bnlrelu_bwd(const float* z, const float* dy, const float* gamma, const float* beta, const float* stats, void* scratch,
                    float* dz, float* dgamma, float* dbeta, int M, int C, float slope, dmc_stream_t stream);

/* ---- ContextNetwork / ContextNetworkAtt in training: the first unit's convolution and the head(s) (csrc/ctx_ends.hip) ----
 * Replaces: Conv2d(5, 32, 3, 1, 1, 1, bias=False) of the first unit, Conv2d(32, 2, 3, 1, 1, 1, bias=False) of predict_flow and
 *           predict_att and the heads' nn.BatchNorm2d(2) in train() + nn.LeakyReLU (+ nn.ReLU behind predict_att) of
 *           code/dmcnet/model.py:45-104 -- forward, data gradient, weight gradient -- in plain fp32 FMAs.
 * Layouts: x, dx NCHW [N][5][H][W]; the first unit's output z and its gradient dz, the trunk activation t and its gradient dt
 *   NHWC [N][H][W][32]; a head's convolution output and its gradient NCHW [N][2][H][W]; w_first OIHW [32][5][3][3]; a head's
 *   weight OHWI [2][3][3][32] (the layouts of dmc_ctx_first_eval / dmc_ctx_heads_eval).  o(t) = (t / 3 - 1, t % 3 - 1); a tap
 *   outside the H x W frame contributes 0.
 * dmc_ctxends_supported (code/dmcnet/model.py:45-104): 1 when N, H, W > 0 and N * H * W * 128 < 2^31, else 0.
 * dmc_ctxends_wgrad_workspace_bytes (code/dmcnet/model.py:45-104): the exact bytes a weight gradient over `planes` planes uses
 *   of `workspace` (5: dmc_ctxends_first_wgrad; 2 per head that has a gradient: dmc_ctxends_heads_wgrad): per-range partial
 *   sums, every byte written before it is read; 0 for an unsupported shape or another plane count.
 * dmc_ctxends_bn_scratch_bytes (code/dmcnet/model.py:45-104): the exact bytes dmc_ctxends_bn_fwd / _bwd use of `scratch` (fp64
 *   per-workgroup partial sums, then 4 floats of the backward); 0 when unsupported or N * H * W < 2.
 * dmc_ctxends_first_fwd (code/dmcnet/model.py:45-104): z[p][co] = sum_{ci,t} x[ci][p + o(t)] w[co][ci][t], summed over
 *   (ci, ky, kx) in that order with fmaf: the sum of dmc_ctx_first_eval, bit for bit.
 * dmc_ctxends_first_dgrad (code/dmcnet/model.py:45-104): dx[ci][p] = sum_{t,co} dz[p - o(t)][co] w[co][ci][t].
 * dmc_ctxends_first_wgrad (code/dmcnet/model.py:45-104): dw[co][ci][t] = sum_p dz[p][co] x[ci][p + o(t)]; every element of dw
 *   is written (a tap no pixel reaches: 0).
 * dmc_ctxends_heads_fwd (code/dmcnet/model.py:45-104): z_k[c][p] = sum_{t,ci} t[p + o(t)][ci] w_k[c][t][ci] for the flow head
 *   and, when w_att and z_att are given (together or not at all), the attention head, in one launch that reads t once: the
 *   sums of dmc_ctx_heads_eval, bit for bit.
 * dmc_ctxends_heads_dgrad (code/dmcnet/model.py:45-104): dt[p][ci] = sum over the heads of sum_{t,c} dz_k[c][p - o(t)]
 *   w_k[c][t][ci], both heads in one launch.  w_att NULL: a network with one head (dz_att must be NULL too).  With w_att, a NULL
 *   dz_flow or dz_att means that head got no gradient (at least one is given).
 * dmc_ctxends_heads_wgrad (code/dmcnet/model.py:45-104): dw_k[c][t][ci] = sum_q t[q][ci] dz_k[c][q - o(t)] for every head whose
 *   (dz, dw) pair is given (a pair is present or absent together; at least one pair); a head without a pair is not touched.
 * dmc_ctxends_bn_fwd (code/dmcnet/model.py:45-104): on the planes z [N][2][H][W] with statistics over M = N H W per channel:
 *   stats = (mean[2], invstd[2]), sums and statistics in fp64 exactly as dmc_bnlrelu_fwd; y = t > 0 ? t : slope * t with
 *   t = fmaf((z - mean) * invstd, gamma, beta), and y = max(y, 0) when relu != 0 (the attention head).  running_mean /
 *   running_var as dmc_bnlrelu_fwd.
 * dmc_ctxends_bn_bwd (code/dmcnet/model.py:45-104): from z, dy and the forward's stats (y is not read):
 *   g = dy * (t > 0 ? 1 : slope), or dy * (t > 0 ? 1 : 0) when relu != 0 (t == 0 takes the lower branch); dbeta = sum g,
 *   dgamma = sum g xhat (fp64 sums), dz = gamma invstd (g - dbeta / M - xhat dgamma / M).
 * Deterministic, no atomics: bit-identical from run to run; the forward / data gradients of a frame are independent of its batch.
 * Inputs are read only.  H * W may be odd (planes need no 16-byte alignment).
 * DMC_E_INVALID before any launch (nothing written): a NULL required pointer, a half-given attention group or (dz, dw) pair,
 * exactly one running pointer, a shape outside dmc_ctxends_supported() (N * H * W < 2 for the BatchNorm), eps <= 0, slope
 * outside (0, 1), momentum outside [0, 1]. */
int dmc_ctxends_supported(int N, int H, int W);
size_t dmc_ctxends_wgrad_workspace_bytes(int N, int H, int W, int planes);
size_t dmc_ctxends_bn_scratch_bytes(int N, int H, int W);
int dmc_ctxends_first_fwd(const float* x, const float* w, float* z, int N, int H, int W, dmc_stream_t stream);
int dmc_ctxends_first_dgrad(const float* dz, const float* w, float* dx, int N, int H, int W, dmc_stream_t stream);
int dmc_ctxends_first_wgrad(const float* x, const float* dz, float* dw, void* workspace, int N, int H, int W, dmc_stream_t stream);
int dmc_ctxends_heads_fwd(const float* t, const float* w_flow, const float* w_att, float* z_flow, float* z_att, int N, int H, int W,
                          dmc_stream_t stream);
int dmc_ctxends_heads_dgrad(const float* dz_flow, const float* dz_att, const float* w_flow, const float* w_att, float* dt, int N,
                            int H, int W, dmc_stream_t stream);
int dmc_ctxends_heads_wgrad(const float* t, const float* dz_flow, const float* dz_att, float* dw_flow, float* dw_att,
                            void* workspace, int N, int H, int W, dmc_stream_t stream);
int dmc_ctxends_bn_fwd(const float* z, const float* gamma, const float* beta, float* running_mean, float* running_var, float* y,
                       float* stats, void* scratch, int N, int H, int W, float slope, float eps, float momentum, int relu,
                       dmc_stream_t stream);
int dmc_ctxends_bn_bwd(const float* z, const float* dy, const float* gamma, const float* beta, const float* stats, void* scratch,
                       float* dz, float* dgamma, float* dbeta, int N, int H, int W, float slope, int relu, dmc_stream_t stream);

/* ---- EstimatorDenseNet / EstimatorDenseNetSmall in eval mode (csrc/dense_eval.hip) ----
 * Replaces: the dense stack of code/dmcnet/model.py:122-170 as the evaluator runs it under model.eval() + no_grad,
 *           x = cat(LeakyReLU_0.1(conv_i(x)), x) five times and predict_flow, every convolution 3x3 / stride 1 / padding 1 with bias,
 *           without materialising a concatenation.
 * The feature buffer: feat NHWC fp32 [N][H][W][CT], channels in slots in production order: [0, 16) = the 5 input channels and 11
 *   zeros, then the output of each layer padded with zeros to a multiple of 32 channels.  A layer reads the prefix [0, K) of every
 *   pixel and writes [K, K + R) of the same buffer; the caller permutes each weight's input channels into buffer order, with
 *   zero rows / columns / bias entries for the pad channels (ops.dense_eval_layout describes the order).
 * dmc_dense_supported: 1 when N, H, W, CT > 0, CT % 4 == 0, K >= 16, K % 16 == 0, N * H * W * CT < 2^31 (what one launch indexes;
 *   the caller splits larger batches into frame ranges) and either R in {32, 64, 96, 128} with K + R <= CT (a layer) or R == 2
 *   with K <= CT, K <= 512 (the head); else 0.
 * dmc_dense_wpack_bytes: K * R * 9 * 3 * 2, the bytes of a layer's weight pack; 0 for an unsupported (K, R).
 * dmc_dense_pack_weights: w OHWI [R][3][3][K] fp32 (padded, buffer order) -> wpack: three bf16 slices, [tap][K / 16][slice][R][16].
 * dmc_dense_ingest: x NCHW [N][5][H][W] -> feat[.][0, 16): the 5 values, then 11 zeros (+0.0).  CT >= 16; other channels untouched.
 * dmc_dense_layer_eval: feat[.][K, K + R) = leaky_0.1(conv3x3(feat[.][0, K)) + bias[R]) in place; bf16x3 arithmetic on the matrix
 *   cores.  Reads only channels < K, writes only channels in [K, K + R): every other byte of feat is left as it is.
 * dmc_dense_head_eval: out NCHW [N][2][H][W] = conv3x3(feat[.][0, K)) + bias[2], w [2][3][3][K] in buffer order; fp32 FMAs in a
 *   fixed order.
 * Deterministic, no atomics, independent of the batch a frame is in; inputs are read only.
 * DMC_E_INVALID before any launch (nothing written): a NULL pointer, a shape outside dmc_dense_supported(). */
int dmc_dense_supported(int N, int H, int W, int CT, int K, int R);
size_t dmc_dense_wpack_bytes(int K, int R);
int dmc_dense_pack_weights(const float* w_ohwi_padded, void* wpack, int K, int R, dmc_stream_t stream);
int dmc_dense_ingest(const float* x_nchw, float* feat, int N, int H, int W, int CT, dmc_stream_t stream);
int dmc_dense_layer_eval(float* feat, const void* wpack, const float* bias, int N, int H, int W, int CT, int K, int R,
                         dmc_stream_t stream);
int dmc_dense_head_eval(const float* feat, const float* w, const float* bias, float* out_nchw, int N, int H, int W, int CT, int K,
                        dmc_stream_t stream);

/* ---- EstimatorDenseNet / EstimatorDenseNetSmall in training: the backward on the feature buffer (csrc/dense_train.hip) ----
 * Replaces: autograd's backward of the dense stack above (code/dmcnet/model.py:122-170) -- five concatenations, six convolutions and
 *           five LeakyReLUs with every intermediate saved -- given the feature buffer feat [N][H][W][CT] the forward (dmc_dense_ingest,
 *           dmc_dense_layer_eval x 5, dmc_dense_head_eval) left behind.  G [N][H][W][CT] fp32, same layout, holds dL/d(feat).
 *           (The prefix is dmc_densetrain_, not dmc_dense_train_: the names under dmc_dense_ are the eval route's and are pinned.)
 * dmc_densetrain_supported: dmc_dense_supported(N, H, W, CT, K, R), and for the head (R == 2) K == CT <= 512.
 * dmc_densetrain_*_workspace_bytes: the bytes the entry point of that name uses of `workspace` (per-range / per-workgroup partial
 *   sums); 0 for an unsupported shape.  mask: ceil(NHW / 1024) * R * 4.  wgrad: ranges * R * 9 * K * 4, ranges as in
 *   dmc_dconv_wgrad (32-pixel steps, at most 256 steps a range, 64 ranges when that allows).  head: ranges * (18 CT + 2) * 4.
 * dmc_densetrain_head_dgrad: G[m][c] = sum_t sum_co dout[m - o(t)][co] w[co][t][c] for every c < CT (w [2][3][3][CT], buffer order;
 *   dout NCHW [N][2][H][W]): writes EVERY float of G; fp32 FMAs in a fixed order.
 * dmc_densetrain_head_wgrad: dw [2][3][3][CT] = sum_m dout[m][co] feat[m + o(t)][c], db [2] = sum_m dout[m][co]; fp32 FMAs, pixels in
 *   order within a range, ranges in order.
 * dmc_densetrain_mask: G[.][K + r] <- feat[.][K + r] > 0 ? g : 0.1f * g in place for r < R, db [R] = the sums of the result over the
 *   pixels.  Every other channel of G is left as it is; feat is read only.
 * dmc_densetrain_layer_wgrad: dw OHWI [R][3][3][K] (buffer order) = sum_m G[m][K + r] feat[m + o(t)][c]; bf16x3 arithmetic on the
 *   matrix cores, at most 8 k pixels per fp32 accumulation.  Reads feat channels [0, K) and G channels [K, K + R) only.
 * dmc_densetrain_layer_dgrad: G[m][c] += sum_t sum_r G[m - o(t)][K + r] w[r][t][c] in place for c0 <= c < min(c0 + cb, K): one block
 *   of at most 128 channels a call.  wpack_t = dmc_dconv_pack_weights(w[:, :, :, c0 : c0 + cb] (zero columns from K on) as
 *   OHWI [R][3][3][cb], cb, R, transposed = 1); cb in {32, 64, 96, 128}, c0 % 16 == 0, c0 < K, c0 + cb <= K + 16.  Reads channels
 *   [K, K + R) only, writes the block only; bf16x3 arithmetic on the matrix cores.
 * dmc_densetrain_export: dx NCHW [N][5][H][W] = G[.][0, 5).
 * Deterministic, no atomics; the caller owns every buffer; nothing allocates or synchronises.
 * DMC_E_INVALID before any launch (nothing written): a NULL pointer, an unsupported shape. */
int dmc_densetrain_supported(int N, int H, int W, int CT, int K, int R);
size_t dmc_densetrain_mask_workspace_bytes(int N, int H, int W, int R);
size_t dmc_densetrain_wgrad_workspace_bytes(int N, int H, int W, int K, int R);
size_t dmc_densetrain_head_workspace_bytes(int N, int H, int W, int CT);
int dmc_densetrain_head_dgrad(const float* dout_nchw, const float* w, float* G, int N, int H, int W, int CT, dmc_stream_t stream);
int dmc_densetrain_head_wgrad(const float* dout_nchw, const float* feat, float* dw, float* db, void* workspace, int N, int H, int W,
                              int CT, dmc_stream_t stream);
int dmc_densetrain_mask(const float* feat, float* G, float* db, void* workspace, int N, int H, int W, int CT, int K, int R,
                        dmc_stream_t stream);
int dmc_densetrain_layer_wgrad(const float* feat, const float* G, float* dw_ohwi, void* workspace, int N, int H, int W, int CT, int K,
                               int R, dmc_stream_t stream);
int dmc_densetrain_layer_dgrad(float* G, const void* wpack_t, int N, int H, int W, int CT, int K, int R, int c0, int cb,
                               dmc_stream_t stream);
int dmc_densetrain_export(const float* G, float* dx_nchw, int N, int H, int W, int CT, dmc_stream_t stream);

/* ---- EstimatorDenseNetTinyEarlyFusionSum / EstimatorDenseNetTinyEarlyFusionStack, forward and backward (csrc/early_fusion.hip) ----
 * Replaces: the two early-fusion estimators of code/dmcnet/model.py:197-250 -- m = LeakyReLU_0.1(conv_0_mv(x[:, :2])),
 *           r = LeakyReLU_0.1(conv_0_r(x[:, 2:])), x = cat(m, r) (Stack) or m + r (Sum), x = cat(LeakyReLU_0.1(conv_i(x)), x) for
 *           i = 1 .. 4, predict_flow(x); every convolution 3x3 / stride 1 / padding 1 with bias -- and autograd's backward of it
 *           with respect to the fourteen parameters, without materialising a concatenation.
 * The feature buffer: feat NHWC fp32 [N][H][W][CT], channels in slots in production order, every slot padded with +0.0 to a
 *   multiple of 4 channels.  Sum: s (0, 8), y1 (8, 8), y2 (16, 6), y3 (24, 4), y4 (28, 2), CT 32.  Stack: m (0, 8), r (8, 8),
 *   y1 (16, 8), y2 (24, 6), y3 (32, 4), y4 (36, 2), CT 40 (first channel, live channels; ops.early_fusion_layout).  A layer reads
 *   the prefix [0, K) of every pixel and writes [K, K + round_up4(R)) of the same buffer; the caller permutes each weight's input
 *   channels into buffer order with zero columns for the pad channels: w [R][9][K] = [output channel][tap ky * 3 + kx][buffer
 *   channel].  G [N][H][W][CT] fp32, same layout, holds dL/d(feat).  o(t) = the pixel offset (ky - 1, kx - 1) of tap t; a tap
 *   outside the frame contributes nothing.
 * dmc_ef_supported: 1 when N, H, W > 0, CT > 0, CT % 4 == 0, CT <= 64, K > 0, K % 4 == 0, R in {2, 4, 6, 8}, N * H * W * CT < 2^31
 *   (what one launch indexes; the caller splits larger batches into frame ranges) and either K + round_up4(R) <= CT (a layer) or
 *   R == 2 with K <= CT (the head); else 0.  The layer entry points (dmc_ef_layer, dmc_ef_layer_mask, dmc_ef_layer_wgrad,
 *   dmc_ef_layer_dgrad) also need K + round_up4(R) <= CT when R == 2.
 * dmc_ef_*_workspace_bytes: the bytes the entry point of that name uses of `workspace` (partial sums per run of 1024 pixels);
 *   0 for an unsupported shape.  parts = ceil(N H W / 1024).  head_wgrad: parts * (18 K + 2) * 4.  layer_wgrad: parts * R * 9 * K * 4.
 *   layer_mask: parts * round_up4(R) * 4.  first_bwd: parts * 376 * 4.
 * dmc_ef_first: x NCHW [N][5][H][W], w_mv [8][2][3][3], b_mv [8], w_r [8][3][3][3], b_r [8] (PyTorch's native layouts).  a =
 *   conv_0_mv(x[:, :2]) + b_mv, b = conv_0_r(x[:, 2:]) + b_r, each summed in its own fixed order (the same bits for both values of
 *   `stack`).  stack = 1: feat[.][0, 8) = leaky(a), feat[.][8, 16) = leaky(b), CT >= 16.  stack = 0: feat[.][0, 8) = leaky(a) +
 *   leaky(b), CT >= 8.  signs (uint16 [N H W], optional: written only when non-NULL): bit c = (a_c > 0), bit 8 + c = (b_c > 0).
 *   Every other channel of feat is left as it is.
 * dmc_ef_layer: feat[.][K, K + R) = leaky_0.1(conv3x3(feat[.][0, K)) + bias[R]) in place, feat[.][K + R, K + round_up4(R)) = +0.0.
 *   Reads only channels < K, writes only its slot.
 * dmc_ef_head: out NCHW [N][2][H][W] = conv3x3(feat[.][0, K)) + bias[2], w [2][9][K]; feat is read only.
 * dmc_ef_head_dgrad: G[m][c] = sum_t sum_co dout[m - o(t)][co] w[co][t][c] for c < K and 0 for K <= c < CT (dout NCHW
 *   [N][2][H][W]): writes EVERY float of G.
 * dmc_ef_head_wgrad: dw [2][9][K] = sum_m dout[m][co] feat[m + o(t)][c], db [2] = sum_m dout[m][co].
 * dmc_ef_layer_mask: G[.][K + r] <- feat[.][K + r] > 0 ? g : 0.1f * g in place for r < round_up4(R), db [R] = the sums of the
 *   result over the pixels.  Every other channel of G is left as it is; feat is read only.
 * dmc_ef_layer_wgrad: dw [R][9][K] = sum_m G[m][K + r] feat[m + o(t)][c].  Reads feat channels [0, K) and G channels
 *   [K, K + round_up4(R)) only.
 * dmc_ef_layer_dgrad: G[m][c] += sum_t sum_r G[m - o(t)][K + r] w[r][t][c] in place for c < K.  Reads channels
 *   [K, K + round_up4(R)) (the gathered slot), reads and writes channels < K of the lane's own pixel: disjoint byte sets.
 * dmc_ef_first_bwd: from G's base slot, x and the branch of each LeakyReLU -- stack = 0: both from `signs` (feat may be NULL),
 *   ga_c = G[.][c] * (bit c ? 1 : 0.1f), gb_c = G[.][c] * (bit 8 + c ? 1 : 0.1f); stack = 1: from the stored activations (signs may
 *   be NULL), ga_c = G[.][c] * (feat[.][c] > 0 ? 1 : 0.1f), gb_c = G[.][8 + c] * (feat[.][8 + c] > 0 ? 1 : 0.1f) -- dw_mv [8][2][3][3] =
 *   sum_m ga_c[m] x[m + o(t)][i], db_mv [8] = sum_m ga_c[m], dw_r [8][3][3][3] and db_r [8] the same of gb and x[:, 2:].  No gradient
 *   with respect to x is produced.
 * Every sum over pixels is formed as fp32 fmaf runs of at most 1024 pixels in order; the runs' partial sums are added in run
 *   order.  Plain fp32 FMAs in a fixed order throughout: deterministic, no atomics, a forward result independent of the batch
 *   its frame is in; the caller owns every buffer; nothing allocates or synchronises; inputs are read only.
 * DMC_E_INVALID before any launch (nothing written): a NULL required pointer, an unsupported shape. */
int dmc_ef_supported(int N, int H, int W, int CT, int K, int R);
size_t dmc_ef_head_wgrad_workspace_bytes(int N, int H, int W, int K);
size_t dmc_ef_layer_wgrad_workspace_bytes(int N, int H, int W, int K, int R);
size_t dmc_ef_layer_mask_workspace_bytes(int N, int H, int W, int R);
size_t dmc_ef_first_bwd_workspace_bytes(int N, int H, int W);
int dmc_ef_first(const float* x_nchw, const float* w_mv, const float* b_mv, const float* w_r, const float* b_r, float* feat,
                 unsigned short* signs, int N, int H, int W, int CT, int stack, dmc_stream_t stream);
int dmc_ef_layer(float* feat, const float* w, const float* bias, int N, int H, int W, int CT, int K, int R, dmc_stream_t stream);
int dmc_ef_head(const float* feat, const float* w, const float* bias, float* out_nchw, int N, int H, int W, int CT, int K,
                dmc_stream_t stream);
int dmc_ef_head_dgrad(const float* dout_nchw, const float* w, float* G, int N, int H, int W, int CT, int K, dmc_stream_t stream);
int dmc_ef_head_wgrad(const float* dout_nchw, const float* feat, float* dw, float* db, void* workspace, int N, int H, int W, int CT,
                      int K, dmc_stream_t stream);
int dmc_ef_layer_mask(const float* feat, float* G, float* db, void* workspace, int N, int H, int W, int CT, int K, int R,
                      dmc_stream_t stream);
int dmc_ef_layer_wgrad(const float* feat, const float* G, float* dw, void* workspace, int N, int H, int W, int CT, int K, int R,
                       dmc_stream_t stream);
int dmc_ef_layer_dgrad(float* G, const float* w, int N, int H, int W, int CT, int K, int R, dmc_stream_t stream);
int dmc_ef_first_bwd(const float* G, const float* x_nchw, const unsigned short* signs, const float* feat, float* dw_mv, float* db_mv,
                     float* dw_r, float* db_r, void* workspace, int N, int H, int W, int CT, int stack, dmc_stream_t stream);

/* ---- Discriminator4's 8 -> 16 block (disc_c8.hip) ---------------------------------------------------------------
 * Replaces: the Conv2d(8, 16, 3, stride 2, padding 1) of `discriminator_block(8, 16)`, code/dmcnet_GAN/model.py:254-265 as
 *           instantiated at :369-385, with its LeakyReLU(0.2) and Dropout2d keep mask, and its autograd.
 * Layouts:  x [N][H][W][8], z and g [N][OH][OW][16] fp32 NHWC (channels_last memory), OH = (H - 1) / 2 + 1, OW alike; w and dw OHWI
 *           [16][3][3][8] (the channels_last memory of the PyTorch weight).
 * dmc_disc_c8_supported: even H and W (odd sizes are refused), every tensor below 2^31 bytes.
 * fwd:   z = conv(x, w) [+ bias] [LeakyReLU(0.2) if act == 1] [* keep[n][co], the [N][16] Dropout2d mask already divided by 1 - p] --
 *        the epilogue of dmc_conv_nhwc_fwd -- and, if stat_partials != NULL, the per-channel (sum, sum of squares) of z per
 *        workgroup in fp64, [stat_blocks = dmc_disc_c8_stat_blocks()][16][2], which dmc_conv_nhwc_stats_final() consumes as they
 *        are; another stat_blocks is refused, nothing is written.
 * dgrad: dx [N][H][W][8] = conv_transpose(g, w); every element is written.
 * wgrad: dw = sum over output pixels, db [16] (nullable) = the channel sums of g: partial sums over runs of 512 consecutive
 *        output pixels ([runs][1168] floats in the workspace of dmc_disc_c8_wgrad_bytes(), whose contents on entry do not matter),
 *        added in run order.
 * Plain fp32 fmaf in a fixed order (72 products per output), no atomics: results are bit-identical from run to run.  The caller
 * owns every buffer; nothing allocates or synchronises; inputs are read only.
 * DMC_E_INVALID before any launch (nothing written): a NULL required pointer (bias, keep, stat_partials and db are optional), an
 * unsupported shape, a stat_blocks that is not the grid's. */
int dmc_disc_c8_supported(int N, int H, int W);
int dmc_disc_c8_stat_blocks(int N, int H, int W);
int dmc_disc_c8_fwd(const float* x, const float* w, const float* bias, const float* keep, float* z, double* stat_partials,
                    int stat_blocks, int N, int H, int W, int act, dmc_stream_t stream);
int dmc_disc_c8_dgrad(const float* g, const float* w, float* dx, int N, int H, int W, dmc_stream_t stream);
size_t dmc_disc_c8_wgrad_bytes(int N, int H, int W);
int dmc_disc_c8_wgrad(const float* x, const float* g, float* dw, float* db, void* workspace, int N, int H, int W,
                      dmc_stream_t stream);

/* ---- The discriminators' head on the NHWC activation (disc_head.hip) --------------------------------------------
 * Replaces: adv_layer = nn.Linear(C * H * W, 2) on `out.view(out.shape[0], -1)`, code/dmcnet_GAN/model.py:290,297-298, and its
 *           autograd, without the NHWC -> NCHW copy of the activation and without a permuted copy of the weight.
 * Layouts:  x and dx [M][H][W][C] fp32 (channels_last memory); weight and dweight [2][C * H * W] in the reference's (c, h, w)
 *           column order; bias, dbias [2]; validity, dvalidity [M][2].
 * dmc_disc_head_supported: C a multiple of 16, M * C * H * W < 2^31.
 * fwd: validity[m][j] = bias[j] + sum x[m][h][w][c] * weight[j][c * H * W + h * W + w], one launch, one workgroup per frame: fp32
 *      fmaf sums per lane, added over lanes and waves in a fixed order, bias last.
 * bwd: dx = dvalidity[m][0] * weight[0] + dvalidity[m][1] * weight[1]; dweight = sum over the frames of dvalidity[m][j] * x[m];
 *      dbias = sum over the frames of dvalidity.  Each of dx, dweight, dbias may be NULL (not all three): a dx-only call reads
 *      neither x nor the workspace (both may be NULL), a call without dx does not read weight (may be NULL).  dweight is summed
 *      over slices of 16 frames ([slices][2][C * H * W] floats in the workspace of dmc_disc_head_bwd_bytes(), whose contents on
 *      entry do not matter) and the slices in order; dbias in a fixed order.
 * No atomics: results are bit-identical from run to run.  The caller owns every buffer; nothing allocates or synchronises; inputs
 * are read only.  DMC_E_INVALID before any launch (nothing written): a NULL required pointer, an unsupported shape. */
int dmc_disc_head_supported(int M, int C, int H, int W);
int dmc_disc_head_fwd(const float* x, const float* weight, const float* bias, float* validity, int M, int C, int H, int W,
                      dmc_stream_t stream);
size_t dmc_disc_head_bwd_bytes(int M, int C, int H, int W);
int dmc_disc_head_bwd(const float* x, const float* weight, const float* dvalidity, float* dx, float* dweight, float* dbias,
                      void* workspace, int M, int C, int H, int W, dmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DMCNET_HIP_H */
