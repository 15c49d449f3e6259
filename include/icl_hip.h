/* icl_hip.h — C ABI of libicl_hip.so, the gfx950 (MI355X) kernels behind the ICL hot path.
 *
 * The reference (zhuye98/ICL) is pure PyTorch and has no FFI of its own; each entry point below
 * replaces the ATen operator the reference dispatches at the cited call site
 * (paths relative to /root/reference/code).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 (unless typed otherwise) owned by the caller;
 *    the library allocates nothing and keeps no state; `ws` arguments are caller-provided scratch
 *    whose size comes from the matching *_ws_bytes() query;
 *  - tensors are dense NC[D]HW unless a batch stride (in elements) is given;
 *  - `stream` is a hipStream_t; launches are asynchronous on it, no device synchronisation inside;
 *  - return 0 on success, a negative code on error (-1 bad argument, -2 launch failure);
 *    icl_last_error() returns a thread-local message.  Nothing throws across the boundary.
 */
#ifndef ICL_HIP_H
#define ICL_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int icl_abi_version(void);
const char* icl_last_error(void);
/* name of the convolution kernel instantiation picked by the most recent icl_conv3d_* call on this thread (profiling aid) */
const char* icl_last_kernel_name(void);
/* For the tests (per thread): which kernel(s) the last pooling / resize / depth-to-space launcher chose (kernels/pool_resize.h).  The
 * kernel's name; icl_upsample2x_concat_norm "<skip copy>|<deep resize>"; the three-pass icl_trilinear_bwd "x:<k>|y:<k>|z:<k>";
 * icl_depth_to_space2 / icl_space_to_depth2 the name + "+big_lds" when the launch raised the dynamic-LDS limit, "+lds" otherwise. */
const char* icl_last_resample_route(void);

/* ---- Conv3d k=3 pad=1 / k=1, stride 1 (networks/utils.py:104,107; networks/unet_3D_icl.py:65,178,196,327).
 * Weights are used in packed form Wp[taps][KP][NP]: mode 0 (forward) K=Cin,N=Cout; mode 1 (dgrad) K=Cout,N=Cin
 * with taps flipped.  KP = round_up(K,4), NP = round_up(N,16). */
int64_t icl_conv3d_packed_elems(int cout, int cin, int ks, int mode);
int icl_conv3d_pack_weights(const float* w, float* wp, int cout, int cin, int ks, int mode, void* stream);
/* both packings (mode 0 into wp_fwd, mode 1 into wp_dgrad) in one launch — a training step needs both of every weight */
int icl_conv3d_pack_weights_both(const float* w, float* wp_fwd, float* wp_dgrad, int cout, int cin, int ks, void* stream);
/* Both packings of `count` weights in one launch per 32 weights (arrays of device pointers and of Cout / Cin / kernel size): the
 * trainer packs every convolution weight of the model once per step (they only change in the optimiser), not once per call. */
int icl_conv3d_pack_weights_multi(const void* const* w, void* const* wp_fwd, void* const* wp_dgrad, const int32_t* cout, const int32_t* cin,
                                  const int32_t* ks, int count, void* stream);
/* y[n, 0:cout] = conv(x[n, 0:cin], Wp) + bias (bias may be NULL).  dgrad: call with Wp packed in mode 1,
 * x = dY, cin/cout swapped, bias NULL.  Batch strides in elements; channel stride is D*H*W.
 * ws: icl_conv3d_fwd_ws_bytes(...) bytes (0 for most shapes): launches with too few output tiles to fill the chip
 * split their Cin range over workgroups, each split writes a partial-output slab there and a fixed-order reduction adds
 * them (bitwise reproducible); ws may be NULL, the launch then runs unsplit.
 * Arithmetic: fp32 operands, fp32 accumulation, fp32 result.  3x3x3 layers with Cin % 16 == 0, W % 4 == 0 and >= 24^3 voxels
 * form their products on the bf16 matrix pipe from exact three-way bf16 splits of both operands (six MFMA terms per product,
 * csrc/kernels/conv_bf16x3.h).  Accuracy, measured against fp64: the OUTPUTS are as close as those of
 * v_mfma_f32_16x16x4_f32 (mean |error| 2.3e-7 vs 3.2e-7 relative), but v_mfma_f32_16x16x32_bf16 does not round its 32-product
 * partial sums to nearest: sums of same-sign products carry a coherent offset of -0.36 * 2^-24 (relative) that the fp32 kernels do
 * not have.  Logits, maps, losses, gradient norms and every compared gradient are unaffected: on the most cancellation-heavy tensor of the
 * step (the sampled 13,824^2 mlp2 gradient) the two paths differ by 1.2e-3 while the quantity itself is only defined to 1.6e-2 (an input
 * perturbation of 1e-7 moves it that far on the fp32 kernels; round 4, profiles/r4_mlp2_grad_sensitivity.txt).  The split weights live in
 * ws (counted by icl_conv3d_fwd_ws_bytes; without ws the fp32 MFMA kernels run).  Environment: ICL_CONV_SPLIT=0 selects the fp32
 * MFMA kernels for every shape.  icl_conv3d_fwd_ws_bytes and the other shape queries below (_presplit_ws_bytes, _stats_slots, _live_ok)
 * read the launcher's plan — a function of the shape and the environment switches alone — and launch nothing. */
int64_t icl_conv3d_fwd_ws_bytes(int n, int cin, int cout, int d, int h, int w, int ks);
/* Split-product convolution with the weight split hoisted out of the call (the weights only change in the optimiser step):
 * icl_conv3d_split_weights_multi turns up to `count` packed weights wp[i] (icl_conv3d_pack_weights, mode 0 or 1; Cin % 16 == 0) into
 * their three bf16 planes wsplit[i] (icl_conv3d_split_ws_bytes(cin, cout) bytes each, 16-byte aligned; 0 = not eligible) in ONE
 * launch; icl_conv3d_fwd_presplit is icl_conv3d_fwd on such planes.  It returns 1 — nothing launched — when the shape does not run on
 * the split-product kernel (volume below 24^3, W % 4 != 0, ICL_CONV_SPLIT=0): the caller then uses icl_conv3d_fwd with the fp32 pack. */
int64_t icl_conv3d_split_ws_bytes(int cin, int cout);
int icl_conv3d_split_weights_multi(const void* const* wp, void* const* wsplit, const int32_t* cin, const int32_t* cout, int count,
                                   void* stream);
int icl_conv3d_fwd_presplit(const float* x, const void* wsplit, const float* bias, float* y, int n, int cin, int cout, int d, int h, int w,
                            int64_t x_bstride, int64_t y_bstride, void* stream);
/* Round 6: the deep levels (rows of 12 or 24 voxels: 18 / 72 output tiles for a batch of two) fill the chip by splitting the channel
 * chunks of a tile over workgroups; every slice writes raw partial sums into a slab of ws and a fixed-order reduction adds them (+ bias)
 * into y — bitwise reproducible.  icl_conv3d_fwd_presplit_ws_bytes: the bytes of ws the launcher's plan needs for this shape (0: the
 * launch is not split; icl_conv3d_fwd_presplit does the same work).  icl_conv3d_fwd_presplit_ws = icl_conv3d_fwd_presplit with that
 * workspace; the 12^3 level (4 x 4 x 12 tiles, Cout % 32 == 0) runs on the split-product kernel only through it.  A split launch hands no
 * statistics to the normalisation (icl_conv3d_fwd_stats_slots returns 0 for such shapes).  Reference: nn.Conv3d of UnetConv3 at the
 * conv3 / conv4 / up_concat4 / up_concat3 levels (/root/reference/code/networks/unet_3D.py:41-47,53-54, networks/utils.py:104,107) and
 * its input gradient.  Environment: ICL_CONV_SPLIT_KSPLIT=0 never splits (the 12^3 level then stays on the fp32 MFMA kernels). */
int64_t icl_conv3d_fwd_presplit_ws_bytes(int n, int cin, int cout, int d, int h, int w);
int icl_conv3d_fwd_presplit_ws(const float* x, const void* wsplit, const float* bias, float* y, void* ws, int n, int cin, int cout, int d,
                               int h, int w, int64_t x_bstride, int64_t y_bstride, void* stream);
/* Convolution + the InstanceNorm statistics of its output from the epilogue's registers (reference: Conv3d -> InstanceNorm3d,
 * /root/reference/code/networks/utils.py:104-105, :107-108) — the stand-alone statistics pass of icl_norm_fwd re-reads the whole output.
 * icl_conv3d_fwd_stats_slots: the number of (count, mean, M2) summaries per (sample, channel) the launch will write (= its workgroup
 * count), or 0 when the shape cannot produce them (not on the split-product kernel, or a workgroup's tile list would span two samples):
 * the caller then runs icl_conv3d_fwd_presplit + icl_norm_fwd.  stats: n * cout * slots * 3 floats, every element written.
 * icl_conv3d_fwd_presplit_stats returns 1 — nothing launched — under the same conditions as icl_conv3d_fwd_presplit. */
int icl_conv3d_fwd_stats_slots(int n, int cin, int cout, int d, int h, int w);
int icl_conv3d_fwd_presplit_stats(const float* x, const void* wsplit, const float* bias, float* y, float* stats, int n, int cin, int cout,
                                  int d, int h, int w, int64_t x_bstride, int64_t y_bstride, void* stream);
int icl_conv3d_fwd(const float* x, const float* wp, const float* bias, float* y, void* ws, int n, int cin, int cout, int d, int h,
                   int w, int ks, int64_t x_bstride, int64_t y_bstride, void* stream);
/* gw[cout][cin][taps] = sum over batch and voxels; ws >= icl_conv3d_wgrad_ws_bytes(n,cin,cout,ks) bytes (one packed
 * partial-sum slab per workgroup row, reduced in a fixed order: bitwise reproducible).  gbias (may be NULL) [cout] = sum of gy. */
int64_t icl_conv3d_wgrad_ws_bytes(int n, int cin, int cout, int ks);
int icl_conv3d_wgrad(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int cin, int cout, int d,
                     int h, int w, int ks, int64_t x_bstride, int64_t gy_bstride, void* stream);
/* The two halves of icl_conv3d_wgrad apart (round 6): `_slabs` runs the weight-gradient kernel only and leaves its per-workgroup partial
 * sums in ws (*nslabs of them); `_reduce_multi` sums the slabs of up to any number of such calls (HOST arrays of `count` entries) into
 * their [Cout, Cin, k, k, k] gradients in ONE launch, each in the order icl_conv3d_wgrad uses (bit-identical).  The weight gradient is
 * a leaf of the backward pass (only the optimiser reads it, utils.py:104-107 / trainer :113-115), so a step scope queues the sums and
 * runs them once at the end of backward (ops.DeferredWgradReduce) instead of one small launch behind each of 23 weight-gradient kernels. */
int icl_conv3d_wgrad_slabs(const float* x, const float* gy, void* ws, int n, int cin, int cout, int d, int h, int w, int ks,
                           int64_t x_bstride, int64_t gy_bstride, int32_t* nslabs, void* stream);
int icl_conv3d_wgrad_reduce_multi(const void* const* ws, void* const* gw, const int32_t* cout, const int32_t* cin, const int32_t* ks,
                                  const int32_t* nslabs, int count, void* stream);

/* ---- Live batch: the backward of the upper decoder on a gradient whose samples [n_live, n) are exactly zero.  The unlabeled stream's
 * logits enter the loss only as a detached target (`de_predicts = predicts.clone().detach()`, /root/reference/code/utils/losses.py:294), so
 * the gradient of the batch split has a zero second half and every operator from `final` down to the skip gradients of conv1 / conv2 and
 * the decoder share of up3's gradient (unet_3D_icl.py:113-117, networks/utils.py:104-109,264,271-276) — all of them per sample — maps it
 * to zeros.  A `_live` sibling takes n and n_live: samples [0, n_live) are computed exactly as the entry point computes them for
 * n = n_live on the same pointers and batch strides; samples [n_live, n) of every output GRADIENT (dense [n][...] tensors) are written as
 * zeros by the same call on the same stream (a fill node under graph capture) — nothing ever reads an unwritten tail.  Weight / bias
 * gradients have no per-sample output: their live form keeps the launch plan of the batch of n — the tile-list kernels launch only the
 * workgroups that own a live tile and write the other slabs as zeros, everything else runs the whole batch — so the sums are bit for bit
 * those of the entry point called with n (workspaces as for n).  n_live == n is the entry point itself.
 * 3x3x3 (and 1x1x1) input gradient = the forward entry points on the transposed pack (utils.py:104,107): */
/* icl_conv3d_fwd_live_ok: 1 when the planner plans the 3x3x3 product for a batch of n_live exactly as for a batch of n (split-product
 * kernels, no split over the channel chunks), so that the live samples equal the full call's bit for bit; 0: run the full batch. */
int icl_conv3d_fwd_live_ok(int n, int n_live, int cin, int cout, int d, int h, int w);
/* For the tests (per thread, like icl_last_kernel_name): the kernel of the last live input-gradient launch, and the workgroups the last
 * tile-list weight-gradient launch started / its plan holds (started < planned: a live batch skipped the workgroups without a live tile). */
const char* icl_last_live_fwd_kernel_name(void);
void icl_last_wgrad_grid(int32_t* launched, int32_t* planned);
int icl_conv3d_fwd_presplit_live(const float* x, const void* wsplit, const float* bias, float* y, int n, int n_live, int cin, int cout, int d,
                                 int h, int w, int64_t x_bstride, int64_t y_bstride, void* stream);
int icl_conv3d_fwd_presplit_ws_live(const float* x, const void* wsplit, const float* bias, float* y, void* ws, int n, int n_live, int cin,
                                    int cout, int d, int h, int w, int64_t x_bstride, int64_t y_bstride, void* stream);
int icl_conv3d_fwd_live(const float* x, const float* wp, const float* bias, float* y, void* ws, int n, int n_live, int cin, int cout, int d,
                        int h, int w, int ks, int64_t x_bstride, int64_t y_bstride, void* stream);
/* weight gradient (utils.py:104,107; with x and gy exchanged: up_concat1.conv1, 48 -> 16).  The workspace queries of the forward forms
 * (icl_conv3d_fwd_ws_bytes, icl_conv3d_fwd_presplit_ws_bytes) are asked with n = n_live. */
int64_t icl_conv3d_wgrad_ws_bytes_live(int n, int n_live, int cin, int cout, int ks);
int icl_conv3d_wgrad_live(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int n_live, int cin, int cout, int d,
                          int h, int w, int ks, int64_t x_bstride, int64_t gy_bstride, void* stream);
int icl_conv3d_wgrad_slabs_live(const float* x, const float* gy, void* ws, int n, int n_live, int cin, int cout, int d, int h, int w, int ks,
                                int64_t x_bstride, int64_t gy_bstride, int32_t* nslabs, void* stream);

/* ---- InstanceNorm3d(+ReLU) (networks/utils.py:105-106,108-109) and BatchNorm3d(+ReLU)
 * (networks/unet_3D_icl.py:325-340).  mode 0 = instance (group = (n,c)), 1 = batch (group = c).
 * use_batch_stats 0 = normalise with the given mean/rstd... (eval-mode BatchNorm: mean=running_mean,
 * rstd computed from running_var by icl_rstd_from_var).  act 0 none / 1 ReLU / 2 LeakyReLU(0.01).  gamma/beta/running_* may be NULL. */
int64_t icl_norm_ws_bytes(int n, int c, int64_t s);
int icl_norm_fwd(const float* x, float* y, float* mean, float* rstd, const float* gamma, const float* beta,
                 float* running_mean, float* running_var, int n, int c, int64_t s, int mode, int use_batch_stats,
                 int act, float eps, float momentum, void* ws, void* stream);
int icl_norm_bwd(const float* gy, const float* x, const float* mean, const float* rstd, const float* gamma,
                 const float* beta, float* gx, float* dgamma, float* dbeta, int n, int c, int64_t s, int mode,
                 int use_batch_stats, int act, void* ws, void* stream);
/* live batch (see icl_conv3d_fwd_presplit_live): InstanceNorm3d + ReLU backward of UnetConv3 (utils.py:105-106,108-109) on samples
 * [0, n_live), zeros to the rest of gx.  mode 0 without an affine pair only (a batch group couples the samples). */
int icl_norm_bwd_live(const float* gy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* gx,
                      float* dgamma, float* dbeta, int n, int n_live, int c, int64_t s, int mode, int use_batch_stats, int act, void* ws,
                      void* stream);
/* Same, with a residual branch: y = act(norm(x) + res) and, backward, gres = act'(.) * gy next to gx.  This is the tail of
 * MONAI 1.0.1 UnetResBlock.forward ("out = norm2(conv2(.)); out += residual; out = lrelu(out)") used by every encoder/decoder
 * block of SwinUNETR (networks/swinunetr_icl.py:123-223).  res / gres may be NULL (then identical to icl_norm_fwd/_bwd). */
/* icl_norm_res_fwd with batch statistics taken from `part` — nslots (count, mean, M2) summaries per (sample, channel) row, layout
 * part[(row * nslots + slot) * 3], as icl_conv3d_fwd_presplit_stats writes them — instead of a statistics pass over x. */
int icl_norm_fwd_given_stats(const float* x, const float* res, float* y, float* mean, float* rstd, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, int n, int c, int64_t s, int mode, int act, float eps,
                             float momentum, const float* part, int nslots, void* stream);
int icl_norm_res_fwd(const float* x, const float* res, float* y, float* mean, float* rstd, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, int n, int c, int64_t s, int mode, int use_batch_stats,
                     int act, float eps, float momentum, void* ws, void* stream);
int icl_norm_res_bwd(const float* gy, const float* x, const float* res, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, float* gx, float* gres, float* dgamma, float* dbeta, int n, int c, int64_t s, int mode,
                     int use_batch_stats, int act, void* ws, void* stream);
int icl_rstd_from_var(const float* var, float* rstd, int c, float eps, void* stream);

/* ---- Deferred InstanceNorm3d + ReLU (round 5).  Reference: Conv3d -> InstanceNorm3d -> ReLU in UnetConv3
 * (/root/reference/code/networks/utils.py:107-109) whose output feeds MaxPool3d / the skip concatenation / nn.Upsample / the `final`
 * convolution (unet_3D_icl.py:41-53,116-117, utils.py:264,276).  The convolution stores its RAW output and (count, mean, M2) summaries
 * (icl_conv3d_fwd_presplit_stats); icl_norm_finalize_stats turns them into mean / rstd (for icl_norm_bwd) and the per-(sample, channel)
 * pair ss = (scale, shift) = (rstd, -mean * rstd); the consumers below apply relu(fma(x, scale, shift)) while they load x, so the
 * normalised tensor is never written.  ss: [n * c][2] floats. */
int icl_norm_finalize_stats(const float* part, int n, int c, int nslots, float eps, float* mean, float* rstd, float* ss, void* stream);
/* y = relu(fma(x, scale, shift)) written out (a consumer that cannot apply the deferred normalisation on load); s % 4 == 0 */
int icl_norm_apply(const float* x, const float* ss, float* y, int n, int c, int64_t s, void* stream);
/* MaxPool3d(2) of the normalised tensor from the raw one (values and argmax of relu(fma(x, scale, shift))) */
int icl_maxpool2_fwd_norm(const float* x, const float* ss, float* y, uint8_t* idx, int64_t nc, int dout, int hout, int wout, int pool_depth,
                          void* stream);
/* out = cat([skip, upsample2x(deep)], 1) (utils.py:264,276): skip [n, cs, d, h, w], deep [n, cd, d/2, h/2, w/2], out [n, cs + cd, d, h, w];
 * skip_ss / deep_ss: that source is raw with deferred normalisation (NULL: used as stored).  d, h even, w % 4 == 0. */
int icl_upsample2x_concat_norm(const float* skip, const float* skip_ss, const float* deep, const float* deep_ss, float* out, int n, int cs,
                               int cd, int d, int h, int w, void* stream);

/* ---- MaxPool3d(2) (networks/unet_3D_icl.py:41-53) and MaxPool2d(2) (networks/unet_icl.py:64, pool_depth = 1 on a
 * D = 1 volume); idx = uint8 argmax within the pool_depth x 2 x 2 window. */
int icl_maxpool2_fwd(const float* x, float* y, uint8_t* idx, int64_t nc, int dout, int hout, int wout, int pool_depth, void* stream);
int icl_maxpool2_bwd(const float* gy, const uint8_t* idx, float* gx, int64_t nc, int dout, int hout, int wout, int pool_depth, void* stream);
/* gx = add + maxpool2 backward of gy: the gradient of a tensor that feeds both a max-pool and a skip connection
 * (/root/reference/code/networks/unet_3D_icl.py:100-116) in one pass.  add: [n][c] planes of the un-pooled extent, batches add_bstride
 * elements apart (a channel slice of the concat gradient). */
int icl_maxpool2_bwd_add(const float* gy, const uint8_t* idx, const float* add, float* gx, int n, int c, int dout, int hout, int wout,
                         int pool_depth, int64_t add_bstride, void* stream);
/* the same where the skip gradient carries a live batch (unet_3D_icl.py:100-101,113-116: the skip gradients of conv1 / conv2 come from
 * the upper decoder): samples >= skip_live take the pooling gradient alone and issue no load of `add` (its bytes there are zeros).  The
 * pooling gradient gy is a full batch; so is gx.  Bit-identical to icl_maxpool2_bwd_add on an addend with a zero tail. */
int icl_maxpool2_bwd_add_live(const float* gy, const uint8_t* idx, const float* add, float* gx, int n, int skip_live, int c, int dout, int hout,
                              int wout, int pool_depth, int64_t add_bstride, void* stream);

/* ---- trilinear / bilinear (D = 1) resize (networks/utils.py:264; networks/unet_icl.py:84-85; utils/losses.py:245,263,281,292).
 * align_corners=0: source scale in/out (what ATen uses for size= and for scale_factor=2); 1: (in-1)/(out-1). */
int icl_trilinear_fwd(const float* x, float* y, int n, int c, int di, int hi, int wi, int dout, int hout, int wout,
                      int64_t y_bstride, int align_corners, void* stream);
/* backward = three separable one-axis gathers (x, y, z); ws >= icl_trilinear_bwd_ws_bytes(...) */
int64_t icl_trilinear_bwd_ws_bytes(int n, int c, int di, int hi, int wi, int dout, int hout, int wout);
int icl_trilinear_bwd(const float* gy, float* gx, void* ws, int n, int c, int di, int hi, int wi, int dout, int hout, int wout,
                      int64_t gy_bstride, int align_corners, void* stream);
/* live batch (see icl_conv3d_fwd_presplit_live): the backward of nn.Upsample(scale_factor=2) in UnetUp3_CT (utils.py:264,271-276) on
 * samples [0, n_live) of gy, zeros to the rest of gx (dense); ws as for n = n_live. */
int icl_trilinear_bwd_live(const float* gy, float* gx, void* ws, int n, int n_live, int c, int di, int hi, int wi, int dout, int hout, int wout,
                           int64_t gy_bstride, int align_corners, void* stream);

/* ---- strided row copy (torch.cat([skip, up], 1), networks/utils.py:276) */
int icl_copy_rows(const float* src, float* dst, int64_t rows, int64_t row_elems, int64_t src_stride, int64_t dst_stride,
                  void* stream);

/* ---- out = [a ; b] of na + nb floats (multiples of 4, 16-byte aligned); a NULL half is written as zeros.  The gradient of the batch
 * split of the ICL forward (train_inherent_consistent_unet_3D_BraTS.py:103-104 slices outputs[:labeled_bs] / [labeled_bs:]; the unlabeled
 * half of the features alone feeds uscl, unet_3D_icl.py:124-131) in one launch. */
int icl_concat2(const float* a, int64_t na, const float* b, int64_t nb, float* out, void* stream);

/* ---- depthwise Conv3d k=3 pad=1 groups=C, no bias (networks/unet_3D_icl.py:320-323).
 * w is [C][27]; flip=1 applies the transposed stencil (input gradient). gw [C][27] is overwritten (per-chunk partial sums in `ws`,
 * icl_dwconv3_wgrad_ws_bytes, added in a fixed order). */
int icl_dwconv3_fwd(const float* x, const float* w, float* y, int n, int c, int d, int h, int wd, int flip, void* stream);
int64_t icl_dwconv3_wgrad_ws_bytes(int n, int c, int d, int h, int wd);
int icl_dwconv3_wgrad(const float* x, const float* gy, float* gw, void* ws, int n, int c, int d, int h, int wd, void* stream);

/* ---- 1x1x1 Conv3d with a handful of channels on a small volume (SeparableConv3d.pointwise and attn_convs1 of the aligner,
 * networks/unet_3D_icl.py:196,327): y[b][o][v] = bias[o] + sum_i w[o * w_ostride + i * w_istride] * x[b][i][v], x [n, cin, s],
 * y [n, cout, s], s % 4 == 0, bias may be NULL.  The input gradient is the same call with the strides swapped. */
int icl_conv1x1_small(const float* x, const float* w, const float* bias, float* y, int n, int cin, int cout, int64_t s, int w_ostride,
                      int w_istride, void* stream);
/* the same with nn.Dropout(p) folded in (the mask of icl_dropout, same seed protocol; unet_3D_icl.py:67-68,117: `final(dropout2(up1))`):
 * mask_mode 1: the INPUT is the dropped tensor (forward); 2: the OUTPUT is (the pair's input gradient).  Returns 1 (nothing launched) for
 * n * s < 65536: run icl_dropout and icl_conv1x1_small then.  icl_conv1x1_wgrad_dropout: the pair's weight gradient from the un-dropped x. */
int icl_conv1x1_dropout(const float* x, const float* w, const float* bias, float* y, int n, int cin, int cout, int64_t s, int w_ostride,
                        int w_istride, int mask_mode, uint32_t seed, float p, const uint32_t* seed_dev, void* stream);
int icl_conv1x1_wgrad_dropout(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int cin, int cout, int64_t s,
                              int64_t gy_bstride, uint32_t seed, float p, const uint32_t* seed_dev, void* stream);
/* the same pair with x given raw + ss (deferred InstanceNorm + ReLU of `up1`, then dropout2, then `final`; p = 0: no mask): forward
 * (n * s >= 65536) and weight gradient; the input gradient is icl_conv1x1_dropout(mask_mode 2) as before. */
int icl_conv1x1_dropout_norm(const float* x, const float* ss, const float* w, const float* bias, float* y, int n, int cin, int cout, int64_t s,
                             int w_ostride, int w_istride, uint32_t seed, float p, const uint32_t* seed_dev, void* stream);
int icl_conv1x1_wgrad_dropout_norm(const float* x, const float* ss, const float* gy, float* gw, float* gbias, void* ws, int n, int cin,
                                   int cout, int64_t s, int64_t gy_bstride, uint32_t seed, float p, const uint32_t* seed_dev, void* stream);
/* live batch (see icl_conv3d_fwd_presplit_live) of the `final` layer's backward (unet_3D_icl.py:116-117): input gradients with a zeroed
 * tail, weight / bias gradients over samples [0, n_live).  The dropout mask hashes the element index (b * C + c) * S + v; the live samples
 * are a prefix, so their masks are those of the full batch.  The two input-gradient forms choose their kernel by the FULL batch (the
 * big-volume kernel from n * s = 65536 on): the live samples are bit for bit those of the full call; icl_conv1x1_dropout_live returns 1
 * (nothing launched, nothing zeroed) for n * s < 65536.  The weight / bias gradient forms run the whole batch (workspaces as for n). */
int icl_conv1x1_small_live(const float* x, const float* w, const float* bias, float* y, int n, int n_live, int cin, int cout, int64_t s,
                           int w_ostride, int w_istride, void* stream);
int icl_conv1x1_dropout_live(const float* x, const float* w, const float* bias, float* y, int n, int n_live, int cin, int cout, int64_t s,
                             int w_ostride, int w_istride, int mask_mode, uint32_t seed, float p, const uint32_t* seed_dev, void* stream);
int icl_conv1x1_wgrad_dropout_live(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int n_live, int cin, int cout,
                                   int64_t s, int64_t gy_bstride, uint32_t seed, float p, const uint32_t* seed_dev, void* stream);
int icl_conv1x1_wgrad_dropout_norm_live(const float* x, const float* ss, const float* gy, float* gw, float* gbias, void* ws, int n, int n_live,
                                        int cin, int cout, int64_t s, int64_t gy_bstride, uint32_t seed, float p, const uint32_t* seed_dev,
                                        void* stream);

/* ---- nn.Dropout(p) (networks/unet_3D_icl.py:67-68,110,116): y = keep ? x/(1-p) : 0 with a counter-based
 * mask keyed by (seed, element index); calling it again with the same seed on dY is the backward.  seed_dev (may be
 * NULL) is a device-resident counter folded into the seed so that replays of a captured hipGraph draw fresh masks. */
int icl_dropout(const float* x, float* y, int64_t n, uint32_t seed, float p, const uint32_t* seed_dev, void* stream);
/* DropPath / stochastic depth (timm, MONAI; networks/unet_3D_icl.py:253, swinunet_icl.py:215): one keep/drop decision per `group`
 * consecutive elements (group = elements per sample), kept samples scaled by 1/(1-p).  Same counter-based mask as icl_dropout. */
int icl_drop_path(const float* x, float* y, int64_t n, int64_t group, uint32_t seed, float p, const uint32_t* seed_dev, void* stream);
/* y = res + DropPath(x): the residual update  x + drop_path(branch)  of the Class_Decoder / Swin blocks (unet_3D_icl.py:262-267,
 * swinunetr_icl.py:871-884) in one pass; res may be NULL (plain icl_drop_path) or alias x (x + drop_path(x), :263). */
int icl_drop_path_add(const float* x, const float* res, float* y, int64_t n, int64_t group, uint32_t seed, float p,
                      const uint32_t* seed_dev, void* stream);

/* ---- fused softmax + Dice / CE / soft-Dice / MSE reductions (utils/losses.py:22-59,68-90,200-231 and the
 * CrossEntropyLoss at train_inherent_consistent_unet_3D_BraTS.py:107).  a is [B,nc,S] logits (or probabilities when
 * a_is_prob); the target is int64 labels [B,S] (modes 0,1) or a second logit tensor b [B,nc,S] (modes 2,3):
 *   mode 0 hard Dice        out = {0, dice}          mode 1 CE + hard Dice   out = {ce, dice}
 *   mode 2 soft Dice        out = {0, dice}          mode 3 softmax MSE      out = {mse, 0}
 * stats: ICL_LOSS_STATS_FLOATS(nc) floats — the 3*nc+1 reduced sums (kept for backward) followed by per-workgroup partials,
 * summed in a fixed order (no atomics: the loss is bit-reproducible and nothing needs zeroing); gout0 / gout1: upstream grads of out[0] / out[1], one float each, NULL when
 * that output does not reach the loss; ga: gradient w.r.t. a.  weight (per-class Dice weights) may be NULL.
 * 1 <= nc <= 256: up to 16 classes stay in registers, 17 .. 256 take the generic-class kernels (same stats buffer, same fixed
 * summation order); outside that range the calls return -1 and launch nothing. */
#define ICL_LOSS_MAX_BLOCKS 1024
#define ICL_LOSS_STATS_FLOATS(nc) ((3 * (nc) + 1) * (1 + ICL_LOSS_MAX_BLOCKS))
int icl_loss_fwd(const float* a, const float* b, const int64_t* labels, const float* weight, float* stats, float* out,
                 int batch, int nc, int64_t s, int mode, int a_is_prob, void* stream);
int icl_loss_bwd(const float* a, const float* b, const int64_t* labels, const float* weight, const float* stats,
                 const float* gout0, const float* gout1, float* ga, int batch, int nc, int64_t s, int mode, int a_is_prob,
                 void* stream);
/* All loss terms of a step in one statistics launch + one finalize launch (icl_loss_fwd_multi) and one gradient launch
 * (icl_loss_bwd_multi): job j is call j of icl_loss_fwd / icl_loss_bwd — same blocks, same partial sums, same order (bit-identical).
 * The trainer's objective (train_inherent_consistent_unet_3D_BraTS.py:105-112) is ten such terms.  `jobs`: HOST array of <= 12;
 * per job the arguments of the single-term calls (stats: ICL_LOSS_STATS_FLOATS(nc) floats, out: 2 floats; gout0 / gout1 / ga: backward).
 * All jobs of one call belong to one class group: nc <= 4, 5 .. 16, or 17 .. 256. */
typedef struct IclLossJob {
  const float* a; const float* b; const int64_t* labels; const float* weight;
  float* stats; float* out;
  const float* gout0; const float* gout1; float* ga;
  int64_t s;
  int batch, nc, mode, a_is_prob;
} IclLossJob;
int icl_loss_fwd_multi(const IclLossJob* jobs, int count, void* stream);
int icl_loss_bwd_multi(const IclLossJob* jobs, int count, void* stream);

/* ---- voxel-wise losses (utils/losses.py: softmax_kl_loss :93-112, compute_kl_loss :334-346, entropy_loss :33-39, entropy_loss_map
 * :62-65, entropy_minmization :321-325, entropy_map :328-331, FocalLoss :149-183), forward and backward.  Tensors are (outer, nc, inner):
 * the class axis has stride `inner` (inner = S: dim 1 of [B, nc, ...]; inner = 1: the last axis of [M, nc]).  1 <= nc <= 256 with the
 * class groups of icl_loss_fwd; outside that range, on a NULL pointer or on outputs that do not fit the call -1 is returned and nothing
 * is launched.  ws: ICL_POINT_LOSS_WS_FLOATS floats of per-workgroup partials, summed in a fixed order (no atomics, nothing to zero,
 * bit-reproducible); nothing is kept from the forward for the backward pass.  out / gout: one float.
 *   KL       out = w_fwd mean KL(q||p) + w_rev mean KL(p||q), p = softmax(a), q = softmax(b), mean over the outer*nc*inner elements
 *            (F.kl_div(reduction='mean')); logs are v - lse (an underflowed class adds 0).  ga or gb may be NULL (no gradient wanted there), not both.
 *   entropy  H_v = -sum_c p_c log(p_c + 1e-6), p = x or softmax(x) (from_logits); out = scale * mean_v H_v and / or map[v] = scale * H_v
 *            (either may be NULL, not both); gout / gmap: their upstream gradients (either may be NULL, not both).
 *   focal    loss_v = -alpha_y (1 - pt)^gamma log pt, pt = softmax(a)_y; out = mean (mean != 0) or sum over the voxels; alpha (nc floats)
 *            may be NULL.  (1 - pt)^gamma is a constant of the backward pass, as in the reference (pt from .data).  A label outside
 *            [0, nc) indexes nothing: its voxel adds 0 to the value and gets a zero gradient, and still counts in the mean. */
#define ICL_POINT_LOSS_WS_FLOATS ICL_LOSS_MAX_BLOCKS
int icl_kl_fwd(const float* a, const float* b, float* ws, float* out, int64_t outer, int nc, int64_t inner, float w_fwd, float w_rev,
               void* stream);
int icl_kl_bwd(const float* a, const float* b, const float* gout, float* ga, float* gb, int64_t outer, int nc, int64_t inner, float w_fwd,
               float w_rev, void* stream);
int icl_entropy_fwd(const float* x, float* ws, float* out, float* map, int64_t outer, int nc, int64_t inner, int from_logits, float scale,
                    void* stream);
int icl_entropy_bwd(const float* x, const float* gout, const float* gmap, float* gx, int64_t outer, int nc, int64_t inner, int from_logits,
                    float scale, void* stream);
int icl_focal_fwd(const float* a, const int64_t* labels, const float* alpha, float* ws, float* out, int64_t outer, int nc, int64_t inner,
                  float gamma, int mean, void* stream);
int icl_focal_bwd(const float* a, const int64_t* labels, const float* alpha, const float* gout, float* ga, int64_t outer, int nc,
                  int64_t inner, float gamma, int mean, void* stream);

/* ---- aligner token operators (networks/unet_3D_icl.py:244-315)
 * LayerNorm over the last axis c of [rows, c] (nn.LayerNorm, eps 1e-5); mean/rstd [rows] are saved for the backward;
 * dgamma/dbeta (may both be NULL) are overwritten: row-chunk partial sums go to `ws` (icl_layernorm_bwd_ws_bytes) and are added in
 * a fixed order (no float atomics).  dgamma NULL with ws given: only the partials are written — ws = part_g [chunks][c] followed by
 * part_b [chunks][c], chunks = ws bytes / (8 c) — and the caller sums them later (icl_colsum_multi; ICLTrainer does that for all
 * LayerNorm layers of a step in one launch).  GELU is the exact erf form (nn.GELU default). */
int icl_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows,
                      int c, float eps, void* stream);
int64_t icl_layernorm_bwd_ws_bytes(int64_t rows, int c);
int icl_layernorm_bwd(const float* gy, const float* x, const float* gamma, const float* mean, const float* rstd, float* gx,
                      float* dgamma, float* dbeta, void* ws, int64_t rows, int c, void* stream);
int icl_gelu_fwd(const float* x, float* y, int64_t n, void* stream);
int icl_gelu_bwd(const float* gy, const float* x, float* gx, int64_t n, void* stream);
/* Prototype cross-attention of Query_Attention.forward (:283-297): q [B,h,nc,d] (reshape-quirk layout of fc_q's output),
 * kv [B,N,2,h,d] (fc_kv output).  logits [B,nc,h,N] = scale*q.k (the pre-softmax map, in the class-major layout the reference returns it in: `attn1.permute(0, 2, 1, 3)`, :296),
 * out [B,h,nc,d] = softmax_N(logits) @ v, stats [B,h,nc,2] = (row max, sum exp).  d in {8,16}, 1 <= nc <= 256 (more than 16: staged in LDS 16 at a time).
 * Backward: gout / glog (either may be NULL) are the upstream gradients of out / logits. */
int icl_attn_fwd(const float* q, const float* kv, float* logits, float* out, float* stats, int b, int h, int nc, int n, int d,
                 float scale, void* stream);
int icl_attn_bwd(const float* q, const float* kv, const float* logits, const float* stats, const float* out, const float* gout,
                 const float* glog, float* gq, float* gkv, int b, int h, int nc, int n, int d, float scale, void* stream);
/* the same with a workspace (icl_attn_bwd_ws_bytes): dQ is summed from per-token-chunk shares written by the dK / dV pass instead of a second
 * walk over K and V by one workgroup per (sample, head, class) row; ws == NULL is icl_attn_bwd */
int64_t icl_attn_bwd_ws_bytes(int b, int h, int nc, int n, int d);
int icl_attn_bwd_ws(const float* q, const float* kv, const float* logits, const float* stats, const float* out, const float* gout,
                    const float* glog, float* gq, float* gkv, void* ws, int b, int h, int nc, int n, int d, float scale, void* stream);

/* out_i[c] = sum_r g_i[r * cols_i + c] for `count` small row-major matrices, one launch per 48 of them: the bias gradients of the
 * aligner / Swin Linear layers (unet_3D_icl.py:244-315) collected over a backward pass. */
int icl_colsum_multi(const void* const* g, void* const* out, const int32_t* rows, const int32_t* cols, int count, void* stream);
/* out[j] = sum_i w[j * n_in + i] * *in[i]: n_in <= 16 device scalars (pointers in a HOST array), n_out <= 16 results, w a HOST array.
 * The scalar arithmetic between the loss terms of an ICL step (weighted sums, means over three scales) in one launch; its backward is
 * the same call with the transposed weights. */
int icl_scalar_combine(const void* const* in, const float* w, int n_in, int n_out, float* out, void* stream);

/* ---- token <-> window order of the Swin blocks (pad + roll + window_partition, window_reverse + roll + crop:
 * networks/swinunetr_icl.py:825-866, networks/swinunet_icl.py:256-283): out[b][m][0..c) = idx[m] >= 0 ? src[b][idx[m]][0..c) : 0,
 * src [b, s, c], out [b, m, c], c % 4 == 0.  The inverse direction and both gradients are gathers with the inverse index. */
int icl_gather_rows(const float* src, const int32_t* idx, float* out, int64_t b, int64_t s, int64_t m, int c, void* stream);
/* out[b][m] = src[b][idx2[m][0]] + src[b][idx2[m][1]] (an index of -1 is absent).  Gradient of icl_gather_rows when the
 * index lists a source row up to twice or not at all: PatchMerging's eight strided slices repeat two and omit two
 * (networks/swinunetr_icl.py:953-961; the 2-D merge networks/swinunet_icl.py:320-326 is a plain permutation). */
int icl_gather_rows_sum2(const float* src, const int32_t* idx2, float* out, int64_t b, int64_t s, int64_t m, int c, void* stream);

/* ---- 3^3 convolutions on tiny volumes (<= 6^3 voxels, hundreds of channels: `encoder10`/`decoder5` of SwinUNETR,
 * networks/swinunetr_icl.py:163-183, and the U-Net `center`, networks/unet_3D_icl.py:54) are skinny GEMMs over the weights:
 * cols [n*S, c*27] with cols[b*S+v][ci*27+tap] = x[b][ci][v+offset(tap)] (zero padded), y = cols * W[cout, c*27]^T on the
 * library GEMM.  col2im3 is the exact transpose (input gradient from d(cols)). */
int icl_im2col3(const float* x, float* cols, int n, int c, int d, int h, int w, void* stream);
/* planes[b][ci*27 + tap][v] = x[b][ci][v + offset(tap)] (zero outside), w % 4 == 0: the first convolution's weight gradient
 * (Cin = 1: networks/unet_3D.py:27, utils.py:104) as icl_conv1x1_wgrad over 27 shifted planes instead of a Cin-padded implicit GEMM. */
int icl_im2col3_planes(const float* x, float* planes, int n, int c, int d, int h, int w, void* stream);

/* The same layer — nn.Conv3d(1, Cout <= 16, 3, padding 1), the first convolution of unet_3D(in_channels=1) (networks/unet_3D.py:27,
 * networks/utils.py:104) — as dedicated kernels (kernels/conv_cin1.h): K = 27, both directions are HBM streams of the Cout-channel tensor.
 * x [N][1][D][H][W] (sample stride x_bstride), w the nn.Conv3d weight [Cout][1][3][3][3], y / gy [N][Cout][D][H][W] (sample stride
 * y_bstride / gy_bstride), gw like w.  The weight gradient needs W % 4 == 0, gy 16-byte aligned and a workspace of
 * icl_conv3d_cin1_wgrad_ws_bytes bytes; partial sums are added in a fixed order. */
int icl_conv3d_cin1_fwd(const float* x, const float* w, const float* bias, float* y, int n, int cout, int d, int h, int wd, int64_t x_bstride,
                        int64_t y_bstride, void* stream);
int64_t icl_conv3d_cin1_wgrad_ws_bytes(int n, int d, int h);
int icl_conv3d_cin1_wgrad(const float* x, const float* gy, float* gw, void* ws, int n, int cout, int d, int h, int wd, int64_t x_bstride,
                          int64_t gy_bstride, void* stream);
int icl_col2im3(const float* g, float* dx, int n, int c, int d, int h, int w, void* stream);

/* ---- ConvTranspose3d(kernel 2, stride 2, no bias) = GEMM + depth-to-space (MONAI UnetrUpBlock.transp_conv in SwinUNETR,
 * networks/swinunetr_icl.py:186-230): yt [n, d*h*w, cout*8] (column co*8 + i*4 + j*2 + k) -> out[b][co][2z+i][2y+j][2x+k];
 * out_bstride lets the result land in the channel slice of the concat buffer that UnetrUpBlock builds next.
 * icl_space_to_depth2 is the inverse (gradient back to the GEMM layout). */
int icl_depth_to_space2(const float* yt, float* out, int n, int d, int h, int w, int cout, int64_t out_bstride, void* stream);
int icl_space_to_depth2(const float* g, float* gt, int n, int d, int h, int w, int cout, int64_t g_bstride, void* stream);

/* ---- nn.Linear forward / input gradient and the other dense fp32 products of the path, on the fp32 matrix cores
 * (csrc/kernels/gemm.h).  Replaces F.linear at networks/unet_3D_icl.py:283-315 (fc_q, fc_kv, proj, MLP.fc1/fc2 and the token-axis
 * Class_Decoder.mlp2, :258-268), query_convs (:197), the token projection (:212), the Swin qkv / proj / MLP / PatchMerging linears
 * (networks/swinunetr_icl.py:703-750,812,946-976) and their autograd input gradients.
 *   icl_linear_fwd    y[rows, out] = act(x[rows, in] W[out, in]^T + bias)     act 0 none, 1 exact-erf GELU (MLP.act, :307); bias may be NULL
 *   icl_linear_dgrad  gx[rows, in] = gy[rows, out] W[out, in]
 *   icl_linear_wgrad_small  dw[out, in] = gy^T x for few rows (tall inputs: icl_linear_wgrad above)
 * rows <= 32 with >= 2^20 weights (the 13,824^2 / 1,728^2 mlp2 matrices): the weight matrix is streamed from HBM exactly once
 * (HBM-bound); everything else runs on LDS-staged 64x64 wave tiles, split over K when the output has too few tiles to fill the chip.
 * ws: icl_linear_ws_bytes(rows, in, out, kind) bytes, kind 0 fwd / 1 dgrad / 2 wgrad_small / 3 dgrad_sgd (may be 0; NULL then allowed). */
int64_t icl_linear_ws_bytes(int64_t rows, int in, int out, int kind);
int icl_linear_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, int64_t rows, int in, int out, int act,
                   void* stream);
int icl_linear_dgrad(const float* gy, const float* w, float* gx, void* ws, int64_t rows, int in, int out, void* stream);
/* gx = gy W AND dW = gy^T x of a Linear layer that sees <= 32 rows (the aligner's query-side layers, unet_3D_icl.py:283-315) in one launch;
 * returns 1 (nothing launched) when the shapes do not take the weight-streaming path: call icl_linear_dgrad + icl_linear_wgrad_small then */
int icl_linear_bwd_small(const float* gy, const float* w, const float* x, float* gx, float* dw, void* ws, int64_t rows, int in, int out,
                         void* stream);
int icl_linear_wgrad_small(const float* gy, const float* x, float* dw, void* ws, int64_t rows, int in, int out, void* stream);
/* Backward + optimiser step of a big skinny Linear in ONE pass over its weight (single rank, the weight used once per step):
 * gx[rows, in] = gy[rows, out] W_old, then W / momentum are updated from the factors of dW = gy^T x with the SGD rule of
 * icl_sgd_step_factored (train_inherent_consistent_unet_3D_BraTS.py:85-86,113-115 on Class_Decoder.mlp2, unet_3D_icl.py:258-268).
 * rows <= 32, in / out multiples of 4; ws: icl_linear_ws_bytes(rows, in, out, 3) bytes. */
int icl_linear_dgrad_sgd(const float* gy, const float* x, float* w, float* mom, float* gx, void* ws, int64_t rows, int in, int out,
                         float lr, float momentum, float weight_decay, int first, const float* lr_dev, void* stream);
/* General (batched) product C[b] = act(A[b] B[b] + bias[n]), C [m, n] with row pitch ldc; act = activation (0 none, 1 GELU)
 * + 16 when the bias is indexed by the output row m instead of the column (1x1x1 convolution: rows are channels).  a_kcontig 1: A is row-major [m][lda]
 * (k contiguous), 0: A is given transposed [k][lda] (m contiguous); b_kcontig 1: B is [n][ldb] (k contiguous, "W^T"), 0: B is
 * [k][ldb].  Batch strides in elements.  Used for ConvTranspose3d(k=2, s=2) as one product (MONAI UnetrUpBlock.transp_conv,
 * networks/swinunetr_icl.py:178-225: A = x[b] as [Cin][S] transposed view, B = W [Cin][Cout*8]) and its gradients, and for the
 * 3^3 convolutions on <= 6^3 voxels through im2col (networks/utils.py:104,107 at the `center` level).
 * ws: icl_gemm_ws_bytes(m, n, k, batch) bytes (split-K slabs, summed in a fixed order); with ws NULL the product runs unsplit. */
int64_t icl_gemm_ws_bytes(int64_t m, int n, int k, int batch);
int icl_gemm(const float* a, const float* b, float* c, const float* bias, void* ws, int64_t m, int n, int k, int64_t lda, int64_t ldb,
             int64_t ldc, int a_kcontig, int b_kcontig, int act, int batch, int64_t a_bstride, int64_t b_bstride, int64_t c_bstride,
             void* stream);

/* ---- nn.Linear weight/bias gradient for tall token matrices (qkv / proj / MLPBlock linears of the Swin stages,
 * networks/swinunetr_icl.py:703,705,812; PatchEmbed; the k2s2 transposed convolutions written as GEMMs):
 * dw[o][i] = sum_r gy[r][o] * x[r][i], db[o] = sum_r gy[r][o] (db may be NULL); gy [rows, o], x [rows, i] row-major.
 * Rows are split over many waves (fp32 MFMA), partial blocks go to ws (icl_linear_wgrad_ws_bytes) and are summed in a fixed order. */
int64_t icl_linear_wgrad_ws_bytes(int64_t rows, int o, int i);
int icl_linear_wgrad(const float* gy, const float* x, float* dw, float* db, void* ws, int64_t rows, int o, int i, void* stream);

/* Weight/bias gradient of a 1x1x1 convolution on a big volume (channel-major operands, s = D*H*W voxels per sample, s % 4 == 0):
 * gw[cout][cin] = sum_{b,v} gy[b][co][v] * x[b][ci][v]; gbias may be NULL.  Same row-split / slab scheme as icl_linear_wgrad. */
int64_t icl_conv1x1_wgrad_ws_bytes(int n, int64_t s, int cin, int cout);
int icl_conv1x1_wgrad(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int cin, int cout, int64_t s,
                      int64_t x_bstride, int64_t gy_bstride, void* stream);
/* live batch (see icl_conv3d_fwd_presplit_live; `final` without dropout, unet_3D_icl.py:117): the entry point on the whole batch */
int icl_conv1x1_wgrad_live(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int n_live, int cin, int cout, int64_t s,
                           int64_t x_bstride, int64_t gy_bstride, void* stream);

/* ---- Swin window attention: WindowAttention.forward core, networks/swinunetr_icl.py:728-747 —
 *   attn = softmax((q*scale) @ k^T + relative_position_bias [+ shift mask]);  out = attn @ v   per (window, head).
 * head_dim 16 (3-D SwinUNETR, n <= 352) or 32 (2-D Swin-UNet 7x7 windows, networks/swinunet_icl.py:120-155, n <= 96).
 * qkv  [B_, n, 3, heads, head_dim]  output of the qkv Linear (B_ = batch * nW windows, window id of row b_ = b_ % nW)
 * bias [heads, n, npad], npad = n rounded up to 16, pad columns = -1e30 (icl_window_attn_bias_elems floats; the caller gathers
 *      relative_position_bias_table[relative_position_index[:n,:n]] into it, :733-737)
 * regions int32 [nW, n] or NULL: region id of every token of the rolled volume; query/key pairs with different ids get -100
 *      (the dense attn_mask of compute_mask, :979-1016, is exactly -100 * (id_i != id_j))
 * out [B_, n, heads*head_dim];  lse [B_, heads, n] = log-sum-exp of every score row (saved for backward).
 * Backward: dqkv (layout of qkv) and, if dbias != NULL, dbias [chunks, heads, n, npad]: one slab per slice of the B_ windows
 * (icl_window_attn_bwd_chunks), to be summed by icl_relpos_bias_bwd_sum. */
int64_t icl_window_attn_bias_elems(int n, int heads);
/* bias[h][i][j] = table[index[i*idx_stride + j]][h] (j < n), -1e30 (n <= j < npad): the gather of :733-737 into the padded layout;
 * index = the int64 relative_position_index buffer [idx_stride, idx_stride] (343 x 343), table [table_rows, heads].
 * Backward: icl_relpos_bias_bwd_sum below. */
int icl_relpos_bias_fwd(const float* table, const int64_t* index, float* bias, int n, int heads, int idx_stride, void* stream);
int icl_window_attn_fwd(const float* qkv, const float* bias, const int32_t* regions, float* out, float* lse, int b_, int n, int heads,
                        int nw, int head_dim, float scale, void* stream);
int icl_window_attn_bwd(const float* qkv, const float* bias, const int32_t* regions, const float* out, const float* lse,
                        const float* dout, float* dqkv, float* dbias, int b_, int n, int heads, int nw, int head_dim, float scale,
                        void* stream);
/* WindowAttention.attn_drop on the soft-max probabilities (swinunetr_icl.py:742-747: attn = self.attn_drop(attn) between the soft-max and
 * attn @ v) inside the same fused kernels: out = (keep * P / (1 - p)) @ v.  The mask is never stored: forward and both backward kernels
 * regenerate keep(k) = hash(seed, k) >= (unsigned)(p * 2^32) — the decision of icl_dropout / icl_drop_path for element k — with
 * k = ((b_ * heads + h) * n + i) * n + j, the flat index of the reference's [B_, heads, n, n] attention tensor.  0 < p < 1; seed_dev as
 * icl_drop_path (optional device-resident step counter hashed into the seed).  lse stays the log-sum-exp of the undropped scores; all
 * other arguments, the kernel choice and the d(bias) slabs as icl_window_attn_fwd / _bwd (which remain the p = 0 entry points). */
int icl_window_attn_fwd_drop(const float* qkv, const float* bias, const int32_t* regions, float* out, float* lse, int b_, int n, int heads,
                             int nw, int head_dim, float scale, uint32_t seed, float p, const uint32_t* seed_dev, void* stream);
int icl_window_attn_bwd_drop(const float* qkv, const float* bias, const int32_t* regions, const float* out, const float* lse,
                             const float* dout, float* dqkv, float* dbias, int b_, int n, int heads, int nw, int head_dim, float scale,
                             uint32_t seed, float p, const uint32_t* seed_dev, void* stream);
/* Unit check of the attn_drop mask (swinunetr_icl.py:742-747).  out[i] = 1 where the attention kernels keep the probability whose flat index in [B_, heads, n, n] is base + i (0 <= i < count <= 2^17), 0
 * where they drop it — their hoisted form of the hash (the high word of the 64-bit index hashed once per (window, head), with and without
 * the carry of base + i) for ANY 64-bit base, so that it can be checked against icl_dropout's decisions beyond 2^32 elements. */
int icl_window_attn_keep_probe(int32_t* out, int64_t base, int count, uint32_t seed, float p, const uint32_t* seed_dev, void* stream);
/* d(bias) of icl_window_attn_bwd arrives as icl_window_attn_bwd_chunks(...) slabs [chunk][heads][n][npad] (one per slice of windows,
 * plain stores, every used element written: no zero fill).  icl_relpos_bias_bwd_sum adds them into the table gradient in a FIXED order —
 * inv: the padded positions i * npad + j of index[:n, :n] sorted by table row (stable), offs[t] .. offs[t + 1] the entries of row t —
 * so the gradient of relative_position_bias_table (swinunetr_icl.py:733-737) is bit-reproducible run to run.  dbias is used as scratch
 * (the slabs are first added, in order, into slab 0). */
int icl_window_attn_bwd_chunks(int b_, int n, int heads, int nw, int head_dim);
int icl_relpos_bias_bwd_sum(float* dbias, int chunks, const int32_t* inv, const int32_t* offs, float* dtable, int64_t table_rows, int n,
                            int heads, void* stream);

/* ---- on-device training augmentation: RandomRotFlip -> RandomCrop -> ToTensor of the 3-D trainers
 * (dataloaders/brats2019.py:80-147,177-189; composed at train_inherent_consistent_unet_3D_BraTS.py:66-73) as one gather over
 * volumes resident in HBM.  images[b] / labels[b]: HOST arrays of device pointers to the fp32 [n0,n1,n2] volume and its uint8
 * label; params: HOST int32 [batch][11] = {n0, n1, n2, k (np.rot90 count on axes 0,1), flip axis (0, 1, -1 none), zero padding
 * p0, p1, p2 (both sides), crop origin c0, c1, c2 (in the padded, rotated, flipped volume)}, drawn by the caller with the
 * reference's numpy call sequence.  image_out [batch,1,o0,o1,o2] fp32, label_out [batch,o0,o1,o2] int64.  batch <= 16. */
int icl_crop_rotflip(const void* const* images, const void* const* labels, const int32_t* params, int batch, float* image_out,
                     int64_t* label_out, int o0, int o1, int o2, void* stream);

/* ---- the same chain on multi-modal volumes (BraTS's four co-registered MR modalities; the reference feeds FLAIR only, its transforms
 * are the ones above, dataloaders/brats2019.py:80-147,177-189): images[b] points to a contiguous fp32 [channels,n0,n1,n2] volume,
 * labels[b] to ONE uint8 [n0,n1,n2] label; params as for icl_crop_rotflip, one geometry for all channels of a sample.  image_out
 * [batch,channels,o0,o1,o2] fp32, label_out [batch,o0,o1,o2] int64.  One launch: the source index of an output position is computed once
 * and used for every channel and for the label.  With channels == 1 the result is icl_crop_rotflip's bit for bit.  Returns -1, launching
 * nothing, for a null pointer, a batch outside 1..16, channels outside 1..16, an output extent < 1 or more than 2^31 - 1 output voxels
 * a sample, and for what icl_crop_rotflip refuses in a row. */
int icl_crop_rotflip_channels(const void* const* images, const void* const* labels, const int32_t* params, int batch, int channels,
                              float* image_out, int64_t* label_out, int o0, int o1, int o2, void* stream);

/* ---- the same chain with an AFFINE stage about the patch centre (arbitrary rotation and zoom: MONAI RandAffined, nnU-Net's rotation
 * and scaling), for one or many channels (crop_rotflip_affine_kernel, csrc/kernels/datafeed.h; the definition is in DESIGN.md "Affine
 * stage of the BraTS feed").  The arguments of icl_crop_rotflip_channels, plus affine_params: HOST double [batch][10] = {flag, M row-major
 * (3x3)}.  flag 0: the sample is gathered as icl_crop_rotflip_channels gathers it, bit for bit.  flag 1: with Y = flip(rot90(x, k), axis)
 * of extents (r0, r1, n2), never materialised, x_a = t_a + ((M_a0 u_0 + M_a1 u_1) + M_a2 u_2), u_a = q_a - (o_a - 1) / 2 and
 * t_a = (c_a - p_a) + (o_a - 1) / 2, in double, every product and sum rounded on its own; every channel of the image is interpolated
 * trilinearly in Y (eight taps in the order (0,0,0) .. (1,1,1), a tap outside Y counting as 0, summed left to right in double, one
 * rounding to fp32) and the label is Y at rint(x_a) (half to even; 0 outside).  x is a coordinate of the WHOLE of Y: voxels outside the
 * crop window are read.  Coordinates, tap offsets and weights are computed once per output voxel and used for every channel and the label.
 * Returns -1, launching nothing, for whatever icl_crop_rotflip_channels refuses and for a null affine_params, a flag other than 0 or 1,
 * or an entry of M (of any sample, whatever its flag) that is not finite or exceeds 16 in magnitude.  All range tests of the kernel are
 * made on the double coordinate, so no M can cause a read outside the volume. */
int icl_crop_rotflip_affine(const void* const* images, const void* const* labels, const int32_t* params, const double* affine_params, int batch,
                            int channels, float* image_out, int64_t* label_out, int o0, int o1, int o2, void* stream);

/* ---- channel-wise intensity normalisation of a resident volume, in place (MONAI's NormalizeIntensityd(nonzero=True,
 * channel_wise=True): mask 0, apply 0; the reference's itensity_normalize_one_volume, dataloaders/brats_proprecessing.py:62-78:
 * mask 1, apply 1).  image: DEVICE fp32 [channels][voxels], channels in 1..16, voxels in 1..2^31 - 1.  mask_mode: 0 x != 0, 1 x > 0,
 * 2 every voxel.
 * icl_channel_norm_stats (four launches, no atomics, nothing read back): stats_out DEVICE double [channels][4] = {count, mean, std, 0}
 *   of the voxels in the mask: mean = sum / count and std = sqrt(sum (x - mean)^2 / count) (population), every sum in double in the
 *   fixed order documented at channel_norm_partial_kernel; an empty mask gives four zeros.  ws: DEVICE scratch of channels * 256 * 2
 *   doubles.
 * icl_channel_norm_apply: x <- fp32(fp32(x - m) / s) with m = fp32(mean), s = fp32(std) and s = 1 where that is 0: a true subtraction
 *   and a true division.  apply_mode 0: the voxels of the mask only; 1: every voxel.  A channel whose count is 0 is left untouched. */
int icl_channel_norm_stats(const float* image, int channels, int64_t voxels, int mask_mode, double* stats_out, double* ws, void* stream);
int icl_channel_norm_apply(float* image, int channels, int64_t voxels, int mask_mode, int apply_mode, const double* stats, void* stream);

/* ---- on-device random transforms of the 3-D AMOS trainer (train_inherent_consistent_unet_3D_AMOS22.py:102-133: RandSpatialCropd ->
 * SpatialPadd -> RandFlipd on axis 0, 1, 2 -> RandRotate90d -> RandShiftIntensityd) as one gather over volumes resident in HBM.
 * images[b] / labels[b]: HOST arrays of device pointers to the fp32 [n0,n1,n2] volume and its uint8 label; int_params: HOST int32
 * [batch][14] = {n0, n1, n2, crop origin c0, c1, c2, crop size s0, s1, s2 (min(R, n)), left zero padding l0, l1, l2 (R - s - l on
 * the right), flip mask (bit a: np.flip on axis a), k (np.rot90 count on axes 0,1, 0..3)}; float_params: HOST fp32 [batch][2] =
 * {mul, add}: every image voxel, padded ones included, becomes fp32(fp32(v * mul) + add); padded labels are 0.  Drawn by the caller
 * (icl_amd.dataloaders.amos.draw_amos_params).  image_out [batch,1,R0,R1,R2] fp32, label_out [batch,R0,R1,R2] int64.  batch <= 16.
 * Returns -1, launching nothing, for a null pointer, a batch outside 1..16, c < 0, s < 1, c + s > n, l < 0, l + s > R, k outside
 * 0..3, or an odd k with R0 != R1 (the rotated patch would not have the output's shape). */
int icl_volume_feed(const void* const* images, const void* const* labels, const int32_t* int_params, const float* float_params, int batch,
                    float* image_out, int64_t* label_out, int R0, int R1, int R2, void* stream);

/* ---- foreground-balanced crops: the centre draws of MONAI's RandCropByPosNegLabeld (utils/data_utils.py:84-99, get_loader) on volumes
 * resident in HBM, without an index list per voxel.  Members: fg = label != 0; bg = label == 0 && image > threshold (NaN is not > t).
 * A RANK INDEX of a volume is, per list, a uint32 array of tiles + 1 entries, tiles = ceil(n0 n1 n2 / icl_rank_tile()): entry t = the
 * number of members among the flat (C-order) voxels before tile t, the last entry = the length of the list.  Integer sums in a fixed
 * order, no atomics: a function of the volume alone. */
int icl_rank_tile(void);      /* consecutive flat voxels per index entry (1024) */
/* Builds both indices of one volume (two launches).  image fp32 [n0,n1,n2], label uint8 [n0,n1,n2], fg_index / bg_index: DEVICE uint32
 * [tiles + 1].  Returns -1, launching nothing, for a null pointer, an extent outside 1..65535 (MONAI casts crop centres to uint16) or
 * more than 2^31 - 1 voxels. */
int icl_rank_index_build(const float* image, const uint8_t* label, int n0, int n1, int n2, float threshold, uint32_t* fg_index,
                         uint32_t* bg_index, void* stream);
/* Crop origins of `batch` samples (<= 16) in one launch, one workgroup a sample: the voxel of rank `rank` in the chosen list is found
 * through the index, unravelled to a centre, and origin_a = clamp(centre_a - s_a / 2, 0, n_a - s_a) (correct_crop_centers followed by
 * SpatialCrop) is stored to origins [batch][3] int32 on the DEVICE.  images / labels / fg_indices / bg_indices: HOST arrays of device
 * pointers; int_params: HOST int32 [batch][8] = {n0, n1, n2, kind (0 foreground, 1 background), rank, crop size s0, s1, s2}; threshold:
 * the one the indices were built with.  rank < length of the list is the CALLER's check (only the host knows the totals); a larger
 * rank still reads nothing outside the volume and yields the origin of voxel 0.  Returns -1, launching nothing, for a null pointer,
 * a batch outside 1..16, extents as above, a kind outside {0, 1}, a negative rank or a crop size outside 1..n. */
int icl_rank_select(const void* const* images, const void* const* labels, const void* const* fg_indices, const void* const* bg_indices,
                    const int32_t* int_params, float threshold, int batch, int32_t* origins, void* stream);
/* icl_volume_feed with the crop origins read from DEVICE memory (origins [batch][3] int32, as icl_rank_select left them on the same
 * stream) instead of int_params, whose c0, c1, c2 are ignored.  Checks everything icl_volume_feed checks except the origin range
 * (crop size: 1 <= s <= n); an origin outside [0, n - s] is clamped into it by the kernel. */
int icl_volume_feed_origins(const void* const* images, const void* const* labels, const int32_t* int_params, const float* float_params,
                            int batch, const int32_t* origins, float* image_out, int64_t* label_out, int R0, int R1, int R2, void* stream);

/* ---- the 3-D feed with an AFFINE stage (arbitrary rotation and zoom: MONAI RandAffined, nnU-Net's rotation and scaling) between the
 * pad and the flips: crop -> symmetric pad -> affine about the patch centre -> flips -> rot90 -> intensity (volume_feed_affine_kernel,
 * csrc/kernels/datafeed.h; the definition is in DESIGN.md "Affine stage of the 3-D feed").  The arguments of icl_volume_feed /
 * icl_volume_feed_origins, plus affine_params: HOST double [batch][10] = {flag, M row-major (3x3)}.  flag 0: the sample is gathered as
 * icl_volume_feed gathers it, bit for bit.  flag 1: the output voxel is mapped back through rot90 and the flips to patch coordinates p,
 * then x_a = t_a + ((M_a0 u_0 + M_a1 u_1) + M_a2 u_2) with u_a = p_a - (R_a - 1) / 2 and t_a = (c_a - l_a) + (R_a - 1) / 2, in double,
 * every product and sum rounded on its own; the image is interpolated trilinearly (eight taps in the order (0,0,0) .. (1,1,1), summed
 * left to right in double, one rounding to fp32, then fp32(fp32(v * mul) + add)) and the label is the voxel at rint(x_a) (half to
 * even).  x is a coordinate of the WHOLE volume: voxels outside the crop window are read, and only what lies outside the volume counts
 * as 0 (grid_sample's padding_mode="zeros").  Return -1, launching nothing, for whatever the siblings refuse and for a null
 * affine_params, a flag other than 0 or 1, or an entry of M (of any sample, whatever its flag) that is not finite or exceeds 16 in
 * magnitude.  All range tests of the kernel are made on the double coordinate, so no M and no origin can cause a read outside the volume. */
int icl_volume_feed_affine(const void* const* images, const void* const* labels, const int32_t* int_params, const float* float_params,
                           const double* affine_params, int batch, float* image_out, int64_t* label_out, int R0, int R1, int R2, void* stream);
int icl_volume_feed_affine_origins(const void* const* images, const void* const* labels, const int32_t* int_params, const float* float_params,
                                   const double* affine_params, int batch, const int32_t* origins, float* image_out, int64_t* label_out,
                                   int R0, int R1, int R2, void* stream);

/* ---- the CACHED prefix of the AMOS trainer (train_inherent_consistent_unet_3D_AMOS22.py:86-101, validation :141-154):
 * ScaleIntensityRanged -> CropForegroundd -> Orientationd("RAS") -> [SpatialPadd] -> Spacingd(bilinear / nearest, border), and its inverse
 * for label maps (csrc/kernels/prefix.h; the definition is in DESIGN.md "AMOS cached prefix").  A case is planned on the host
 * (icl_amd.dataloaders.amos.plan_prefix) and handed over as
 *   int_params:    HOST int32 [24] = {raw extents n[3], box lo[3], box hi[3] (exclusive, raw axes), perm[3] (oriented axis a is raw axis
 *                  perm[a]), sign[3] (1, or -1: reversed), pad front f[3], padded extents m[3], output extents o[3]}, the last four per
 *                  ORIENTED axis;
 *   double_params: HOST double [6] = {source spacing s[3], target spacing p[3]} per oriented axis;
 *   window:        HOST fp32 [5] = {a_min, fp32(a_max - a_min), b_min, fp32(b_max - b_min), b_max}; clip: clamp into [b_min, b_max].
 * Both plan-taking functions return -1, launching nothing, for a null pointer, a raw extent outside 1..65535 or more than 2^31 - 1 raw
 * or output voxels, a perm that is no permutation, a sign other than 1 / -1, a non-finite or non-positive spacing, a box that is empty or
 * outside the volume, f < 0 or f + (box extent) > m, or an output extent other than rint((m - 1) * (s / p) + 1) (half to even). */
/* The foreground box: the smallest box holding every voxel whose windowed value is > 0.  image: DEVICE fp32 [n0,n1,n2]; box: DEVICE
 * int32 [6] = {lo0, lo1, lo2, hi0, hi1, hi2}, hi INCLUSIVE ({INT_MAX x 3, -1 x 3} when no voxel qualifies); ws: DEVICE int32
 * [6 * 1024] of scratch.  Two launches, integer min / max in a fixed order, no atomics. */
int icl_prefix_box(const float* image, int n0, int n1, int n2, const float* window, int clip, int32_t* box, int32_t* ws, void* stream);
/* One launch writes image_out fp32 [o0,o1,o2] and label_out uint8 [o0,o1,o2] from the raw DEVICE arrays image fp32 / label uint8
 * [n0,n1,n2]: fp64 coordinates, eight windowed taps summed in a fixed order in double and rounded once; label at rint(x). */
int icl_prefix_resample(const float* image, const uint8_t* label, const int32_t* int_params, const double* double_params, const float* window,
                        int clip, float* image_out, uint8_t* label_out, void* stream);
/* The inverse for a label map on the respaced grid: prediction DEVICE [o0,o1,o2], elem_kind 0 = uint8, 1 = int64 (the low byte is kept);
 * out DEVICE uint8 [n0,n1,n2]: 0 outside the box, inside the prediction at rint(min(max(u * (s / p), 0), o - 1)) per oriented axis. */
int icl_prefix_restore(const void* prediction, int elem_kind, const int32_t* int_params, const double* double_params, uint8_t* out,
                       void* stream);

/* ---- the INTENSITY stage of the 3-D feed (csrc/kernels/intensity.h; the definition is in DESIGN.md "Intensity stage of the 3-D feed"):
 * five entry points that act on the image batch the gather has written and leave their result in it, image DEVICE fp32
 * [batch][R0][R1][R2], in the order noise, blur, lowres, stats, point, on the caller's stream.  Every row of `params` is a HOST row per
 * sample (double; int32 for lowres and stats) whose flags are exactly 0 or 1; EVERY field of EVERY row is checked, whatever the flags (a caller fills the rows of a sample without the transform with legal
 * values); a launch whose samples all have the flag 0 launches nothing and returns 0.  All five return -1, launching nothing, for a null
 * pointer, batch outside 1..16, an extent below 1, or more than 2^31 - 1 voxels a sample. */
/* Gaussian noise (nnU-Net GaussianNoiseTransform, MONAI RandGaussianNoised, the reference's RandomNoise, brats2019.py:150-161):
 * params [batch][4] = {flag, seed (an integer in 0 .. 2^32 - 1), sigma, clip}.  x = fp32(x + n), n = fp32(sigma z) clipped to
 * +- fp32(clip sigma) when clip > 0; z from the mix32 counter hash of (seed, flat voxel index) and a Box-Muller step in double, one pair
 * of uniforms per voxel.  Refused: a seed that is no such integer, a non-finite or non-positive sigma, a non-finite or negative clip. */
int icl_intensity_noise(float* image, const double* params, int batch, int R0, int R1, int R2, void* stream);
/* Gaussian blur (nnU-Net GaussianBlurTransform, MONAI RandGaussianSmoothd): scipy.ndimage.gaussian_filter(x, sigma, mode="reflect",
 * truncate=4.0) per sample.  params [batch][15] = {flag, sigma, w_0 .. w_12}: the radius is r = int(4 sigma + 0.5) and w_0 .. w_r are
 * the normalised weights the caller formed in double (w_k beyond r is not read).  Axis 0 goes batch -> scratch, axis 1 scratch -> batch,
 * axis 2 in place through LDS; scratch: DEVICE fp32 of the batch's size, distinct from it.  r = 0 is the identity and is not launched.
 * Refused: a non-finite or non-positive sigma, r above 12, r above the smallest of R0, R1, R2 (one reflection must suffice), a weight
 * outside [0, 1] (or NaN), R2 above 4096. */
int icl_intensity_blur(float* image, float* scratch, const double* params, int batch, int R0, int R1, int R2, void* stream);
/* Simulated low resolution (nnU-Net SimulateLowResolutionTransform as batchgeneratorsv2 defines it: interpolate "nearest-exact" down to
 * the low extents, "trilinear" with align_corners=False back up), between blur and stats.  params HOST int32 [batch][4] = {flag, L0, L1,
 * L2}, 1 <= L_a <= R_a.  One gather, batch -> scratch, reads per output the 8 patch voxels its 8 low-resolution cells stand for (no
 * low-resolution volume is written) and combines them in double along axis 2, 1, 0 with one rounding to fp32; a second launch copies
 * the samples that drew the transform back into the batch.  scratch: DEVICE fp32 of the batch's size, distinct from it.  A sample whose
 * L_a = R_a on all three axes is the identity and is not launched; L_a = R_a on one axis leaves that axis alone.  Refused: a flag
 * outside {0, 1}, an L_a outside 1 .. R_a (of ANY row, whatever its flag), scratch == image. */
int icl_intensity_lowres(float* image, float* scratch, const int32_t* params, int batch, int R0, int R1, int R2, void* stream);
/* Statistics of the samples whose flag is 1 (those that drew contrast or gamma; nnU-Net ContrastAugmentationTransform's mean, minimum
 * and maximum, MONAI RandAdjustContrast's minimum and maximum): flags HOST int32 [batch]; stats DEVICE fp32 [batch][4] = {min, max,
 * mean, 0}, mean = fp32(double sum / N) with the sum in the fixed order documented at intensity_stats_partial_kernel; the row of a
 * sample whose flag is 0 is not written.  ws: DEVICE double [16 * 64 * 3] of scratch.  Two launches, no atomics.  Refused: a flag
 * outside {0, 1}. */
int icl_intensity_stats(const float* image, const int32_t* flags, int batch, int R0, int R1, int R2, float* stats, double* ws, void* stream);
/* Contrast (nnU-Net ContrastAugmentationTransform, preserve_range) and gamma (MONAI RandAdjustContrast's formula, nnU-Net GammaTransform's
 * invert_image as a flag), pointwise, from the rows of `stats` that icl_intensity_stats left: params [batch][5] = {contrast flag, f,
 * gamma flag, g, invert flag}.  contrast: y = fp32(fp32(fp32(x - mean) f) + mean) clipped to [min, max]; gamma, on that result, with mn
 * and mx the images of min and max: t = (x - mn) / ((mx - mn) + 1e-7), y = fp32(fp32(pow(t, g) (mx - mn)) + mn) in double (g = 1:
 * pow(t, 1) is t), with invert on -x and negated again.  Refused: f or g that is not finite and positive (f as fp32). */
int icl_intensity_point(float* image, const float* stats, const double* params, int batch, int R0, int R1, int R2, void* stream);

/* ---- on-device RandomGenerator of the 2-D trainers (dataloaders/dataset.py:147-166; composed at
 * train_inherent_consistent_unet_2D.py:75 and ..._swinunet_2D.py): "maybe rot90 + flip, else maybe ndimage.rotate by an integer
 * angle, then ndimage.zoom to the patch", all order 0, as ONE gather over slices resident in HBM, bit for bit scipy's result.
 * images[b] / labels[b]: HOST arrays of device pointers to the fp32 [n0,n1] slice and its uint8 label; int_params: HOST int32
 * [batch][5] = {n0, n1, branch (0 none, 1 rot90 + flip, 2 rotate), k (np.rot90 count, 0..3), flip axis (0, 1)}; double_params:
 * HOST double [batch][8] = {M00, M01, M10, M11, off0, off1 (rotate: [[cos, sin], [-sin, cos]] and centre - M @ centre), z0, z1
 * (zoom: (r - 1) / (o - 1) of the extents r after rot90)}, drawn by the caller with the reference's call sequence
 * (icl_amd.dataloaders.dataset.draw_generator).  image_out [batch,1,o0,o1] fp32, label_out [batch,o0,o1] uint8.  batch <= 32. */
int icl_slice_augment(const void* const* images, const void* const* labels, const int32_t* int_params, const double* double_params,
                      int batch, float* image_out, uint8_t* label_out, int o0, int o1, void* stream);
/* scipy.ndimage.zoom(slice, (o0 / n0, o1 / n1), order=0) of `batch` slices [n0,n1] -> [o0,o1] sharing one extent: both resizes of the
 * 2-D validation loop (val_2D.py:41,48).  elem_kind 0: fp32 (the slices going in), 1: int64 (the arg-max maps going
 * back).  Zero last rows / columns where scipy's coordinate overshoots the source extent are reproduced. */
int icl_slice_resize(const void* src, void* dst, int64_t batch, int n0, int n1, int o0, int o1, int elem_kind, void* stream);

/* ---- fused SGD(momentum, weight decay) step, torch.optim.SGD semantics (train_inherent_consistent_unet_3D_BraTS.py:85-86,115):
 * d = g + wd*p; m = first ? d : momentum*m + d; p -= lr*m.  The multi form takes HOST arrays of device pointers.
 * lr_dev (may be NULL): when given, the learning rate is read from this device scalar instead of `lr` (hipGraph replay). */
int icl_sgd_step(float* p, const float* g, float* m, int64_t n, float lr, float momentum, float weight_decay, int first,
                 const float* lr_dev, void* stream);
/* The same step for a Linear weight p [n, k] whose gradient is still factored, dW[n][k] = sum_{r < rows} g[r][n] * x[r][k]
 * (g [rows, n] = dL/dy, x [rows, k] = the layer input): the 13,824^2 token-axis MLP weights of Class_Decoder.mlp2
 * (networks/unet_3D_icl.py:258,267) are updated in one pass over p and m without ever forming the 764 MB gradient. */
int icl_sgd_step_factored(float* p, float* m, const float* g, const float* x, int rows, int n, int k, float lr, float momentum,
                          float weight_decay, int first, const float* lr_dev, void* stream);
/* The same update for MANY factor rows (gathered factors of a data-parallel step, nc = 16: 64 ... 1536 rows): d = g^T x on the bf16
 * matrix pipe from exact three-way bf16 splits of both factors (six MFMA terms per product, fp32 accumulation — fp32 accuracy), so
 * that the update stays an HBM stream (0.86 -> ~0.6 ms at 128 rows on a 13,824^2 matrix).  ws: icl_sgd_factored_split_ws_bytes. */
int64_t icl_sgd_factored_split_ws_bytes(int rows, int n, int k);
int icl_sgd_step_factored_split(float* p, float* m, const float* g, const float* x, void* ws, int rows, int n, int k, float lr,
                                float momentum, float weight_decay, int first, const float* lr_dev, void* stream);
/* icl_sgd_step_factored for <= 16 factor rows as a NARROW persistent launch: `workgroups` workgroups of 1,024 threads (one CU each) walk the
 * matrix, so that the 16 B / weight stream can run under the under-filled launches of the deep backward levels without taking their CUs
 * (FusedSGD.update_placement "deep"; same sums in the same order as icl_sgd_step_factored: bit-identical).  Returns 1 (nothing launched)
 * for more than 16 rows. */
int icl_sgd_step_factored_narrow(float* p, float* m, const float* g, const float* x, int rows, int n, int k, float lr, float momentum,
                                 float weight_decay, int first, const float* lr_dev, int workgroups, void* stream);
int icl_sgd_step_multi(void* const* p, const void* const* g, void* const* m, const int64_t* n, int count, float lr,
                       float momentum, float weight_decay, int first, const float* lr_dev, void* stream);

/* ---- fused AdamW step, torch.optim.AdamW semantics (amsgrad = False, maximize = False), per fp32 element (csrc/kernels/adamw.h):
 *   p1 = p*decay;  m' = m + (g - m)*omb1;  v' = v*beta2 + omb2*g*g;  denom = sqrt(v')/bc2_sqrt + eps;  p' = p1 - step_size*(m'/denom)
 * The caller forms decay = 1 - lr*wd, step_size = lr/(1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), omb1 = 1 - beta1, omb2 = 1 - beta2
 * in double and rounds each ONCE to fp32 (1 - beta is never formed in fp32).  IEEE sqrt and division.
 * first != 0: m and v count as 0 and are never read (the state may be uninitialised memory); they are written.
 * hyper_dev (may be NULL): when given, {decay, step_size, bc2_sqrt} are read from these three device floats instead of the by-value
 * arguments (hipGraph replay, as lr_dev of the SGD entries).
 * Bad arguments — a null p / g / m / v, n < 1 — return non-zero with icl_last_error() set and launch nothing. */
int icl_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float decay, float step_size, float bc2_sqrt, float beta2,
                   float omb1, float omb2, float eps, int first, const float* hyper_dev, void* stream);
/* The same step for `count` tensors: HOST arrays of device pointers and element counts, 48 tensors per launch (longer lists are split).
 * One set of scalars and one `first` serve the whole list.  Bad arguments — a null array, count < 1, a null pointer or n[i] < 1 in
 * ANY entry — return non-zero with icl_last_error() set and launch nothing (the list is checked before the first launch). */
int icl_adamw_step_multi(void* const* p, const void* const* g, void* const* m, void* const* v, const int64_t* n, int count, float decay,
                         float step_size, float bc2_sqrt, float beta2, float omb1, float omb2, float eps, int first,
                         const float* hyper_dev, void* stream);
/* The same step for a Linear weight p [n, k] whose gradient is still factored, gg[n][k] = sum_{r < rows} g[r][n] * x[r][k] (g [rows, n],
 * x [rows, k]; fp32 sums in row order): one pass over p, m and v (24 B per weight) without ever forming the gradient.  Any rows >= 1.
 * Bad arguments — a null pointer, rows < 1, n < 1, k % 4 != 0, or p / m / v / x not 16-byte aligned — return non-zero with
 * icl_last_error() set and launch nothing. */
int icl_adamw_step_factored(float* p, float* m, float* v, const float* g, const float* x, int rows, int n, int k, float decay,
                            float step_size, float bc2_sqrt, float beta2, float omb1, float omb2, float eps, int first,
                            const float* hyper_dev, void* stream);

/* ---- gradient clipping by the global 2-norm, torch.nn.utils.clip_grad_norm_ semantics (csrc/kernels/gradclip.h).  The norm is measured
 * from dense gradients and from gradients that are still factored (G = g^T x) without multiplying them out:
 *   |g^T x|_F^2 = sum_{r,s} (g_r . g_s)(x_r . x_s)
 * Every square, product and sum is formed in double; every workgroup writes one double to a slot fixed by its index (no atomics, fixed
 * summation order: two runs give the same bits).  The caller lays the partial sums of all its calls out in ONE array of doubles and
 * finishes with icl_gradclip_finish; the scale kernels read the coefficient from device memory, so nothing returns to the host.
 * Bad arguments return non-zero with icl_last_error() set and launch nothing.
 *
 * icl_gradclip_sumsq: `count` tensors (HOST arrays of device pointers and element counts, 48 per launch), `chunks` workgroups each
 * (1 .. 4096): partial[i * chunks + c] = workgroup c's share of sum g_i^2; writes count * chunks doubles.  A pointer that is not
 * 16-byte aligned takes a scalar path. */
int icl_gradclip_sumsq(const void* const* g, const int64_t* n, int count, int chunks, double* partial, void* stream);
/* g [rows, n], x [rows, k] (fp32, contiguous; 1 <= rows <= 1024, any n >= 1, k >= 1): partial Gram entries per slab of the long axes in
 * `ws` (icl_gradclip_factored_ws_bytes bytes, 8-byte aligned), summed in slab order and combined to icl_gradclip_factored_parts(rows)
 * doubles in `partial`, whose sum is |g^T x|_F^2. */
int64_t icl_gradclip_factored_ws_bytes(int rows, int n, int k);
int icl_gradclip_factored_parts(int rows);
int icl_gradclip_sumsq_factored(const float* g, const float* x, int rows, int n, int k, void* ws, double* partial, void* stream);
/* One workgroup: clip_dev[0] = total_norm = (float)sqrt(sum of partial[0 .. count)), rounded once; clip_dev[1] = coef =
 * min(1, max_norm / (total_norm + 1e-6f)) evaluated in fp32 (torch's operations; a NaN norm gives a NaN coefficient, an infinite one 0). */
int icl_gradclip_finish(const double* partial, int64_t count, float max_norm, float* clip_dev, void* stream);
/* dst[i] = src[i] * clip_dev[1] for `count` tensors (48 per launch, `chunks` workgroups each), in place (dst == src) or out of place.
 * In place with a coefficient of exactly 1 nothing is read or written. */
int icl_gradclip_scale(void* const* dst, const void* const* src, const int64_t* n, int count, int chunks, const float* clip_dev,
                       void* stream);

/* ---- the aligner's QUERY chain as fused stages (round 6; csrc/kernels/qchain.h).  Replaces, per resolution level of
 * InherentConsistent, the operator-by-operator mirror of Class_Decoder's query half — norm1_query -> attn.fc_q -> [read-out of
 * softmax(QK^T)V: icl_attn_fwd / icl_attn_bwd_ws] -> attn.proj -> q + drop_path(q) -> norm2 -> mlp.fc1 -> GELU -> mlp.fc2 ->
 * q + drop_path(.) -> query_convs (networks/unet_3D_icl.py:258-264, 283-297, 299-315, 197/220-222) — on tensors of <= 32 rows
 * (batch * classes) by <= 256 channels: one stage launch = rows -> row prologue -> slice of a product with ONE weight matrix ->
 * element epilogue -> rows.  The struct is plain C (pointers, sizes; device pointers unless stated).
 *   trans 0: y[R][N] = epi(pro(x)[R][K] W[N][K]^T + bias)     (a Linear's forward; K % 4 == 0, K <= 1024)
 *   trans 1: y[R][N] = epi(pro(x)[R][K] W[K][N])               (its input gradient; N % 4 == 0, K <= 1024)
 *   trans 2: y[R][K] = epi(pro(x))                             (no product; epi 5: y[nc][K] = sum over samples, R <= 8)
 *   pro 0 none | 1 LayerNorm(pa = gamma, pb = beta; so0 <- xhat, so1 <- rstd, so2 <- result) | 2 GELU (so2 <- result) |
 *       3 LayerNorm backward (x = d(normalised), pa = xhat, pb = rstd, pc = gamma, + pd residual rows, x (1 + f0) if pro_dp; so2 <- result) |
 *       4 rows x f1 (so2 <- result)
 *   epi 0 none | 1 x (1 + f0) | 2 ea[r][n] + f1 * v | 3 v * gelu'(ea[r][n]) | 4 + ea rows on [ea_r0, ea_r1), + eb rows on [eb_r0, eb_r1) |
 *       5 (trans 2) sum over the batch
 *   f0 / f1: the per-sample drop-path factors of the two residual sites (keep ? 1/(1-p) : 0; thresh 0, scale 1 = inactive = 1),
 *   same hash as icl_drop_path (sample index as the counter), dp_seed_dev as there.  R <= 32; sample of row r = r / nc.
 *   x_rows (0 = R): row r reads x row r % x_rows (a [1, nc, C] query broadcast over the batch). */
typedef struct IclQcStage {
  const float* x; int x_rows;
  const float* w; const float* bias; float* y;
  int R, K, N, trans, nc, npw;       /* npw: filled in by the launcher */
  int pro, epi;
  const float* pa; const float* pb; const float* pc; const float* pd; int pro_dp;
  float* so0; float* so1; float* so2;
  const float* ea; const float* eb; int ea_r0, ea_r1, eb_r0, eb_r1;
  uint32_t dp_seed[2], dp_thresh[2]; float dp_scale[2]; const uint32_t* dp_seed_dev;
  float eps;
} IclQcStage;
int icl_qchain_stage(const IclQcStage* stage, void* stream);
/* Every parameter gradient of a level in ONE launch (they are leaves of the chain).  Job arrays are HOST arrays of `count` (<= 12) entries:
 * kind 0: dw[N][K] = g[R][N]^T x[R][K], db[N] = column sums of g (db[i] may be NULL)  — Linear weight / bias;
 * kind 1: dw[K] = sum_r g[r][k] x[r][k], db[K] = sum_r g[r][k]                         — LayerNorm gamma / beta from (d(normalised), xhat). */
int icl_qchain_wgrad(const void* const* g, const void* const* x, void* const* dw, void* const* db, const int32_t* rows, const int32_t* n,
                     const int32_t* k, const int32_t* kind, int count, void* stream);

/* ---- validation metrics: Dice and HD95 counts of every foreground class (val_3D.py:85-97, val_2D.py:10-22: cal_metric /
 * calculate_metric_percase -> medpy.metric.binary.dc / hd95 on `label == c`, `prediction == c`; restated in icl_amd/val_3D.py).
 * pred / gt: dense [n0][n1][n2] label maps (axis 2 fastest), element size pred_dtype / gt_dtype: 1 = uint8 (h5 labels), 8 = int64 (argmax); a
 * voxel belongs to class c (1 <= c < num_classes) when its label equals c, other labels belong to no class.  all_border = 1: the maps
 * carry further axes of length 1 (the AMOS path scores [1, D, H, W] arrays), so every voxel of a class is a surface voxel.
 * out: DEVICE int64 [num_classes - 1][6], row c - 1 = {|P|, |G|, |P & G|, n = |dP| + |dG|, s0, s1}: dP / dG the border voxels
 * (S ^ binary_erosion(S, connectivity 1), voxels on the volume faces included), s0 / s1 the squared surface distances of ranks
 * k0 = floor(0.95 (n - 1)) and k0 + 1 in the sorted union of both directed sets (-1 when |P| = 0 or |G| = 0).  Exact integers: the host
 * forms dice = 2 |P & G| / (|P| + |G|) and hd95 = numpy's linear interpolation between sqrt(s0) and sqrt(s1) (bit-equal to
 * np.percentile(np.hstack((a, b)), 95)).  2 <= num_classes <= 256; ws: icl_seg_metrics_ws_bytes bytes (-1: shape not supported),
 * about 10 bytes per voxel.  About 7 (num_classes - 1) + 3 launches, no synchronisation. */
int64_t icl_seg_metrics_ws_bytes(int n0, int n1, int n2, int num_classes);
int icl_seg_metrics(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int n0, int n1, int n2, int num_classes, int all_border,
                    int64_t* out, void* ws, void* stream);

/* ---- surface metrics with a voxel spacing, every foreground class (csrc/kernels/metrics_surface.h).  Replaces
 * medpy.metric.binary.hd95 / hd / asd / assd called with `voxelspacing` (the reference's val_3D.py:85-97 / val_2D.py:10-22 call hd95 without
 * it, so its HD95 is in voxel units), and the voxel-border NSD; restated in icl_amd/val_3D.py (binary_hd95, binary_hd, binary_asd,
 * binary_assd, binary_nsd).  pred / gt, dtypes and class rule as icl_seg_metrics; the maps are exactly 3-D.  (s0, s1, s2): the voxel
 * spacing along n0, n1, n2, finite and positive; tolerance: the NSD tolerance tau in the spacing's units, finite and >= 0.
 * counts: DEVICE int64 [num_classes - 1][7], row c - 1 = {|P|, |G|, |P & G|, |dP|, |dG|, #{p in dP: d(p, dG)^2 <= tau^2},
 * #{g in dG: d(g, dP)^2 <= tau^2}}.  values: DEVICE double [num_classes - 1][6], row c - 1 = {sq[k0], sq[k0 + 1], max d^2 (dP -> dG),
 * max d^2 (dG -> dP), sum d (dP -> dG), sum d (dG -> dP)}: sq the sorted union of the squared distances sum_a ((double)delta_a s_a)^2 of
 * both directions, k0 = floor(0.95 (n - 1)), n = |dP| + |dG|; every value is -1 when dP or dG is empty.  The squares are exact distance
 * transform values (each product and sum rounded once, no contraction); the host takes the roots of the two order statistics and of the
 * maxima.  The sums are added in a fixed order: two calls are bit-equal.  2 <= num_classes <= 256; ws: icl_seg_surface_ws_bytes bytes
 * (-1: shape not supported), 34 bytes per voxel plus about 150 KiB.  15 (num_classes - 1) + 3 launches, no synchronisation.  A bad
 * argument (also a non-finite or non-positive spacing, a negative or non-finite tolerance) returns -1 and launches nothing. */
int64_t icl_seg_surface_ws_bytes(int n0, int n1, int n2, int num_classes);
int icl_seg_surface_metrics(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int n0, int n1, int n2, int num_classes, double s0,
                            double s1, double s2, double tolerance, int64_t* counts, double* values, void* ws, void* stream);

/* ---- connected components of a label map, every foreground class in one labelling, and the keep-largest / minimum-size filter that
 * validation pipelines apply between the arg-max and the scores (csrc/kernels/components.h; scipy.ndimage.label once per class on the host,
 * restated in icl_amd/val_3D.py keep_components).  map: dense [n0][n1][n2] label map (axis 2 fastest), element size dtype: 1 = uint8,
 * 8 = int64; class rule as icl_seg_metrics.  Two neighbouring voxels belong to one component when they carry the same class;
 * connectivity 1 / 2 / 3: 6 / 18 / 26 neighbours (scipy.ndimage.generate_binary_structure(3, connectivity)).
 * labels: DEVICE int32 [n0 n1 n2]: 0 on background, else 1 + the linear index of the component's first voxel in raster order — a function
 * of the map alone; two calls are bit-equal.  counts: DEVICE int64 [num_classes - 1][3], row c - 1 = {components of class c, voxels in
 * the largest, label of the largest (0 when the class is absent)}; among components of equal size the one whose first voxel comes first
 * counts as the largest (np.argmax over scipy's sizes).
 * icl_seg_filter_components: out[v] = the class of v when its component is kept, else 0 (labels outside 1..num_classes-1 are background
 * and come out as 0); a component is kept iff (keep_largest == 0 or it is its class's largest) and its voxel count >= min_size.  out:
 * DEVICE, the map's element size; it may be the map itself.  counts may be NULL there.
 * 2 <= num_classes <= 256, n0 n1 n2 <= 2^31 - 2; ws: icl_seg_components_ws_bytes bytes (-1: shape not supported), 12 bytes per voxel plus
 * about 780 KiB.  5 launches (6 with the filter) whatever the data and num_classes, no synchronisation, no workgroup waits for another.  A bad
 * argument (also a connectivity outside 1..3, a negative min_size, an element size other than 1 / 8, a null pointer) returns -1 and
 * launches nothing. */
int64_t icl_seg_components_ws_bytes(int n0, int n1, int n2, int num_classes);
int icl_seg_components(const void* map, int dtype, int n0, int n1, int n2, int num_classes, int connectivity, int32_t* labels, int64_t* counts,
                       void* ws, void* stream);
int icl_seg_filter_components(const void* map, int dtype, int n0, int n1, int n2, int num_classes, int connectivity, int keep_largest,
                              int64_t min_size, void* out, int64_t* counts /* may be NULL */, void* ws, void* stream);

/* ---- the 3-D sliding window of the validation loops on the device (csrc/kernels/window.h; val_3D.py:18-73: test_single_case_base's pad,
 * window grid, soft-max, score / count maps, divide, arg-max and crop; val_3D.py:128-132: monai.inferers.sliding_window_inference as the
 * AMOS loop calls it; both restated in icl_amd/val_3D.py).  Volumes are dense with the last axis fastest.  origins: HOST int32 [n][3], the
 * windows' origins in the PADDED frame p0 x p1 x p2 (copied into the kernel arguments), n <= 16 windows of extent r0 x r1 x r2; the unpadded
 * volume s0 x s1 x s2 starts at (a0, a1, a2) of the padded frame.  Each call returns -1 (nothing launched, icl_last_error() says why) for
 * n outside 1..16, classes outside 1..256, or an origin that puts a window outside the padded extent.
 * icl_window_gather (val_3D.py:18-41,57-62 and :128-132; replaces F.pad + one slice per window + stack + contiguous, bit-equal):
 *   out [n][cin][r0][r1][r2] <- vol [cin][s0][s1][s2], voxels outside the unpadded volume read as 0. */
int icl_window_gather(const float* vol, float* out, const int32_t* origins, int n, int cin, int s0, int s1, int s2, int a0, int a1, int a2,
                      int p0, int p1, int p2, int r0, int r1, int r2, void* stream);
/* icl_window_gather_flipped (mirror test-time augmentation): icl_window_gather with one mirror mask per window, flips: HOST int32 [n], bit a
 *   set = axis a of the window mirrored (0 .. 7; copied into the kernel arguments).  out[w] = flip(window w, the axes of flips[w]), bit-equal
 *   to torch.flip of icl_window_gather's window, zero fill included: the same gather with a reversed source index, no second tensor.  A
 *   mask outside 0..7 returns -1 (nothing launched), as does everything icl_window_gather refuses. */
int icl_window_gather_flipped(const float* vol, float* out, const int32_t* origins, const int32_t* flips, int n, int cin, int s0, int s1,
                              int s2, int a0, int a1, int a2, int p0, int p1, int p2, int r0, int r1, int r2, void* stream);
/* icl_window_accumulate (val_3D.py:63-70 and :128-132): score [c][p0][p1][p2] and weight [p0][p1][p2] += the batch's windows, logits
 *   [n][c][r0][r1][r2].  One thread owns a destination voxel and walks the windows in their given order: the adds are those of the loop
 *   over windows, in its order, with no atomics; the launch covers the bounding box of the windows.  softmax != 0: the value added is the
 *   soft-max over the class axis of the window's logits (the BraTS loop), else the logits (the AMOS loop).  importance == NULL:
 *   score += value, weight += 1; else importance [r0][r1][r2]: score = score + importance * value (product and sum rounded one after the
 *   other, never fused), weight += importance. */
int icl_window_accumulate(const float* logits, const float* importance, float* score, float* weight, const int32_t* origins, int n, int c,
                          int p0, int p1, int p2, int r0, int r1, int r2, int softmax, void* stream);
/* icl_window_accumulate_flipped (mirror test-time augmentation): icl_window_accumulate for logits computed on mirrored windows, flips as in
 *   icl_window_gather_flipped.  The value of window w is mirrored back along the axes of flips[w] as it is read — score[:, window] +=
 *   flip(value, axes) — in the same order and with the same roundings; the importance map is NOT mirrored: it is indexed in the volume's
 *   frame.  A mask outside 0..7 returns -1 (nothing launched), as does everything icl_window_accumulate refuses. */
int icl_window_accumulate_flipped(const float* logits, const float* importance, float* score, float* weight, const int32_t* origins,
                                  const int32_t* flips, int n, int c, int p0, int p1, int p2, int r0, int r1, int r2, int softmax,
                                  void* stream);
/* icl_window_finalize (val_3D.py:71-73 and :128-132): label [s0][s1][s2] int64 = arg-max over the classes of score / weight (IEEE fp32
 *   division; the lowest index wins among equals, NaN as torch.argmax treats it) on the unpadded extent; quotients (may be NULL): the
 *   quotients themselves, cropped, [c][s0][s1][s2] — where nothing is cropped they may be `score` itself (division in place).  label may
 *   be NULL when the quotients are all that is wanted. */
int icl_window_finalize(const float* score, const float* weight, int64_t* label, float* quotients, int c, int p0, int p1, int p2, int a0,
                        int a1, int a2, int s0, int s1, int s2, void* stream);

#ifdef __cplusplus
}
#endif
#endif
