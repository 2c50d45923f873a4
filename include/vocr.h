/*
 * vocr.h — C-ABI of libvocr.so: the MI355X (gfx950) kernels behind VistaOCR's CnnOcrModel hot path.
 *
 * The reference (isi-vista/VistaOCR) is pure Python and has NO FFI of its own: every entry point below
 * replaces a PyTorch/cuDNN/warp-ctc call that the reference makes from Python.  Each declaration cites the
 * reference call site it stands in for (paths under /root/reference/).  INTEGRATION.md shows the ctypes
 * binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, ints, floats; `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 on success, a negative VOCR_E* code otherwise; vocr_last_error() returns a
 *     thread-local message.  No C++ exception crosses the boundary.
 *   - the caller owns every buffer; the library allocates nothing and never synchronises the stream.
 *   - tensors are contiguous fp32 unless stated; images NCHW; sequences time-major [T,B,...].
 */
#ifndef VOCR_H
#define VOCR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VOCR_OK          0
#define VOCR_EINVAL     -1   /* bad argument (shape, null pointer, unsupported size) */
#define VOCR_ELAUNCH    -2   /* HIP launch error */
#define VOCR_ENODEVICE  -3   /* no gfx950 device visible */
#define VOCR_ECOMM      -4   /* RCCL missing or a collective failed */

/* "health" words: an optional caller-owned int32[2] in device memory.  The library only ever SETS them (report-only: no
 * kernel's result depends on their value), the caller zeroes them — once, and again after it has handled a report.
 *   health[0] != 0: a hand-off inside a persistent LSTM sweep timed out (THAT sweep's output is NaN-poisoned: the sweep
 *                   decides on a per-call word in its workspace, so later sweeps are unaffected);
 *   health[1] != 0: a NaN gradient reached vocr_clamp_adam / vocr_clamp (the reference's clamp_ propagates NaN too).
 * The host reads it whenever it synchronises anyway (vistaocr_amd.train() copies it next to the loss and clears it
 * before raising; vistaocr_amd.ops.reset_health() clears it explicitly). */

const char* vocr_last_error(void);
/* The contract this header describes.  History: 2 = round 2 (caller-owned health word); 3 = round 3/4 (health words report-only and
 * cleared by the caller, LSTM workspace survives between the vocr_lstm_fwd_range calls of a sweep, larger vocr_gemm_workspace_bytes,
 * vocr_gemm_pair / vocr_lstm_bwd_parts / vocr_profile_range_*, x-fastest conv weight pack); 4 = round 5 (packed sequence rows:
 * vocr_lstm_*_packed, vocr_seq_rowmap, vocr_gather_rows; VOCR_LSTM_SWEEP validated; experiment switches compiled out); 5 = round 6
 * (vocr_dropout_mask, and the next layer's x-projection behind the forward sweep); 6 = that x-projection path removed again, slower
 * than the GEMM in every form it was built in: four entry points for the follower waves, their weight pack, its size and their shape
 * query are gone, and a forward sweep reads one x-projection.  A binding compares vocr_abi_version()
 * with the VOCR_ABI_VERSION it was written against and refuses a library that answers anything else. */
#define VOCR_ABI_VERSION 6
int  vocr_abi_version(void);
/* Named ranges on the profiler's timeline (rocprofv3 --marker-trace), nested push / pop on the calling thread.  roctx is dlopen'ed on
 * first use; returns 0 when the range was recorded, 1 when roctx is not available (not an error), negative on a bad argument.  The
 * reference's only instrumentation is wall-clock prints around the step (src/train_cnn_lstm.py:382-393): the Python mirror marks the
 * same phases (forward / loss / backward / exchange / optimizer, and the model's stages) when VOCR_ROCTX=1. */
int  vocr_profile_range_push(const char* name);
int  vocr_profile_range_pop(void);
/* number of visible HIP devices (>=0) or VOCR_ENODEVICE */
int  vocr_device_count(void);

/* ---- convolution: nn.Conv2d(k=3, pad=1) — src/models/cnnlstm.py:118,264 ------------------------------ */
/* wpack_fwd[(ci*9+kh*3+kw)][co] = w[co][ci][kh][kw];  wpack_dgrad[(co*9+kh*3+kw)][ci] = w[co][ci][2-kh][2-kw] */
int vocr_conv3x3_pack_weights(const float* w, float* wpack_fwd, float* wpack_dgrad, int cout, int cin, void* stream);
/* y[n,co,h,w] = bias[co] + sum wpack[k][co] * x[n,ci,h+kh-1,w+kw-1]   (bias may be NULL).
 * dgrad is the same call with x=dy, cin=Cout, wpack=wpack_dgrad, cout=Cin, bias=NULL. */
int vocr_conv3x3_fwd(const float* x, const float* wpack, const float* bias, float* y,
                     int n, int cin, int h, int w, int cout, void* stream);
/* dw[co][ci][3][3] = sum_{n,h,w} dy[n,co,h,w] * x[n,ci,h+kh-1,w+kw-1];  workspace from *_workspace_bytes. */
size_t vocr_conv3x3_wgrad_workspace_bytes(int n, int cin, int h, int w, int cout);
int vocr_conv3x3_wgrad(const float* x, const float* dy, float* dw, void* workspace,
                       int n, int cin, int h, int w, int cout, void* stream);
/* Same op with a minimal-filtering transform ALONG THE ROW (conv_wino.hip), fp32 operands and accumulation: F(4,3) - half of the
 * direct form's multiplications - for a convolution with at least 64 output channels, F(2,3) - two thirds - below.  A weight pack is
 * OPAQUE: the transformed filter rows in the layout of the kernel that vocr_conv3x3_wino_fwd will pick for a convolution with THAT
 * many output channels, followed by the direct pack's 9 rows per channel (the last partial round of tiles is computed in the direct
 * form).  vocr_conv3x3_wino_pack_floats(cout, cin) = floats of the pack of a convolution with `cout` outputs and `cin` inputs
 * (cout*cin*27 or *21; the data-gradient pack of a layer is the pack of the convolution with cin outputs: ..._pack_floats(cin, cout)),
 * 16-byte aligned.  Needs cout % 4 == 0 (input channels are padded inside) (vocr_conv3x3_wino_supported).
 * dgrad = vocr_conv3x3_wino_fwd(dy, wpack_dgrad, NULL, dx, n, cout, h, w, cin).  Tensors below 2^29 elements. */
int vocr_conv3x3_wino_supported(int cin, int cout);
size_t vocr_conv3x3_wino_pack_floats(int cout, int cin);
int vocr_conv3x3_wino_pack_weights(const float* w, float* wpack_fwd, float* wpack_dgrad, int cout, int cin, void* stream);
/* which kernel vocr_conv3x3_wino_fwd takes for a launch (0: shape refused).  1 / 2 = F(2,3), 64 / 128 output channels per workgroup;
 * F(4,3): 3 / 4 = one 4-wave workgroup per CU, 5 / 6 = one 8-wave workgroup, 7 / 8 = two 4-wave workgroups per CU (64 / 128 channels);
 * 9 / 10 = the round-3 F(2,3) kernels (tensors of 2^29 elements or more).  +16: the last partial round of tiles is cut into direct-form
 * tail pieces that lead the launch.  A data gradient is the launch vocr_conv3x3_wino_plan(n, cout, h, w, cin). */
int vocr_conv3x3_wino_plan(int n, int cin, int h, int w, int cout);
int vocr_conv3x3_wino_fwd(const float* x, const float* wpack, const float* bias, float* y,
                          int n, int cin, int h, int w, int cout, void* stream);
/* Weight gradient with the transposed minimal-filtering transform F(3,2) along the row and - when cin * cout is a multiple of 4 -
 * across row pairs as well (16 multiplications per 2 x 2 block of gradient pixels and filter instead of 36; otherwise along the row
 * only: 4 per column pair instead of 6): same contract as vocr_conv3x3_wgrad, needs cin >= 4; the workspace (ask
 * vocr_conv3x3_wgrad_wino_workspace_bytes: it differs between the two forms) holds the split partial planes that a second kernel
 * adds in a fixed order - the result is bitwise reproducible. */
size_t vocr_conv3x3_wgrad_wino_workspace_bytes(int n, int cin, int h, int w, int cout);
int vocr_conv3x3_wgrad_wino(const float* x, const float* dy, float* dw, void* workspace,
                            int n, int cin, int h, int w, int cout, void* stream);
/* Round 5: one input channel (the first layer of a grey-line model, configs[4]'s rapid_ds stage) as plain vector arithmetic - the layer is
 * bound by writing its output once, not by 576 FLOP per pixel.  w = the layer's own weight [cout][1][3][3] (no pack), y fp32
 * [n][cout][h][wd] (+ bias); round_f16 != 0 rounds x and w to fp16 first (the fp16-operand configuration's arithmetic; fp32 accumulate
 * either way).  vocr_conv3x3_c1_wgrad: dw[cout][1][3][3] from x [n][1][h][wd] and dy [n][cout][h][wd], exact fp32, split partial sums
 * added in a fixed order (workspace: vocr_conv3x3_c1_wgrad_workspace_bytes); dbias[cout] (may be NULL) = the per-channel sum of dy, from
 * the same pass over dy. */
int vocr_conv3x3_c1_fwd(const float* x, const float* w, const float* bias, float* y, int n, int h, int wd, int cout, int round_f16,
                        void* stream);
size_t vocr_conv3x3_c1_wgrad_workspace_bytes(int n, int h, int cout);
int vocr_conv3x3_c1_wgrad(const float* x, const float* dy, float* dw, float* dbias, void* workspace, int n, int h, int wd, int cout,
                          void* stream);
/* fp16-operand variant (BASELINE config 5: "fp16 conv MFMA", fp32 accumulate): tensors stay fp32 in HBM, operands are
 * rounded to fp16 on the way into the matrix cores (v_mfma_f32_32x32x16_f16).  Weight packs are fp16:
 * fwd  [ceil(cin/16)][9][2][cout][8],  dgrad [ceil(cout/16)][9][2][cin][8] (taps flipped); sizes from *_pack_bytes.
 * dgrad = vocr_conv3x3_f16_fwd(dy, wpack_dgrad, NULL, dx, n, cout, h, w, cin).
 * vocr_conv3x3_wgrad_f16: same contract and workspace as vocr_conv3x3_wgrad, dy and x rounded to fp16 for the MFMA. */
size_t vocr_conv3x3_f16_pack_bytes(int cout, int cin, int dgrad);
int vocr_conv3x3_f16_pack_weights(const float* w, void* wpack_fwd, void* wpack_dgrad, int cout, int cin, void* stream);
int vocr_conv3x3_f16_fwd(const float* x, const void* wpack, const float* bias, float* y,
                         int n, int cin, int h, int w, int cout, void* stream);
int vocr_conv3x3_wgrad_f16(const float* x, const float* dy, float* dw, void* workspace,
                           int n, int cin, int h, int w, int cout, void* stream);
/* Round 5: the same fp16-operand convolution on a channel-blocked fp16 copy of the activation, x16 = [n][cin/16][h][w][16] (cin % 16 == 0;
 * ask vocr_conv3x3_h16_supported): the 16 channels of a block are 32 contiguous bytes per pixel and consecutive pixels follow each
 * other, so the kernel's 16-byte LDS-DMA pieces use whole cache lines.  vocr_f32_to_f16_layouts (below) writes the copy in one HBM-bound
 * pass per use.  vocr_conv3x3_h16_fwd: x16 in that layout, the weight packs of vocr_conv3x3_f16_pack_weights, y fp32 [n][cout][h][w]
 * (+ bias): every operand reaches LDS by DMA and the loop holds nothing but MFMAs and their fragment reads.  Results equal
 * vocr_conv3x3_f16_fwd's bit for bit (same operand rounding, same summation order per output).
 * dgrad = vocr_conv3x3_h16_fwd(dy16, wpack_dgrad, NULL, dx, n, cout, h, w, cin). */
int vocr_conv3x3_h16_supported(int cin, int cout);
/* which forward / data-gradient kernel vocr_conv3x3_h16_fwd takes for a launch (0: shape not taken; 1 = 64-channel tile of 16 rows x 32
 * pixels; 2 / 3 / 4 = 128 channels x 8 / 12 / 16 rows x 32 pixels; 5 = 128 channels x 8 rows x 64 pixels): the tests assert that every
 * variant a BASELINE configuration runs is seen by them */
int vocr_conv3x3_h16_plan(int n, int cin, int h, int w, int cout);
int vocr_conv3x3_h16_fwd(const void* x16, const void* wpack, const float* bias, float* y,
                         int n, int cin, int h, int w, int cout, void* stream);
/* Round 5, weight gradient with fp16 operands: both operands as channel-major fp16 copies [n][c][h][WP] whose rows are zero-padded to
 * WP = vocr_f16_padded_row(w) = ceil8(w) + 8 (8 consecutive pixels of a channel = 16 bytes = what a lane half of the MFMA needs when the
 * contraction runs over pixels; the zero tail is every row's right AND the next row's left halo).  vocr_f32_to_f16_layouts writes the
 * channel-blocked copy [n][c/16][h][w][16] (`nhwc`, may be NULL; needs c % 16 == 0) and / or the padded channel-major one (`nchwp`, may
 * be NULL) in ONE pass over the fp32 tensor (c % 8 == 0).
 * vocr_conv3x3_wgrad_h16: x16p [n][cin][h][WP], dy16p [n][cout][h][WP] -> dw[cout][cin][3][3] fp32; cin % 64 == 0 and cout 64 or a
 * multiple of 128 (ask vocr_conv3x3_wgrad_h16_supported); workspace = split slabs added in a fixed order (bitwise reproducible).
 * Same arithmetic as vocr_conv3x3_wgrad_f16 (operands rounded to fp16, fp32 accumulate), another summation order. */
int vocr_f16_padded_row(int w);
int vocr_f32_to_f16_layouts(const float* x, void* nhwc, void* nchwp, int n, int c, int h, int w, void* stream);
int vocr_conv3x3_wgrad_h16_supported(int cin, int cout);
size_t vocr_conv3x3_wgrad_h16_workspace_bytes(int n, int cin, int h, int w, int cout);
int vocr_conv3x3_wgrad_h16(const void* x16p, const void* dy16p, float* dw, void* workspace,
                           int n, int cin, int h, int w, int cout, void* stream);
/* per-channel sum over (n,h,w): conv bias gradient.  out[c].  workspace (vocr_channel_sum_workspace_bytes, may be NULL =
 * one workgroup per channel) holds per-chunk partial sums that are added in a fixed order: bitwise reproducible. */
size_t vocr_channel_sum_workspace_bytes(int n, int c, int hw);
int vocr_channel_sum(const float* x, float* out, int n, int c, int hw, void* workspace, void* stream);

/* ---- BatchNorm2d + ReLU — src/models/cnnlstm.py:265-266 -------------------------------------------------- */
/* training statistics: mean[c], invstd[c] (biased var, eps) and running-stat update (momentum, unbiased var);
 * *num_batches_tracked (device int64) += 1; xhat_sum[c] = sum over the batch of (y-mean)*invstd (the rounding residue of the
 * fp32 mean; the backward turns it into the conv-bias gradient).  running_mean/var, num_batches_tracked, xhat_sum may be NULL.
 * workspace: 2*c*nchunk doubles, see vocr_bn_workspace_bytes. */
size_t vocr_bn_workspace_bytes(int n, int c, int hw);
int vocr_bn_train_stats(const float* y, int n, int c, int hw, float eps, float momentum,
                        float* mean, float* invstd, float* running_mean, float* running_var,
                        int64_t* num_batches_tracked, float* xhat_sum, void* workspace, void* stream);
/* eval: mean/invstd from running stats */
int vocr_bn_eval_stats(const float* running_mean, const float* running_var, int c, float eps,
                       float* mean, float* invstd, void* stream);
/* out = relu((y-mean)*invstd*gamma + beta), the ReLU as `v > 0 ? v : 0`: a NaN pre-activation (a NaN in y or in a statistic) comes out
 * as 0, where torch's relu would keep the NaN.  The same holds for every fused forward below that contains this pass. */
int vocr_bn_relu_apply(const float* y, const float* mean, const float* invstd, const float* gamma,
                       const float* beta, float* out, int n, int c, int hw, void* stream);
/* Training-mode BatchNorm2d + ReLU of a layer in TWO launches instead of three (round 4): the statistics pass leaves per-chunk
 * partial sums in `workspace` (vocr_bn_workspace_bytes) and every workgroup of the apply pass adds its channel's chunks itself, in
 * chunk order - bit-identical to vocr_bn_train_stats followed by vocr_bn_relu_apply (src/models/cnnlstm.py:265-266), without the
 * "final" launch and its two kernel boundaries on the forward's critical path.  mean / invstd / xhat_sum (saved for the backward)
 * and the running statistics / num_batches_tracked are written as vocr_bn_train_stats writes them. */
int vocr_bn_train_relu_apply(const float* y, const float* gamma, const float* beta, float* out, int n, int c, int hw, float eps,
                             float momentum, float* mean, float* invstd, float* running_mean, float* running_var,
                             int64_t* num_batches_tracked, float* xhat_sum, void* workspace, void* stream);
/* The same for a layer followed by FractionalMaxPool2d (vocr_bn_relu_fracpool2x2_fwd's pass, src/models/cnnlstm.py:127,130):
 * bit-identical to vocr_bn_train_stats followed by vocr_bn_relu_fracpool2x2_fwd.  A NaN or an infinity in y makes its channel's
 * statistics non-finite; every activation of that channel is then 0 (see vocr_bn_relu_apply) and every window elects its first pixel. */
int vocr_bn_train_relu_fracpool2x2_fwd(const float* y, const float* gamma, const float* beta, const float* samples, float* out,
                                       int32_t* idx, int n, int c, int h, int w, int oh, int ow, float eps, float momentum,
                                       float* mean, float* invstd, float* running_mean, float* running_var,
                                       int64_t* num_batches_tracked, float* xhat_sum, void* workspace, void* stream);
/* given da = dL/d(out): dgamma, dbeta and dy = dL/d(y) (training-mode batch-stat backward through ReLU);
 * dconv_bias (may be NULL) receives sum_{n,h,w} dy per channel = the gradient of the conv bias in front (rounding
 * noise around zero, from the fixed-order reduction: no float atomics anywhere in this call). */
int vocr_bn_relu_bwd(const float* da, const float* y, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, const float* xhat_sum, float* dy, float* dgamma, float* dbeta,
                     float* dconv_bias, int n, int c, int hw, void* workspace, void* stream);

/* ---- FractionalMaxPool2d(2, output_ratio=(0.5,0.7)) — src/models/cnnlstm.py:127,130 --------------------- */
/* samples[n][c][2] (u_w, u_h) as ATen's _random_samples; idx = flat h*W+w of the winner (int32).  1 <= oh <= h-1, 1 <= ow <= w-1
 * (out 1: the one window sits at in-2).  Bit for bit ATen's CPU op, non-finite inputs included (`val > max || isnan(val)`): a NaN
 * takes every window it lies in (the last NaN of several) and a window of four -inf keeps its first pixel. */
int vocr_fracpool2x2_fwd(const float* x, const float* samples, float* out, int32_t* idx,
                         int n, int c, int h, int w, int oh, int ow, void* stream);
/* BatchNorm-apply + ReLU + the same pooling in one pass over the conv output y (vocr_bn_relu_apply followed by
 * vocr_fracpool2x2_fwd, bit for bit), for layers whose activation is only ever consumed by the pool.  The pooled activation is
 * never NaN or negative: a NaN or -inf in y is 0 before the pool sees it (vocr_bn_relu_apply). */
int vocr_bn_relu_fracpool2x2_fwd(const float* y, const float* mean, const float* invstd, const float* gamma,
                                 const float* beta, const float* samples, float* out, int32_t* idx,
                                 int n, int c, int h, int w, int oh, int ow, void* stream);
/* Backward of vocr_bn_relu_fracpool2x2_fwd in one go: dout/idx are the pooled gradient and winner indices, samples the
 * forward's; returns dy = dL/d(conv output), dgamma, dbeta, dconv_bias like vocr_bn_relu_bwd, without materialising the
 * un-pooled gradient.  Needs window starts that strictly increase (vocr_bn_relu_fracpool2x2_bwd_supported: both
 * (in-2)/(out-1) >= 1.01 in float32, true for the reference's 0.5 x 0.7 ratios; w % 4 == 0; (2w + 8 + 2h) * 4 <= 65536 bytes of
 * LDS for the inverse window maps, met with equality at h = 4, w = 8184); otherwise use vocr_fracpool2x2_bwd + vocr_bn_relu_bwd.
 * A refused shape returns an error before anything is launched.  y and dy are read and written as 16-byte pixel groups. */
int vocr_bn_relu_fracpool2x2_bwd_supported(int h, int w, int oh, int ow);
int vocr_bn_relu_fracpool2x2_bwd(const float* dout, const int32_t* idx, const float* samples, const float* y,
                                 const float* mean, const float* invstd, const float* gamma, const float* beta,
                                 const float* xhat_sum, float* dy, float* dgamma, float* dbeta, float* dconv_bias,
                                 int n, int c, int h, int w, int oh, int ow, void* workspace, void* stream);
/* dx[n][c][h][w] = sum of dout over the windows whose winner is that pixel; every element of dx is written
 * (no zero-fill needed) */
int vocr_fracpool2x2_bwd(const float* dout, const int32_t* idx, float* dx,
                         int n, int c, int h, int w, int oh, int ow, void* stream);

/* ---- rapid_ds tail: ReLU + MaxPool2d(2,2) — src/models/cnnlstm.py:119-120 -------------------------------- */
/* out[n][c][h/2][w/2] = max over the 2x2 window of max(x, 0) (fmaxf: a NaN in x counts as 0, where torch propagates it), idx = flat
 * h*W+w of the first maximum; an odd last row / column is dropped.
 * The backward stores dout where out > 0 (else 0) at each winner and touches nothing else: dx must arrive ZERO-FILLED - the three
 * pixels of a window that did not win, and the dropped odd row / column, keep what the caller put there. */
int vocr_relu_maxpool2_fwd(const float* x, float* out, int32_t* idx, int n, int c, int h, int w, void* stream);
int vocr_relu_maxpool2_bwd(const float* dout, const float* out, const int32_t* idx, float* dx,
                           int n, int c, int h, int w, void* stream);

/* ---- dense layers: bridge Linear+ReLU, LSTM input projections, prob Linear — cnnlstm.py:143-154,278,294 -- */
/* C[M,N] (ldc) = op(A)[M,K] * op(B)[K,N] (+ bias[N]) (relu) — row-major.
 * transa=0: A is [M,K] lda;  transa=1: A is stored [K,M] lda.   transb=0: B is [K,N] ldb;  transb=1: B is [N,K] ldb.
 * accumulate!=0: C += result.  Long-K products with few output tiles (the weight gradients) are split along K: each
 * slice writes its own [M][N] slab into `workspace` (vocr_gemm_workspace_bytes; 16-byte aligned; may be NULL or smaller
 * = fewer or no slices) and the slabs are added in slice order — results are bitwise reproducible run to run. */
size_t vocr_gemm_workspace_bytes(int m, int n, int k, int has_bias_or_relu);
int vocr_gemm(int transa, int transb, int m, int n, int k,
              const float* a, int lda, const float* b, int ldb, float* c, int ldc,
              const float* bias, int relu, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* Which launch vocr_gemm (nprob = nseg = 1) or vocr_gemm_pair (mode 0: nprob = 2, nseg = 1; mode 1: nprob = 1, nseg = 2) takes for a call,
 * answered by the planner the two entry points launch from; touches no device memory (256 CUs are assumed when no device is visible).
 * aligned: bit 0 = a and b are 16-byte aligned, bit 1 = c and the biases are (3: every pointer).  workspace_bytes: what a 16-byte aligned
 * workspace holds (0: NULL).  tiles_only: vocr_gemm_pair's co-scheduling hint (mode | 4).  plan[VOCR_GEMM_PLAN_INTS]:
 *   [0] kernel: 0 / 1 / 2 = tile kernel with 64x64 / 128x64 / 128x128 tiles, 3 = DMA-staged panel kernel
 *   [1] 16-byte operand loads (1) or 4-byte ones (0; the panel kernel only has the 16-byte form)
 *   tile kernel:  [2] whole tiles that lead the launch (0: every tile is cut along K), [3] K pieces per cut tile (1: nothing is cut),
 *                 [4] k per piece
 *   panel kernel: [5] column panels, [6] row groups, [7] K splits (1: no slabs), [8] k per split, [9] the most 32-row tiles a group holds
 *   [10] launches of the product kernel: 1, or 2 when vocr_gemm_pair falls back to two vocr_gemm calls ([0] .. [4] then describe a call
 *        with the flags given here; ask for each call with nprob = nseg = 1 when their flags differ)
 *   [11] bytes of workspace the launch uses (K slabs) */
#define VOCR_GEMM_PLAN_INTS 12
int vocr_gemm_plan(int transa, int transb, int m, int n, int k, int lda, int ldb, int ldc, int aligned, int has_bias_or_relu,
                   int accumulate, size_t workspace_bytes, int nprob, int nseg, int tiles_only, int* plan);
/* Two products of ONE shape in one launch — the two directions of a bidirectional nn.LSTM layer (cnnlstm.py:148-149,288-290):
 *   mode 0: c0 = op(a0) op(b0) (+bias0)(relu),  c1 = op(a1) op(b1) (+bias1)(relu)      (x W_ih^T of both directions: a0 == a1;
 *           the weight gradients dgates_dir^T x and dgates_dir^T h of both directions)
 *   mode 1: c0 = op(a0) op(b0) + op(a1) op(b1) (+bias0)(relu), c1 = bias1 = NULL        (dx = dgates_fwd W_ih_fwd + dgates_rev W_ih_rev:
 *           one product with the K dimension running through both operands pairs instead of a product and an accumulating one)
 * Same operand conventions as vocr_gemm; all leading dimensions are shared by the two products.  Large 16-byte aligned shapes run
 * as ONE launch of the panel kernel whose workgroups cover both products (no partial last round); anything else is two vocr_gemm
 * calls.  workspace: vocr_gemm_pair_workspace_bytes (K slabs, fixed-order sum: reproducible). */
size_t vocr_gemm_pair_workspace_bytes(int m, int n, int k, int mode);
int vocr_gemm_pair(int mode, int transa, int transb, int m, int n, int k, const float* a0, const float* a1, int lda,
                   const float* b0, const float* b1, int ldb, float* c0, float* c1, int ldc, const float* bias0, const float* bias1,
                   int relu, void* workspace, size_t workspace_bytes, void* stream);
/* out[N] = sum over M rows of x[M,N] (bias gradients); partial rows in `workspace` (vocr_colsum_workspace_bytes, may be
 * NULL = one workgroup per 64 columns), added in a fixed order */
size_t vocr_colsum_workspace_bytes(int m, int n);
int vocr_colsum(const float* x, float* out, int m, int n, void* workspace, void* stream);
/* dz = (out > 0) ? dy : 0  (ReLU backward, elementwise) */
int vocr_relu_bwd(const float* dy, const float* out, float* dz, size_t count, void* stream);
/* bchw -> (w,b,c*h) and back — cnn_output.permute(3,0,1,2).contiguous(), cnnlstm.py:276 */
int vocr_bchw_to_wbch(const float* x, float* out, int b, int c, int h, int w, void* stream);
int vocr_wbch_to_bchw(const float* x, float* out, int b, int c, int h, int w, void* stream);
/* out = x * mask (inter-layer LSTM dropout with an explicit, pre-scaled mask) */
int vocr_mul(const float* x, const float* mask, float* out, size_t count, void* stream);
/* out = x + y ; out = x * (*scalar) with the scalar read from device memory (no host sync) */
int vocr_add(const float* x, const float* y, float* out, size_t count, void* stream);
int vocr_scale_dev(const float* x, const float* scalar, float* out, size_t count, void* stream);
/* mask[i] = (hash(seed,i) >= p) ? 1/(1-p) : 0 ; out = x*mask */
int vocr_dropout_fwd(const float* x, float* out, float* mask, size_t count, float p, uint64_t seed, void* stream);
/* the mask of vocr_dropout_fwd alone (it depends on the seed and the element index only): lets a consumer that applies the mask itself
 * (through vocr_mul, on packed rows) have it before x exists */
int vocr_dropout_mask(float* mask, size_t count, float p, uint64_t seed, void* stream);

/* ---- nn.LSTM recurrence on a packed, length-sorted batch — src/models/cnnlstm.py:148-149,288-290 ---------- */
/* One direction pair of one layer.  xproj[dir][T][B][4H] = x W_ih^T + b_ih + b_hh (gate order i,f,g,o),
 * whh_fwd / whh_rev [4H][H] (the two directions' weight_hh), lens[B] int32 (device, descending).  Outputs y[T][B][2H] (zeros past lens),
 * gates[dir][T][B][H][4] (post-activation i,f,g,o interleaved per unit) and cell[dir][T][B][H] for backward.  The forward writes EVERY
 * frame of gates and cell, zeros past lens (the caller need not clear them), and the backward entries never read a frame past lens.
 * gates must be 16-byte aligned in every entry that takes it, forward and backward (each unit's four gates move as one 16-byte
 * piece): a call with another pointer fails with VOCR_EINVAL before any launch.  whh_*, y, whht_* and dgates may have any float alignment (the
 * sweeps then run one generic launch per step).  h_{t-1}/c_{t-1} are read back from y/cell, so the sweep keeps no separate state.
 * workspace: vocr_lstm_workspace_bytes (256-byte aligned device memory; contents need not be preserved between calls, except
 * between the vocr_lstm_fwd_range calls of ONE sweep: the forward sweep's hand-off buffer lives there).
 * Supports B <= 64 per call, H % 16 == 0 (a larger batch is several calls on batch tiles: the recurrence never couples batch rows and
 * a tile of a length-sorted batch is itself a valid packed batch - vistaocr_amd.CnnOcrModel does that).  For H in {64,128,256,512} a whole sweep is ONE persistent launch whose workgroups
 * hand h_t (forward) / partial sums (backward) to each other through memory: it needs its grid (<= two workgroups per CU)
 * co-resident, so do not run two sweeps concurrently on one device; a hand-off that times out (seconds) poisons the
 * output with NaN instead of hanging.  Environment: VOCR_LSTM_SWEEP=step selects one launch per time step instead (several processes
 * sharing one GPU; VOCR_LSTM_PERSISTENT=0 is accepted as the old spelling), VOCR_LSTM_SWEEP=wide4|chain4|chain16 starts the kernel
 * search at that kind (A/B, tests), an unknown value makes the call fail with VOCR_EINVAL; VOCR_LSTM_WRITE_THROUGH=1 forces the
 * hand-off mode of a chain whose workgroups are spread over several XCDs.  These are the library's only runtime switches: the
 * kernel-variant experiments of scripts/ exist only in -DVOCR_EXPERIMENTS builds.
 * `health` (may be NULL): see the note on health words at the top; the timeout flag the sweep itself tests lives in the workspace
 * (an implementation detail: callers watch `health`). */
size_t vocr_lstm_workspace_bytes(int t, int b, int h);
int vocr_lstm_fwd(const float* xproj, const float* whh_fwd, const float* whh_rev, const int32_t* lens, float* y,
                  float* gates, float* cell, void* workspace, int t, int b, int h, int32_t* health, void* stream);
/* Steps [step_begin, step_end) of the same sweep (step s is time s for the forward direction, T-1-s for the reverse
 * one): a later range resumes from the h (in y) and c (in cell) an earlier call left.  Lets the host overlap the
 * x-projection GEMM of the later time steps with the first half of the sweep.  vocr_lstm_fwd == range [0, t). */
int vocr_lstm_fwd_range(const float* xproj, const float* whh_fwd, const float* whh_rev, const int32_t* lens, float* y,
                        float* gates, float* cell, void* workspace, int t, int b, int h, int step_begin, int step_end,
                        int32_t* health, void* stream);
/* dy[T][B][2H] -> dgates[dir][T][B][4H] (gradient w.r.t. pre-activation gates = w.r.t. xproj).
 * whht_* are the TRANSPOSED recurrent weights [H][4H] (vocr_bchw_to_wbch with b=1 transposes a matrix). */
int vocr_lstm_bwd(const float* dy, const float* whht_fwd, const float* whht_rev, const int32_t* lens, const float* gates,
                  const float* cell, float* dgates, void* workspace, int t, int b, int h, int32_t* health, void* stream);
/* Same, and dbias[dir][4H] = sum over (t, b) of dgates[dir] (the gradient of b_ih and of b_hh): accumulated inside the
 * sweep where the kernel supports it, else by column sums afterwards.  dbias may be NULL. */
int vocr_lstm_bwd_bias(const float* dy, const float* whht_fwd, const float* whht_rev, const int32_t* lens, const float* gates,
                       const float* cell, float* dgates, float* dbias, void* workspace, int t, int b, int h, int32_t* health,
                       void* stream);
/* The same sweep for a caller that overlaps: (1) `dy_mask` (NULL: none): dy is multiplied element-wise by it as it is read - the
 * backward of nn.LSTM's inter-layer dropout (src/train_cnn_lstm.py:331: the mask that scaled this layer's output) without a pass of
 * its own; (2) the bias gradient stays as per-chain partial rows in the workspace and vocr_lstm_bias_from_parts finishes it on ANY
 * stream ordered behind this call (the workspace must live until then) - so the data-gradient GEMM that follows the sweep on the
 * critical path does not queue behind a reduction nobody downstream reads.  Only for shapes the self-validating 4-row sweeps cover:
 * ask vocr_lstm_bwd_parts_supported (else use vocr_lstm_bwd_bias). */
int vocr_lstm_bwd_parts_supported(int t, int b, int h);
int vocr_lstm_bwd_parts(const float* dy, const float* dy_mask, const float* whht_fwd, const float* whht_rev, const int32_t* lens,
                        const float* gates, const float* cell, float* dgates, void* workspace, int t, int b, int h,
                        int32_t* health, void* stream);
int vocr_lstm_bias_from_parts(float* dbias, const void* workspace, int t, int b, int h, void* stream);

/* ---- fp32 GEMM on the bf16 matrix pipe by EXACT operand splitting ("bf16x6") — the LSTM projections and their gradients (cnnlstm.py:143-154) ---- */
/* Every fp32 operand element is written as a0 + a1 + a2 (three bf16 values whose sum is the fp32 value exactly) and a product is accumulated in fp32
 * from the six partial products of order <= 2^-16; the three dropped ones are <= 2^-23 |a b| (one unit roundoff of an fp32 product).
 * v_mfma_f32_32x32x16_bf16 runs at 16x the rate of the f32 MFMA: six per product = 2.67x the f32 matrix peak.
 * Domain of "exactly": every finite |a| >= 2^-110, the top of the range included (from 2^127 (2 - 2^-8) up, where rounding a0 to nearest would
 * overflow bf16, a0 is taken by truncation).  Below 2^-110 the last plane is a bf16 denormal, whose step 2^-133 is coarser than the operand's: the
 * planes sum to a rounded to a multiple of 2^-133, |error| <= 2^-134 (fp32 denormals included; the conversions and the matrix pipe keep denormals -
 * tests/test_x6_fp64_gpu.py pins both ends).  Inf and NaN stay non-finite in the planes and poison their output row / column.
 * vocr_gemm_x6_split writes the three planes of an operand in MFMA-fragment order (vocr_gemm_x6_planes_bytes(rows, k) bytes; rows padded to 256, K to
 * 32): x is [rows][k] with leading dimension ld (k_contiguous = 1) or [k][rows] (k_contiguous = 0: the transposed operands of the weight
 * gradients).  vocr_gemm_x6: C[m][n] = A[m][k] . B[n][k]^T (+ bias)(relu) from the planes of A and B, both outputs with ldc.  What is left of the
 * last round of 256 x 128 tiles (one workgroup per CU) is cut along K into slabs in `workspace` (vocr_gemm_x6_workspace_bytes; NULL: no cut)
 * that are added in a fixed order. */
size_t vocr_gemm_x6_planes_bytes(int rows, int k);
/* x may come in two pieces (the two direction planes of the LSTM's gate tensors, the two directions' weights): seg_axis = 0: k < seg from x, the
 * rest from x2 at k - seg; seg_axis = 1: row < seg from x, the rest from x2 at row - seg (seg <= 0: one piece; seg %% 8 == 0; both pieces with ld).
 * mask (K-contiguous only, may be NULL): an element-wise factor with x's addressing (the inter-layer dropout mask rides on the operand's read). */
int vocr_gemm_x6_split(const float* x, const float* x2, int seg, int seg_axis, const float* mask, long ld, int rows, int k, int k_contiguous,
                       void* planes, void* stream);
size_t vocr_gemm_x6_workspace_bytes(int m, int n, int k);
/* Which launches vocr_gemm_x6 / vocr_gemm_h3 (b_row0_2 < 0) or their _two_views forms (b_row0_2 = the second view's b_row0) make for a product, answered
 * by the planner they launch from; the plan does not depend on the split scheme.  Touches no device memory (256 CUs are assumed when no device is
 * visible).  b_rows: the rows B's plane set was written for; has_workspace: 0 = the call passes workspace NULL.  plan[VOCR_GEMM_X6_PLAN_INTS]:
 *   [0] 32-column tiles per workgroup tile: 4 (256 x 128) or 8 (256 x 256)      [1] workgroup tiles of the product
 *   [2] tiles of the launch that runs the whole K (0: none)                     [3] tiles of the launch that is cut along K (0: no cut)
 *   [4] K splits that launch runs (1: no cut)                                   [5] k16 stages per split (the last split may be shorter)
 *   [6] 1 if the 256 x 256 tile was admissible (every 8-tile block it reads exists in B's plane set)
 *   [7] the CU count the plan was made for                                      [8] bytes of workspace the K-cut launch uses */
#define VOCR_GEMM_X6_PLAN_INTS 9
int vocr_gemm_x6_plan(int m, int n, int k, int b_rows, int b_row0, int b_row0_2, int has_workspace, int* plan);
/* A = rows a_row0 .. + m and k16 steps a_kk0 .. + k/16 of a plane set written for (a_rows, a_k) - a view: the row-shifted operands of the recurrent
 * weight gradient are k windows of ONE plane set -; B likewise (its rows are the output columns).  Two outputs: columns >= csplit go to c1 at
 * col - csplit, or rows >= rsplit to c1 at row - rsplit (<= 0: no cut). */
int vocr_gemm_x6(const void* a_planes, int a_rows, int a_k, int a_row0, int a_kk0, const void* b_planes, int b_rows, int b_k, int b_row0, int b_kk0,
                 int m, int n, int k, float* c0, float* c1, int csplit, int rsplit, int ldc, const float* bias0, const float* bias1, int relu,
                 void* workspace, void* stream);

/* Two products of one shape from ONE pair of plane sets in one launch: rows < rsplit (a multiple of 256) of the m x n result read the views
 * (a_row0, a_kk0 | b_row0, b_kk0) and go to c0; rows >= rsplit read (a_row0 + rsplit .., a_kk0_2 | b_row0_2, b_kk0_2) and go to c1 at row - rsplit.
 * The recurrent weight gradients of both directions - each a time-shifted k window of the gate gradients' and the layer outputs' transposed planes -
 * with half the K-cut slabs of two launches. */
int vocr_gemm_x6_two_views(const void* a_planes, int a_rows, int a_k, int a_row0, const void* b_planes, int b_rows, int b_k, int m, int n, int k,
                           int rsplit, int a_kk0, int b_row0, int b_kk0, int a_kk0_2, int b_row0_2, int b_kk0_2, float* c0, float* c1, int ldc,
                           void* workspace, void* stream);

/* ---- the same products from TWO fp16 planes per operand and three partial products ("fp16x3") - OPT-IN, not what CnnOcrModel runs by default ---- */
/* a s = h0 + h1 with h0 = fp16(a s), h1 = fp16(a s - h0), s = the power of two that brings the ROW's largest magnitude into [2^14, 2^15): 22 - 23 of
 * fp32's 24 significant bits per element (elements more than 2^17 below their row's maximum lose low bits to fp16's exponent range: absolute error
 * <= 2^-40 of the row's maximum); a b ~ h0 g1 + h1 g0 + h0 g0, the dropped term <= 2^-24 |a b|; fp32 accumulate; both rows' scales undone exactly in
 * the epilogue.  Half the matrix instructions and 2/3 of the operand bytes of bf16x6 for a NORM-WISE error bound (<= 2^-22 sum |a||b| + K 2^-39
 * max|a| max|b| per dot product) instead of bf16x6's per-product one: measured against fp64 it stays below the f32-MFMA kernels' own error on the
 * training step's shapes (tests/test_x6_gpu.py), but it is an approximation of the operands, which bf16x6 is not.  Same contracts as the three entry
 * points above; a plane set is vocr_gemm_h3_planes_bytes(rows, k) bytes (the rows' maxima ride behind the planes) and is not interchangeable with a
 * bf16x6 one.  The split takes the maxima in a pass of its own (order-free integer maximum: deterministic). */
size_t vocr_gemm_h3_planes_bytes(int rows, int k);
/* bound > 0: the caller's bound on every |element| (after the mask) stands in for the rows' maxima - no pass over the source for them (an LSTM
 * output lies inside (-1, 1)); an element above the bound overflows fp16 and poisons its row, as an Inf in the source would.  bound = 0: measured. */
int vocr_gemm_h3_split(const float* x, const float* x2, int seg, int seg_axis, const float* mask, long ld, int rows, int k, int k_contiguous,
                       float bound, void* planes, void* stream);
int vocr_gemm_h3(const void* a_planes, int a_rows, int a_k, int a_row0, int a_kk0, const void* b_planes, int b_rows, int b_k, int b_row0, int b_kk0,
                 int m, int n, int k, float* c0, float* c1, int csplit, int rsplit, int ldc, const float* bias0, const float* bias1, int relu,
                 void* workspace, void* stream);
int vocr_gemm_h3_two_views(const void* a_planes, int a_rows, int a_k, int a_row0, const void* b_planes, int b_rows, int b_k, int m, int n, int k,
                           int rsplit, int a_kk0, int b_row0, int b_kk0, int a_kk0_2, int b_row0_2, int b_kk0_2, float* c0, float* c1, int ldc,
                           void* workspace, void* stream);

/* ---- the same recurrence without the padding: pack_padded_sequence's economy — src/models/cnnlstm.py:285-290 ---------- */
/* The reference packs the length-sorted batch before nn.LSTM, so cuDNN never computes a padded frame.  Here the rows of every
 * sequence-side tensor (bridge output, xproj, y, gates, cell, dy, dgates) can be kept in a PACKED, chain-major order instead of
 * [T][B]: batch rows are taken in chains of 4 (4c .. 4c+3; sorted lengths make lens[4c] the chain's longest, L_c); a GROUP is one
 * time step of one chain = 4 consecutive rows; the groups are [zero][chain 0: L_0 groups, t ascending][zero][chain 1: L_1]...[zero]:
 *     rows = 4 * (sum_c L_c + chains + 1),      row(t, b) = 4 * (1 + c + sum_{c' < c} L_c' + t) + (b & 3)   for t < L_c, c = b >> 2.
 * All GEMMs of the LSTM stack then run over `rows` rows instead of T*B, the recurrent weight gradient is still ONE product of
 * row-shifted views (shift 4: the all-zero group in front of / behind a chain is its h_{-1} / h_{L_c}), and a chain's workgroups leave
 * a sweep after their own L_c steps.  Contract: the caller zero-fills y before vocr_lstm_fwd_packed and dgates before
 * vocr_lstm_bwd_packed (the zero groups, a last chain's rows >= B and nothing else stay untouched by the sweeps: in gates and cell
 * these rows keep whatever they held, and nothing a sweep writes depends on them or on the same rows of xproj, dy and dy_mask); rows of a chain past
 * their own length are written as zeros like in the dense layout.  Results per frame are those of the dense entry points (same
 * kernels, same summation orders).  Shapes: ask vocr_lstm_packed_supported (B <= 32, H in {256, 512} on a device that can hold the
 * persistent sweep's grid) and keep rows * 2H * 4 below 2 GB (the sweeps' 32-bit offsets); otherwise use the dense entry points above.
 * vocr_seq_rowmap builds both index maps on the device from lens: to_packed[T*B] (packed row of frame (t, b), -1: none) and
 * to_dense[rows] (t*B + b of a packed row, -1: zero group / beyond B); either may be NULL.  vocr_gather_rows moves rows through such a
 * map: dst[r][0..n) = src[map[r]][0..n), or fill[0..n) (NULL: zeros) where map[r] < 0 (16-byte pieces when n % 4 == 0 and src, dst, fill
 * are 16-byte aligned, element by element otherwise) — packing (map = to_dense, nrows = rows) and
 * unpacking (map = to_packed, nrows = T*B; fill = the output layer's bias reproduces the reference's logits of a padded frame). */
int vocr_lstm_packed_supported(int b, int h);
int vocr_seq_rowmap(const int32_t* lens, int t, int b, int rows, int32_t* to_packed, int32_t* to_dense, void* stream);
int vocr_gather_rows(const float* src, float* dst, const int32_t* map, long nrows, int n, const float* fill, void* stream);
/* gradient of vocr_gather_rows' fill row: dfill[0..n) = sum of dout[r][0..n) over the rows with map[r] < 0 (fixed summation order);
 * workspace: vocr_gather_rows_fill_grad_workspace_bytes(n) */
size_t vocr_gather_rows_fill_grad_workspace_bytes(int n);
int vocr_gather_rows_fill_grad(const float* dout, const int32_t* map, long nrows, int n, float* dfill, void* workspace, void* stream);
int vocr_lstm_fwd_packed(const float* xproj, const float* whh_fwd, const float* whh_rev, const int32_t* lens, float* y,
                         float* gates, float* cell, void* workspace, int t, int b, int h, int rows, int32_t* health, void* stream);
/* dy_mask (may be NULL) as in vocr_lstm_bwd_parts; dbias (may be NULL) as in vocr_lstm_bwd_bias */
int vocr_lstm_bwd_packed(const float* dy, const float* dy_mask, const float* whht_fwd, const float* whht_rev, const int32_t* lens,
                         const float* gates, const float* cell, float* dgates, float* dbias, void* workspace, int t, int b, int h,
                         int rows, int32_t* health, void* stream);

/* ---- CTC: warpctc_pytorch.CTCLoss — src/train_cnn_lstm.py:358,138 ------------------------------------------ */
/* logits[T][B][V] pre-softmax, blank = 0.  labels flat int32 (device), label_offsets[B], label_lens[B],
 * act_lens[B] (device int32).  nll[B] = -log p(labels|x); dlogits[T][B][V] = d(sum_b nll)/dlogits
 * (zeros for t >= act_lens[b]).  max_label_len = max(label_lens) (host value, sizes the workspace). */
size_t vocr_ctc_workspace_bytes(int t, int b, int v, int max_label_len);
int vocr_ctc_loss_grad(const float* logits, const int32_t* labels, const int32_t* label_offsets,
                       const int32_t* label_lens, const int32_t* act_lens, float* nll, float* dlogits,
                       void* workspace, int t, int b, int v, int max_label_len, void* stream);

/* ---- greedy decode: decode_without_lm / ArgmaxDecoder — cnnlstm.py:479-541, decoder.py:116-185 ------------ */
/* per row of x[rows][v]: first index of the maximum and the maximum */
int vocr_argmax_rows(const float* x, int32_t* idx, float* maxv, int rows, int v, void* stream);
/* CTC best-path collapse on device.  canon[v] = smallest index with the same alphabet string (string
 * comparison of the reference), thresh = 3/len(alphabet) applied to the raw maximum.
 * out_labels[B][T], out_counts[B]. */
int vocr_greedy_collapse(const int32_t* idx, const float* maxv, const int32_t* lens, const int32_t* canon,
                         int32_t* out_labels, int32_t* out_counts, int t, int b, float thresh, void* stream);

/* ---- CTC prefix beam search with a character n-gram LM: the search of decode_with_lm — decoder.py:11-109, cnnlstm.py:298-475 ---- */
/* The eesen WFST of the reference is replaced by a character n-gram given as backoff-resolved dense tables over lm_states states:
 * lm_logp[S][V] = ln P(c | state) (backoff applied), lm_next[S][V] = the state after c, lm_eos[S] = ln P(</s> | state), lm_start
 * the <s> state; all three NULL: no LM.  logits[T][B][V] raw (log-softmax inside), lens[B] device int32 (clamped to [0, T]).
 * canon[V] as for vocr_greedy_collapse (NULL: identity): columns of one class are one symbol (logsumexp of the members) and the
 * emitted labels are canonical indices.  Candidates are ranked by logsumexp(p_blank, p_nonblank) + lm_weight * LM +
 * insertion_bonus * length (total order: score, then parent rank and class, so results are bit-identical from run to run);
 * prune_logp: classes whose frame log-prob is below it are not extended (-INFINITY: off).  1 <= beam <= 128,
 * 1 <= nbest <= beam, v <= 256.  Outputs, best first: out_labels[B][nbest][T] (zero past the length), out_lens[B][nbest],
 * out_scores[B][nbest][3] = {total, acoustic (CTC log-prob of the labelling), LM log-prob including </s>}; a rank the search
 * did not fill has length 0 and total -inf.  Workspace (the prefix node pool, T*beam nodes per line) from
 * vocr_ctc_beam_workspace_bytes (0 for an unsupported shape). */
size_t vocr_ctc_beam_workspace_bytes(int t, int b, int v, int beam, int nbest);
int vocr_ctc_beam_search(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon, int beam, int nbest,
                         const float* lm_logp, const int32_t* lm_next, const float* lm_eos, int lm_states, int lm_start,
                         float lm_weight, float insertion_bonus, float prune_logp, int32_t* out_labels, int32_t* out_lens,
                         float* out_scores, void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC prefix beam search with a word n-gram and a lexicon: the TLG.fst decode of decode_with_lm — decoder.py:11-109 ---- */
/* The search, inputs, limits and outputs of vocr_ctc_beam_search (no pruning); hypotheses are scored by a word n-gram over the tokens
 * of form_tokenized_words (textutils.py:290-323).  cls_kind[V]: 1 letter, 2 space (u0020), 3 single (punctuation / digit, a token of
 * its own, cls_tok[V] its LM token), 0 none.  Letter runs are words, limited to the lexicon trie trie_next[trie_nodes][V] (-1: no
 * child, root 0), trie_tok[trie_nodes] (the word ending at a node, -1: none), trie_la[trie_nodes] (the largest 1-gram ln P below the
 * node: the look-ahead of an open word).  LM over lm_tokens token ids: lm_states states (0 = the empty history, every history's
 * back-off state lm_back[s] < s), successors of state s at lm_off[s]..lm_off[s+1] of lm_succ_tok (sorted) / lm_succ_logp (ln) /
 * lm_succ_next (state 0: dense over all tokens, lm_off[1] = lm_tokens), lm_bow[S] the ln backoff weights; lm_succ entries in all.
 * A candidate is ranked by logsumexp(p_blank, p_nonblank) + lm_weight * (LM of the closed tokens + look-ahead of the open word) +
 * word_bonus * closed tokens; a word outside the lexicon scores ln P(<unk>) + oov_penalty (-INFINITY: closed vocabulary, such words
 * are never hypotheses).  The final score closes the open word and adds ln P(</s>) (tok_eos); out_scores = {total, acoustic, LM}.
 * Workspace from vocr_ctc_word_beam_workspace_bytes (0 for an unsupported shape). */
size_t vocr_ctc_word_beam_workspace_bytes(int t, int b, int v, int beam, int nbest);
int vocr_ctc_word_beam_search(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon, int beam, int nbest,
                              const int32_t* cls_kind, const int32_t* cls_tok, const int32_t* trie_next, const int32_t* trie_tok,
                              const float* trie_la, int trie_nodes, const int32_t* lm_off, const int32_t* lm_succ_tok,
                              const float* lm_succ_logp, const int32_t* lm_succ_next, const float* lm_bow, const int32_t* lm_back,
                              int lm_states, int lm_succ, int lm_tokens, int lm_start, int tok_unk, int tok_eos, float lm_weight,
                              float word_bonus, float oov_penalty, int32_t* out_labels, int32_t* out_lens, float* out_scores,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC forced alignment: conf_utils.form_confidence_gt of src/conf_test.py (a module the reference never shipped) ---- */
/* The best (Viterbi) CTC path of a KNOWN labelling through the frames, the frame span of every label on it, per-label scores, and the
 * forward score of the labelling from the same sweep: what per-character positions and confidences are made of.  One independent
 * problem per (line b, hypothesis q).  logits[T][B][V] raw (log-softmax inside), lens[B] device int32 (clamped to [0, T]), canon[V]
 * as for vocr_ctc_beam_search (NULL: identity): a class's log-probability is the logsumexp of its member columns and a label given
 * as any member index stands for its class.  labels[B][n][label_stride], label_lens[B][n] device int32: the layout the beam searches
 * write (n = nbest, label_stride = T); a greedy or ground-truth transcript packs as n = 1.  Blank = 0, S = 2L+1 extended positions,
 * the skip s-2 -> s allowed iff position s is not blank and its class differs from that of s-2 (vocr_ctc_loss_grad's rule).
 * Viterbi tie rule: among equal predecessors prefer s, then s-1, then s-2; at the last frame the final blank 2L wins over 2L-1.
 * Outputs: out_scores[B][n][2] = {ln P(best path), ln P_ctc(labels | x)}; out_spans[B][n][max_label_len][2] = {first, last} frame
 * (inclusive) of label p, -1 for p >= L and on lines without an alignment; out_label_scores[B][n][max_label_len][2] = {peak, sum}
 * of the class's frame log-probability over the span (0 where the span is -1; mean = sum / span length).  L = 0: both scores are
 * the sum of ln p_t(blank) (0 when lens[b] = 0).  Both scores -inf and every span -1: a labelling that does not fit the frames or
 * uses a class the frames give -inf, a label <= 0 or >= v or in the blank's class, label_lens > max_label_len.  -inf logits are
 * legal and never yield NaN.  Results are bit-identical from run to run.  Limits: 2 <= v <= 256, 1 <= n <= 128,
 * 0 <= max_label_len <= t, label_stride >= max_label_len, any t the beam searches take (t * b * n < 2^31).  Workspace (the class
 * log-probabilities; the back pointers where they do not fit the LDS; beyond 1663 labels also the rows of the sweep) from
 * vocr_ctc_align_workspace_bytes (0 for an unsupported shape); an unsupported shape fails with VOCR_EINVAL before any launch. */
size_t vocr_ctc_align_workspace_bytes(int t, int b, int v, int n, int max_label_len);
int vocr_ctc_align(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                   const int32_t* labels, const int32_t* label_lens, int n, int label_stride, int max_label_len,
                   float* out_scores, int32_t* out_spans, float* out_label_scores,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC edit scores: eesen's lattice (lattice_beam of init_lm) and the confidence experiment of src/conf_test.py ---- */
/* The exact CTC forward score of EVERY labelling one edit away from a hypothesis: what a per-character posterior, ranked alternatives
 * and a "something is missing here" signal are made of.  Inputs, classes, blank, transition rule and the (line b, hypothesis q)
 * layout are vocr_ctc_align's.  Outputs, fp32 natural log, M = max_label_len, L = label_lens[b][q]:
 *   out_ctc[B][n]         ln P_ctc(labels | x) (vocr_ctc_align's second score);
 *   out_sub[B][n][M][V]   at [p][c] the score of the labelling with label p replaced by the class of column c: columns of one class
 *                         hold the same bits, column 0 and every column of the blank's class hold -inf, the column of the label's
 *                         own class holds the unedited score (from the edit's own sum: equal to out_ctc up to rounding);
 *   out_del[B][n][M]      the score with label p removed;
 *   out_ins[B][n][M+1][V] at [q][c] the score with the class of column c inserted before label q (q = L appends);
 * entries at p >= L or q > L are -inf.  Every entry is the forward score of the edited labelling with no special case: a hypothesis
 * that does not fit its frames still has finite deletion scores where the shortened labelling fits, and with lens[b] = 0 the
 * deletion of an only label scores 0.  A labelling with a label <= 0 or >= v or in the blank's class, or label_lens outside
 * [0, M], gives -inf everywhere.  -inf logits are legal and never yield NaN.  Results are bit-identical from run to run.
 * Limits: 2 <= v <= 256, 1 <= n <= 128, 0 <= max_label_len <= t, label_stride >= max_label_len, t * b * n < 2^31, the forward and
 * backward lattices of all labellings (b * n * 8 * t * (2 * max_label_len + 1) bytes) at most 2 GiB, max_label_len <= 1823 (one row
 * of the sweep in the LDS).  Workspace (the class log-probabilities and the lattices) from vocr_ctc_edit_workspace_bytes (0 for an
 * unsupported shape); an unsupported shape fails with VOCR_EINVAL before any launch. */
size_t vocr_ctc_edit_workspace_bytes(int t, int b, int v, int n, int max_label_len);
int vocr_ctc_edit_scores(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                         const int32_t* labels, const int32_t* label_lens, int n, int label_stride, int max_label_len,
                         float* out_ctc, float* out_sub, float* out_del, float* out_ins,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- Weighted n-best CTC scores and gradient: what minimum-error-rate training over a beam search's n-best list is made of ---- */
/* For n labellings of each line: out_ctc[B][n] = ln P_ctc(labels[b][q] | x_b), and with weights[B][n] (device fp32) given,
 *   dlogits[T][B][V] = d/dlogits  sum_b sum_q weights[b][q] * ln P_ctc(labels[b][q] | x_b)
 * in one tensor, the sum over the SCORABLE hypotheses (finite out_ctc).  Inputs, classes, blank, transition rule, the (line b,
 * hypothesis q) layout and the validity rules are vocr_ctc_align's and vocr_ctc_edit_scores's: logits raw (log-softmax inside), lens
 * clamped to [0, T], canon NULL = identity, a label given as any member index stands for its class.  out_ctc is vocr_ctc_align's
 * second score and holds the same bits as vocr_ctc_edit_scores's out_ctc (the same kernel computes it), -inf in the same places: a
 * labelling that does not fit the frames or uses a class the frames give -inf, a label <= 0 or >= v or in the blank's class,
 * label_lens outside [0, max_label_len], lens[b] = 0 with L > 0 (L = 0 then scores 0).
 * With p_t(v) the softmax of frame t, P_t(c) the sum of p_t over the columns of class c and occ_q(t, c) the posterior probability,
 * given labelling q, that frame t is spent in class c (the sum over the extended positions s of class c of
 * alpha_t(s) * beta_t(s) / (P_t(c) * P_q); it sums to 1 over c):
 *   dlogits[t][b][v] = p_t(v) * ( sum_q w_q * occ_q(t, class(v)) / P_t(class(v))  -  sum_q w_q ).
 * Rows t >= lens[b] are written as zeros.  A hypothesis with a -inf score contributes exactly nothing, whatever its weight; a
 * duplicate labelling counts twice.  -inf logits are legal: a column with p_t(v) = 0 gets 0, and a class with P_t(c) = 0 never yields
 * NaN or inf.  No floating-point atomics: every sum has a fixed order, results are bit-identical from run to run, and a line's rows
 * depend on that line alone.  weights == NULL (then dlogits must be NULL, and the other way round): scores only - the forward sweep
 * alone, no lattice stored; out_ctc holds the same bits as in a call with weights.
 * Limits: 2 <= v <= 256, 1 <= n <= 128, 0 <= max_label_len <= t, label_stride >= max_label_len, t * b * n < 2^31, max_label_len <=
 * 1823 (one row of the sweep in the LDS), and the forward and backward lattices of all labellings,
 * b * n * 8 * t * (2 * max_label_len + 1) bytes, at most 2 GiB.  Workspace from vocr_ctc_nbest_workspace_bytes (0 for an unsupported
 * shape) = the class log-probabilities (t * b * v * 4 bytes rounded up to 16) + the lattices; a scores-only call uses, and checks
 * for, the class log-probabilities alone.  Bad arguments and unsupported shapes fail with VOCR_EINVAL before any launch. */
size_t vocr_ctc_nbest_workspace_bytes(int t, int b, int v, int n, int max_label_len);
int vocr_ctc_nbest_grad(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                        const int32_t* labels, const int32_t* label_lens, int n, int label_stride, int max_label_len,
                        const float* weights, float* out_ctc, float* dlogits,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC keyword search: "does this line contain the word X" without decoding (the lattice use of eesen's decode, lattice-free) ---- */
/* For every (line b, query q) the EXPECTED NUMBER of occurrences of the query as a contiguous substring of the collapsed labelling,
 * E = sum over all frame paths pi of P(pi | x) * #occurrences(query in B(pi)): exact under the CTC model, a sum over all v^len paths
 * with no beam, no hypothesis and no pruning; min(1, E) bounds the probability that the query occurs at all from above (E is NOT that
 * probability, and no language model is involved).  And the best single occurrence with its frame span.  Inputs, classes, blank and
 * transition rule are vocr_ctc_align's; "equal" and "different" always compare classes.  queries[nq][query_stride], query_lens[nq],
 * query_flags[nq] (NULL: all 0) device int32, shared by all lines.  A query k_1 .. k_L (no blanks) has S = 2L-1 extended positions
 * k_1, blank, k_2, .., blank, k_L.  An occurrence is a MAXIMAL frame span [s, e]: pi_s in k_1's class, pi_e in k_L's, pi_s .. pi_e
 * collapses to the query, pi_(s-1) not in k_1's class (or s = 0), pi_(e+1) not in k_L's class (or e = len-1).  One pass, with
 * notc_t(c) = ln(1 - P_t(class of c)) computed as the log of the SUM over the other classes' columns (never 1 - p):
 *   entry(t) = 0 if t = 0 else notc_(t-1)(k_1);  exit(t) = 0 if t = len-1 else notc_(t+1)(k_L);
 *   a_t(0) = lp_t(k_1) + lse(a_(t-1)(0), entry(t));  a_t(s) = lp_t(ext_s) + lse(a_(t-1)(s), a_(t-1)(s-1), a_(t-1)(s-2) if the skip is
 *   allowed);  ln E = lse over t of a_t(S-1) + exit(t).
 * query_flags bit 0 (ANCHOR_START): only occurrences at the very beginning of the labelling, entry(t) = sum of ln p_u(blank), u < t;
 * bit 1 (ANCHOR_END): the same at the end, exit(t) = sum of ln p_u(blank), u > t; both bits: E = P_ctc(query | x), vocr_ctc_align's
 * second score.  Bits 2 / 3 (TRIM_START / TRIM_END) change only the reported span: it starts at the first frame of k_2 / ends at the
 * last frame of k_(L-1) (a whole-word search pads the word with spaces and wants the word's frames); such a query needs L >= 2, with
 * both bits L >= 3.  The best occurrence is the same recursion with max: the maximum over spans and over the paths inside them of
 * entry(s) + sum of lp_t(pi_t) + exit(e); every cell carries the start frame of its best path (no back-pointer table).  Tie rule:
 * among equal candidates prefer s (stay), then s-1, then s-2, then the fresh entry (position 0 only); among equal end frames the
 * earliest wins.  Outputs: out_log_count[B][nq] = ln E (-inf for 0); out_best[B][nq] = the best occurrence's score;
 * out_span[B][nq][2] = its {first, last} frame (inclusive).  -inf / -inf / {-1, -1}: a query that does not fit the line's frames or
 * uses a class the frames give -inf, lens[b] = 0, and for every line an invalid query (query_lens outside [1, max_query_len], a label
 * <= 0 or >= v or in the blank's class, too few labels for its trim bits); an invalid query poisons only its own column.  -inf logits are legal and never yield NaN (a
 * frame whose logits are all -inf gives -inf to every class and every notc).  Results are bit-identical from run to run, and written
 * at the caller's query index: the queries are sorted by length on the device so that those of at most 8 / 16 labels share a wave,
 * 4 / 2 per wave.  Limits: 2 <= v <= 256, nq >= 1, 1 <= max_query_len <= 128, query_stride >= max_query_len, t * b * nq < 2^31.
 * Workspace (class log-probabilities, notc rows, blank prefix / suffix sums, the sort) from vocr_ctc_keyword_workspace_bytes (0 for an
 * unsupported shape); an unsupported shape fails with VOCR_EINVAL before any launch. */
size_t vocr_ctc_keyword_workspace_bytes(int t, int b, int v, int nq, int max_query_len);
int vocr_ctc_keyword_scores(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                            const int32_t* queries, const int32_t* query_lens, const int32_t* query_flags, int nq, int query_stride,
                            int max_query_len, float* out_log_count, float* out_best, int32_t* out_span,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC grammar search: the exact probability that a line's text belongs to a regular language (the unweighted half of eesen's decode) ---- */
/* For every (line b, automaton k) ln P = ln of the sum of P(pi | x) over ALL frame paths pi whose collapsed labelling the automaton
 * accepts - exact under the CTC model, no beam, no hypothesis, no pruning - and the best single path with its labelling.  Inputs,
 * classes, blank and the repeat rule are vocr_ctc_align's ("equal" and "different" always compare classes).  The g automata are shared by
 * all lines and concatenated: automaton k has the states g_state_off[k] .. g_state_off[k+1] of accept[] (non-zero: accepting; local
 * state 0 is the start) and the arcs g_arc_off[k] .. g_arc_off[k+1] of arc_src / arc_cls / arc_dst (LOCAL state numbers; arc_cls a
 * non-blank column, any member of its class).  The arcs of one automaton are SORTED by (dst, class, src), so that a state's incoming
 * arcs are contiguous and grouped by class.  All device int32.  With W[s] = "in s, the last frame was blank or nothing was emitted yet"
 * and A[a] = "the last frame emitted cls_a on arc a":
 *   t = 0: W[0] = lp_0(blank), A[a] = lp_0(cls_a) if src_a = 0, everything else -inf;
 *   t > 0: W'[s] = lp_t(blank) + lse(W[s], A[a'] for every a' with dst_a' = s);
 *          A'[a] = lp_t(cls_a) + lse(A[a], W[src_a], A[a'] for every a' with dst_a' = src_a and class(cls_a') != class(cls_a));
 *   ln P = lse(W[s] for accepting s, A[a] for every a with accepting dst_a) after frame lens[b]-1.
 * The excluded term is CTC's repeat rule: the same class twice in a row needs a blank between, the route through W.  It is evaluated as
 * lse(prefix, suffix) over the class-sorted incoming arcs, never as a subtraction.  For a DETERMINISTIC automaton every labelling has
 * one state sequence and P is exactly the probability that the labelling is accepted; for a non-deterministic one it is the sum over
 * (frame path, automaton path) pairs.  WHAT IT IS NOT: this entry has no weights on the arcs (vocr_ctc_grammar_scores_weighted below
 * has), and the best
 * score is the maximum over single PATHS through the product (frame path and automaton path), not the most probable accepted
 * labelling.  The best path is the same recursion with max, a back pointer per frame and cell in the workspace; a candidate replaces
 * the choice only when strictly greater - W: stay, then the incoming arcs in arc order; A: stay, then W[src], then the incoming arcs in
 * arc order; at the end the accepting W cells in state order, then the arc cells in arc order.  Outputs: out_logp[B][g] = ln P;
 * out_best[B][g] = the best path's score; out_labels[B][g][label_stride] / out_lens[B][g] = its collapsed labelling as canonical
 * columns (0 behind its end) and its length, -1 where nothing is accepted: the beam searches' layout, label_stride >= t, so the result
 * goes into vocr_ctc_align and vocr_edit_stats with n = g as it is.  out_best, out_labels and out_lens are all NULL or all given; all
 * NULL: scores only, no max pass and no back pointers.  lens[b] = 0: ln P = best = 0 if the start state accepts, else -inf.
 * -inf / -inf / -1, for every line, for an automaton that breaks a rule: 1 <= states <= max_states, 0 <= arcs <= max_arcs, src and dst
 * in range, 0 < cls < v and not in the blank's class, the sort order; it poisons only its own column.  (The offsets themselves must
 * point into the arrays.)  -inf logits are legal and never yield NaN.  No floating-point atomics: every lse has a fixed order, results
 * are bit-identical from run to run, and out_logp has the same bits with and without best paths.  Limits: 2 <= v <= 256, g >= 1,
 * t * b * g < 2^31, max_states + max_arcs <= 8192 (one workgroup per (line, automaton) keeps two rows and two scans of that many words
 * in LDS; larger lexicons stay with vocr_ctc_word_beam_search), and with best paths t * b * g * (max_states + max_arcs) * 4 bytes of
 * back pointers <= 2 GiB.  Workspace (16-byte aligned: class log-probabilities, the plan, the back pointers when want_best) from
 * vocr_ctc_grammar_workspace_bytes (0 for an unsupported shape); bad arguments and unsupported shapes fail with VOCR_EINVAL before any
 * launch.  The gradient of ln P with respect to the logits: vocr_ctc_grammar_grad below. */
size_t vocr_ctc_grammar_workspace_bytes(int t, int b, int v, int g, int max_states, int max_arcs, int want_best);
int vocr_ctc_grammar_scores(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                            const int32_t* g_state_off, const int32_t* g_arc_off, int g,
                            const int32_t* arc_src, const int32_t* arc_cls, const int32_t* arc_dst,
                            const int32_t* accept, int max_states, int max_arcs,
                            float* out_logp, float* out_best, int32_t* out_labels, int32_t* out_lens, int label_stride,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- weighted grammars: the same sweep over an automaton whose arcs and accepting states carry weights ---- */
/* vocr_ctc_grammar_scores with two more device fp32 tables: arc_logw[a], one natural-log weight per arc (the arcs' own order and
 * offsets), and final_logw[s], one per state (the states' order and offsets), read for ACCEPTING states only.  The weight w(rho) of an
 * automaton path rho is the sum of its arcs' weights plus the final weight of its last state.  Sum pass: ln Z = ln of the sum of
 * P(pi | x) * exp(w(rho)) over all (frame path pi, automaton path rho) pairs whose labelling rho accepts - a probability only when the
 * weights normalise; max pass: max of ln P(pi | x) + w(rho).
 *   t = 0: W[0] = lp_0(blank), A[a] = lp_0(cls_a) + w_a if src_a = 0, everything else -inf;
 *   t > 0: W'[s] = lp_t(blank) + lse(W[s], A[a'] for every a' into s)                                              (unchanged)
 *          A'[a] = lp_t(cls_a) + lse(A[a], w_a + lse(W[src_a], A[a'] into src_a of another class));
 *   end  : lse(W[s] + f_s for accepting s, A[a] + f_dst_a for accepting dst_a);   lens[b] = 0: f_0 if state 0 accepts.
 * An arc's weight is paid once per traversal - never on a stay, and again each time a self-loop is re-entered through its W cell.  (The
 * kernels pay it when the arc cell is LEFT, which shifts every arc cell by a constant of its own and changes neither ln Z nor the
 * maxima.)  The max pass keeps the tie rule and the back pointers: the same candidates in the same order, each with its weight added.
 * Both tables must be finite: an automaton with a NaN or infinite arc weight, or such a final weight on an accepting state, breaks a
 * rule like a mis-sorted arc and poisons its own column.  The two tables go together (one without the other: VOCR_EINVAL before any
 * launch); BOTH NULL runs the unweighted code: the bits of vocr_ctc_grammar_scores.  Limits, outputs and workspace are those of
 * vocr_ctc_grammar_scores (vocr_ctc_grammar_weighted_workspace_bytes returns the same figure): the weights are staged in LDS with the
 * plan where they fit beside the rows, else read from global memory, one coalesced float per arc cell and frame. */
size_t vocr_ctc_grammar_weighted_workspace_bytes(int t, int b, int v, int g, int max_states, int max_arcs, int want_best);
int vocr_ctc_grammar_scores_weighted(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                                     const int32_t* g_state_off, const int32_t* g_arc_off, int g,
                                     const int32_t* arc_src, const int32_t* arc_cls, const int32_t* arc_dst,
                                     const int32_t* accept, const float* arc_logw, const float* final_logw,
                                     int max_states, int max_arcs,
                                     float* out_logp, float* out_best, int32_t* out_labels, int32_t* out_lens, int label_stride,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- grammar-constrained CTC training: the gradient of the match score (graph-based temporal classification) ---- */
/* out_logp[b] = ln P(line b's labelling is accepted by automaton which[b]) and dlogits = d/dlogits sum_b weights[b] * ln P_b.  The
 * automaton tables, their sort order (dst, class, src), classes, blank, the repeat rule and the validity rules are exactly those of
 * vocr_ctc_grammar_scores; which[B] device int32 pairs line b with ONE automaton (several lines may share one): one workgroup per
 * line, not per (line, automaton).  out_logp[b] holds the bits of vocr_ctc_grammar_scores' out_logp[b][which[b]] for the same
 * tables, max_states and max_arcs, with or without weights (the same device code runs the forward sweep).
 * With the cells c = W[s], A[a], e(c) the class a cell emits (blank for W, cls_a for A), alpha_t(c) the recursion above and
 * bhat_t(c) = the log-sum over all accepted continuations that start in c at frame t, frame t's emission included:
 *   t = len-1: bhat(W[s]) = lp_t(blank) if s accepts, bhat(A[a]) = lp_t(cls_a) if dst_a accepts, everything else -inf;
 *   t < len-1: bhat(W[s]) = lp_t(blank) + lse(bhat'(W[s]), bhat'(A[a']) for every a' with src_a' = s);
 *              bhat(A[a]) = lp_t(cls_a) + lse(bhat'(A[a]), bhat'(W[dst_a]), bhat'(A[a']) for every a' with src_a' = dst_a and
 *                           class(cls_a') != class(cls_a))                                   (bhat' the row of frame t + 1)
 * - the alpha recursion over the mirrored automaton (arcs (dst, cls, src) sorted by (src, class, dst), every accepting state a
 * start) on the frames read backwards, and evaluated as that: the call sorts the arcs itself.
 *   occ(t, k) = sum over the cells with e(c) = k of exp(alpha_t(c) + bhat_t(c) - lp_t(k) - ln P)            (sums to 1 over k)
 *   dlogits[t][b][v] = w_b * p_t(v) * (occ(t, class(v)) / P_t(class(v)) - 1)                 (the form of vocr_ctc_nbest_grad)
 * For a non-deterministic automaton the same formula is the gradient of the sum over (frame path, automaton path) pairs.
 * THE FAMILY'S RULES: rows t >= lens[b] are zeros.  A line whose ln P = -inf, whose automaton breaks a rule or whose which[b] lies
 * outside [0, g) gets out_logp = -inf and rows that are exactly zero whatever its weight; it poisons nothing else.  lens[b] = 0:
 * 0 or -inf by the start state's accept flag, and zero rows.  -inf logits are legal: a column with p = 0 gets 0, and a class with
 * P_t(c) = 0 never yields NaN or inf.  No floating-point atomics: the per-class occupancy sum runs over a class-sorted arc index built
 * on the device, one wave per class, in a fixed order; results are bit-identical from run to run, and a line's rows depend on that
 * line and its automaton alone.  weights (device fp32 [B]) and dlogits ([T][B][V]) are both NULL or both given; both NULL: scores
 * only, nothing is stored and no backward sweep runs.  WHAT IT IS NOT: weighted (vocr_ctc_grammar_grad_weighted below is), a best path (vocr_ctc_grammar_scores
 * has it), and the forward rows are STORED: t * b * (max_states + max_arcs) * 4 bytes of workspace, which must stay within 2 GiB -
 * the caller cuts the batch (every line is independent).  Limits: those of vocr_ctc_grammar_scores (2 <= v <= 256, g >= 1,
 * t * b * g < 2^31, max_states + max_arcs <= 8192) plus that lattice.  Workspace (16-byte aligned: class log-probabilities, the plan,
 * and with want_grad the mirrored tables, their plan, the sort keys and the lattice) from vocr_ctc_grammar_grad_workspace_bytes (0
 * for an unsupported shape); bad arguments and unsupported shapes fail with VOCR_EINVAL before any launch. */
size_t vocr_ctc_grammar_grad_workspace_bytes(int t, int b, int v, int g, int max_states, int max_arcs, int want_grad);
int vocr_ctc_grammar_grad(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                          const int32_t* g_state_off, const int32_t* g_arc_off, int g,
                          const int32_t* arc_src, const int32_t* arc_cls, const int32_t* arc_dst,
                          const int32_t* accept, int max_states, int max_arcs,
                          const int32_t* which, const float* weights, float* out_logp, float* dlogits,
                          void* workspace, size_t workspace_bytes, void* stream);

/* The same under a weighted automaton (arc_logw, final_logw: vocr_ctc_grammar_scores_weighted): out_logp[b] = ln Z_b, with the bits of
 * vocr_ctc_grammar_scores_weighted's out_logp[b][which[b]], and dlogits = d/dlogits sum_b weights[b] * ln Z_b.  The occupancy form
 * above is unchanged; alpha and bhat carry the weights.  The backward sweep runs the same recursion over the mirrored automaton, where
 * "enter arc a" is the original's "leave arc a": the mirror kernel permutes the weights with the arcs, the mirror's start weights are
 * the original's final weights and the original's start state has none, and every arc weight and every final weight of a path is
 * counted exactly once in alpha_t(c) + bhat_t(c), for every cell and frame - so every frame's occupancies still sum to 1.  There is no
 * gradient with respect to the weights themselves.  The two tables go together; both NULL runs the unweighted code, the bits of
 * vocr_ctc_grammar_grad.  The workspace holds the mirrored weights too: vocr_ctc_grammar_grad_weighted_workspace_bytes. */
size_t vocr_ctc_grammar_grad_weighted_workspace_bytes(int t, int b, int v, int g, int max_states, int max_arcs, int want_grad);
int vocr_ctc_grammar_grad_weighted(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                                   const int32_t* g_state_off, const int32_t* g_arc_off, int g,
                                   const int32_t* arc_src, const int32_t* arc_cls, const int32_t* arc_dst,
                                   const int32_t* accept, const float* arc_logw, const float* final_logw,
                                   int max_states, int max_arcs,
                                   const int32_t* which, const float* weights, float* out_logp, float* dlogits,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- grammar-constrained CTC prefix beam search: the most probable labellings a deterministic automaton accepts ---- */
/* vocr_ctc_beam_search - the same inputs, classes, optional character n-gram tables, score formula, total order, pruning, limits
 * (1 <= nbest <= beam <= 128, v <= 256, t * b * beam < 2^31), outputs and workspace (the node pool) - restricted to the labellings
 * that line b's automaton which[b] accepts.  The g automata are concatenated as DENSE tables: automaton k has the states
 * g_state_off[k] .. g_state_off[k+1] (g_state_off[g] = all states) of dfa_next[states][v] (the LOCAL state after class c, -1: no arc;
 * local state 0 is the start; only canonical columns are read) and dfa_dist[states] (the fewest symbols from the state to an
 * accepting one: 0 exactly for accepting states, so there is no accept array).  All device int32; which[B] device int32.  The
 * automaton is deterministic, so a prefix has one state, each beam carries it, and the exact prefix merge is unchanged.  With
 * rem = lens[b] - 1 - t frames left after frame t, an extension by class c of a beam in state s is a candidate only if
 * n = dfa_next[s][c] is a state of the automaton and 0 <= dfa_dist[n] <= rem, and a stay only if 0 <= dfa_dist[s] <= rem: every
 * further symbol needs a frame, so only prefixes without an accepted completion are dropped (a lower bound: the blank between
 * repeated symbols is not counted).  The final ranking keeps accepting states only.  The beam may run empty (the language needs more
 * symbols than the line has frames): ranks the search did not fill have length 0 and total -inf, as in vocr_ctc_beam_search.
 * lens[b] = 0: the empty labelling iff state 0 accepts.  Device contents are never trusted: which[b] outside [0, g) or a state range
 * that is empty, reversed or past g_state_off[g] gives that line no hypothesis, a next state outside the automaton counts as no arc, a
 * negative distance as "cannot accept"; none of them becomes a load address.  Under the one-state automaton that accepts everything
 * the search takes the decisions of vocr_ctc_beam_search.  WHAT IT IS NOT: exact beyond the beam (a labelling whose prefix fell out
 * of the beam is lost, as in every beam search), weighted (vocr_ctc_grammar_beam_search_weighted below is), or
 * non-deterministic.  There is no limit on the automaton's size but the memory of the dense tables (states * v * 4 bytes).  Only
 * integer LDS atomics; results are bit-identical from run to run.  Bad arguments (g < 1, a NULL table, a short workspace) fail with
 * VOCR_EINVAL before any launch.  Workspace from vocr_ctc_grammar_beam_workspace_bytes (0 for an unsupported shape). */
size_t vocr_ctc_grammar_beam_workspace_bytes(int t, int b, int v, int beam, int nbest);
int vocr_ctc_grammar_beam_search(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon, int beam, int nbest,
                                 const int32_t* g_state_off, const int32_t* dfa_next, const int32_t* dfa_dist, int g,
                                 const int32_t* which, const float* lm_logp, const int32_t* lm_next, const float* lm_eos,
                                 int lm_states, int lm_start, float lm_weight, float insertion_bonus, float prune_logp,
                                 int32_t* out_labels, int32_t* out_lens, float* out_scores,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* The same under a weighted automaton: dfa_logw[states][v] (device fp32, dfa_next's indexing: the natural-log weight of the arc from
 * the state on class c; only canonical columns that have an arc are read) and dfa_final[states] (the final weight, read for accepting
 * states).  The automaton is deterministic, so a prefix has one state and ONE accumulated weight gacc, carried by its beam, and the
 * exact prefix merge stays valid.  A candidate's rank adds grammar_weight * gacc_k for a stay and grammar_weight * (gacc_k +
 * dfa_logw[state_k][c]) for an extension; the final rank adds grammar_weight * (gacc + dfa_final[state]).  The distance rule, the
 * merge, top-K and the total order are untouched.  out_scores keeps its three columns (total, acoustic, LM); total includes the
 * grammar term, and out_grammar[B][nbest] (device fp32, NULL: not wanted) is the hypothesis's raw weight gacc + dfa_final[state], 0
 * for a rank the search did not fill.  grammar_weight must be finite.  An arc whose weight is NaN or infinite counts as no arc, an
 * accepting state with such a final weight as not accepting.  dfa_logw and dfa_final go together (one without the other: VOCR_EINVAL
 * before any launch); BOTH NULL runs the unweighted search - the bits of vocr_ctc_grammar_beam_search, out_grammar zeros.  Limits and
 * workspace: vocr_ctc_grammar_beam_search's. */
int vocr_ctc_grammar_beam_search_weighted(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon, int beam,
                                          int nbest, const int32_t* g_state_off, const int32_t* dfa_next, const int32_t* dfa_dist,
                                          const float* dfa_logw, const float* dfa_final, int g, const int32_t* which,
                                          const float* lm_logp, const int32_t* lm_next, const float* lm_eos, int lm_states, int lm_start,
                                          float lm_weight, float grammar_weight, float insertion_bonus, float prune_logp,
                                          int32_t* out_labels, int32_t* out_lens, float* out_scores, float* out_grammar,
                                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- edit statistics: compute_cer_wer of test_on_val (src/textutils.py:264-351, src/train_cnn_lstm.py:32-100) and src/edit_dist_trace.py ---- */
/* Levenshtein statistics (unit costs) of np (hypothesis, reference) pairs that are already on the device: distances and lengths over
 * characters and over the tokens of form_tokenized_words, and - on request - the operation trace.  Integer arithmetic: every output
 * equals the cell-by-cell DP's bit for bit.  A is ALWAYS the hypothesis side, B the reference side.  a_labels[na][a_stride],
 * a_lens[na], b_labels[nb][b_stride], b_lens[nb] device int32: the layout the beam searches and vocr_greedy_collapse write ([B][n][T]
 * is [B*n][T]); pairs[np][2] = {index into a, index into b}.  canon[V] as everywhere (NULL: identity): two labels are equal iff
 * their classes are.  kinds[V] = vocr_ctc_word_beam_search's cls_kind (1 letter, 2 space, 3 single; read at the class): a run of
 * letters is one word, every single a word of its own, anything else separates; two words are equal iff they have the same length
 * and the same classes.  kinds = NULL: no word statistics (the word fields are -1; asking for words alone is then an error).
 * want: bit 0 character statistics, bit 1 word statistics (at least one of the two), bit 2 the trace (needs bit 0): the operation
 * counts of what bits 0 / 1 ask for, out_confusion and out_ops.  Without bit 2 only distances and lengths are produced and no back
 * pointer is stored.  out_stats[np][12] = {char_dist, char_sub, char_ins, char_del, hyp_chars, ref_chars, word_dist, word_sub,
 * word_ins, word_del, hyp_words, ref_words}; a field that was not asked for is -1; sub + ins + del = dist.  INS: a hypothesis
 * element without a counterpart in the reference; DEL: a reference element missing from the hypothesis.  Trace tie rule
 * (edit_dist_trace.py): at a cell take the diagonal (COPY when the elements are equal, else SUB) if its cost is <= both others,
 * otherwise INS (from i-1) if its cost is <= DEL's, otherwise DEL (from j-1); the walk starts at (|A|, |B|) and is complete: at
 * j = 0 the remaining i are INS, at i = 0 the remaining j are DEL.  out_confusion[V][V] (may be NULL; the caller zeroes it, the call
 * ADDS to it with integer atomics): over the character trace of every pair, COPY and SUB at [reference class][hypothesis class],
 * INS at [0][hypothesis class], DEL at [reference class][0].  out_ops[np][ops_stride] (may be NULL; ops_stride >= max_a_len +
 * max_b_len): the character trace from the front, 1 COPY, 2 SUB, 3 INS, 4 DEL, 0 past its end (every byte of a row is written).
 * A length of 0 is legal on either side.  A label <= 0 or >= v or in the blank's class, a length outside [0, max], or a pair index out
 * of range makes every statistic of THAT pair -1 (and its row of out_ops 0); it adds nothing to the confusion.  Nothing past a
 * sequence's length is read as content.  Results are bit-identical from run to run.  Limits: 2 <= v <= 256, na, nb, np >= 1,
 * 0 <= max_a_len, max_b_len <= 2048, strides >= the maxima.  Workspace (with bit 2 and a pair table beyond the LDS share, 2 bits per
 * cell: one slab per RESIDENT workgroup, at most 256 of them - it does not grow with np) from vocr_edit_stats_workspace_bytes (0 for an
 * unsupported shape); an unsupported shape fails with VOCR_EINVAL before any launch. */
size_t vocr_edit_stats_workspace_bytes(int na, int nb, int np, int v, int max_a_len, int max_b_len, int want);
int vocr_edit_stats(const int32_t* a_labels, const int32_t* a_lens, int na, int a_stride, int max_a_len,
                    const int32_t* b_labels, const int32_t* b_lens, int nb, int b_stride, int max_b_len,
                    const int32_t* pairs, int np, const int32_t* canon, const int32_t* kinds, int v, int want,
                    int32_t* out_stats, int32_t* out_confusion, uint8_t* out_ops, int ops_stride,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- training augmentation of a collated batch: src/train_cnn_lstm.py:203-274 (--synth_input, --stripe), src/imagetransforms.py:71-406 ---- */
/* y = the augmented batch.  x[b][c][h][wmax] fp32 in [0, 1] as the collater builds it and the model takes it, widths[b] device int32
 * (clamped to [0, wmax]), c = 1 or 3; y has the same shape and must not be x or overlap it.  WIDTHS DO NOT CHANGE: every line keeps
 * its own box [0, h) x [0, w), so the model's sorted widths, its length map and the packed LSTM rows are untouched; the reference's
 * crop / pad jitter is therefore a mild zoom and shift INSIDE the box (part of A below), not a new width.  All randomness is drawn on
 * the host and arrives in tables; the call is a pure function of its arguments, bit-identical from run to run (no floating-point
 * atomics; the only reduction is a min / max).
 * params[b][24] device 32-bit words, one record per line (f: fp32 bits, i: int32, u: uint32):
 *    0..5  f  A = a00 a01 a02 a10 a11 a12, the INVERSE affine map from output pixel indices to source pixel indices:
 *             xs = a00 px + a01 py + a02, ys = a10 px + a11 py + a12
 *    6..10 f  block filter taps k00 k01 k10 k11 and bias
 *   11     f  contrast factor alpha (exactly 1: the contrast step is skipped, so that an identity record is a bitwise identity)
 *   12 13  f  noise probability per pixel, noise sigma            14 15  f  delete probability per pixel, delete value
 *   16     f  stripe value
 *   17     u  flags: bit 0 mesh warp, bit 1 block filter, bit 2 invert
 *   18     i  gw, the line's number of mesh CELLS along x (clamped to [1, gw_max]); it has gw + 1 node columns
 *   19 20  i  stripe rows [r0, r1) (empty when r0 >= r1)
 *   21 22  u  the line's 64-bit noise key, low word first        23  reserved, 0
 * mesh[b][2][gh + 1][gw_max + 1] fp32 (may be NULL: no line is warped and bit 0 is ignored): node displacements in pixels, plane 0
 * along x, plane 1 along y, of a regular control grid of gh x gw cells spanning the line (WarpImage's grid with
 * fit_interval_to_image: gw = max(1, round(w / interval)), gh likewise from h); node (i, j) sits at (j w / gw, i h / gh).
 * Per output pixel (ch, oy, ox < w), in fp32, every multiply-add fused as written here:
 *  1 geometry: px = ox, py = oy; with bit 0: u = px * (gw / w), v = py * (gh / h), j = min(floor u, gw - 1), i = min(floor v, gh - 1),
 *    D = bilinear interpolation of the four nodes of cell (i, j) at (u - j, v - i), p += D.  (The reference interpolates the scattered
 *    nodes with scipy's Delaunay griddata; here it is bilinear on the regular grid.)  Without bit 0, D is exactly 0.  (xs, ys) = A (p, 1),
 *    xs clamped to [0, w - 1], ys to [0, h - 1] (border replicate, the rule of the reference's warpAffine call; a NaN becomes 0).
 *    R(oy, ox) = bilinear sample of x[b][ch] at (xs, ys) with taps floor and min(floor + 1, limit), lerp(a, b, t) = fma(t, b - a, a):
 *    no tap ever reads a column >= w, so the pad columns of x may hold anything, NaN included.  All channels share the geometry.
 *  2 block filter (bit 1, TessBlockConv: a 2x2 convolution with zero padding 1 cropped to the top-left h x w):
 *    F(oy, ox) = bias + sum_{i,j in {0,1}} k[i][j] R(oy - 1 + i, ox - 1 + j), R = 0 outside [0, h) x [0, w); then the reference's
 *    renormalisation over the WHOLE line, all channels: v = (F - min) / (max - min), 0 when max = min (the reference divides by zero
 *    there).  No quantisation to uint8.  Without bit 1, v = R.
 *  3 photometric, in this order: contrast v = (v - 0.5) alpha + 0.5; invert (bit 2) v = 1 - v; noise: with probability p_noise
 *    v += sigma n, n standard normal; delete: with probability p_del v = del_value; stripe: rows [r0, r1) = stripe_value; clamp to
 *    [0, 1] (a NaN becomes 0).  The draws: bits(draw) = upper 32 bits of vocr_dropout_fwd's hash (the splitmix64 finaliser) of
 *    key * 0x9e3779b97f4a7c15 + (ox | oy << 24 | ch << 48 | draw << 56): a function of the line's key and the pixel only, not of
 *    wmax, b or the launch.  A uniform is (bits >> 8) * 2^-24, exactly representable, so the decisions u < p are exact.  draw 0: the
 *    noise decision; n = sqrt(-2 ln u1) cos(2 pi u2) (Box-Muller in fp32), u1 = ((bits(1) >> 8) + 1) * 2^-24, u2 = (bits(2) >> 8) *
 *    2^-24; draw 3: the delete decision.
 *  4 padding: y[b][:][:][ox >= w] = 0, the collater's zero pad.
 * with_filter = 0 promises that no record has bit 1 set: the min / max pass is not launched, bit 1 is ignored and workspace may be
 * NULL.  Otherwise pass 1 writes one (min, max) per workgroup to the workspace (8-byte aligned, vocr_augment_workspace_bytes; 0 for
 * an unsupported shape) and pass 2 folds them; min and max do not depend on the order.  WHAT IT IS NOT: no gradient, no change of
 * width or batch order, no parity claim against OpenCV or imgaug; imgaug's Grayscale and Emboss are not built.  Limits: 1 <= b <=
 * 65535, h, wmax <= 2^24.  Bad arguments (a null pointer, b, c, h or wmax < 1, c not 1 or 3, y = x, a workspace too small) fail with
 * VOCR_EINVAL before any launch. */
size_t vocr_augment_workspace_bytes(int b, int c, int h, int wmax);
int vocr_augment_lines(const float* x, const int32_t* widths, int b, int c, int h, int wmax, const uint32_t* params,
                       const float* mesh, int gh, int gw_max, int with_filter, float* y,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- alignment entropy of a labelling and its gradient: entropy-regularised CTC training (EnCTC, Liu, Jin and Zhang 2018) ---- */
/* For the ONE labelling of each line, with p(pi) = prod_t P_t(pi_t) over the frame paths pi that collapse to it:
 *   out_ctc[B]     = ln P,  P = sum_pi p(pi)                  the same bits as vocr_ctc_nbest_grad's out_ctc, with or without coeff
 *   out_entropy[B] = H = - sum_pi (p / P) ln (p / P) = N / P + ln P >= 0 (clamped at 0),   N = sum_pi p(pi) * (-ln p(pi))
 * the entropy, in nats, of the posterior over the feasible alignments: 0 when one alignment holds all the mass, ln(number of feasible
 * paths) on uniform logits.  With coeff[B][2] = (w_ctc, w_ent) (device fp32) given,
 *   dlogits[T][B][V] = d/dlogits  sum_b ( w_ctc_b * ln P_b + w_ent_b * H_b )
 *   dlogits[t][b][v] = p_t(v) / P_t(c) * ( w_ctc occ(t, c) + w_ent (occN(t, c) - (N / P) occ(t, c)) ) - p_t(v) w_ctc,    c = class(v),
 * occ as in vocr_ctc_nbest_grad and occN(t, c) = (1 / P) * the sum of p * (-ln p) over the paths with pi_t = c.  Rows t >= lens[b] are
 * zeros.  Inputs, classes, blank, transition rule, validity rules and the -inf places are vocr_ctc_nbest_grad's with n = 1 (labels
 * [B][label_stride], label_lens [B]).  A labelling that cannot be scored gets out_ctc = -inf and out_entropy = 0 and contributes
 * exactly nothing to dlogits (its rows are zeros); L = 0 has one path and H = 0.  -inf logits are legal and never yield NaN or inf.
 * No floating-point atomics: every sum has a fixed order, results are bit-identical from run to run, and a line's rows depend on that
 * line alone.  coeff == NULL (then dlogits must be NULL, and the other way round): scores only - the forward sweep alone, nothing
 * stored.  Limits: 2 <= v <= 256, 0 <= max_label_len <= min(t, 1663) (the sweep keeps TWO rows in the LDS, the path sum's and the
 * entropy's, where the other labelling entries keep one and reach 1823), label_stride >= max_label_len, t * b < 2^31, and with coeff the four lattices,
 * b * 16 * t * (2 * max_label_len + 1) bytes, at most 2 GiB.  Workspace from vocr_ctc_entropy_workspace_bytes (0 for an unsupported
 * shape) = the class log-probabilities (t * b * v * 4 bytes rounded up to 16), and with want_grad the
 * lattices behind them.  Bad arguments and unsupported shapes fail with VOCR_EINVAL before any launch. */
size_t vocr_ctc_entropy_workspace_bytes(int t, int b, int v, int max_label_len, int want_grad);
int vocr_ctc_entropy(const float* logits, const int32_t* lens, int t, int b, int v, const int32_t* canon,
                     const int32_t* labels, const int32_t* label_lens, int label_stride, int max_label_len,
                     const float* coeff, float* out_ctc, float* out_entropy, float* dlogits,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- optimiser: grad clamp + torch.optim.Adam — src/train_cnn_lstm.py:143-149,363 -------------------------- */
/* g = clamp(g*grad_scale, -clamp, clamp) (+ wd*p); Adam(m, v); step is the 1-based step count.  A NaN gradient stays NaN
 * (torch's clamp_ propagates NaN) and sets health[1] (health may be NULL).  clamp < 0 or NaN: VOCR_EINVAL, as vocr_clamp;
 * count == 0: VOCR_OK, nothing touched. */
int vocr_clamp_adam(float* p, const float* g, float* m, float* v, size_t count, float lr, float beta1, float beta2,
                    float eps, float weight_decay, float clamp, float grad_scale, int step, int32_t* health, void* stream);
/* in place x = clamp(x, -clamp, clamp), NaN preserved: `param.grad.data.clamp_(min=-5, max=5)` (train_cnn_lstm.py:143-145)
 * for callers that keep their own optimiser (torch.optim.Adam). */
int vocr_clamp(float* x, size_t count, float clamp, int32_t* health, void* stream);

/* ---- data-parallel exchange: nn.DataParallel's gradient reduction — cnnlstm.py:198-199, train_cnn_lstm.py:333 ---- */
/* One process per GPU; the only collective of the path is a SUM all-reduce of the flat fp32 gradient before the clamp.
 * Thin RCCL wrapper (xGMI inside a node) for hosts that do not use torch.distributed; RCCL is dlopen'ed on first use.
 * Rank 0 calls vocr_comm_unique_id and hands the 128 bytes to every rank (any transport); every rank then calls
 * vocr_comm_create(device = its GPU).  The handle is the only object the library ever allocates. */
typedef struct vocr_comm vocr_comm;
int vocr_comm_unique_id(void* id128);
int vocr_comm_create(vocr_comm** out, const void* id128, int nranks, int rank, int device);
int vocr_allreduce_sum_f32(vocr_comm* comm, float* buf, size_t count, void* stream);   /* in place, stream-ordered */
int vocr_comm_destroy(vocr_comm* comm);

#ifdef __cplusplus
}
#endif
#endif
