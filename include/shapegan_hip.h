/* include/shapegan_hip.h — C ABI of libshapegan_hip.so (MI355X / gfx950 only).
 *
 * The reference (marian42/shapegan) has no FFI of its own: its hot path is the set of ATen kernels that
 * torch.nn launches underneath model/gan.py, model/autoencoder.py, model/progressive_gan.py and
 * model/sdf_net.py.  This header is the boundary a maintainer binds instead of those ATen calls; every entry
 * point names the reference site it replaces.  The Python shells in shapegan_amd/model/ (gan.py, ...) (same class names,
 * constructor arguments, state_dict keys and file names as the reference's model/ package) call these through
 * ctypes on tensor.data_ptr() — see INTEGRATION.md.
 *
 * Conventions
 *   - all tensors fp32, contiguous, device pointers; NCDHW for voxel tensors, row-major [N,features] for MLPs;
 *   - every call is asynchronous and ordered on `stream` (pass torch.cuda.current_stream().cuda_stream);
 *   - the caller owns every buffer, including workspaces (sizes from the *_workspace_bytes helpers); nothing is
 *     retained past the call; no global mutable state, so calls are re-entrant across threads/streams;
 *   - return 0 on success, <0 on error (SG_ERR_*); sg_last_error() gives a thread-local message;
 *   - `act` is one of SG_ACT_*, fused into the producing kernel's epilogue (slope = LeakyReLU negative slope).
 */
#ifndef SHAPEGAN_HIP_H
#define SHAPEGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_ABI_VERSION 8

typedef struct ihipStream_t* hipStream_t; /* the opaque handle hip_runtime_api.h declares (identical re-typedef) */

#define SG_ACT_NONE_C 0
#define SG_ACT_LEAKY_C 1
#define SG_ACT_RELU_C 2
#define SG_ACT_TANH_C 3
#define SG_ACT_SIGMOID_C 4

int sg_abi_version(void);
const char* sg_last_error(void);

/* ---- K1: nn.Conv3d(kernel 4, stride 2, padding 1) --------------------------------------------------------
 * reference: model/gan.py:49-53 (Discriminator), model/autoencoder.py:16-24 (encoder),
 *            model/progressive_gan.py:38 (optional_layers[i][0])  -> aten::convolution / convolution_backward.
 * x [batch,Cx,ID,IH,IW] -> y [batch,Cout,ID/2,IH/2,IW/2]; w [Cout,Cin_total,4,4,4].
 * Only input channels [0,Cin) are read (Cin < Cin_total reproduces from_SDF's zero padding,
 * model/progressive_gan.py:9-16, without materialising the zero channels). */
size_t sg_conv3d_k4s2p1_fwd_workspace_bytes(int batch, int Cin, int Cout, int OD, int OH, int OW);
int sg_conv3d_k4s2p1_fwd(const float* x, const float* w, const float* bias, float* y, int batch, int Cin, int Cin_total,
                         int Cx, int Cout, int ID, int IH, int IW, int act, float slope, void* workspace,
                         size_t workspace_bytes, hipStream_t stream);
/* Kept weight images (see sg_conv3d_k4s2p1_dgrad_keep below) for the forward form, and the images of up to 8 forthcoming
 * _keep calls packed in ONE launch: a critic update packs four images of two weights (model/gan.py:51-53 forward and input
 * gradient), one small launch each before.  kinds[i]: 0 forward, 1 input gradient; dims[8 i ..] = {batch, Cin, Cin_total, Cx, Cout,
 * ID, IH, IW} of call i; served[i] = 1: make call i with weights_unchanged = 1. */
int sg_conv3d_k4s2p1_fwd_keep(const float* x, const float* w, const float* bias, float* y, int batch, int Cin, int Cin_total,
                              int Cx, int Cout, int ID, int IH, int IW, int act, float slope, void* workspace,
                              size_t workspace_bytes, int weights_unchanged, hipStream_t stream);
/* 0: the call {kind, dims[8]} (as in sg_conv3d_k4s2p1_pack_images) with a workspace of workspace_bytes is not served by a kernel
 * with a kept weight image.  Otherwise a number that is equal for two calls exactly when they read the same image: callers key their
 * kept images on it instead of on the full shape (the batch size does not enter the LDS-halo kernels' images).  Host code only. */
long long sg_conv3d_k4s2p1_image_layout(int kind, const int* dims, size_t workspace_bytes);
int sg_conv3d_k4s2p1_pack_images(int n, const int* kinds, const float* const* weights, void* const* workspaces,
                                 const size_t* workspace_bytes, const int* dims, int* served, hipStream_t stream);
/* testing / tuning: force one forward implementation (0 = gather implicit GEMM, 1 = LDS-halo implicit GEMM).  debug bit 8 (256)
 * with impl 1: the depth-skip form of the 8^3 -> 4^3 kernel (conv_fwd_halo4_dskip_kernel; SG_ERR_ARG on other grids); without it a
 * forced call gets conv_fwd_halo4_kernel.  The dispatching entries take the depth-skip form wherever the 4^3 kernel runs without a
 * channel split.  Depth-skip forms (forward and input gradient) do not issue the products whose activation operand is the zero
 * padding beyond the DEPTH range: for finite weights the result is that of the full sum; for a non-finite weight on such a tap the
 * full sum is NaN (0 x inf) and the depth-skip form returns the convolution's definition, the sum over the in-range positions (as
 * the weight-gradient skip form does).  The h / w padding is multiplied as before. */
int sg_conv3d_k4s2p1_fwd_impl(const float* x, const float* w, const float* bias, float* y, int batch, int Cin,
                              int Cin_total, int Cx, int Cout, int ID, int IH, int IW, int act, float slope,
                              void* workspace, size_t workspace_bytes, int impl, int debug, hipStream_t stream);
/* dx[batch,Cx(first Cin channels),ID,IH,IW] = conv^T(dy, w) (+bias[ci], act: used when this is a ConvTranspose fwd) */
size_t sg_conv3d_k4s2p1_dgrad_workspace_bytes(int Cout, int Cin);
/* the same with the batch and the output grid of the convolution (O = I/2): also covers the tap-plane scratch of the
 * one-channel layers (Cin == 1: ConvTranspose3d(C -> 1) forward / Conv3d(1 -> C) input gradient) */
size_t sg_conv3d_k4s2p1_dgrad_workspace_bytes_for(int batch, int Cin, int Cout, int OD, int OH, int OW);
int sg_conv3d_k4s2p1_dgrad(const float* dy, const float* w, const float* bias, float* dx, int batch, int Cin,
                           int Cin_total, int Cx, int Cout, int ID, int IH, int IW, int act, float slope,
                           void* workspace, size_t workspace_bytes, hipStream_t stream);
/* sg_conv3d_k4s2p1_dgrad with the packed weight image KEPT between calls — the forward of a ConvTranspose3d whose weights
 * did not change since its last call (model/gan.py:29-35: the WGAN generator is evaluated six times per 5+1 training unit of
 * train_wgan.py:60-84 and updated once).  `workspace` is a buffer the caller dedicates to this weight tensor (size as for
 * sg_conv3d_k4s2p1_dgrad); weights_unchanged != 0 promises that the previous call on it had the same weight values and the same
 * shapes and that nothing else wrote to it: the packing launch is then skipped.  Results are those of sg_conv3d_k4s2p1_dgrad. */
int sg_conv3d_k4s2p1_dgrad_keep(const float* dy, const float* w, const float* bias, float* dx, int batch, int Cin,
                                int Cin_total, int Cx, int Cout, int ID, int IH, int IW, int act, float slope,
                                void* workspace, size_t workspace_bytes, int weights_unchanged, hipStream_t stream);
int sg_conv3d_k4s2p1_dgrad_impl(const float* dy, const float* w, const float* bias, float* dx, int batch, int Cin,
                                int Cin_total, int Cx, int Cout, int ID, int IH, int IW, int act, float slope,
                                void* workspace, size_t workspace_bytes, int impl, hipStream_t stream); /* tests */
/* (impl 1: the LDS-halo kernel, 3: one output parity per workgroup, 1 + 4 ppw: ppw parities; + 64: the depth-skip form of the
 * 4^3 -> 8^3 64-row kernel, conv_dgrad_halo_dskip_kernel, at any batch size (SG_ERR_ARG on other grids) — without it a forced call
 * gets conv_dgrad_halo_kernel<1> / conv_dgrad_halo32_kernel<1>; the dispatching entries take the depth-skip form for every 64-row
 * 4^3 call.  Semantics of the depth-skip forms: see sg_conv3d_k4s2p1_fwd_impl.
 * + 128: the depth-walk form of the 8^3 -> 16^3 64-row kernel, conv_dgrad_halo_dwalk_kernel, at any batch size: dy grids of depth 8
 * (h, w multiples of 8), Cin > 32, an even Cout / 16; SG_ERR_ARG on other shapes and together with the ppw / one-parity / + 64
 * bits.  A workgroup walks one depth half of a sample so that every wave carries the same share of the products with the depth
 * padding, which are not issued (1/16 of the MFMAs; semantics as the depth-skip forms, bit-equal to conv_dgrad_halo_kernel<0> for
 * finite inputs up to the sign of a zero).  Without the bit a forced call gets conv_dgrad_halo_kernel<0> /
 * conv_dgrad_halo32_kernel<0>; the dispatching entries take the depth-walk form where its grid has at least 512 workgroups.) */
/* Which kernel sg_conv3d_k4s2p1_dgrad / _dgrad_keep launch for a call on tensors of exactly Cin / Cout channels (dy grid O) with a
 * workspace of workspace_bytes: the plan the call itself makes.  Host code only, no GPU needed (addition to ABI 8, backward
 * compatible).  SG_DGRAD_FORM_NONE: another kernel family (one-channel layers, the gather kernel). */
#define SG_DGRAD_FORM_NONE 0
#define SG_DGRAD_FORM_DSKIP4 1       /* conv_dgrad_halo_dskip_kernel (4^3 grids) */
#define SG_DGRAD_FORM_ROWS32_4 2     /* conv_dgrad_halo32_kernel<1> */
#define SG_DGRAD_FORM_ROWS64_4 3     /* conv_dgrad_halo_kernel<1> */
#define SG_DGRAD_FORM_ROWS32 4       /* conv_dgrad_halo32_kernel<0> */
#define SG_DGRAD_FORM_ROWS64 5       /* conv_dgrad_halo_kernel<0> */
#define SG_DGRAD_FORM_DEPTH_WALK 6   /* conv_dgrad_halo_dwalk_kernel */
int sg_conv3d_k4s2p1_dgrad_form(int batch, int Cin, int Cout, int OD, int OH, int OW, size_t workspace_bytes);
/* dw[Cout, Cin_total(first Cin channels written), 4,4,4] = sum_{n,o} dy * x-patches; split-K workspace optional */
size_t sg_conv3d_k4s2p1_wgrad_workspace_bytes(int batch, int Cin, int Cout, int OD, int OH, int OW);
int sg_conv3d_k4s2p1_wgrad_impl(const float* dy, const float* x, float* dw, int batch, int Cin, int Cin_total, int Cx,
                                int Cout, int ID, int IH, int IW, void* workspace, size_t workspace_bytes, int impl,
                                hipStream_t stream); /* tests */
int sg_conv3d_k4s2p1_wgrad(const float* dy, const float* x, float* dw, int batch, int Cin, int Cin_total, int Cx,
                           int Cout, int ID, int IH, int IW, void* workspace, size_t workspace_bytes,
                           hipStream_t stream);
/* Weight AND bias gradient of y = act(conv(x) + b) from dy = dLoss/dy in one pass: dz = dy * act'(y) is formed inside the
 * weight-gradient kernel (act'(y) from the activated output, as sg_act_bwd), db[co] = sum of dz over batch and positions.  For a
 * layer whose input needs no gradient (the critic's first layer, model/gan.py:49 under train_wgan.py:69) the activation backward
 * then is no pass of its own.  Served shapes: sg_conv3d_k4s2p1_wgrad_act_eligible (one-channel layers, LeakyReLU / ReLU). */
/* The incoming gradient's fragment image of the LDS-halo weight-gradient kernel written by the gradient's PRODUCER:
 * sg_conv3d_k4s2p1_wgrad_dy_image says whether the weight-gradient call (dy [batch, Cout, O^3], the workspace it will get) is served
 * that way (1: the image is [mt_total][nslice][8][64] float4 at the start of that workspace; 0: use sg_conv3d_k4s2p1_wgrad);
 * sg_act_bwd_rowsum_pack8 = sg_act_bwd_rowsum on [N, C, 8, 8, 8] tensors (LeakyReLU / ReLU) + the image; sg_head_dot_bwd writes it
 * for 4^3 grids; sg_conv3d_k4s2p1_wgrad_prepacked = sg_conv3d_k4s2p1_wgrad without its packing launch. */
int sg_conv3d_k4s2p1_wgrad_dy_image(int batch, int Cin, int Cout, int OD, int OH, int OW, size_t workspace_bytes, int* mt_total,
                                    long* nslice);
int sg_act_bwd_rowsum_pack8(const float* y, const float* dy, float* dz, float* rowsum, void* dz_image, long N, int C, long nslice,
                            int act, float slope, hipStream_t stream);
int sg_conv3d_k4s2p1_wgrad_prepacked(const float* dy, const float* x, float* dw, int batch, int Cin, int Cin_total, int Cx,
                                     int Cout, int ID, int IH, int IW, void* workspace, size_t workspace_bytes, hipStream_t stream);
int sg_conv3d_k4s2p1_wgrad_act_eligible(int batch, int Cin, int Cout, int OD, int OH, int OW, int act);
int sg_conv3d_k4s2p1_wgrad_act(const float* dy, const float* y, const float* x, float* dw, float* db, int batch, int Cin,
                               int Cin_total, int Cx, int Cout, int ID, int IH, int IW, int act, float slope, void* workspace,
                               size_t workspace_bytes, hipStream_t stream);

/* ---- K2: nn.ConvTranspose3d(kernel 4, stride 2, padding 1) -------------------------------------------------
 * reference: model/gan.py:13,17,21 (Generator), model/autoencoder.py:55,59,63 (decoder).
 * x [batch,Cin_T,ID,IH,IW] -> y [batch,Cout_T,2ID,2IH,2IW]; w [Cin_T,Cout_T,4,4,4]. */
int sg_convT3d_k4s2p1_fwd(const float* x, const float* w, const float* bias, float* y, int batch, int Cin_T, int Cout_T,
                          int ID, int IH, int IW, int act, float slope, void* workspace, size_t workspace_bytes,
                          hipStream_t stream);
/* The same for C -> 1 channel (C <= 64, planes of at most 256 positions) with the INPUT taken through
 * act_in(x * in_scale[c] + in_shift[c]) inside the kernel's loads: a BatchNorm3d + LeakyReLU between the producing layer and this
 * one (model/gan.py:18-21, model/autoencoder.py:60-63) then never is a pass of its own — sg_bn_train_stats supplies
 * scale / shift.  in_act: none, LeakyReLU (0 <= in_slope <= 1) or ReLU. */
int sg_convT3d_k4s2p1_to1_pre_eligible(int batch, int C, int ID, int IH, int IW);
int sg_convT3d_k4s2p1_to1_pre(const float* x, const float* w, const float* bias, float* y, const float* in_scale,
                              const float* in_shift, int in_act, float in_slope, int batch, int C, int ID, int IH, int IW, int act,
                              float slope, hipStream_t stream);
/* the same with the kernel form chosen by the caller (tests / tuning; the library reads no environment variable): form 0 = the
 * dispatch rule, 1 / 2 = one output-row parity per workgroup with one / two plane walks, 5 = all 64 taps per workgroup with the
 * plane ranges per sample chosen by the library, 6 / 7 / 8 = the same with 1 / 2 / 4 plane ranges.  Forms 3 / 4 (both row parities
 * per workgroup) were retired: SG_ERR_ARG.  Every form computes the same sums in the same order (bit-identical results). */
int sg_convT3d_k4s2p1_to1_pre_impl(const float* x, const float* w, const float* bias, float* y, const float* in_scale,
                                   const float* in_shift, int in_act, float in_slope, int batch, int C, int ID, int IH, int IW,
                                   int act, float slope, int form, hipStream_t stream);
/* Several independent batches in one pass ("groups" of samples_per_group samples: e.g. the generator evaluations of four
 * consecutive critic updates, train_wgan.py:60-63, whose BatchNorm statistics are per evaluation): sample n takes row n /
 * samples_per_group of in_scale / in_shift ([groups][C]) and is written at y + (n / samples_per_group) * y_group_stride +
 * (n % samples_per_group) * (2I)^3 — each group into its own destination (the fake half of its critic batch). */
int sg_convT3d_k4s2p1_to1_pre_grouped(const float* x, const float* w, const float* bias, float* y, const float* in_scale,
                                      const float* in_shift, int in_act, float in_slope, int batch, int C, int ID, int IH, int IW,
                                      int act, float slope, int samples_per_group, long y_group_stride, hipStream_t stream);
int sg_convT3d_k4s2p1_dgrad(const float* dy, const float* w, float* dx, int batch, int Cin_T, int Cout_T, int ID, int IH,
                            int IW, void* workspace, size_t workspace_bytes, hipStream_t stream);
int sg_convT3d_k4s2p1_wgrad(const float* dy, const float* x, float* dw, int batch, int Cin_T, int Cout_T, int ID, int IH,
                            int IW, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* ---- K3/K6: GEMM + bias (+activation) -------------------------------------------------------------------------
 * reference: nn.Linear (model/autoencoder.py:34,41-42,45; model/progressive_gan.py:28,30) -> aten::addmm/mm, and the
 * kernel-4 stride-1 convolutions on 1^3 / 4^3 grids (model/gan.py:9,55; model/autoencoder.py:28,51).
 *   C(i,j) = act( sum_k A(i,k) B(k,j) + bias_i[i] + bias_j[j >> bias_j_shift] ), element strides for all operands;
 *   each of A, B needs a unit stride on one axis. */
size_t sg_gemm_workspace_bytes(int M, int N);
int sg_gemm(const float* A, long sai, long sak, const float* B, long sbk, long sbj, float* C, long sci, long scj,
            const float* bias_i, const float* bias_j, int bias_j_shift, int M, int N, int K, int act, float slope,
            void* workspace, size_t workspace_bytes, hipStream_t stream);
/* Which kernel sg_gemm launches for a call, and how: the value sg_gemm itself launches from (host code only, no GPU needed;
 * additions to ABI 8, backward compatible).  A, B, workspace: the pointers of the call (only their alignment / being null is read).
 * plan[0..7] = { kind (SG_GEMM_KIND_*), tm, tn (the 16-k skeleton's 32 x 32 MFMA tiles per wave: a workgroup tile of 64 tm x 64 tn;
 * 0 for the other kinds), nsplit (partial images in the workspace; 1: no K split), kchunk (k range of a split), finalize
 * (SG_GEMM_FINALIZE_*), grid (workgroups of the product kernel), layout (2 * (A is k-major) + (B is k-major)) }. */
#define SG_GEMM_KIND_SKELETON 0
#define SG_GEMM_KIND_GEMM128 1
#define SG_GEMM_KIND_GEMM128_SPLIT 2
#define SG_GEMM_KIND_PERSISTENT 3
#define SG_GEMM_FINALIZE_NONE 0
#define SG_GEMM_FINALIZE_FLAT 1
#define SG_GEMM_FINALIZE_DEEP 2
int sg_gemm_plan(const void* A, long sai, long sak, const void* B, long sbk, long sbj, long sci, long scj, int has_bias_i, int M, int N,
                 int K, const void* workspace, size_t workspace_bytes, long* plan);
/* The same for sg_gemm_nt (batch = 1) and sg_gemm_nt_batched / _lnrelu: plan[0..4] = { direct (1: one launch straight into C, no
 * workspace), nsplit, kchunk, grid, workspace bytes the call insists on }. */
int sg_gemm_nt_plan(int batch, int M, int N, long K, long* plan);
/* C[M,N] = A[M,K] B[N,K]^T, K contiguous in both operands and K >> M, N: the SDFNet weight gradients dW_l = dZ_l H_{l-1}^T over
 * the points of a batch (autograd of model/sdf_net.py:56-61).  Deterministic split-K; rows of C have stride ldc. */
size_t sg_gemm_nt_workspace_bytes(int M, int N, long K);
int sg_gemm_nt(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N, long K, void* workspace,
               size_t workspace_bytes, hipStream_t stream);
/* up to 8 such products in one launch: member b multiplies A + a_off[b] with B + b_off[b] (element offsets, shared leading
 * dimensions and sizes) into C + c_off[b] with row stride ldc[b] — all weight gradients of an SDFNet backward at once */
size_t sg_gemm_nt_batched_workspace_bytes(int batch, int M, int N, long K);
int sg_gemm_nt_batched(const float* A, const long* a_off, long lda, const float* B, const long* b_off, long ldb, float* C,
                       const long* c_off, const long* ldc, int batch, int M, int N, long K, void* workspace,
                       size_t workspace_bytes, hipStream_t stream);
/* The same with B_b holding LayerNorm-normalised rows: C_b = A_b * relu(gamma_b (.) B_b + beta_b)^T with gamma_b = gamma + g_off[b],
 * beta_b = beta + g_off[b] ([N] each): the hidden weight gradients of the LayerNorm MLP (K7b) straight from the xhat images. */
int sg_gemm_nt_batched_lnrelu(const float* A, const long* a_off, long lda, const float* B, const long* b_off, long ldb,
                              const float* gamma, const float* beta, const long* g_off, float* C, const long* c_off, const long* ldc,
                              int batch, int M, int N, long K, void* workspace, size_t workspace_bytes, hipStream_t stream);
int sg_colsum(const float* x, float* out, int rows, int cols, long ld, hipStream_t stream); /* bias grads */
int sg_rowsum(const float* x, float* out, long rows, long len, long ld, hipStream_t stream);
/* rows [d*rows_per_dst, (d+1)*rows_per_dst) go to outs[d] (ndst <= 8 host-side pointers to device buffers): one launch for
 * bias gradients that live in separate slices of a flat gradient buffer */
int sg_rowsum_multi(const float* x, float* const* outs, const long* out_strides, int ndst, long rows_per_dst, long len, long ld,
                    hipStream_t stream); /* out_strides (optional, host array): element stride of each destination, default 1 */
/* out[r*nseg + s] = sum of x[r*ld + e] over e in [seg_off[s], seg_off[s+1])  (per-shape sums of SDFNet dZ columns) */
int sg_segsum(const float* x, float* out, long rows, long ld, const int64_t* seg_off, long nseg, hipStream_t stream);

/* ---- K4: nn.BatchNorm3d / nn.BatchNorm1d (+ fused following activation) -------------------------------------
 * reference: model/gan.py:10,14,18; model/autoencoder.py:17,21,25,29,38,46,56,60,64 -> aten::batch_norm(_backward).
 * x [N,C,S]; momentum/eps as torch (0.1 / 1e-5); running_var gets the unbiased estimate. */
size_t sg_bn_workspace_bytes(int C);
/* The launch plan of the entries below for x [N,C,S] (host code, no GPU needed): *nsplit slices per channel in the statistics passes
 * (at most 64), *napply >= *nsplit in the apply passes.  S % 4 == 0 takes the float4 form of every kernel, anything else the scalar one. */
int sg_bn_plan(int N, int C, long S, int* nsplit, int* napply);
int sg_bn_train_fwd(const float* x, const float* gamma, const float* beta, float* y, float* save_mean, float* save_invstd,
                    float* running_mean, float* running_var, long long* num_batches_tracked, int N, int C, long S,
                    float eps, float momentum, int act, float slope, void* workspace, size_t workspace_bytes,
                    hipStream_t stream);
/* Batch statistics WITHOUT the normalised output: mean / invstd, the running-statistics update exactly as sg_bn_train_fwd does
 * it, and the affine map scale[c] = gamma[c] * invstd[c], shift[c] = beta[c] - mean[c] * scale[c] that a consumer applies on its
 * loads (sg_convT3d_k4s2p1_to1_pre). */
int sg_bn_train_stats(const float* x, const float* gamma, const float* beta, float* save_mean, float* save_invstd,
                      float* running_mean, float* running_var, long long* num_batches_tracked, float* scale, float* shift, int N,
                      int C, long S, float eps, float momentum, void* workspace, size_t workspace_bytes, hipStream_t stream);
/* The two above for a tensor [groups][N][C][S] whose groups are independent batches (statistics per group; save_mean / save_invstd
 * / scale / shift are [groups][C]; workspace: groups * sg_bn_workspace_bytes(C)).  The running statistics receive the groups'
 * updates one after the other, exactly as `groups` separate calls would apply them; num_batches_tracked += groups. */
int sg_bn_train_fwd_grouped(const float* x, const float* gamma, const float* beta, float* y, float* save_mean, float* save_invstd,
                            float* running_mean, float* running_var, long long* num_batches_tracked, int groups, int N, int C,
                            long S, float eps, float momentum, int act, float slope, void* workspace, size_t workspace_bytes,
                            hipStream_t stream);
int sg_bn_train_stats_grouped(const float* x, const float* gamma, const float* beta, float* save_mean, float* save_invstd,
                              float* running_mean, float* running_var, long long* num_batches_tracked, float* scale, float* shift,
                              int groups, int N, int C, long S, float eps, float momentum, void* workspace, size_t workspace_bytes,
                              hipStream_t stream);
int sg_bn_eval_fwd(const float* x, const float* gamma, const float* beta, float* y, const float* running_mean,
                   const float* running_var, float* save_mean, float* save_invstd, int N, int C, long S, float eps,
                   int act, float slope, hipStream_t stream);
int sg_bn_bwd(const float* dy, const float* x, const float* gamma, const float* beta, const float* save_mean,
              const float* save_invstd, float* dx, float* dgamma, float* dbeta, int N, int C, long S, int train, int act,
              float slope, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* ---- K5: activations (standalone; normally fused into K1-K4/K7 epilogues) ------------------------------------
 * sg_act_bwd takes the activation OUTPUT y (LeakyReLU/ReLU masks, 1-y^2, y(1-y)); it is also LeakyReLU's
 * double-backward (mask * gg) used by the WGAN-GP graph (train_hybrid_progressive_gan.py:102-111). */
int sg_act_fwd(const float* x, float* y, long n, int act, float slope, hipStream_t stream);
int sg_act_bwd(const float* y, const float* dy, float* dx, long n, int act, float slope, hipStream_t stream);
/* dx = dy * act'(y) and rowsum[r] = sum of dx over row r of S voxels (r = sample * C + channel): the activation backward of a
 * conv layer with the row sums its bias gradient needs, in one pass */
int sg_act_bwd_rowsum(const float* y, const float* dy, float* dx, float* rowsum, long rows, long S, int act, float slope,
                      hipStream_t stream);

/* ---- K7: SDFNet fused MLP -------------------------------------------------------------------------------------
 * reference: SDFNet.forward, model/sdf_net.py:26-61 (+ autograd).  `params` = 16 device pointers in state_dict order
 * (layers1.{0,2,4,6}.{weight,bias}, layers2.{0,2,4,6}.{weight,bias}).  sg_sdfnet_pack builds the MFMA-fragment
 * image of the weights (call once per optimizer step); kin_used = 3+latent (per-point latents, reference
 * semantics) or 3 (per-shape latents folded into zb1/zb5 biases; replaces the [B*R^3, L] tiling of
 * train_hybrid_wgan.py:67-70 / train_hybrid_progressive_gan.py:90-93). */
size_t sg_sdfnet_packed_floats(int kin_used);
/* floats of the activation buffer `acts` of a training call (sg_sdfnet_fwd writes it, sg_sdfnet_bwd and the weight-gradient
 * GEMMs read it): the fp32 images H1..H7 [7][256][ldn], followed by their SIGN MASKS, unsigned short [7][16][ldn] — bit q of
 * mask[l][2 w + h][p] is (H_{l+1}[32 w + (q & 3) + 8 (q >> 2) + 4 h][p] > 0), one 16-bit word per point and group of 16 rows.
 * The backward takes ReLU' of H1..H6 from the masks (1/32 of the bytes) instead of re-reading the images. */
size_t sg_sdfnet_acts_floats(long ldn);
int sg_sdfnet_pack(const float* const* params, int latent, int kin_used, float* packed, hipStream_t stream);
int sg_sdfnet_fwd(const float* points, long points_period, const float* latent, const int64_t* latent_idx,
                  int latent_size, const float* packed, int kin_used, const float* zb1, const float* zb5,
                  long points_per_shape, const int* shape_index, float* out, float* acts, long ldn, long N,
                  hipStream_t stream);
/* Point tiles of the backward = rows of bias_partials: tile t covers the points [sg_sdfnet_bwd_tile_start(N, t),
 * sg_sdfnet_bwd_tile_start(N, t + 1)).  With tiles = ceil(N / 64), rem = tiles % 512, full = tiles - rem: 64 points per tile,
 * except for the last, partly filled round of workgroups (512 = two per CU):
 *   256 < rem <= 384: 64-point tiles up to full + 256 (one more per CU), the points after them in 32-point tiles;
 *   full > 0 and 0 < rem <= 256: the points from 64 * full on in 32-point tiles.
 * A pure function of N: the layout does not depend on the device. */
long sg_sdfnet_bwd_blocks(long N);
long sg_sdfnet_bwd_tile_start(long N, long t);
/* bias_partials (optional): TILE-MAJOR [blocks][SG_SDFNET_PARTIAL_ROW] (ABI 7; it was [14*256][blocks]: 3 584 scattered 4-byte
 * writes per tile).  Row t holds the sums over the points of tile t: floats [256 b, 256 b + 256), b = 0..6: the row sums of
 * dZ_{b+1} (sum over the tiles: bias gradients); float 14*256: the sum of dz8 (the layers2.6 bias gradient).  With `points` (the
 * xyz of the batch, as given to sg_sdfnet_fwd) also b = 7: sum_p dz8[p] H7[row][p] (the layers2.6 weight gradient) and b = 8+c /
 * 11+c: sum_p dZ1 / dZ5 [row][p] * xyz_c[p] (the three point columns of the layers1.0 / layers2.0 weight gradients) — sums the
 * kernel has the operands on chip for, instead of three more passes over the [256][N] images.  sg_sdfnet_bwd_finish reduces
 * them. */
#define SG_SDFNET_PARTIAL_ROW 3616 /* 14 * 256 + 32 */
#define SG_SDFGEN_PARTIAL_ROW 7200 /* SG_SDFNET_PARTIAL_ROW + 14 * 256: the LayerNorm form (sg_sdfgen_bwd) */
int sg_sdfnet_bwd(const float* dout, const float* out, const float* acts, float* dz, float* dz8, float* bias_partials,
                  const float* points, long points_period, float* dx, long dx_ld, const float* packed, int kin_used, long ldn,
                  long N, hipStream_t stream);
/* Per-shape mode: the latent fold zb1[s][o] = b1[o] + sum_k z[s][k] W1[o][3+k], zb5[s][o] = b5[o] + sum_k z[s][k] W5[o][259+k]
 * (W1 [256][3+L], W5 [256][259+L]: the reference multiplies these columns with the tiled latents of every point,
 * model/sdf_net.py:27,41,57-59), both [nshapes][256] outputs in one launch, accumulated in double and rounded once. */
int sg_sdfnet_shape_bias(const float* z, long nshapes, int latent, const float* W1, const float* b1, const float* W5, const float* b5,
                         float* zb1, float* zb5, hipStream_t stream);
/* sg_sdfnet_pack(params, latent, 3, packed) and sg_sdfnet_shape_bias(z, ..., zb1, zb5) of the same parameters in ONE launch (ABI 8):
 * every step of the shape-sorted auto-decoder needs both behind its optimizer step (train_sdf_autodecoder.py:80-91). */
int sg_sdfnet_pack_shape_bias(const float* const* params, int latent, float* packed, const float* z, long nshapes, float* zb1,
                              float* zb5, hipStream_t stream);
/* Per-shape mode: backward of the latent fold zb1[s][o] = b1[o] + sum_k z[s][k] W1[o][3+k], zb5[s][o] = b5[o] + sum_k z[s][k] W5[o][259+k]
 * (the latent columns of layers1.0 / layers2.0, model/sdf_net.py:27,41, enter sg_sdfnet_fwd as bias rows) from the per-shape sums
 * t1 / t5 [256][nshapes] of dZ1 / dZ5, in one launch: the latent columns of dW1 [256][3+L] / dW5 [256][259+L] written in place
 * (NULL, NULL to skip) and the latent gradient gz [nshapes][L] (NULL to skip); nshapes <= 6144. */
/* (reg_scale != 0: gz additionally receives reg_weight[s] * reg_scale * z[s][k] (reg_weight NULL: 1) — the gradient of the DeepSDF
 * latent regulariser SIGMA * mean(z_batch^2) through shape counts (train_sdf_autodecoder.py:88), so that the latent table gets ONE
 * gradient contribution, written where its flat-buffer slice lives, instead of two tensors that autograd adds and the optimizer copies) */
int sg_sdfnet_shape_bias_bwd(const float* t1, const float* t5, long nshapes, const float* z, int latent, const float* W1,
                             const float* W5, float* dW1, float* dW5, float* gz, const float* reg_weight, float reg_scale,
                             hipStream_t stream);
/* Everything that is derived from the bias_partials of ONE sg_sdfnet_bwd call, in one launch (replaces five: the segment sums,
 * two multi-row sums and the two-stage sum of dz8 of train_sdf_autodecoder.py:80-91's backward):
 *   bias_grads[0..6] (256 floats each; NULL: skip all column sums), b8_grad[1], and with `extended` (sg_sdfnet_bwd was given
 *   `points`) w8_grad[256] and the three point columns of dW1 / dW5: element (row, c) at w1_cols[row * w1_ld + c] / w5_cols[...];
 *   nseg > 0: t1[256][nseg], t5[256][nseg] = sums of dZ1 / dZ5 over every segment [seg_off[s], seg_off[s+1]) of points (per-shape
 *   sums: the latent-table gradient and the latent columns of the layers1.0 / layers2.0 weight gradients of the shape-sorted step),
 *   interior tiles from the partials, the cut tiles from `dz`.
 * Deterministic (two-level column sums, added in split order by whichever block finishes last).  `tickets`: 16 unsigned, zero
 * before the first call; every call leaves them zero (one buffer per stream of concurrent calls). */
size_t sg_sdfnet_bwd_finish_workspace_bytes(long N);
int sg_sdfnet_bwd_finish(const float* dz, const float* bias_partials, long ldn, long N, int extended, float* const* bias_grads,
                         float* w8_grad, float* b8_grad, float* w1_cols, long w1_ld, float* w5_cols, long w5_ld,
                         const int64_t* seg_off, long nseg, float* t1, float* t5, void* workspace, size_t workspace_bytes,
                         unsigned* tickets, hipStream_t stream);

/* ---- K7c: latent codes of unseen shapes — the loss and its latent-only gradient with the weights frozen (serves
 * shapegan_amd/reconstruct.py fit_latent_codes and SDFNet.latent_loss_and_grad; the reference has no encoder and never wrote the
 * fit: create_plot.py's sdf_net_reconstruction only renders training codes).  Additions to ABI 8, backward compatible.
 * Shape s owns the points [seg_off[s], seg_off[s+1]) of points [*][3] / target [*] (n_s of them, n_s >= 1) and uses
 * m_s = n_s (win_count <= 0) or min(win_count, n_s) of them: used point i < m_s is seg_off[s] + (win_start + i) mod n_s.
 * Tiles of SG_SDFNET_LATENT_TILE used points never straddle shapes: shape s has ceil(m_s / TILE) of them, laid end to end in
 * shape order; tiles [T][2] (int32: shape, first used point i of the tile) and tile_off [S+1] (int64: shape s owns the tiles
 * [tile_off[s], tile_off[s+1])) are built by the caller once per fit.
 * sg_sdfnet_latent_grad: one launch; per tile the forward of sg_sdfnet_fwd (per-shape mode, zb1 / zb5 [S][256] of
 *   sg_sdfnet_shape_bias, packed with kin_used = 3; bit for bit), out = tanh(v), d = out - clamp(target, +-cutoff),
 *   dz8 = sign(d) (1 - out^2) / m_s with sign(0) = 0, and the backward chain through the transposed packs with ReLU' from sign words
 *   that never leave the chip.  partials [T][SG_SDFNET_LATENT_PARTIAL_ROW]: floats [0, 256) the tile's row sums of dZ1, [256, 512)
 *   of dZ5, float 512 its sum of |d|; every row is written in full.  A shape's rows do not depend on the other shapes of the call.
 *   SG_ERR_ARG: nshapes < 1, win_start < 0, ntiles < 1 (an empty shape is refused where seg_off can be read: by the twin, and by
 *   the caller that builds the tile table).
 * sg_sdfnet_latent_reduce: t1 / t5 [256][nshapes] (the layout sg_sdfnet_shape_bias_bwd takes: dW1 = dW5 = NULL, gz, reg_scale =
 *   2 sigma / L give the gradient of the objective with sigma mean_k z_k^2) and loss [nshapes] = sum |d| / m_s; a shape's tiles
 *   are added in tile order in double: deterministic. */
#ifndef SG_SDFNET_LATENT_TILE
#define SG_SDFNET_LATENT_TILE 32
#endif
#define SG_SDFNET_LATENT_PARTIAL_ROW 513 /* 2 * 256 + 1 */
int sg_sdfnet_latent_grad(const float* points, const float* target, const int64_t* seg_off, long nshapes, const float* zb1,
                          const float* zb5, const float* packed, float cutoff, long win_start, long win_count, const int* tiles,
                          long ntiles, float* partials, hipStream_t stream);
int sg_sdfnet_latent_reduce(const float* partials, const int64_t* tile_off, const int64_t* seg_off, long nshapes, long win_count,
                            float* t1, float* t5, float* loss, hipStream_t stream);

/* ---- K7e: the pose of a cloud fitted together with its latent code (csrc/latent_fit.hip; serves shapegan_amd/reconstruct.py
 * fit_codes_and_poses and SDFNet.latent_pose_loss_and_grad).  Additions to ABI 8, backward compatible.  Everything K7c says about
 * points, target, seg_off, the window, tiles and tile_off holds; `points` are OBSERVED coordinates q, and shape s carries
 * pose [S][16] (floats): floats 0..11 a row-major 3x4 affine A|t that maps q to canonical x = A q + t, float 12 the target scale ts,
 * floats 13..15 ignored.
 * sg_sdfnet_latent_pose_grad: one launch; per tile, in float32 and in this order,
 *     x_c = fma(A_c0, qx, fma(A_c1, qy, fma(A_c2, qz, t_c)))      (c = 0, 1, 2)
 *   then K7c at x with target' = clamp(ts * target, +-cutoff): out = tanh(v), d = out - target', dz8 = sign(d) (1 - out^2) / m_s, the
 *   chain back, and the point gradient of K7d, g = W5[:, 256:259]^T dZ5 + W1[:, 0:3]^T dZ1, which stays on the chip; per point also
 *   e = -sign(d) target / m_s where -cutoff < ts * target < cutoff, else 0.
 *   partials [T][SG_SDFNET_POSE_PARTIAL_ROW]: floats [0, 513) as K7c's row; [513, 522) sum_p g_c q_j, row-major (c, j): d loss / dA;
 *   [522, 525) sum_p g_c: d loss / dt; 525 sum_p e: d loss / d ts; 526, 527 zero.  Every row is written in full, the row of a tile
 *   that names nothing (all zeros) included; every sum has a fixed order, so a shape's rows do not depend on the other shapes of the
 *   call.  With the identity pose and ts = 1, floats [0, 513) equal sg_sdfnet_latent_grad's bit for bit.
 * sg_sdfnet_latent_pose_reduce: t1, t5, loss as sg_sdfnet_latent_reduce, and gpose [nshapes][16]: floats 0..11 the gradient of
 *   loss_s with respect to A|t in pose's layout, float 12 with respect to ts, floats 13..15 zero; a shape's tiles are added in tile
 *   order in double.
 * SG_ERR_ARG before any launch: a NULL pointer, nshapes < 1, ntiles < 1 or >= 2^31, win_start < 0, cutoff < 0. */
#define SG_SDFNET_POSE_PARTIAL_ROW 528 /* 513 + 9 + 3 + 1 + 2 */
int sg_sdfnet_latent_pose_grad(const float* points, const float* target, const int64_t* seg_off, long nshapes, const float* zb1,
                               const float* zb5, const float* packed, const float* pose, float cutoff, long win_start,
                               long win_count, const int* tiles, long ntiles, float* partials, hipStream_t stream);
int sg_sdfnet_latent_pose_reduce(const float* partials, const int64_t* tile_off, const int64_t* seg_off, long nshapes,
                                 long win_count, float* t1, float* t5, float* loss, float* gpose, hipStream_t stream);

/* ---- K7d: points onto a level set of a frozen SDFNet — value, point gradient and Newton steps of a tile in one launch (serves
 * SDFNet.sdf_and_gradient / project_to_level_set and shapegan_amd/surface.py: exact normals, refined meshes, oriented surface
 * clouds).  The reference takes normals and surface points from autograd with respect to the points and one first-order step that
 * assumes |grad f| = 1 (model/sdf_net.py:118-156).  Addition to ABI 8, backward compatible.
 * points [N][3] are grouped by shape: shape s owns [seg_off[s], seg_off[s+1]).  zb1 / zb5 [S][256] come from sg_sdfnet_shape_bias,
 * `packed` is packed with kin_used = 3.  tiles [T][2] (int32: shape, first point of the tile within the shape) are built by the
 * caller as for K7c: SG_SDFNET_PROJECT_TILE points each, never straddling shapes; a row that names nothing (shape outside
 * [0, nshapes), negative first point, first point beyond the run) is skipped.
 * Per tile, `iterations + 1` rounds of: the forward of sg_sdfnet_fwd (per-shape mode, bit for bit) at the tile's current points,
 * out = tanh(v), dz8 = 1 - out^2, the backward chain through the transposed packs with ReLU' from sign words that never leave the
 * chip, and g = W5[:, 256:259]^T dZ5 + W1[:, 0:3]^T dZ1 per point.  On all rounds but the last the point moves (float32, in this
 * order; csrc/project_core.h is the one statement both libraries compile):
 *   d = out - level;  n2 = fma(gx, gx, fma(gy, gy, gz gz));  t = d / n2 (rule 0, Newton) or d / sqrt(n2) (rule 1, the reference's
 *   step);  s = t g;  len = |t| sqrt(n2);  max_step > 0 and len > max_step: s *= max_step / len;  !(n2 > 0) or a component of s not
 *   finite: s = 0;  x -= s.
 * out_points [N][3]: x after `iterations` steps (NULL allowed only with iterations == 0; may alias `points`: a tile reads all its
 * points before it writes any); value [N]: f at out_points; grad [N][3]: grad f at out_points, unnormalised.  Every element of every
 * row a tile names is written, ragged last tiles included; nothing is read from the outputs.  With iterations == 0 `value` is
 * sg_sdfnet_fwd's bit for bit.  A point's outputs do not depend on what else is in the call or where it stands: there is no
 * reduction across points and the k order of its sums is fixed.
 * SG_ERR_ARG before any launch: a NULL pointer, nshapes < 1, ntiles < 1 or >= 2^31, iterations outside [0, 64], rule outside {0, 1},
 * max_step < 0, out_points == NULL with iterations > 0. */
#define SG_SDFNET_PROJECT_TILE 32
int sg_sdfnet_project(const float* points, const int64_t* seg_off, long nshapes, const float* zb1, const float* zb5,
                      const float* packed, float level, int iterations, int rule, float max_step, const int* tiles, long ntiles,
                      float* out_points, float* value, float* grad, hipStream_t stream);

/* ---- K7b: the LayerNorm form of the fused MLP — SDFGenerator (model/point_sdf_net.py:49-119) with hidden_channels 256 and
 * num_layers 8: x = relu(LayerNorm(lin_i(x) [+ z_lin(z)])) for i = 0..6 (:104-116), cat([x, pos]) in front of lins.4 (:100), a
 * plain Linear(256, 1) at the end (ABI 8).  The eight Linear layers have the shapes of an SDFNet without latent columns, so the
 * kernels are those of K7 with the LayerNorm statistics combined across the waves of a tile through LDS; the latent enters as
 * the per-shape rows zb1 = z_lin1(z) + lins.0.bias, zb5 = z_lin2(z) + lins.4.bias ([S,256], built by the caller: two small
 * Linear layers).  `params`: lins.{0..7}.{weight,bias} (16 pointers); `norm_params`: norms.{0..6}.{weight,bias} (14 pointers);
 * `packed`: sg_sdfnet_packed_floats(3) floats.
 * Training: `acts` (sg_sdfgen_acts_floats(ldn) floats) receives the images xhat_l = (x - mean) * rstd [7][256][ldn] (the
 * LayerNorm backward needs them where the ReLU is off too), the sign masks of the ReLU inputs (layout of sg_sdfnet_acts_floats)
 * and rstd [7][ldn].  sg_sdfgen_bwd (32-point tiles, sg_sdfgen_bwd_blocks(N) of them) writes dz8 = dout, the images dZ_l (gradient
 * of the LayerNorm INPUT) and per-tile partial sums [blocks][SG_SDFGEN_PARTIAL_ROW]: the SDFNet row (b = 0..13 and float 14*256,
 * see sg_sdfnet_bwd) followed at float SG_SDFNET_PARTIAL_ROW by 7 blocks sum_p dY_l xhat_l (LayerNorm weight gradients) and 7
 * blocks sum_p dY_l (LayerNorm bias gradients).  sg_sdfgen_bwd_finish reduces them (norm_grads[0..6]: weight, [7..13]: bias
 * gradients; tickets: 32 unsigned, zero); the six 256 x 256 weight gradients are sg_gemm_nt_batched_lnrelu products of the dZ and
 * xhat images. */
size_t sg_sdfgen_acts_floats(long ldn);
long sg_sdfgen_packed_norm_offset(int which); /* float offset of the packed LayerNorm weight (0) / bias (1) vectors [7][256] */
int sg_sdfgen_pack(const float* const* params, const float* const* norm_params, float* packed, hipStream_t stream);
int sg_sdfgen_fwd(const float* points, const float* packed, const float* zb1, const float* zb5, long points_per_shape,
                  const int* shape_index, float eps, float* out, float* acts, long ldn, long N, hipStream_t stream);
long sg_sdfgen_bwd_blocks(long N);
int sg_sdfgen_bwd(const float* dout, const float* acts, float* dz, float* dz8, float* partials, const float* points,
                  const float* packed, long ldn, long N, hipStream_t stream);
size_t sg_sdfgen_bwd_finish_workspace_bytes(long N);
int sg_sdfgen_bwd_finish(const float* dz, const float* partials, long ldn, long N, float* const* bias_grads, float* w8_grad,
                         float* b8_grad, float* w1_cols, long w1_ld, float* w5_cols, long w5_ld, float* const* norm_grads,
                         const int64_t* seg_off, long nseg, float* t1, float* t5, void* workspace, size_t workspace_bytes,
                         unsigned* tickets, hipStream_t stream);

/* ---- K8/K9/K10/K11: blends, reductions, latent-table rows, optimizers ------------------------------------------
 * reference: fade-in / GP lerp (model/progressive_gan.py:50, train_hybrid_progressive_gan.py:105), batch means
 * (train_wgan.py:68,82), latent_codes[model_indices] (train_sdf_autodecoder.py:78-82), optim.RMSprop / optim.Adam
 * with torch defaults (train_wgan.py:45-46, train_autoencoder.py:35, ...), clip_weights (model/gan.py:67-69;
 * fused into the RMSprop step when clip > 0). grad_scale multiplies the gradient on load (1/world for DP). */
int sg_axpby(const float* x, const float* y, float* out, long n, float a, float b, hipStream_t stream);
size_t sg_reduce_workspace_bytes(void);
int sg_reduce_sum(const float* x, float* out, long n, float scale, void* workspace, size_t workspace_bytes,
                  hipStream_t stream);
int sg_gather_rows(const float* table, const int64_t* idx, float* out, long n, int L, hipStream_t stream);
int sg_scatter_add_rows(const float* rows, long rows_ld, const int64_t* idx, float* table_grad, long n, int L,
                        hipStream_t stream);
/* Batch assembly of the auto-decoder step in shape-sorted order (train_sdf_autodecoder.py:78-85: model_indices =
 * indices // POINTCLOUD_SIZE, points[indices], sdf[indices]) as ONE stable counting sort on the shape id: out_points[n,3] /
 * out_sdf[n] / out_shape[n] hold the batch grouped by shape (entries of a shape keep their order in `indices`),
 * seg_off[nshapes+1] bounds every shape's run, counts[nshapes] = run lengths as floats (weights of the latent regulariser).
 * nshapes <= sg_sdf_batch_sort_max_shapes(); an index outside [0, nshapes*pointcloud_size) — an IndexError in the reference —
 * sets *bad_index_flag and is clamped.  The flag is an int the kernel can write — device memory, or pinned host memory (what the
 * Python shell passes: the host then polls it with a plain load, no copy / launch / synchronisation per step); sticky, caller-zeroed,
 * written only when an index is bad: it receives bad_index_value (!= 0; e.g. a call sequence number).  bad_index_device (optional):
 * a second sticky word, in DEVICE memory, set together with the first — the `skip_if_nonzero` word of sg_adam_step_guarded: the
 * reference raises before any update (train_sdf_autodecoder.py:79 -> :90-91), here the optimizer kernels behind the sort in the same
 * stream turn into no-ops from that batch on and the host raises when it next looks at the first word.  With the device word
 * given, both words keep the value of the FIRST call that met a bad index until the caller zeroes them. */
int sg_sdf_batch_sort_max_shapes(void);
size_t sg_sdf_batch_sort_workspace_bytes(long n, long nshapes);
int sg_sdf_batch_sort(const int64_t* indices, long n, long pointcloud_size, long nshapes, const float* points,
                      const float* sdf, float* out_points, float* out_sdf, int* out_shape, int64_t* seg_off, float* counts,
                      int* bad_index_flag, int* bad_index_device, int bad_index_value, void* workspace, size_t workspace_bytes,
                      hipStream_t stream);
int sg_rmsprop_step(float* p, const float* g, float* square_avg, long n, float lr, float alpha, float eps,
                    float grad_scale, float clip, hipStream_t stream);
int sg_adam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1, float beta2,
                 float eps, long step, float grad_scale, hipStream_t stream);
/* Adam with the step counter (int64) in device memory: identical arithmetic, but the call has no host-side state that changes
 * between steps, so a captured hipGraph of a training step replays it.  corr_dev: SG_ADAM_DEV_WORDS 32-bit words, zero before the
 * first call — [0..1] the two bias corrections of the last applied step (for the host to read), [2] and [32 + 32 i], i < 16: the
 * arrival tickets of the one launch (the workgroup that is last to have read the counter advances it; two levels, 128 bytes apart:
 * atomics on one word are served one after the other), left at zero by every call. */
#define SG_ADAM_DEV_WORDS 544
int sg_adam_step_dev(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1, float beta2,
                     float eps, long long* step_dev, float* corr_dev, float grad_scale, hipStream_t stream);
/* The two Adam entries with a guard word (device memory, may be NULL = unguarded): when *skip_if_nonzero != 0 at the time the
 * kernels run, parameters, both moments and (…_dev) the device step counter are left exactly as they were. */
int sg_adam_step_guarded(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1, float beta2,
                         float eps, long step, float grad_scale, const int* skip_if_nonzero, hipStream_t stream);
int sg_adam_step_dev_guarded(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long n, float lr, float beta1,
                             float beta2, float eps, long long* step_dev, float* corr_dev, float grad_scale,
                             const int* skip_if_nonzero, hipStream_t stream);
/* sg_adam_step_dev_guarded for up to four flat buffers in ONE launch (ABI 8): the optimizers of one training step
 * (train_sdf_autodecoder.py:44-45,90-91 steps the network's and the latent table's one after the other).  Every argument is an array
 * of nsets entries; one guard word (may be NULL) covers all. */
int sg_adam_step_dev_multi(int nsets, float* const* p, const float* const* g, float* const* exp_avg, float* const* exp_avg_sq,
                           const long* n, const float* lr, const float* beta1, const float* beta2, const float* eps,
                           long long* const* step_dev, float* const* corr_dev, const float* grad_scale, const int* skip_if_nonzero,
                           hipStream_t stream);
int sg_clamp(float* p, long n, float lo, float hi, hipStream_t stream);
/* clamp of `ntensors` tensors (host arrays of device pointers and element counts) in one launch per 16 tensors:
 * Discriminator.clip_weights (model/gan.py:67-69) over the module-level surface, eight parameter tensors per critic update */
int sg_clamp_multi(float* const* tensors, const long* counts, int ntensors, float lo, float hi, hipStream_t stream);

/* ---- K8/K9: loss compositions, gradient-penalty pieces, fade-in blend ---------------------------
 * Each loss is one streaming pass + a finishing wave (deterministic, double partial sums) writing a device scalar;
 * each backward is one elementwise pass that reads the upstream scalar gradient `gloss` from device memory.
 * sg_loss_weighted_l1: get_reconstruction_loss, train_autoencoder.py:57-62 (neg_weight 32: d *= 32 where target < 0),
 *   and with neg_weight 1 the DeepSDF data term mean|out - sdf|, train_sdf_autodecoder.py:88.
 * sg_loss_kld: kld_loss, train_autoencoder.py:54-55.
 * sg_loss_meansq: sum_r w_r |x_r|^2 / denom (w = 1 when row_weight is null): the latent regulariser
 *   mean(batch_latent_codes^2), train_sdf_autodecoder.py:88 (row_weight = how often a shape occurs in the batch).
 * sg_gradient_penalty: ((||g_b||_2 - 1)^2).mean() * weight over rows g_b of `grad` [B, M],
 *   train_hybrid_progressive_gan.py:110-111, train_point_gan.py:68-70; sg_lerp_rows: alpha*real + (1-alpha)*fake (:105).
 * sg_fade_blend: fade*x + half_scale*from_SDF(half) (model/progressive_gan.py:48-50): `half` [B,S] lands on channel 0 of
 *   x [B,C,S], the C-1 zero channels of from_SDF are never built (x may be NULL: the embedding alone); sg_channel0 is its
 *   adjoint w.r.t. `half`; sg_subsample2 / _adjoint: x_in[:, ::2, ::2, ::2] (bit-exact index work) and its adjoint. */
size_t sg_loss_workspace_bytes(void);
int sg_loss_weighted_l1_fwd(const float* out, const float* target, long n, float neg_weight, float* loss, void* workspace,
                            size_t workspace_bytes, hipStream_t stream);
int sg_loss_weighted_l1_bwd(const float* out, const float* target, const float* gloss, float* dout, long n, float neg_weight,
                            hipStream_t stream);
/* w_first * mean(x[0, n_first)) + w_rest * mean(x[n_first, n)) and its backward dx = gloss * (w / count) per part, one small
 * launch each: the WGAN losses mean(fake) - mean(real) over the critic's concatenated batch (train_wgan.py:68,
 * train_hybrid_wgan.py:89, train_hybrid_progressive_gan.py:147) and -mean(fake) (train_wgan.py:82; n_first = n, w_first = -1) */
int sg_loss_mean_split_fwd(const float* x, long n, long n_first, float w_first, float w_rest, float* loss, float* dx_unit,
                           hipStream_t stream);   /* dx_unit (optional, [n]): the backward for gloss == 1, from the same launch */
int sg_loss_mean_split_bwd(const float* gloss, float* dx, long n, long n_first, float w_first, float w_rest, hipStream_t stream);
/* Classic-GAN losses on the [B] vector of discriminator outputs, train_gan.py:30,78,84 (torch.nn.functional.binary_cross_entropy
 * against a constant target: mean of -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)), backward g (p - t) / max((1 - p) p,
 * 1e-12) / n as torch computes it) and train_gan.py:65 (-torch.mean(torch.log(p))). */
int sg_loss_bce_fwd(const float* p, long n, float target, float* loss, hipStream_t stream);
int sg_loss_bce_bwd(const float* p, const float* gloss, float* dp, long n, float target, hipStream_t stream);
int sg_loss_neg_mean_log_fwd(const float* p, long n, float* loss, hipStream_t stream);
int sg_loss_neg_mean_log_bwd(const float* p, const float* gloss, float* dp, long n, hipStream_t stream);
/* VAE reparameterisation, model/autoencoder.py:77-82: z = mean + exp(0.5 log_variance) * eps (eps drawn by the caller);
 * backward: d mean = gz (no kernel), d log_variance = gz * eps * 0.5 * exp(0.5 log_variance). */
int sg_vae_reparam_fwd(const float* mean, const float* log_variance, const float* eps, float* z, long n, hipStream_t stream);
int sg_vae_reparam_bwd(const float* log_variance, const float* eps, const float* gz, float* dlog_variance, long n,
                       hipStream_t stream);
/* The critic's last layer together with the activation below it, model/gan.py:54-55 (LeakyReLU -> Conv3d(256 -> 1, kernel 4,
 * stride 1) on a 4^3 grid = one dot product over K = C * 64 values per sample):
 *   fwd  y[n] = bias[0] + sum_k act(z[n, k]) * w[k]          z [N, K] = the PRE-activation of the layer below, act in {none,
 *                                                            leaky, relu} is applied on load
 *   bwd  gz[n, k] = gy[n] * w[k] * act'(z[n, k]);  gw[k] = sum_n gy[n] * act(z[n, k]);  gb[0] = sum_n gy[n];
 *        gbz[c] = sum_{n, s} gz[n, c * S + s]  (the bias gradient of the layer below)     gw / gb / gbz optional, S must be 64
 * One streaming pass each way; every sum in a fixed order. */
int sg_head_dot_fwd(const float* z, const float* w, const float* bias, float* y, int N, long K, int act, float slope,
                    hipStream_t stream);
int sg_head_dot_bwd(const float* z, const float* w, const float* gy, float* gz, float* gw, float* gb, float* gbz, void* gz_image,
                    int N, int C, int S, int act, float slope, hipStream_t stream);
/* gz_image (optional; C a multiple of 128): gz once more, in the A-fragment order of the LDS-halo weight-gradient kernel for 4^3
 * grids, so that the convolution below needs no packing pass over gz — see sg_conv3d_k4s2p1_wgrad_dy_image. */
int sg_loss_kld_fwd(const float* mean, const float* log_variance, long n, float* loss, void* workspace, size_t workspace_bytes,
                    hipStream_t stream);
int sg_loss_kld_bwd(const float* mean, const float* log_variance, const float* gloss, float* dmean, float* dlog_variance,
                    long n, hipStream_t stream);
int sg_loss_meansq_fwd(const float* x, const float* row_weight, long rows, int L, double denom, float* loss, void* workspace,
                       size_t workspace_bytes, hipStream_t stream);
int sg_loss_meansq_bwd(const float* x, const float* row_weight, const float* gloss, float* dx, long rows, int L, double denom,
                       hipStream_t stream);
/* The whole DeepSDF loss of train_sdf_autodecoder.py:88, loss = mean|out - target| + sum_r w_r |z_r|^2 / denom, as ONE pass over
 * both operands + the finishing wave, and its backward (dout[n], dz[rows][L]) as one launch: the arithmetic and its order are
 * those of sg_loss_weighted_l1 with neg_weight 1, sg_loss_meansq and an fp32 add of the two rounded terms, bit for bit. */
int sg_loss_deepsdf_fwd(const float* out, const float* target, long n, const float* z, const float* row_weight, long rows, int L,
                        double denom, float* loss, void* workspace, size_t workspace_bytes, hipStream_t stream);
int sg_loss_deepsdf_bwd(const float* out, const float* target, long n, const float* z, const float* row_weight, long rows, int L,
                        double denom, const float* gloss, float* dout, float* dz, hipStream_t stream);
/* The same loss AND its gradient for an upstream gradient of exactly 1 (dout_unit[n], dz_unit[rows][L]; either may be NULL) in
 * ONE launch: the loss is the root of the trainer's backward (train_sdf_autodecoder.py:88-89).  Bit-identical to
 * sg_loss_deepsdf_fwd / sg_loss_deepsdf_bwd with gloss = 1; the workgroup that arrives last runs the finishing wave.
 * `ticket`: one unsigned, zero before the first call, left zero. */
int sg_loss_deepsdf_fused(const float* out, const float* target, long n, const float* z, const float* row_weight, long rows, int L,
                          double denom, float* loss, float* dout_unit, float* dz_unit, void* workspace, size_t workspace_bytes,
                          unsigned* ticket, hipStream_t stream);
/* voxel_difference, train_autoencoder.py:50-52: count[0] = #{e : (a[e] * b[e]) < 0} with the product rounded to fp32 as the
 * reference's `(input * target) < 0` does (a product that underflows to -0, or a NaN, does not count).  Integer arithmetic
 * throughout: bit-exact.  The caller divides by n (`torch.sum(wrong_signs).item() / wrong_signs.nelement()`). */
int sg_count_sign_mismatch(const float* a, const float* b, long n, long long* count, void* workspace, size_t workspace_bytes,
                           hipStream_t stream);
int sg_gradient_penalty_fwd(const float* grad, long B, long M, float weight, float* norms, float* loss, hipStream_t stream);
int sg_gradient_penalty_bwd(const float* grad, const float* norms, const float* gloss, float* dgrad, long B, long M,
                            float weight, hipStream_t stream);
int sg_lerp_rows(const float* a, const float* b, const float* alpha, float* out, long B, long M, hipStream_t stream);
int sg_fade_blend(const float* x, const float* half, float* out, long B, int C, long S, float fade, float half_scale,
                  hipStream_t stream);
int sg_channel0(const float* g, float* out, long B, int C, long S, float scale, hipStream_t stream);
int sg_subsample2(const float* x, float* out, long B, int R, hipStream_t stream);
int sg_subsample2_adjoint(const float* g, float* out, long B, int R, hipStream_t stream);
/* second-order term of sg_act_bwd for tanh / sigmoid: out = ggx * dy * d(act'(y))/dy  (-2y resp. 1-2y) */
int sg_act_bwd_dy(const float* y, const float* dy, const float* ggx, float* out, long n, int act, hipStream_t stream);

/* ---- input pipeline -------------------------------------------------------------------------
 * reference: VoxelDataset.__getitem__ (datasets.py:16-23): result.clamp_(-clamp, clamp); result /= clamp when
 * rescale_sdf.  out = clamp(x, -clamp, clamp) / divisor on the device (divisor <= 0: no division); x == out allowed.
 * Bit-exact with the reference's CPU arithmetic (NaN-propagating clamp, IEEE fp32 division). */
int sg_voxel_prepare(const float* x, float* out, long n, float clamp, float divisor, hipStream_t stream);

/* ---- PointNet-discriminator GAN family --------------------------------------------------------
 * reference: model/point_sdf_net.py.  SDFGenerator (:49-119): x = lin(x) [+ z_lin(z) per shape]; LayerNorm; ReLU —
 *   y[r] = act(gamma * normalise(x[r] + rowbias[r / rows_per_shape]) + beta), act in {none, relu}; rows may be strided
 *   (ld*), so the skip concat `cat([x, pos])` (:100) is a 259-float row whose first 256 columns LayerNorm writes.
 *   The backward returns dz (gradient of the pre-norm row, also of the per-shape bias rows) and dgamma / dbeta.
 * PointNet (:11-47): `x.max(dim=-2)[0]` over the points of a shape: x [B,P,C] -> out [B,C] + argmax (first
 *   occurrence); scatter = its adjoint (backward), gather = the adjoint of the scatter (double backward under the
 *   gradient penalty, train_point_gan.py:61-70).
 * sg_colsum_tall: out[b][c] = sum_r x[b*batch_stride + r*ld + c]: column sums of `batch` tall [rows, cols] matrices in
 *   two deterministic passes (bias gradients of per-point Linear layers: rows = points; per-shape sums for the
 *   z-injection gradient: batch = shapes). */
int sg_layernorm_fwd(const float* x, long ldx, const float* rowbias, long rows_per_shape, const float* gamma,
                     const float* beta, float* y, long ldy, float* mean, float* rstd, long R, int C, float eps, int act,
                     hipStream_t stream);
size_t sg_layernorm_bwd_workspace_bytes(long R, int C);
int sg_layernorm_bwd(const float* x, long ldx, const float* rowbias, long rows_per_shape, const float* gamma, const float* y,
                     long ldy, const float* dy, long lddy, const float* mean, const float* rstd, float* dz, long lddz,
                     float* dgamma, float* dbeta, long R, int C, int act, void* workspace, size_t workspace_bytes,
                     hipStream_t stream);
size_t sg_colsum_tall_workspace_bytes(long batch, long rows, int cols);
int sg_colsum_tall(const float* x, float* out, long batch, long batch_stride, long rows, int cols, long ld, void* workspace,
                   size_t workspace_bytes, hipStream_t stream);
/* PointNet.nn1 (Linear 4 -> 64 -> 128 -> 256 -> 512, ReLU between; model/point_sdf_net.py:14-23) over whole clouds followed by the
 * max over each cloud's points (:40) as ONE fused launch that never writes the per-point layers (ABI 8): out [B][512] = the maxima,
 * idx [B][512] = the point of the cloud that holds each (int32; lowest point on a tie; NaN is ignored by the maximum).  x [B][P][4],
 * P a multiple of 32; `packed`: sg_pointnet_packed_floats() floats from sg_pointnet_pack(nn1.{0,2,4,6}.weight); biases:
 * nn1.{0,2,4,6}.bias.  The plain pass of the sparse-adjoint critic: the recorded evaluation runs on the selected points only. */
size_t sg_pointnet_packed_floats(void);
int sg_pointnet_pack(const float* const* weights, float* packed, hipStream_t stream);
size_t sg_pointnet_select_workspace_bytes(long B, long P);
int sg_pointnet_select(const float* x, const float* packed, const float* const* biases, long B, long P, float* out, int* idx,
                       void* workspace, size_t workspace_bytes, hipStream_t stream);
size_t sg_segmax_workspace_bytes(long B, long P, int C);   /* scratch of sg_segmax_fwd (0 when it needs none) */
int sg_segmax_fwd(const float* x, float* out, int* idx, long B, long P, int C, void* workspace, size_t workspace_bytes,
                  hipStream_t stream);
int sg_segmax_scatter(const float* dy, const int* idx, float* dx, long B, long P, int C, hipStream_t stream);
int sg_segmax_gather(const float* x, const int* idx, float* out, long B, long P, int C, hipStream_t stream);
/* The diagonal last layer of the critic's selected-points pass (ABI 8): row r = b C + c of the gathered batch h [B*C][K] is the point
 * that holds the maximum of channel c, so nn1's last Linear (model/point_sdf_net.py:22) reduces to out[r] = bias[c] + h[r] . w[c]
 * (sg_rowdot); its adjoints out[r][k] = g[r] w[c][k] (sg_rowscale) and out[c][k] = sum_b g[b C + c] h[b C + c][k] (sg_rowouter)
 * make the three closed under differentiation (the gradient penalty of train_point_gan.py:61-70 differentiates twice). */
/* Deterministic adjoint of gathering C rows per group out of x [N][K] (the selected points of every cloud, rows of a group may repeat:
 * several channels can select the same point): dx[rows[b C + c]][k] += g[b C + c][k] without atomics — the first channel that names
 * a row receives the sum of its duplicates through a fixed tree of additions.  dx zeroed by the caller; rows of different groups are
 * distinct; C <= 1024, C K <= 8192. */
int sg_scatter_rows_grouped(const float* g, const int64_t* rows, float* dx, long B, int C, int K, hipStream_t stream);
int sg_rowdot(const float* h, const float* w, const float* bias, float* out, long B, int C, int K, hipStream_t stream);
int sg_rowscale(const float* g, const float* w, float* out, long B, int C, int K, hipStream_t stream);
int sg_rowouter(const float* g, const float* h, float* out, long B, int C, int K, hipStream_t stream);
/* torch_scatter.scatter_max over a ragged `batch` vector (model/point_sdf_net.py:42-43, train_point_gan_ref.py:109-110):
 * out[b][c] = max over rows i with batch[i] == b of x[i][c] (0 for a segment without members, as torch_scatter), arg = the
 * first row attaining it (-1 when empty); scatter = backward (zero-filled), gather = backward of the backward. */
size_t sg_scatter_max_workspace_bytes(long B, int C);
int sg_scatter_max_fwd(const float* x, const int64_t* batch, float* out, int* arg, long N, long B, int C, void* workspace,
                       size_t workspace_bytes, hipStream_t stream);
int sg_scatter_max_scatter(const float* dy, const int* arg, float* dx, long N, long B, int C, hipStream_t stream);
int sg_scatter_max_gather(const float* x, const int* arg, float* out, long N, long B, int C, hipStream_t stream);

/* ---- K12: batched marching cubes and surface sampling ---------------------------------------------------------------------
 * reference: SDFNet.get_mesh / get_uniform_surface_points, model/sdf_net.py:97-116 (skimage.measure.marching_cubes_lewiner, then
 *            trimesh.Trimesh(...).sample), and metrics.py:31-46 (sample_point_clouds / sample_from_voxels: the same per shape, in a
 *            Python loop) -> S grids meshed and sampled on the device in a handful of launches.
 * grids [S][R0][R1][R2] fp32.  pad = 1 surrounds every grid with a virtual shell of one cell of value pad_value (the reference's
 * np.pad(voxels, 1, constant_values=1)); the grid seen by the meshing then has P_k = R_k + 2 pad corners along axis k and the
 * padded index 0 is the shell.  A corner is inside when v < level; one vertex per grid edge that crosses the level, shared by
 * the triangles of every cell around that edge (welded), at t = (level - a) / (b - a) from the corner of lower index:
 *   position[k] = (index[k] + t [k == edge axis]) * spacing[k] + origin[k]          (index in the padded grid),
 *   normal = the central-difference gradient of the padded grid (one-sided at its outermost layer, divided by spacing), interpolated
 *            with t and normalised: it points toward increasing values, outward for an SDF; (v1 - v0) x (v2 - v0) of every
 *            triangle does too.  Ambiguous cube faces always separate their two inside corners (csrc/mc_tables.h), so every closed
 *            surface comes out watertight.
 * Order (deterministic, no atomics): vertices by owning corner (row-major over the padded corners), then by the axis (0, 1, 2) of
 * the edge it owns toward +1; triangles by cell (row-major), then in table order.  vert_offsets / tri_offsets [S+1] (int64): shape
 * s owns vertices [vert_offsets[s], vert_offsets[s+1]) and triangles [tri_offsets[s], tri_offsets[s+1]); faces [F][3] (int64)
 * are local to their shape.  Int32 indices inside: S * P0 * P1 * P2 * 24 must not exceed 2^31 - 1 (SG_ERR_ARG; split the batch).
 * sg_mc_count writes the offsets (and keeps per-workgroup offsets in `workspace`); the caller reads the totals vert_offsets[S],
 * tri_offsets[S] to size the outputs and then calls sg_mc_emit with the same grids, arguments and workspace.  max_verts /
 * max_tris: the capacity of vertices / normals [max_verts][3] and faces [max_tris][3]; nothing is written beyond them. */
size_t sg_mc_workspace_bytes(long S, int R0, int R1, int R2, int pad);
int sg_mc_count(const float* grids, long S, int R0, int R1, int R2, float level, int pad, float pad_value, int64_t* vert_offsets,
                int64_t* tri_offsets, void* workspace, size_t workspace_bytes, hipStream_t stream);
int sg_mc_emit(const float* grids, long S, int R0, int R1, int R2, float level, int pad, float pad_value, float spacing0,
               float spacing1, float spacing2, float origin0, float origin1, float origin2, const int64_t* vert_offsets,
               const int64_t* tri_offsets, float* vertices, float* normals, int64_t* faces, long max_verts, long max_tris,
               void* workspace, size_t workspace_bytes, hipStream_t stream);
/* Area-weighted surface sampling of the packed meshes above (trimesh.sample): P points per shape from caller-supplied uniforms
 * [S][P][3] (u0, u1, u2).  Per shape: the cumulative triangle areas in double; triangle = the first whose cumulative area reaches
 * u0 * total (numpy.searchsorted), point = v0 + (u1 (v1 - v0) + u2 (v2 - v0)) with (u1, u2) -> (1 - u1, 1 - u2) when u1 + u2 > 1.
 * out [S][P][3]; a shape without triangles gets zeros and empty[s] = 1 (0 otherwise).  F = tri_offsets[S]. */
size_t sg_mesh_sample_workspace_bytes(long S, long F);
int sg_mesh_sample(const float* vertices, const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S,
                   long F, const float* uniforms, long P, float* out, int* empty, void* workspace, size_t workspace_bytes,
                   hipStream_t stream);

/* ---- K12b: mesh topology: connected components, their statistics, the compaction that keeps some ---------------------------------
 * reference: what its callers took from trimesh one mesh at a time on the host (Trimesh.split, body_count, is_watertight, volume,
 *            euler_number) -> a packed batch of meshes labelled, measured and cleaned on the device.
 * Input: K12's packed meshes.  vertices / normals [V][3] fp32, faces [F][3] int64 local to their shape, vert_offsets / tri_offsets
 * [S+1] int64, non-decreasing from 0 to V / F; S >= 1; shapes without triangles are legal anywhere, V = 0 and F = 0 too.  V and F
 * up to 2^31 - 1, beyond that SG_ERR_ARG before any launch, as for S < 1, a negative size, C outside [0, V] or a NULL array that
 * has elements.  A triangle that names an index outside [0, n_s) of its shape (vert_offsets[s] + n_s <= V) is SKIPPED by every
 * entry point: it connects nothing, counts nowhere and is dropped by the compaction.
 *
 * sg_topo_label.  Two vertices of a shape are connected when a (not skipped) triangle names both; a triangle with a repeated index
 * still connects its distinct vertices.  vertex_component [V] int32: the number of the vertex's component within its shape, the
 * components of a shape numbered 0, 1, .. in increasing order of their lowest vertex index; -1 for a vertex no such triangle names.
 * comp_offsets [S+1] int64: the exclusive sum of the components per shape; component c of shape s is number comp_offsets[s] + c of
 * the batch, the caller reads the total C = comp_offsets[S] once (as it reads K12's totals).  Method: a union-find over the
 * triangles (int32 parents, the root of larger index hooked under the smaller by compare-and-swap, paths halved by atomic minimum),
 * a flatten pass, an exclusive scan of the root flags built as sg_mc_count builds its offsets.  The result is the partition: the
 * root of a component is its lowest vertex whatever the schedule.  Visibility across the chip's L2s: inside the hooking kernel
 * every read of a parent is a relaxed agent-scope atomic load or the value an atomic returned, and a root changes only by a
 * compare-and-swap against the word itself; initialisation, hooking and flattening are separate kernels.  workspace: int32 words
 * (parents, flags, roots, positions, per-workgroup totals), nothing kept between calls.
 *
 * sg_topo_keys: tri_keys [F] int32 = the batch-wide component number of each triangle (2^31 - 1 for a skipped one), edge_keys
 * [F][3] int64 = per side a -> b of a triangle (v0 -> v1, v1 -> v2, v2 -> v0, GLOBAL vertex indices):
 *   (min(a, b) << 32) | (max(a, b) << 1) | (1 when a > b),      2^63 - 1 for a == b and for the sides of a skipped triangle.
 * The caller sorts both (any sort: equal keys are interchangeable; triangles stably, so that a component's triangles keep their
 * order) and hands sg_topo_stats: tri_order [F] int64 = the triangle indices in sorted key order, seg_offsets [C+1] int64 =
 * component c owns positions [seg_offsets[c], seg_offsets[c+1]) of tri_order, tile_offsets [C+1] int64 = the exclusive sum of
 * ceil(n_c / 256) over the components (n_c = its triangles), edge_sorted [F][3] int64 = the sorted edge keys.
 *
 * sg_topo_stats, per component (arrays of length C, component c of shape s at comp_offsets[s] + c):
 *   n_vertices, n_triangles int32;  n_edges int32 = its distinct undirected edges {a, b}, a != b;  n_open int32 = those that are
 *   not closed, an edge being closed iff exactly one side runs a -> b and exactly one b -> a (so boundaries, non-manifold fans and
 *   flipped neighbours all count as open);  area, volume float64: the sums over its triangles of
 *     area_t = |(p1 - p0) x (p2 - p0)| / 2,      volume_t = p0 . (p1 x p2) / 6
 *   in double from the fp32 corners (csrc/topology_core.h states both with explicit fma, contraction off).  With K12's orientation
 *   a solid has positive volume, an internal cavity negative.  The sums have ONE order, shared by the GPU and the twin, so both are
 *   bit-identical between them and from run to run: the component's triangles t[0..n) in increasing triangle index, in tiles of 256;
 *     per tile k and group g = 0..3:  s[l] = term of t[256 k + 64 g + l] (0.0 beyond n), l = 0..63;
 *                                     for off = 32, 16, .., 1:  s[l] += s[l + off] for l < off;   G[g] = s[0];
 *     T[k] = ((G[0] + G[1]) + G[2]) + G[3];      sum = ((0.0 + T[0]) + T[1]) + ...      (tiles added in increasing k).
 *   Counts use integer atomics only.  workspace: the per-tile sums (float64).
 *
 * sg_topo_keep_count / sg_topo_keep_emit, a pair like sg_mc_count / sg_mc_emit.  keep [C] uint8 (non-zero: keep).  count writes
 * new_vert_offsets / new_tri_offsets [S+1] (every element) and keeps positions in `workspace` (int32 words); the caller reads the
 * two totals once, sizes the outputs and calls emit with the same mesh and workspace.  emit writes the vertices and normals of the
 * kept components (their bits copied unchanged) and their triangles, both in their original relative order, faces renumbered
 * locally; vertices of component -1 and skipped triangles are dropped.  max_verts / max_tris: the capacities of out_vertices /
 * out_normals [max_verts][3] and out_faces [max_tris][3]; nothing is written beyond them, every element below the totals is
 * written, nothing is read from an output. */
size_t sg_topo_label_workspace_bytes(long S, long V);
int sg_topo_label(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                  int* vertex_component, int64_t* comp_offsets, void* workspace, size_t workspace_bytes, hipStream_t stream);
int sg_topo_keys(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                 const int* vertex_component, const int64_t* comp_offsets, long C, int* tri_keys, int64_t* edge_keys,
                 hipStream_t stream);
size_t sg_topo_stats_workspace_bytes(long F, long C);
int sg_topo_stats(const float* vertices, const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V,
                  long F, const int* vertex_component, const int64_t* comp_offsets, long C, const int64_t* tri_order,
                  const int64_t* seg_offsets, const int64_t* tile_offsets, const int64_t* edge_sorted, int* n_vertices,
                  int* n_triangles, int* n_edges, int* n_open, double* area, double* volume, void* workspace, size_t workspace_bytes,
                  hipStream_t stream);
size_t sg_topo_keep_workspace_bytes(long S, long V, long F);
int sg_topo_keep_count(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                       const int* vertex_component, const int64_t* comp_offsets, long C, const uint8_t* keep,
                       int64_t* new_vert_offsets, int64_t* new_tri_offsets, void* workspace, size_t workspace_bytes,
                       hipStream_t stream);
int sg_topo_keep_emit(const float* vertices, const float* normals, const int64_t* faces, const int64_t* vert_offsets,
                      const int64_t* tri_offsets, long S, long V, long F, const int64_t* new_vert_offsets, float* out_vertices,
                      float* out_normals, int64_t* out_faces, long max_verts, long max_tris, void* workspace, size_t workspace_bytes,
                      hipStream_t stream);

/* ---- K12c: mesh simplification: quadric vertex clustering of packed meshes --------------------------------------------------------
 * reference: its STL export meshes at 256^3 (create_plot.py:914-933) and nothing after marching cubes makes such a mesh smaller; what
 *            trimesh users take from simplify_* -> one pass over a whole batch on the device (Lindstrom 2000, Garland-Heckbert quadrics).
 * Input: K12's packed meshes with K12b's rule for a triangle that COUNTS.  S in [1, 2^20), V and F up to 2^31 - 1, else SG_ERR_ARG
 * before any launch.  The contract (keys, clusters, quadrics, placement, surviving triangles) and the order of every sum are stated
 * in csrc/simplify_core.h and shared with the twin: every output is bit-identical between the two and from run to run.
 *
 * The grid of shape s lives on the device: origin [S][3] fp32, cell [S][2] fp32 = (h_s, inv_h_s), cells [S] int32 = n_s.  The caller
 * (shapegan_amd/simplify.py) refuses n > 16384 and an h that is not a positive finite number before any launch; a kernel that meets
 * other values clamps n into [1, 16384] and takes a negative or non-finite product to cell 0, so a key is a key whatever it reads.
 *
 * sg_simplify_bounds: lo, hi [S][3] fp32 = the bounding box of the finite coordinates of each shape ([0, 0] on an axis without one).
 * sg_simplify_keys: keys [V] int64 = s << 42 | ix << 28 | iy << 14 | iz.
 * sg_simplify_count: counts [S] int32 = the counting triangles of each shape whose three keys differ (integer atomics): what a grid
 *   would leave, without a sort.
 * The caller sorts the keys STABLY (sorted_keys, order [V] int64: the vertex at each sorted position).
 * sg_simplify_clusters: sorted_cluster [V] int32 = the cluster number (batch-wide, in key order) at each sorted position,
 *   vertex_cluster [V] int32 = the same per vertex, cluster_offsets [S+1] int64 = the clusters before each shape; the caller reads
 *   C = cluster_offsets[S] once.  workspace: int32 words.
 * sg_simplify_corners: corner_keys [F][3] int64 = per counting triangle one record cluster << 31 | triangle for each DISTINCT
 *   cluster among its corners, 2^63 - 1 in every other slot (and for a triangle that does not count); the caller sorts them.
 * sg_simplify_place: cluster_vertices, cluster_normals [C][3] fp32.  One wave per cluster walks its run of sorted vertices and its
 *   run of sorted corner records (both found by bisection) in tiles of 64; placement 0 = quadric, 1 = mean.
 * sg_simplify_faces_count / sg_simplify_faces_emit, a pair like sg_topo_keep_count / _emit: count marks the clusters that a
 *   surviving triangle names, writes new_vert_offsets / new_tri_offsets [S+1] (every element) and keeps positions in `workspace`
 *   (int32 words); the caller reads the two totals once, sizes the outputs and calls emit with the same mesh and workspace.  emit
 *   writes the named clusters' vertices and normals in cluster order and the surviving triangles in input order with their winding,
 *   faces local to their shape; nothing is written beyond max_verts / max_tris, every element below the totals is written, nothing
 *   is read from an output.  Coincident duplicate triangles are kept. */
int sg_simplify_bounds(const float* vertices, const int64_t* vert_offsets, long S, long V, float* lo, float* hi, hipStream_t stream);
int sg_simplify_keys(const float* vertices, const int64_t* vert_offsets, long S, long V, const float* origin, const float* cell,
                     const int* cells, int64_t* keys, hipStream_t stream);
int sg_simplify_count(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                      const int64_t* keys, int* counts, hipStream_t stream);
size_t sg_simplify_clusters_workspace_bytes(long S, long V);
int sg_simplify_clusters(const int64_t* sorted_keys, const int64_t* order, const int64_t* vert_offsets, long S, long V,
                         int* sorted_cluster, int* vertex_cluster, int64_t* cluster_offsets, void* workspace, size_t workspace_bytes,
                         hipStream_t stream);
int sg_simplify_corners(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                        const int* vertex_cluster, int64_t* corner_keys, hipStream_t stream);
int sg_simplify_place(const float* vertices, const float* normals, const int64_t* faces, const int64_t* vert_offsets,
                      const int64_t* tri_offsets, long S, long V, long F, const int64_t* sorted_keys, const int64_t* order,
                      const int* sorted_cluster, const int64_t* corner_sorted, long C, const float* origin, const float* cell,
                      int placement, float* cluster_vertices, float* cluster_normals, hipStream_t stream);
size_t sg_simplify_faces_workspace_bytes(long S, long C, long F);
int sg_simplify_faces_count(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                            const int* vertex_cluster, const int64_t* cluster_offsets, long C, int64_t* new_vert_offsets,
                            int64_t* new_tri_offsets, void* workspace, size_t workspace_bytes, hipStream_t stream);
int sg_simplify_faces_emit(const float* cluster_vertices, const float* cluster_normals, const int64_t* faces,
                           const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F, const int* vertex_cluster,
                           long C, const int64_t* new_vert_offsets, float* out_vertices, float* out_normals, int64_t* out_faces,
                           long max_verts, long max_tris, void* workspace, size_t workspace_bytes, hipStream_t stream);

/* ---- K13: point-cloud evaluation: Chamfer matrices, nearest neighbours, occupancy histograms -----------------------------------
 * Clouds are [S][P][3] fp32, contiguous.  Every pair (a, b) of points has ONE value, in f32:
 *   dx = ax - bx, dy = ay - by, dz = az - bz;   d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx))
 * (three roundings of the differences, one of the product, two fused steps; written with explicit fmaf, contraction off).  It is
 * bitwise the same with a and b exchanged, and a minimum of such values does not depend on the order it is taken in: dist_*,
 * idx_* and every minimum inside sg_chamfer_matrix are the same bit for bit on the GPU, in the twin and under any tiling.  A
 * tie takes the LOWEST index.  Non-finite coordinates give unspecified values in the rows and columns they touch, but no fault
 * and no index outside [0, Q) / [0, P).
 *
 * sg_chamfer_matrix: A [Sa][P][3], B [Sb][Q][3] -> ab, ba [Sa][Sb] float64 (either may be NULL):
 *   ab[i][j] = mean over the points a of A_i of  min over the points b of B_j of d2(a, b),   ba[i][j] = the same from B_j to A_i.
 * The Chamfer distance is ab + ba (squared distances, the convention of Achlioptas et al.'s evaluation code).  Means are float64
 * sums of the f32 minima m[0..n) in ONE order, shared by the GPU and the twin, so ab and ba are bit-identical between them:
 *   per tile t of 2048 points:  s[l] = ((0 + m[t*2048 + l]) + m[t*2048 + 256 + l]) + ... (k = 0..7, indices >= n skipped),
 *                               l = 0..255;  then for off = 128, 64, .., 1:  s[l] += s[l + off] for l < off;  T[t] = s[0];
 *   mean = (T[0] + T[1] + ...) / n      (tiles added in increasing t, one float64 division).
 * Any Sa, Sb, P, Q >= 1 (Sa, Sb <= 65535 per call: split the batch; P, Q <= 2^26; beyond either SG_ERR_ARG, on the GPU and in
 * the twin alike).  workspace: the per-tile sums.
 *
 * sg_chamfer_nearest: matched batches A [S][P][3], B [S][Q][3] -> dist_a [S][P] fp32 / idx_a [S][P] int32: for every point of
 * A_s the smallest d2 to a point of B_s and the lowest index that attains it; dist_b / idx_b [S][Q] the same from B_s to A_s.
 * Either pair may be NULL (both of a pair or neither).
 *
 * sg_occupancy_histogram: hist [R][R][R] int64 += the number of points of clouds [S][P][3] per cell of the grid with centres
 * c_i = -0.5 + i / (R - 1) per axis (the caller zeroes hist; 2 <= R <= 1024).  The index along an axis is, in f32 without contraction,
 *   t = (x + 0.5f) * (float)(R - 1);   i = (int) min(max(floorf(t + 0.5f), 0.f), (float)(R - 1))      (max(NaN, 0) = 0)
 * i.e. the nearest centre, clamped; cell = (i_x * R + i_y) * R + i_z.  Integer atomics only: the counts do not depend on order.
 * reference: metrics.py:18-46 (sample_point_clouds / sample_from_voxels write the clouds, rescaled to the half unit sphere, that
 *            these entry points consume; the reference leaves the scoring to an outside tool). */
size_t sg_chamfer_matrix_workspace_bytes(long Sa, long Sb, long P, long Q);
int sg_chamfer_matrix(const float* A, const float* B, long Sa, long Sb, long P, long Q, double* ab, double* ba, void* workspace,
                      size_t workspace_bytes, hipStream_t stream);
int sg_chamfer_nearest(const float* A, const float* B, long S, long P, long Q, float* dist_a, int* idx_a, float* dist_b, int* idx_b,
                       hipStream_t stream);
int sg_occupancy_histogram(const float* clouds, long S, long P, int R, int64_t* hist, hipStream_t stream);

/* ---- K14: tiled triangle rasteriser: the headless MeshRenderer -----------------------------------------------------------------
 * reference: rendering/__init__.py (MeshRenderer: _render_shadow_texture, _render, _draw_floor) with vertex.glsl / fragment.glsl ->
 *            S shapes drawn in a handful of launches, no window and no GL context.
 * Input: S triangle soups packed as the reference's _update_buffers takes them: positions [T][3][3] fp32, normals [T][3][3] fp32 or
 * NULL (flat shading), tri_offsets [S+1] int64 (shape s owns triangles [tri_offsets[s], tri_offsets[s+1])).  Any S >= 1
 * (<= 65535), any T >= 0, any shape may be empty; width, height <= 16384.  A view is a 4x4 row-major `vp` of 16 host doubles,
 * rounded ONCE to fp32.  All arithmetic below is fp32 with the fused steps written out (contraction off) or integer, and exists
 * once (csrc/raster_core.h): the GPU and the twin agree bit for bit on every output, bins compared as sets.
 *
 * sg_raster_setup, per triangle and view:
 *   clip[k][i] = fmaf(M[i][2], z, fmaf(M[i][1], y, fmaf(M[i][0], x, M[i][3])))           corner k = (x, y, z), i = 0..3, w = clip[k][3]
 *   window, snapped to 8 sub-pixel bits (int32; y runs DOWN, row 0 is NDC y = +1; sample (px, py) has its centre at px*256+128):
 *     X = rint(fmaf(clip_x / w, 128 width, 128 width)),   Y = rint(fmaf(clip_y / w, -128 height, 128 height))
 *   z = clip_z / w (NDC depth), iw = 1 / w.   recs [T][16] int32 words: X0 X1 X2 Y0 Y1 Y2 | z0 z1 z2 | iw0 iw1 iw2 (float bits) |
 *   px0 py0 px1 py1 = the samples whose centres lie in the snapped bounding box, clamped to the image.
 *   flags [T] int32, the FIRST that applies: 1 a corner has w <= near_w (no clipping: the triangle is dropped; near_w = the near
 *   distance of rendering/math.py's PROJECTION_MATRIX, 0.1); 2 a snapped coordinate would leave +-2^22 (keeps the 64-bit edge
 *   products exact); 4 zero area; 8 back face, only when cull_back: front = counter-clockwise on the screen (GL's default) =
 *   (v1 - v0) x (v2 - v0) faces the camera, K12's orientation; the shadow pass culls nothing; 16 kept, but no sample centre in its
 *   box.  Flags 1..8 are DROPPED: their record is zeros with an empty box, dropped[s] (int32 [S]) counts them per shape.
 *   clip (may be NULL): [T][3][4].  ground (may be NULL): [S] fp32 = min over the shape's corners of y, found with integer atomicMin
 *   on the order-preserving image of the float, no host read; -1 for an empty shape.  tile_counts [S][nty][ntx] int32 = the number
 *   of kept triangles whose box touches each tile of 16 x 16 samples (ntx = ceil(width / 16), nty likewise; integer atomics).
 * sg_raster_scan: tile_offsets [n+1] int64 = exclusive sum of the n = S nty ntx counts; cursor [n] int32 = 0; active [n] int32 = the
 *   non-empty tiles in increasing order (first totals[1] entries); totals [2] int64 = {tile_offsets[n], number of non-empty tiles}.
 *   The caller reads totals (the one device -> host read of a view) to size `lists` and the visibility launch.
 * sg_raster_fill: lists [capacity] int32: the triangles of tile g are lists[tile_offsets[g] .. tile_offsets[g+1]), as a SET: the
 *   order inside a list is not specified (the GPU takes slots from an atomic cursor, the twin fills in triangle order) and no
 *   result depends on it.  Nothing is written outside [0, capacity).
 * sg_raster_visibility: id [S][H][W] int32 (-1 = nothing; NULL in the shadow pass), depth [S][H][W] fp32 (1.0 = cleared).  Sample
 *   (px, py) is covered by a triangle when the three int64 edge functions at its centre, signed so that the inside is positive,
 *   are > 0, or = 0 on a top or left edge (edge vector (dx, dy) along the inside-positive orientation: dy < 0, or dy = 0 and
 *   dx > 0) — a sample on an edge shared by two triangles on opposite sides belongs to exactly one.  Depth of a covered sample:
 *     inv = 1 / (float)|2 area|,  l1 = (float)e1 * inv,  l2 = (float)e2 * inv,  z = fmaf(l2, z2 - z0, fmaf(l1, z1 - z0, z0))
 *   (screen-space barycentrics, as GL interpolates gl_FragCoord.z; e_i = the edge function opposite corner i).  Winner = smallest z,
 *   a tie goes to the lowest triangle index; depth is not clipped to the far plane.  shadow != 0: depth = fmaf(0.5, z, 0.5).
 *   An entry of `active` or `lists` that names no tile / no triangle of the tile's shape is skipped.
 * sg_raster_shade: image [S][H][W][3] uint8 = floor(fmaf(clamp(c, 0, 1), 255, 0.5)).  params: 60 host doubles, rounded once to fp32:
 *   VP [16], lightVP [16], VP^-1 [16], camera position [3], lightPosition = xyz of VP lightVP^-1 (0, 0, -1, 1) [3], albedo [3],
 *   background [3].  shadow_map [S][N][N] = the depth of the light pass (N = shadow_size).  For a sample with id >= 0:
 *     perspective-correct barycentrics b_i = q_i / ((q0 + q1) + q2), q_i = ((float)e_i * inv) * iw_i;  world p = fmaf(b2, v2, fmaf(b1,
 *     v1, b0 v0)); n = the corner normals interpolated the same way, or (v1 - v0) x (v2 - v0) (each component fmaf(a, b, -(c d)));
 *     position = (VP (p, 1)).xyz, shadowPosition = lightVP (p, 1) (rows as clip above), normal = normalize((VP (n, 0)).xyz),
 *     L = normalize(lightPosition - position), V = normalize(-position), R = -normalize(L - 2 (n.L) n), d = clamp(n.L, 0, 1);
 *     colour = ((a/2 + (a/2 d) lit) + (0.3 s^20) lit) + 0.3 m^4 per channel, a = albedo, lit = 1 - shadow, s = max(0, R.V) with
 *     s^20 = ((((s^2)^2)^2)^2) (s^2)^2, m = 1 - clamp(-n_z, 0, 1) with m^4 = (m^2)^2; dot(a, b) = fmaf(a2, b2, fmaf(a1, b1, a0 b0)).
 *   shadow(shadowPosition sp, d): c = fmaf(sp.xyz / sp.w, 0.5, 0.5); 0 unless c.z <= 1; ref = c.z - max(0.002 (1 - d), 0.001) / sp.w;
 *     the mean over the offsets (ox, oy) in {-1, 0, 1}^2 (ox outer) of the bilinear blend, t = fmaf(fmaf(o, 1/N, c), N, 0.5) per axis,
 *     weights t - floor(t), of the four comparisons ref > map at texels floor(t) + {0, 1} (clamped to the edge; texel row v counts
 *     from NDC y = -1), mix(a, b, f) = fmaf(b - a, f, a); clamped to [0, 1].
 *   The floor is analytic and is tested first: the eye ray from the camera position through VP^-1 (nx, ny, 1, 1) (nx, ny = the NDC
 *   of the sample centre) meets y = ground[s] at t > 0; it is a floor sample when the camera is above the plane, |x|, |z| <= 6, its
 *   clip w > 0, its NDC depth is in [-1, 1] and smaller than depth at the sample (1.0 where nothing was drawn); colour =
 *   fmaf(shadow, -0.6, 1) with d from the normal normalize(VP (0, 1, 0, 0)).  A sample that is neither is the background colour.
 * sg_raster_resolve: image [S][H][W][3] = the rounded mean of ssaa x ssaa blocks of samples [S][H ssaa][W ssaa][3], in integers
 *   ((2 sum + n) / (2 n), n = ssaa^2). */
int sg_raster_setup(const float* positions, const int64_t* tri_offsets, long S, long T, const double* vp, int width, int height,
                    int cull_back, double near_w, int* recs, int* flags, float* clip, int* dropped, float* ground, int* tile_counts,
                    hipStream_t stream);
int sg_raster_scan(const int* tile_counts, long ntiles, int64_t* tile_offsets, int* cursor, int* active, int64_t* totals,
                   hipStream_t stream);
int sg_raster_fill(const int* recs, const int* flags, const int64_t* tri_offsets, long S, long T, int width, int height,
                   const int64_t* tile_offsets, int* cursor, int* lists, long capacity, hipStream_t stream);
int sg_raster_visibility(const int* recs, const int64_t* tri_offsets, long S, int width, int height, const int64_t* tile_offsets,
                         const int* lists, long capacity, const int* active, long nactive, int* id, float* depth, int shadow,
                         hipStream_t stream);
int sg_raster_shade(const float* positions, const float* normals, long T, const int* recs, const int* id, const float* depth,
                    const float* shadow_map, int shadow_size, const float* ground, const double* params, long S, int width, int height,
                    unsigned char* image, hipStream_t stream);
int sg_raster_resolve(const unsigned char* samples, long S, int width, int height, int ssaa, unsigned char* image, hipStream_t stream);

/* ---- K15: earth mover's distance between point clouds: forward auction with eps-scaling ------------------------------------------
 * The second family of scores of Achlioptas et al.'s evaluation code (MMD-EMD, COV-EMD; K13 is the Chamfer family).  Two clouds a, b
 * [P][3] fp32 of the SAME point count P, 1 <= P <= SG_EMD_MAX_POINTS.  d(i, j) = sqrtf(d2(a_i, b_j)) in f32, d2 exactly K13's value
 * (sqrtf and the f32 division below are the correctly rounded IEEE operations).  Distances are Euclidean, NOT squared:
 *   emd*(a, b) = min over the permutations pi of (1/P) sum_i d(i, pi(i))        (that code's match_cost / P)
 * The library returns a permutation `match` and emd = (1/P) sum_i d(i, match[i]), the float64 sum of the f32 d in K13's order
 * (s[l] = d[l] + d[256 + l] + ..., halving tree over l = 0..255, one division by P).
 * GUARANTEE (status 0): match is a permutation of [0, P) and emd <= emd* + eps; eps > 0 is the caller's absolute bound, in
 * coordinate units per point.
 *
 * Arithmetic: all of the auction is int32, so the GPU and the twin execute the same rounds and agree BIT FOR BIT on match, emd,
 * rounds and status.  u = the largest f32 that is not above eps / 4; the cost of a pair is  q = d / u (f32);  k = q < 2^22 ? (int) floorf(q) : 2^22
 * (SG_EMD_MAX_COST; NaN and inf land there: the comparison is false).  kmax = the largest k of the pair of clouds.
 * Phases: e = max(1, kmax >> 4); a phase runs with e; after it e = max(1, e >> 2); the phase with e = 1 is the last.  Prices p[j]
 * (int32, 0 at the start) are KEPT between phases, the assignment is RESET (everybody unassigned, nothing owned).
 * Round (Jacobi: every bid of a round is computed from the prices at its start): each unassigned i finds over the objects j
 *   v(j) = -k(i, j) - p[j];   w1 = max v,  j1 = the LOWEST j with v(j) = w1,  w2 = max over j != j1 of v(j)  (w2 = w1 when P = 1)
 * and bids  p[j1] + (w1 - w2) + e  for j1.  An object that received bids takes the HIGHEST, from the LOWEST bidder index on a tie:
 * its price becomes the bid, the bidder its owner, the previous owner unassigned.  A phase ends when nobody is unassigned.  These
 * maxima do not depend on the order they are taken in.
 * Bound: the last phase ends with sum k(match) <= sum k(pi*) + P (Bertsekas: within P e of the optimum of the integer problem).
 * k u <= d < (k + 1) u up to ONE unit of k for the rounding of d / u (q < 2^22, so |fl(q) - q| < 1/2), hence per point
 * d(match) < (k(match) + 2) u and k(pi*) u <= d(pi*) + u:  emd < emd* + (1 + 2 + 1) u = emd* + eps.
 * Prices stay below 2^28: a phase raises the largest by at most 2 (2^22 + e) and there are at most 11 phases.
 * Every loop is bounded: a phase that has not ended after SG_EMD_ROUND_CAP rounds stops the pair.
 * status (int32 per pair): 0 ok; SG_EMD_STATUS_ROUND_CAP: emd = NaN, match in range but no permutation; SG_EMD_STATUS_EPS: a FINITE
 * d of the pair has d / u >= 2^22 — eps is smaller than the arithmetic supports for these clouds (the smallest accepted is
 * 2^-20 x their largest distance: 1.7e-6 inside the unit cube); no auction is run, emd = NaN, match[i] = i.  Non-finite coordinates
 * are no error: status 0 and a valid permutation, the value unspecified, no fault and no index outside [0, P).
 *
 * sg_emd_match: matched batches A, B [S][P][3] -> emd [S] float64, status [S], match [S][P] int32 (match[s][i] = the point of B_s
 *   that point i of A_s is sent to; may be NULL), rounds [S] int32 (all phases; may be NULL).  S <= 65535 per call.
 * sg_emd_matrix: A [Sa][P][3], B [Sb][P][3] -> emd, status [Sa][Sb]: entry [i][j] has A_i as bidders and B_j as objects and is
 *   BITWISE sg_emd_match's value of that pair.  symmetric != 0: the caller passes the same set twice (Sa = Sb); only i < j is
 *   computed, [j][i] is its copy and the diagonal exact 0 with status 0.  workspace: rounds [Sa][Sb] int32, written like status
 *   (a count for the caller to read, never an index).  Sa, Sb <= 65535 per call.
 * Errors (SG_ERR_ARG): P < 1, P > SG_EMD_MAX_POINTS: larger clouds are refused, not mishandled;, eps <= 0 or not finite.
 * One workgroup per pair, all auction state in LDS; sg_emd_match_impl (testing / tuning) sets the number of bidders of a round
 * at or below which a whole wave scans the objects for one bidder (wave_scan_at <= 256; above it: one lane per bidder) and the
 * number at or below which the whole workgroup does (block_scan_at <= 16); < 0 = the default.  The results do not depend on them.
 * reference: metrics.py:18-46 (as K13: the clouds are written for that evaluation code). */
#define SG_EMD_MAX_POINTS 2048
#define SG_EMD_MAX_COST 4194304   /* 2^22 */
#define SG_EMD_ROUND_CAP 1048576   /* 2^20 */
#define SG_EMD_STATUS_ROUND_CAP 1
#define SG_EMD_STATUS_EPS 2
int sg_emd_match(const float* A, const float* B, long S, long P, double eps, int* match, double* emd, int* rounds, int* status,
                 hipStream_t stream);
int sg_emd_match_impl(const float* A, const float* B, long S, long P, double eps, int* match, double* emd, int* rounds, int* status,
                      int wave_scan_at, int block_scan_at, hipStream_t stream);
size_t sg_emd_matrix_workspace_bytes(long Sa, long Sb, long P);
int sg_emd_matrix(const float* A, const float* B, long Sa, long Sb, long P, double eps, int symmetric, double* emd, int* status,
                  void* workspace, size_t workspace_bytes, hipStream_t stream);

/* ---- K16: meshes to signed distances: exact point-triangle distances, the sign from orthographic depth scans --------------------------
 * reference: prepare_shapenet_dataset.py:69-131 and prepare_data.py, which sit on mesh_to_sdf's "depth" method (USE_DEPTH_BUFFER =
 *            True): a point is OUTSIDE when at least one of K virtual scans sees it — what makes ShapeNet's open, inconsistently
 *            oriented meshes usable.  Two deliberate differences: the magnitude is the exact distance to the triangles (mesh_to_sdf:
 *            the distance to a scanned point cloud through a kd-tree), and the scans are orthographic, so depth is linear in distance
 *            and one bias holds everywhere (mesh_to_sdf: perspective at fov 1 rad).
 * Input: S triangle soups packed as K14 takes them (positions [T][3][3] fp32, tri_offsets [S+1] int64; any shape may be empty) and
 * Q query points per shape, points [S][Q][3] fp32.  1 <= S <= 65535, 0 <= T <= SG_MESHSDF_MAX_TRIANGLES, 1 <= Q <=
 * SG_MESHSDF_MAX_POINTS, S Q <= SG_MESHSDF_MAX_TOTAL_POINTS; beyond: SG_ERR_ARG, in the library and the twin alike.  All arithmetic is
 * fp32 with the fused steps written out (contraction off) and exists once (csrc/meshsdf_core.h); a minimum of f32 values does not
 * depend on the order it is taken in: dist2, tri, closest, outside and sdf are the same BIT FOR BIT on the GPU, in the twin and
 * under any tiling.
 *
 * sg_meshsdf_distance: dist2 [S][Q] fp32 = the minimum over the triangles of shape s of the squared distance from the point to the
 *   closest point of the triangle; tri [S][Q] int32 (may be NULL) = the LOWEST triangle index, local to the shape, that attains it;
 *   closest [S][Q][3] fp32 (may be NULL) = that triangle's closest point.  A shape without triangles: dist2 = +inf, tri = -1,
 *   closest = 0.  Per triangle (a, b, c), made once per call: ab = b - a, bc = c - b, ca = a - c; i_e = 1 / |e|^2 per edge, 0 when
 *   |e|^2 < 1e-30 (no division has a divisor that can be 0); n = ab x ac; gv = (ac x n) i_n, gw = (n x ab) i_n, i_n = 1 / |n|^2 or 0
 *   alike.  dot(a, b) = fmaf(a2, b2, fmaf(a1, b1, a0 b0)); cross components fmaf(a, b, -(c d)).  Per pair, four candidates, each the
 *   squared length |r|^2 = dot(r, r) of the residual of a point of the triangle:
 *     edge from corner o along e, q = p - o:  t = dot(q, e) i_e, clamped to [0, 1] by comparisons (NaN -> 0);  r = fmaf(-t, e, q)
 *       (ab from a, bc from b, ca from c: a point ON a corner has r = 0 and dist2 exactly 0);
 *     face, q = p - a:  v = dot(q, gv), w = dot(q, gw);  counted only when v >= 0, w >= 0, v + w <= 1;  r = fmaf(w, ca, fmaf(-v, ab, q)).
 *   The pair's value is the smallest, the first of (ab, bc, ca, face) on a tie; its point is fmaf(t, e, o), or for the face
 *   fmaf(-w, ca, fmaf(v, ab, a)).  Every candidate is the distance to a point of the triangle, so a zero-area or collinear triangle
 *   (gv = gw = 0, or weights without meaning) gives a finite value that is one, for every finite input.  A candidate replaces the
 *   running minimum only when it is smaller (strict, NaN never): non-finite points or corners give unspecified values, no fault,
 *   and tri in [-1, T_s).
 *   The grid is (blocks of queries) x (split) x S: the triangles of a shape are cut into `split` runs of whole LDS chunks of
 *   SG_MESHSDF_CHUNK records, and the partial minima meet in a 64-bit unsigned atomicMin on (bits(d2) << 32 | tri) — d2 >= +0, so
 *   its bits order like the value and the lowest index wins a tie.  workspace: the triangle records [T][32] fp32, then the packed
 *   minima [S][Q] uint64, which the entry point itself sets to all ones before the launch (nothing is read that the call did not
 *   write).  sg_meshsdf_distance_impl (testing / tuning): split > 0 forces the factor (capped by the number of chunks T allows),
 *   <= 0 = the host's choice; chosen (may be NULL) receives the factor used.  The results do not depend on it.
 *
 * sg_meshsdf_sign: depth [K][S][N][N] fp32 = K14's depth (NDC z, smaller = nearer the scan, 1.0 = nothing drawn) of the shapes under
 *   the K views vps [K][16] (host doubles, row-major, rounded ONCE to fp32 = M; 1 <= K <= SG_MESHSDF_MAX_SCANS, N <= 16384).  A row
 *   3 other than (0, 0, 0, 1) — a perspective view — is refused with SG_ERR_ARG.  Per point (x, y, z) and scan k:
 *     c_j = fmaf(M[j][2], z, fmaf(M[j][1], y, fmaf(M[j][0], x, M[j][3])))   j = 0, 1, 2       (the rows of sg_raster_setup)
 *     fx = fmaf(c_0, 0.5f N, 0.5f N),  fy = fmaf(c_1, -0.5f N, 0.5f N)
 *     in_window = fx >= 0 && fx < N && fy >= 0 && fy < N                                   (false for NaN)
 *     t = depth[k][s][(int) fy][(int) fx]                                                 (read only when in_window)
 *     visible_k = !in_window || t == 1.0f || c_2 < t - bias
 *   outside [S][Q] uint8 (may be NULL) = OR_k visible_k;  sdf [S][Q] fp32 = outside ? sqrtf(dist2) : -sqrtf(dist2), given iff dist2
 *   [S][Q] is given.  bias >= 0, finite; the callers' default is 2 / N, one texel in NDC units.  No map is read outside [0, N)^2
 *   for any input, non-finite included.
 * The scans of shapegan_amd/prepare.py: K directions on a Fibonacci sphere, computed on the host in float64:
 *   y = 1 - (2 i + 1) / K,  r = sqrt(1 - y^2),  phi = i pi (3 - sqrt 5),  d = (r cos phi, y, r sin phi);
 *   up = (0, 1, 0), or (1, 0, 0) when |d_y| > 0.9;  u = normalize(up x d),  v = d x u;  for the bounding radius rho the view has the
 *   rows u / rho, v / rho, -d / rho, (0, 0, 0, 1);  depth map k = sg_raster_* of the soup under it, N x N, nothing culled. */
#define SG_MESHSDF_CHUNK 256
#define SG_MESHSDF_MAX_SCANS 64
#define SG_MESHSDF_MAX_TRIANGLES 16777216      /* 2^24 */
#define SG_MESHSDF_MAX_POINTS 16777216         /* 2^24 per shape */
#define SG_MESHSDF_MAX_TOTAL_POINTS 268435456  /* 2^28 per call */
size_t sg_meshsdf_distance_workspace_bytes(long S, long T, long Q);
int sg_meshsdf_distance(const float* positions, const int64_t* tri_offsets, long S, long T, const float* points, long Q, float* dist2,
                        int* tri, float* closest, void* workspace, size_t workspace_bytes, hipStream_t stream);
int sg_meshsdf_distance_impl(const float* positions, const int64_t* tri_offsets, long S, long T, const float* points, long Q,
                             float* dist2, int* tri, float* closest, void* workspace, size_t workspace_bytes, int split, int* chosen,
                             hipStream_t stream);
int sg_meshsdf_sign(const float* points, long S, long Q, const float* depth, const double* vps, int K, int N, float bias,
                    const float* dist2, float* sdf, unsigned char* outside, hipStream_t stream);

/* ---- K17: exact t-SNE of a latent table: joint probabilities, the gradient of the KL divergence, the descent step ------------------
 * reference: demo_latent_space.py:58-60 (TSNE(n_components=2).fit_transform of all latent codes, the map the traversal walks on) and
 *            create_plot.py:88-96 (create_tsne_plot: the same embedding for the autoencoder, the auto-decoder and the GAN).  Those go
 *            through scikit-learn's Barnes-Hut approximation on the host; this is the exact form, whose gradient is one pass over the
 *            N x N affinities.
 * All tensors fp32, contiguous; 64-bit indexing throughout.  4 <= N <= SG_TSNE_MAX_POINTS = 65536, where P is 16 GiB; 1 <= D <=
 * SG_TSNE_MAX_DIMS, 1 <= perplexity < N - 1; beyond: SG_ERR_ARG before any launch, in the library and the twin alike.  Every sum has
 * a fixed order and there are no floating-point atomics: a repeated call gives the same bits.  The arithmetic of an element exists
 * once (csrc/tsne_core.h).
 *
 * sg_tsne_affinities: X [N][D] -> P [N][N], beta [N], plogp (one double).  Every step works in place in P:
 *   1. P[i][j] = sum_k (x_ik - x_jk)^2, differences squared and added in increasing k with fmaf (never |a|^2 + |b|^2 - 2ab);
 *      (a - b)^2 = (b - a)^2, so the distances are symmetric bit for bit.
 *   2. per row i, m = min_{j != i} P[i][j] and the search for beta: p_j = expf(-beta (P[i][j] - m)) for j != i (f32), sum_p = sum p_j
 *      and sum_dp = sum (P[i][j] - m) p_j in float64, H = log(sum_p) + beta sum_dp / sum_p; the rule is scikit-learn's
 *      _binary_search_perplexity: beta = 1 first; H > log(perplexity): lower bound = beta, beta doubles while the upper bound is open
 *      and becomes the midpoint afterwards; otherwise the mirror image with halving; over when |H - log(perplexity)| <= tol or after
 *      max_steps evaluations (max_steps >= 1, tol >= 0).  beta[i] is the LAST EVALUATED beta, and the row becomes
 *      P[i][j] = (float)(p_j / sum_p) at it, P[i][i] = 0.
 *   3. P[i][j] = P[j][i] = (P[i][j] + P[j][i]) / (float)(2N): one thread owns the pair, the sum commutes: P is exactly symmetric with
 *      an exactly zero diagonal.
 *   4. plogp = sum_{P > 0} P log P in float64: rows in float64 in a fixed order, then the rows in a fixed order.
 *   workspace: N doubles (sg_tsne_affinities_workspace_bytes).
 *
 * sg_tsne_gradient: Y [N][2], P [N][N], exaggeration -> grad [N][2] and, when kl is given, kl (one double; plogp, the double of
 *   sg_tsne_affinities, must be given with it).  With w_ij = 1 / (1 + |y_i - y_j|^2), j != i:
 *     s_i = sum_j w,  a_i = sum_j P_ij w (y_i - y_j),  r_i = sum_j w^2 (y_i - y_j),  k_i = sum_j P_ij log1p(|y_i - y_j|^2)
 *   in ONE pass over P (nothing of size N^2 is written, Z is not inside the pair sums); Z = sum_i s_i,
 *     grad_i = 4 (exaggeration a_i - r_i / Z),   kl = plogp + sum_i k_i + log Z       (always the KL of the un-exaggerated P).
 *   A row's sums are float partial sums over SG_TSNE_FLUSH pairs flushed into float64; Z and sum k_i are float64 in a fixed order.
 *   The full matrix is walked (no i < j shortcut): a row's sums belong to one workgroup.  workspace: 6 N + 2 doubles.
 *
 * sg_tsne_update: scikit-learn's _gradient_descent step on the 2N elements of Y, velocity, gains (in place):
 *     gains = velocity grad < 0 ? gains + 0.2 : gains 0.8;  gains = max(gains, min_gain);
 *     velocity = momentum velocity - lr (gains grad);  Y += velocity        (f32, no contraction).
 *
 * sg_tsne_step: sg_tsne_gradient followed by sg_tsne_update in the same launches, bit for bit what the two calls give; grad (and kl, when
 *   given) are outputs as there.  Nothing synchronises: a loop may queue every iteration. */
#define SG_TSNE_MAX_POINTS 65536
#define SG_TSNE_MAX_DIMS 65536
#define SG_TSNE_FLUSH 16
size_t sg_tsne_affinities_workspace_bytes(long N);
int sg_tsne_affinities(const float* X, long N, long D, double perplexity, double tol, int max_steps, float* P, float* beta,
                       double* plogp, void* workspace, size_t workspace_bytes, hipStream_t stream);
size_t sg_tsne_gradient_workspace_bytes(long N);
int sg_tsne_gradient(const float* Y, const float* P, long N, float exaggeration, const double* plogp, float* grad, double* kl,
                     void* workspace, size_t workspace_bytes, hipStream_t stream);
int sg_tsne_update(float* Y, float* velocity, float* gains, const float* grad, long N, float momentum, float lr, float min_gain,
                   hipStream_t stream);
int sg_tsne_step(float* Y, const float* P, long N, float exaggeration, const double* plogp, float* velocity, float* gains,
                 float momentum, float lr, float min_gain, float* grad, double* kl, void* workspace, size_t workspace_bytes,
                 hipStream_t stream);

/* ---- sphere tracing of SDFNet shapes (rendering/raymarching.py:render_image, get_shadows) ----------------------------------
 * S images of the same camera, M = width^2 pixels each; ray r = s * M + pixel.  Rays live in segments with an active list each
 * (active [2][nrays], counts [3][nseg] int32, seg_off [nseg + 1] int64): step `iter` reads list iter & 1 / counts iter % 3 and
 * appends the rays that neither hit nor missed to list / counts iter + 1 (in no particular order: results do not depend on it).
 * A segment that a step left with fewer than 2 rays is finished and its last ray counts as a hit (raymarching.py:119-124,
 * :57-60), which makes a batch of images equal to the images rendered one by one.
 *
 * sg_raymarch_rays (raymarching.py:65-102): camera [13] (host): position, right, up, forward (float64 xyz each), focal distance.
 * dir [M][3] = normalised float32 pixel rays; pos [S][M][3] = the entry into the sphere of `radius` (the camera position for rays
 * that miss it); status [S*M] = 0; active list 0 of segment s (seg_off = s * M) = the rays that enter the sphere; `counts` must
 * be zero on entry. */
int sg_raymarch_rays(const double* camera, int width, long nshapes, double radius, float* dir, float* pos, unsigned char* status,
                     int* active, int* counts, hipStream_t stream);
/* `steps` march steps from iteration first_iter (raymarching.py:104-122 / :46-58), enqueued without a host synchronisation:
 * the SDFNet forward (packed / zb1 / zb5 of sg_sdfnet_pack_shape_bias, per-shape mode) of every active ray, segment s using
 * latent s % nshapes, sdf = clamp(tanh + sdf_offset, -clampv, clampv), pos += dir * sdf; hit (status = 1) when
 * 0 < sdf < threshold, else dropped when |pos| > radius (shadow = 0) or pos.y > radius (shadow = 1), radius = radius0 for
 * segments < nshapes and radius1 for the others.  dir_period > 0: ray r uses dir[r % dir_period].  evals (optional, uint64):
 * += the number of SDFNet evaluations.  max_rays: a bound on the active rays of all segments (counts only fall from step to
 * step: the total the caller last read, or nrays); 0 enqueues nothing.  At most 256 segments. */
int sg_raymarch_steps(const float* packed, const float* zb1, const float* zb5, float* pos, const float* dir, long dir_period,
                      unsigned char* status, int* active, long nrays, int* counts, const int64_t* seg_off, long nseg, long nshapes,
                      long max_rays, long first_iter, int steps, float clampv, float threshold, float sdf_offset, float radius0, float radius1,
                      int shadow, unsigned long long* evals, hipStream_t stream);
/* the rays still active before step `iter` are hits (the iteration cap, raymarching.py:124 / :60) */
int sg_raymarch_finish(unsigned char* status, const int* active, long nrays, const int* counts, const int64_t* seg_off, long nseg,
                       long iter, hipStream_t stream);
/* After the camera march (raymarching.py:126-130, :155-163): sg_raymarch_classify applies the vertical cutoff to status (if
 * use_cutoff), writes ground[s] = the minimum y of image s's hits (+inf, the minimum over nothing, for an image without hits)
 * and the per-image offsets (int64 [S+1]) of the hits and of the
 * ground rays (pixels looking down that are not hits, met with the plane y = ground[s] within |xz| < 3; none when the image has
 * no hit).  The caller reads hit_off[S] / gnd_off[S] to size the outputs of sg_raymarch_emit (same arguments, same workspace):
 * hits in pixel order grouped by image (hit_pos [H][3], hit_sid [H]), slot [S*M] = hit index, -2 - ground index, or -1, and the
 * shadow rays of both get_shadows calls (raymarching.py:136, :165): rays [0, H) from the hits, [H, H + G) from the ground
 * points, start q + 0.1 d with d the float64 direction to `light` (host [3]); 2S segments (hits of image s, then its ground rays),
 * shadow_seg [2S + 1], shadow_counts [3][2S] and list 0 of shadow_active [2][H + G] ready for sg_raymarch_steps. */
size_t sg_raymarch_workspace_bytes(long M, long nshapes);
int sg_raymarch_classify(unsigned char* status, const float* pos, const float* dir, long M, long nshapes, int use_cutoff,
                         float vertical_cutoff, float* ground, int64_t* hit_off, int64_t* gnd_off, void* workspace,
                         size_t workspace_bytes, hipStream_t stream);
int sg_raymarch_emit(const unsigned char* status, const float* pos, const float* dir, long M, long nshapes, const float* ground,
                     const int64_t* hit_off, const int64_t* gnd_off, const double* light, float* hit_pos, int* hit_sid, int* slot,
                     float* shadow_pos, float* shadow_dir, int* shadow_active, int* shadow_counts, int64_t* shadow_seg,
                     const void* workspace, size_t workspace_bytes, hipStream_t stream);
/* Shading (raymarching.py:132-175) in float64: grad [H][3] = d sdf / d hit_pos (normalised here), shadow = status of the shadow
 * rays; diffuse, specular^20, rim light, color (host [3]) * (0.5 diffuse + 0.5), ground pixels darkened by 0.35 * shadow;
 * image [S][M][3] uint8 = truncated 255 * value. */
int sg_raymarch_shade(const int* slot, const float* hit_pos, const float* grad, const unsigned char* shadow, const float* dir, long M,
                      long nshapes, long nhits, const double* light, const double* color, unsigned char* image, hipStream_t stream);

/* ---- K18: narrow-band voxel grids: the SDFNet evaluated only in bricks near the surface ---------------------------------------------
 * reference: SDFNet.get_voxels / get_mesh, model/sdf_net.py:77-112, which evaluate the network at all R^3 lattice points although
 * marching cubes (K12) reads values only next to the surface.  These entry points are the bookkeeping of an evaluation that runs
 * sg_sdfnet_fwd on whole bricks near the level set and leaves one constant per brick elsewhere (shapegan_amd/brickgrid.py drives them).
 *
 * Lattice: S shapes of R^3 points, flat index x R^2 + y R + z, point (x, y, z) = (axis_x[x], axis_y[y], axis_z[z]) (three fp32
 * tables [R]).  mask (optional): [R^3] bytes shared by all shapes; a point whose byte is 0 is left out: its value is 1 whatever
 * the network says.  Bricks: B^3 points, B in {4, 8, 16}, R a multiple of B (anything else: SG_ERR_ARG before any launch);
 * nb = (R / B)^3 per shape, brick (bx, by, bz) of shape s has the id s nb + (bx (R / B) + by) (R / B) + bz (int32: S nb < 2^31),
 * its point (lx, ly, lz) the local index lx B^2 + ly B + lz, its corner n the local point ((n >> 2) & 1, (n >> 1) & 1, n & 1) (B - 1).
 * A value v is INSIDE when v < level (K12's test).
 *
 * Every brick is inactive (state 0), active (1) or newly active (2: listed by the last compaction).  At the end every point of
 * an active brick holds its value (the network's, or 1 where masked: the EVALUATED points) and every point of an inactive brick
 * the brick's FILL, the value of its corner 0 (masked points hold 1 there too).
 *
 * Seed.  sg_brick_points with corners = 1 lists the 8 corners of the bricks (bricks = NULL: of all S nb bricks, in order),
 * [M][8][3] and the shape of every point; one sg_sdfnet_fwd gives corner_values [S nb][8].  sg_brick_seed writes fill, state = 0,
 * the whole grid [S][R^3] (fill, or 1 where masked) and flag = 1 for every brick that
 *   (a) has corners on both sides of the level, or
 *   (b) has a corner with |v - level| <= band, or
 *   (c) touches the border of the lattice while pad = 1 and has a corner inside (K12's virtual shell of 1 makes a crossing), or
 *   (d) has one of its 26 neighbours with a fill on the other side (which flags both).
 * Continuation, one round: sg_brick_compact turns the flags into the ascending list of newly active bricks (state 2; the
 * previous ones become 1; the flags are cleared) and its count, by a scan in `workspace`, not by atomics: the list is the same on
 * every run.  sg_brick_points with corners = 0 lists their points [M][B^3][3] (masked points included, so that a brick is a fixed
 * block), sg_sdfnet_fwd evaluates them, sg_brick_scatter stores the values (1 where masked) at the bricks' places, and
 * sg_brick_grow flags every inactive brick N for which some point of a listed brick within Chebyshev distance 2 lattice steps of
 * a point of N lies on the other side of the level than N's fill (2, not 1: a K12 normal reads the central difference one step
 * beyond a crossing edge's corners).  The caller repeats until a count is 0 (the driver takes more than 3 R / B rounds for an internal error).
 *
 * Guarantee.  At the end every lattice point within Chebyshev distance 2 of an evaluated point that lies on the other side of the
 * level than anything next to it (another evaluated point, or the fill of an inactive brick within that distance) is itself
 * evaluated, and no two adjacent inactive bricks have fills on different sides.  sg_sdfnet_fwd gives a point the same bits wherever
 * it stands in a launch, so the evaluated values are those of the dense grid.  It follows that a crossing edge of the dense grid
 * between two evaluated points has its whole neighbourhood evaluated (the corners of its cells and the points K12's normals read),
 * that the surface component through it is followed to its end, and that the narrow-band grid has no crossing the dense grid lacks:
 * K12 of the narrow-band grid is EXACTLY K12 of the dense grid, vertices, normals and faces, except for the surface components of
 * the dense mesh that have no crossing edge between two evaluated points.  Those are pieces whose own lattice points (the inside of
 * a floater, the outside of a bubble) all lie in inactive bricks, on the other side than the brick's fill, and which no brick corner
 * came within `band` of: smaller than a brick.  Such a piece is absent as a whole; the surface is never open at a brick border.
 * band >= 0; the driver's default is the largest distance from a brick point to its nearest corner, sqrt(3) (B - 1) / 2 lattice
 * steps, times a Lipschitz bound of the field.
 *
 * Lists are written up to their count only; the grid is written in full by sg_brick_seed. */
size_t sg_brick_compact_workspace_bytes(long S, int R, int B);
int sg_brick_points(const int* bricks, long M, int corners, long S, int R, int B, const float* axis_x, const float* axis_y,
                    const float* axis_z, float* points, int* shape_index, hipStream_t stream);
int sg_brick_seed(const float* corner_values, const unsigned char* mask, long S, int R, int B, float level, float band, int pad,
                  int* state, float* fill, int* flag, float* grid, hipStream_t stream);
int sg_brick_compact(int* state, int* flag, long S, int R, int B, int* list, int* count, void* workspace, size_t workspace_bytes,
                     hipStream_t stream);
int sg_brick_scatter(const float* values, const int* bricks, long M, const unsigned char* mask, long S, int R, int B, float* grid,
                     hipStream_t stream);
int sg_brick_grow(const int* bricks, long M, const float* grid, const int* state, const float* fill, long S, int R, int B, float level,
                  int* flag, hipStream_t stream);

/* ---- K19: signed distances from oriented point clouds: k nearest neighbours, normals, the normal-vote sign -----------------------
 * reference: mesh_to_sdf's sign_method = 'normal' (the package's default; demo_training.py:16, create_plot.py:636, and what
 *            prepare_shapenet_dataset.py:33,129 selects with USE_DEPTH_BUFFER = False): the distance to the nearest sample of an
 *            oriented cloud, the sign from a vote of the normals of the sample_count = 11 nearest samples.  K16 is the 'depth' method.
 * Input: S ragged clouds, points [N][3] fp32 with cloud_offsets [S+1] int64, and S ragged query sets, queries [M][3] fp32 with
 * query_offsets [S+1] int64 (device pointers; any run may be empty; a pointer whose array is empty may be NULL).  Every index in a
 * result is LOCAL to its shape's cloud.  1 <= S <= 65535; offsets start at 0, do not decrease and end at N / M; every run holds at
 * most 2^26 points (K13's limit); anything else is SG_ERR_ARG, on the GPU and in the twin alike.  The offsets decide every bound of
 * the walk, so the entry points read them back before the launch (one small copy and a wait on `stream`: the calls cannot be
 * captured in a graph).  No workspace: the only stores are to the result arrays, every element of which is written.
 *
 * sg_cloud_knn: idx [M][K] int32, d2 [M][K] fp32, 1 <= K <= SG_CLOUD_MAX_K.  For every query the K points of its shape's cloud that
 *   are smallest in the order (d2, index), ascending; d2 = K13's value of the pair (csrc/pointcloud_core.h), bit for bit.  Slots
 *   beyond the number of neighbours hold idx = -1, d2 = +inf.  A pair whose d2 is NaN or +inf is never a neighbour (non-finite
 *   coordinates: no fault, every idx in [-1, size)).  exclude_self != 0: the query runs must EQUAL the cloud runs (else SG_ERR_ARG),
 *   query i of a shape is its cloud point i, and the search skips the point with that INDEX — a duplicate of it at another index
 *   is a neighbour at distance 0.  The result is defined by the order alone: the same bits on the GPU, in the twin, under any tiling
 *   and wherever the shape stands in a batch.
 *
 * sg_cloud_normals: normals [N][3], variation [N] fp32 from idx [N][K] of a self-query with exclude_self.  All arithmetic is fp32,
 *   stated once in csrc/cloud_core.h with explicit fmaf (contraction off).  The samples of a point are itself and then its valid
 *   neighbours (0 <= idx < size) in slot order, n of them, each taken RELATIVE TO THE POINT: q_j = p_j - p_self (q_0 = 0), so the
 *   result does not change under a translation that is exact in fp32.  Centroid c = (sum of the q_j in sample order) / (float) n;
 *   with e_j = q_j - c the six sums xx, xy, xz, yy, yz, zz of the products, s = fmaf(e_a, e_b, s) in sample order.  The symmetric 3x3
 *   is diagonalised by SG_CLOUD_JACOBI_SWEEPS cyclic Jacobi sweeps over the pairs (0,1), (0,2), (1,2) — a fixed count, no test for
 *   convergence; a pair whose off-diagonal element is 0 is left alone:
 *     theta = (a_qq - a_pp) / (2 a_pq);  t = copysign(1, theta) / (|theta| + sqrtf(fmaf(theta, theta, 1)));  c = 1 / sqrtf(fmaf(t, t, 1));
 *     s = t c;  a_pp -= t a_pq;  a_qq += t a_pq;  a_pq = 0;  (x_p, x_q) <- (fmaf(c, x_p, -(s x_q)), fmaf(s, x_p, c x_q)) for the remaining
 *     row r of a and for the three rows of the eigenvector matrix (identity at the start).
 *   lambda = the diagonal; lambda_0 <= lambda_1 <= lambda_2.  normal = the column of the smallest (the LOWEST column on a tie),
 *   divided by its length sqrtf(fmaf(z, z, fmaf(y, y, x x)));  variation = lambda_0 / ((lambda_0 + lambda_1) + lambda_2).
 *   Orientation: view (x, y, z, w) fp32, [S][4], or [N][4] when view_per_point != 0: e = (x, y, z) - w p_self (a product, a
 *   difference), the normal is negated when fmaf(n_z, e_z, fmaf(n_y, e_y, n_x e_x)) < 0.  w = 1: a scanner position; w = 0: the
 *   direction toward an orthographic scanner (the d of K16's scans).  view = NULL ("unoriented"): the component of largest magnitude
 *   (the lowest axis on a tie) is made positive.  Degenerate: n < 3, or not lambda_1 > 2^-20 lambda_2 (a line, a point, NaN):
 *   normal = (0, 0, 0), variation = -1.  One lane per point; K as in sg_cloud_knn.
 *
 * sg_cloud_sdf: mesh_to_sdf's get_sdf(use_depth_buffer = False, sample_count = K) in one launch: sdf [M] fp32, nearest [M] int32
 *   (may be NULL).  The walk of sg_cloud_knn without exclude_self; for each valid neighbour j, in slot order, with its normal n
 *   (normals [N][3]): d = q - p_j, t_j = fmaf(d_z, n_z, fmaf(d_y, n_y, d_x n_x)); inside = 2 #{t_j < 0} > n_valid (a tie is not
 *   inside; a normal (0, 0, 0) gives t_j = 0, a vote for outside); sdf = sqrtf(d2[0]), negated when inside; nearest = idx[0].  No
 *   neighbour (an empty cloud, nothing finite): sdf = +inf, nearest = -1.  The same bits on the GPU and in the twin.
 *
 * Kernels (csrc/cloud.hip): one workgroup of SG_CLOUD_QUERY_TILE queries of ONE shape walks that shape's cloud, staged through LDS
 * in chunks of SG_CLOUD_STAGE points; every lane keeps its sorted list in registers (forms for 8, 16 and 32 entries: the smallest
 * that holds K runs, the first K entries are stored). */
#define SG_CLOUD_MAX_K 32
#define SG_CLOUD_QUERY_TILE 256
#define SG_CLOUD_STAGE 1024
#define SG_CLOUD_MAX_POINTS 67108864 /* 2^26 per run */
int sg_cloud_knn(const float* points, const int64_t* cloud_offsets, const float* queries, const int64_t* query_offsets, long S, long N,
                 long M, int K, int exclude_self, int* idx, float* d2, hipStream_t stream);
int sg_cloud_normals(const float* points, const int64_t* cloud_offsets, long S, long N, const int* idx, int K, const float* view,
                     int view_per_point, float* normals, float* variation, hipStream_t stream);
int sg_cloud_sdf(const float* points, const float* normals, const int64_t* cloud_offsets, const float* queries,
                 const int64_t* query_offsets, long S, long N, long M, int K, float* sdf, int* nearest, hipStream_t stream);

/* ---- K20: upscaling voxel grids: cubic B-spline prefilter, zoom and sampling --------------------------------------------------------
 * reference: scipy.ndimage.zoom(voxels_32, 4) of create_plot.py:826-828 ("hybrid_gan_upscaling"): a cubic B-spline prefilter with the
 *            mirror boundary, then a resampling at the positions o (n - 1) / (N - 1).  All three entry points follow that call's
 *            defaults (order 3, mode 'constant', grid_mode False); sg_spline_sample is scipy.ndimage.map_coordinates of the same kind.
 * Grids are [S][D][H][W] fp32, 1 <= D, H, W <= SG_SPLINE_MAX_AXIS, at most 2^36 elements per array and call; anything else is
 * SG_ERR_ARG before any launch.  S = 0, P = 0: 0 is returned and nothing is launched.  No workspace: the only stores are to the result
 * arrays, every element of which is written; an input and an output must not be the same array.  All arithmetic is fp32, stated once
 * in csrc/spline_core.h with explicit fmaf (contraction off): the same bits on the GPU, in the twin, in every kernel form and wherever
 * a grid stands in a batch.
 *
 * sg_spline_prefilter (create_plot.py:826-828): coefficients [S][D][H][W] of the grids: the line filter along W, then H, then D.  A
 *   line of n = 1 is copied; otherwise, with z = (float)(sqrt(3) - 2) and zn = z^(n-1): every c[i] times 6; c[0] = (sum over
 *   i = 0 .. n-2 of z^i (c[i] + zn c[n-1-i])) / (1 - zn zn); c[i] += z c[i-1] upward; c[n-1] = (z c[n-2] + c[n-1]) z / (z z - 1);
 *   c[i] = z (c[i+1] - c[i]) downward.  Forms (sg_spline_prefilter_form): 0 when D H (W | 1) <= SG_SPLINE_LDS_FLOATS — one workgroup
 *   holds the grid in LDS —, else 1: one pass per axis through global memory, the W pass staged through LDS.
 *
 * sg_spline_zoom (create_plot.py:826-828): out [S][D2][H2][W2] from the coefficients (order 3) or from the grids themselves
 *   (order 1; any other order is SG_ERR_ARG).  Per axis, output index o of N over an input of n: num = o (n - 1) in integers,
 *   f = num / (N - 1), t = (float)(num % (N - 1)) / (float)(N - 1); N = 1: f = 0, t = 0.  The taps f - 1 .. f + 2 carry the weights
 *   (1-t)^3/6, (3t^3 - 6t^2 + 4)/6, (-3t^3 + 3t^2 + 3t + 1)/6, t^3/6 (order 1: 0, 1 - t, t, 0) and are folded by the periodic mirror of
 *   period 2 (n - 1) (n = 1: index 0).  The 64 products are summed along W first, then H, then D (sg_spline_dot4).  Downscaling uses
 *   the same formula, without anti-aliasing.  Forms (sg_spline_zoom_form): 0 when the coefficient box of an 8 x 8 x 64 output tile and
 *   its two intermediates fit SG_SPLINE_ZOOM_LDS_FLOATS, as with every zoom factor >= 1, — tiles evaluated separably in LDS —, else 1:
 *   one lane per output.
 *
 * sg_spline_sample (create_plot.py:826-828, at arbitrary positions): values [S][P] and, unless NULL, gradient [S][P][3] at points
 *   [S][P][3] given in index coordinates (d, h, w) of the coefficients [S][D][H][W].  Inside 0 <= x <= n - 1 on every axis:
 *   f = floor(x), at most n - 2 (so x = n - 1 is t = 1), the same 64 taps, and the derivative weights for the gradient, which is
 *   with respect to the index coordinates.  Outside on any axis (NaN included): the value is `outside`, the gradient 0. */
#define SG_SPLINE_FORM_LDS 0
#define SG_SPLINE_FORM_GLOBAL 1
int sg_spline_prefilter_form(long D, long H, long W);
int sg_spline_zoom_form(long D, long H, long W, long D2, long H2, long W2);
int sg_spline_prefilter(const float* grids, long S, long D, long H, long W, float* coefficients, hipStream_t stream);
int sg_spline_zoom(const float* coefficients, long S, long D, long H, long W, long D2, long H2, long W2, int order, float* out,
                   hipStream_t stream);
int sg_spline_sample(const float* coefficients, long S, long D, long H, long W, const float* points, long P, float outside, float* values,
                     float* gradient, hipStream_t stream);

/* ---- K21: distance transforms of voxel grids: exact Euclidean distance transform and redistancing ------------------------------------
 * reference: the voxel models and VoxelDataset (datasets.py:7-40) hold distances clamped to +-0.1, stored as sdf / 0.1: beyond the
 *            truncation a grid says nothing but a sign.  scipy.ndimage.distance_transform_edt is the transform of an occupancy mask;
 *            the same transform from the level crossings of a grid ("redistancing") gives a truncated grid its distances back.
 * Grids are [S][D][H][W] fp32, 1 <= D, H, W <= SG_EDT_MAX_AXIS, at most 2^36 elements per array and call; spacing_d / _h / _w > 0 is
 * the world length of one index step, a voxel's position its index times the spacing.  Anything else is SG_ERR_ARG before any launch;
 * S = 0: 0 is returned and nothing is launched.  A SITE is a point q with an offset f(q) >= 0; the transform of a site set Q is
 *   T(p) = min over q in Q of f(q) + |p - q|^2   over the voxels p of the same grid, +inf when the grid has no site.
 * The grids of a call are independent.  T is computed by one pass per axis.  EXACTNESS: every pass returns, for every output p of a
 * line, the exact minimum over the line's candidates fmaf(d, d, g[q]), d = (float)(p - q) * spacing of that axis in fp32, g the
 * previous pass's result: min is exact and order-free, so the GPU in both forms and the twin return the same bits (csrc/edt_core.h
 * states the arithmetic once, contraction off).  The scan goes outward from p and stops when d d alone exceeds the best so far, which
 * is exact because g >= 0.  TIES are broken inside each pass by the smaller q; the nearest-site outputs follow from that.
 *
 * sg_edt_voxels (scipy.ndimage.distance_transform_edt): the sites are the background voxels, f = 0: a voxel with !(v < level), or with
 *   v < level when `inside` is not 0.  Passes: W, then H, then D.  squared [S][D][H][W] = T; with unit spacing every candidate is an
 *   integer below 2^24 and T is exact.  nearest (or NULL) [S][D][H][W] int: the linear index, within its grid, of a site that attains
 *   T, -1 when the grid has none.
 * sg_edt_crossings (redistancing): the sites are the points where a grid edge crosses `level` by linear interpolation, exactly the
 *   vertices sg_mc_emit makes of the unpadded grid with origin 0: an edge from voxel a to its successor b along an axis crosses when
 *   (va < level) != (vb < level), at the index coordinate u = (float)a + t, t = (level - va) / (vb - va) (mesh_core.h), f = 0.  The
 *   edges along one axis are a family: its first pass runs along that axis, candidate fmaf(d, d, 0), d = ((float)p - u) * spacing,
 *   and the two other axes follow in increasing order with integer offsets.  The families D, H, W are computed in this order and
 *   squared = their minimum, the earlier family on a tie.  closest (or NULL) [S][D][H][W][3]: the world position of the attaining
 *   crossing, ((float)a + t) * spacing on the edge's axis and index * spacing on the others; NaN when the grid has none.
 * sg_edt_finish: out = s sqrt(squared), s = -1 where v < level, else +1; sqrt is correctly rounded; a grid without sites gives s inf.
 *   keep_band != 0: a voxel with a 6-neighbour on the other side of the level keeps (v - level) * value_scale (world distance per
 *   grid unit: 0.1 for VoxelDataset grids, 1 for raw distances).  out may be `squared` itself.  grids = NULL (keep_band must be 0):
 *   out = sqrt(squared), the plain root, as scipy's transform returns it; level and value_scale are not used.
 * Forms (sg_edt_form, from the shape alone): 0 when D H W <= SG_EDT_LDS_FLOATS — one workgroup holds the grid in LDS and runs every
 *   pass there —, else 1: one launch per pass through global memory, neighbouring lanes on neighbouring w.
 * workspace: caller-owned, sg_edt_workspace_bytes(sites, S, D, H, W, nearest) bytes (sites: SG_EDT_VOXELS / SG_EDT_CROSSINGS; nearest:
 *   whether the optional output is requested; 0 bytes is possible, and NULL then allowed); fewer returns SG_ERR_WORKSPACE with the
 *   outputs untouched.  Nothing is read from it that the same call did not write.  Every element of every requested output is
 *   written.  All entries are asynchronous on `stream`, read no environment and keep no state. */
#define SG_EDT_FORM_LDS 0
#define SG_EDT_FORM_GLOBAL 1
#define SG_EDT_VOXELS 0
#define SG_EDT_CROSSINGS 1
int sg_edt_form(long D, long H, long W);
size_t sg_edt_workspace_bytes(int sites, long S, long D, long H, long W, int nearest);
int sg_edt_voxels(const float* grids, long S, long D, long H, long W, float level, int inside, float spacing_d, float spacing_h,
                  float spacing_w, float* squared, int* nearest, void* workspace, size_t workspace_bytes, hipStream_t stream);
int sg_edt_crossings(const float* grids, long S, long D, long H, long W, float level, float spacing_d, float spacing_h, float spacing_w,
                     float* squared, float* closest, void* workspace, size_t workspace_bytes, hipStream_t stream);
int sg_edt_finish(const float* grids, const float* squared, long S, long D, long H, long W, float level, float value_scale, int keep_band,
                  float* out, hipStream_t stream);

/* ---- data-parallel gradient exchange: libshapegan_comm.so ----------------------------------------------
 * reference: nn.DataParallel's gradient reduce-add, train_hybrid_progressive_gan.py:62-68.  One process per GPU; one
 * ncclAllReduce(sum, fp32) of a slice of the flat gradient buffer per call, on the communicator's own stream, ordered after
 * the work already enqueued on `compute_stream` (sg_allreduce_launch) — backward kernels enqueued afterwards overlap with it;
 * sg_allreduce_wait makes `compute_stream` wait for every exchange launched so far.  No host synchronisation.  The library
 * owns the communicator, its stream and two events between init and destroy; buffers stay the caller's.  Rank 0 makes the
 * unique id (sg_allreduce_unique_id) and distributes it out of band (a file, MPI, torch.distributed's store). */
typedef struct sg_comm sg_comm;
const char* sg_comm_last_error(void);
/* libshapegan_comm.so does not link RCCL: sg_comm_bind opens the RCCL the host process names (NULL: "librccl.so.1" by the loader's
 * search order) — for a PyTorch process the one torch.distributed's nccl backend has mapped, so that both live in one RCCL
 * instance — and must be called before any sg_allreduce_* entry.  sg_comm_versions: the NCCL_VERSION_CODE of the header the
 * library was compiled against and the version the bound library reports; a different major version is refused by sg_comm_bind. */
int sg_comm_bind(const char* librccl_path);
int sg_comm_versions(int* header_version, int* runtime_version);
size_t sg_allreduce_unique_id_bytes(void);
int sg_allreduce_unique_id(void* id_out, size_t bytes);
int sg_allreduce_init(sg_comm** comm, int rank, int world, const void* unique_id, size_t id_bytes, int device);
/* read back from the communicator: ranks = ncclCommCount, rank = ncclCommUserRank, device = ncclCommCuDevice, rccl_version =
 * ncclGetVersion (any pointer may be NULL) */
int sg_allreduce_info(sg_comm* comm, int* ranks, int* rank, int* device, int* rccl_version);
int sg_allreduce_launch(sg_comm* comm, float* buf, long count, hipStream_t compute_stream);
int sg_allreduce_wait(sg_comm* comm, hipStream_t compute_stream);
int sg_allreduce_destroy(sg_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* SHAPEGAN_HIP_H */
