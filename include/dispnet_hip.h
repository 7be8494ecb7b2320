/*
 * dispnet_hip.h -- flat C ABI of libdispnet_hip.so, the MI355X (gfx950) implementation of the
 * zenithfang/supervised_dispnet training hot path (encoder-decoder forward/backward + per-pixel losses).
 *
 * This is the drop-in boundary.  The reference has no native code: every entry
 * point below replaces the ATen/cuDNN op(s) that the cited reference line dispatches.  Host code (Python,
 * supervised_dispnet_amd/) binds these with ctypes; a reference maintainer would bind them the same way
 * (INTEGRATION.md).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP C++ types in signatures (dn_stream_t is a hipStream_t
 *     passed as void*; NULL = the null stream).
 *   - the library never allocates, frees or owns device memory; every buffer (workspace included) belongs to
 *     the caller and is borrowed for the duration of the enqueue.  No internal synchronisation.
 *   - every call returns 0 on success or a negative dn_status; dn_last_error() gives a thread-local message.
 *     Nothing throws across the ABI, nothing aborts.
 *   - re-entrant: no mutable global state (safe from PyTorch's autograd worker threads).
 *   - activations are NHWC fp32 (channels fastest).  Operands carry explicit element strides so NCHW user
 *     tensors (the 3-channel image) can be consumed without a transpose pass.
 *   - results are fp32 throughout.  The DEFAULT arithmetic of the matrix-core kernels (dn_conv_desc.compute = 0) forms every fp32
 *     product on the bf16 matrix cores from three exact bf16 pieces per operand (DN_COMPUTE_F32X3: six partial products on
 *     v_mfma_f32_32x32x16_bf16 / _16x16x32_bf16, fp32 accumulation; error against fp64 <= 1.5x an fp32 FMA chain's,
 *     tests/test_gpu_f32x3_fp64.py); kernels without a three-piece form, and every kernel under DN_COMPUTE_F32, run exact fp32 FMA
 *     chains on v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32.  The 3x3 / stride 1 / pad 1 layers with aligned channels use
 *     Winograd F(2x2,3x3): fp32 transforms (adds, halves) around those products, error at the level of the direct contraction
 *     (tests/test_gpu_kernels.py).
 */
#ifndef DISPNET_HIP_H_
#define DISPNET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dn_stream_t;

enum dn_status {
  DN_OK = 0,
  DN_ERR_BAD_ARG = -1,
  DN_ERR_UNSUPPORTED = -2,
  DN_ERR_WORKSPACE = -3,
  DN_ERR_LAUNCH = -4
};

void dn_reload_knobs(void);          /* re-read the DN_* tuning / test switches (they are read once, at first use) */
int dn_version(void);                 /* ABI version, bumped on any signature/struct change */
const char* dn_last_error(void);      /* thread-local, valid until the next failing call on this thread */
const char* dn_last_kernel(void);     /* thread-local: name (as rocprofv3 prints it) of the main kernel the last conv-family (or dn_colour_jitter_*) call launched */
int dn_device_arch_ok(void);          /* 1 if the current HIP device is gfx950, 0 otherwise, <0 on error */

/* ------------------------------------------------------------------------------------------------------------
 * Convolution family (implicit GEMM on MFMA).  One descriptor serves
 *   conv forward            nn.Conv2d            models/Disp_vgg_BN.py:40-50,66-70; torchvision vgg16_bn features
 *   conv input-gradient     autograd of the same  train.py:521 (loss.backward())
 *   conv-transpose forward  nn.ConvTranspose2d   models/Disp_vgg_BN.py:53-64; models/DispNetS.py:30-34
 *   conv-transpose input-gradient, and both weight gradients.
 * Fused on the way in : virtual channel-concat of up to 3 operands (torch.cat, Disp_vgg_BN.py:162-185), nearest x2
 *                       upsample of an operand (upsample_nn_nearest, Disp_vgg_BN.py:10-11), BatchNorm-apply + ReLU of
 *                       the producer layer (features[...] BatchNorm2d + ReLU).
 * Fused on the way out: bias, activation (ReLU / LeakyReLU(0.1) / ELU / alpha*sigmoid+beta of predict_disp,
 *                       Disp_vgg_BN.py:66-70,168), per-channel batch-statistic partial sums for the following
 *                       BatchNorm, channel-split of the result into up to 3 destination tensors (backward of cat),
 *                       accumulate-into-destination (skip connections with two consumers).
 * ------------------------------------------------------------------------------------------------------------ */
#define DN_MAX_OPERANDS 3

enum dn_activation {
  DN_ACT_NONE = 0,
  DN_ACT_RELU = 1,
  DN_ACT_LEAKY = 2,        /* p0 = negative slope */
  DN_ACT_ELU = 3,          /* alpha = 1 */
  DN_ACT_SIGMOID_AFFINE = 4 /* p0 * sigmoid(x) + p1 */
};

enum dn_conv_kind {
  DN_CONV_FWD = 0,         /* y = conv(x, w)                 in: x pieces,  out: y            */
  DN_CONV_DGRAD = 1,       /* dx = conv_dgrad(dy, w)         in: dy,        out: dx pieces    */
  DN_CONVT_FWD = 2,        /* y = conv_transpose(x, w)       in: x,         out: y            */
  DN_CONVT_DGRAD = 3       /* dx = conv_transpose_dgrad(dy)  in: dy,        out: dx           */
};

typedef struct dn_operand {        /* a read-only activation operand */
  const float* data;
  int32_t C;                       /* channels of this operand */
  int32_t up_shift;                /* 0, or 1 = stored at half resolution, nearest-x2 upsampled on the fly */
  int64_t stride_n, stride_h, stride_w, stride_c;   /* element strides of the STORED tensor */
  const float* scale;              /* optional [C]: value := max(0, value*scale[c] + shift[c]) on load */
  const float* shift;
} dn_operand;

typedef struct dn_result {         /* a destination tensor (channel stride 1) */
  float* data;
  int32_t C;
  int32_t accumulate;              /* 0: overwrite, 1: += */
  int64_t stride_n, stride_h, stride_w;
} dn_result;

typedef struct dn_conv_desc {
  int32_t kind;                    /* dn_conv_kind */
  int32_t N;
  int32_t IH, IW;                  /* spatial size seen by the taps (logical size of `in`, after up_shift) */
  int32_t OH, OW;                  /* spatial size of `out` (may crop a conv-transpose result, DispNetS.py:37-39) */
  int32_t R, S, stride, pad;       /* of the underlying nn.Conv2d / nn.ConvTranspose2d */
  int32_t n_in;
  dn_operand in[DN_MAX_OPERANDS];
  int32_t n_out;
  dn_result out[DN_MAX_OPERANDS];
  const float* w_packed;           /* from dn_conv_pack_weights for this kind */
  const float* bias;               /* optional [sum of out C] */
  int32_t act;                     /* dn_activation applied after bias */
  float act_p0, act_p1;
  float* bn_partial;               /* optional: [dn_conv_bn_partial_rows()][Cout][2] = (sum, sum of squared deviations from the
                                      tile mean) of the PRE-BIAS result per 128-row tile; requires n_out == 1 */
  int32_t pad_mode;                /* 0: zero padding; 1: reflection padding (nn.ReflectionPad2d(pad) in front of the conv,
                                      layers.py:124-136).  Reflection is honoured by DN_CONV_FWD and by the weight gradient;
                                      its input gradient = DN_CONV_DGRAD with pad 0 on the padded extent + dn_reflect_fold. */
  int32_t compute;                 /* Arithmetic of the matrix-core kernels that offer a choice (the Winograd, tiled and LDS-resident
                                      convolution kernels); tensors, statistics, transforms and all other kernels are fp32 in every mode.
                                      DN_COMPUTE_DEFAULT (0, what a zeroed descriptor gets): the library's default = DN_COMPUTE_F32X3.
                                      DN_COMPUTE_F32 (3): fp32 FMA chain on v_mfma_f32_32x32x2_f32 everywhere (0.74x the default's speed
                                        on the metric configuration); any unknown value is treated as this one.
                                      DN_COMPUTE_BF16: operands ROUNDED to bf16, fp32 accumulation (v_mfma_f32_32x32x16_bf16) -- the
                                        "mixed precision" mode of BASELINE configs[4]; ~4e-3 relative error per layer.
                                      DN_COMPUTE_F32X3: fp32 products on the bf16 matrix cores: each fp32 operand is split EXACTLY
                                        into three bf16 pieces (x = x0 + x1 + x2) and the six partial products of weight <= 2^-16
                                        (x0y0, x0y1, x1y0, x0y2, x1y1, x2y0) are accumulated in fp32; what is dropped is below
                                        2^-24 of |x||y|, the rounding an fp32 FMA chain commits itself (measured against fp64: the
                                        same error as DN_COMPUTE_F32 or less, tools/ubench/bf16x3.hip, tests/test_gpu_kernels.py). */
  int32_t dilation;                /* 0 / 1: none.  d > 1: nn.Conv2d(dilation = d) -- kernel tap (r, s) reads input offset
                                      (r*d - pad, s*d - pad) (models/ASPP.py:62-72,107-113: the dilated bottlenecks and the ASPP
                                      classifier).  Stride-1 DN_CONV_FWD / DN_CONV_DGRAD and their weight gradient, zero padding. */
  /* Optional, DN_CONV_DGRAD only (round 3): the column sums of the BatchNorm backward of the layer BELOW, taken in this call's epilogue.
   * The input gradient dx written here is dL/d(relu(bn(y))) of the producer of this layer's input; with bnb_y .. bnb_invstd set ([pixels][C]
   * dense like the result, [C] vectors) every 128-pixel tile also writes bnb_partial[tile][C][2] = (sum dz, sum dz * xhat),
   * dz = dx * [y * scale + shift > 0], xhat = (y - mean) * invstd -- exactly what dn_bn_relu_bwd_sums computes in a separate pass over dx
   * and y (one full read of dx and one launch saved per layer); rows = dn_conv_bn_partial_rows().  Honoured only where
   * dn_conv_dgrad_fuses_bn_sums() returns 1 (the Winograd input-gradient kernels, single non-accumulating result); otherwise ignored. */
  const float* bnb_y;
  const float* bnb_scale;
  const float* bnb_shift;
  const float* bnb_mean;
  const float* bnb_invstd;
  float* bnb_partial;
  /* Optional (round 3): workspace for the K split of small grids (Winograd input channels; chunks of the three-piece direct kernel).  A 4-image shard of the metric's batch leaves the
   * deep layers 32-104 blocks for 256 CUs, each walking all 32-48 chunks of the K axis alone; with a workspace of at least
   * dn_conv_splitk_workspace_bytes(desc) bytes the three-piece Winograd forward / input gradient splits K over 2-8 blocks per tile; the
   * partial output tiles meet here and the block that arrives last sums them in index order (deterministic) and runs the epilogue.
   * The first 4096 bytes are int counters: they must be ZERO before the first use and are left zero by every launch (self-resetting), so
   * one buffer serves every launch of ONE stream; launches on different streams need different buffers.  NULL: never split. */
  void* splitk_ws;
  int64_t splitk_ws_bytes;
  /* Optional (round 4): second result of a one-channel disparity head.  The reference computes depth = 1 / disp in
   * the caller, right behind the network (train.py:445, `depth = [1/disp for disp in disparities]`); when dn_conv_fwd_fuses_reciprocal(desc)
   * returns 1 the head kernel that writes disp = alpha * sigmoid(conv) + beta also writes 1 / disp here (dense [N][OH][OW] floats, the
   * same IEEE division dn_reciprocal_fwd performs), so the caller's reciprocal needs no launch.  Otherwise ignored; NULL: not wanted. */
  float* recip_out;
  /* Optional (round 5), DN_CONV_FWD with bn_partial: finish the BatchNorm batch statistics INSIDE this launch.  The block that arrives
   * last for a 64-channel slice of the result merges the slice's bn_partial rows and writes what dn_bn_finalize would have written
   * (mean, invstd, the folded (scale, shift), the running statistics, the step counter) -- same arithmetic, same order, same bits
   * (dn_bn_finalize takes the same sliced order for up to 128 partial rows); the conv bias is this descriptor's `bias`.  Honoured only
   * where dn_conv_fwd_folds_bn_finalize(desc) returns 1 (three-piece Winograd kernels, <= 128 partial rows, a splitk_ws whose last 256
   * bytes serve as self-resetting counters); otherwise ignored and the caller runs dn_bn_finalize.  bnf_scale == NULL: not wanted. */
  const float* bnf_gamma;
  const float* bnf_beta;
  float* bnf_running_mean;         /* may be NULL together with bnf_running_var (untracked statistics) */
  float* bnf_running_var;
  int64_t* bnf_num_batches_tracked;   /* may be NULL */
  float bnf_momentum, bnf_eps;
  float* bnf_mean;
  float* bnf_invstd;
  float* bnf_scale;
  float* bnf_shift;
  /* Optional (round 5), DN_CONV_DGRAD with bnb_*: also FINISH the two BatchNorm-backward sums of the layer below inside this launch:
   * bnb_dbeta[c] = sum dz, bnb_dgamma[c] = sum dz * xhat -- the parameter gradients dn_bn_bwd_apply_relu derives from bnb_partial with a
   * launch of its own (pass partial = NULL there: the sums are final).  Same sliced order as that launch for <= 128 rows.  Honoured
   * only where dn_conv_dgrad_folds_bn_sums(desc) returns 1. */
  float* bnb_dgamma;
  float* bnb_dbeta;
} dn_conv_desc;

enum { DN_COMPUTE_DEFAULT = 0, DN_COMPUTE_BF16 = 1, DN_COMPUTE_F32X3 = 2, DN_COMPUTE_F32 = 3 };

/* Elements of the packed weight buffer for desc->kind (depends on R,S,stride,pad, operand/result channels). */
int64_t dn_conv_packed_weight_elems(const dn_conv_desc* d);
/* Re-lay the framework weight tensor for desc->kind.  `w` is nn.Conv2d.weight [Cout][Cin][R][S] for DN_CONV_*,
 * nn.ConvTranspose2d.weight [Cin][Cout][R][S] for DN_CONVT_*.  Run once per optimizer step per kind. */
int dn_conv_pack_weights(const dn_conv_desc* d, const float* w, float* w_packed, dn_stream_t stream);
/* Every weight re-lay of a training step in (at most) two launches.  The caller keeps a table of dn_pack_entry_bytes()-sized rows:
 * dn_pack_entry_fill() writes one row on the HOST for (descriptor, framework weights, packed destination) and returns 1 for a
 * Winograd-layout row, 2 for a bf16 Winograd row, 3 for a three-piece bf16 Winograd row, 0 for a direct-layout row (<0: error); the
 * caller orders the rows direct, Winograd, bf16, three-piece, copies the table to the device once, and calls dn_pack_many(device table,
 * #direct, #winograd, #bf16, #three-piece, stream) after every optimizer step (same arithmetic as
 * dn_conv_pack_weights per row; the pointers in the rows must still be valid). */
int64_t dn_pack_entry_bytes(void);
int dn_pack_entry_fill(const dn_conv_desc* d, const float* w, float* w_packed, void* entry_host);
int dn_pack_many(const void* entries_dev, int32_t n_direct, int32_t n_wino, int32_t n_wino_bf16, int32_t n_wino_x3, dn_stream_t stream);
/* Which packed layout dn_conv_pack_weights produces for this descriptor: 0 = implicit-GEMM [phase][Npad][K chunks], 2 = the Winograd
 * layout below rounded to bf16 (descriptor compute = DN_COMPUTE_BF16), 3 = the same as three exact bf16 pieces (DN_COMPUTE_F32X3),
 * 1 = Winograd
 * F(2x2,3x3) transformed weights in MFMA fragment order (3x3 / stride 1 / pad 1 layers with 16-aligned channels and even
 * extents that fill the kernel's tiles).  The layout depends on the geometry, not only on the weights: a caller that caches
 * packed weights must key the cache on it (the same layer at another resolution may pick the other algorithm). */
int32_t dn_conv_weight_layout(const dn_conv_desc* d);
/* Number of row tiles (first dimension of bn_partial) the launch of this descriptor uses. */
int32_t dn_conv_bn_partial_rows(const dn_conv_desc* d);
/* Bytes of dn_conv_desc.splitk_ws this call would use at most (0: the call does not split; < 0: bad descriptor).  Two kernel families
 * split: the three-piece Winograd forward / input gradient (input channels) and the three-piece direct kernel with one scheduled operand
 * (chunks of the K axis: the 4x13 / 8x26 transposed convolutions of the decoder). */
int64_t dn_conv_splitk_workspace_bytes(const dn_conv_desc* d);
/* 1 when dn_conv2d_fwd(desc) will finish the BatchNorm statistics itself (dn_conv_desc.bnf_*), 0 when the caller has to run
 * dn_bn_finalize; likewise for the input gradient and the BatchNorm-backward sums (dn_conv_desc.bnb_dgamma / bnb_dbeta). */
int32_t dn_conv_fwd_folds_bn_finalize(const dn_conv_desc* d);
int32_t dn_conv_dgrad_folds_bn_sums(const dn_conv_desc* d);
/* 1 if dn_conv2d_dgrad(d) will write bnb_partial (see dn_conv_desc), 0 if it ignores the bnb_* fields, < 0 on a bad descriptor. */
int32_t dn_conv_dgrad_fuses_bn_sums(const dn_conv_desc* d);
/* 1 if dn_conv2d_fwd(d) writes 1 / out[0] to d->recip_out (a one-channel head on the second-generation head kernel), else 0. */
int32_t dn_conv_fwd_fuses_reciprocal(const dn_conv_desc* d);
/* Enqueue the convolution described by d. */
int dn_conv2d_fwd(const dn_conv_desc* d, dn_stream_t stream);      /* kind == DN_CONV_FWD */
int dn_conv2d_dgrad(const dn_conv_desc* d, dn_stream_t stream);    /* kind == DN_CONV_DGRAD */
int dn_convT2d_fwd(const dn_conv_desc* d, dn_stream_t stream);     /* kind == DN_CONVT_FWD */
int dn_convT2d_dgrad(const dn_conv_desc* d, dn_stream_t stream);   /* kind == DN_CONVT_DGRAD */

/* Weight gradient.  The descriptor is the FORWARD one (DN_CONV_FWD or DN_CONVT_FWD) with `in` = the forward
 * input pieces (same fused load transforms) and w_packed/bias/out ignored.  `dy` is the gradient w.r.t. the
 * pre-activation forward result, NHWC [N][OH][OW][Cout] contiguous.  Writes dw in the framework layout
 * ([Cout][Cin][R][S] / [Cin][Cout][R][S]).  Workspace: dn_conv_wgrad_workspace_bytes(). */
size_t dn_conv_wgrad_workspace_bytes(const dn_conv_desc* fwd);
int dn_conv2d_wgrad(const dn_conv_desc* fwd, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                    dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * BatchNorm (training statistics), ReLU, MaxPool 2x2, activations  --  all NHWC, HBM-bound.
 * Reference: torchvision vgg16_bn features used by models/Disp_vgg_BN.py:137-141.
 * ------------------------------------------------------------------------------------------------------------ */
/* partial (sum, M2 about the tile mean) [rows][C][2] of the pre-bias conv result (128-row tiles, merged with the
 * parallel-variance update in fp64) -> batch mean / biased var, folded affine
 * (scale = gamma*invstd, shift = beta - mean*scale), running-stat update (momentum, unbiased var), save mean/invstd.
 * count = N*H*W.  training != 0.  num_batches_tracked (nullable): nn.BatchNorm2d's int64 step counter, incremented by one. */
int dn_bn_finalize(const float* partial, int32_t rows, int32_t C, int64_t count, const float* conv_bias,
                   const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                   float eps, float* mean, float* invstd, float* scale, float* shift, int64_t* num_batches_tracked,
                   dn_stream_t stream);
/* eval mode: scale/shift from running statistics. */
int dn_bn_eval_affine(int32_t C, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, float* scale, float* shift, dn_stream_t stream);
/* p = maxpool2x2(relu(y*scale+shift));  idx (uint8, one per output element): bits0-1 = argmax position in the
 * window (first max in row-major order, like ATen), bit2 = pooled value > 0.  scale == shift == NULL: y is a plain tensor
 * (already activated), p = maxpool2x2(y) -- the BatchNorm-free VGG encoders (reference models/Disp_vgg.py:79-100). */
int dn_bn_relu_pool_fwd(const float* y, const float* scale, const float* shift, int32_t N, int32_t H, int32_t W,
                        int32_t C, float* pooled, uint8_t* idx, dn_stream_t stream);
/* dz (full resolution, pre-ReLU gradient; zero where not routed) from dpooled, plus per-channel partial sums
 * [blocks][C][2] of (dz, dz*xhat), xhat = (y-mean)*invstd.  Returns blocks used via dn_reduce_blocks(). */
int dn_bn_relu_pool_bwd(const float* dpooled, const uint8_t* idx, const float* y, const float* mean,
                        const float* invstd, int32_t N, int32_t H, int32_t W, int32_t C, float* dz, float* partial,
                        dn_stream_t stream);
/* gradient of the plain 2x2 max-pool (dn_bn_relu_pool_fwd with NULL scale): dx[window arg-max] (+)= dpooled, 0 elsewhere. */
int dn_maxpool2_bwd(const float* dpooled, const uint8_t* idx, int32_t N, int32_t H, int32_t W, int32_t C, float* dx, int32_t accumulate,
                    dn_stream_t stream);
/* dz = da * (y*scale+shift > 0) in place on `da`, plus the same partial sums. */
int dn_bn_relu_bwd_reduce(float* da_dz, const float* y, const float* scale, const float* shift, const float* mean,
                          const float* invstd, int64_t rows, int32_t C, float* partial, dn_stream_t stream);
/* finalize partial sums -> dgamma, dbeta; then dy = gamma*invstd*(dz - dbeta/count - xhat*dgamma/count) in place.
 * partial: [partial_rows][C][partial_stride] with (sum dz, sum dz*xhat) at offsets partial_offset, partial_offset+1
 * (stride 2 / offset 0 for the reduce kernels above; stride 4 / offset 0 or 2 for dn_bn_add_relu_bwd). */
int dn_bn_bwd_apply(float* dz_dy, const float* y, const float* mean, const float* invstd, const float* gamma,
                    const float* partial, int32_t partial_rows, int32_t partial_stride, int32_t partial_offset, int64_t rows,
                    int32_t C, float* dgamma, float* dbeta, dn_stream_t stream);
/* The two passes above without a materialised dz: the *_sums calls only produce the partial sums (no full-size write), and the
 * apply_* calls re-derive dz on the fly -- from da and the ReLU mask (y*scale+shift > 0; `da_dy` is overwritten with dy), or from
 * the pooled gradient and the arg-max codes (`dy` [N,H,W,C] is written; the sparse full-resolution dz of a max-pool never exists). */
int dn_bn_relu_bwd_sums(const float* da, const float* y, const float* scale, const float* shift, const float* mean, const float* invstd,
                        int64_t rows, int32_t C, float* partial, dn_stream_t stream);
int dn_bn_relu_pool_bwd_sums(const float* dpooled, const uint8_t* idx, const float* y, const float* mean, const float* invstd, int32_t N,
                             int32_t H, int32_t W, int32_t C, float* partial, dn_stream_t stream);
int dn_bn_bwd_apply_relu(float* da_dy, const float* y, const float* scale, const float* shift, const float* mean, const float* invstd,
                         const float* gamma, const float* partial, int32_t partial_rows, int32_t partial_stride, int32_t partial_offset,
                         int64_t rows, int32_t C, float* dgamma, float* dbeta, dn_stream_t stream);
int dn_bn_bwd_apply_pool(const float* dpooled, const uint8_t* idx, const float* y, const float* mean, const float* invstd, const float* gamma,
                         const float* partial, int32_t partial_rows, int32_t partial_stride, int32_t partial_offset, int32_t N, int32_t H,
                         int32_t W, int32_t C, float* dy, float* dgamma, float* dbeta, dn_stream_t stream);
int32_t dn_reduce_blocks(int64_t rows, int32_t C);   /* rows of `partial` the reduce kernels above write */

/* ---- backward of a FROZEN BatchNorm (a module in eval mode inside a network that trains): mean = running_mean and
 * invstd = 1 / sqrt(running_var + eps) are constants, so  dy = (gamma * invstd) * dz,  dbeta = sum dz,  dgamma = sum dz * xhat,
 * xhat = (y - mean) * invstd.  Each form is ONE full-size pass: it writes dy and leaves partial[dn_reduce_blocks(rows, C)][C][2]
 * = per-block sums of (dz, dz * xhat) (rows = the pooled pixels for the pool form; [..][C][4] for the tail: main branch at 0,
 * downsample branch at 2), which dn_bn_frozen_finalize turns into dgamma, dbeta and the gradient of a conv bias in front of the
 * BatchNorm.  C % 4 == 0.  Every form evaluates an element with the same device function: same bits whichever form handles it. */
/* dn_bn_eval_affine that also hands out invstd[C] */
int dn_bn_frozen_affine(int32_t C, const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                        float* scale, float* shift, float* invstd, dn_stream_t stream);
/* gradient given as dz (a ReLU-less BatchNorm); overwritten with dy */
int dn_bn_frozen_bwd(float* dz_dy, const float* y, const float* mean, const float* invstd, const float* gamma, int64_t rows, int32_t C,
                     float* partial, dn_stream_t stream);
/* gradient given as da under the pending ReLU: dz = da * [y * scale + shift > 0]; overwritten with dy */
int dn_bn_frozen_bwd_relu(float* da_dy, const float* y, const float* scale, const float* shift, const float* mean, const float* invstd,
                          const float* gamma, int64_t rows, int32_t C, float* partial, dn_stream_t stream);
/* through the fused 2x2 max-pool: (dpooled, idx of dn_bn_relu_pool_fwd) expanded straight into dy [N,H,W,C]; dz is never written */
int dn_bn_frozen_bwd_pool(const float* dpooled, const uint8_t* idx, const float* y, const float* mean, const float* invstd, const float* gamma,
                          int32_t N, int32_t H, int32_t W, int32_t C, float* dy, float* partial, dn_stream_t stream);
/* the tail of dn_bn_add_relu_fwd with frozen BatchNorms: m = gout * [out > 0]; dy = (gamma * invstd) * m; with r_mean / r_invstd /
 * r_gamma (a frozen downsample BatchNorm) dr = (r_gamma * r_invstd) * m (overwrite), without them dr (+)= m (dr may be NULL). */
int dn_bn_frozen_add_relu_bwd(const float* gout, const float* out, const float* y, const float* mean, const float* invstd, const float* gamma,
                              const float* r, const float* r_mean, const float* r_invstd, const float* r_gamma, int64_t rows, int32_t C,
                              float* dy, float* dr, int32_t dr_accumulate, float* partial, dn_stream_t stream);
/* dbeta[c] = sum_r partial[r][c][offset], dgamma[c] = sum_r partial[r][c][offset + 1] (rows met in fp64, fixed order) and, unless
 * dbias is NULL, dbias[c] = (gamma[c] * invstd[c]) * dbeta[c] = sum dy: the gradient of a conv bias in front of the BatchNorm. */
int dn_bn_frozen_finalize(const float* partial, int32_t partial_rows, int32_t partial_stride, int32_t partial_offset, int32_t C,
                          const float* gamma, const float* invstd, float* dgamma, float* dbeta, float* dbias, dn_stream_t stream);

/* g_pre = g * act'(.) in place, using the stored POST-activation tensor y_post; also per-channel partial sums
 * [blocks][C] of g_pre (the conv bias gradient).  act: RELU / LEAKY(p0) / SIGMOID_AFFINE(p0,p1) / NONE. */
int dn_act_bwd_reduce_from(const float* g_in, float* g_out, const float* y_post, int32_t act, float p0, float p1, int64_t rows, int32_t C,
                           float* partial, dn_stream_t stream);   /* the same, out of place (g_in is not written) */
int dn_act_bwd_reduce(float* g, const float* y_post, int32_t act, float p0, float p1, int64_t rows, int32_t C,
                      float* partial, dn_stream_t stream);
/* out[c] = sum over rows of partial[row][c*stride + offset]  (finishes bias / gamma / beta gradients). */
int dn_colsum_finalize(const float* partial, int32_t rows, int32_t C, int32_t stride, int32_t offset, float* out,
                       dn_stream_t stream);
/* dlow[n,h,w] (+)= sum of the 2x2 block of dfull[n,2h..,2w..]   (backward of nearest x2 upsample, C == 1) */
int dn_upsample2x_nearest_bwd(const float* dfull, int32_t N, int32_t h, int32_t w, float* dlow, int32_t accumulate,
                              dn_stream_t stream);
/* the same for an NHWC tensor with C channels (layers.upsample, layers.py:193-196; C % 4 == 0 or C == 1) */
int dn_upsample2x_nearest_bwd_nhwc(const float* dfull, int32_t N, int32_t h, int32_t w, int32_t C, float* dlow, int32_t accumulate,
                                   dn_stream_t stream);
/* backward of ReflectionPad2d(pad): dxp is the gradient on the padded extent [N][H+2p][W+2p][C]; dx[N][H][W][C] (+)= the
 * sum over the padded positions that mirror onto each pixel. */
int dn_reflect_fold(const float* dxp, int32_t N, int32_t H, int32_t W, int32_t C, int32_t pad, float* dx, int32_t accumulate,
                    dn_stream_t stream);
/* out = relu( (y*scale + shift) + (r_scale ? r*r_scale + r_shift : r) )  -- the tail of a ResNet bottleneck:
 * bn3(conv3) + identity / downsample-BN, then ReLU (models/Disp_res_50.py:229-247).  NHWC, C % 4 == 0.
 * r == NULL: no residual, i.e. a materialised relu(bn(y)) (a BatchNorm+ReLU output that leaves the engine as a tensor). */
int dn_bn_add_relu_fwd(const float* y, const float* scale, const float* shift, const float* r, const float* r_scale, const float* r_shift,
                       int64_t rows, int32_t C, float* out, dn_stream_t stream);
/* m = gout * (out > 0).  dz_y = m; partial [dn_reduce_blocks(rows,C)][C][4] = sums of (m, m*xhat_y, m, m*xhat_r).
 * Residual branch: with r_mean/r_invstd (a downsample BatchNorm) dr = m (overwrite); without, dr (+)= m (dr may be NULL). */
int dn_bn_add_relu_bwd(const float* gout, const float* out, const float* y, const float* mean, const float* invstd, const float* r,
                       const float* r_mean, const float* r_invstd, int64_t rows, int32_t C, float* dz_y, float* dr, int32_t dr_accumulate,
                       float* partial, dn_stream_t stream);
/* MaxPool2d(kernel 3, stride 2, padding 1) on NHWC (models/Disp_res_50.py:73); idx (uint8 per output element) = window
 * position 0..8 of the first maximum in row-major order.  Backward gathers (deterministic), dx overwrite / accumulate. */
/* ceil_mode != 0: nn.MaxPool2d(..., ceil_mode=True) (models/ASPP.py:138): OH = ceil((H - 1) / 2) + 1 unless that window starts past the
 * input; the caller sizes out / idx with dn_maxpool3s2_out(H, ceil_mode). */
int32_t dn_maxpool3s2_out(int32_t H, int32_t ceil_mode);
int dn_maxpool3s2_fwd(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ceil_mode, float* out, uint8_t* idx, dn_stream_t stream);
int dn_maxpool3s2_bwd(const float* dout, const uint8_t* idx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ceil_mode, float* dx,
                      int32_t accumulate, dn_stream_t stream);
/* out = (x - sub) / div  element-wise (the input normalisation of networks/vgg_encoder.py:80, resnet_encoder.py:89) */
int dn_sub_div(const float* x, int64_t n, float sub, float div, float* out, dn_stream_t stream);
/* bilinear x2, align_corners = False, 1 channel (models/DispNetS.py:120,126,132), cropped to (OH,OW). */
int dn_upsample2x_bilinear_fwd(const float* low, int32_t N, int32_t h, int32_t w, int32_t OH, int32_t OW, float* out,
                               dn_stream_t stream);
int dn_upsample2x_bilinear_bwd(const float* dout, int32_t N, int32_t h, int32_t w, int32_t OH, int32_t OW, float* dlow,
                               int32_t accumulate, dn_stream_t stream);
/* ---- pieces of the FCRN / ASPP nets (reference models/FCRN.py, models/ASPP.py, models/res_aspp.py) ----
 * Batch statistics of a MATERIALISED NHWC tensor in the layout the conv epilogues write and dn_bn_finalize merges:
 * partial[dn_bn_stats_rows(rows)][C][2] = (sum, sum of squared deviations from the tile mean) per 128-row tile.  FCRN's up-projection
 * normalises a map interleaved from four convolutions (models/FCRN.py:97-113), so no single conv epilogue sees its statistics. */
int32_t dn_bn_stats_rows(int64_t rows);
int dn_bn_stats_partial(const float* x, int64_t rows, int32_t C, float* partial, dn_stream_t stream);
/* out = y*scale[c] + shift[c]: a BatchNorm output WITHOUT ReLU that leaves as a tensor (FCRN bn2, models/FCRN.py:236-237). */
int dn_bn_apply_fwd(const float* y, const float* scale, const float* shift, int64_t rows, int32_t C, float* out, dn_stream_t stream);
/* FCRN's up-projection (models/FCRN.py:74-113) interleaves four convolutions -- 3x3, 2x3, 3x2, 2x2, each with one zero row above and one
 * zero column to the left -- into a 2H x 2W map: phase (a, b) = (row parity, column parity).  That is exactly a ConvTranspose2d(6x6,
 * stride 2, padding 2) whose weight is assembled from the four (wt[ci][co][a + 4 - 2 kr][b + 4 - 2 ks] = w_ab[co][ci][kr][ks], zero
 * elsewhere), so the engine runs DN_CONVT_* on that composite weight; what the transposed convolution cannot carry are the four
 * separate biases:  x[n][2y+a][2x+b][c] += bias4[a][b][c]  and, backwards,  out4[a][b][c] = sum of g over phase (a, b) (fixed-order sums;
 * workspace of dn_phase_colsum_workspace_bytes(C)). */
int dn_phase_bias_add(float* x, int32_t N, int32_t H2, int32_t W2, int32_t C, const float* bias4, dn_stream_t stream);
size_t dn_phase_colsum_workspace_bytes(int32_t C);
int dn_phase_colsum(const float* g, int32_t N, int32_t H, int32_t W, int32_t C, float* workspace, float* out4, dn_stream_t stream);
/* out = act(x) element-wise (the ASPP classifier sums four dilated convolutions BEFORE its sigmoid, models/ASPP.py:117-123). */
int dn_act_fwd(const float* x, int64_t n, int32_t act, float p0, float p1, float* out, dn_stream_t stream);
/* F.interpolate(x, size=(OH, OW), mode='bilinear', align_corners=...) of a one-channel map [N][IH][IW] (models/FCRN.py:253,
 * models/ASPP.py:192); source index and weights computed in fp32 exactly as ATen does.  Backward gathers (deterministic). */
int dn_resize_bilinear_fwd(const float* in, int32_t N, int32_t IH, int32_t IW, int32_t OH, int32_t OW, int32_t align_corners, float* out,
                           dn_stream_t stream);
int dn_resize_bilinear_bwd(const float* dout, int32_t N, int32_t IH, int32_t IW, int32_t OH, int32_t OW, int32_t align_corners, float* din,
                           int32_t accumulate, dn_stream_t stream);
/* out[n][c] = scale * mean over pixels of x[n][p][c] (NHWC): pose = 0.01 * pose_pred(...).mean(3).mean(2), models/PoseExpNet.py:73-75 */
int dn_spatial_mean_fwd(const float* x, int32_t N, int64_t HW, int32_t C, float scale, float* out, dn_stream_t stream);
int dn_spatial_mean_bwd(const float* dout, int32_t N, int64_t HW, int32_t C, float scale, float* dx, dn_stream_t stream);
/* Tail of monodepth2's PoseDecoder, scale * mean_hw(conv1x1(x) + bias), as mean then product (csrc/dn_posetail.hip).
 * x [P][HW][C] fp32 NHWC, 16-byte aligned; w [O][C]; bias [O].  Only the first O_used outputs are produced:
 *   mean[p][c] = (1 / HW) sum_s x[p][s][c]                                   (kept for the backward)
 *   out[p][o]  = scale * (bias[o] + sum_c w[o][c] * mean[p][c]),  o < O_used   (dense [P][O_used])
 * Backward, one launch: dx[p][s][c] = (scale / HW) sum_{o < O_used} dout[p][o] w[o][c] (the plain gradient with respect to x),
 *   dw[o][c] = scale * sum_p dout[p][o] mean[p][c], dbias[o] = scale * sum_p dout[p][o], sums over p in index order; rows o >= O_used of
 *   dw [O][C] and dbias [O] are written as zeros.  Deterministic: fixed summation orders, no float atomics.
 * DN_ERR_BAD_ARG unless C % 64 == 0, C <= 512, 1 <= O_used <= O <= 24, HW >= 1, P >= 1. */
int dn_pose_tail_fwd(const float* x, const float* w, const float* bias, int32_t P, int64_t HW, int32_t C, int32_t O, int32_t O_used,
                     float scale, float* mean, float* out, dn_stream_t stream);
int dn_pose_tail_bwd(const float* dout, const float* mean, const float* w, int32_t P, int64_t HW, int32_t C, int32_t O, int32_t O_used,
                     float scale, float* dx, float* dw, float* dbias, dn_stream_t stream);
/* y = 1/x (train.py:445); dx = -dy * y*y */
int dn_reciprocal_fwd(const float* x, float* y, int64_t n, dn_stream_t stream);
int dn_reciprocal_bwd(const float* dy, const float* y, float* dx, int64_t n, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Losses and metrics (loss_functions.py)
 * ------------------------------------------------------------------------------------------------------------ */
enum dn_masked_loss_kind { DN_LOSS_L1 = 0, DN_LOSS_L2 = 1, DN_LOSS_BERHU = 2, DN_LOSS_SCALE_INV = 3 };
#define DN_LOSS_STATS 8   /* floats of per-group statistics kept between forward and backward */
/* The masked depth-loss family: l1_loss / l2_loss / berhu_loss / Scale_invariant_loss (loss_functions.py:77-189, one
 * group per SAMPLE: G = B, pixels = H*W) and Multiscale_{L1,FULL_L1,L2,berhu,scale_inv}_loss (:217-315, one group per
 * SCALE over the whole batch: G = 1, pixels = B*h*w, weight = 1/2^i, accumulate = (i > 0)).
 * Per group: mean over valid = 0 < gt < max_depth of f(gt, clamp(pred, 1e-3, max_depth)); then
 *   loss[0] = (accumulate ? loss[0] : 0) + weight * (1/G) * sum_g L_g.   Empty mask -> NaN like the reference.
 * stats: [G][DN_LOSS_STATS] (kept for the backward); workspace: dn_masked_loss_workspace_bytes(). */
size_t dn_masked_loss_workspace_bytes(int32_t G, int64_t pixels);
int dn_masked_loss_fwd(const float* gt, const float* pred, int32_t G, int64_t pixels, float max_depth, int32_t kind, float weight,
                       int32_t accumulate, float* stats, void* workspace, size_t workspace_bytes, float* loss, dn_stream_t stream);
/* The same forward as ONE launch (kinds L1 / L2 / scale-invariant, G <= 256): the block that arrives last reduces the split partials and
 * turns them into the loss, in the order of the separate launches -- bit-identical to dn_masked_loss_fwd.  `counter`: one int32 in device
 * memory, zero before the first call and left zero (calls that may overlap on the device need counters of their own). */
int dn_masked_loss_fwd_fused(const float* gt, const float* pred, int32_t G, int64_t pixels, float max_depth, int32_t kind, float weight,
                             int32_t accumulate, float* stats, void* workspace, size_t workspace_bytes, float* loss, int32_t* counter,
                             dn_stream_t stream);
/* dn_masked_loss_fwd in pieces, for one-process-per-GPU runs of the whole-batch losses (the reference's DataParallel sees the
 * gathered batch on GPU0, loss_functions.py:232-237): pass 0 -> stats[g][0..3] = (sum f, n, sum d, max r) of THIS rank's pixels;
 * the caller all-reduces them (columns 0..2 add, column 3 takes the max); kind berHu then runs pass 1 -> stats[g][0], [2], [4]
 * (sums that depend on the global max; they add across ranks); dn_masked_loss_finalize turns the stats into the loss. */
int dn_masked_loss_stats(const float* gt, const float* pred, int32_t G, int64_t pixels, float max_depth, int32_t kind, int32_t pass,
                         float* stats, void* workspace, size_t workspace_bytes, dn_stream_t stream);
int dn_masked_loss_finalize(float* stats, int32_t G, int32_t kind, float weight, int32_t accumulate, float* loss, dn_stream_t stream);
/* dpred = dloss * weight/G * dL_g/dpred  (0 outside the mask / clamp range).  berHu includes the gradient through its
 * max-residual threshold, like torch autograd.  dloss: device scalar. */
int dn_masked_loss_bwd(const float* gt, const float* pred, const float* stats, const float* dloss, int32_t G, int64_t pixels,
                       float max_depth, int32_t kind, float weight, float* dpred, dn_stream_t stream);
/* One level of generate_{max,avg,bilinear}_pyramid (loss_functions.py:191-215): [N][H][W] -> [N][H/2][W/2];
 * mode 0 max_pool2d(2,2), 1 avg_pool2d(2,2), 2 F.interpolate(scale_factor=0.5, bilinear, align_corners=False). */
int dn_pyramid_down2(const float* in, int32_t N, int32_t H, int32_t W, int32_t mode, float* out, dn_stream_t stream);
/* F.upsample(x, scale_factor=s, mode) of a 1-channel map (Multiscale_FULL_L1_loss, loss_functions.py:243):
 * mode 0 nearest, 1 bilinear (align_corners=False).  [N][h][w] -> [N][h*s][w*s]. */
int dn_upsample_int_fwd(const float* low, int32_t N, int32_t h, int32_t w, int32_t scale, int32_t mode, float* out, dn_stream_t stream);
int dn_upsample_int_bwd(const float* dout, int32_t N, int32_t h, int32_t w, int32_t scale, int32_t mode, float* dlow, dn_stream_t stream);
/* explainability_loss (loss_functions.py:357-364) for one mask tensor of n elements: binary_cross_entropy(mask, 1).
 * partial: [dn_reduce1d_blocks(n)] scratch. */
int32_t dn_reduce1d_blocks(int64_t n);
int dn_explainability_fwd(const float* mask, int64_t n, float weight, int32_t accumulate, float* partial, float* loss, dn_stream_t stream);
int dn_explainability_bwd(const float* mask, const float* dloss, int64_t n, float* dmask, dn_stream_t stream);
/* smooth_loss for ONE map [B][H][W] (loss_functions.py:367-386): sum of the 4 second-difference |.|.mean() terms,
 * scaled by `weight`, accumulated into loss[0] (caller zeroes it).  partial: scratch [dn_smooth_blocks][4]. */
int32_t dn_smooth_blocks(int32_t B, int32_t H, int32_t W);
int dn_smooth2_fwd(const float* map, int32_t B, int32_t H, int32_t W, float weight, float* partial, float* loss,
                   dn_stream_t stream);
int dn_smooth2_bwd(const float* map, const float* dloss, int32_t B, int32_t H, int32_t W, float weight, float* dmap,
                   dn_stream_t stream);
/* compute_errors (loss_functions.py:401-448): out[8] = abs_diff, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3.
 * crop rows [y1,y2) cols [x1,x2) (pass 0,H,0,W for none).  median_scaling != 0: valid_pred *= median(gt)/median(pred)
 * per sample (:432-433, torch.median = lower middle; exact radix select).  scratch: [B][11] floats. */
int dn_compute_errors(const float* gt, const float* pred, int32_t B, int32_t H, int32_t W, float max_depth, int32_t y1,
                      int32_t y2, int32_t x1, int32_t x2, int32_t median_scaling, float* scratch, float* out8,
                      dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Geometry / photometric family (inverse_warp.py, loss_functions.py:317-354, layers.py:199-245)
 * Images are planar [B][3][h][w]; depth [B][h][w]; rotation_mode 0 euler / 1 quat; padding_mode 0 zeros / 1 border;
 * align_corners is F.grid_sample's flag (the reference passes none: False on torch >= 1.3, True on its pinned 1.0.1).
 * ------------------------------------------------------------------------------------------------------------ */
/* pose_vec2mat + `intrinsics @ pose_mat` (inverse_warp.py:141-157,185-188) with the per-scale intrinsics rescaling of
 * loss_functions.py:328-329 folded in (downscale = 1 for plain inverse_warp):
 *   proj[b] (3x4) = K_s @ [R(pose)|t],  kinv_scaled[b] (3x3) = Kinv with columns 0,1 * downscale.
 * pose element (b, j) at pose[b*pose_stride_b + j], j = tx,ty,tz,rx,ry,rz. */
int dn_pose_proj_fwd(const float* pose, int64_t pose_stride_b, const float* K, const float* Kinv, int32_t B, int32_t rotation_mode,
                     float downscale, float* proj, float* kinv_scaled, dn_stream_t stream);
/* dpose from the per-block partial sums of dproj ([B][nblk][12], nblk = dn_warp_blocks(h,w)) written by the *_bwd below. */
int32_t dn_warp_blocks(int32_t h, int32_t w);
int dn_pose_proj_bwd(const float* pose, int64_t pose_stride_b, const float* K, int32_t B, int32_t rotation_mode, float downscale,
                     const float* dproj_partial, int32_t nblk, float* dpose, int64_t dpose_stride_b, int32_t accumulate,
                     dn_stream_t stream);
/* inverse_warp (inverse_warp.py:160-193): pixel2cam, projection, cam2pixel (zeros padding: out-of-range coordinates := 2,
 * no gradient), bilinear grid_sample.  warped: [B][3][h][w]. */
int dn_inverse_warp_fwd(const float* img, const float* depth, const float* proj, const float* kinv, int32_t B, int32_t h, int32_t w,
                        int32_t padding_mode, int32_t align_corners, float* warped, dn_stream_t stream);
/* gradients w.r.t. depth ([B][h][w], overwrite / accumulate) and the projection (partials, see dn_pose_proj_bwd). */
int dn_inverse_warp_bwd(const float* img, const float* depth, const float* proj, const float* kinv, int32_t B, int32_t h, int32_t w,
                        int32_t padding_mode, int32_t align_corners, const float* dwarped, float* ddepth, int32_t accumulate_depth,
                        float* dproj_partial, dn_stream_t stream);
/* One (scale, reference image) term of photometric_reconstruction_loss (loss_functions.py:331-342), fused: warp `ref`,
 * out-of-bound mask = 1 - prod_c(warped_c == 0), diff = (tgt - warped) * oob [* mask], loss (+)= weight * mean|diff|.
 * mask: explainability mask element (b,y,x) at mask[b*mask_stride_b + y*w + x], or NULL.
 * partial: [B * dn_warp_blocks(h,w)] scratch. */
int dn_photometric_fwd(const float* tgt, const float* ref, const float* depth, const float* proj, const float* kinv, const float* mask,
                       int64_t mask_stride_b, int32_t B, int32_t h, int32_t w, int32_t padding_mode, int32_t align_corners, float weight,
                       int32_t accumulate, float* partial, float* loss, dn_stream_t stream);
int dn_photometric_bwd(const float* tgt, const float* ref, const float* depth, const float* proj, const float* kinv, const float* mask,
                       int64_t mask_stride_b, int32_t B, int32_t h, int32_t w, int32_t padding_mode, int32_t align_corners, float weight,
                       const float* dloss, float* ddepth, int32_t accumulate_depth, float* dproj_partial, float* dmask,
                       int64_t dmask_stride_b, dn_stream_t stream);
/* F.interpolate(x, (H/f, W/f), mode='area') for an exact integer factor (loss_functions.py:326-327): f x f mean. */
int dn_area_down(const float* in, int64_t planes, int32_t H, int32_t W, int32_t factor, float* out, dn_stream_t stream);
/* layers.SSIM.forward (layers.py:215-245) on [planes][H][W]; backward workspace: 5*planes*H*W floats; dx / dy nullable. */
int dn_ssim_fwd(const float* x, const float* y, int64_t planes, int32_t H, int32_t W, float* out, dn_stream_t stream);
int dn_ssim_bwd(const float* x, const float* y, const float* dout, int64_t planes, int32_t H, int32_t W, float* workspace, float* dx,
                float* dy, dn_stream_t stream);
/* layers.get_smooth_loss (layers.py:199-212): disp [B][1][H][W], img [B][C][H][W]; partial: [dn_edge_smooth_blocks][2]. */
int32_t dn_edge_smooth_blocks(int32_t B, int32_t H, int32_t W);
int dn_edge_smooth_fwd(const float* disp, const float* img, int32_t B, int32_t C, int32_t H, int32_t W, float* partial, float* loss,
                       dn_stream_t stream);
int dn_edge_smooth_bwd(const float* disp, const float* img, const float* dloss, int32_t B, int32_t C, int32_t H, int32_t W, float* ddisp,
                       dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * monodepth2 self-supervision (csrc/dn_reproj.hip; reference layers.py:28-103,139-190).  Matrices are row-major 4x4 ([B][16]).
 * ------------------------------------------------------------------------------------------------------------ */
/* (axisangle, translation) -> M [F][B][16].  Element e of the vector of (batch b, frame f) is read at p[b*sb + f*sf + e*se] (views of one
 * pose tensor: no contiguous copy).  mode 0: rot_from_axisangle (translation unused), 1: get_translation_matrix (axisangle unused),
 * 2: transformation_from_parameters, M = T R, or R^T T(-t) for a frame whose bit of invert_mask is set.  angle = |v|,
 * axis = v / (angle + 1e-7).  The backward writes daxisangle / dtranslation as contiguous [F][B][3] (either may be NULL). */
int dn_pose_matrix_fwd(const float* axisangle, int64_t aa_sb, int64_t aa_sf, int64_t aa_se, const float* translation, int64_t t_sb,
                       int64_t t_sf, int64_t t_se, int32_t B, int32_t F, int32_t mode, uint32_t invert_mask, float* M, dn_stream_t stream);
int dn_pose_matrix_bwd(const float* axisangle, int64_t aa_sb, int64_t aa_sf, int64_t aa_se, const float* translation, int64_t t_sb,
                       int64_t t_sf, int64_t t_se, int32_t B, int32_t F, int32_t mode, uint32_t invert_mask, const float* dM,
                       float* daxisangle, float* dtranslation, dn_stream_t stream);
/* BackprojectDepth: points [B][4][H*W], rows 0-2 = depth * inv_K[:3,:3] (x, y, 1), row 3 = 1 (the pixel grid is computed in the kernel). */
int dn_backproject_fwd(const float* depth, const float* inv_K, int32_t B, int32_t H, int32_t W, float* points, dn_stream_t stream);
int dn_backproject_bwd(const float* dpoints, const float* inv_K, int32_t B, int32_t H, int32_t W, float* ddepth, dn_stream_t stream);
/* Project3D: grid [B][H][W][2] = ((c[:2] / (c[2] + eps)) / (W-1, H-1) - 0.5) * 2 with c = (K T)[:3,:] points; no clamp on c[2].
 * Backward: dpoints [B][4][H*W], dT [B][16]; partial: [B * dn_reproj_blocks(H, W) * 12] scratch. */
int32_t dn_reproj_blocks(int32_t H, int32_t W);
int dn_project3d_fwd(const float* points, const float* K, const float* T, int32_t B, int32_t H, int32_t W, float eps, float* grid,
                     dn_stream_t stream);
int dn_project3d_bwd(const float* points, const float* K, const float* T, const float* dgrid, int32_t B, int32_t H, int32_t W, float eps,
                     float* dpoints, float* partial, float* dT, dn_stream_t stream);
/* One channel of the minimum-reprojection loss, term [B][H][W] = w * mean_c SSIM(pred, tgt) + (1 - w) * mean_c |tgt - pred|, in one launch.
 * warp != 0: pred = ref sampled (bilinear, border padding, align_corners) where Project3D(BackprojectDepth(depth)) lands, computed per
 * tile into LDS; depth = 1 / (d_lo + d_span * disp) (disp_mode 1) or disp itself (disp_mode 0).  warp == 0: pred = ref (the identity
 * term of the automask; disp, K, inv_K, T unused). */
int dn_reproj_term(const float* tgt, const float* ref, const float* disp, const float* K, const float* inv_K, const float* T, int32_t B,
                   int32_t H, int32_t W, int32_t warp, int32_t align_corners, int32_t disp_mode, float d_lo, float d_span, float eps,
                   float ssim_weight, float* term, dn_stream_t stream);
/* m [n] = min over terms [C][n], sel [n] = the winning channel (a tie goes to the lowest), partial [dn_reproj_select_blocks(n)] scratch;
 * loss (nullable) = mean(m), a fixed-order fp64 sum in a second launch. */
int32_t dn_reproj_select_blocks(int64_t n);
int dn_reproj_select(const float* terms, int32_t C, int64_t n, float* m, uint8_t* sel, float* partial, float* loss, dn_stream_t stream);
/* Backward of one warped channel (two launches): the pixels with sel == channel carry dloss[0] / (B H W) (or dmap [B][H*W] when given).
 * workspace: 9 * B * H * W floats.  ddisp [B][H*W] is overwritten or (accumulate != 0) added to; partial: [B * dn_reproj_blocks * 12]. */
int dn_reproj_bwd(const float* tgt, const float* ref, const float* disp, const float* K, const float* inv_K, const float* T, int32_t B,
                  int32_t H, int32_t W, int32_t align_corners, int32_t disp_mode, float d_lo, float d_span, float eps, float ssim_weight,
                  const uint8_t* sel, int32_t channel, const float* dloss, const float* dmap, float* workspace, float* ddisp,
                  int32_t accumulate, float* partial, dn_stream_t stream);
/* partial [F][B][nblk][12] -> dT [F][B][16] (nullable) and, when the matrices came from dn_pose_matrix_fwd mode 2, the gradient of the
 * pose parameters, written with the strides of the parameters themselves (daxisangle, dtranslation: nullable together). */
int dn_reproj_pose_bwd(const float* partial, int32_t nblk, const float* K, int32_t B, int32_t F, float* dT, const float* axisangle,
                       int64_t aa_sb, int64_t aa_sf, int64_t aa_se, const float* translation, int64_t t_sb, int64_t t_sf, int64_t t_se,
                       uint32_t invert_mask, float* daxisangle, float* dtranslation, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * monodepth2's multi-scale objective (csrc/dn_mono2.hip): S <= 4 disparity maps, disp_s [B][H >> s][W >> s] (disp1..3 NULL beyond S),
 * H and W divisible by 2^(S-1).  up_s = disp_s upsampled bilinearly (align_corners=False) to H x W, depth = 1 / (d_lo + d_span * up_s).
 * The number of launches of every entry point is independent of S.
 * ------------------------------------------------------------------------------------------------------------ */
/* The warped channel of one source frame at every scale in one launch: terms + s * scale_stride is the [B][H][W] term of scale s (the
 * formula of dn_reproj_term with warp != 0); the upsampled disparity exists in registers only. */
int dn_mono2_term(const float* tgt, const float* ref, const float* disp0, const float* disp1, const float* disp2, const float* disp3,
                  const float* K, const float* inv_K, const float* T, int32_t B, int32_t H, int32_t W, int32_t S, int32_t align_corners,
                  float d_lo, float d_span, float eps, float ssim_weight, float* terms, int64_t scale_stride, dn_stream_t stream);
/* Per scale the minimum over [ident [n_ident][n] (shared by the scales; n_ident may be 0), warped [S][F][n]], a tie going to the lowest
 * channel: sel [S][n], partial [S][dn_mono2_blocks(n)] = block sums of the minimum (times weights [S][n] when not NULL). */
int32_t dn_mono2_blocks(int64_t n);
int dn_mono2_select(const float* ident, int32_t n_ident, const float* warped, int32_t F, int32_t S, int64_t n, const float* weights,
                    uint8_t* sel, float* partial, dn_stream_t stream);
/* Three launches: mu [S][B] = per-sample mean of disp_s; the edge-aware smoothness of disp_s / (mu + 1e-7) under the 2^s x 2^s box
 * average of tgt, per 8 x 32 tile of the coarse map (T = dn_mono2_tiles(H, W) tiles per sample): smooth_partial [S * B * T * 2] scratch,
 * gbuf [sum_s B (H >> s)(W >> s)] = the gradient with respect to the normalised disparity and dot_partial [S * B * T] = the tiles' shares
 * of sum_j g_j d_j, both kept for dn_mono2_disp_grad; parts [S][2] = (mean minimum, smoothness) and
 * loss = (1 / S) sum_s (parts[s][0] + smoothness / 2^s * parts[s][1]) by fixed-order fp64 sums.  sel_partial: dn_mono2_select's. */
int32_t dn_mono2_tiles(int32_t H, int32_t W);
int dn_mono2_finish_fwd(const float* tgt, const float* disp0, const float* disp1, const float* disp2, const float* disp3, int32_t B, int32_t H,
                        int32_t W, int32_t S, const float* sel_partial, float smoothness, float* mu, float* smooth_partial, float* gbuf,
                        float* dot_partial, float* parts, float* loss, dn_stream_t stream);
/* Backward of one warped channel at every scale (two launches): the pixels of scale s with sel == channel carry dloss[0] / (S B H W)
 * (times weights).  workspace: S * 9 * B * H * W floats; ddfull [S][B][H*W], the gradient of the UPSAMPLED disparities, is overwritten
 * or (accumulate != 0) added to; partial: [B][S * dn_reproj_blocks(H, W)][12], which dn_reproj_pose_bwd takes with nblk = S * blocks. */
int dn_mono2_bwd(const float* tgt, const float* ref, const float* disp0, const float* disp1, const float* disp2, const float* disp3,
                 const float* K, const float* inv_K, const float* T, int32_t B, int32_t H, int32_t W, int32_t S, int32_t align_corners,
                 float d_lo, float d_span, float eps, float ssim_weight, const uint8_t* sel, int32_t channel, const float* dloss,
                 const float* weights, float* workspace, float* ddfull, int32_t accumulate, float* partial, dn_stream_t stream);
/* One launch: ddisp_s = upsampling^T ddfull[s] + dloss[0] * smoothness / (2^s S) * (g / (mu + 1e-7) - sum_j g_j d_j / (N (mu + 1e-7)^2)),
 * a gather in a fixed order; mu, gbuf, dot_partial: dn_mono2_finish_fwd's. */
int dn_mono2_disp_grad(int32_t B, int32_t H, int32_t W, int32_t S, const float* mu, const float* dloss, float smoothness, const float* ddfull,
                       const float* gbuf, const float* dot_partial, float* ddisp0, float* ddisp1, float* ddisp2, float* ddisp3,
                       dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * DORN ordinal head and loss (models/Disp_vgg_BN_DORN.py:196-227, loss_functions.py:16-74, utils.py:106-175)
 * ------------------------------------------------------------------------------------------------------------ */
/* OrdinalRegressionLayer: pre = logits, element (n, pixel, channel) at pre[n*stride_n + pixel*stride_pix + channel*stride_c]
 * (NHWC: 2K*HW, 2K, 1; NCHW: 2K*HW, 1, HW), channel pairs (A,B) = (2k, 2k+1); ord = planar [N][K][HW] =
 * softmax(clamp(A), clamp(B))[1]; decode = [N][HW] int64 count of ord > 0.5.  dpre has the layout of pre. */
int dn_ordinal_fwd(const float* pre, int64_t stride_n, int64_t stride_pix, int64_t stride_c, int32_t N, int64_t HW, int32_t K, float* ord,
                   int64_t* decode, dn_stream_t stream);
int dn_ordinal_bwd(const float* pre, int64_t stride_n, int64_t stride_pix, int64_t stride_c, const float* ord, const float* dord, int32_t N,
                   int64_t HW, int32_t K, float* dpre, dn_stream_t stream);
/* DORN_loss: target = SID labels int32 [N][HW]; stats[2] = (sum, num_valid) kept for the backward; loss = sum / -num_valid.
 * One process per GPU (the reference's DataParallel sees the gathered batch on GPU0 and divides by ITS valid count,
 * loss_functions.py:69-73): the caller sums `stats` over the ranks between dn_ordinal_loss_fwd and dn_ordinal_loss_finalize
 * (loss = stats[0] / -stats[1] again, from the exchanged pair) and passes grad_scale = world size to the backward, whose 1/num_valid
 * is then the whole batch's; grad_scale = 1 otherwise. */
int32_t dn_ordinal_loss_blocks(int32_t N, int64_t HW);
int dn_ordinal_loss_fwd(const float* ord, const float* gt, const int32_t* target, int32_t N, int64_t HW, int32_t K, float max_depth,
                        float* partial, float* stats, float* loss, dn_stream_t stream);
int dn_ordinal_loss_finalize(const float* stats, float* loss, dn_stream_t stream);
int dn_ordinal_loss_bwd(const float* ord, const float* gt, const int32_t* target, const float* stats, const float* dloss, int32_t N,
                        int64_t HW, int32_t K, float max_depth, float grad_scale, float* dord, dn_stream_t stream);
/* get_labels_sid / get_depth_sid (beta = 80.999 kitti, 10.999 nyu). */
/* Fused head (models/Disp_vgg_BN_DORN.py:112-114,191-227): Dropout2d channel mask (mask[N][16] = 0 or 1/(1-p), NULL = none) ->
 * 1x1 convolution 16 -> 2K (w = conv_ord.weight [2K][16], bias [2K]) -> clamp -> pair softmax.  The 2K-channel logits never reach
 * HBM: forward writes ord [N][K][HW] (planar, the reference's NCHW) and decode [N][HW] int64; backward takes dord (planar) and
 * recomputes the logits, producing dx [N][HW][16] (NHWC, accumulate != 0 adds), dw [2K][16] and dbias [2K] (fixed-order sums of
 * per-block partials in `workspace`: dn_ord_head_bwd_blocks() * (2K*16 + 2K) floats).  Supported (dn_ord_head_supported): 16 input
 * channels, H*W % 64 == 0, K <= 80; otherwise use dn_conv2d_fwd + dn_ordinal_fwd. */
int32_t dn_ord_head_supported(int32_t C_in, int64_t HW, int32_t K);
int32_t dn_ord_head_bwd_blocks(int32_t N, int64_t HW);
int dn_ord_head_fwd(const float* x, const float* mask, const float* w, const float* bias, int32_t N, int64_t HW, int32_t K, float* ord,
                    int64_t* decode, dn_stream_t stream);
int dn_ord_head_bwd(const float* x, const float* mask, const float* w, const float* bias, const float* dord, int32_t N, int64_t HW, int32_t K,
                    float* dx, int32_t accumulate, float* workspace, float* dw, float* dbias, dn_stream_t stream);
int dn_sid_labels(const float* depth, int64_t n, float ordinal_c, float beta, int32_t* labels, dn_stream_t stream);
int dn_sid_depth(const int64_t* labels, int64_t n, float ordinal_c, float beta, float* depth, dn_stream_t stream);
/* Dropout2d apply (and its backward): out[n][p][c] = x[n][p][c] * mask[n][c], NHWC. */
int dn_channel_scale(const float* x, const float* mask, int32_t N, int64_t HW, int32_t C, float* out, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Optimizer (train.py:303-305,520-522: torch.optim.Adam, wd = 0) over a flat parameter arena.
 * g is multiplied by grad_scale first (1/world_size folded in).  step >= 1.
 * ------------------------------------------------------------------------------------------------------------ */
int dn_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                 double eps, double weight_decay, int32_t step, double grad_scale, dn_stream_t stream);
/* The same update with the step counter and the learning rate on the DEVICE (hyper = {lr, beta1, beta2} as doubles, step = int32
 * counter the call increments first, derived = 4 floats of scratch), so that a captured hipGraph of the training step advances
 * the bias corrections on every replay and a scheduler changes lr by writing hyper[0]. */
int dn_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const double* hyper, double eps, double weight_decay,
                     int32_t* step, float* derived, double grad_scale, dn_stream_t stream);
/* Ranges of one arena updated by several calls (a bucket at a time, as its gradients -- and their all-reduce -- complete, under the rest of
 * the backward pass): dn_adam_tick advances the counter and the derived values ONCE per optimizer step, then every range is a
 * dn_adam_step_dev with step = NULL (no tick; `derived` as the tick left it).  Element-wise arithmetic: the same result as one call. */
int dn_adam_tick(const double* hyper, int32_t* step, float* derived, dn_stream_t stream);
/* torch.optim.SGD with momentum (train.py:300-301; dampening 0, nesterov off) over the same arena, fp32:
 *   gi = g*grad_scale; if (weight_decay != 0) gi += weight_decay*p; buf = momentum*buf + gi; p -= lr*buf.
 * buf is the momentum buffer and starts as ZEROS: momentum*0 + gi is the gradient copy torch's first step makes, so there is no step
 * counter.  momentum == 0 takes the same path.  p, g, buf: any 4-byte-aligned pointers, n >= 1; 16-byte accesses are used where the three
 * share their offset within 16 bytes, and every element sees the same arithmetic whichever lane handles it. */
int dn_sgd_step(float* p, const float* g, float* buf, int64_t n, double lr, double momentum, double weight_decay, double grad_scale,
                dn_stream_t stream);
/* The same update with hyper = {lr, momentum} as doubles on the DEVICE (narrowed to float as the host form narrows its arguments: the
 * two agree bit for bit), so that a captured step follows a scheduler that writes hyper[0].  A range of the arena per call (a bucket
 * at a time under the backward pass) needs nothing further: there is no per-step state besides buf. */
int dn_sgd_step_dev(float* p, const float* g, float* buf, int64_t n, const double* hyper, double weight_decay, double grad_scale,
                    dn_stream_t stream);
/* The same update with one learning rate per parameter GROUP (torch-style param_groups; train.py --diff-lr), as ONE launch over
 * elements [lo, hi) of the arena whatever the number of runs inside.  p, g, buf: the arena BASES, 16-byte aligned; lo, hi: multiples of
 * 4 (arena slices are padded to 4 elements; a slice's padding belongs to its group).  The arena is a sequence of runs of equal group,
 * described by three DEVICE arrays: seg_end[r] = element offset one past run r (ascending, multiples of 4, seg_end[n_seg-1] >= hi),
 * seg_group[r] = its group in [0, n_groups), group_lr[grp] = that group's learning rate (double, narrowed to float as dn_sgd_step
 * narrows lr: every element gets bit for bit what dn_sgd_step gives it with its group's rate).  Any n_seg >= 1.  The rates live on the
 * device in every mode, so an eager step and a replayed launch tape run the same kernel and both follow a write to group_lr.
 * 16-byte accesses only, 20 bytes of traffic per element; the run of an element is looked up per wave through the scalar cache. */
int dn_sgd_step_groups(float* p, const float* g, float* buf, int64_t lo, int64_t hi, const int64_t* seg_end, const int32_t* seg_group,
                       int32_t n_seg, const double* group_lr, int32_t n_groups, double momentum, double weight_decay, double grad_scale,
                       dn_stream_t stream);
int dn_fill(float* p, float value, int64_t n, dn_stream_t stream);
/* dst[i] = src[i], n floats (the owned copy engine.seed_grad takes of a gradient autograd hands over; on the launch tape like every
 * other kernel of this library, which a framework-side copy would not be). */
int dn_copy(const float* src, float* dst, int64_t n, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Launch tape (round 3).  The reference drives one training step as ~200 framework calls (train.py:437-455: forward, loss, backward,
 * optimizer.step()); at 4 images per GPU -- BASELINE.json's b32 over 8 GPUs -- the device needs ~4 ms for them and the Python side of
 * this library ~4 ms to issue them.  While a tape is being recorded (between dn_tape_begin and dn_tape_end, any thread) every kernel
 * launch of this library is ALSO kept: kernel, grid, block, LDS bytes, stream and the by-value kernel arguments.  dn_tape_replay
 * re-issues them with plain launches on the recorded streams (~2 us of host time each; a hipGraph of the same step replays SLOWER on
 * the device than the eager launches on ROCm 7.2).  The caller guarantees that every pointer the recorded
 * arguments hold is still valid and means the same at replay (graph.TapedStep records under a private memory pool and replays into the
 * same buffers), that the recorded streams exist, and that NO work the step needs was done outside this library while recording.
 *   dn_tape_fence(tape, waiter, waitee)  record "waiter waits for everything enqueued on waitee so far" (event record + stream wait at
 *                                        replay; does nothing now -- the caller fences the live run itself)
 *   dn_tape_fence_device(...)            the same between two streams whose work stays on THIS device (the engine's main and weight-gradient
 *                                        streams): the event is created without the system-scope fence (hipEventDisableSystemFence), which
 *                                        costs the recording stream's queue 2.3-5.9 us instead of 4.5-8.5 (tools/ubench/fence_cost.hip).  NOT for
 *                                        a stream whose results another GPU or the host reads (the communication stream).  When the last thing
 *                                        recorded on `waitee` is a kernel launch, the event is re-issued as that launch's STOP event
 *                                        (hipExtLaunchKernel) -- the dispatch's own completion signal, no marker packet behind the kernel
 *   dn_tape_mark(tape)                   cut: returns the number of the segment that starts here; the caller replays segment by
 *                                        segment and does its own host work in between (a gradient bucket's all-reduce)
 *   dn_tape_pause(tape, 1 / 0)           launches in between are executed but not recorded (such host work, when it is live at replay);
 *                                        a later dn_tape_fence_device never rides on a launch recorded in front of the pause
 *   dn_tape_replay(tape, segment)        segment -1: the whole tape
 * ------------------------------------------------------------------------------------------------------------ */
void* dn_tape_begin(void);
int dn_tape_end(void* tape);
int dn_tape_pause(void* tape, int32_t paused);
int dn_tape_fence(void* tape, dn_stream_t waiter, dn_stream_t waitee);
int dn_tape_fence_device(void* tape, dn_stream_t waiter, dn_stream_t waitee);
int32_t dn_tape_mark(void* tape);
int32_t dn_tape_segments(void* tape);
int64_t dn_tape_launches(void* tape);
int64_t dn_tape_fences(void* tape);
int64_t dn_tape_riding_fences(void* tape);   /* of those: device-scope fences that became the stop event of the launch in front of them */
int dn_tape_replay(void* tape, int32_t segment);
int32_t dn_tape_replay_timed(void* tape, int64_t* host_ns, const char** name, int32_t cap);   /* diagnostics: host time of every op of one replay */
void dn_tape_free(void* tape);

/* ------------------------------------------------------------------------------------------------------------
 * Input pipeline on the device (reference custom_transforms.py: RandomHorizontalFlip :56-72, ArrayToTensor :40-53, Normalize :25-37;
 * datasets/sequence_folders.py:60-77).  src = pre-decoded uint8 frames [B,H,W,C] (NHWC, as imread returns them); flip = one byte per
 * sample (non-zero: mirror along W) or NULL; dst = fp32 [B,C,H,W] with the given plane / sample strides (in floats):
 *     dst[n,c,y,x] = ((float)src[n,y,x',c] / 255 - mean[c]) / std[c],  x' = flip[n] ? W-1-x : x      (IEEE fp32, that order)
 * mean / std: device pointers (general path); mean_host / std_host: the same values on the host, used by the C == 3, W % 4 == 0
 * fast path (pass both).  dn_flip_w applies the same per-sample mirror to the fp32 ground-truth depth [B,H,W] (out of place).
 * ------------------------------------------------------------------------------------------------------------ */
int dn_u8_normalize_flip(const uint8_t* src, const uint8_t* flip, int32_t B, int32_t H, int32_t W, int32_t C, const float* mean, const float* stdv,
                         const float* mean_host, const float* std_host, float* dst, int64_t dst_stride_n, int64_t dst_stride_c, dn_stream_t stream);
int dn_flip_w(const float* src, const uint8_t* flip, int32_t B, int32_t H, int32_t W, float* dst, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Random scale-and-crop of the shard loader (reference custom_transforms.py: RandomScaleCrop :73-113), fused with
 * the flip and the normalisation above.  Equality with the host chain (data.Transform(scale_crop=True)) is the contract.
 * Draws per sample, on the host, in the reference's Compose order: the flip draw first, as without the augmentation; then
 * sx, sy = uniform(1, 1.15, 2) (x first); sh = int(H * sy), sw = int(W * sx) (fp64 product, truncated); oy = randint(sh - H + 1),
 * ox = randint(sw - W + 1).  All images of a sample (target and references) and its depth share them.
 * Image, per frame F (uint8 [H][W][3]; the reference sees the same integers as float32):
 *   1. flip: F'[y][x] = F[y][W-1-x] if the sample is flipped;
 *   2. byte-scale by the frame's own min / max over all three channels, the rule of dn_imresize_u8 below:
 *      uint8(clip(fp32((fp32(a) - cmin) * fp32(255.0 / (cmax - cmin))) + 0.5f, 0, 255)), scale 1 for a constant frame.  ALWAYS applied,
 *      also when sh == H and sw == W (the reference calls imresize unconditionally, on a float array); every frame has its own min / max;
 *   3. horizontal pass at the crop columns X = ox + x: Pillow's 8-bit bilinear coefficients of the axis W -> sw at output index X are a
 *      first input index and at most 3 fixed-point taps of 22 bits; out = clip8((2^21 + sum_i k_i * A[y][first + i]) >> 22), stored as
 *      uint8.  Skipped when sw == W;
 *   4. vertical pass at the crop rows Y = oy + y, the same on the uint8 result of step 3 for the axis H -> sh.  Skipped when sh == H;
 *   5. img[c][y][x] = ((float)u8 / 255 - mean[c]) / std[c] in IEEE fp32, that order: bit-identical to dn_u8_normalize_flip of the uint8
 *      result.
 * Depth, fp32 [H][W], finite values: 1. flip; 2. gmax = max(D) in fp32; 3. the same byte-scale over the map's own min / max (fp32
 * subtraction, scale = fp32(255.0 / (fp64(max) - fp64(min))); a sparse map has min 0, an all-zero map scale 1); 4. the same two passes on
 * one channel; 5. out = fp32(fp64(u8) / 255.0 * fp64(gmax)).  This is the reference as written: it multiplies by the maximum only (the
 * minimum is not added back) and the ground truth comes out quantised to 256 levels.
 * Intrinsics (host, after the flip rule): row 0 times sx and row 1 times sy, each product in fp64 and rounded to fp32 once; then
 * cx -= ox, cy -= oy, in fp64 and rounded once; the inverse as without the augmentation.
 *
 * dn_scale_crop_minmax writes DN_IMAGE_CHUNKS partial (min, max) pairs per image in one launch: minmax_u8 = int32[N * B][DN_IMAGE_CHUNKS][2]
 * over the uint8 frames [N][B][H][W][3] (N images per sample: target, references) and minmax_depth = float[B][DN_IMAGE_CHUNKS][2] over the
 * fp32 maps [B][H][W]; the two consumers below fold them.  frames or depth may be NULL (with its workspace).
 * table = int32[B][W + H][4] on the device, built on the host per sample: rows [0, W) are the crop columns, rows [W, W + H) the crop rows,
 * each {first input index, k0, k1, k2} with unused k = 0.  A skipped axis is written as the identity, {index, 1 << 22, 0, 0}, which the
 * same arithmetic passes through exactly.  `first` counts in the FLIPPED frame; the kernels mirror the index when they load.
 * scaled_hw_host = int32[B][2] {sh, sw} on the host and max_taps = the largest tap count of the rows: sh < H, sw < W or more than
 * DN_SCALE_CROP_TAPS taps is DN_ERR_BAD_ARG and nothing is launched -- never a truncated filter (upscaling has support 1, so valid draws
 * cannot need more).  The kernels clamp every table index into the window they staged: a foreign table gives wrong pixels, not a fault.
 * dn_scale_crop_u8: one launch for all N * B frames -> out = fp32[N][B][3][H][W]; flip = uint8[B] or NULL; mean_host / std_host: 3 floats
 * each on the host.  dn_scale_crop_depth: depth fp32[B][H][W] -> out = fp32[B][H][W] (out of place).  Any H, W.
 * ------------------------------------------------------------------------------------------------------------ */
#define DN_SCALE_CROP_TAPS 3
int dn_scale_crop_minmax(const uint8_t* frames, const float* depth, int32_t N, int32_t B, int32_t H, int32_t W, int32_t* minmax_u8,
                         float* minmax_depth, dn_stream_t stream);
int dn_scale_crop_u8(const uint8_t* frames, const uint8_t* flip, int32_t N, int32_t B, int32_t H, int32_t W, const int32_t* minmax_u8,
                     const int32_t* table, const int32_t* scaled_hw_host, int32_t max_taps, const float* mean_host, const float* std_host,
                     float* out, dn_stream_t stream);
int dn_scale_crop_depth(const float* depth, const uint8_t* flip, int32_t B, int32_t H, int32_t W, const float* minmax_depth,
                        const int32_t* table, const int32_t* scaled_hw_host, int32_t max_taps, float* out, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * monodepth2's colour jitter of the shard loader, fused with the flip and the normalisation above.  Equality with
 * the host chain (data.colour_jitter_u8 -- Pillow itself --, then data.Transform.apply) is the contract: no tolerance.
 * frames = uint8 [N][B][H][W][3] (N images per sample: target, references); params = int32 [B][DN_COLOUR_PARAMS] on the device, one row
 * per sample shared by its N frames: {jittered (0 / 1), order, fp32 bits of the brightness, contrast and saturation factors, hue shift in
 * 0..255, 0, 0}; order = the four operations in the sequence they are applied, 2 bits each, the first in the low bits: 0 brightness,
 * 1 contrast, 2 saturation, 3 hue (each exactly once; an order that names contrast twice applies it twice with the first one's mean).
 * Per operation, on the frame as it is at that point of the chain (every blend in fp32 WITHOUT a fused multiply-add, clipped to
 * [0, 255] and truncated: blend(a, x, f) = fp32(a) + f * (fp32(x) - fp32(a))):
 *   brightness  blend(0, x, b);   saturation  blend(L, x, s), L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16;
 *   contrast    blend(m, x, c), m = int(sum(L) / (H * W) + 0.5) over the whole frame (integer sum, one fp64 division);
 *   hue         Pillow's rgb2hsv_row (V = max; grey -> H = S = 0; else fp32 quotients, the hue sextant in double rounded to fp32,
 *               fmod(h / 6 + 1, 1) in double, H and S = the double products with 255.0 truncated), H = (H + shift) mod 256, Pillow's
 *               hsv2rgb (double, round half away).  Taken also for shift 0: the round trip is lossy.
 * dn_colour_jitter_sums writes sum_ws = uint64 [N * B][DN_IMAGE_CHUNKS], the partial sums of L of every jittered frame after the
 * operations that precede contrast in its order (rows of unjittered samples are left untouched and never read).
 * dn_colour_jitter_normalize_flip: out = fp32 [N][B][3][H][W] = dn_u8_normalize_flip (same flip rule, same arithmetic) of the jittered
 * bytes; plain (or NULL) = the same of the bytes as they came, from the same read.  An unjittered sample gives out == plain.
 * dn_colour_jitter_u8: out = uint8 [N][B][H][W][3], the jittered bytes (a copy for an unjittered sample), no flip; out != frames.
 * Any H, W; N * B <= 65535.  mean_host / std_host: 3 floats each on the host.
 * ------------------------------------------------------------------------------------------------------------ */
#define DN_COLOUR_PARAMS 8
int dn_colour_jitter_sums(const uint8_t* frames, const int32_t* params, int32_t N, int32_t B, int32_t H, int32_t W, uint64_t* sum_ws,
                          dn_stream_t stream);
int dn_colour_jitter_normalize_flip(const uint8_t* frames, const uint8_t* flip, const int32_t* params, const uint64_t* sum_ws, int32_t N,
                                    int32_t B, int32_t H, int32_t W, const float* mean_host, const float* std_host, float* out, float* plain,
                                    dn_stream_t stream);
int dn_colour_jitter_u8(const uint8_t* frames, const int32_t* params, const uint64_t* sum_ws, int32_t N, int32_t B, int32_t H, int32_t W,
                        uint8_t* out, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * NYU Depth v2 input chain (reference datasets/nyu_depth_v2.py:76-110).  Training: raw = the stored samples [B,5,H0,W0] fp32 (RGB 0..255,
 * depth in metres, 0/1 mask); params = double[B][8] {flip, angle in degrees, crop row, crop column, zoom s >= 1, colour gain, 0, 0},
 * drawn on the host.  dn_nyu_prefilter writes minmax = float[B][DN_NYU_MINMAX_CHUNKS][2] partial (min, max) over all five channels and
 * coef = double[B][4][H0][W0], the cubic B-spline coefficients (mirror boundaries, fp64) of the flipped RGB + depth (W0 <= 1024).
 * dn_nyu_train_resample then writes, per output pixel of the OH x OW crop: the rotated value (scipy.ndimage.rotate order 3, mode
 * 'constant') rounded to fp32 and clipped to [min, max], zoomed bilinearly toward the top-left corner (skimage warp, fp64), depth / s,
 * RGB * gain clipped to [0, 255], cast to fp32 and normalised: img[B,3,OH,OW] = (x - mean[c]) / std[c] (IEEE fp32), depth[B,OH,OW].
 * Validation: dn_nyu_val_resize = scipy.ndimage.zoom(order=1) of src [B,3,IH,IW] fp32 to [B,3,OH,OW], rounded to fp32, then normalised.
 * mean_host / std_host: 3 floats each on the host.
 * ------------------------------------------------------------------------------------------------------------ */
#define DN_NYU_MINMAX_CHUNKS 16
int dn_nyu_prefilter(const float* raw, const double* params, int32_t B, int32_t H0, int32_t W0, double* coef, float* minmax, dn_stream_t stream);
int dn_nyu_train_resample(const double* coef, const float* minmax, const double* params, int32_t B, int32_t H0, int32_t W0, int32_t OH,
                          int32_t OW, const float* mean_host, const float* std_host, float* img, float* depth, dn_stream_t stream);
int dn_nyu_val_resize(const float* src, int32_t B, int32_t IH, int32_t IW, int32_t OH, int32_t OW, const float* mean_host, const float* std_host,
                      float* dst, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Evaluation chain on the device (reference test_disp.py:391-398, :453-469).  pred = the network-resolution depth [B,h,w] fp32.
 * dn_eval_normalize: dst = ((div255 ? x / 255 : x) - mean[c]) / std[c] over fp32 frames [B,3,HW] (IEEE fp32, that order; mean_host /
 * std_host: 3 floats each on the host) -- the frames test_disp.py does not resize, and NYU's, which it does not divide by 255.
 * dn_zoom3_prefilter writes coef = double[B][h][w], the cubic B-spline coefficients (mirror boundaries, fp64; 3 <= h, 3 <= w <= 2048).
 * dn_zoom3_clip is scipy.ndimage.zoom(pred[b], (H_b/h, W_b/w)) with scipy's defaults (order 3, mode 'constant', cval 0,
 * grid_mode=False) followed by .clip(lo, hi): out_hw = int32[B][2] {H_b, W_b} and out_off = int64[B] (element offsets) on the device;
 * image b is written as H_b x W_b fp32 at out + out_off[b].  max_h / max_w: the largest H_b / W_b of the batch (sizes the grid).
 * Per axis, output o reads x = o * ((n-1)/(O-1)) (fp64; 0 if O == 1); x outside [0, n-1] gives exactly 0 (then lo).
 * dn_eval_errors: per image over the pixels with mask != 0 of the same ragged layout (npix[b] elements at off[b]):
 * scale_mode 0: 1; 1: fixed_scale; 2: np.median(gt) / np.median(pred) (fp32, even counts average the two middle elements);
 * pred * scale is rounded to fp32; a1..a3 compare max(gt/pred, pred/gt) in IEEE fp32; the four means take fp64 terms and fp64 sums.
 * out = float[B][8]: abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, scale (NaN for an empty mask).  One block per image does the
 * selection and the sums, so there is no workspace.  Masked gt and pred must be positive (the selection orders bit patterns).
 * ------------------------------------------------------------------------------------------------------------ */
int dn_eval_normalize(const float* src, int32_t B, int64_t HW, int32_t div255, const float* mean_host, const float* std_host, float* dst,
                      dn_stream_t stream);
int dn_zoom3_prefilter(const float* pred, int32_t B, int32_t h, int32_t w, double* coef, dn_stream_t stream);
int dn_zoom3_clip(const double* coef, int32_t B, int32_t h, int32_t w, const int32_t* out_hw, const int64_t* out_off, int32_t max_h,
                  int32_t max_w, float lo, float hi, float* out, dn_stream_t stream);
int dn_eval_errors(const float* gt, const float* pred, const uint8_t* mask, const int64_t* off, const int32_t* npix, int32_t B,
                   int32_t scale_mode, float fixed_scale, float* out, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * monodepth2's depth evaluation on the device (evaluate_depth.py; eval_disp.py --protocol monodepth2).
 * disp = the network's eval-mode disparity at network resolution, fp32.  Every step below is fp64 arithmetic on the fp32 inputs, without
 * contraction, and rounds to fp32 exactly once.
 * dn_mono2_post_process (batch_post_process_disparity): disp = fp32[2B][h][w]; planes B .. 2B-1 are the predictions for the horizontally
 * mirrored frames and are read mirrored (there is no un-flip pass); out = fp32[B][h][w], out != disp, w >= 2.  Per pixel (y, x):
 *     l = x / (w - 1);  lm(x) = 1 - clip(20 * (l - 0.05), 0, 1);  rm(x) = lm(w - 1 - x);
 *     L = disp[b][y][x];  R = disp[B + b][y][w - 1 - x];  out = rm * L + lm * R + (1 - lm - rm) * (0.5 * (L + R)).
 * dn_bilinear_recip_ragged: disp = fp32[B][h][w] resized bilinearly to a per-image size (H_b, W_b), then inverted; cv2 INTER_LINEAR /
 * F.interpolate(align_corners=False) geometry: half-pixel centres, replicated edges, no antialiasing when shrinking.  Per axis, output
 * index o, input length n, output length O:
 *     s = (o + 0.5) * (n / O) - 0.5;  i0 = floor(s);  f = s - i0;  i0 < 0: i0 = 0, f = 0;  i0 >= n - 1: i0 = n - 1, f = 0;
 *     i1 = min(i0 + 1, n - 1).
 * top = (1 - fx) * d[y0][x0] + fx * d[y0][x1], bot the same on row y1, value = (1 - fy) * top + fy * bot, out = fp32(1 / value): equal
 * sizes give exactly fp32(1 / disp).  out_hw = int32[B][2] {H_b, W_b} and out_off = int64[B] (element offsets) on the device, the ragged
 * layout of dn_zoom3_clip: image b is H_b x W_b fp32 at out + out_off[b], nothing is written between the images; max_h / max_w: the
 * largest H_b / W_b of the batch (sizes the grid).  Any h, w >= 1 and H_b, W_b >= 1; B <= 65535.  Four consecutive outputs are stored
 * as 16 bytes where out + out_off[b] is 16-byte aligned.
 * dn_eval_errors_clamp: dn_eval_errors (same arguments, same selection and sums, same out = float[B][8] with the scale in column 7)
 * in monodepth2's order: the scale -- in mode 2 the fp32 ratio of the medians of gt and of the UNCLAMPED pred over the mask -- is applied
 * first, p = min(max(fp32(pred * scale), lo), hi) second, then the metrics of (gt, p).  0 < lo <= hi.  Masked gt and pred must be
 * positive.
 * ------------------------------------------------------------------------------------------------------------ */
int dn_mono2_post_process(const float* disp, int32_t B, int32_t h, int32_t w, float* out, dn_stream_t stream);
int dn_bilinear_recip_ragged(const float* disp, int32_t B, int32_t h, int32_t w, const int32_t* out_hw, const int64_t* out_off, int32_t max_h,
                             int32_t max_w, float* out, dn_stream_t stream);
int dn_eval_errors_clamp(const float* gt, const float* pred, const uint8_t* mask, const int64_t* off, const int32_t* npix, int32_t B,
                         int32_t scale_mode, float fixed_scale, float lo, float hi, float* out, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Image arithmetic around the network (reference run_inference.py:121-183, utils.py:45-76).  Equality with the
 * host libraries is the contract: every step is integer or fixed fp32 / fp64 arithmetic.
 * dn_imresize_u8 = scipy.misc.imresize(frame, (h, w)) for a ragged batch of RGB uint8 frames: frame b is H_b x W_b x 3 bytes at byte offset
 * off[b] of `frames`; hw = int32[B][2] {H_b, W_b} and off = int64[B] on the device.  A frame that already is h x w is passed through.
 * Otherwise: byte-scale by the frame's min / max over all channels, uint8(clip(fp32((fp32(a) - cmin) * fp32(255.0 / (cmax - cmin))) + 0.5f,
 * 0, 255)) (scale 1 for a constant frame), then Pillow's 8-bit bilinear resize: the horizontal pass into uint8, then the vertical pass, a
 * pass whose axis keeps its size skipped; out = clip8((2^21 + sum k_x * in_x) >> 22).  The coefficients come from the host: `tabs` is a pool
 * of int32 tables on the device, one per resized axis, [O][2 + T] = {first input index, taps, k[T]} per output index (T = the table's
 * largest tap count, unused k are 0), and tab_idx = int32[B][4] {x table offset, its T, y table offset, its T} (in int32 elements; T = 0 for
 * an axis that keeps its size).  max_taps = the largest T: more than DN_IMRESIZE_MAX_TAPS is DN_ERR_BAD_ARG, never a truncated filter.
 * minmax = int32[B][DN_IMAGE_CHUNKS][2] workspace.  Outputs are dense and either may be NULL: out_u8 = uint8[B][h][w][3], out_f32 =
 * fp32[B][3][h][w] = (u8 / 255 - mean[c]) / std[c] in IEEE fp32, bit-identical to dn_u8_normalize_flip(flip = NULL) of out_u8
 * (mean_host / std_host: 3 floats each on the host).
 * dn_colorize_u8 = 255 * tensor2array(x[b, r0:r1, c0:c1]) as uint8[B][r1-r0][c1-c0][3] of fp32 maps x[B][h][w]; reciprocal != 0 colours
 * 1 / x (one IEEE division).  max_value < 0: the per-image maximum over the rectangle (max_ws = float[B][DN_IMAGE_CHUNKS], a NaN wins).
 * table = uint8[256][3] RGB on the device: index uint8(clip(fp32(fp32(255 * x) / max), 0, 255)), truncating; table = NULL: the grey
 * branch, uint8(fp32(255 * clip(fp32(x / max), 0, 1))) in all three channels.  A NaN (inf / inf) gives index / grey 0.
 * dn_contrast_u8 = PIL.ImageEnhance.Contrast(im).enhance(factor) on uint8[B][h][w][3]: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16,
 * m = int(sum(L) / (h * w) + 0.5) (integer sum, one fp64 division), out = uint8(clip(fp32(m) + factor * (fp32(p) - fp32(m)), 0, 255)).
 * sum_ws = uint64[B][DN_IMAGE_CHUNKS] workspace; src != dst.
 * dn_resize_u8 = PIL's Image.fromarray(frame).resize((w, h), Image.BILINEAR): dn_imresize_u8's two passes on the same tables WITHOUT the
 * byte-scale, which is what scipy.misc.imresize does to a frame that is uint8 already (data/kitti_raw_loader.py:224).  Same ragged
 * layout, tables and tap bound; the only output is out_u8 = uint8[B][h][w][3]; no workspace.
 * ------------------------------------------------------------------------------------------------------------ */
#define DN_IMAGE_CHUNKS 64
#define DN_IMRESIZE_MAX_TAPS 32
int dn_imresize_u8(const uint8_t* frames, const int32_t* hw, const int64_t* off, int32_t B, int32_t h, int32_t w, const int32_t* tabs,
                   const int32_t* tab_idx, int32_t max_taps, int32_t* minmax, uint8_t* out_u8, const float* mean_host, const float* std_host,
                   float* out_f32, dn_stream_t stream);
int dn_colorize_u8(const float* x, int32_t B, int32_t h, int32_t w, int32_t r0, int32_t r1, int32_t c0, int32_t c1, int32_t reciprocal,
                   float max_value, const uint8_t* table, float* max_ws, uint8_t* out, dn_stream_t stream);
int dn_contrast_u8(const uint8_t* src, int32_t B, int32_t h, int32_t w, float factor, uint64_t* sum_ws, uint8_t* dst, dn_stream_t stream);
int dn_resize_u8(const uint8_t* frames, const int32_t* hw, const int64_t* off, int32_t B, int32_t h, int32_t w, const int32_t* tabs,
                 const int32_t* tab_idx, int32_t max_taps, uint8_t* out_u8, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Pose evaluation on the device (eval_pose.py): odometry ATE / RE of the pose networks.
 * dn_snippet_gather: dst[n][3k + c][y][x] = ((ring[idx[n][k] mod R][y][x][c] / 255) - mean[c]) / std[c], IEEE fp32 in exactly that order
 * (dn_eval_normalize's rule).  ring = uint8[R][H][W][3], the resident resized frames, slot = frame index mod R (a negative index wraps
 * too: no table reads outside the ring); idx = int32[N][K] on the device; dst = fp32[N][3K][H][W], dense, the channel-concatenated
 * snippets one forward takes as ONE operand.  mean_host / std_host: 3 floats each on the host.  Any H, W >= 1: where H * W is a multiple
 * of 4 (and ring is 4-byte, dst 16-byte aligned) a thread moves 4 pixels as three words in and three float4 out, otherwise pixel by pixel.
 * dn_pose_eval_sfm (SfMLearner's test_pose.py): pose = fp32[N][L-1][6], the (tx, ty, tz, rx, ry, rz) of the reference frames in temporal
 * order; a zero row is inserted at L / 2 (the target), P[L][6].  M_k = pose_vec2mat(P_k) as [R|t] in fp64 FROM the fp32 vector
 * (rotation_mode 0: Rx Ry Rz, 1: the (1, x, y, z) quaternion normalised), R_k = inv(M_k[:, :3]), t_k = -R_k M_k[:, 3],
 * F_k = [M_0r R_k | M_0r t_k + M_0t].  gt = fp64[N][L][3][4], the compensated ground-truth poses.  With p = F:
 * s = sum(g_t . p_t) / sum(p_t . p_t) over all L translations, ATE = |g_t - s p_t|_2 / L,
 * RE = (1/L) sum_k atan2(|(D01 - D10, D12 - D21, D02 - D20)|_2, trace(D) - 1), D = g_kr inv(p_kr).  out = fp64[N][2] {ATE, RE}.
 * 2 <= L <= DN_POSE_EVAL_MAX_L.  All-zero predicted translations give ATE = 0 / 0 = NaN, as numpy does.
 * dn_pose_eval_mono2 (monodepth2's evaluate_pose.py): pose = fp32[P][6], (axisangle, translation) of the pairs (i, i + 1);
 * T_i = transformation_from_parameters(invert = False) = [Rodrigues(axisangle / (|axisangle| + 1e-7)) | translation] in fp64 from the
 * fp32 numbers; Q = fp64[P][4][4], the ground-truth local transforms (rows 0..2 are read).  Window i = 0 .. P-1 takes transforms
 * i .. min(i + track - 1, P) - 1 (shorter at the end): both trajectories start at the origin with C_0 = I, C_{j+1} = C_j T,
 * xyz_{j+1} = C_{j+1}[:3, 3]; s = sum(gt . pred) / sum(pred . pred); out[i] = sqrt(sum((s pred - gt)^2)) / points.  out = fp64[P].
 * 2 <= track <= DN_POSE_EVAL_MAX_TRACK (the original: 5).
 * Both metric kernels: one thread per snippet / window, fp64 without contraction, every sum in index order, no atomics: two runs are
 * bit-identical.  Every argument is checked before any launch.
 * ------------------------------------------------------------------------------------------------------------ */
#define DN_POSE_EVAL_MAX_L 33
#define DN_POSE_EVAL_MAX_TRACK 64
int dn_snippet_gather(const uint8_t* ring, int32_t R, const int32_t* idx, int32_t N, int32_t K, int32_t H, int32_t W, const float* mean_host,
                      const float* std_host, float* dst, dn_stream_t stream);
int dn_pose_eval_sfm(const float* pose, int32_t rotation_mode, const double* gt, int32_t N, int32_t L, double* out, dn_stream_t stream);
int dn_pose_eval_mono2(const float* pose, const double* Q, int32_t P, int32_t track, double* out, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Velodyne clouds -> sparse depth maps (reference data/kitti_raw_loader.py:243-300), a batch per call.
 * points = fp32[total_points][4], the .bin files back to back as they are (column 3 is ignored and taken as 1.0; 16-byte aligned);
 * pt_off = int64[B + 1] on the device, frame b owns points [pt_off[b], pt_off[b + 1]); M = fp64[B][12] on the device, the frame's 3 x 4
 * P_velo2im (formed on the host); out = fp32[B][h][w], w >= 2.  A point with !(x >= 0) is dropped; per row i of M, in fp64 without
 * contraction, p_i = ((M[i][0] * x + M[i][1] * y) + M[i][2] * z) + M[i][3]; u = p_0 / p_2, v = p_1 / p_2; col = rint(u) - 1,
 * row = rint(v) - 1 (half to even); the point is kept iff col >= 0, row >= 0, col < lim_w, row < lim_h (NaN and inf fail); depth = p_2.
 * 0 < lim_h <= h and 0 < lim_w <= w (the reference tests against img_height / ratio, the map has img_height // ratio rows).
 * Every hit pixel takes the depth of the point with the largest index on it; every key row * (w - 1) + col - 1 (the reference's sub2ind:
 * pixels (r, 0) and (r - 1, w - 1) share one) hit by more than one point then writes the minimum depth of its group at the pixel of the
 * group's lowest-index point; negative values become 0; one fp64 -> fp32 rounding at the store.  Integer atomics only: the result does
 * not depend on scheduling.  workspace: dn_velo_depth_workspace_bytes(B, h, w, total_points) bytes (0 for a bad shape), 8-byte aligned,
 * contents irrelevant.  B <= 65535, total_points < 2^31 - 1.
 * ------------------------------------------------------------------------------------------------------------ */
size_t dn_velo_depth_workspace_bytes(int32_t B, int32_t h, int32_t w, int64_t total_points);
int dn_velo_depth(const float* points, const int64_t* pt_off, int64_t total_points, const double* M, int32_t B, int32_t h, int32_t w,
                  double lim_h, double lim_w, void* workspace, size_t workspace_bytes, float* out, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Attainable-peak probes (SURVEY.md section 8d "Peaks"; used by bench.py only): a float4 streaming copy of n floats
 * (n % 4 == 0, 16-byte aligned; moves 8*n bytes) and a register-resident v_mfma_f32_32x32x2_f32 loop
 * (out: blocks*256 floats; dn_ubench_mfma_f32_flops = the FLOPs one launch executes).
 * ------------------------------------------------------------------------------------------------------------ */
int dn_ubench_copy(const float* src, float* dst, int64_t n, dn_stream_t stream);
int64_t dn_ubench_mfma_f32_flops(int32_t blocks, int32_t iters);
int dn_ubench_mfma_f32(float* out, int32_t blocks, int32_t iters, dn_stream_t stream);
/* store-only probe: n floats (multiple of 1024) written with 16-byte stores; mode 0: 1 KiB contiguous per wave instruction, mode 1: 64-byte
 * segments at a 256-byte stride (the four-instruction pattern of a 64-channel result whose lanes hold 4 channels of one pixel). */
int dn_ubench_store(float* dst, int64_t n, int32_t mode, dn_stream_t stream);
/* Block -> XCD placement probe: out[x + gx*(y + gy*z)] = HW_REG_XCC_ID of block (x, y, z) of a (gx, gy, gz) grid.  The K-split paths
 * (dn_conv_desc.splitk_ws) meet the partial tiles of one output tile in ONE XCD's L2 (no agent-scope fence); that is only correct if
 * all blocks with the same blockIdx.x land on the same XCD when gridDim.x is a multiple of 8 -- observed on MI355X, promised by
 * nobody.  The caller runs this probe once per device before it hands out a split workspace and leaves splitk_ws NULL (no split,
 * same results) if the placement is anything else. */
int dn_xcd_probe(int32_t* out, int32_t gx, int32_t gy, int32_t gz, dn_stream_t stream);
/* Probe (round 5): a reduction finished by the LAST block of a grid, across XCDs, without an agent-scope fence -- records written with
 * agent-scope relaxed atomic stores, an agent-scope counter, records read back with agent-scope relaxed atomic loads by the block that
 * arrives last (mode 0; mode 1 = plain stores / loads, the control).  data: blocks * rec floats, counter: one zeroed int (left zero),
 * result: 3 ints (+= mismatching floats, last block, += 1 per launch).  tools/exp/last_arrival_probe.py. */
int dn_last_arrival_probe(float* data, int32_t* counter, int32_t* result, int32_t blocks, int32_t rec, int32_t round, int32_t mode, dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DISPNET_HIP_H_ */
