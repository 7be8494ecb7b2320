// Evaluation chain on the device (reference test_disp.py:391-398 and :453-469): everything between the network's depth map and the
// seven error numbers of one image.
//   dn_eval_normalize   (x [/ 255] - mean) / std of frames that arrive as fp32 (uint8 frames take dn_u8_normalize_flip);
//   dn_zoom3_prefilter  cubic B-spline coefficients (mirror boundaries, fp64) of the network-resolution depth [B,h,w], axis 0 then
//                       axis 1 like scipy's spline_filter: the recurrences of the NYU prefilter (dn_nyu.hip) on one plane per image;
//   dn_zoom3_clip       scipy.ndimage.zoom(order=3, mode='constant', grid_mode=False) to a per-image target size, then .clip(lo, hi):
//                       one block per 16 x 64 output tile, the coefficient window the tile reads staged in LDS, the four row / column
//                       weights computed once per output row / column, 16 taps summed in fp64 row-major as coef * (wrow * wcol),
//                       one rounding to fp32, fp32 clip.  A source coordinate outside [0, n-1] gives exactly 0 (scipy does: for
//                       128 -> 375 rows the product 374 * (127/374) rounds above 127 and the whole last row is 0, then lo);
//   dn_eval_errors      one block per image over the pixels with mask != 0: numpy's median of gt and of pred by an exact radix select
//                       on the bit patterns (both arrays per sweep), scale = fp32 ratio, pred * scale rounded to fp32, thresholds
//                       from IEEE fp32 divisions, the four means from fp64 terms and fp64 sums in a fixed order.
// Ragged layout: image b occupies npix[b] = H_b * W_b elements at element offset off[b] of gt / pred / mask.
#include "dn_internal.h"
#include "dn_eval_errors.h"
#include "dn_spline.h"

#pragma clang fp contract(off)

namespace dn {

constexpr int kColThreads = 256;
constexpr int kLineThreads = 64;
constexpr int kMaxLines = 8;                        // lines per block of the axis-1 pass (fewer where 8 lines exceed kLineLdsBytes)
constexpr int kLineLdsBytes = 64 * 1024;
constexpr int kZoomMaxW = 2048;
constexpr int kZoomThreads = 256;
constexpr int kZTileH = 16, kZTileW = 64;           // output tile of the zoom
constexpr int kWinH = kZTileH + 4, kWinW = kZTileW + 4;   // coefficient window of a tile at ratios <= 1 (15 + 4 rows, 63 + 4 columns)

// ---- the input normalisation of frames that arrive as fp32 (not resized, or NYU, which the reference does not divide by 255):
// dst = ((div255 ? x / 255 : x) - mean[c]) / std[c] over [B,3,HW], IEEE fp32 in that order (test_disp.py:203-218)
__global__ void __launch_bounds__(kColThreads) eval_normalize_kernel(const float* __restrict__ src, long long total, long long HW, int div255,
                                                                    float m0, float m1, float m2, float s0, float s1, float s2,
                                                                    float* __restrict__ dst) {
  for (long long t = blockIdx.x * (long long)kColThreads + threadIdx.x; t < total; t += (long long)gridDim.x * kColThreads) {
    const int c = (int)((t / HW) % 3);
    float v = src[t];
    if (div255) v = __fdiv_rn(v, 255.f);
    const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
    dst[t] = __fdiv_rn(__fsub_rn(v, mean), sd);
  }
}

// ---- prefilter along axis 0: one thread per (image, column); the recurrences are dn_spline.h's, shared with the NYU chain
__global__ void __launch_bounds__(kColThreads) zoom3_prefilter_cols_kernel(const float* __restrict__ pred, int B, int H, int W,
                                                                          double* __restrict__ coef) {
  const long long t = blockIdx.x * (long long)kColThreads + threadIdx.x;
  if (t >= (long long)B * W) return;
  const int j = (int)(t % W), b = (int)(t / W);
  const float* src = pred + (long long)b * H * W + j;
  double* dst = coef + (long long)b * H * W + j;
  spline_prefilter_column(src, dst, H, W);
}

// ---- prefilter along axis 1: nlines lines of W doubles staged in LDS (coalesced in and out), one thread per line filters.
__global__ void __launch_bounds__(kLineThreads) zoom3_prefilter_rows_kernel(long long lines, int nlines, int W, double* __restrict__ coef) {
  extern __shared__ double sline[];          // [nlines][W]
  const long long l0 = (long long)blockIdx.x * nlines;
  const int nl = (int)(lines - l0 < nlines ? lines - l0 : nlines);
  double* g = coef + l0 * W;
  for (int e = threadIdx.x; e < nl * W; e += kLineThreads) sline[e] = g[e];
  __syncthreads();
  if ((int)threadIdx.x < nl) {
    spline_prefilter_line(sline + threadIdx.x * W, W);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nl * W; e += kLineThreads) g[e] = sline[e];
}

// one output index of one axis: source coordinate o * ((n-1)/(O-1)), its floor (or -1: outside [0, n-1], the output is 0) and weights
static __device__ __forceinline__ int axis_tap(int o, int n, int O, double* w) {
  const double x = O > 1 ? (double)o * ((double)(n - 1) / (double)(O - 1)) : 0.0;
  if (!(x >= 0.0 && x <= (double)(n - 1))) return -1;
  const double f = floor(x);
  cubic_weights(x - f, w);
  return (int)f;
}

__global__ void __launch_bounds__(kZoomThreads) zoom3_clip_kernel(const double* __restrict__ coef, int h, int w, const int* __restrict__ out_hw,
                                                                  const long long* __restrict__ out_off, float lo, float hi,
                                                                  float* __restrict__ out) {
  __shared__ double wy[kZTileH][4], wx[kZTileW][4];
  __shared__ int fy[kZTileH], fx[kZTileW];
  __shared__ double win[kWinH][kWinW];
  const int b = blockIdx.z;
  const int H = out_hw[2 * b], W = out_hw[2 * b + 1];
  const int r0 = blockIdx.y * kZTileH, c0 = blockIdx.x * kZTileW;
  if (r0 >= H || c0 >= W) return;                        // the grid covers the largest image of the batch
  const int tid = threadIdx.x;
  const int nrow = min(kZTileH, H - r0), ncol = min(kZTileW, W - c0);
  if (tid < nrow) fy[tid] = axis_tap(r0 + tid, h, H, wy[tid]);
  if (tid >= 64 && tid - 64 < ncol) fx[tid - 64] = axis_tap(c0 + tid - 64, w, W, wx[tid - 64]);
  __syncthreads();
  // the window of coefficient rows / columns the tile's valid outputs read (floors are monotone in the output index), before mirroring
  int ly = nrow - 1, lx = ncol - 1;
  while (ly >= 0 && fy[ly] < 0) --ly;
  while (lx >= 0 && fx[lx] < 0) --lx;
  const bool any = ly >= 0 && lx >= 0;
  const int wr0 = any ? fy[0] - 1 : 0, wc0 = any ? fx[0] - 1 : 0;
  const int nr = any ? fy[ly] + 2 - wr0 + 1 : 0, nc = any ? fx[lx] + 2 - wc0 + 1 : 0;
  const bool staged = nr <= kWinH && nc <= kWinW;        // always at ratios <= 1; a shrinking zoom reads global memory instead
  const double* cp = coef + (long long)b * h * w;
  if (staged) {
    for (int e = tid; e < nr * nc; e += kZoomThreads) {
      const int i = e / nc, j = e % nc;
      win[i][j] = cp[(long long)mirror_idx(wr0 + i, h) * w + mirror_idx(wc0 + j, w)];
    }
    __syncthreads();
  }
  float* op = out + out_off[b];
  const int cc = tid % kZTileW;
  for (int rr = tid / kZTileW; rr < nrow; rr += kZoomThreads / kZTileW) {
    if (cc >= ncol) break;
    float v = 0.f;
    const int iy = fy[rr], ix = fx[cc];
    if (iy >= 0 && ix >= 0) {
      double acc = 0.0;
      if (staged) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc += win[iy - 1 + i - wr0][ix - 1 + j - wc0] * (wy[rr][i] * wx[cc][j]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double* row = cp + (long long)mirror_idx(iy - 1 + i, h) * w;
#pragma unroll
          for (int j = 0; j < 4; ++j) acc += row[mirror_idx(ix - 1 + j, w)] * (wy[rr][i] * wx[cc][j]);
        }
      }
      v = (float)acc;
    }
    op[(long long)(r0 + rr) * W + c0 + cc] = fminf(fmaxf(v, lo), hi);
  }
}

// ---- errors: the selection and the sums are dn_eval_errors.h's, shared with monodepth2's chain (dn_eval_mono2.hip)
__global__ void __launch_bounds__(kErrThreads) eval_errors_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                                  const uint8_t* __restrict__ mask, const long long* __restrict__ off,
                                                                  const int* __restrict__ npix, int scale_mode, float fixed_scale,
                                                                  float* __restrict__ out) {
  eval_errors_image<false>(gt, pred, mask, off, npix, scale_mode, fixed_scale, 0.f, 0.f, out);
}

}  // namespace dn

using namespace dn;

extern "C" {

int dn_eval_normalize(const float* src, int32_t B, int64_t HW, int32_t div255, const float* mean_host, const float* std_host, float* dst,
                      dn_stream_t stream) {
  DN_REQUIRE(src && dst && mean_host && std_host && B > 0 && HW > 0, DN_ERR_BAD_ARG, "dn_eval_normalize: bad argument");
  const long long total = 3LL * B * HW;
  long long blocks = (total + kColThreads - 1) / kColThreads;
  if (blocks > 4096) blocks = 4096;
  DN_LAUNCH(eval_normalize_kernel, dim3((unsigned)blocks), dim3(kColThreads), 0, as_stream(stream), src, total, (long long)HW, (int)div255,
            mean_host[0], mean_host[1], mean_host[2], std_host[0], std_host[1], std_host[2], dst);
  return check_launch("eval_normalize_kernel");
}

int dn_zoom3_prefilter(const float* pred, int32_t B, int32_t h, int32_t w, double* coef, dn_stream_t stream) {
  DN_REQUIRE(pred && coef && B > 0 && h >= 3 && w >= 3, DN_ERR_BAD_ARG, "dn_zoom3_prefilter: bad argument");
  DN_REQUIRE(w <= kZoomMaxW, DN_ERR_UNSUPPORTED, "dn_zoom3_prefilter: w = %d exceeds %d", (int)w, kZoomMaxW);
  hipStream_t s = as_stream(stream);
  DN_LAUNCH(zoom3_prefilter_cols_kernel, dim3((unsigned)(((long long)B * w + kColThreads - 1) / kColThreads)), dim3(kColThreads), 0, s, pred,
            (int)B, (int)h, (int)w, coef);
  int rc = check_launch("zoom3_prefilter_cols_kernel");
  if (rc) return rc;
  const long long lines = (long long)B * h;
  const int fit = kLineLdsBytes / (int)(w * sizeof(double));
  const int nlines = fit < kMaxLines ? fit : kMaxLines;            // >= 4 at w <= 2048
  DN_LAUNCH(zoom3_prefilter_rows_kernel, dim3((unsigned)((lines + nlines - 1) / nlines)), dim3(kLineThreads), (size_t)nlines * w * sizeof(double),
            s, lines, nlines, (int)w, coef);
  return check_launch("zoom3_prefilter_rows_kernel");
}

int dn_zoom3_clip(const double* coef, int32_t B, int32_t h, int32_t w, const int32_t* out_hw, const int64_t* out_off, int32_t max_h,
                  int32_t max_w, float lo, float hi, float* out, dn_stream_t stream) {
  DN_REQUIRE(coef && out_hw && out_off && out && B > 0 && B <= 65535 && h >= 3 && w >= 3 && max_h > 0 && max_w > 0, DN_ERR_BAD_ARG,
             "dn_zoom3_clip: bad argument");
  dim3 grid((unsigned)((max_w + kZTileW - 1) / kZTileW), (unsigned)((max_h + kZTileH - 1) / kZTileH), (unsigned)B);
  DN_REQUIRE(grid.y <= 65535, DN_ERR_UNSUPPORTED, "dn_zoom3_clip: max_h = %d is too large", (int)max_h);
  DN_LAUNCH(zoom3_clip_kernel, grid, dim3(kZoomThreads), 0, as_stream(stream), coef, (int)h, (int)w, (const int*)out_hw,
            (const long long*)out_off, lo, hi, out);
  return check_launch("zoom3_clip_kernel");
}

int dn_eval_errors(const float* gt, const float* pred, const uint8_t* mask, const int64_t* off, const int32_t* npix, int32_t B,
                   int32_t scale_mode, float fixed_scale, float* out, dn_stream_t stream) {
  DN_REQUIRE(gt && pred && mask && off && npix && out && B > 0, DN_ERR_BAD_ARG, "dn_eval_errors: bad argument");
  DN_REQUIRE(scale_mode >= 0 && scale_mode <= 2, DN_ERR_BAD_ARG, "dn_eval_errors: bad scale_mode %d", (int)scale_mode);
  DN_LAUNCH(eval_errors_kernel, dim3((unsigned)B), dim3(kErrThreads), 0, as_stream(stream), gt, pred, mask, (const long long*)off,
            (const int*)npix, (int)scale_mode, fixed_scale, out);
  return check_launch("eval_errors_kernel");
}

}  // extern "C"
