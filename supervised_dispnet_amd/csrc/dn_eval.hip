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
constexpr int kErrThreads = 1024;

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

// ---- errors
// f(i) for every i < n with m[i] != 0: the aligned middle of the mask is read four bytes at a time.  The order in which one thread
// meets its pixels is fixed, so the sums are reproducible.
template <typename F>
static __device__ __forceinline__ void for_each_masked(const uint8_t* __restrict__ m, int n, F f) {
  const int tid = threadIdx.x;
  const int head = min(n, (int)((4 - (reinterpret_cast<uintptr_t>(m) & 3)) & 3));
  if (tid < head && m[tid]) f(tid);
  const int nwords = (n - head) / 4;
  const uint32_t* mw = reinterpret_cast<const uint32_t*>(m + head);
  for (int wi = tid; wi < nwords; wi += kErrThreads) {
    const uint32_t v = mw[wi];
    if (v == 0) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((v >> (8 * k)) & 255u) f(head + 4 * wi + k);
  }
  const int i = head + 4 * nwords + tid;
  if (i < n && m[i]) f(i);
}

// sum over the block in a fixed tree order; every thread returns the total
template <typename T>
static __device__ __forceinline__ T block_total(T v, T* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kErrThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(kErrThreads) eval_errors_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                                  const uint8_t* __restrict__ mask, const long long* __restrict__ off,
                                                                  const int* __restrict__ npix, int scale_mode, float fixed_scale,
                                                                  float* __restrict__ out) {
  __shared__ double red[kErrThreads];
  __shared__ unsigned hist[2][256];
  __shared__ unsigned s_prefix[2], s_rank[2], s_more[2], s_next[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* g = gt + off[b];
  const float* p = pred + off[b];
  const uint8_t* m = mask + off[b];
  const int n = npix[b];
  float scale = 1.f;
  if (scale_mode == 1) scale = fixed_scale;
  if (scale_mode == 2) {
    // np.median of both arrays: the element of rank (cnt-1)/2 by a 4-pass radix select on the bit patterns (positive values order
    // like their bits), gt in histogram 0 and pred in histogram 1 of the same sweep; for an even count also the next element up
    unsigned prefix[2] = {0, 0}, cnt = 0;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      for (int k = tid; k < 512; k += kErrThreads) hist[k >> 8][k & 255] = 0;
      __syncthreads();
      // a thread's consecutive values mostly share a bucket (all depths share the first byte): count the run, add it once
      unsigned last[2] = {0, 0}, run[2] = {0, 0};
      for_each_masked(m, n, [&](int i) {
        const unsigned bits[2] = {__float_as_uint(g[i]), __float_as_uint(p[i])};
#pragma unroll
        for (int a = 0; a < 2; ++a)
          if (pass == 0 || (bits[a] >> (shift + 8)) == (prefix[a] >> (shift + 8))) {
            const unsigned k = (bits[a] >> shift) & 255u;
            if (k != last[a] && run[a]) {
              atomicAdd(&hist[a][last[a]], run[a]);
              run[a] = 0;
            }
            last[a] = k;
            ++run[a];
          }
      });
#pragma unroll
      for (int a = 0; a < 2; ++a)
        if (run[a]) atomicAdd(&hist[a][last[a]], run[a]);
      __syncthreads();
      if (tid < 2) {
        unsigned r = s_rank[tid];
        if (pass == 0) {
          unsigned c = 0;
          for (int k = 0; k < 256; ++k) c += hist[tid][k];
          r = c > 0 ? (c - 1) / 2 : 0;
          s_next[tid] = c;                      // the count, until the last pass
        }
        unsigned k = 0;
        for (; k < 255; ++k) {
          if (r < hist[tid][k]) break;
          r -= hist[tid][k];
        }
        s_prefix[tid] = prefix[tid] | (k << shift);
        s_rank[tid] = r;
        s_more[tid] = r + 1 < hist[tid][k];     // after the last pass: another copy of the selected value sits above its rank
      }
      __syncthreads();
      prefix[0] = s_prefix[0];
      prefix[1] = s_prefix[1];
      cnt = s_next[0];
      __syncthreads();
    }
    float med[2] = {__uint_as_float(prefix[0]), __uint_as_float(prefix[1])};
    if (cnt > 0 && cnt % 2 == 0) {
      if (tid < 2) s_next[tid] = 0xFFFFFFFFu;
      __syncthreads();
      unsigned mn[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
      for_each_masked(m, n, [&](int i) {
        const unsigned bg = __float_as_uint(g[i]), bp = __float_as_uint(p[i]);
        if (bg > prefix[0]) mn[0] = min(mn[0], bg);
        if (bp > prefix[1]) mn[1] = min(mn[1], bp);
      });
      atomicMin(&s_next[0], mn[0]);
      atomicMin(&s_next[1], mn[1]);
      __syncthreads();
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const float up = s_more[a] ? med[a] : __uint_as_float(s_next[a]);
        med[a] = __fdiv_rn(__fadd_rn(med[a], up), 2.f);   // numpy: the fp32 mean of the two middle elements
      }
    }
    scale = cnt > 0 ? __fdiv_rn(med[0], med[1]) : __uint_as_float(0x7FC00000u);
  }
  double s_abs = 0.0, s_sq_rel = 0.0, s_sq = 0.0, s_log = 0.0;
  unsigned c1 = 0, c2 = 0, c3 = 0, cn = 0;
  for_each_masked(m, n, [&](int i) {
    const float gv = g[i], pv = __fmul_rn(p[i], scale);
    const float thr = fmaxf(__fdiv_rn(gv, pv), __fdiv_rn(pv, gv));
    c1 += thr < 1.25f;
    c2 += thr < 1.5625f;
    c3 += thr < 1.953125f;
    ++cn;
    const double gd = (double)gv, pd = (double)pv;
    const double d = gd - pd, dl = log(gd) - log(pd);
    s_abs += fabs(d) / gd;
    s_sq_rel += d * d / gd;
    s_sq += d * d;
    s_log += dl * dl;
  });
  unsigned* ured = reinterpret_cast<unsigned*>(red);
  const double count = (double)block_total(cn, ured);
  const double r[7] = {block_total(s_abs, red) / count,
                       block_total(s_sq_rel, red) / count,
                       sqrt(block_total(s_sq, red) / count),
                       sqrt(block_total(s_log, red) / count),
                       (double)block_total(c1, ured) / count,
                       (double)block_total(c2, ured) / count,
                       (double)block_total(c3, ured) / count};   // 0 / 0 = NaN for an empty mask, like numpy's mean of nothing
  if (tid < 7) out[b * 8 + tid] = (float)r[tid];
  if (tid == 7) out[b * 8 + 7] = scale;
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
