// NYU Depth v2 input chain on the device (reference datasets/nyu_depth_v2.py:76-110, datasets/image_utils.py).
//
// Training: per sample the reference takes the stored (5, H0, W0) float32 array (RGB 0..255, depth in metres, 0/1 mask) and runs, in
// numpy on a DataLoader worker: flip -> scipy.ndimage.rotate(order=3, mode='constant') clipped to the sample's min / max over all
// five channels -> random crop -> skimage warp (bilinear zoom by s toward the top-left corner, depth / s) -> colour gain with clip on
// RGB -> ToTensor (no /255) -> float32 -> Normalize.  Here:
//   dn_nyu_prefilter      per-sample min / max partials, then the cubic B-spline prefilter (mirror boundaries) of RGB + depth in
//                         fp64, axis 0 then axis 1 like scipy's spline_filter, with the flip folded into the first pass;
//   dn_nyu_train_resample one block per 16 x 64 output tile: the rotated, fp32-rounded, clipped source window the tile's bilinear
//                         zoom reads is evaluated once into LDS, then each output pixel combines its four neighbours in fp64,
//                         divides depth by s, applies the gain with clip, casts to fp32 and normalises;
// Validation: dn_nyu_val_resize is scipy.ndimage.zoom(order=1) to 320x448, rounded to fp32, then the same Normalize.
//
// Numbers: the geometry and the spline arithmetic follow scipy's and skimage's operation order in fp64 (no contraction: this file
// is compiled with fp-contract off), so the fp32 roundings the reference takes (after the rotate, after the warp chain, after the
// normalisation) see the same fp64 values up to a few ulp of fp64.  The one step left out is the warp's clip to its input range: a
// convex combination of values inside [min, max] leaves it only by fp64 rounding, far below the fp32 cast that follows.
// Per-sample parameters come as double[B][8] = {flip, angle (degrees), crop row, crop column, s, gain, 0, 0}; the host draws them.
#include "dn_internal.h"
#include "dn_spline.h"

#pragma clang fp contract(off)

namespace dn {

constexpr int kNyuThreads = 256;
constexpr int kTileH = 16, kTileW = 64;            // output tile of the train resample
constexpr int kRegH = kTileH + 1, kRegW = kTileW + 1;   // crop-space window a tile reads at s >= 1
constexpr int kRowLines = 8;                       // lines per block of the axis-1 prefilter pass
constexpr int kRowThreads = 64;
constexpr int kMaxRowW = 1024;

// ---- per-sample min / max over all five stored channels: partial[b][chunk] = (min, max)
__global__ void __launch_bounds__(kNyuThreads) nyu_minmax_kernel(const float* __restrict__ raw, long long per_sample, float* __restrict__ partial) {
  const int b = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x;
  const float* p = raw + (long long)b * per_sample;
  const long long lo = per_sample * chunk / nchunk, hi = per_sample * (chunk + 1) / nchunk;
  float mn = INFINITY, mx = -INFINITY;
  for (long long i = lo + threadIdx.x; i < hi; i += kNyuThreads) {
    const float v = p[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  __shared__ float smn[kNyuThreads], smx[kNyuThreads];
  smn[threadIdx.x] = mn;
  smx[threadIdx.x] = mx;
  __syncthreads();
  for (int o = kNyuThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      smn[threadIdx.x] = fminf(smn[threadIdx.x], smn[threadIdx.x + o]);
      smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[((long long)b * nchunk + chunk) * 2 + 0] = smn[0];
    partial[((long long)b * nchunk + chunk) * 2 + 1] = smx[0];
  }
}

// ---- prefilter along axis 0: one thread per (sample, channel 0..3, output column); the flip picks the source column.
// scipy's order per line: gain, mirror causal init, causal pass, anti-causal init, anti-causal pass.
__global__ void __launch_bounds__(kNyuThreads) nyu_prefilter_cols_kernel(const float* __restrict__ raw, const double* __restrict__ params, int B,
                                                                        int H, int W, double* __restrict__ coef) {
  const long long t = blockIdx.x * (long long)kNyuThreads + threadIdx.x;
  if (t >= (long long)B * 4 * W) return;
  const int j = (int)(t % W);
  const int ch = (int)((t / W) % 4), b = (int)(t / (4LL * W));
  const int sj = params[b * 8 + 0] != 0.0 ? W - 1 - j : j;
  const float* src = raw + ((long long)b * 5 + ch) * H * W + sj;
  double* dst = coef + ((long long)b * 4 + ch) * H * W + j;
  spline_prefilter_column(src, dst, H, W);
}

// ---- prefilter along axis 1: kRowLines lines of W doubles staged in LDS (coalesced in and out), one thread per line filters.
__global__ void __launch_bounds__(kRowThreads) nyu_prefilter_rows_kernel(long long lines, int W, double* __restrict__ coef) {
  extern __shared__ double sline[];          // [kRowLines][W]
  const long long l0 = (long long)blockIdx.x * kRowLines;
  const int nl = (int)(lines - l0 < kRowLines ? lines - l0 : kRowLines);
  double* g = coef + l0 * W;
  for (int e = threadIdx.x; e < nl * W; e += kRowThreads) sline[e] = g[e];
  __syncthreads();
  if ((int)threadIdx.x < nl) {
    spline_prefilter_line(sline + threadIdx.x * W, W);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nl * W; e += kRowThreads) g[e] = sline[e];
}

// scipy.ndimage.rotate's order-3 value at source (y, x) of one H x W coefficient plane: 0 outside [0, H-1] x [0, W-1], mirrored taps
static __device__ __forceinline__ double spline_at(const double* __restrict__ c, int H, int W, double y, double x) {
  if (!(y >= 0.0 && y <= (double)(H - 1) && x >= 0.0 && x <= (double)(W - 1))) return 0.0;
  const double fy = floor(y), fx = floor(x);
  double wy[4], wx[4];
  cubic_weights(y - fy, wy);
  cubic_weights(x - fx, wx);
  const int iy = (int)fy, ix = (int)fx;
  int cols[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) cols[j] = mirror_idx(ix - 1 + j, W);
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double* row = c + (long long)mirror_idx(iy - 1 + i, H) * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += row[cols[j]] * wy[i] * wx[j];
  }
  return acc;
}

__global__ void __launch_bounds__(kNyuThreads) nyu_train_resample_kernel(const double* __restrict__ coef, const float* __restrict__ minmax, int nchunk,
                                                                        const double* __restrict__ params, int H, int W, int OH, int OW,
                                                                        float m0, float m1, float m2, float s0, float s1, float s2,
                                                                        float* __restrict__ img, float* __restrict__ depth) {
  __shared__ float win[4][kRegH][kRegW];
  const int b = blockIdx.z;
  const int rt0 = blockIdx.y * kTileH, ct0 = blockIdx.x * kTileW;
  const double* pp = params + b * 8;
  const double angle = pp[1], crop_r = pp[2], crop_c = pp[3], s = pp[4], mult = pp[5];
  // scipy.ndimage.rotate: rot = [[c, s], [-s, c]], offset = in_center - rot @ out_center (numpy's deg2rad = x * (pi / 180))
  const double th = angle * (M_PI / 180.0);
  const double cs = cos(th), sn = sin(th);
  const double cy = (H - 1) / 2.0, cx = (W - 1) / 2.0;
  const double off0 = cy - (cs * cy + sn * cx), off1 = cx - (-sn * cy + cs * cx);
  const double inv = 1.0 / s;                        // skimage: the inverse matrix's entry, coordinates = index * inv
  float mi = INFINITY, ma = -INFINITY;
  for (int k = 0; k < nchunk; ++k) {
    mi = fminf(mi, minmax[(b * nchunk + k) * 2 + 0]);
    ma = fmaxf(ma, minmax[(b * nchunk + k) * 2 + 1]);
  }
  // crop-space window of this tile (monotone in the output index); clamped to the LDS window and to the crop
  const int rlast = min(rt0 + kTileH, OH) - 1, clast = min(ct0 + kTileW, OW) - 1;
  const int wr0 = max(0, (int)floor(rt0 * inv)), wc0 = max(0, (int)floor(ct0 * inv));
  const int wr1 = min(min(OH - 1, (int)ceil(rlast * inv)), wr0 + kRegH - 1);
  const int wc1 = min(min(OW - 1, (int)ceil(clast * inv)), wc0 + kRegW - 1);
  const int nr = max(0, wr1 - wr0 + 1), nc = max(0, wc1 - wc0 + 1);
  const long long plane = (long long)H * W;
  for (int e = threadIdx.x; e < 4 * nr * nc; e += kNyuThreads) {
    const int ch = e / (nr * nc), rem = e % (nr * nc);
    const int i = rem / nc, j = rem % nc;
    const double R = (double)(wr0 + i) + crop_r, C = (double)(wc0 + j) + crop_c;   // position in the rotated (full) image
    double y = 0.0;
    y += R * cs;
    y += C * sn;
    y += off0;
    double x = 0.0;
    x += R * -sn;
    x += C * cs;
    x += off1;
    const float v = (float)spline_at(coef + ((long long)b * 4 + ch) * plane, H, W, y, x);
    win[ch][i][j] = fminf(fmaxf(v, mi), ma);                                      // np.clip(rotated, mi, ma) in fp32
  }
  __syncthreads();
  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
  for (int e = threadIdx.x; e < kTileH * kTileW; e += kNyuThreads) {
    const int r = rt0 + e / kTileW, c = ct0 + e % kTileW;
    if (r >= OH || c >= OW) continue;
    const double rr = r * inv, cc = c * inv;
    const double fr = floor(rr), fc = floor(cc), ur = ceil(rr), uc = ceil(cc);
    const double dr = rr - fr, dc = cc - fc;
    const int ir[2] = {(int)fr, (int)ur}, ic[2] = {(int)fc, (int)uc};
    const long long o = (long long)r * OW + c;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      double v[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int li = ir[a] - wr0, lj = ic[q] - wc0;
          const bool in = ir[a] >= 0 && ir[a] < OH && ic[q] >= 0 && ic[q] < OW && li >= 0 && li < nr && lj >= 0 && lj < nc;
          v[a][q] = in ? (double)win[ch][li][lj] : 0.0;
        }
      const double top = (1.0 - dc) * v[0][0] + dc * v[0][1];
      const double bottom = (1.0 - dc) * v[1][0] + dc * v[1][1];
      const double w = (1.0 - dr) * top + dr * bottom;
      if (ch == 3) {
        depth[(long long)b * OH * OW + o] = (float)(w / s);
      } else {
        const double g = fmin(fmax(w * mult, 0.0), 255.0);
        img[((long long)b * 3 + ch) * OH * OW + o] = __fdiv_rn((float)g - mean[ch], stdv[ch]);
      }
    }
  }
}

// scipy.ndimage.zoom(order=1, grid_mode=False) of [B,3,IH,IW] fp32 to [B,3,OH,OW]: output i reads i * ((IH-1)/(OH-1)), weights
// (1 - f, 1 - (1 - f)), taps summed row-major, rounded to fp32; then Normalize
__global__ void __launch_bounds__(kNyuThreads) nyu_val_resize_kernel(const float* __restrict__ src, int B, int IH, int IW, int OH, int OW,
                                                                    float m0, float m1, float m2, float s0, float s1, float s2,
                                                                    float* __restrict__ dst) {
  const long long total = (long long)B * 3 * OH * OW;
  const double zy = (double)(IH - 1) / (double)(OH - 1), zx = (double)(IW - 1) / (double)(OW - 1);
  for (long long t = blockIdx.x * (long long)kNyuThreads + threadIdx.x; t < total; t += (long long)gridDim.x * kNyuThreads) {
    const int j = (int)(t % OW);
    const long long rest = t / OW;
    const int i = (int)(rest % OH);
    const long long bc = rest / OH;
    const int c = (int)(bc % 3);
    const double y = fmin(i * zy, (double)(IH - 1)), x = fmin(j * zx, (double)(IW - 1));
    const int y0 = (int)floor(y), x0 = (int)floor(x);
    const int y1 = min(y0 + 1, IH - 1), x1 = min(x0 + 1, IW - 1);
    const double wy0 = 1.0 - (y - y0), wx0 = 1.0 - (x - x0);
    const double wy1 = 1.0 - wy0, wx1 = 1.0 - wx0;
    const float* p = src + bc * IH * IW;
    double acc = (double)p[(long long)y0 * IW + x0] * wy0 * wx0;
    acc += (double)p[(long long)y0 * IW + x1] * wy0 * wx1;
    acc += (double)p[(long long)y1 * IW + x0] * wy1 * wx0;
    acc += (double)p[(long long)y1 * IW + x1] * wy1 * wx1;
    const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
    dst[t] = __fdiv_rn((float)acc - mean, sd);
  }
}

static inline int nyu_blocks(long long n) {
  long long b = (n + kNyuThreads - 1) / kNyuThreads;
  const long long cap = 256 * 16;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace dn

using namespace dn;

extern "C" {

int dn_nyu_prefilter(const float* raw, const double* params, int32_t B, int32_t H0, int32_t W0, double* coef, float* minmax, dn_stream_t stream) {
  DN_REQUIRE(raw && params && coef && minmax && B > 0 && H0 >= 3 && W0 >= 3, DN_ERR_BAD_ARG, "dn_nyu_prefilter: bad argument");
  DN_REQUIRE(W0 <= kMaxRowW, DN_ERR_UNSUPPORTED, "dn_nyu_prefilter: W0 = %d exceeds %d", (int)W0, kMaxRowW);
  hipStream_t s = as_stream(stream);
  DN_LAUNCH(nyu_minmax_kernel, dim3(DN_NYU_MINMAX_CHUNKS, B), dim3(kNyuThreads), 0, s, raw, 5LL * H0 * W0, minmax);
  int rc = check_launch("nyu_minmax_kernel");
  if (rc) return rc;
  DN_LAUNCH(nyu_prefilter_cols_kernel, dim3((unsigned)((4LL * B * W0 + kNyuThreads - 1) / kNyuThreads)), dim3(kNyuThreads), 0, s, raw, params, B,
            H0, W0, coef);
  rc = check_launch("nyu_prefilter_cols_kernel");
  if (rc) return rc;
  const long long lines = 4LL * B * H0;
  DN_LAUNCH(nyu_prefilter_rows_kernel, dim3((unsigned)((lines + kRowLines - 1) / kRowLines)), dim3(kRowThreads),
            (size_t)kRowLines * W0 * sizeof(double), s, lines, W0, coef);
  return check_launch("nyu_prefilter_rows_kernel");
}

int dn_nyu_train_resample(const double* coef, const float* minmax, const double* params, int32_t B, int32_t H0, int32_t W0, int32_t OH,
                          int32_t OW, const float* mean_host, const float* std_host, float* img, float* depth, dn_stream_t stream) {
  DN_REQUIRE(coef && minmax && params && mean_host && std_host && img && depth && B > 0 && H0 >= 3 && W0 >= 3 && OH > 0 && OW > 0 &&
                 OH <= H0 && OW <= W0,
             DN_ERR_BAD_ARG, "dn_nyu_train_resample: bad argument");
  dim3 grid((unsigned)((OW + kTileW - 1) / kTileW), (unsigned)((OH + kTileH - 1) / kTileH), (unsigned)B);
  DN_LAUNCH(nyu_train_resample_kernel, grid, dim3(kNyuThreads), 0, as_stream(stream), coef, minmax, (int)DN_NYU_MINMAX_CHUNKS, params, (int)H0,
            (int)W0, (int)OH, (int)OW, mean_host[0], mean_host[1], mean_host[2], std_host[0], std_host[1], std_host[2], img, depth);
  return check_launch("nyu_train_resample_kernel");
}

int dn_nyu_val_resize(const float* src, int32_t B, int32_t IH, int32_t IW, int32_t OH, int32_t OW, const float* mean_host, const float* std_host,
                      float* dst, dn_stream_t stream) {
  DN_REQUIRE(src && dst && mean_host && std_host && B > 0 && IH >= 2 && IW >= 2 && OH >= 2 && OW >= 2, DN_ERR_BAD_ARG,
             "dn_nyu_val_resize: bad argument");
  DN_LAUNCH(nyu_val_resize_kernel, dim3(nyu_blocks((long long)B * 3 * OH * OW)), dim3(kNyuThreads), 0, as_stream(stream), src, (int)B, (int)IH,
            (int)IW, (int)OH, (int)OW, mean_host[0], mean_host[1], mean_host[2], std_host[0], std_host[1], std_host[2], dst);
  return check_launch("nyu_val_resize_kernel");
}

}  // extern "C"
