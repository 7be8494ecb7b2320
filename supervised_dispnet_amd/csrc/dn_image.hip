// Image arithmetic around the network for run_inference.py and eval_disp.py --device-resize: what the reference
// does per image in numpy / PIL on the host, as integer and fixed fp32 arithmetic on the device -- the target is equality, not a tolerance.
//   dn_imresize_u8   scipy.misc.imresize(frame, (h, w)) of a ragged batch of RGB uint8 frames (reference run_inference.py:124-125,
//                    test_disp.py:193-194): byte-scale by the frame's own min / max (a 256-entry table per frame), Pillow's 8-bit
//                    bilinear resize -- horizontal pass into a uint8 intermediate, then the vertical pass, 22-bit fixed-point
//                    coefficients the host hands over --, then optionally (x / 255 - mean) / std into the NCHW batch.  One block per
//                    8 x 64 output tile: the horizontal pass covers the source rows the tile's vertical taps read and writes bytes into
//                    LDS, the vertical pass reads LDS.  A frame that already is h x w passes through untouched.
//   dn_resize_u8     the same two passes without the byte-scale: PIL's Image.resize((w, h), BILINEAR), which is what imresize does to a
//                    frame that is uint8 already (kitti_raw_loader.py:224).
//   dn_colorize_u8   utils.tensor2array of the reference (:45-76) times 255: crop, [1 / x], max, byte-scale, colour table or grey.
//   dn_contrast_u8   PIL.ImageEnhance.Contrast(im).enhance(f): blend with the rounded mean of the image's luma.
// The per-image reductions (min / max, max, luma sum) are two launches: DN_IMAGE_CHUNKS partials per image written by a first kernel and
// folded by every block of the second (the nyu_minmax_kernel pattern) -- integer or max reductions, so the result has no order.
#include "dn_internal.h"

#pragma clang fp contract(off)

namespace dn {

constexpr int kImgThreads = 256;
constexpr int kRTileH = 8, kRTileW = 64;                 // output tile of the resize
constexpr int kRMaxTaps = DN_IMRESIZE_MAX_TAPS;
constexpr int kRTabRow = 2 + kRMaxTaps + 1;              // {first input, taps, k[taps]} per output index; odd stride: no LDS bank conflicts
constexpr int kRMaxRows = 64;                            // intermediate rows staged at once (>= kRMaxTaps: one output row always fits)
constexpr int kPrecBits = 22;                            // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)

static __device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ---- min / max of every frame that will be resized: DN_IMAGE_CHUNKS partial (min, max) pairs per frame over all three channels
__global__ void __launch_bounds__(kImgThreads) image_minmax_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ hw,
                                                                   const long long* __restrict__ off, int h, int w, int* __restrict__ partial) {
  __shared__ int smn[kImgThreads], smx[kImgThreads];
  const int b = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x, tid = threadIdx.x;
  const int H = hw[2 * b], W = hw[2 * b + 1];
  if (H == h && W == w) return;                          // passed through: no byte-scale
  const long long n = 3LL * H * W;
  const long long lo = n * chunk / nchunk, hi = n * (chunk + 1) / nchunk;
  const uint8_t* p = frames + off[b] + lo;
  const long long len = hi - lo;
  int mn = 255, mx = 0;
  const int head = (int)min(len, (long long)((4 - (reinterpret_cast<uintptr_t>(p) & 3)) & 3));
  if (tid < head) mn = mx = p[tid];
  const long long nwords = (len - head) / 4;
  const uint32_t* pw = reinterpret_cast<const uint32_t*>(p + head);
  for (long long i = tid; i < nwords; i += kImgThreads) {
    const uint32_t v = pw[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int a = (int)((v >> (8 * k)) & 255u);
      mn = min(mn, a);
      mx = max(mx, a);
    }
  }
  const long long t = head + 4 * nwords + tid;
  if (t < len) {
    const int a = p[t];
    mn = min(mn, a);
    mx = max(mx, a);
  }
  smn[tid] = mn;
  smx[tid] = mx;
  __syncthreads();
  for (int o = kImgThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      smn[tid] = min(smn[tid], smn[tid + o]);
      smx[tid] = max(smx[tid], smx[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    partial[(b * nchunk + chunk) * 2 + 0] = smn[0];
    partial[(b * nchunk + chunk) * 2 + 1] = smx[0];
  }
}

// ---- byte-scale + Pillow bilinear resize + normalise, one 8 x 64 output tile per block
__global__ void __launch_bounds__(kImgThreads) imresize_u8_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ hw,
                                                                  const long long* __restrict__ off, const int* __restrict__ tabs,
                                                                  const int* __restrict__ tab_idx, const int* __restrict__ minmax, int h, int w,
                                                                  uint8_t* __restrict__ out_u8, float* __restrict__ out_f32, float m0, float m1,
                                                                  float m2, float s0, float s1, float s2) {
  __shared__ int xt[kRTileW][kRTabRow];
  __shared__ int yt[kRTileH][kRTabRow];
  __shared__ int smm[DN_IMAGE_CHUNKS][2];
  __shared__ uint8_t lut[256];
  __shared__ uint8_t inter[kRMaxRows][kRTileW * 3];
  __shared__ uint8_t otile[kRTileH][kRTileW * 3];
  const int b = blockIdx.z, tid = threadIdx.x;
  const int r0 = blockIdx.y * kRTileH, c0 = blockIdx.x * kRTileW;
  const int H = hw[2 * b], W = hw[2 * b + 1];
  const int xoff = tab_idx[4 * b], xT = tab_idx[4 * b + 1], yoff = tab_idx[4 * b + 2], yT = tab_idx[4 * b + 3];
  if (r0 >= h || c0 >= w || H <= 0 || W <= 0 || xT < 0 || yT < 0 || xT > kRMaxTaps || yT > kRMaxTaps) return;
  const bool hskip = W == w, vskip = H == h;
  const int nrow = min(kRTileH, h - r0), ncol = min(kRTileW, w - c0);
  const uint8_t* f = frames + off[b];

  // the frame's byte-scale as a table: uint8(clip(fp32((fp32(a) - cmin) * fp32(255.0 / (cmax - cmin))) + 0.5f, 0, 255)); identity when
  // the frame is passed through, and for dn_resize_u8 (minmax == nullptr: no stretch)
  if (minmax != nullptr && !(hskip && vskip)) {
    if (tid < DN_IMAGE_CHUNKS * 2) smm[tid >> 1][tid & 1] = minmax[b * DN_IMAGE_CHUNKS * 2 + tid];
    __syncthreads();
    int cmin = 255, cmax = 0;
    for (int k = 0; k < DN_IMAGE_CHUNKS; ++k) {
      cmin = min(cmin, smm[k][0]);
      cmax = max(cmax, smm[k][1]);
    }
    const float scale = (float)(cmax > cmin ? 255.0 / (double)(cmax - cmin) : 1.0);
    const float t = __fadd_rn(__fmul_rn(__fsub_rn((float)tid, (float)cmin), scale), 0.5f);
    lut[tid] = (uint8_t)fminf(fmaxf(t, 0.f), 255.f);
  } else {
    lut[tid] = (uint8_t)tid;
  }
  if (!hskip) {
    const int rowlen = 2 + xT;
    for (int e = tid; e < ncol * rowlen; e += kImgThreads) xt[e / rowlen][e % rowlen] = tabs[xoff + (long long)c0 * rowlen + e];
  }
  if (!vskip) {
    const int rowlen = 2 + yT;
    for (int e = tid; e < nrow * rowlen; e += kImgThreads) yt[e / rowlen][e % rowlen] = tabs[yoff + (long long)r0 * rowlen + e];
  }
  __syncthreads();

  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
  // output rows [g0, g1) of the tile whose source rows fit the staged intermediate (one group unless the frame shrinks > 7x)
  for (int g0 = 0; g0 < nrow;) {
    const int ry0 = vskip ? r0 + g0 : yt[g0][0];
    int g1 = g0 + 1;
    while (g1 < nrow && (vskip ? g1 + 1 - g0 : yt[g1][0] + yt[g1][1] - ry0) <= kRMaxRows) ++g1;
    const int ry1 = min(H, vskip ? r0 + g1 : yt[g1 - 1][0] + yt[g1 - 1][1]);
    const int nr = min(ry1 - ry0, kRMaxRows);
    // horizontal pass of source rows [ry0, ry0 + nr) at the tile's columns -> bytes in LDS
    for (int item = tid; item < nr * ncol; item += kImgThreads) {
      const int rr = item / ncol, cc = item % ncol;
      const uint8_t* row = f + (long long)(ry0 + rr) * W * 3;
      if (hskip) {
        const uint8_t* p = row + (c0 + cc) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) inter[rr][cc * 3 + c] = lut[p[c]];
      } else {
        const int xmin = xt[cc][0], cnt = xt[cc][1];
        int a0 = 1 << (kPrecBits - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < cnt; ++j) {
          const int k = xt[cc][2 + j];
          const uint8_t* p = row + min(xmin + j, W - 1) * 3;
          a0 += k * (int)lut[p[0]];
          a1 += k * (int)lut[p[1]];
          a2 += k * (int)lut[p[2]];
        }
        inter[rr][cc * 3 + 0] = (uint8_t)clip8(a0 >> kPrecBits);
        inter[rr][cc * 3 + 1] = (uint8_t)clip8(a1 >> kPrecBits);
        inter[rr][cc * 3 + 2] = (uint8_t)clip8(a2 >> kPrecBits);
      }
    }
    __syncthreads();
    // vertical pass from LDS; column fastest, so the fp32 planes are written 256 contiguous bytes per wave
    for (int item = tid; item < (g1 - g0) * 3 * ncol; item += kImgThreads) {
      const int cc = item % ncol, c = (item / ncol) % 3, gr = g0 + item / (3 * ncol);
      int v;
      if (vskip) {
        v = inter[gr - g0][cc * 3 + c];
      } else {
        const int ymin = yt[gr][0] - ry0, cnt = yt[gr][1];
        int acc = 1 << (kPrecBits - 1);
        for (int j = 0; j < cnt; ++j) acc += yt[gr][2 + j] * (int)inter[min(ymin + j, nr - 1)][cc * 3 + c];
        v = clip8(acc >> kPrecBits);
      }
      otile[gr][cc * 3 + c] = (uint8_t)v;
      if (out_f32)
        out_f32[(((long long)b * 3 + c) * h + r0 + gr) * w + c0 + cc] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.f), mean[c]), stdv[c]);
    }
    __syncthreads();
    g0 = g1;
  }
  if (out_u8) {
    const int rowlen = ncol * 3;
    for (int e = tid; e < nrow * rowlen; e += kImgThreads) {
      const int rr = e / rowlen, k = e % rowlen;
      out_u8[(((long long)b * h + r0 + rr) * w + c0) * 3 + k] = otile[rr][k];
    }
  }
}

// ---- colourise
// the value tensor2array sees at (row, col) of the rectangle: the map, or 1 / map as one IEEE division
static __device__ __forceinline__ float colour_value(const float* __restrict__ x, int recip) {
  const float v = *x;
  return recip ? __fdiv_rn(1.f, v) : v;
}

// torch's max: a NaN wins and stays
static __device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

__global__ void __launch_bounds__(kImgThreads) colorize_max_kernel(const float* __restrict__ x, int h, int w, int r0, int c0, int rh, int rw,
                                                                   int recip, float* __restrict__ partial) {
  __shared__ float smx[kImgThreads];
  const int b = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x, tid = threadIdx.x;
  const long long n = (long long)rh * rw;
  const long long lo = n * chunk / nchunk, hi = n * (chunk + 1) / nchunk;
  const float* p = x + (long long)b * h * w;
  float m = -INFINITY;
  for (long long i = lo + tid; i < hi; i += kImgThreads) {
    const int r = (int)(i / rw), c = (int)(i % rw);
    m = nan_max(m, colour_value(p + (long long)(r0 + r) * w + c0 + c, recip));
  }
  smx[tid] = m;
  __syncthreads();
  for (int o = kImgThreads / 2; o > 0; o >>= 1) {
    if (tid < o) smx[tid] = nan_max(smx[tid], smx[tid + o]);
    __syncthreads();
  }
  if (tid == 0) partial[b * nchunk + chunk] = smx[0];
}

// one thread per output byte.  table != nullptr: index = uint8(clip(fp32(fp32(255 * x) / max), 0, 255)) into uint8[256][3];
// else grey = uint8(fp32(255 * clip(fp32(x / max), 0, 1))).  A NaN (inf / inf) gives 0.
__global__ void __launch_bounds__(kImgThreads) colorize_u8_kernel(const float* __restrict__ x, int h, int w, int r0, int c0, int rh, int rw,
                                                                  int recip, float max_value, const float* __restrict__ partial,
                                                                  const uint8_t* __restrict__ table, uint8_t* __restrict__ out) {
  __shared__ float smx[DN_IMAGE_CHUNKS];
  const int b = blockIdx.y, tid = threadIdx.x;
  float mx = max_value;
  if (partial != nullptr) {
    if (tid < DN_IMAGE_CHUNKS) smx[tid] = partial[b * DN_IMAGE_CHUNKS + tid];
    __syncthreads();
    mx = -INFINITY;
    for (int k = 0; k < DN_IMAGE_CHUNKS; ++k) mx = nan_max(mx, smx[k]);
  }
  const long long n = 3LL * rh * rw;
  const float* p = x + (long long)b * h * w;
  uint8_t* o = out + (long long)b * n;
  for (long long i = blockIdx.x * (long long)kImgThreads + tid; i < n; i += (long long)gridDim.x * kImgThreads) {
    const int c = (int)(i % 3);
    const long long px = i / 3;
    const int r = (int)(px / rw), col = (int)(px % rw);
    const float v = colour_value(p + (long long)(r0 + r) * w + c0 + col, recip);
    int byte;
    if (table != nullptr) {
      const float t = __fdiv_rn(__fmul_rn(255.f, v), mx);
      const int idx = t == t ? (int)fminf(fmaxf(t, 0.f), 255.f) : 0;
      byte = table[idx * 3 + c];
    } else {
      const float g = __fdiv_rn(v, mx);
      byte = g == g ? (int)__fmul_rn(255.f, fminf(fmaxf(g, 0.f), 1.f)) : 0;
    }
    o[i] = (uint8_t)byte;
  }
}

// ---- contrast
static __device__ __forceinline__ unsigned luma(const uint8_t* p) {   // Pillow's RGB -> L: L24 >> 16 with rounding
  return (19595u * p[0] + 38470u * p[1] + 7471u * p[2] + 0x8000u) >> 16;
}

__global__ void __launch_bounds__(kImgThreads) contrast_sum_kernel(const uint8_t* __restrict__ src, long long npix,
                                                                   unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long ssum[kImgThreads];
  const int b = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x, tid = threadIdx.x;
  const long long lo = npix * chunk / nchunk, hi = npix * (chunk + 1) / nchunk;
  const uint8_t* p = src + (long long)b * npix * 3;
  unsigned long long s = 0;
  for (long long i = lo + tid; i < hi; i += kImgThreads) s += luma(p + i * 3);
  ssum[tid] = s;
  __syncthreads();
  for (int o = kImgThreads / 2; o > 0; o >>= 1) {
    if (tid < o) ssum[tid] += ssum[tid + o];
    __syncthreads();
  }
  if (tid == 0) partial[b * nchunk + chunk] = ssum[0];
}

// out = uint8(clip(fp32(m) + f * (fp32(p) - fp32(m)), 0, 255)), m = int(mean(L) + 0.5): ImageEnhance.Contrast is Image.blend(grey m, im, f)
__global__ void __launch_bounds__(kImgThreads) contrast_u8_kernel(const uint8_t* __restrict__ src, long long npix, float factor,
                                                                  const unsigned long long* __restrict__ partial, uint8_t* __restrict__ dst) {
  __shared__ unsigned long long ssum[DN_IMAGE_CHUNKS];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (tid < DN_IMAGE_CHUNKS) ssum[tid] = partial[b * DN_IMAGE_CHUNKS + tid];
  __syncthreads();
  unsigned long long total = 0;
#pragma unroll 4
  for (int k = 0; k < DN_IMAGE_CHUNKS; ++k) total += ssum[k];
  const float m = (float)(int)((double)total / (double)npix + 0.5);
  const long long n = 3 * npix;
  const uint8_t* p = src + (long long)b * n;
  uint8_t* o = dst + (long long)b * n;
  for (long long i = blockIdx.x * (long long)kImgThreads + tid; i < n; i += (long long)gridDim.x * kImgThreads) {
    const float t = __fadd_rn(m, __fmul_rn(factor, __fsub_rn((float)p[i], m)));
    o[i] = (uint8_t)fminf(fmaxf(t, 0.f), 255.f);
  }
}

static inline unsigned img_blocks(long long n) {
  const long long b = (n + kImgThreads - 1) / kImgThreads;
  return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

}  // namespace dn

using namespace dn;

extern "C" {

int dn_imresize_u8(const uint8_t* frames, const int32_t* hw, const int64_t* off, int32_t B, int32_t h, int32_t w, const int32_t* tabs,
                   const int32_t* tab_idx, int32_t max_taps, int32_t* minmax, uint8_t* out_u8, const float* mean_host, const float* std_host,
                   float* out_f32, dn_stream_t stream) {
  DN_REQUIRE(frames && hw && off && tabs && tab_idx && minmax && B > 0 && B <= 65535 && h > 0 && w > 0, DN_ERR_BAD_ARG,
             "dn_imresize_u8: bad argument");
  DN_REQUIRE(out_u8 || out_f32, DN_ERR_BAD_ARG, "dn_imresize_u8: no output");
  DN_REQUIRE(!out_f32 || (mean_host && std_host), DN_ERR_BAD_ARG, "dn_imresize_u8: the fp32 output needs mean / std");
  DN_REQUIRE(max_taps >= 0 && max_taps <= kRMaxTaps, DN_ERR_BAD_ARG,
             "dn_imresize_u8: %d taps per output exceed the bound of %d (a frame shrunk more than %d times along an axis)", (int)max_taps,
             kRMaxTaps, (kRMaxTaps - 1) / 2);
  dim3 grid((unsigned)((w + kRTileW - 1) / kRTileW), (unsigned)((h + kRTileH - 1) / kRTileH), (unsigned)B);
  DN_REQUIRE(grid.y <= 65535, DN_ERR_UNSUPPORTED, "dn_imresize_u8: h = %d is too large", (int)h);
  hipStream_t s = as_stream(stream);
  DN_LAUNCH(image_minmax_kernel, dim3(DN_IMAGE_CHUNKS, (unsigned)B), dim3(kImgThreads), 0, s, frames, (const int*)hw, (const long long*)off,
            (int)h, (int)w, (int*)minmax);
  int rc = check_launch("image_minmax_kernel");
  if (rc) return rc;
  const float one[3] = {1.f, 1.f, 1.f}, zero[3] = {0.f, 0.f, 0.f};
  const float* m = out_f32 ? mean_host : zero;
  const float* sd = out_f32 ? std_host : one;
  DN_LAUNCH(imresize_u8_kernel, grid, dim3(kImgThreads), 0, s, frames, (const int*)hw, (const long long*)off, (const int*)tabs,
            (const int*)tab_idx, (const int*)minmax, (int)h, (int)w, out_u8, out_f32, m[0], m[1], m[2], sd[0], sd[1], sd[2]);
  return check_launch("imresize_u8_kernel");
}

int dn_resize_u8(const uint8_t* frames, const int32_t* hw, const int64_t* off, int32_t B, int32_t h, int32_t w, const int32_t* tabs,
                 const int32_t* tab_idx, int32_t max_taps, uint8_t* out_u8, dn_stream_t stream) {
  DN_REQUIRE(frames && hw && off && tabs && tab_idx && out_u8 && B > 0 && B <= 65535 && h > 0 && w > 0, DN_ERR_BAD_ARG,
             "dn_resize_u8: bad argument");
  DN_REQUIRE(max_taps >= 0 && max_taps <= kRMaxTaps, DN_ERR_BAD_ARG,
             "dn_resize_u8: %d taps per output exceed the bound of %d (a frame shrunk more than %d times along an axis)", (int)max_taps,
             kRMaxTaps, (kRMaxTaps - 1) / 2);
  dim3 grid((unsigned)((w + kRTileW - 1) / kRTileW), (unsigned)((h + kRTileH - 1) / kRTileH), (unsigned)B);
  DN_REQUIRE(grid.y <= 65535, DN_ERR_UNSUPPORTED, "dn_resize_u8: h = %d is too large", (int)h);
  DN_LAUNCH(imresize_u8_kernel, grid, dim3(kImgThreads), 0, as_stream(stream), frames, (const int*)hw, (const long long*)off,
            (const int*)tabs, (const int*)tab_idx, (const int*)nullptr, (int)h, (int)w, out_u8, (float*)nullptr, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f);
  return check_launch("imresize_u8_kernel");
}

int dn_colorize_u8(const float* x, int32_t B, int32_t h, int32_t w, int32_t r0, int32_t r1, int32_t c0, int32_t c1, int32_t reciprocal,
                   float max_value, const uint8_t* table, float* max_ws, uint8_t* out, dn_stream_t stream) {
  DN_REQUIRE(x && out && B > 0 && B <= 65535 && h > 0 && w > 0, DN_ERR_BAD_ARG, "dn_colorize_u8: bad argument");
  DN_REQUIRE(0 <= r0 && r0 < r1 && r1 <= h && 0 <= c0 && c0 < c1 && c1 <= w, DN_ERR_BAD_ARG,
             "dn_colorize_u8: rectangle [%d, %d) x [%d, %d) is empty or outside %d x %d", (int)r0, (int)r1, (int)c0, (int)c1, (int)h, (int)w);
  const bool own_max = max_value < 0.f;
  DN_REQUIRE(!own_max || max_ws, DN_ERR_WORKSPACE, "dn_colorize_u8: the per-image maximum needs max_ws");
  hipStream_t s = as_stream(stream);
  const int rh = r1 - r0, rw = c1 - c0;
  if (own_max) {
    DN_LAUNCH(colorize_max_kernel, dim3(DN_IMAGE_CHUNKS, (unsigned)B), dim3(kImgThreads), 0, s, x, (int)h, (int)w, (int)r0, (int)c0, rh, rw,
              (int)(reciprocal != 0), max_ws);
    const int rc = check_launch("colorize_max_kernel");
    if (rc) return rc;
  }
  DN_LAUNCH(colorize_u8_kernel, dim3(img_blocks(3LL * rh * rw), (unsigned)B), dim3(kImgThreads), 0, s, x, (int)h, (int)w, (int)r0, (int)c0, rh,
            rw, (int)(reciprocal != 0), max_value, own_max ? (const float*)max_ws : (const float*)nullptr, table, out);
  return check_launch("colorize_u8_kernel");
}

int dn_contrast_u8(const uint8_t* src, int32_t B, int32_t h, int32_t w, float factor, uint64_t* sum_ws, uint8_t* dst, dn_stream_t stream) {
  DN_REQUIRE(src && dst && sum_ws && B > 0 && B <= 65535 && h > 0 && w > 0, DN_ERR_BAD_ARG, "dn_contrast_u8: bad argument");
  hipStream_t s = as_stream(stream);
  const long long npix = (long long)h * w;
  DN_LAUNCH(contrast_sum_kernel, dim3(DN_IMAGE_CHUNKS, (unsigned)B), dim3(kImgThreads), 0, s, src, npix, (unsigned long long*)sum_ws);
  const int rc = check_launch("contrast_sum_kernel");
  if (rc) return rc;
  DN_LAUNCH(contrast_u8_kernel, dim3(img_blocks(3 * npix), (unsigned)B), dim3(kImgThreads), 0, s, src, npix, factor,
            (const unsigned long long*)sum_ws, dst);
  return check_launch("contrast_u8_kernel");
}

}  // extern "C"
