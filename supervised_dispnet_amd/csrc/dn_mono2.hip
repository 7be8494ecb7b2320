// monodepth2's multi-scale objective (loss_functions.monodepth2_loss): per scale s of the decoder the minimum-reprojection term of the
// disparity upsampled to the input size, plus the edge-aware smoothness of the mean-normalised disparity at its own resolution.
//   * warped terms: per source frame ONE launch over (tile, sample, scale); a block obtains the disparity of its tile + halo from the
//     coarse map through the bilinear upsampling (DispCoarse, dn_reproj_dev.h), so neither the upsampled disparity nor the warped image
//     reaches HBM.  The identity terms do not depend on the scale: dn_reproj_term computes them once.
//   * one select launch over (pixels, scale), one launch for the per-sample means, one for the smoothness (the colour image of a
//     scale is the box average of the target, taken into LDS per tile while it is read; the same pass leaves the gradient with respect
//     to the normalised disparity and the per-sample sums  sum_j g_j d_j  behind), one finalize with fixed-order fp64 sums.
//   * backward: per source frame the coefficient and the gather pass over all scales (full-resolution ddisp per scale), then one
//     launch that gathers the adjoint of the upsampling into the coarse maps and adds the smoothness gradient through the
//     normalisation.
// The number of launches does not depend on the number of scales.  No atomics: every sum has a fixed order.
#include "dn_reproj_dev.h"

namespace dn {

constexpr int kMaxScales = 4;

struct Mono2Disps {
  const float* p[kMaxScales];         // [B][H >> s][W >> s]
};
struct Mono2Out {
  float* p[kMaxScales];
};

__device__ __forceinline__ DispCoarse mono2_disp(const Mono2Disps& d, int s, int H, int W) {
  const DispCoarse r = {d.p[s], H >> s, W >> s, 1 << s};
  return r;
}

// grid (tiles x, tiles y, B * S); terms + s * sstride is the [B][H][W] map of scale s
__global__ void __launch_bounds__(256) mono2_term_kernel(const ReprojArgs a, const Mono2Disps d, float* __restrict__ terms, long long sstride) {
  __shared__ float sx[3][kHN], sy[3][kHN];
  __shared__ float P[12];
  const int s = blockIdx.z / a.B, b = blockIdx.z - s * a.B;
  reproj_term_tile<true>(a, mono2_disp(d, s, a.H, a.W), b, blockIdx.y * kTH, blockIdx.x * kTW, sx, sy, P, terms + s * sstride);
}

// Scale s = blockIdx.y: the minimum over [ident (n_id channels, shared by the scales), warped[s] (F channels)] of n pixels each (a tie
// goes to the lowest channel), sel [S][n] = its index, partial [S][gridDim.x] = the block's sum of the minimum (times wgt [S][n] when
// given).  The loop and the sum are those of reproj_select_kernel.
__global__ void __launch_bounds__(256) mono2_select_kernel(const float* __restrict__ ident, int n_id, const float* __restrict__ warped, int F,
                                                           long long n, const float* __restrict__ wgt, unsigned char* __restrict__ sel,
                                                           float* __restrict__ partial) {
  const int s = blockIdx.y;
  const float* wp = warped + (long long)s * F * n;
  float acc = 0.f;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float best = n_id > 0 ? ident[i] : wp[i];
    int bi = 0;
    for (int c = 1; c < n_id + F; ++c) {
      const float v = c < n_id ? ident[(long long)c * n + i] : wp[(long long)(c - n_id) * n + i];
      if (v < best) { best = v; bi = c; }
    }
    sel[(long long)s * n + i] = (unsigned char)bi;
    acc += wgt != nullptr ? best * wgt[(long long)s * n + i] : best;
  }
  __shared__ float lds[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long long)s * gridDim.x + blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// block-wide fp64 sum in thread 0 (256 threads; the scheme of reproj_finalize_kernel); lds4 may be reused after the call
__device__ __forceinline__ double block_sum_d(double s, double* lds4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = s;
  __syncthreads();
  return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}

// mu [S][B] = mean of disparity map s of sample b.  grid (B, S): one block per map, fixed order.
// 1024 threads with four independent accumulators each: the loop is a chain of load latencies, not of bytes.
__global__ void __launch_bounds__(1024) mono2_mean_kernel(const Mono2Disps d, int B, int H, int W, float* __restrict__ mu) {
  __shared__ double lds16[16];
  const int b = blockIdx.x, s = blockIdx.y;
  const int n = (H >> s) * (W >> s);
  const float* p = d.p[s] + (long long)b * n;
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  int i = threadIdx.x;
  for (; i + 3 * 1024 < n; i += 4 * 1024) {
    a0 += (double)p[i]; a1 += (double)p[i + 1024]; a2 += (double)p[i + 2 * 1024]; a3 += (double)p[i + 3 * 1024];
  }
  for (; i < n; i += 1024) a0 += (double)p[i];
  double t = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if ((threadIdx.x & 63) == 0) lds16[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0;
    for (int k = 0; k < 16; ++k) tot += lds16[k];
    mu[s * B + b] = (float)(tot / (double)n);
  }
}

// offset of scale s in a buffer that holds the S coarse maps [B][h_s][w_s] one after the other
__device__ __forceinline__ long long coarse_offset(int s, int B, int H, int W) {
  long long o = 0;
  for (int k = 0; k < s; ++k) o += (long long)B * (H >> k) * (W >> k);
  return o;
}

__device__ __forceinline__ float edge_weight(const float* a, const float* b) {      // planes kHN apart
  return expf(-((fabsf(a[0] - b[0]) + fabsf(a[kHN] - b[kHN]) + fabsf(a[2 * kHN] - b[2 * kHN])) / 3.f));
}

// Edge-aware smoothness of norm_s = disp_s / (mu + 1e-7) under colour_s, the scale x scale box average of the target, forward and the
// gradient with respect to norm_s in one pass.  A block owns an 8 x 32 tile of the COARSE map of (sample, scale) = blockIdx.z and first
// box-averages the colour of the tile and its one-pixel halo out of the full-resolution target into LDS (every box is read once per
// block; no colour pyramid in HBM); the four edge weights of a pixel then come from LDS.  Written: partial [S][B][tiles][2] (the sums of
// the x and y direction), g (gbuf: the S maps one after the other) = d smooth_s / d norm_s, and dotp [S][B][tiles] = the tile's share of
// sum_j g_j d_j, which the normalisation's gradient needs.  The grid is that of scale 0: tiles beyond a coarser map write zeros.
__global__ void __launch_bounds__(256) mono2_smooth_kernel(const float* __restrict__ tgt, const Mono2Disps d, const float* __restrict__ mu,
                                                           int B, int H, int W, float* __restrict__ partial, float* __restrict__ gbuf,
                                                           float* __restrict__ dotp) {
  __shared__ float col[3 * kHN];
  __shared__ float lds[8];
  __shared__ double lds4[4];
  const int s = blockIdx.z / B, b = blockIdx.z - s * B;
  const int h = H >> s, w = W >> s, scale = 1 << s;
  const int ty0 = blockIdx.y * kTH, tx0 = blockIdx.x * kTW;
  const long long tile = ((long long)s * B + b) * (gridDim.x * gridDim.y) + blockIdx.y * gridDim.x + blockIdx.x;
  if (ty0 >= h || tx0 >= w) {
    if (threadIdx.x == 0) { partial[tile * 2] = 0.f; partial[tile * 2 + 1] = 0.f; dotp[tile] = 0.f; }
    return;
  }
  const long long plane = (long long)H * W;
  const float* img = tgt + (long long)b * 3 * plane;
  const float inv = 1.f / (float)(scale * scale);
  for (int idx = threadIdx.x; idx < kHN; idx += 256) {
    const int hy = idx / kHW, hx = idx - hy * kHW;
    const int y = ty0 + hy - 1, x = tx0 + hx - 1;
    float c[3] = {0.f, 0.f, 0.f};
    if (y >= 0 && y < h && x >= 0 && x < w) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float* q = img + k * plane + (long long)y * scale * W + x * scale;
        float sum = 0.f;
        for (int dy = 0; dy < scale; ++dy)
          for (int dx = 0; dx < scale; ++dx) sum += q[dy * W + dx];
        c[k] = sum * inv;
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) col[k * kHN + idx] = c[k];
  }
  __syncthreads();
  const int ly = threadIdx.x / kTW, lx = threadIdx.x % kTW;
  const int y = ty0 + ly, x = tx0 + lx;
  float ax = 0.f, ay = 0.f;
  double dot = 0;
  if (y < h && x < w) {
    const float* D = d.p[s] + (long long)b * h * w;
    const float den = mu[s * B + b] + 1e-7f;
    const float nx = (float)B * h * (w - 1), ny = (float)B * (h - 1) * w;
    auto sgnf = [](float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); };
    const int i = y * w + x;
    const float* c0 = col + (ly + 1) * kHW + lx + 1;
    const float v = D[i] / den;
    float g = 0.f;
    if (x < w - 1) {
      const float e = v - D[i + 1] / den, wt = edge_weight(c0, c0 + 1);
      ax = fabsf(e) * wt;
      g += sgnf(e) * wt / nx;
    }
    if (x > 0) g -= sgnf(D[i - 1] / den - v) * edge_weight(c0 - 1, c0) / nx;
    if (y < h - 1) {
      const float e = v - D[i + w] / den, wt = edge_weight(c0, c0 + kHW);
      ay = fabsf(e) * wt;
      g += sgnf(e) * wt / ny;
    }
    if (y > 0) g -= sgnf(D[i - w] / den - v) * edge_weight(c0 - kHW, c0) / ny;
    gbuf[coarse_offset(s, B, H, W) + (long long)b * h * w + i] = g;
    dot = (double)g * (double)D[i];
  }
  ax = wave_sum(ax);
  ay = wave_sum(ay);
  if ((threadIdx.x & 63) == 0) { lds[threadIdx.x >> 6] = ax; lds[4 + (threadIdx.x >> 6)] = ay; }
  dot = block_sum_d(dot, lds4);
  if (threadIdx.x == 0) {
    partial[tile * 2] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    partial[tile * 2 + 1] = (lds[4] + lds[5]) + (lds[6] + lds[7]);
    dotp[tile] = (float)dot;
  }
}


// parts [S][2] = (mean of the minimum, smoothness) per scale; loss = (1 / S) sum_s (parts[s][0] + smoothness / 2^s * parts[s][1]).
// One block; every sum is a fixed-order fp64 sum.  A direction of a map that has no neighbour pair (a map one pixel high or wide)
// contributes 0.
__global__ void __launch_bounds__(256) mono2_finalize_kernel(const float* __restrict__ sel_partial, int nb_sel, const float* __restrict__ sm_partial,
                                                             int nb_sm, int B, int H, int W, int S, float smoothness, float* __restrict__ parts,
                                                             float* __restrict__ loss) {
  __shared__ double lds4[4];
  double total = 0;
  for (int s = 0; s < S; ++s) {
    const int h = H >> s, w = W >> s;
    double a = 0, ax = 0, ay = 0;
    for (int i = threadIdx.x; i < nb_sel; i += 256) a += (double)sel_partial[(long long)s * nb_sel + i];
    for (int i = threadIdx.x; i < nb_sm; i += 256) {
      ax += (double)sm_partial[((long long)s * nb_sm + i) * 2];
      ay += (double)sm_partial[((long long)s * nb_sm + i) * 2 + 1];
    }
    a = block_sum_d(a, lds4);
    ax = block_sum_d(ax, lds4);
    ay = block_sum_d(ay, lds4);
    if (threadIdx.x == 0) {
      const double rep = a / ((double)B * H * W);
      const float smx = w > 1 ? (float)(ax / ((double)B * h * (w - 1))) : 0.f;
      const float smy = h > 1 ? (float)(ay / ((double)B * (h - 1) * w)) : 0.f;
      const float sm = smx + smy;
      parts[s * 2] = (float)rep;
      parts[s * 2 + 1] = sm;
      total += rep + (double)(smoothness / (float)(1 << s)) * (double)sm;
    }
  }
  if (threadIdx.x == 0) loss[0] = (float)(total / (double)S);
}

// upstream gradient of the minimum of scale s (sel, wgt: that scale's maps): the pixels won by `channel` carry dloss * scale (* wgt)
struct Mono2Up {
  const unsigned char* sel;
  int channel;
  const float* dloss;
  const float* wgt;
  float scale;              // 1 / (B H W) / S
  __device__ __forceinline__ float operator()(long long i) const {
    if (sel[i] != (unsigned char)channel) return 0.f;
    const float g = dloss[0] * scale;
    return wgt != nullptr ? g * wgt[i] : g;
  }
};

__device__ __forceinline__ Mono2Up mono2_up(Mono2Up u, int s, long long n) {
  u.sel += (long long)s * n;
  if (u.wgt != nullptr) u.wgt += (long long)s * n;
  return u;
}

// grid (tiles x, tiles y, B * S); coef [S][3][B*3][HW]
__global__ void __launch_bounds__(256) mono2_bwd_coef_kernel(const ReprojArgs a, const Mono2Disps d, const Mono2Up u, float* __restrict__ coef) {
  __shared__ float sx[3][kHN], sy[3][kHN];
  __shared__ float P[12];
  const int s = blockIdx.z / a.B, b = blockIdx.z - s * a.B;
  const long long n = (long long)a.B * a.H * a.W;
  reproj_coef_tile(a, mono2_disp(d, s, a.H, a.W), mono2_up(u, s, n), b, blockIdx.y * kTH, blockIdx.x * kTW, sx, sy, P, coef + 9 * n * s);
}

// grid (blocks, B, S); ddfull [S][B][HW]: the gradient of the UPSAMPLED disparity of every scale; partial [B][S * gridDim.x][12]
__global__ void __launch_bounds__(256) mono2_bwd_kernel(const ReprojArgs a, const Mono2Disps d, const Mono2Up u, const float* __restrict__ coef,
                                                        float* __restrict__ ddfull, int accumulate, float* __restrict__ partial) {
  __shared__ float P[12];
  __shared__ float lds[48];
  const int b = blockIdx.y, s = blockIdx.z;
  if (threadIdx.x == 0) proj_matrix(a.K, a.T, b, P);
  __syncthreads();
  const long long n = (long long)a.B * a.H * a.W;
  float acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.f;
  reproj_bwd_pixels(a, mono2_disp(d, s, a.H, a.W), mono2_up(u, s, n), P, b, blockIdx.x * 256ll + threadIdx.x, (long long)gridDim.x * 256,
                    coef + 9 * n * s, ddfull + n * s, accumulate, acc);
  block_sum12(acc, lds, partial + (((long long)b * gridDim.z + s) * gridDim.x + blockIdx.x) * 12);
}


// ddisp_s = (adjoint of the bilinear upsampling) ddfull[s]  +  up_s * (g / (mu + eps) - sum_j g_j d_j / (N (mu + eps)^2)) with
// up_s = dloss * smoothness / 2^s / S and g, the tiles' shares of the sum (dotp [S][B][tiles]) from mono2_smooth_kernel.  The adjoint is a
// gather in the fixed order of upsample_int_bwd_kernel.  grid (blocks, B, S).
__global__ void __launch_bounds__(256) mono2_disp_grad_kernel(const float* __restrict__ mu, const float* __restrict__ dloss, float smoothness,
                                                              float inv_s, const float* __restrict__ ddfull, const float* __restrict__ gbuf,
                                                              const float* __restrict__ dotp, int tiles, int B, int H, int W, const Mono2Out out) {
  __shared__ float sh[2];
  __shared__ double lds4[4];
  const int b = blockIdx.y, s = blockIdx.z;
  const int h = H >> s, w = W >> s, scale = 1 << s;
  double t = 0;
  for (int k = threadIdx.x; k < tiles; k += 256) t += (double)dotp[((long long)s * B + b) * tiles + k];
  t = block_sum_d(t, lds4);
  if (threadIdx.x == 0) {
    const float den = mu[s * B + b] + 1e-7f;
    sh[0] = den;
    sh[1] = (float)(t / ((double)h * w * (double)den * (double)den));
  }
  __syncthreads();
  const float den = sh[0], shift = sh[1];
  const float up = dloss[0] * (smoothness / (float)scale) * inv_s;
  const float* Dd = ddfull + ((long long)s * B + b) * H * W;
  const float* G = gbuf + coarse_offset(s, B, H, W) + (long long)b * h * w;
  float* O = out.p[s] + (long long)b * h * w;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < h * w; i += gridDim.x * 256) {
    const int y = i / w, x = i - y * w;
    float acc = 0.f;
    if (scale == 1) {
      acc = Dd[i];
    } else {
      // the output rows whose two source rows include y: their half-pixel source index lies in (y - 1, y + 1), plus the clamped ends
      const int oy_lo = max(0, y * scale - scale / 2), oy_hi = min(H, (y + 1) * scale + scale / 2);
      const int ox_lo = max(0, x * scale - scale / 2), ox_hi = min(W, (x + 1) * scale + scale / 2);
      for (int oy = oy_lo; oy < oy_hi; ++oy) {
        int y0, y1;
        float ly;
        bil_src(oy, scale, h, &y0, &y1, &ly);
        float wy = 0.f;
        if (y0 == y) wy += 1.f - ly;
        if (y1 == y) wy += ly;
        if (wy == 0.f) continue;
        for (int ox = ox_lo; ox < ox_hi; ++ox) {
          int x0, x1;
          float lx;
          bil_src(ox, scale, w, &x0, &x1, &lx);
          float wx = 0.f;
          if (x0 == x) wx += 1.f - lx;
          if (x1 == x) wx += lx;
          if (wx != 0.f) acc += wy * wx * Dd[oy * W + ox];
        }
      }
    }
    O[i] = acc + up * (G[i] / den - shift);
  }
}

static int mono2_check(const float* const* disps, int B, int H, int W, int S) {
  DN_REQUIRE(S >= 1 && S <= kMaxScales && B > 0 && H >= 2 && W >= 2, DN_ERR_BAD_ARG, "mono2: 1 to 4 scales and H, W >= 2 expected");
  DN_REQUIRE(H % (1 << (S - 1)) == 0 && W % (1 << (S - 1)) == 0, DN_ERR_BAD_ARG, "mono2: %d x %d is not divisible by 2^%d", H, W, S - 1);
  DN_REQUIRE((long long)B * S <= 65535, DN_ERR_BAD_ARG, "mono2: B * S exceeds the grid");
  for (int s = 0; s < S; ++s) DN_REQUIRE(disps[s] != nullptr, DN_ERR_BAD_ARG, "mono2: disparity of scale %d is null", s);
  return DN_OK;
}

static inline int mono2_tiles(int H, int W) { return ((W + kTW - 1) / kTW) * ((H + kTH - 1) / kTH); }

static inline Mono2Disps mono2_disps(const float* const* p, int S) {
  Mono2Disps d;
  for (int s = 0; s < kMaxScales; ++s) d.p[s] = s < S ? p[s] : nullptr;
  return d;
}

}  // namespace dn

using namespace dn;

extern "C" {

int32_t dn_mono2_blocks(int64_t n) { return rp_blocks(n, 1024); }

int dn_mono2_term(const float* tgt, const float* ref, const float* disp0, const float* disp1, const float* disp2, const float* disp3,
                  const float* K, const float* inv_K, const float* T, int32_t B, int32_t H, int32_t W, int32_t S, int32_t align_corners,
                  float d_lo, float d_span, float eps, float ssim_weight, float* terms, int64_t scale_stride, dn_stream_t stream) {
  const float* dp[kMaxScales] = {disp0, disp1, disp2, disp3};
  int rc = mono2_check(dp, B, H, W, S);
  if (rc != DN_OK) return rc;
  ReprojArgs a;
  rc = fill_reproj_args(&a, tgt, ref, nullptr, K, inv_K, T, B, H, W, align_corners, 1, d_lo, d_span, eps, ssim_weight);
  if (rc != DN_OK) return rc;
  DN_REQUIRE(K && inv_K && T && terms && scale_stride >= (int64_t)B * H * W, DN_ERR_BAD_ARG, "dn_mono2_term: bad argument");
  DN_LAUNCH(mono2_term_kernel, dim3((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, B * S), dim3(256), 0, as_stream(stream), a, mono2_disps(dp, S),
            terms, (long long)scale_stride);
  return check_launch("mono2_term_kernel");
}

int dn_mono2_select(const float* ident, int32_t n_ident, const float* warped, int32_t F, int32_t S, int64_t n, const float* weights,
                    uint8_t* sel, float* partial, dn_stream_t stream) {
  DN_REQUIRE(warped && sel && partial && F >= 1 && n_ident >= 0 && n_ident + F <= 255 && (n_ident == 0 || ident) && S >= 1 &&
                 S <= kMaxScales && n > 0,
             DN_ERR_BAD_ARG, "dn_mono2_select: bad argument");
  DN_LAUNCH(mono2_select_kernel, dim3(rp_blocks(n, 1024), S), dim3(256), 0, as_stream(stream), ident, n_ident, warped, F, (long long)n, weights,
            sel, partial);
  return check_launch("mono2_select_kernel");
}

int dn_mono2_finish_fwd(const float* tgt, const float* disp0, const float* disp1, const float* disp2, const float* disp3, int32_t B, int32_t H,
                        int32_t W, int32_t S, const float* sel_partial, float smoothness, float* mu, float* smooth_partial, float* gbuf,
                        float* dot_partial, float* parts, float* loss, dn_stream_t stream) {
  const float* dp[kMaxScales] = {disp0, disp1, disp2, disp3};
  int rc = mono2_check(dp, B, H, W, S);
  if (rc != DN_OK) return rc;
  DN_REQUIRE(tgt && sel_partial && mu && smooth_partial && gbuf && dot_partial && parts && loss, DN_ERR_BAD_ARG,
             "dn_mono2_finish_fwd: null pointer");
  hipStream_t st = as_stream(stream);
  const Mono2Disps d = mono2_disps(dp, S);
  const dim3 tiles((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, B * S);
  DN_LAUNCH(mono2_mean_kernel, dim3(B, S), dim3(1024), 0, st, d, B, H, W, mu);
  DN_LAUNCH(mono2_smooth_kernel, tiles, dim3(256), 0, st, tgt, d, (const float*)mu, B, H, W, smooth_partial, gbuf, dot_partial);
  DN_LAUNCH(mono2_finalize_kernel, dim3(1), dim3(256), 0, st, sel_partial, rp_blocks((long long)B * H * W, 1024), (const float*)smooth_partial,
            (int)(tiles.x * tiles.y) * B, B, H, W, S, smoothness, parts, loss);
  return check_launch("mono2_finish_fwd");
}

int dn_mono2_bwd(const float* tgt, const float* ref, const float* disp0, const float* disp1, const float* disp2, const float* disp3,
                 const float* K, const float* inv_K, const float* T, int32_t B, int32_t H, int32_t W, int32_t S, int32_t align_corners,
                 float d_lo, float d_span, float eps, float ssim_weight, const uint8_t* sel, int32_t channel, const float* dloss,
                 const float* weights, float* workspace, float* ddfull, int32_t accumulate, float* partial, dn_stream_t stream) {
  const float* dp[kMaxScales] = {disp0, disp1, disp2, disp3};
  int rc = mono2_check(dp, B, H, W, S);
  if (rc != DN_OK) return rc;
  ReprojArgs a;
  rc = fill_reproj_args(&a, tgt, ref, nullptr, K, inv_K, T, B, H, W, align_corners, 1, d_lo, d_span, eps, ssim_weight);
  if (rc != DN_OK) return rc;
  DN_REQUIRE(K && inv_K && T && sel && dloss && workspace && ddfull && partial, DN_ERR_BAD_ARG, "dn_mono2_bwd: null pointer");
  const Mono2Up u = {sel, channel, dloss, weights, 1.f / ((float)B * (float)H * (float)W) / (float)S};
  const Mono2Disps d = mono2_disps(dp, S);
  hipStream_t st = as_stream(stream);
  DN_LAUNCH(mono2_bwd_coef_kernel, dim3((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, B * S), dim3(256), 0, st, a, d, u, workspace);
  DN_LAUNCH(mono2_bwd_kernel, dim3(reproj_blocks(H, W), B, S), dim3(256), 0, st, a, d, u, (const float*)workspace, ddfull, accumulate, partial);
  return check_launch("mono2_bwd");
}

int dn_mono2_disp_grad(int32_t B, int32_t H, int32_t W, int32_t S, const float* mu, const float* dloss, float smoothness, const float* ddfull,
                       const float* gbuf, const float* dot_partial, float* ddisp0, float* ddisp1, float* ddisp2, float* ddisp3,
                       dn_stream_t stream) {
  DN_REQUIRE(S >= 1 && S <= kMaxScales && B > 0 && H >= 2 && W >= 2 && H % (1 << (S - 1)) == 0 && W % (1 << (S - 1)) == 0 &&
                 (long long)B * S <= 65535,
             DN_ERR_BAD_ARG, "dn_mono2_disp_grad: bad size");
  float* op[kMaxScales] = {ddisp0, ddisp1, ddisp2, ddisp3};
  Mono2Out out;
  for (int s = 0; s < kMaxScales; ++s) {
    DN_REQUIRE(s >= S || op[s] != nullptr, DN_ERR_BAD_ARG, "dn_mono2_disp_grad: gradient of scale %d is null", s);
    out.p[s] = s < S ? op[s] : nullptr;
  }
  DN_REQUIRE(mu && dloss && ddfull && gbuf && dot_partial, DN_ERR_BAD_ARG, "dn_mono2_disp_grad: null pointer");
  DN_LAUNCH(mono2_disp_grad_kernel, dim3(reproj_blocks(H, W), B, S), dim3(256), 0, as_stream(stream), mu, dloss, smoothness, 1.f / (float)S,
            ddfull, gbuf, dot_partial, mono2_tiles(H, W), B, H, W, out);
  return check_launch("mono2_disp_grad_kernel");
}

int32_t dn_mono2_tiles(int32_t H, int32_t W) { return mono2_tiles(H, W); }

}  // extern "C"
