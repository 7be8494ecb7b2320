// BatchNorm on NHWC tensors, gfx950 only: batch statistics (the finalize of the conv epilogues' partial rows in both orders, the partial
// rows of a materialised tensor, the eval-mode affine), BN + ReLU + MaxPool 2x2 forward, the backward (the column sums of dz -- after a
// ReLU, through a pool --, their finalize in both orders, the apply pass in its dz / ReLU / pool forms), the ResNet bottleneck tail, and
// the backward of a FROZEN BatchNorm (running statistics: one pass per form that writes dy and takes the sums, plus its finalize).
// HBM-bound; the column reductions are the two-stage ones of dn_colreduce.h.
#include "dn_colreduce.h"
#include "dn_fold.h"

namespace dn {

// -------------------------------------------------------------------------------------------------- BN statistics
// one block per channel.  partial[t][c] = (sum, M2 about the tile mean) of row tile t (kBnTileRows rows, the last one ragged);
// merged in fp64: mean = sum_t s_t / N,  M2 = sum_t [ M2_t + n_t (s_t/n_t - mean)^2 ]   (Chan et al.)
constexpr int kBnTileRows = 128;   // = BM of every igemm_conv_kernel instantiation
__global__ void __launch_bounds__(kThreads) bn_finalize_kernel(const float* __restrict__ partial, int rows, int C, double count,
                                                               const float* __restrict__ conv_bias, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* running_mean, float* running_var,
                                                               float momentum, float eps, float* mean_out, float* invstd_out, float* scale,
                                                               float* shift, long long* num_batches_tracked) {
  const int c = blockIdx.x;
  if (num_batches_tracked != nullptr && c == 0 && threadIdx.x == 0) num_batches_tracked[0] += 1;   // nn.BatchNorm2d's step counter
  // One pass over the partial rows: per row t the pair (s_t, M2_t about the tile's own mean) is read once and three sums are kept in
  // fp64 -- S = sum s_t, Q = sum M2_t, P = sum n_t (s_t / n_t - pivot)^2 with pivot = the first tile's mean -- from which
  //   mean = S / N,   M2 = Q + sum_t n_t (m_t - mean)^2 = Q + P - N (mean - pivot)^2      (Chan et al., expanded about the pivot).
  // About a pivot inside the data's range the two terms that cancel are both of the order of the between-tile spread, so a channel
  // with |mean| >> std (mean^2 / var ~ 1e10 and beyond) keeps its variance; the expansion about 0 lost it there.
  __shared__ double red[3][4];
  double s1 = 0.0, q = 0.0, pp = 0.0;
  const double n0 = count < (double)kBnTileRows ? count : (double)kBnTileRows;
  const double pivot = (double)partial[(long long)c * 2] / n0;
#pragma unroll 8
  for (int r = threadIdx.x; r < rows; r += kThreads) {      // (8 strided 8-byte loads in flight)
    const float2 v = *reinterpret_cast<const float2*>(partial + ((long long)r * C + c) * 2);
    const double left = count - (double)r * kBnTileRows;
    const double nt = left < (double)kBnTileRows ? left : (double)kBnTileRows;
    const double dm = (double)v.x / nt - pivot;
    s1 += (double)v.x;
    q += (double)v.y;
    pp += nt * dm * dm;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    q += __shfl_xor(q, o);
    pp += __shfl_xor(pp, o);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s1;
    red[1][threadIdx.x >> 6] = q;
    red[2][threadIdx.x >> 6] = pp;
  }
  __syncthreads();
  double macc = 0.0, m2tot = 0.0;
  if (threadIdx.x == 0) {
    const double S = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    const double Q = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const double P = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    macc = S / count;
    m2tot = Q + (P - count * (macc - pivot) * (macc - pivot));
  }
  if (threadIdx.x == 0) {
    double var = m2tot / count;   // biased; the conv bias shifts the mean only
    if (var < 0.0) var = 0.0;
    const float mean = (float)(macc + (conv_bias ? (double)conv_bias[c] : 0.0));
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gamma[c] * invstd;
    mean_out[c] = mean;
    invstd_out[c] = invstd;
    scale[c] = sc;
    shift[c] = beta[c] - mean * sc;
    if (running_mean) {
      const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
    }
  }
}

// The sliced order of dn_fold.h as kernels of their own (<= kFoldMaxRows partial rows): one block per 64 channels.  The Winograd kernels
// run the same device functions in their last-arriving block when the caller asked for it -- same bits either way.
__global__ void __launch_bounds__(256) bn_finalize_sliced_kernel(const float* __restrict__ partial, int rows, int C, double count, BnFinalizeArgs a) {
  __shared__ double red[3 * kFoldSlices * 64];
  const int c0 = blockIdx.x * 64;
  bn_finalize_sliced<false>(partial, rows, C, c0, C - c0 < 64 ? C - c0 : 64, count, a, red, threadIdx.x);
}

__global__ void __launch_bounds__(256) colsum2_sliced_kernel(const float* __restrict__ partial, int rows, int C, int stride, int offset,
                                                             float* __restrict__ out0, float* __restrict__ out1) {
  __shared__ double red[2 * kFoldSlices * 64];
  const int c0 = blockIdx.x * 64;
  colsum2_sliced<false>(partial, rows, C, stride, offset, c0, C - c0 < 64 ? C - c0 : 64, out0, out1, red, threadIdx.x);
}

// invstd_out (nullable): what a frozen BatchNorm's backward needs besides the affine (dn_bn_frozen_affine)
__global__ void bn_eval_affine_kernel(int C, const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                                      float* scale, float* shift, float* invstd_out) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    float invstd = 1.f / sqrtf(rv[c] + eps);
    float sc = gamma[c] * invstd;
    scale[c] = sc;
    shift[c] = beta[c] - rm[c] * sc;
    if (invstd_out != nullptr) invstd_out[c] = invstd;
  }
}

// Batch statistics of a materialised tensor in the conv epilogues' partial layout (FCRN's interleaved up-projection maps).
// one block per (row tile, 64-channel group): thread (c, q) sums rows q, q+4, ... of its channel, the four partial sums meet in LDS;
// second pass about the tile's own mean (the tile is re-read from L2)
__global__ void __launch_bounds__(kThreads) bn_stats_partial_kernel(const float* __restrict__ x, long long rows, int C, float* __restrict__ partial) {
  __shared__ float red[4][64];
  __shared__ float mean_s[64];
  const int c = blockIdx.y * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * kBnTileRows;
  const long long left = rows - r0;
  const int n = left < kBnTileRows ? (int)left : kBnTileRows;
  float s = 0.f;
  if (c < C)
    for (int r = q; r < n; r += 4) s += x[(r0 + r) * C + c];
  red[q][threadIdx.x & 63] = s;
  __syncthreads();
  float tot = 0.f;
  if (q == 0) {
    tot = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    mean_s[threadIdx.x] = tot / (float)n;
  }
  __syncthreads();
  const float mu = mean_s[threadIdx.x & 63];
  float m2 = 0.f;
  if (c < C)
    for (int r = q; r < n; r += 4) {
      const float d = x[(r0 + r) * C + c] - mu;
      m2 += d * d;
    }
  __syncthreads();
  red[q][threadIdx.x & 63] = m2;
  __syncthreads();
  if (q == 0 && c < C) {
    float* dst = partial + ((long long)blockIdx.x * C + c) * 2;
    dst[0] = tot;
    dst[1] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
  }
}

// BatchNorm apply without ReLU (FCRN: bn2 feeds the first up-projection as a plain tensor)
__global__ void __launch_bounds__(kThreads) bn_apply_kernel(const float* __restrict__ y, const float* __restrict__ scale, const float* __restrict__ shift,
                                                            long long rows, int C, float* __restrict__ out) {
  const int G = C / 4;
  const long long total = rows * G;
  for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int g = (int)(i % G);
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + i * 4);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + 4 * g), sh = *reinterpret_cast<const f32x4*>(shift + 4 * g);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = v[e] * sc[e] + sh[e];
    *reinterpret_cast<f32x4*>(out + i * 4) = o;
  }
}

// --------------------------------------------------------------------------------------- BN + ReLU + MaxPool 2x2
__global__ void __launch_bounds__(kThreads) bn_relu_pool_fwd_kernel(const float* __restrict__ y, const float* __restrict__ scale,
                                                                    const float* __restrict__ shift, int N, int H, int W, int C,
                                                                    float* __restrict__ pooled, uint8_t* __restrict__ idx) {
  const int PH = H / 2, PW = W / 2, G = C / 4;
  const long long total = (long long)N * PH * PW * G;
  for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int g = (int)(i % G);
    long long pix = i / G;
    const int px = (int)(pix % PW);
    pix /= PW;
    const int py = (int)(pix % PH), n = (int)(pix / PH);
    const int c = g * 4;
    // scale == nullptr: y is a plain (already activated) tensor -- nn.MaxPool2d(2, 2) after conv + ReLU (models/Disp_vgg.py:79-100)
    const f32x4 sc = scale ? *reinterpret_cast<const f32x4*>(scale + c) : f32x4{1.f, 1.f, 1.f, 1.f};
    const f32x4 sh = scale ? *reinterpret_cast<const f32x4*>(shift + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    const float* base = y + (((long long)n * H + 2 * py) * W + 2 * px) * C + c;
    f32x4 best;
    int bi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(base + ((long long)(q >> 1) * W + (q & 1)) * C);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = scale ? fmaxf(0.f, v[e] * sc[e] + sh[e]) : v[e];
        if (q == 0 || a > best[e]) {
          best[e] = a;
          bi[e] = q;
        }
      }
    }
    const long long o = i * 4;
    *reinterpret_cast<f32x4*>(pooled + o) = best;
    uchar4 code;
    code.x = (uint8_t)(bi[0] | (best[0] > 0.f ? 4 : 0));
    code.y = (uint8_t)(bi[1] | (best[1] > 0.f ? 4 : 0));
    code.z = (uint8_t)(bi[2] | (best[2] > 0.f ? 4 : 0));
    code.w = (uint8_t)(bi[3] | (best[3] > 0.f ? 4 : 0));
    *reinterpret_cast<uchar4*>(idx + o) = code;
  }
}

// ------------------------------------------------------------------------------------------- backward: the column sums
struct PoolBwdOp {
  static constexpr int NACC = 2;
  const float* dpooled;
  const uint8_t* idx;
  const float* y;
  const float* mean;
  const float* invstd;
  float* dz;
  int PH, PW, H, W, C;
  template <int V>
  __device__ __forceinline__ void apply(long long row, int c0, float (&acc)[V][2]) const {
    const int px = (int)(row % PW);
    long long t = row / PW;
    const int py = (int)(t % PH), n = (int)(t / PH);
    const Vec<V> dp = ldv<V>(dpooled + row * C + c0);
    const Vec<V> mu = ldv<V>(mean + c0), is = ldv<V>(invstd + c0);
    const long long base = (((long long)n * H + 2 * py) * W + 2 * px) * C + c0;
    Vec<V> out[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < V; ++e) out[q].v[e] = 0.f;
    unsigned codes = 0;                                   // the V routing bytes of this thread in one load when they form a dword
    if constexpr (V == 4) codes = *reinterpret_cast<const unsigned*>(idx + row * C + c0);
    // the four window pixels as whole vectors, all in flight at once (the arg-max positions of a thread's channels touch nearly every
    // 32-byte sector of the window anyway; four coalesced 16-byte loads replace four dependent, divergent 4-byte gathers)
    Vec<V> yq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) yq[q] = ldv<V>(y + base + ((long long)(q >> 1) * W + (q & 1)) * C);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int code = V == 4 ? (int)((codes >> (8 * e)) & 0xffu) : (int)idx[row * C + c0 + e];
      if (code & 4) {
        const int q = code & 3;
        const float g = dp.v[e];
        const float yv = q == 0 ? yq[0].v[e] : (q == 1 ? yq[1].v[e] : (q == 2 ? yq[2].v[e] : yq[3].v[e]));
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
          if (qq == q) out[qq].v[e] = g;
        acc[e][0] += g;
        acc[e][1] += g * (yv - mu.v[e]) * is.v[e];
      }
    }
    if (dz != nullptr) {
#pragma unroll
      for (int q = 0; q < 4; ++q) stv<V>(dz + base + ((long long)(q >> 1) * W + (q & 1)) * C, out[q]);
    }
  }
};

struct BnReluBwdOp {
  static constexpr int NACC = 2;
  int write;                      // 0: sums only (the apply pass re-derives the mask from y, dn_bn_bwd_apply_relu)
  float* da_dz;
  const float* y;
  const float* scale;
  const float* shift;
  const float* mean;
  const float* invstd;
  int C;
  template <int V>
  __device__ __forceinline__ void apply(long long row, int c0, float (&acc)[V][2]) const {
    const long long o = row * C + c0;
    Vec<V> g = ldv<V>(da_dz + o);
    const Vec<V> yv = ldv<V>(y + o), sc = ldv<V>(scale + c0), sh = ldv<V>(shift + c0), mu = ldv<V>(mean + c0), is = ldv<V>(invstd + c0);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float dz = (yv.v[e] * sc.v[e] + sh.v[e] > 0.f) ? g.v[e] : 0.f;
      g.v[e] = dz;
      acc[e][0] += dz;
      acc[e][1] += dz * (yv.v[e] - mu.v[e]) * is.v[e];
    }
    if (write) stv<V>(da_dz + o, g);
  }
};

// both BatchNorm-backward sums of a channel in one launch: out0[c] = sum_r partial[r][c][offset], out1[c] = sum_r partial[r][c][offset + 1].
// One block of 256 threads per channel (was: one wave per channel, four channels per block): at 32 images the input-gradient epilogues
// leave up to 13 312 partial rows per channel, and 16 blocks of strided 8-byte reads took 22-40 us per layer.  The rows meet in double
// precision in a fixed order (thread-strided partial sums, then a tree over the 256 threads): deterministic.
__global__ void __launch_bounds__(256) colsum2_finalize_kernel(const float* __restrict__ partial, int rows, int C, int stride, int offset,
                                                               float* __restrict__ out0, float* __restrict__ out1) {
  const int c = blockIdx.x;
  double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
  for (int r = threadIdx.x; r < rows; r += 256) {
    const float* q = partial + ((long long)r * C + c) * stride + offset;
    s0 += (double)q[0];
    s1 += (double)q[1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o);
    s1 += __shfl_xor(s1, o);
  }
  __shared__ double red[2][4];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s0;
    red[1][threadIdx.x >> 6] = s1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out0[c] = (float)((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
    out1[c] = (float)((red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
  }
}

// ---------------------------------------------------------------------------------------------- backward: the apply pass
// dy = gamma * invstd * (dz - sum(dz) / n - xhat * sum(dz * xhat) / n), written with explicit fused steps: every kernel below goes
// through this one function, so the same element gets the SAME bits whatever the compiler hoists out of a loop (the hoisted form keeps
// the per-channel factors in registers across iterations); tests/test_gpu_bn_backward.py,
// tests/test_gpu_graph.py::test_bn_backward_without_materialised_dz_is_bitwise_the_two_pass_form
__device__ __forceinline__ float bn_bwd_value(float z, float yv, float mu, float is, float ga, float dg, float db, float inv_count) {
#pragma clang fp contract(off)
  const float xhat = (yv - mu) * is;
  float t = __builtin_fmaf(-db, inv_count, z);
  t = __builtin_fmaf(-(xhat * dg), inv_count, t);
  return (ga * is) * t;
}

// RELU = false: g holds dz (ResNet bottleneck bn3 / downsample BatchNorms, whose gradient arrives as dz from bn_add_relu_bwd; scale and
// shift are null).  RELU = true: g holds da, the gradient w.r.t. relu(bn(y)), and the mask is RE-DERIVED here instead of read back from a
// materialised dz -- dz = da * (y*scale+shift > 0) --, so the reduce pass only produces the two sums (no full-size write).  g is
// overwritten with dy.  The plain loop: any C % 4 == 0.
template <bool RELU>
__global__ void __launch_bounds__(kThreads) bn_bwd_apply_kernel(float* __restrict__ g_dy, const float* __restrict__ y,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                                const float* __restrict__ dbeta, long long rows, int C, float inv_count) {
  const int G = C / 4;
  const long long total = rows * G;
  for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int c = (int)(i % G) * 4;
    const long long o = i * 4;
    f32x4 dz = *reinterpret_cast<const f32x4*>(g_dy + o);
    const f32x4 yv = *reinterpret_cast<const f32x4*>(y + o);
    f32x4 sc, sh;
    if constexpr (RELU) sc = *reinterpret_cast<const f32x4*>(scale + c), sh = *reinterpret_cast<const f32x4*>(shift + c);
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c), is = *reinterpret_cast<const f32x4*>(invstd + c);
    const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + c), dg = *reinterpret_cast<const f32x4*>(dgamma + c),
                db = *reinterpret_cast<const f32x4*>(dbeta + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float z = dz[e];
      if constexpr (RELU) z = (yv[e] * sc[e] + sh[e] > 0.f) ? z : 0.f;
      dz[e] = bn_bwd_value(z, yv[e], mu[e], is[e], ga[e], dg[e], db[e], inv_count);
    }
    *reinterpret_cast<f32x4*>(g_dy + o) = dz;
  }
}

// The same pass when the grid stride (blocks x 256 threads) is a multiple of the channel groups G = C / 4 (the launcher rounds the
// grid; every layer of the nets here, also C = 2048, where G = 512 spans two blocks): a thread's channel group is the same in every
// iteration of its grid-stride loop, so the per-channel vectors are loaded ONCE (the plain kernel re-reads them and takes a 64-bit
// remainder per element group), and four element groups are in flight per thread (round 5: the plain kernel ran at 4.0 TB/s, this one
// does 5.0-5.3).  Same arithmetic (bn_bwd_value), same bits.
template <bool RELU>
__global__ void __launch_bounds__(kThreads) bn_bwd_apply_hoisted_kernel(float* __restrict__ g_dy, const float* __restrict__ y,
                                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                                        const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                        const float* __restrict__ gamma, const float* __restrict__ dgamma,
                                                                        const float* __restrict__ dbeta, long long rows, int C, float inv_count) {
  const int G = C / 4;
  const long long total = rows * G;
  const long long first = blockIdx.x * (long long)kThreads + threadIdx.x;
  const int c = (int)(first % G) * 4;
  f32x4 sc, sh;
  if constexpr (RELU) sc = *reinterpret_cast<const f32x4*>(scale + c), sh = *reinterpret_cast<const f32x4*>(shift + c);
  const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c), is = *reinterpret_cast<const f32x4*>(invstd + c);
  const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + c), dg = *reinterpret_cast<const f32x4*>(dgamma + c),
              db = *reinterpret_cast<const f32x4*>(dbeta + c);
  const long long step = (long long)gridDim.x * kThreads;
  for (long long i0 = first; i0 < total; i0 += 4 * step) {
    f32x4 dz[4], yv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long i = i0 + u * step;
      if (i < total) {
        dz[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g_dy + i * 4));
        yv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(y + i * 4));
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long i = i0 + u * step;
      if (i < total) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float z = dz[u][e];
          if constexpr (RELU) z = (yv[u][e] * sc[e] + sh[e] > 0.f) ? z : 0.f;
          dz[u][e] = bn_bwd_value(z, yv[u][e], mu[e], is[e], ga[e], dg[e], db[e], inv_count);
        }
        *reinterpret_cast<f32x4*>(g_dy + i * 4) = dz[u];
      }
    }
  }
}

// The same BatchNorm backward with the max-pool routing expanded here: after a pool the sparse full-resolution dz never exists.
//   pool:  dz[n, 2py+a, 2px+b, c] = dpooled[n,py,px,c] if idx says (a,b) is the arg-max and the pooled value was > 0, else 0
__global__ void __launch_bounds__(kThreads) bn_bwd_apply_pool_kernel(const float* __restrict__ dpooled, const uint8_t* __restrict__ idx,
                                                                     const float* __restrict__ y, const float* __restrict__ mean,
                                                                     const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                     const float* __restrict__ dgamma, const float* __restrict__ dbeta, int N,
                                                                     int H, int W, int C, float inv_count, float* __restrict__ dy) {
  const int G = C / 4, PH = H / 2, PW = W / 2;
  const long long total = (long long)N * PH * PW * G;
  for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int g = (int)(i % G);
    long long pix = i / G;
    const int px = (int)(pix % PW);
    pix /= PW;
    const int py = (int)(pix % PH), n = (int)(pix / PH);
    const int c = g * 4;
    const f32x4 dp = *reinterpret_cast<const f32x4*>(dpooled + i * 4);
    const uchar4 code = *reinterpret_cast<const uchar4*>(idx + i * 4);
    const int cd[4] = {code.x, code.y, code.z, code.w};
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c), is = *reinterpret_cast<const f32x4*>(invstd + c);
    const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + c), dg = *reinterpret_cast<const f32x4*>(dgamma + c),
                db = *reinterpret_cast<const f32x4*>(dbeta + c);
    const long long base = (((long long)n * H + 2 * py) * W + 2 * px) * C + c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long o = base + ((long long)(q >> 1) * W + (q & 1)) * C;
      const f32x4 yv = *reinterpret_cast<const f32x4*>(y + o);
      f32x4 out;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float z = ((cd[e] & 4) && (cd[e] & 3) == q) ? dp[e] : 0.f;
        out[e] = bn_bwd_value(z, yv[e], mu[e], is[e], ga[e], dg[e], db[e], inv_count);
      }
      *reinterpret_cast<f32x4*>(dy + o) = out;
    }
  }
}

// ------------------------------------------------------------------------------------------ ResNet bottleneck tail
__global__ void __launch_bounds__(kThreads) bn_add_relu_fwd_kernel(const float* __restrict__ y, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, const float* __restrict__ r,
                                                                   const float* __restrict__ r_scale, const float* __restrict__ r_shift,
                                                                   long long rows, int C, float* __restrict__ out) {
  const int G = C / 4;
  const long long total = rows * G;
  for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int c = (int)(i % G) * 4;
    const long long o = i * 4;
    const f32x4 yv = *reinterpret_cast<const f32x4*>(y + o);
    const f32x4 rv = r != nullptr ? *reinterpret_cast<const f32x4*>(r + o) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c), sh = *reinterpret_cast<const f32x4*>(shift + c);
    f32x4 res;
    if (r_scale != nullptr) {
      const f32x4 rs = *reinterpret_cast<const f32x4*>(r_scale + c), rb = *reinterpret_cast<const f32x4*>(r_shift + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) res[e] = fmaxf(0.f, (yv[e] * sc[e] + sh[e]) + (rv[e] * rs[e] + rb[e]));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) res[e] = fmaxf(0.f, (yv[e] * sc[e] + sh[e]) + rv[e]);
    }
    *reinterpret_cast<f32x4*>(out + o) = res;
  }
}

struct AddReluBwdOp {
  static constexpr int NACC = 4;
  const float* gout;
  const float* out;
  const float* y;
  const float* mean;
  const float* invstd;
  const float* r;
  const float* r_mean;     // nullable: plain identity
  const float* r_invstd;
  float* dz_y;
  float* dr;
  int dr_accumulate;
  int C;
  template <int V>
  __device__ __forceinline__ void apply(long long row, int c0, float (&acc)[V][4]) const {
    const long long o = row * C + c0;
    const Vec<V> g = ldv<V>(gout + o), ov = ldv<V>(out + o), yv = ldv<V>(y + o), mu = ldv<V>(mean + c0), is = ldv<V>(invstd + c0);
    Vec<V> m;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      m.v[e] = ov.v[e] > 0.f ? g.v[e] : 0.f;
      acc[e][0] += m.v[e];
      acc[e][1] += m.v[e] * (yv.v[e] - mu.v[e]) * is.v[e];
    }
    stv<V>(dz_y + o, m);
    if (r_mean != nullptr) {
      const Vec<V> rv = ldv<V>(r + o), rm = ldv<V>(r_mean + c0), ri = ldv<V>(r_invstd + c0);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        acc[e][2] += m.v[e];
        acc[e][3] += m.v[e] * (rv.v[e] - rm.v[e]) * ri.v[e];
      }
      stv<V>(dr + o, m);
    } else if (dr != nullptr) {
      if (dr_accumulate) {
        Vec<V> d = ldv<V>(dr + o);
#pragma unroll
        for (int e = 0; e < V; ++e) d.v[e] += m.v[e];
        stv<V>(dr + o, d);
      } else {
        stv<V>(dr + o, m);
      }
    }
  }
};

// ------------------------------------------------------------------------------ backward of a FROZEN BatchNorm (running statistics)
// mean = running_mean, invstd = 1 / sqrt(running_var + eps) are constants of the step, so
//   dy = (gamma * invstd) * dz,   dbeta = sum dz,   dgamma = sum dz * xhat,   xhat = (y - mean) * invstd
// has no batch-mean terms: every form below is ONE full-size pass that writes dy and leaves the per-block partial rows of both sums
// (dn_colreduce.h); bn_frozen_finalize_kernel meets the rows.  All forms go through this one function (contraction off): the same
// element gets the same bits whichever form handles it (tests/test_gpu_bn_frozen.py).  Two rounded operations for dy (gamma * invstd,
// the product), three for the dgamma term (a difference, two products).
__device__ __forceinline__ float bn_frozen_bwd_value(float z, float yv, float mu, float is, float ga, float& term) {
#pragma clang fp contract(off)
  const float xhat = (yv - mu) * is;
  term = z * xhat;
  return (ga * is) * z;
}

// the pre-BatchNorm map is dead after this pass (its consumers' weight gradients ran before it): read it past the caches
template <int V>
__device__ __forceinline__ Vec<V> ldv_stream(const float* p) {
  Vec<V> r;
  if constexpr (V == 4) {
    const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[i] = t[i];
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) r.v[i] = p[i];
  }
  return r;
}

// RELU: g holds da, the gradient w.r.t. relu(bn(y)), dz = da * [y * scale + shift > 0]; else g holds dz.  g is overwritten with dy.
template <bool RELU>
struct BnFrozenBwdOp {
  static constexpr int NACC = 2;
  float* g_dy;
  const float* y;
  const float* scale;
  const float* shift;
  const float* mean;
  const float* invstd;
  const float* gamma;
  int C;
  template <int V>
  __device__ __forceinline__ void apply(long long row, int c0, float (&acc)[V][2]) const {
    const long long o = row * C + c0;
    Vec<V> g = ldv<V>(g_dy + o);
    const Vec<V> yv = ldv_stream<V>(y + o), mu = ldv<V>(mean + c0), is = ldv<V>(invstd + c0), ga = ldv<V>(gamma + c0);
    Vec<V> sc, sh;
    if constexpr (RELU) sc = ldv<V>(scale + c0), sh = ldv<V>(shift + c0);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float z = g.v[e];
      if constexpr (RELU) z = (yv.v[e] * sc.v[e] + sh.v[e] > 0.f) ? z : 0.f;
      float term;
      g.v[e] = bn_frozen_bwd_value(z, yv.v[e], mu.v[e], is.v[e], ga.v[e], term);
      acc[e][0] += z;
      acc[e][1] += term;
    }
    stv<V>(g_dy + o, g);
  }
};

// Through the fused 2x2 max-pool: one POOLED pixel per visit, its (dpooled, idx) expanded straight into the four window pixels of dy;
// the sparse dz is never written (train mode: PoolBwdOp for the sums, then bn_bwd_apply_pool_kernel).
struct BnFrozenPoolBwdOp {
  static constexpr int NACC = 2;
  const float* dpooled;
  const uint8_t* idx;
  const float* y;
  const float* mean;
  const float* invstd;
  const float* gamma;
  float* dy;
  int PH, PW, H, W, C;
  template <int V>
  __device__ __forceinline__ void apply(long long row, int c0, float (&acc)[V][2]) const {
    const int px = (int)(row % PW);
    const long long t = row / PW;
    const int py = (int)(t % PH), n = (int)(t / PH);
    const Vec<V> dp = ldv<V>(dpooled + row * C + c0);
    const Vec<V> mu = ldv<V>(mean + c0), is = ldv<V>(invstd + c0), ga = ldv<V>(gamma + c0);
    const long long base = (((long long)n * H + 2 * py) * W + 2 * px) * C + c0;
    unsigned codes = 0;
    if constexpr (V == 4) codes = *reinterpret_cast<const unsigned*>(idx + row * C + c0);
    Vec<V> yq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) yq[q] = ldv_stream<V>(y + base + ((long long)(q >> 1) * W + (q & 1)) * C);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int code = V == 4 ? (int)((codes >> (8 * e)) & 0xffu) : (int)idx[row * C + c0 + e];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float z = ((code & 4) && (code & 3) == q) ? dp.v[e] : 0.f;
        float term;
        yq[q].v[e] = bn_frozen_bwd_value(z, yq[q].v[e], mu.v[e], is.v[e], ga.v[e], term);
        acc[e][0] += z;
        acc[e][1] += term;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) stv<V>(dy + base + ((long long)(q >> 1) * W + (q & 1)) * C, yq[q]);
  }
};

// The residual tail out = relu(bn(y) + r') with both BatchNorms frozen: from d(out) the masked gradient m = d(out) * [out > 0] becomes
// dy of the main branch and, in the same pass, dr of a frozen downsample branch (r_mean given) or the plain m of an identity branch
// (overwritten or accumulated); sums of both branches (partial[blk][C][4]: main at 0, downsample at 2).
struct BnFrozenAddReluBwdOp {
  static constexpr int NACC = 4;
  const float* gout;
  const float* out;
  const float* y;
  const float* mean;
  const float* invstd;
  const float* gamma;
  const float* r;
  const float* r_mean;     // nullable: plain identity
  const float* r_invstd;
  const float* r_gamma;
  float* dy;
  float* dr;
  int dr_accumulate;
  int C;
  template <int V>
  __device__ __forceinline__ void apply(long long row, int c0, float (&acc)[V][4]) const {
    const long long o = row * C + c0;
    const Vec<V> g = ldv<V>(gout + o), ov = ldv<V>(out + o), yv = ldv_stream<V>(y + o);
    const Vec<V> mu = ldv<V>(mean + c0), is = ldv<V>(invstd + c0), ga = ldv<V>(gamma + c0);
    Vec<V> m, d;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      m.v[e] = ov.v[e] > 0.f ? g.v[e] : 0.f;
      float term;
      d.v[e] = bn_frozen_bwd_value(m.v[e], yv.v[e], mu.v[e], is.v[e], ga.v[e], term);
      acc[e][0] += m.v[e];
      acc[e][1] += term;
    }
    stv<V>(dy + o, d);
    if (r_mean != nullptr) {
      const Vec<V> rv = ldv_stream<V>(r + o), rm = ldv<V>(r_mean + c0), ri = ldv<V>(r_invstd + c0), rg = ldv<V>(r_gamma + c0);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        float term;
        d.v[e] = bn_frozen_bwd_value(m.v[e], rv.v[e], rm.v[e], ri.v[e], rg.v[e], term);
        acc[e][2] += m.v[e];
        acc[e][3] += term;
      }
      stv<V>(dr + o, d);
    } else if (dr != nullptr) {
      if (dr_accumulate) {
        Vec<V> a = ldv<V>(dr + o);
#pragma unroll
        for (int e = 0; e < V; ++e) a.v[e] += m.v[e];
        stv<V>(dr + o, a);
      } else {
        stv<V>(dr + o, m);
      }
    }
  }
};

// The partial rows of a frozen pass become dbeta[c] = sum_r partial[r][c][offset], dgamma[c] = sum_r partial[r][c][offset + 1] and,
// when asked for, the gradient of a conv bias in front of the BatchNorm: with frozen statistics it is no longer identically zero,
//   dbias[c] = sum dy = (gamma[c] * invstd[c]) * dbeta[c]      (two fp32 products on the ROUNDED dbeta, contraction off),
// at no extra pass.  The rows meet in double precision in a fixed order: the sliced order of dn_fold.h for up to kFoldMaxRows rows
// (one block per 64 channels), else colsum2_finalize_kernel's (one block per channel).
__device__ __forceinline__ float bn_frozen_dbias(float ga, float is, float db) {
#pragma clang fp contract(off)
  return (ga * is) * db;
}

__global__ void __launch_bounds__(256) bn_frozen_finalize_sliced_kernel(const float* __restrict__ partial, int rows, int C, int stride, int offset,
                                                                        const float* __restrict__ gamma, const float* __restrict__ invstd,
                                                                        float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                        float* __restrict__ dbias) {
  __shared__ double red[2 * kFoldSlices * 64];
  const int c0 = blockIdx.x * 64;
  const int nlive = C - c0 < 64 ? C - c0 : 64;
  colsum2_sliced<false>(partial, rows, C, stride, offset, c0, nlive, dbeta, dgamma, red, threadIdx.x);
  // (thread (channel, slice 0) wrote dbeta[c] itself: program order, no barrier)
  const int cl = threadIdx.x & 63;
  if (dbias != nullptr && (threadIdx.x >> 6) == 0 && cl < nlive) dbias[c0 + cl] = bn_frozen_dbias(gamma[c0 + cl], invstd[c0 + cl], dbeta[c0 + cl]);
}

__global__ void __launch_bounds__(256) bn_frozen_finalize_kernel(const float* __restrict__ partial, int rows, int C, int stride, int offset,
                                                                 const float* __restrict__ gamma, const float* __restrict__ invstd,
                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dbias) {
  const int c = blockIdx.x;
  double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
  for (int r = threadIdx.x; r < rows; r += 256) {
    const float* q = partial + ((long long)r * C + c) * stride + offset;
    s0 += (double)q[0];
    s1 += (double)q[1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o);
    s1 += __shfl_xor(s1, o);
  }
  __shared__ double red[2][4];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s0;
    red[1][threadIdx.x >> 6] = s1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float db = (float)((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]));
    dbeta[c] = db;
    dgamma[c] = (float)((red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
    if (dbias != nullptr) dbias[c] = bn_frozen_dbias(gamma[c], invstd[c], db);
  }
}

// The apply pass of both entry points below.  Hoisted form: a grid whose stride (blocks x 256 threads) is a multiple of the channel
// groups G = C / 4 -- per = lcm(G, 256) / 256 = G / gcd(G, 256) blocks span a whole number of pixels, and the grid is rounded up to a
// multiple of per --, unless that takes more than 64 blocks: then the plain loop.
template <bool RELU>
static int launch_bn_bwd_apply(float* g_dy, const float* y, const float* scale, const float* shift, const float* mean, const float* invstd,
                               const float* gamma, const float* dgamma, const float* dbeta, int64_t rows, int32_t C, hipStream_t s,
                               const char* what) {
  const int G = C / 4;
  int blocks = ew_blocks((rows * (long long)G + 3) / 4);
  int ga = G, gb = kThreads;
  while (gb != 0) {
    const int t = ga % gb;
    ga = gb;
    gb = t;
  }
  const int per = G / ga;
  if (per <= 64) {
    blocks = (blocks + per - 1) / per * per;
    set_last_kernel(RELU ? "dn::bn_bwd_apply_hoisted_kernel<true>" : "dn::bn_bwd_apply_hoisted_kernel<false>");
    DN_LAUNCH(bn_bwd_apply_hoisted_kernel<RELU>, dim3(blocks), dim3(kThreads), 0, s, g_dy, y, scale, shift, mean, invstd, gamma, dgamma, dbeta,
              (long long)rows, C, (float)(1.0 / (double)rows));
  } else {
    set_last_kernel(RELU ? "dn::bn_bwd_apply_kernel<true>" : "dn::bn_bwd_apply_kernel<false>");
    DN_LAUNCH(bn_bwd_apply_kernel<RELU>, dim3(ew_blocks(rows * (C / 4))), dim3(kThreads), 0, s, g_dy, y, scale, shift, mean, invstd, gamma, dgamma,
              dbeta, (long long)rows, C, (float)(1.0 / (double)rows));
  }
  return check_launch(what);
}

}  // namespace dn

using namespace dn;

extern "C" {

int dn_bn_finalize(const float* partial, int32_t rows, int32_t C, int64_t count, const float* conv_bias, const float* gamma,
                   const float* beta, float* running_mean, float* running_var, float momentum, float eps, float* mean, float* invstd,
                   float* scale, float* shift, int64_t* num_batches_tracked, dn_stream_t stream) {
  DN_REQUIRE(partial && gamma && beta && mean && invstd && scale && shift && rows > 0 && C > 0 && count > 0, DN_ERR_BAD_ARG,
             "dn_bn_finalize: bad argument");
  if (rows <= kFoldMaxRows) {          // the order a folded finalize uses (dn_conv_desc.bnf_*): bit-identical results either way
    const BnFinalizeArgs a{conv_bias, gamma, beta, running_mean, running_var, reinterpret_cast<long long*>(num_batches_tracked), momentum, eps,
                           mean, invstd, scale, shift};
    DN_LAUNCH(bn_finalize_sliced_kernel, dim3((C + 63) / 64), dim3(256), 0, as_stream(stream), partial, rows, C, (double)count, a);
    return check_launch("bn_finalize_sliced_kernel");
  }
  DN_LAUNCH(bn_finalize_kernel, dim3(C), dim3(kThreads), 0, as_stream(stream), partial, rows, C, (double)count, conv_bias, gamma,
                     beta, running_mean, running_var, momentum, eps, mean, invstd, scale, shift,
                     reinterpret_cast<long long*>(num_batches_tracked));
  return check_launch("bn_finalize_kernel");
}

int dn_bn_eval_affine(int32_t C, const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                      float* scale, float* shift, dn_stream_t stream) {
  DN_REQUIRE(C > 0 && gamma && beta && running_mean && running_var && scale && shift, DN_ERR_BAD_ARG, "dn_bn_eval_affine: bad argument");
  DN_LAUNCH(bn_eval_affine_kernel, dim3((C + 255) / 256), dim3(256), 0, as_stream(stream), C, gamma, beta, running_mean,
                     running_var, eps, scale, shift, (float*)nullptr);
  return check_launch("bn_eval_affine_kernel");
}

int dn_bn_frozen_affine(int32_t C, const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                        float* scale, float* shift, float* invstd, dn_stream_t stream) {
  DN_REQUIRE(C > 0 && gamma && beta && running_mean && running_var && scale && shift && invstd, DN_ERR_BAD_ARG,
             "dn_bn_frozen_affine: bad argument");
  DN_LAUNCH(bn_eval_affine_kernel, dim3((C + 255) / 256), dim3(256), 0, as_stream(stream), C, gamma, beta, running_mean,
                     running_var, eps, scale, shift, invstd);
  return check_launch("bn_eval_affine_kernel");
}

int dn_bn_frozen_bwd(float* dz_dy, const float* y, const float* mean, const float* invstd, const float* gamma, int64_t rows, int32_t C,
                     float* partial, dn_stream_t stream) {
  DN_REQUIRE(dz_dy && y && mean && invstd && gamma && partial && rows > 0 && C > 0, DN_ERR_BAD_ARG, "dn_bn_frozen_bwd: bad argument");
  DN_REQUIRE(C % 4 == 0, DN_ERR_UNSUPPORTED, "dn_bn_frozen_bwd: need C%%4==0");
  BnFrozenBwdOp<false> op{dz_dy, y, nullptr, nullptr, mean, invstd, gamma, C};
  return launch_colreduce(op, rows, C, partial, as_stream(stream), "bn_frozen_bwd");
}

int dn_bn_frozen_bwd_relu(float* da_dy, const float* y, const float* scale, const float* shift, const float* mean, const float* invstd,
                          const float* gamma, int64_t rows, int32_t C, float* partial, dn_stream_t stream) {
  DN_REQUIRE(da_dy && y && scale && shift && mean && invstd && gamma && partial && rows > 0 && C > 0, DN_ERR_BAD_ARG,
             "dn_bn_frozen_bwd_relu: bad argument");
  DN_REQUIRE(C % 4 == 0, DN_ERR_UNSUPPORTED, "dn_bn_frozen_bwd_relu: need C%%4==0");
  BnFrozenBwdOp<true> op{da_dy, y, scale, shift, mean, invstd, gamma, C};
  return launch_colreduce(op, rows, C, partial, as_stream(stream), "bn_frozen_bwd_relu");
}

int dn_bn_frozen_bwd_pool(const float* dpooled, const uint8_t* idx, const float* y, const float* mean, const float* invstd, const float* gamma,
                          int32_t N, int32_t H, int32_t W, int32_t C, float* dy, float* partial, dn_stream_t stream) {
  DN_REQUIRE(dpooled && idx && y && mean && invstd && gamma && dy && partial && N > 0 && H > 0 && W > 0 && C > 0, DN_ERR_BAD_ARG,
             "dn_bn_frozen_bwd_pool: bad argument");
  DN_REQUIRE(C % 4 == 0 && H % 2 == 0 && W % 2 == 0, DN_ERR_UNSUPPORTED, "dn_bn_frozen_bwd_pool: need C%%4==0 and even H,W");
  BnFrozenPoolBwdOp op{dpooled, idx, y, mean, invstd, gamma, dy, H / 2, W / 2, H, W, C};
  return launch_colreduce(op, (long long)N * (H / 2) * (W / 2), C, partial, as_stream(stream), "bn_frozen_bwd_pool");
}

int dn_bn_frozen_add_relu_bwd(const float* gout, const float* out, const float* y, const float* mean, const float* invstd, const float* gamma,
                              const float* r, const float* r_mean, const float* r_invstd, const float* r_gamma, int64_t rows, int32_t C,
                              float* dy, float* dr, int32_t dr_accumulate, float* partial, dn_stream_t stream) {
  DN_REQUIRE(gout && out && y && mean && invstd && gamma && dy && partial && rows > 0 && C > 0, DN_ERR_BAD_ARG,
             "dn_bn_frozen_add_relu_bwd: bad argument");
  DN_REQUIRE(C % 4 == 0, DN_ERR_UNSUPPORTED, "dn_bn_frozen_add_relu_bwd: need C%%4==0");
  DN_REQUIRE((r_mean == nullptr) == (r_invstd == nullptr) && (r_mean == nullptr) == (r_gamma == nullptr), DN_ERR_BAD_ARG,
             "dn_bn_frozen_add_relu_bwd: r_mean / r_invstd / r_gamma go together");
  DN_REQUIRE(r_mean == nullptr || (r && dr), DN_ERR_BAD_ARG, "dn_bn_frozen_add_relu_bwd: the downsample branch needs r and dr");
  BnFrozenAddReluBwdOp op{gout, out, y, mean, invstd, gamma, r, r_mean, r_invstd, r_gamma, dy, dr, dr_accumulate, C};
  return launch_colreduce(op, rows, C, partial, as_stream(stream), "bn_frozen_add_relu_bwd");
}

int dn_bn_frozen_finalize(const float* partial, int32_t partial_rows, int32_t partial_stride, int32_t partial_offset, int32_t C,
                          const float* gamma, const float* invstd, float* dgamma, float* dbeta, float* dbias, dn_stream_t stream) {
  DN_REQUIRE(partial && dgamma && dbeta && partial_rows > 0 && C > 0, DN_ERR_BAD_ARG, "dn_bn_frozen_finalize: bad argument");
  DN_REQUIRE(dbias == nullptr || (gamma && invstd), DN_ERR_BAD_ARG, "dn_bn_frozen_finalize: the bias gradient needs gamma and invstd");
  DN_REQUIRE(partial_stride >= 2 && partial_offset >= 0 && partial_offset + 1 < partial_stride, DN_ERR_BAD_ARG,
             "dn_bn_frozen_finalize: partial layout");
  hipStream_t s = as_stream(stream);
  if (partial_rows <= kFoldMaxRows && (partial_stride & 1) == 0 && (partial_offset & 1) == 0 && (reinterpret_cast<uintptr_t>(partial) & 7) == 0)
    DN_LAUNCH(bn_frozen_finalize_sliced_kernel, dim3((C + 63) / 64), dim3(256), 0, s, partial, partial_rows, C, partial_stride, partial_offset, gamma,
              invstd, dgamma, dbeta, dbias);
  else
    DN_LAUNCH(bn_frozen_finalize_kernel, dim3(C), dim3(256), 0, s, partial, partial_rows, C, partial_stride, partial_offset, gamma, invstd, dgamma,
              dbeta, dbias);
  return check_launch("bn_frozen_finalize");
}

int32_t dn_bn_stats_rows(int64_t rows) { return (int32_t)((rows + kBnTileRows - 1) / kBnTileRows); }

int dn_bn_stats_partial(const float* x, int64_t rows, int32_t C, float* partial, dn_stream_t stream) {
  DN_REQUIRE(x && partial && rows > 0 && C > 0, DN_ERR_BAD_ARG, "dn_bn_stats_partial: bad argument");
  DN_REQUIRE((rows + kBnTileRows - 1) / kBnTileRows < 65536ll * 32768ll, DN_ERR_UNSUPPORTED, "dn_bn_stats_partial: too many rows");
  DN_LAUNCH(bn_stats_partial_kernel, dim3((unsigned)((rows + kBnTileRows - 1) / kBnTileRows), (C + 63) / 64), dim3(kThreads), 0, as_stream(stream), x,
                     (long long)rows, C, partial);
  return check_launch("bn_stats_partial_kernel");
}

int dn_bn_apply_fwd(const float* y, const float* scale, const float* shift, int64_t rows, int32_t C, float* out, dn_stream_t stream) {
  DN_REQUIRE(y && scale && shift && out && rows > 0 && C > 0, DN_ERR_BAD_ARG, "dn_bn_apply_fwd: bad argument");
  DN_REQUIRE(C % 4 == 0, DN_ERR_UNSUPPORTED, "dn_bn_apply_fwd: need C%%4==0");
  DN_LAUNCH(bn_apply_kernel, dim3(ew_blocks(rows * (C / 4))), dim3(kThreads), 0, as_stream(stream), y, scale, shift, (long long)rows, C, out);
  return check_launch("bn_apply_kernel");
}

int dn_bn_relu_pool_fwd(const float* y, const float* scale, const float* shift, int32_t N, int32_t H, int32_t W, int32_t C, float* pooled,
                        uint8_t* idx, dn_stream_t stream) {
  DN_REQUIRE(y && pooled && idx && ((scale == nullptr) == (shift == nullptr)), DN_ERR_BAD_ARG, "dn_bn_relu_pool_fwd: null pointer");
  DN_REQUIRE(C % 4 == 0 && H % 2 == 0 && W % 2 == 0 && N > 0, DN_ERR_UNSUPPORTED, "dn_bn_relu_pool_fwd: need C%%4==0 and even H,W");
  const long long total = (long long)N * (H / 2) * (W / 2) * (C / 4);
  DN_LAUNCH(bn_relu_pool_fwd_kernel, dim3(ew_blocks(total)), dim3(kThreads), 0, as_stream(stream), y, scale, shift, N, H, W, C,
                     pooled, idx);
  return check_launch("bn_relu_pool_fwd_kernel");
}

int dn_bn_relu_pool_bwd(const float* dpooled, const uint8_t* idx, const float* y, const float* mean, const float* invstd, int32_t N,
                        int32_t H, int32_t W, int32_t C, float* dz, float* partial, dn_stream_t stream) {
  DN_REQUIRE(dpooled && idx && y && mean && invstd && dz && partial, DN_ERR_BAD_ARG, "dn_bn_relu_pool_bwd: null pointer");
  DN_REQUIRE(C % 4 == 0 && H % 2 == 0 && W % 2 == 0, DN_ERR_UNSUPPORTED, "dn_bn_relu_pool_bwd: need C%%4==0 and even H,W");
  PoolBwdOp op{dpooled, idx, y, mean, invstd, dz, H / 2, W / 2, H, W, C};
  return launch_colreduce(op, (long long)N * (H / 2) * (W / 2), C, partial, as_stream(stream), "bn_relu_pool_bwd");
}

int dn_bn_relu_pool_bwd_sums(const float* dpooled, const uint8_t* idx, const float* y, const float* mean, const float* invstd, int32_t N,
                             int32_t H, int32_t W, int32_t C, float* partial, dn_stream_t stream) {
  DN_REQUIRE(dpooled && idx && y && mean && invstd && partial, DN_ERR_BAD_ARG, "dn_bn_relu_pool_bwd_sums: null pointer");
  DN_REQUIRE(C % 4 == 0 && H % 2 == 0 && W % 2 == 0, DN_ERR_UNSUPPORTED, "dn_bn_relu_pool_bwd_sums: need C%%4==0 and even H,W");
  PoolBwdOp op{dpooled, idx, y, mean, invstd, nullptr, H / 2, W / 2, H, W, C};
  return launch_colreduce(op, (long long)N * (H / 2) * (W / 2), C, partial, as_stream(stream), "bn_relu_pool_bwd_sums");
}

int dn_bn_relu_bwd_reduce(float* da_dz, const float* y, const float* scale, const float* shift, const float* mean, const float* invstd,
                          int64_t rows, int32_t C, float* partial, dn_stream_t stream) {
  DN_REQUIRE(da_dz && y && scale && shift && mean && invstd && partial && rows > 0 && C > 0, DN_ERR_BAD_ARG,
             "dn_bn_relu_bwd_reduce: bad argument");
  BnReluBwdOp op{1, da_dz, y, scale, shift, mean, invstd, C};
  return launch_colreduce(op, rows, C, partial, as_stream(stream), "bn_relu_bwd_reduce");
}

int dn_bn_relu_bwd_sums(const float* da, const float* y, const float* scale, const float* shift, const float* mean, const float* invstd,
                        int64_t rows, int32_t C, float* partial, dn_stream_t stream) {
  DN_REQUIRE(da && y && scale && shift && mean && invstd && partial && rows > 0 && C > 0, DN_ERR_BAD_ARG, "dn_bn_relu_bwd_sums: bad argument");
  BnReluBwdOp op{0, const_cast<float*>(da), y, scale, shift, mean, invstd, C};
  return launch_colreduce(op, rows, C, partial, as_stream(stream), "bn_relu_bwd_sums");
}

static void launch_colsum2(const float* partial, int32_t partial_rows, int32_t C, int32_t partial_stride, int32_t partial_offset, float* out0,
                           float* out1, hipStream_t s) {
  // few rows: the sliced order a folded sum uses (dn_conv_desc.bnb_dgamma / bnb_dbeta) -- bit-identical either way
  if (partial_rows <= kFoldMaxRows && (partial_stride & 1) == 0 && (partial_offset & 1) == 0 && (reinterpret_cast<uintptr_t>(partial) & 7) == 0)
    DN_LAUNCH(colsum2_sliced_kernel, dim3((C + 63) / 64), dim3(256), 0, s, partial, partial_rows, C, partial_stride, partial_offset, out0, out1);
  else
    DN_LAUNCH(colsum2_finalize_kernel, dim3(C), dim3(256), 0, s, partial, partial_rows, C, partial_stride, partial_offset, out0, out1);
}

// partial == nullptr: dgamma / dbeta already hold the two sums (the input-gradient launch that produced the partial rows finished them
// itself: dn_conv_desc.bnb_dgamma / bnb_dbeta, dn_conv_dgrad_folds_bn_sums)
static int bn_bwd_sums_to_params(const float* partial, int32_t partial_rows, int32_t partial_stride, int32_t partial_offset, int32_t C,
                                 float* dgamma, float* dbeta, hipStream_t s, const char* who) {
  DN_REQUIRE(dgamma && dbeta, DN_ERR_BAD_ARG, "%s: bad argument", who);
  DN_REQUIRE(C % 4 == 0, DN_ERR_UNSUPPORTED, "%s: need C%%4==0", who);
  if (partial == nullptr) return DN_OK;
  DN_REQUIRE(partial_rows > 0, DN_ERR_BAD_ARG, "%s: bad argument", who);
  DN_REQUIRE(partial_stride >= 2 && partial_offset >= 0 && partial_offset + 1 < partial_stride, DN_ERR_BAD_ARG, "%s: partial layout", who);
  launch_colsum2(partial, partial_rows, C, partial_stride, partial_offset, dbeta, dgamma, s);
  return DN_OK;
}

int dn_bn_bwd_apply_relu(float* da_dy, const float* y, const float* scale, const float* shift, const float* mean, const float* invstd,
                         const float* gamma, const float* partial, int32_t partial_rows, int32_t partial_stride, int32_t partial_offset,
                         int64_t rows, int32_t C, float* dgamma, float* dbeta, dn_stream_t stream) {
  DN_REQUIRE(da_dy && y && scale && shift && mean && invstd && gamma && rows > 0, DN_ERR_BAD_ARG, "dn_bn_bwd_apply_relu: bad argument");
  hipStream_t s = as_stream(stream);
  int rc = bn_bwd_sums_to_params(partial, partial_rows, partial_stride, partial_offset, C, dgamma, dbeta, s, "dn_bn_bwd_apply_relu");
  if (rc != DN_OK) return rc;
  return launch_bn_bwd_apply<true>(da_dy, y, scale, shift, mean, invstd, gamma, dgamma, dbeta, rows, C, s, "bn_bwd_apply_relu");
}

int dn_bn_bwd_apply_pool(const float* dpooled, const uint8_t* idx, const float* y, const float* mean, const float* invstd, const float* gamma,
                         const float* partial, int32_t partial_rows, int32_t partial_stride, int32_t partial_offset, int32_t N, int32_t H,
                         int32_t W, int32_t C, float* dy, float* dgamma, float* dbeta, dn_stream_t stream) {
  DN_REQUIRE(dpooled && idx && y && mean && invstd && gamma && dy && N > 0, DN_ERR_BAD_ARG, "dn_bn_bwd_apply_pool: bad argument");
  DN_REQUIRE(H % 2 == 0 && W % 2 == 0, DN_ERR_UNSUPPORTED, "dn_bn_bwd_apply_pool: need even H, W");
  hipStream_t s = as_stream(stream);
  int rc = bn_bwd_sums_to_params(partial, partial_rows, partial_stride, partial_offset, C, dgamma, dbeta, s, "dn_bn_bwd_apply_pool");
  if (rc != DN_OK) return rc;
  const long long total = (long long)N * (H / 2) * (W / 2) * (C / 4);
  DN_LAUNCH(bn_bwd_apply_pool_kernel, dim3(ew_blocks(total)), dim3(kThreads), 0, s, dpooled, idx, y, mean, invstd, gamma, dgamma, dbeta, N,
                     H, W, C, (float)(1.0 / ((double)N * H * W)), dy);
  return check_launch("bn_bwd_apply_pool");
}

int dn_bn_bwd_apply(float* dz_dy, const float* y, const float* mean, const float* invstd, const float* gamma, const float* partial,
                    int32_t partial_rows, int32_t partial_stride, int32_t partial_offset, int64_t rows, int32_t C, float* dgamma,
                    float* dbeta, dn_stream_t stream) {
  DN_REQUIRE(dz_dy && y && mean && invstd && gamma && partial && dgamma && dbeta && rows > 0, DN_ERR_BAD_ARG, "dn_bn_bwd_apply: bad argument");
  DN_REQUIRE(C % 4 == 0, DN_ERR_UNSUPPORTED, "dn_bn_bwd_apply: need C%%4==0");
  DN_REQUIRE(partial_stride >= 2 && partial_offset >= 0 && partial_offset + 1 < partial_stride, DN_ERR_BAD_ARG, "dn_bn_bwd_apply: partial layout");
  hipStream_t s = as_stream(stream);
  launch_colsum2(partial, partial_rows, C, partial_stride, partial_offset, dbeta, dgamma, s);
  return launch_bn_bwd_apply<false>(dz_dy, y, nullptr, nullptr, mean, invstd, gamma, dgamma, dbeta, rows, C, s, "bn_bwd_apply");
}

int dn_bn_add_relu_fwd(const float* y, const float* scale, const float* shift, const float* r, const float* r_scale, const float* r_shift,
                       int64_t rows, int32_t C, float* out, dn_stream_t stream) {
  DN_REQUIRE(y && scale && shift && out && rows > 0 && C > 0 && ((r_scale == nullptr) == (r_shift == nullptr)) && (r || !r_scale),
             DN_ERR_BAD_ARG, "dn_bn_add_relu_fwd: bad argument");
  DN_REQUIRE(C % 4 == 0, DN_ERR_UNSUPPORTED, "dn_bn_add_relu_fwd: need C%%4==0");
  DN_LAUNCH(bn_add_relu_fwd_kernel, dim3(ew_blocks(rows * (C / 4))), dim3(kThreads), 0, as_stream(stream), y, scale, shift, r, r_scale,
                     r_shift, (long long)rows, C, out);
  return check_launch("bn_add_relu_fwd_kernel");
}

int dn_bn_add_relu_bwd(const float* gout, const float* out, const float* y, const float* mean, const float* invstd, const float* r,
                       const float* r_mean, const float* r_invstd, int64_t rows, int32_t C, float* dz_y, float* dr, int32_t dr_accumulate,
                       float* partial, dn_stream_t stream) {
  DN_REQUIRE(gout && out && y && mean && invstd && dz_y && partial && rows > 0 && C > 0, DN_ERR_BAD_ARG, "dn_bn_add_relu_bwd: bad argument");
  DN_REQUIRE((r_mean == nullptr) == (r_invstd == nullptr), DN_ERR_BAD_ARG, "dn_bn_add_relu_bwd: r_mean / r_invstd go together");
  DN_REQUIRE(r_mean == nullptr || (r && dr), DN_ERR_BAD_ARG, "dn_bn_add_relu_bwd: the downsample branch needs r and dr");
  AddReluBwdOp op{gout, out, y, mean, invstd, r, r_mean, r_invstd, dz_y, dr, dr_accumulate, C};
  return launch_colreduce(op, rows, C, partial, as_stream(stream), "bn_add_relu_bwd");
}

}  // extern "C"
